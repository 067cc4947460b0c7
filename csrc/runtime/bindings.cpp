// pybind11 bindings of the native serving runtime (pilottai_amd/_runtime.so).
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "grammar.h"
#include "scheduler.h"
#include "shm_ring.h"
#include "tokenizer.h"

namespace py = pybind11;
using namespace rt;

namespace {

std::unique_ptr<Grammar> make_grammar(const py::object& segs) {
  if (segs.is_none()) return nullptr;
  std::vector<Segment> out;
  for (const auto& item : segs) {
    py::tuple t = item.cast<py::tuple>();
    Segment s;
    s.kind = t[0].cast<int32_t>();
    s.tokens = t[1].cast<std::vector<int32_t>>();
    s.cls = t[2].cast<int32_t>();
    s.cls_last = t[3].cast<int32_t>();
    s.end_tok = t[4].cast<int32_t>();
    s.sep_tok = t[5].cast<int32_t>();
    s.max_tokens = t[6].cast<int32_t>();
    s.min_items = t[7].cast<int32_t>();
    s.max_items = t[8].cast<int32_t>();
    out.push_back(std::move(s));
  }
  return std::make_unique<Grammar>(std::move(out));
}

py::list outputs_to_py(const std::vector<SeqOutput>& outs) {
  py::list l;
  for (const auto& o : outs) {
    // last element: None, or per generated token (logprob, [(token id, logprob) x <= n])
    py::object lps = py::none();
    if (o.logprobs >= 0) {
      py::list recs;
      for (const LogprobRecord& r : o.lp_records) {
        py::list top;
        for (int32_t i = 0; i < o.logprobs && i < LOGPROB_TOP && r.ids[i] >= 0; ++i)
          top.append(py::make_tuple(r.ids[i], (double)r.lps[i]));
        recs.append(py::make_tuple((double)r.lp, top));
      }
      lps = recs;
    }
    // ... of a scoring request (it generates nothing, so it has no such records): per scored
    // prompt token (logprob, rank, [(token id, logprob) x <= n])
    if (o.score_from >= 0) {
      py::list recs;
      for (const ScoreRecord& r : o.score_records) {
        py::list top;
        for (int32_t i = 0; i < o.score_n && i < LOGPROB_TOP && r.ids[i] >= 0; ++i)
          top.append(py::make_tuple(r.ids[i], (double)r.lps[i]));
        recs.append(py::make_tuple((double)r.lp, r.rank, top));
      }
      lps = recs;
    }
    l.append(py::make_tuple(o.id, o.tokens, o.finish_reason, o.prompt_len, o.cached_prompt_tokens,
                            o.num_sampled, o.num_forced, o.t_first_token, o.t_finish, o.embed_slot, lps));
  }
  return l;
}

}  // namespace

PYBIND11_MODULE(_runtime, m) {
  m.doc() = "pilottai_amd native serving runtime (scheduler, paged KV, grammar, tokenizer)";
  m.def("now", &now_seconds);
  m.def("hash_block", [](uint64_t parent, const std::vector<int32_t>& toks) {
    return hash_block(parent, toks.data(), (int)toks.size());
  });

  py::class_<ShmRing>(m, "ShmRing")
      .def(py::init<const std::string&, int, int, int, bool, double>(), py::arg("name"), py::arg("ints"),
           py::arg("slots"), py::arg("consumers"), py::arg("create"), py::arg("attach_timeout_s") = 60.0)
      .def("put", [](ShmRing& r, const std::vector<int64_t>& rec, double timeout_s) {
             if ((int)rec.size() != r.ints()) throw std::invalid_argument("record length mismatch");
             bool ok;
             {
               py::gil_scoped_release nogil;
               ok = r.put(rec.data(), timeout_s);
             }
             return ok;
           }, py::arg("rec"), py::arg("timeout_s") = 600.0)
      .def("get", [](ShmRing& r, int c, double timeout_s) -> py::object {
             std::vector<int64_t> rec(r.ints());
             bool ok;
             {
               py::gil_scoped_release nogil;
               ok = r.get(c, rec.data(), timeout_s);
             }
             if (!ok) return py::none();
             return py::cast(rec);
           }, py::arg("consumer"), py::arg("timeout_s") = 600.0)
      .def("published", &ShmRing::published)
      .def("unlink", &ShmRing::unlink);

  py::class_<ShmGather>(m, "ShmGather")
      .def(py::init<const std::string&, int, int, size_t, bool, double>(), py::arg("name"), py::arg("world"),
           py::arg("rank"), py::arg("slot_bytes"), py::arg("create"), py::arg("attach_timeout_s") = 60.0)
      // payload: bytes (<= slot_bytes) -> list of `world` bytes (rank order), or None on timeout
      // offset / length: return only bytes [offset, offset + length) of each peer's payload
      // (an all-to-all when every rank's payload is the concatenation of per-destination chunks)
      .def("all_gather", [](ShmGather& g, const py::bytes& payload, double timeout_s, int64_t offset,
                            int64_t length) -> py::object {
             char* buf = nullptr;
             Py_ssize_t n = 0;
             if (PyBytes_AsStringAndSize(payload.ptr(), &buf, &n) != 0) throw py::error_already_set();
             if ((size_t)n > g.slot_bytes()) throw std::length_error("ShmGather payload larger than the slot");
             bool ok;
             {
               py::gil_scoped_release nogil;
               ok = g.publish(buf, (size_t)n, timeout_s);
             }
             if (!ok) return py::none();
             py::list res;
             for (int q = 0; q < g.world(); ++q) {
               const int64_t m = g.peer_size(q);
               const int64_t a = std::min<int64_t>(std::max<int64_t>(offset, 0), m);
               const int64_t e = length < 0 ? m : std::min<int64_t>(m, a + length);
               res.append(py::bytes(g.peer(q) + a, (size_t)(e - a)));
             }
             g.finish();
             return res;
           }, py::arg("payload"), py::arg("timeout_s") = 600.0, py::arg("offset") = 0, py::arg("length") = -1)
      .def_property_readonly("slot_bytes", &ShmGather::slot_bytes)
      .def_property_readonly("waited_s", &ShmGather::waited_s)
      .def("unlink", &ShmGather::unlink);

  py::class_<Tokenizer>(m, "Tokenizer")
      .def(py::init([](const std::vector<py::bytes>& vocab) {
        std::vector<std::string> v;
        v.reserve(vocab.size());
        for (const auto& b : vocab) v.push_back(b);
        return std::make_unique<Tokenizer>(v);
      }))
      .def("encode", [](const Tokenizer& t, const py::object& text) {
        std::string s = py::isinstance<py::bytes>(text) ? text.cast<std::string>()
                                                          : text.cast<std::string>();
        py::gil_scoped_release nogil;
        return t.encode(s);
      })
      .def("decode", [](const Tokenizer& t, const std::vector<int32_t>& ids) {
        return py::bytes(t.decode(ids));
      })
      .def("lookup", [](const Tokenizer& t, const py::bytes& p) { return t.lookup(p); })
      .def_property_readonly("vocab_size", &Tokenizer::vocab_size);

  py::class_<Grammar>(m, "Grammar")
      .def(py::init([](const py::object& segs) { return make_grammar(segs); }))
      .def("done", &Grammar::done)
      .def("next", [](const Grammar& g) {
        int32_t c, f;
        g.next(&c, &f);
        return py::make_tuple(c, f);
      })
      .def("advance", &Grammar::advance)
      .def("take_forced_run", [](Grammar& g, int32_t max) {
        std::vector<int32_t> out;
        g.take_forced_run(out, max);
        return out;
      });

  py::class_<BlockManager>(m, "BlockManager")
      .def(py::init<int32_t, int32_t, bool, int32_t>(), py::arg("num_blocks"), py::arg("block_size") = 16,
           py::arg("prefix_caching") = true, py::arg("host_slots") = 0)
      .def("allocate", [](BlockManager& bm, int32_t n) -> py::object {
        std::vector<int32_t> out;
        if (!bm.allocate(n, out)) return py::none();
        return py::cast(out);
      })
      .def("release", &BlockManager::release)
      .def("add_ref", &BlockManager::add_ref)
      .def("ref_count", [](const BlockManager& bm, int32_t b) {
        if (b < 0 || b >= bm.num_blocks()) throw std::out_of_range("block id");
        return bm.ref_count(b);
      })
      .def("lookup", [](BlockManager& bm, uint64_t hash, const std::vector<int32_t>& toks) {
        if ((int32_t)toks.size() != bm.block_size()) throw std::invalid_argument("lookup takes one block of tokens");
        return bm.lookup(hash, toks.data());
      })
      .def("register_block", [](BlockManager& bm, int32_t b, uint64_t hash, const std::vector<int32_t>& toks,
                                uint64_t parent) {
        if (b < 0 || b >= bm.num_blocks()) throw std::out_of_range("block id");
        if ((int32_t)toks.size() != bm.block_size()) throw std::invalid_argument("register_block takes one block of tokens");
        bm.register_block(b, hash, toks.data(), parent);
      }, py::arg("block"), py::arg("hash"), py::arg("tokens"), py::arg("parent") = 0)
      .def("register_partial", [](BlockManager& bm, int32_t b, uint64_t parent, const std::vector<int32_t>& toks) {
        bm.register_partial(b, parent, toks.data(), (int32_t)toks.size());
      }, py::arg("block"), py::arg("parent"), py::arg("tokens"))
      // -> (donor block with a reference taken, common head j), or (-1, 0)
      .def("match_head", [](BlockManager& bm, uint64_t parent, const std::vector<int32_t>& toks, int32_t max_j,
                            int32_t min_j) {
        int32_t j = 0;
        const int32_t d = bm.match_head(parent, toks.data(), (int32_t)toks.size(), max_j, min_j, &j);
        return py::make_tuple(d, j);
      }, py::arg("parent"), py::arg("tokens"), py::arg("max_j") = 16, py::arg("min_j") = 1)
      .def_property_readonly("num_free", &BlockManager::num_free)
      .def_property_readonly("num_cached", &BlockManager::num_cached)
      .def_property_readonly("num_donors", &BlockManager::num_donors)
      // host tier: slot holding the block (-1: none), no side effects
      .def("host_peek", [](const BlockManager& bm, uint64_t hash, const std::vector<int32_t>& toks) {
        if ((int32_t)toks.size() != bm.block_size()) throw std::invalid_argument("host_peek takes one block of tokens");
        return bm.host_peek(hash, toks.data());
      })
      .def("restore", &BlockManager::restore)
      // -> (spills [(block, slot)], fills [(slot, block)])
      .def("take_moves", [](BlockManager& bm) {
        std::vector<KvMove> sp, fi;
        bm.take_moves(sp, fi);
        py::list a, b;
        for (const KvMove& m : sp) a.append(py::make_tuple(m.block, m.slot));
        for (const KvMove& m : fi) b.append(py::make_tuple(m.slot, m.block));
        return py::make_tuple(a, b);
      })
      .def_property_readonly("num_host_cached", &BlockManager::num_host_cached)
      .def_property_readonly("host_hit_blocks", &BlockManager::host_hit_blocks)
      .def_property_readonly("host_spilled_blocks", &BlockManager::host_spilled_blocks)
      .def_property_readonly("host_evicted_blocks", &BlockManager::host_evicted_blocks);

  py::class_<Scheduler>(m, "Scheduler")
      .def(py::init([](const py::dict& d) {
        SchedulerConfig c;
        if (d.contains("num_blocks")) c.num_blocks = d["num_blocks"].cast<int32_t>();
        if (d.contains("block_size")) c.block_size = d["block_size"].cast<int32_t>();
        if (d.contains("max_num_seqs")) c.max_num_seqs = d["max_num_seqs"].cast<int32_t>();
        if (d.contains("max_num_batched_tokens"))
          c.max_num_batched_tokens = d["max_num_batched_tokens"].cast<int32_t>();
        if (d.contains("max_prefill_tokens"))
          c.max_prefill_tokens = d["max_prefill_tokens"].cast<int32_t>();
        if (d.contains("max_model_len")) c.max_model_len = d["max_model_len"].cast<int32_t>();
        if (d.contains("gqa_group")) c.gqa_group = d["gqa_group"].cast<int32_t>();
        if (d.contains("att_qcols")) c.att_qcols = d["att_qcols"].cast<int32_t>();
        if (d.contains("att_wide_min_tokens")) c.att_wide_min_tokens = d["att_wide_min_tokens"].cast<int32_t>();
        if (d.contains("prefill_split_keys")) c.prefill_split_keys = d["prefill_split_keys"].cast<int32_t>();
        if (d.contains("prefix_caching")) c.prefix_caching = d["prefix_caching"].cast<bool>();
        if (d.contains("dedup_inflight_prefix")) c.dedup_inflight_prefix = d["dedup_inflight_prefix"].cast<bool>();
        if (d.contains("max_prefix_defer")) c.max_prefix_defer = d["max_prefix_defer"].cast<int32_t>();
        if (d.contains("same_step_prefix")) c.same_step_prefix = d["same_step_prefix"].cast<bool>();
        if (d.contains("partial_block_reuse")) c.partial_block_reuse = d["partial_block_reuse"].cast<bool>();
        if (d.contains("partial_block_min")) c.partial_block_min = d["partial_block_min"].cast<int32_t>();
        if (d.contains("embed_first")) c.embed_first = d["embed_first"].cast<bool>();
        if (d.contains("embed_first_max_wait")) c.embed_first_max_wait = d["embed_first_max_wait"].cast<int32_t>();
        if (d.contains("split_decode")) c.split_decode = d["split_decode"].cast<bool>();
        if (d.contains("token_align")) c.token_align = d["token_align"].cast<int32_t>();
        if (d.contains("kv_heads")) c.kv_heads = d["kv_heads"].cast<int32_t>();
        if (d.contains("align_slack")) c.align_slack = d["align_slack"].cast<int32_t>();
        if (d.contains("small_step_tokens")) c.small_step_tokens = d["small_step_tokens"].cast<int32_t>();
        if (d.contains("small_step_part")) c.small_step_part = d["small_step_part"].cast<int32_t>();
        if (d.contains("decode_part_target")) c.decode_part_target = d["decode_part_target"].cast<int32_t>();
        if (d.contains("small_step_target")) c.small_step_target = d["small_step_target"].cast<int32_t>();
        if (d.contains("penalty_slots")) c.penalty_slots = d["penalty_slots"].cast<int32_t>();
        if (d.contains("embed_span_slots")) c.embed_span_slots = d["embed_span_slots"].cast<int32_t>();
        if (d.contains("host_slots")) c.host_slots = d["host_slots"].cast<int32_t>();
        if (d.contains("host_cache_step_blocks"))
          c.host_cache_step_blocks = d["host_cache_step_blocks"].cast<int32_t>();
        if (c.host_slots < 0 || c.host_cache_step_blocks < 0)
          throw std::invalid_argument("scheduler: host_slots and host_cache_step_blocks must not be negative");
        if (c.host_slots > 0 && !c.prefix_caching)
          throw std::invalid_argument("scheduler: the host tier (host_slots > 0) needs prefix_caching");
        if (d.contains("eos_ids")) c.eos_ids = d["eos_ids"].cast<std::vector<int32_t>>();
        return std::make_unique<Scheduler>(c);
      }))
      .def("layout", [](const Scheduler& s) {
        const StepLayout& L = s.layout();
        py::dict d;
        d["max_tokens"] = L.max_tokens; d["max_seqs"] = L.max_seqs; d["max_blocks"] = L.max_blocks;
        d["max_items"] = L.max_items;
        d["input_ids"] = L.input_ids; d["positions"] = L.positions; d["slots"] = L.slots;
        d["q_start"] = L.q_start; d["q_len"] = L.q_len; d["ctx_len"] = L.ctx_len;
        d["logit_rows"] = L.logit_rows; d["mask_class"] = L.mask_class; d["forced"] = L.forced;
        d["offsets"] = L.offsets; d["temperature"] = L.temperature; d["seeds"] = L.seeds;
        d["top_k"] = L.top_k; d["top_p"] = L.top_p;
        d["items"] = L.items; d["n_items"] = L.n_items; d["part_size"] = L.part_size;
        d["counts"] = L.counts; d["block_table"] = L.block_table; d["embed_rows"] = L.embed_rows;
        d["lp_n"] = L.lp_n;
        d["pen_slot"] = L.pen_slot; d["pen_reset"] = L.pen_reset; d["pen_presence"] = L.pen_presence;
        d["pen_frequency"] = L.pen_frequency; d["pair_start"] = L.pair_start; d["pair_n"] = L.pair_n;
        d["pair_tok"] = L.pair_tok; d["pair_cap"] = L.pair_cap;
        d["bias_start"] = L.bias_start; d["bias_n"] = L.bias_n; d["minp"] = L.minp; d["ln_minp"] = L.ln_minp;
        d["bias_tok"] = L.bias_tok; d["bias_val"] = L.bias_val; d["bias_cap"] = L.bias_cap;
        d["rep_slot"] = L.rep_slot; d["rep_reset"] = L.rep_reset; d["rep_r"] = L.rep_r;
        d["rep_inv_r"] = L.rep_inv_r; d["rep_start"] = L.rep_start; d["rep_n"] = L.rep_n;
        d["rep_tok"] = L.rep_tok; d["rep_cap"] = L.rep_cap; d["rep_total"] = L.rep_total;
        d["score_target"] = L.score_target; d["score_total"] = L.score_total;
        d["n_copies"] = L.n_copies; d["copy_list"] = L.copy_list; d["copy_total"] = L.copy_total;
        d["run_first"] = L.run_first; d["run_len"] = L.run_len; d["spec_total"] = L.spec_total;
        d["span_n"] = L.span_n; d["span_segs"] = L.span_segs; d["span_slots"] = L.span_slots;
        d["span_total"] = L.span_total;
        d["total"] = L.total;
        return d;
      })
      .def("add_request",
           [](Scheduler& s, int64_t id, const std::vector<int32_t>& prompt, float temperature,
              int32_t max_tokens, int64_t seed, bool ignore_eos,
              const std::vector<int32_t>& stop_ids, const py::object& grammar, int32_t top_k,
              float top_p, bool embed, bool embed_last, int32_t logprobs, float presence_penalty,
              float frequency_penalty, const std::vector<std::pair<int32_t, float>>& logit_bias,
              float min_p, float ln_min_p, float repetition_penalty, float inv_repetition_penalty,
              int32_t score_from, const std::vector<int32_t>& prediction, bool prompt_lookup,
              int32_t draft_len, const std::vector<std::pair<int32_t, int32_t>>& spans) {
             s.add_request(id, prompt, temperature, max_tokens, seed, ignore_eos, stop_ids,
                           make_grammar(grammar), top_k, top_p, embed, embed_last, logprobs,
                           presence_penalty, frequency_penalty, logit_bias, min_p, ln_min_p,
                           repetition_penalty, inv_repetition_penalty, score_from, prediction,
                           prompt_lookup, draft_len, spans);
           },
           py::arg("id"), py::arg("prompt"), py::arg("temperature"), py::arg("max_tokens"),
           py::arg("seed"), py::arg("ignore_eos"), py::arg("stop_ids"), py::arg("grammar"),
           py::arg("top_k") = 0, py::arg("top_p") = 1.0f, py::arg("embed") = false,
           py::arg("embed_last") = false, py::arg("logprobs") = -1, py::arg("presence_penalty") = 0.0f,
           py::arg("frequency_penalty") = 0.0f,
           py::arg("logit_bias") = std::vector<std::pair<int32_t, float>>{}, py::arg("min_p") = 0.0f,
           py::arg("ln_min_p") = 0.0f, py::arg("repetition_penalty") = 1.0f,
           py::arg("inv_repetition_penalty") = 0.0f, py::arg("score_from") = -1,
           py::arg("prediction") = std::vector<int32_t>{}, py::arg("prompt_lookup") = false,
           py::arg("draft_len") = 0, py::arg("spans") = std::vector<std::pair<int32_t, int32_t>>{})
      // words: the buffer's size in 32-bit words (0 = not stated: steps of requests with a
      // repetition penalty, which write behind layout()["total"], are then refused)
      .def("schedule", [](Scheduler& s, uintptr_t buf, int32_t words) {
        py::gil_scoped_release nogil;
        return s.schedule(reinterpret_cast<int32_t*>(buf), words);
      }, py::arg("buf"), py::arg("words") = 0)
      // logprobs: address of the step's LogprobRecord array (41 32-bit words per sampling row:
      // logprob, 20 ids, 20 logprobs), 0 = the step computed none
      // scores: address of the step's ScoreRecord array (42 words per row: logprob, rank, 20 ids,
      // 20 logprobs; indexed by row like `sampled`), 0 = the step computed none
      // accept_len: address of the step's acceptance lengths (one int32 per row, indexed like
      // `sampled`; csrc/ops/spec_verify.hip), 0 = every run commits one token
      .def("commit", [](Scheduler& s, uintptr_t sampled, int32_t n, uintptr_t logprobs, uintptr_t scores,
                        uintptr_t accept_len) {
        std::vector<SeqOutput> outs;
        {
          py::gil_scoped_release nogil;
          outs = s.commit(reinterpret_cast<const int32_t*>(sampled), n,
                          reinterpret_cast<const LogprobRecord*>(logprobs),
                          reinterpret_cast<const ScoreRecord*>(scores),
                          reinterpret_cast<const int32_t*>(accept_len));
        }
        return outputs_to_py(outs);
      }, py::arg("sampled"), py::arg("n"), py::arg("logprobs") = 0, py::arg("scores") = 0,
         py::arg("accept_len") = 0)
      .def_property_readonly_static("COUNTS9_SPEC_BIT", [](const py::object&) { return (int)COUNTS9_SPEC_BIT; })
      .def_property_readonly_static("MAX_DRAFT_LEN", [](const py::object&) { return (int)MAX_DRAFT_LEN; })
      .def_property_readonly("spec_draft_tokens", &Scheduler::spec_draft_tokens)
      .def_property_readonly("spec_accepted_tokens", &Scheduler::spec_accepted_tokens)
      .def_property_readonly("spec_draft_steps", &Scheduler::spec_draft_steps)
      .def_property_readonly("spec_runs_full", &Scheduler::spec_runs_full)
      // [(id, proposed, accepted, prediction_matched)] of the drafting requests finished since the last call
      .def("take_draft_counts", [](Scheduler& s) {
        py::list l;
        for (const auto& c : s.take_draft_counts()) l.append(py::make_tuple(c.id, c.proposed, c.accepted, c.matched));
        return l;
      })
      .def("planned_draft", &Scheduler::planned_draft)
      .def_property_readonly_static("COUNTS9_SPAN_BIT", [](const py::object&) { return (int)COUNTS9_SPAN_BIT; })
      // [(id, [span slot per span])] of the span requests finished or aborted since the last call
      .def("take_span_finishes", &Scheduler::take_span_finishes)
      .def_property_readonly("num_free_span_slots", &Scheduler::num_free_span_slots)
      .def_property_readonly_static("LOGPROB_RECORD_WORDS",
                                    [](const py::object&) { return (int)(sizeof(LogprobRecord) / 4); })
      .def_property_readonly_static("SCORE_RECORD_WORDS",
                                    [](const py::object&) { return (int)(sizeof(ScoreRecord) / 4); })
      .def_property_readonly_static("COUNTS9_SCORE_BIT", [](const py::object&) { return (int)COUNTS9_SCORE_BIT; })
      .def_property_readonly_static("FINISH_SCORE", [](const py::object&) { return (int)FINISH_SCORE; })
      .def("abort", &Scheduler::abort)
      .def("take_embed_resets", &Scheduler::take_embed_resets)
      // host tier: -> (spills [(block, slot)], fills [(slot, block)]) of the last schedule() call;
      // run all spills, then all fills, before the step
      .def("take_kv_moves", [](Scheduler& s) {
        const Scheduler::KvMoves m = s.take_kv_moves();
        py::list a, b;
        for (const KvMove& x : m.spills) a.append(py::make_tuple(x.block, x.slot));
        for (const KvMove& x : m.fills) b.append(py::make_tuple(x.slot, x.block));
        return py::make_tuple(a, b);
      })
      .def_property_readonly("host_hit_blocks", &Scheduler::host_hit_blocks)
      .def_property_readonly("host_spilled_blocks", &Scheduler::host_spilled_blocks)
      .def_property_readonly("host_evicted_blocks", &Scheduler::host_evicted_blocks)
      .def_property_readonly("num_host_cached", &Scheduler::num_host_cached)
      // [(tier, id)]: tier 0 = device block, 1 = host slot; stops at the first miss
      .def("prefix_blocks", &Scheduler::prefix_blocks)
      .def("planned_ids", &Scheduler::planned_ids)
      .def("num_free_embed_rows", &Scheduler::num_free_embed_rows)
      .def_property_readonly("num_free_penalty_slots", &Scheduler::num_free_penalty_slots)
      .def_property_readonly("prefix_defers", &Scheduler::prefix_defers)
      .def_property_readonly("partial_hit_tokens", &Scheduler::partial_hit_tokens)
      .def_property_readonly("same_step_shares", &Scheduler::same_step_shares)
      .def_property_readonly("num_donor_blocks", &Scheduler::num_donor_blocks)
      .def("block_ref", &Scheduler::block_ref)
      .def_property_readonly("inflight_steps", &Scheduler::inflight_steps)
      .def_property_readonly("spec_rows", &Scheduler::spec_rows)
      .def_property_readonly("spec_voided", &Scheduler::spec_voided)
      .def("debug_state", [](const Scheduler& s) {
        py::list l;
        for (const auto& x : s.debug_state())
          l.append(py::make_tuple(x.id, x.running, x.embed, x.embed_slot, x.num_computed, x.num_tokens,
                                  x.num_blocks));
        return l;
      })
      .def("drain_aborted", [](Scheduler& s) { return outputs_to_py(s.drain_aborted()); })
      .def("has_work", &Scheduler::has_work)
      .def("reset_prefix_cache", &Scheduler::reset_prefix_cache)
      .def_property_readonly("num_running", &Scheduler::num_running)
      .def_property_readonly("num_waiting", &Scheduler::num_waiting)
      .def_property_readonly("num_free_blocks", &Scheduler::num_free_blocks)
      .def_property_readonly("num_cached_blocks", &Scheduler::num_cached_blocks)
      .def_property_readonly("total_prompt_tokens", &Scheduler::total_prompt_tokens)
      .def_property_readonly("total_cached_tokens", &Scheduler::total_cached_tokens)
      .def_property_readonly("total_preemptions", &Scheduler::total_preemptions)
      .def_property_readonly("steps", &Scheduler::steps)
      .def_property_readonly("aligned_steps", &Scheduler::aligned_steps);
}
