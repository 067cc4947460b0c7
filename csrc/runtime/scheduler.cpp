#include "scheduler.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <unordered_set>

namespace rt {

double now_seconds() {
  using namespace std::chrono;
  return duration<double>(steady_clock::now().time_since_epoch()).count();
}

static int32_t align4(int32_t x) { return (x + 3) & ~3; }

// the record of a token the grammar left no choice for: probability 1 among the allowed tokens
static LogprobRecord forced_record(int32_t tok, int32_t n) {
  LogprobRecord r;
  r.lp = 0.f;
  for (int32_t i = 0; i < LOGPROB_TOP; ++i) {
    r.ids[i] = -1;
    r.lps[i] = -INFINITY;
  }
  if (n > 0) {
    r.ids[0] = tok;
    r.lps[0] = 0.f;
  }
  return r;
}

Scheduler::Scheduler(const SchedulerConfig& cfg)
    : cfg_(cfg), bm_(cfg.num_blocks, cfg.block_size, cfg.prefix_caching, cfg.host_slots) {
  StepLayout& L = lay_;
  L.max_tokens = cfg.max_num_batched_tokens;
  L.max_seqs = cfg.max_num_seqs;
  L.max_blocks = (cfg.max_model_len + cfg.block_size - 1) / cfg.block_size;
  const int32_t tpw = 16 / std::max(1, cfg.gqa_group);
  const int32_t max_parts = (cfg.max_model_len + 511) / 512;
  L.max_items = L.max_tokens / (2 * tpw) + L.max_seqs * (max_parts + 1) + 4;
  int32_t o = 0;
  auto take = [&](int32_t n) {
    const int32_t at = o;
    o = align4(o + n);
    return at;
  };
  L.counts = take(12);
  L.n_items = take(1);
  L.part_size = take(1);
  L.input_ids = take(L.max_tokens);
  L.positions = take(L.max_tokens);
  L.slots = take(L.max_tokens);
  L.q_start = take(L.max_seqs);
  L.q_len = take(L.max_seqs);
  L.ctx_len = take(L.max_seqs);
  L.logit_rows = take(L.max_seqs);
  L.mask_class = take(L.max_seqs);
  L.forced = take(L.max_seqs);
  L.offsets = take(L.max_seqs);
  L.temperature = take(L.max_seqs);
  L.top_k = take(L.max_seqs);
  L.top_p = take(L.max_seqs);
  L.seeds = take(2 * L.max_seqs);
  L.lp_n = take(L.max_seqs);
  L.items = take(4 * L.max_items);
  L.block_table = take(L.max_seqs * L.max_blocks);
  L.embed_rows = take(L.max_tokens);
  L.pen_slot = take(L.max_seqs);
  L.pen_reset = take(L.max_seqs);
  L.pen_presence = take(L.max_seqs);
  L.pen_frequency = take(L.max_seqs);
  L.pair_start = take(L.max_seqs);
  L.pair_n = take(L.max_seqs);
  L.pair_cap = L.max_tokens + cfg.max_model_len;
  L.pair_tok = take(L.pair_cap);
  L.bias_start = take(L.max_seqs);
  L.bias_n = take(L.max_seqs);
  L.minp = take(L.max_seqs);
  L.ln_minp = take(L.max_seqs);
  L.bias_cap = L.max_seqs * LOGIT_BIAS_MAX;
  L.bias_tok = take(L.bias_cap);
  L.bias_val = take(L.bias_cap);
  L.total = o;
  L.rep_slot = take(L.max_seqs);
  L.rep_reset = take(L.max_seqs);
  L.rep_r = take(L.max_seqs);
  L.rep_inv_r = take(L.max_seqs);
  L.rep_start = take(L.max_seqs);
  L.rep_n = take(L.max_seqs);
  L.rep_cap = L.max_tokens + cfg.max_model_len;
  L.rep_tok = take(L.rep_cap);
  L.rep_total = o;
  L.score_target = take(L.max_seqs);
  L.score_total = o;
  L.n_copies = L.n_items + 1;  // a word of the header's padding: every step copies it
  L.copy_list = take(3 * L.max_seqs);
  L.copy_total = o;
  L.run_first = take(L.max_seqs);
  L.run_len = take(L.max_seqs);
  L.spec_total = o;
  L.span_slots = std::max(0, cfg.embed_span_slots);
  L.span_n = take(1);
  L.span_segs = take(4 * L.span_slots);
  L.span_total = o;
  for (int32_t r = L.span_slots; r-- > 0;) span_free_.push_back(r);
  for (int32_t r = L.max_seqs; r-- > 0;) embed_free_.push_back(r);
  for (int32_t r = std::max(0, std::min(cfg.max_num_seqs, cfg.penalty_slots)); r-- > 0;) pen_free_.push_back(r);
}

void Scheduler::add_request(int64_t id, std::vector<int32_t> prompt, float temperature,
                            int32_t max_tokens, int64_t seed, bool ignore_eos,
                            std::vector<int32_t> stop_ids, std::unique_ptr<Grammar> grammar,
                            int32_t top_k, float top_p, bool embed, bool embed_last, int32_t logprobs,
                            float presence_penalty, float frequency_penalty,
                            std::vector<std::pair<int32_t, float>> logit_bias, float min_p,
                            float ln_min_p, float repetition_penalty, float inv_repetition_penalty,
                            int32_t score_from, std::vector<int32_t> prediction, bool prompt_lookup,
                            int32_t draft_len, std::vector<std::pair<int32_t, int32_t>> spans) {
  if (!spans.empty()) {
    // like a scoring request's positions, nothing of a span may be dropped or moved silently
    if (!embed || embed_last || score_from != -1)
      throw std::invalid_argument("scheduler: spans belong to a mean-pooled embedding request");
    if ((int32_t)prompt.size() >= cfg_.max_model_len)
      throw std::invalid_argument("scheduler: a request with spans needs a prompt shorter than max_model_len");
    if ((int32_t)spans.size() > lay_.span_slots)
      throw std::invalid_argument("scheduler: more spans than embed_span_slots");
    if (lay_.rep_cap >= (1 << 26))
      throw std::invalid_argument("scheduler: spans need max_num_batched_tokens + max_model_len < 2^26");
    for (size_t i = 0; i < spans.size(); ++i)
      if (spans[i].first < 0 || spans[i].first >= spans[i].second || spans[i].second > (int32_t)prompt.size() ||
          (i > 0 && spans[i].first < spans[i - 1].first))
        throw std::invalid_argument("scheduler: spans must be ranges 0 <= a < b <= prompt_len sorted by a");
  }
  draft_len = std::max(0, std::min(draft_len, MAX_DRAFT_LEN));
  const bool drafting = draft_len > 0 && (!prediction.empty() || prompt_lookup);
  if (drafting) {
    // a draft row samples before the tokens in front of it are known to be real: state kept per
    // committed token (penalty counts, seen sets) and records per token cannot follow that
    if (embed || score_from != -1 || logprobs >= 0 || presence_penalty != 0.f || frequency_penalty != 0.f ||
        (repetition_penalty != 1.f && repetition_penalty > 0.f))
      throw std::invalid_argument("scheduler: a drafting request takes no embed, score_from, logprobs, "
                                  "presence / frequency penalty or repetition_penalty");
    for (int32_t t : prediction)
      if (t < 0) throw std::invalid_argument("scheduler: prediction token ids must be >= 0");
  }
  if (score_from != -1) {
    // nothing of a scoring request may be dropped or changed silently: its records are
    // per prompt position
    if (score_from < 1 || score_from > (int32_t)prompt.size() - 1)
      throw std::invalid_argument("scheduler: score_from must lie in [1, prompt_len - 1]");
    if ((int32_t)prompt.size() >= cfg_.max_model_len)
      throw std::invalid_argument("scheduler: a scoring request's prompt must be shorter than max_model_len");
    if (embed || grammar || presence_penalty != 0.f || frequency_penalty != 0.f || !logit_bias.empty() ||
        min_p != 0.f || repetition_penalty != 1.f)
      throw std::invalid_argument("scheduler: a scoring request takes no embed, grammar, penalty, "
                                  "logit_bias, min_p or repetition_penalty");
  }
  auto s = std::make_unique<Sequence>();
  s->id = id;
  if (score_from != -1) {
    s->score_from = score_from;
    s->score_n = std::max(0, std::min(logprobs, LOGPROB_TOP));
    logprobs = -1;  // no record per generated token: there are none
    score_requested_ = true;
    ++score_live_;
  }
  if ((int32_t)prompt.size() >= cfg_.max_model_len)
    prompt.resize(cfg_.max_model_len - 1);  // keep room for at least one generated token
  if (prompt.empty()) prompt.push_back(0);
  s->tokens = std::move(prompt);
  s->prompt_len = (int32_t)s->tokens.size();
  s->temperature = temperature;
  s->top_k = std::max(0, top_k);
  s->top_p = (top_p > 0.f && top_p < 1.f) ? top_p : 1.f;
  s->max_tokens = std::max(1, max_tokens);
  s->seed = seed;
  s->ignore_eos = ignore_eos;
  s->stop_ids = std::move(stop_ids);
  s->grammar = embed ? nullptr : std::move(grammar);
  s->embed = embed;
  s->embed_last = embed && embed_last;
  s->logprobs = embed ? -1 : std::min(logprobs, LOGPROB_TOP);
  s->presence_penalty = (embed || !std::isfinite(presence_penalty)) ? 0.f : presence_penalty;
  s->frequency_penalty = (embed || !std::isfinite(frequency_penalty)) ? 0.f : frequency_penalty;
  if (!embed) {
    // the device pass wants unique ids per row: sorted by id, the first entry of an id kept
    logit_bias.erase(std::remove_if(logit_bias.begin(), logit_bias.end(),
                                    [](const std::pair<int32_t, float>& e) {
                                      return e.first < 0 || e.second == 0.f || !std::isfinite(e.second);
                                    }),
                     logit_bias.end());
    std::stable_sort(logit_bias.begin(), logit_bias.end(),
                     [](const std::pair<int32_t, float>& a, const std::pair<int32_t, float>& b) {
                       return a.first < b.first;
                     });
    logit_bias.erase(std::unique(logit_bias.begin(), logit_bias.end(),
                                 [](const std::pair<int32_t, float>& a, const std::pair<int32_t, float>& b) {
                                   return a.first == b.first;
                                 }),
                     logit_bias.end());
    if ((int32_t)logit_bias.size() > LOGIT_BIAS_MAX) logit_bias.resize(LOGIT_BIAS_MAX);
    s->logit_bias = std::move(logit_bias);
    if (min_p > 0.f && min_p <= 1.f && std::isfinite(ln_min_p) && ln_min_p <= 0.f) {
      s->min_p = min_p;
      s->ln_min_p = ln_min_p;
    }
  }
  if (!embed && std::isfinite(repetition_penalty) && repetition_penalty > 0.f && repetition_penalty <= 2.f &&
      repetition_penalty != 1.f) {
    s->repetition_penalty = repetition_penalty;
    rep_requested_ = true;
    s->inv_repetition_penalty = (std::isfinite(inv_repetition_penalty) && inv_repetition_penalty > 0.f)
                                    ? inv_repetition_penalty : (float)(1.0 / (double)repetition_penalty);
  }
  if (drafting) {
    s->prediction = std::move(prediction);
    s->prompt_lookup = prompt_lookup;
    s->draft_len = draft_len;
    ++draft_live_;
  }
  if (!spans.empty()) {
    s->spans = std::move(spans);
    span_requested_ = true;
  }
  s->arrival = arrival_counter_++;
  // a grammar that starts with forced text (e.g. '{"key": ') is jump-forwarded into the prompt
  if (s->grammar) {
    const int32_t room = cfg_.max_model_len - (int32_t)s->tokens.size() - 1;
    const int32_t k = s->grammar->take_forced_run(s->tokens, std::min(room, s->max_tokens - 1));
    s->num_generated += k;
    s->num_forced += k;
    if (s->logprobs >= 0)
      for (int32_t j = 0; j < k; ++j)
        s->lp_records.push_back(forced_record(s->tokens[s->prompt_len + j], s->logprobs));
  }
  follow_prediction(s.get(), (size_t)s->prompt_len);  // the forced head of the reply
  Sequence* raw = s.get();
  seqs_.emplace(id, std::move(s));
  waiting_.push_back(raw);
}

uint64_t Scheduler::prefix_key(const Sequence* s) const {
  // hash chain of the first two full blocks (what match_prefix would look up first)
  const int32_t B = cfg_.block_size;
  if ((int32_t)s->tokens.size() <= 2 * B) return 0;
  const uint64_t h1 = hash_block(0, s->tokens.data(), B);
  return hash_block(h1, s->tokens.data() + B, B) | 1ull;
}

void Scheduler::free_seq(Sequence* s, bool keep_embed_slot) {
  if (s->embed_slot >= 0 && !keep_embed_slot) {
    embed_free_.push_back(s->embed_slot);
    s->embed_slot = -1;
  }
  if (!keep_embed_slot) {  // recycled without clearing: the next holder's first segment has init = 1
    span_free_.insert(span_free_.end(), s->span_slots.begin(), s->span_slots.end());
    s->span_slots.clear();
  }
  drop_copy(s);
  for (int32_t b : s->blocks) bm_.release(b);
  s->blocks.clear();
  s->block_hashes.clear();
}

void Scheduler::drop_copy(Sequence* s) {
  if (s->copy_j > 0) bm_.release(s->copy_src);
  s->copy_src = s->copy_dst = -1;
  s->copy_j = 0;
}

void Scheduler::preempt(Sequence* s) {
  // an embedding request keeps its pooling row, but restarts from token 0: the row's
  // partial sums must be cleared before the next step runs (take_embed_resets)
  if (s->embed_slot >= 0) embed_resets_.push_back(s->embed_slot);
  free_seq(s, true);
  s->score_records.clear();  // a scoring request starts over: its final output is that of one run
  s->num_computed = 0;
  s->tail_listed = false;
  s->running = false;
  s->preempted = true;
  waiting_.push_front(s);
  ++stat_preemptions_;
}

bool Scheduler::ensure_blocks(Sequence* s, int32_t upto_tokens) {
  const int32_t need =
      (upto_tokens + cfg_.block_size - 1) / cfg_.block_size - (int32_t)s->blocks.size();
  if (need <= 0) return true;
  return bm_.allocate(need, s->blocks);
}

void Scheduler::match_prefix(Sequence* s) {
  const int32_t B = cfg_.block_size;
  if (cfg_.prefix_caching && (!s->embed || s->embed_last)) {
    // never reuse the last token; a scoring request computes position score_from - 1 (its first
    // logits row) itself, everything before it may come from the cache
    const int32_t n_full = (s->scoring() ? s->score_from - 1 : (int32_t)s->tokens.size() - 1) / B;
    uint64_t parent = 0;
    if (cfg_.host_slots <= 0) {
      for (int32_t b = 0; b < n_full; ++b) {
        const int32_t* t = s->tokens.data() + (size_t)b * B;
        const uint64_t h = hash_block(parent, t, B);
        const int32_t blk = bm_.lookup(h, t);
        if (blk < 0) break;
        s->blocks.push_back(blk);
        s->block_hashes.push_back(h);
        parent = h;
      }
    } else {
      // Two passes. First find how far the chain goes on the device or in the host tier, taking
      // the device references (and pinning the host slots): only then is a device block
      // allocated per host hit, so that bringing the head of a chain back never evicts a
      // resident block -- or a host slot -- further along the same chain.
      struct Hit {
        uint64_t h;
        int32_t blk, slot;
      };
      std::vector<Hit> hits;
      int32_t host_hits = 0;
      for (int32_t b = 0; b < n_full; ++b) {
        const int32_t* t = s->tokens.data() + (size_t)b * B;
        const uint64_t h = hash_block(parent, t, B);
        const int32_t blk = bm_.lookup(h, t);
        int32_t slot = -1;
        if (blk < 0) {
          if (host_hits >= fills_left_ || (slot = bm_.host_peek(h, t)) < 0) break;  // the cap ends the chain
          bm_.host_pin(slot, 1);
          ++host_hits;
        }
        hits.push_back({h, blk, slot});
        parent = h;
      }
      const int32_t watermark = std::max(1, cfg_.num_blocks / 100);
      bool ended = false;
      for (const Hit& x : hits) {
        int32_t blk = x.blk;
        if (ended) {  // behind a block that could not be brought back: not part of the chain
          if (blk >= 0) bm_.release(blk);
        } else if (blk < 0) {
          blk = bm_.num_free() > watermark ? bm_.restore(x.slot) : -1;
          if (blk < 0) ended = true;
          else --fills_left_;
        }
        if (x.slot >= 0) bm_.host_pin(x.slot, -1);
        if (ended) continue;
        s->blocks.push_back(blk);
        s->block_hashes.push_back(x.h);
      }
    }
  }
  s->num_computed = (int32_t)s->blocks.size() * B;
}

// Full blocks of the prompt of `s` that `r` -- planned in the step being built, r_end tokens
// computed at its end -- holds: the common prefix in whole blocks, never the last token of `s`.
static int32_t shareable_blocks(const Sequence* s, const Sequence* r, int32_t r_end, int32_t B) {
  const int32_t limit = s->scoring() ? s->score_from - 1 : (int32_t)s->tokens.size() - 1;
  const int32_t cap = std::min(std::min(limit, r_end), (int32_t)r->tokens.size());
  int32_t c = 0;
  while (c < cap && s->tokens[c] == r->tokens[c]) ++c;
  return std::min<int32_t>(c / B, (int32_t)r->blocks.size());
}

int32_t Scheduler::share_same_step(Sequence* s, const Sequence* r, int32_t r_end) {
  const int32_t B = cfg_.block_size;
  const int32_t m = shareable_blocks(s, r, r_end, B);
  int32_t added = 0;
  // behind what the hash cache gave: these blocks are registered only when the step commits
  for (int32_t b = (int32_t)s->blocks.size(); b < m; ++b) {
    bm_.add_ref(r->blocks[b]);
    s->blocks.push_back(r->blocks[b]);
    ++added;
  }
  s->num_computed = (int32_t)s->blocks.size() * B;
  return added;
}

void Scheduler::match_partial(Sequence* s) {
  const int32_t B = cfg_.block_size;
  if (!cfg_.prefix_caching || !cfg_.partial_block_reuse || !copies_ok_ || s->copy_j > 0) return;
  if (s->embed && !s->embed_last) return;
  if (s->block_hashes.size() != s->blocks.size()) return;  // the chain's end is not a cached block
  const int32_t base = (int32_t)s->blocks.size() * B;
  // at least one token is computed (a scoring request: position score_from - 1)
  const int32_t limit = s->scoring() ? s->score_from - 1 : (int32_t)s->tokens.size() - 1;
  const int32_t max_j = std::min(B, limit - base);
  if (max_j < std::max(1, cfg_.partial_block_min)) return;
  if (bm_.num_free() <= std::max(1, cfg_.num_blocks / 100)) return;  // the admission watermark
  const uint64_t parent = s->block_hashes.empty() ? 0 : s->block_hashes.back();
  int32_t j = 0;
  const int32_t donor = bm_.match_head(parent, s->tokens.data() + base, (int32_t)s->tokens.size() - base,
                                       max_j, cfg_.partial_block_min, &j);
  if (donor < 0) return;
  if (!bm_.allocate(1, s->blocks)) {
    bm_.release(donor);
    return;
  }
  s->copy_src = donor;
  s->copy_dst = s->blocks.back();
  s->copy_j = j;
  s->num_computed = base + j;
}

void Scheduler::count_cached(Sequence* s) {
  if (s->cached_prompt_tokens >= 0) return;
  s->cached_prompt_tokens = std::min(s->num_computed, s->prompt_len);
  stat_cached_tokens_ += s->cached_prompt_tokens;
  stat_prompt_tokens_ += s->prompt_len;
  stat_partial_tokens_ += s->copy_j;
}

void Scheduler::register_full_blocks(Sequence* s) {
  if (!cfg_.prefix_caching) return;
  const int32_t B = cfg_.block_size;
  const int32_t full = std::min<int32_t>(s->num_computed / B, (int32_t)s->blocks.size());
  for (int32_t b = (int32_t)s->block_hashes.size(); b < full; ++b) {
    const uint64_t parent = b ? s->block_hashes[b - 1] : 0;
    const int32_t* t = s->tokens.data() + (size_t)b * B;
    const uint64_t h = hash_block(parent, t, B);
    bm_.register_block(s->blocks[b], h, t, parent);
    s->block_hashes.push_back(h);
  }
  // the prompt's partly filled last block, once the prompt is computed: a donor of its head
  if (cfg_.partial_block_reuse && !s->tail_listed && !s->embed && !s->scoring() &&
      s->num_computed >= s->prompt_len) {
    const int32_t idx = s->prompt_len / B, fill = s->prompt_len % B;
    if (fill > 0 && idx < (int32_t)s->blocks.size() && (int32_t)s->block_hashes.size() == idx)
      bm_.register_partial(s->blocks[idx], idx ? s->block_hashes[idx - 1] : 0,
                           s->tokens.data() + (size_t)idx * B, fill);
    s->tail_listed = true;
  }
}

// Tokens tokens[from:] were just committed: the prediction cursor follows them while they are
// the prediction's own next tokens, and loses its alignment at the first one that is not.
int32_t Scheduler::follow_prediction(Sequence* s, size_t from) {
  int32_t matched = 0;
  if (s->prediction.empty()) return matched;
  for (size_t i = from; i < s->tokens.size() && s->pred_synced; ++i) {
    if (s->pred_c < (int32_t)s->prediction.size() && s->prediction[s->pred_c] == s->tokens[i]) {
      ++s->pred_c;
      ++matched;
    } else {
      // the cursor steps over the token that failed, so the resync looks behind it: a reply of
      // one repeated token would otherwise resync onto the same wrong token for ever
      s->pred_synced = false;
      if (s->pred_c < (int32_t)s->prediction.size()) ++s->pred_c;
    }
  }
  return matched;
}

// The draft of a decode row, t = the request's tokens so far:
//   prediction  with the cursor c aligned (the tokens committed last were the prediction's):
//               prediction[c : c + k]. Otherwise resync: for n = 4, 3, 2 the first i >= c with
//               prediction[i - n : i] == t[-n:] becomes c. No n matches: the prediction proposes
//               nothing and c stays (it never moves back; follow_prediction has put it behind the
//               prediction token that failed).
//   lookup      (prompt_lookup, and the prediction proposed nothing) for n = 4, 3, 2 the latest
//               i <= len(t) - 1 with t[i - n : i] == t[-n:]: t[i : i + k], cut at the end of t.
std::vector<int32_t> Scheduler::propose(Sequence* s, int32_t k, bool* from_prediction) const {
  std::vector<int32_t> out;
  *from_prediction = false;
  if (k <= 0) return out;
  const std::vector<int32_t>& t = s->tokens;
  const std::vector<int32_t>& P = s->prediction;
  const int32_t len = (int32_t)t.size(), plen = (int32_t)P.size();
  if (plen > 0) {
    if (!s->pred_synced) {
      for (int32_t n = 4; n >= 2 && !s->pred_synced; --n) {
        if (len < n) continue;
        for (int32_t i = std::max(s->pred_c, n); i < plen; ++i)
          if (std::equal(P.begin() + (i - n), P.begin() + i, t.end() - n)) {
            s->pred_c = i;
            s->pred_synced = true;
            break;
          }
      }
    }
    if (s->pred_synced && s->pred_c < plen) {
      out.assign(P.begin() + s->pred_c, P.begin() + std::min(plen, s->pred_c + k));
      *from_prediction = true;
      return out;
    }
  }
  if (s->prompt_lookup) {
    for (int32_t n = 4; n >= 2; --n) {
      if (len <= n) continue;
      for (int32_t i = len - 1; i >= n; --i)
        if (std::equal(t.begin() + (i - n), t.begin() + i, t.end() - n)) {
          out.assign(t.begin() + i, t.begin() + std::min(len, i + k));
          return out;
        }
    }
  }
  return out;
}

int32_t Scheduler::schedule(int32_t* buf, int32_t buf_words) {
  const StepLayout& L = lay_;
  const int32_t B = cfg_.block_size;
  if (rep_requested_ && buf_words < L.rep_total)  // before anything is planned or written
    throw std::invalid_argument("scheduler: a request with a repetition penalty needs a step buffer of "
                                "layout().rep_total words, stated as schedule()'s second argument");
  if (score_requested_ && buf_words < L.score_total)
    throw std::invalid_argument("scheduler: a scoring request needs a step buffer of "
                                "layout().score_total words, stated as schedule()'s second argument");
  if (span_requested_ && buf_words < L.span_total)
    throw std::invalid_argument("scheduler: a request with spans needs a step buffer of "
                                "layout().span_total words, stated as schedule()'s second argument");
  copies_ok_ = buf_words >= L.copy_total;
  fills_left_ = std::max(0, cfg_.host_cache_step_blocks);
  drafts_ok_ = buf_words >= L.spec_total && plans_.empty();
  last_plan_.clear();
  // rows of the step (sampling rows + scoring rows) never exceed max_num_seqs. A scoring request
  // can own many: every running sequence that may sample keeps one in reserve, so decode rows are
  // served first whatever the order, and a scoring chunk is cut to the rows that are left (it
  // continues next step). Without scoring requests none of this binds: one row per sequence.
  // The reserve is taken before the token budget is dealt out, so it is an upper bound: a
  // sequence whose remaining tokens could fit this step counts even if the budget then runs out
  // before it (a scoring chunk is cut a little harder than needed, never the other way round);
  // one still more than a step's tokens away from its last prompt token cannot sample and does
  // not count. All of it is skipped while no scoring request is alive (score_live_).
  // Draft rows (a drafting request's rows beyond its first) are budgeted the same way and
  // counted in score_rows_used: plain decode rows are served first, a draft is cut to what is left.
  int32_t rows_reserved = 0, score_rows_used = 0;
  const bool budget_rows = score_live_ > 0 || (drafts_ok_ && draft_live_ > 0);
  if (budget_rows)
    for (const Sequence* r : running_)
      if (r->running && !r->embed && !r->scoring() &&
          (int32_t)r->tokens.size() - r->num_computed <= cfg_.max_num_batched_tokens)
        ++rows_reserved;
  // a scoring entry of n tokens from c0 owns the rows of its positions >= score_from - 1
  auto score_rows_of = [](const Sequence* s, int32_t c0, int32_t n) {
    return s->scoring() ? std::max(0, c0 + n - std::max(c0, s->score_from - 1)) : 0;
  };
  // cut n so that the entry's rows fit what is left; 0 = nothing fits this step
  auto fit_score_rows = [&](const Sequence* s, int32_t n) {
    const int32_t avail = std::max(0, cfg_.max_num_seqs - rows_reserved - score_rows_used);
    const int32_t pre = std::max(0, s->score_from - 1 - s->num_computed);  // tokens before the first row
    return std::min(n, pre + avail);
  };
  auto samples = [](const Sequence* s, int32_t n) {
    return !s->embed && !s->scoring() && s->num_computed + n == (int32_t)s->tokens.size();
  };
  int32_t tok_budget = cfg_.max_num_batched_tokens;
  int32_t prefill_budget = cfg_.max_prefill_tokens;
  // words of the pair region (penalties) the planned sampling rows will take: a penalised row
  // samples only in a step that carries ALL of its unsent generated tokens
  int32_t pair_used = 0;
  auto pair_need = [](const Sequence* s, int32_t n) {
    return (s->penalised() && s->num_computed + n == (int32_t)s->tokens.size())
               ? (int32_t)s->tokens.size() - s->prompt_len - s->pen_synced : 0;
  };
  // the same for the repetition region: such a row samples only in a step that carries ALL the
  // tokens (prompt and generated) its slot has not seen yet
  int32_t rep_used = 0;
  auto rep_need = [](const Sequence* s, int32_t n) {
    return (s->repetitive() && s->num_computed + n == (int32_t)s->tokens.size())
               ? (int32_t)s->tokens.size() - s->rep_synced : 0;
  };

  // 1) running sequences: decode tokens, jump-forward runs, unfinished prefill chunks.
  //    With a step in flight (pipelined use), a row that samples in it is continued
  //    speculatively (predict()); rows listed by an in-flight step are never preempted.
  if (plans_.size() > 1) throw std::logic_error("scheduler: at most one uncommitted step may be in flight");
  const int64_t prev_id = plans_.empty() ? -1 : plans_.back().id;
  for (size_t i = 0; i < running_.size(); ++i) {
    Sequence* s = running_[i];
    if (!s->running || s->abort_pending) continue;
    if (prev_id >= 0 && s->pend_plan == prev_id) {
      Planned e{s, 0, true};
      if (tok_budget <= 0 || !predict(s, e)) continue;  // may finish: wait for the commit
      e.n = 1 + (int32_t)e.run.size();
      if (e.n > tok_budget || !ensure_blocks(s, s->num_computed + e.n)) continue;
      e.spec = true;
      e.src_idx = s->pend_idx;
      tok_budget -= e.n;
      ++stat_spec_rows_;
      last_plan_.push_back(std::move(e));
      continue;
    }
    const int32_t pending = s->compute_len() - s->num_computed;
    if (pending <= 0 || tok_budget <= 0) continue;
    int32_t n = std::min(pending, tok_budget);
    if (s->scoring() && (n = fit_score_rows(s, n)) <= 0) continue;  // no row left: next step
    const int32_t pairs = pair_need(s, n);
    if (pair_used + pairs > L.pair_cap) continue;  // its new tokens do not fit the pair region: next step
    const int32_t reps = rep_need(s, n);
    if (rep_used + reps > L.rep_cap) continue;  // nor does its backlog fit the repetition region
    bool ok = ensure_blocks(s, s->num_computed + n);
    while (!ok) {
      // preempt the most recently arrived running sequence that is not yet planned
      // (and not listed by an in-flight step)
      Sequence* victim = nullptr;
      for (size_t j = running_.size(); j-- > i + 1;) {
        if (running_[j]->running && running_[j]->inflight == 0 && !running_[j]->abort_pending) {
          victim = running_[j];
          break;
        }
      }
      if (!victim) break;
      preempt(victim);
      ok = ensure_blocks(s, s->num_computed + n);
    }
    if (!ok) {
      if (s->inflight == 0) preempt(s);
      continue;
    }
    Planned e{s, n, samples(s, n)};
    tok_budget -= n;
    if (e.sample && drafts_ok_ && s->drafting()) {
      // k: the smallest of draft_len, the tokens the request may still generate minus the one
      // the last row samples, the rows and tokens the step has left, and the free blocks beyond
      // what the running sequences behind this one need for their own next tokens and the
      // admission watermark -- a draft never preempts anybody
      int32_t k = std::min(s->draft_len, s->max_tokens - s->num_generated - 1);
      k = std::min(k, cfg_.max_model_len - (int32_t)s->tokens.size() - 1);
      k = std::min(k, cfg_.max_num_seqs - rows_reserved - score_rows_used);
      k = std::min(k, tok_budget);
      if (k > 0) {
        int32_t others = 0;
        for (size_t j = i + 1; j < running_.size(); ++j) {
          const Sequence* r = running_[j];
          if (r->running) others += std::max(0, (r->compute_len() + B - 1) / B - (int32_t)r->blocks.size());
        }
        const int32_t spare = bm_.num_free() - others - std::max(1, cfg_.num_blocks / 100);
        k = std::min(k, ((int32_t)s->blocks.size() + std::max(0, spare)) * B - (s->num_computed + n));
      }
      if (k > 0) e.draft = propose(s, k, &e.draft_pred);
      if (!e.draft.empty()) {
        // the grammar runs ahead along the draft on a copy of the cursor: row j samples in the
        // state behind j draft tokens. A forced token that differs from the draft ends the draft
        // (that row emits the forced token, the correction, at no cost); so does a draft token
        // that would end the reply (the row in front of it samples it, and the commit finishes
        // the request as ever). A draft token the mask does not allow needs no care: advance_at
        // only compares it with the segment's closing tokens, and the row that verifies it can
        // never sample it, so every row behind it is dropped.
        int32_t cls = -1, forced = -1;
        if (s->grammar) {
          const Grammar& g = *s->grammar;
          Grammar::Cursor c = g.cursor();
          size_t j = 0;
          for (; j < e.draft.size(); ++j) {
            g.next_at(c, &cls, &forced);
            e.row_gram.emplace_back(cls, forced);
            if (forced >= 0 && forced != e.draft[j]) break;
            Grammar::Cursor c2 = c;
            g.advance_at(c2, e.draft[j]);
            if (g.done_at(c2)) break;
            c = c2;
          }
          if (j < e.draft.size()) {
            e.draft.resize(j);  // row j (already listed) is the run's last
          } else {
            g.next_at(c, &cls, &forced);
            e.row_gram.emplace_back(cls, forced);
          }
        } else {
          e.row_gram.assign(e.draft.size() + 1, {-1, -1});
        }
      }
      if (!e.draft.empty()) {
        const int32_t k2 = (int32_t)e.draft.size();
        if (ensure_blocks(s, s->num_computed + n + k2)) {
          e.n = n + k2;
          tok_budget -= k2;
          score_rows_used += k2;
          s->draft_proposed += k2;
          stat_draft_tokens_ += k2;
        } else {  // cannot happen: k was cut to the free blocks
          e.draft.clear();
        }
      }
      if (e.draft.empty()) e.row_gram.clear();
    }
    pair_used += pairs;
    rep_used += reps;
    score_rows_used += score_rows_of(s, s->num_computed, n);
    last_plan_.push_back(std::move(e));
  }
  running_.erase(std::remove_if(running_.begin(), running_.end(),
                                [](Sequence* s) { return !s->running; }),
                 running_.end());

  // 2) admit waiting sequences (FCFS) into the remaining budget. A request whose
  //    leading blocks another sequence is prefilling right now (same prefix_key) is
  //    deferred (at most max_prefix_defer steps) so it reuses them once registered:
  //    an agent task's orchestrator analysis, agent analysis and tool selection arrive
  //    together and all start with the task text.
  const int32_t watermark = std::max(1, cfg_.num_blocks / 100);
  const bool dedup = cfg_.prefix_caching && cfg_.dedup_inflight_prefix;
  std::unordered_set<uint64_t> inflight;
  if (dedup)
    for (const Sequence* r : running_)
      if (r->running && !r->embed && r->num_computed < 2 * B) {
        const uint64_t k = prefix_key(r);
        if (k) inflight.insert(k);
      }
  if (cfg_.embed_first) {
    // embedding requests ahead of generation prompts, arrival order kept within each class;
    // preempted sequences and prompts already passed over embed_first_max_wait times keep
    // their place ahead of the embeds
    const int32_t max_wait = cfg_.embed_first_max_wait;
    auto ahead = [max_wait](const Sequence* s) {
      return !s->embed && (s->preempted || s->embed_passed >= max_wait);
    };
    auto it = std::stable_partition(waiting_.begin(), waiting_.end(), ahead);
    auto emb_end = std::stable_partition(it, waiting_.end(), [](const Sequence* s) { return s->embed; });
    if (it != emb_end)  // embeds went ahead of these prompts this step
      for (auto p = emb_end; p != waiting_.end(); ++p) ++(*p)->embed_passed;
  }
  // same-step sharing: prefix key -> the entry of this step that computes those blocks
  std::unordered_map<uint64_t, size_t> key_entry;
  if (dedup && cfg_.same_step_prefix)
    for (size_t i = 0; i < last_plan_.size(); ++i) {
      const Planned& p = last_plan_[i];
      if (p.spec || p.s->embed || p.s->num_computed >= 2 * B) continue;
      const uint64_t k = prefix_key(p.s);
      if (k) key_entry.emplace(k, i);
    }
  std::vector<Sequence*> deferred;
  while (!waiting_.empty() && (int32_t)last_plan_.size() < cfg_.max_num_seqs &&
         (int32_t)running_.size() < cfg_.max_num_seqs && tok_budget > 0 && prefill_budget > 0) {
    Sequence* s = waiting_.front();
    const uint64_t key = (dedup && !s->embed && s->blocks.empty()) ? prefix_key(s) : 0;
    size_t share_from = SIZE_MAX;
    if (key && inflight.count(key) && s->defer_count < cfg_.max_prefix_defer) {
      // join the step when the other sequence's chunk covers a full block of the common prefix
      const auto ke = key_entry.find(key);
      if (ke != key_entry.end()) {
        const Planned& e = last_plan_[ke->second];
        if (shareable_blocks(s, e.s, e.s->num_computed + e.n, B) > 0) share_from = ke->second;
      }
      if (share_from == SIZE_MAX) {
        waiting_.pop_front();
        ++s->defer_count;
        ++stat_prefix_defers_;
        deferred.push_back(s);
        continue;
      }
    }
    // a span request without enough free span slots waits (the requests behind it do not)
    if (s->span_slots.empty() && s->spans.size() > span_free_.size()) {
      waiting_.pop_front();
      deferred.push_back(s);
      continue;
    }
    if (s->embed && s->embed_slot < 0) {
      if (embed_free_.empty()) break;  // every pooling row is in use: wait
      s->embed_slot = embed_free_.back();
      embed_free_.pop_back();
    }
    // a penalised request without a free penalty slot waits (the requests behind it do not)
    if (s->needs_slot() && s->pen_slot < 0 && pen_free_.empty()) {
      waiting_.pop_front();
      deferred.push_back(s);
      continue;
    }
    // with scoring requests about, a request that will sample needs a row that no scoring chunk
    // of this step took (never binding otherwise: one row per planned sequence)
    if (budget_rows && !s->embed && !s->scoring() &&
        rows_reserved + score_rows_used >= cfg_.max_num_seqs)
      break;
    int32_t shared = 0;
    if (s->blocks.empty()) {
      match_prefix(s);
      if (share_from != SIZE_MAX) {
        const Planned& e = last_plan_[share_from];
        shared = share_same_step(s, e.s, e.s->num_computed + e.n);
      }
      if (shared == 0) match_partial(s);
    }
    // a request that is not admitted after all gives the shared blocks back: they hold KV only
    // once the step it would have joined has run
    auto unshare = [&]() {
      if (shared > 0) {
        free_seq(s, true);
        s->num_computed = 0;
      }
    };
    const int32_t pending = s->compute_len() - s->num_computed;
    int32_t n = std::min(pending, std::min(tok_budget, prefill_budget));
    if (s->scoring() && (n = fit_score_rows(s, n)) <= 0) {  // no row left: the requests behind it may fit
      unshare();
      waiting_.pop_front();
      deferred.push_back(s);
      continue;
    }
    const int32_t pairs = pair_need(s, n);
    const int32_t reps = rep_need(s, n);
    // never with an empty step: one backlog always fits either region
    if (pair_used + pairs > L.pair_cap || rep_used + reps > L.rep_cap) {
      unshare();
      waiting_.pop_front();
      deferred.push_back(s);
      continue;
    }
    const int32_t need =
        (s->num_computed + n + B - 1) / B - (int32_t)s->blocks.size();
    if ((need > 0 && bm_.num_free() - need < (running_.empty() ? 0 : watermark)) ||
        !ensure_blocks(s, s->num_computed + n)) {
      unshare();
      break;
    }
    waiting_.pop_front();
    count_cached(s);
    if (shared > 0) {
      // the alignment trim (2b) must leave the tokens whose blocks this entry reads
      Planned& e = last_plan_[share_from];
      e.keep = std::max(e.keep, s->num_computed - e.s->num_computed);
      ++stat_same_step_;
    }
    if (s->needs_slot() && s->pen_slot < 0) {
      s->pen_slot = pen_free_.back();
      pen_free_.pop_back();
      s->pen_fresh = true;
      s->rep_fresh = true;
    }
    if (s->span_slots.empty())
      for (size_t i = 0; i < s->spans.size(); ++i) {
        s->span_slots.push_back(span_free_.back());
        span_free_.pop_back();
      }
    pair_used += pairs;
    rep_used += reps;
    s->running = true;
    s->preempted = false;
    running_.push_back(s);
    last_plan_.push_back({s, n, samples(s, n)});
    if (key && s->num_computed < 2 * B) {  // its leading blocks are computed now
      inflight.insert(key);
      if (cfg_.same_step_prefix) key_entry.emplace(key, last_plan_.size() - 1);
    }
    score_rows_used += score_rows_of(s, s->num_computed, n);
    if (budget_rows && samples(s, n)) ++rows_reserved;
    tok_budget -= n;
    prefill_budget -= n;
  }
  waiting_.insert(waiting_.begin(), deferred.begin(), deferred.end());  // keep arrival order

  // 2b) align the step size (see SchedulerConfig::token_align): trim chunk tails,
  //     newest entries first, never below one token per entry
  if (cfg_.token_align > 0) {
    int32_t T = 0;
    for (const Planned& p : last_plan_) T += p.n;
    const int32_t r = T % cfg_.token_align;
    if (T > cfg_.token_align && r > 0 && r <= cfg_.align_slack) {
      int32_t cap = 0;
      for (const Planned& p : last_plan_) cap += (p.spec || !p.draft.empty()) ? 0 : std::max(0, p.n - p.keep);
      if (cap >= r) {
        int32_t left = r;
        for (size_t i = last_plan_.size(); i-- > 0 && left > 0;) {
          Planned& p = last_plan_[i];
          if (p.spec || !p.draft.empty()) continue;
          const int32_t cut = std::min(left, std::max(0, p.n - p.keep));
          p.n -= cut;
          left -= cut;
          p.sample = samples(p.s, p.n);
        }
        ++stat_aligned_steps_;
      }
    }
  }

  // 3) emit the step description
  int32_t* counts = buf + L.counts;
  int32_t* ids = buf + L.input_ids;
  int32_t* pos = buf + L.positions;
  int32_t* slots = buf + L.slots;
  int32_t* qs = buf + L.q_start;
  int32_t* ql = buf + L.q_len;
  int32_t* cl = buf + L.ctx_len;
  int32_t* lr = buf + L.logit_rows;
  int32_t* mc = buf + L.mask_class;
  int32_t* fc = buf + L.forced;
  int32_t* off = buf + L.offsets;
  float* temp = reinterpret_cast<float*>(buf + L.temperature);
  int32_t* tk = buf + L.top_k;
  int32_t* lpn = buf + L.lp_n;
  int32_t nlp = 0;
  float* tp = reinterpret_cast<float*>(buf + L.top_p);
  int32_t ntrunc = 0;
  int64_t* seeds = reinterpret_cast<int64_t*>(buf + L.seeds);
  int32_t* items = buf + L.items;
  int32_t* bt = buf + L.block_table;
  int32_t* er = buf + L.embed_rows;
  int32_t nembed = 0;
  // penalties: these regions are written only when a planned row is penalised and samples
  bool any_pen = false;
  for (const Planned& p : last_plan_) any_pen = any_pen || (p.sample && p.s->penalised());
  int32_t* psl = buf + L.pen_slot;
  int32_t* prs = buf + L.pen_reset;
  float* ppr = reinterpret_cast<float*>(buf + L.pen_presence);
  float* pfr = reinterpret_cast<float*>(buf + L.pen_frequency);
  int32_t* pst = buf + L.pair_start;
  int32_t* pnn = buf + L.pair_n;
  int32_t* ptk = buf + L.pair_tok;
  int32_t npen = 0, npair = 0;
  // logit_bias / min_p: these regions are written only when a planned sampling row is shaped
  bool any_shape = false;
  for (const Planned& p : last_plan_) any_shape = any_shape || (p.sample && p.s->shaped());
  int32_t* bst = buf + L.bias_start;
  int32_t* bnn = buf + L.bias_n;
  float* bmp = reinterpret_cast<float*>(buf + L.minp);
  float* bln = reinterpret_cast<float*>(buf + L.ln_minp);
  int32_t* btk = buf + L.bias_tok;
  float* bvl = reinterpret_cast<float*>(buf + L.bias_val);
  int32_t nbias = 0;
  // repetition penalty: these regions are written only when a planned sampling row carries one
  // and the grammar leaves it a choice, i.e. exactly in the steps that set bit 1 of counts[9]
  bool any_rep = false;
  for (const Planned& p : last_plan_) {
    if (!p.sample || p.spec || !p.s->repetitive() || p.s->pen_slot < 0) continue;
    int32_t cls = -1, forced = -1;
    if (p.s->grammar) p.s->grammar->next(&cls, &forced);
    any_rep = any_rep || forced < 0;
  }
  int32_t* rsl = buf + L.rep_slot;
  int32_t* rrs = buf + L.rep_reset;
  float* rrr = reinterpret_cast<float*>(buf + L.rep_r);
  float* rir = reinterpret_cast<float*>(buf + L.rep_inv_r);
  int32_t* rst = buf + L.rep_start;
  int32_t* rnn = buf + L.rep_n;
  int32_t* rtk = buf + L.rep_tok;
  int32_t nrep = 0, nreptok = 0;
  // prompt scoring: the target region is written only when a planned entry owns scoring rows
  bool any_score = false;
  for (Planned& p : last_plan_) {
    p.score_rows = score_rows_of(p.s, p.s->num_computed, p.n);
    any_score = any_score || p.score_rows > 0;
  }
  int32_t* stg = buf + L.score_target;
  const int32_t tpw = 16 / std::max(1, cfg_.gqa_group);

  int32_t* cpl = buf + L.copy_list;
  int32_t ncopy = 0;
  // draft steps: the run regions are written only when a planned entry owns draft rows
  bool any_draft = false;
  for (const Planned& p : last_plan_) any_draft = any_draft || !p.draft.empty();
  int32_t* rfi = buf + L.run_first;
  int32_t* rln = buf + L.run_len;

  // span pooling: the segment region is written only when a span has rows in the step
  int32_t* sps = buf + L.span_segs;
  int32_t nspan = 0;

  int32_t T = 0, ns = 0, nsamp = 0, nit = 0, nparted = 0, pslot = 0;
  // decode partition size: with few decode rows, 256-key flash-decoding partitions
  // give the attention launch more workgroups. 128-key partitions lose more to the
  // extra partial merges than they gain (profiles/r1_attention_small_batch.jsonl:
  // 8 rows x ctx 1000: 13.8 us at 128, 10.9 at 256, 11.2 at 512; 16 rows: 24.2 /
  // 17.7 / 18.5). The item list must still fit max_items.
  // prefill item width: the 4-wave LDS-staged items (att_qcols columns) only pay when
  // the step has enough prefill work to fill the chip with 4x fewer items (tools/
  // attn_bench.py --scan: 8 x 512 tokens 50.8 us wide vs 68.8 narrow, 8 x 128 14.8 vs
  // 13.8, a single 512-token chunk 19.5 vs 12.7)
  // (a single long chunk gains nothing: its causal imbalance makes the longest item the
  // critical path, 4x longer per workgroup with the wide items; --scan pf2048: 79.6 vs 79.0)
  int64_t prefill_tokens = 0;
  int32_t prefill_seqs = 0;
  for (const Planned& p : last_plan_)
    if (p.n > tpw) {
      prefill_tokens += p.n;
      ++prefill_seqs;
    }
  const bool wide = prefill_tokens >= cfg_.att_wide_min_tokens && prefill_seqs >= 2;
  const int32_t qcols = wide ? std::max(32, cfg_.att_qcols) : 32;
  const int32_t qtile = std::max(1, qcols / std::max(1, cfg_.gqa_group));
  int32_t psz = 512;
  if (cfg_.split_decode) {
    int64_t parts512 = 0, parts256 = 0, nprefill = 0;
    for (const Planned& p : last_plan_) {
      const int32_t c = p.s->num_computed + p.n;
      if (p.n <= tpw) {
        parts512 += std::max(1, (c + 511) / 512);
        parts256 += std::max(1, (c + 255) / 256);
      } else {
        nprefill += (p.n + qtile - 1) / qtile;  // exactly the q-tiles emitted below
      }
    }
    const int64_t kv = std::max(1, cfg_.kv_heads), target = 512;
    if (parts512 * kv < target && nprefill + parts256 <= L.max_items) psz = 256;
    int32_t t_step = 0;
    for (const Planned& p : last_plan_) t_step += p.n;
    if (cfg_.small_step_part > 0 && t_step <= cfg_.small_step_tokens && parts512 * kv < target)
      psz = std::max(psz, cfg_.small_step_part);
    const int32_t dpt = t_step > cfg_.small_step_tokens ? cfg_.decode_part_target : cfg_.small_step_target;
    if (dpt > 0 && (t_step > cfg_.small_step_tokens || cfg_.small_step_part > 0)) {
      // one balanced round of workgroups instead of 512-key parts + short remainders
      int64_t ndec = 0, maxc = 0, sumc = 0;
      for (const Planned& p : last_plan_)
        if (p.n <= tpw) {
          ++ndec;
          const int64_t c = p.s->num_computed + p.n;
          maxc = std::max<int64_t>(maxc, c);
          sumc += c;
        }
      if (ndec > 0) {
        const int64_t tgt = dpt;
        // the balanced share of all decode keys per (partition, KV head) workgroup: no
        // partition is longer than that, so one long row among many short ones is split
        // instead of becoming the one serial work item of every layer (uniform contexts are
        // unaffected: there the share is at least the longest context / the parts below)
        const int64_t share = ((sumc * kv + tgt - 1) / tgt + 31) / 32 * 32;
        int64_t cand;
        if (ndec * kv >= tgt) {
          cand = std::max<int64_t>(32, std::min(maxc, std::max<int64_t>(share, 128)));
        } else {
          const int64_t np = (tgt + ndec * kv - 1) / (ndec * kv);
          cand = std::max<int64_t>(128, std::min(((maxc + np - 1) / np + 31) / 32 * 32, share));
        }
        int64_t parts = 0;
        for (const Planned& p : last_plan_)
          if (p.n <= tpw) parts += std::max<int64_t>(1, (p.s->num_computed + p.n + cand - 1) / cand);
        if (nprefill + parts <= L.max_items) psz = (int32_t)cand;
      }
    }
  }
  buf[L.part_size] = psz;

  // prefill (q-split) tiles go first in the item list, heaviest (most keys) first across
  // all chunks, then the decode items, longest partition first: the attention grid strides
  // over the items in this order, so the long items start first and the short ones fill in
  // behind them
  struct ItemCost {
    int32_t keys, a, b, c, d;
  };
  std::vector<ItemCost> pre, dec;
  for (size_t si = 0; si < last_plan_.size(); ++si) {
    const int32_t n = last_plan_[si].n;
    if (n <= tpw) continue;
    const int32_t c0 = last_plan_[si].s->num_computed;
    for (int32_t qb = ((n - 1) / qtile) * qtile; qb >= 0; qb -= qtile) {
      const int32_t nq = std::min(qtile, n - qb);
      pre.push_back({c0 + qb + nq, (int32_t)si, qb, nq | (1 << 20), 0});
    }
  }
  const int64_t plan_id = next_plan_id_;
  for (size_t pi = 0; pi < last_plan_.size(); ++pi) {
    Planned& p = last_plan_[pi];
    Sequence* s = p.s;
    const int32_t n = p.n, c0 = s->num_computed, ctx = c0 + n;
    qs[ns] = T;
    ql[ns] = n;
    cl[ns] = ctx;
    const int32_t erow = s->embed_slot >= 0 ? s->embed_slot : L.max_seqs;
    for (int32_t j = 0; j < n; ++j) {
      const int32_t ppos = c0 + j;
      // speculative entry: the pending token comes from the in-flight step's sampled row
      // src_idx (the device patches -(src_idx + 1) before the embedding lookup)
      const int32_t nreal = n - (int32_t)p.draft.size();  // the tokens behind them are the draft
      ids[T + j] = p.spec ? (j == 0 ? -(p.src_idx + 1) : p.run[j - 1])
                          : (j < nreal ? s->tokens[ppos] : p.draft[j - nreal]);
      pos[T + j] = ppos;
      slots[T + j] = s->blocks[ppos / B] * B + ppos % B;
      // last-token pooling: only the prompt's final token feeds the request's pooling row
      er[T + j] = (s->embed_last && ppos + 1 != (int32_t)s->tokens.size()) ? L.max_seqs : erow;
    }
    if (s->embed_slot >= 0) nembed += n;
    // the chunk's rows inside each span: one segment for the span's slot, re-initialising it
    // when the rows start at the span's first token
    for (size_t i = 0; i < s->span_slots.size(); ++i) {
      const int32_t lo = std::max(s->spans[i].first, c0), hi = std::min(s->spans[i].second, ctx);
      if (lo >= hi) continue;
      if (nspan >= L.span_slots || buf_words < L.span_total)  // one segment per held slot at most
        throw std::logic_error("scheduler: span segments overflow the step buffer");
      int32_t* q = sps + 4 * nspan++;
      q[0] = T + (lo - c0);
      q[1] = hi - lo;
      q[2] = s->span_slots[i];
      q[3] = lo == s->spans[i].first ? 1 : 0;
    }
    const int32_t nb = (ctx + B - 1) / B;
    std::memcpy(bt + (size_t)ns * L.max_blocks, s->blocks.data(), sizeof(int32_t) * nb);
    if (s->copy_j > 0) {
      // the head of its first own block comes from a cached one: the step's first kernel copies
      // it. The reference on the donor is given back now that the copy is listed -- no block is
      // allocated between here and the step's launch, and later steps run behind it.
      if (!copies_ok_ || ncopy >= L.max_seqs)
        throw std::logic_error("scheduler: a partial-block copy without room in the step buffer");
      cpl[3 * ncopy] = s->copy_src;
      cpl[3 * ncopy + 1] = s->copy_dst;
      cpl[3 * ncopy + 2] = s->copy_j;
      ++ncopy;
      drop_copy(s);
    }
    // a draft entry owns 1 + k rows, one per token from the last real one on: row r samples the
    // token at position ctx - k + r from the logits of the token in front of it
    const int32_t kd = (int32_t)p.draft.size();
    const int32_t run0 = nsamp;
    for (int32_t r = 0; p.sample && r <= kd; ++r) {
      if (nsamp >= L.max_seqs)  // the planning above budgeted the rows
        throw std::logic_error("scheduler: sampling rows overflow max_num_seqs");
      lr[nsamp] = T + n - 1 - kd + r;
      int32_t cls = -1, forced = -1;
      if (kd > 0) {
        cls = p.row_gram[r].first;
        forced = p.row_gram[r].second;
      } else if (s->grammar) {
        if (p.spec) s->grammar->next_at(p.cur, &cls, &forced);
        else s->grammar->next(&cls, &forced);
      }
      mc[nsamp] = cls;
      fc[nsamp] = forced;
      off[nsamp] = ctx - kd + r;  // the sampled token's position (= tokens.size() for a known row)
      if (r == 0) {
        s->pend_plan = plan_id;
        s->pend_idx = nsamp;
      }
      if (any_draft) {
        rfi[nsamp] = run0;
        rln[nsamp] = kd + 1;
      }
      temp[nsamp] = s->temperature;
      tk[nsamp] = s->top_k;
      tp[nsamp] = s->top_p;
      if (s->temperature > 0.f && (s->top_k > 0 || s->top_p < 1.f) && forced < 0) ++ntrunc;
      seeds[nsamp] = s->seed;
      lpn[nsamp] = s->logprobs;
      if (s->logprobs >= 0) ++nlp;
      if (any_score) stg[nsamp] = -1;
      if (any_pen) {
        psl[nsamp] = -1;
        prs[nsamp] = 0;
        ppr[nsamp] = pfr[nsamp] = 0.f;
        pst[nsamp] = npair;
        pnn[nsamp] = 0;
        // a forced row is not penalised and the device reads nothing for it: its backlog
        // (and the slot's reset) waits for the row's next free sampling step
        if (s->penalised() && s->pen_slot >= 0 && forced < 0 && !p.spec) {
          const int32_t from = s->prompt_len + s->pen_synced, upto = (int32_t)s->tokens.size();
          if (npair + (upto - from) > L.pair_cap)  // the planning above reserved this room
            throw std::logic_error("scheduler: penalty pair region overflows");
          psl[nsamp] = s->pen_slot;
          prs[nsamp] = s->pen_fresh ? 1 : 0;
          ppr[nsamp] = s->presence_penalty;
          pfr[nsamp] = s->frequency_penalty;
          pnn[nsamp] = upto - from;
          std::memcpy(ptk + npair, s->tokens.data() + from, sizeof(int32_t) * (size_t)(upto - from));
          npair += upto - from;
          s->pen_synced = upto - s->prompt_len;
          s->pen_fresh = false;
          ++npen;
        }
      }
      if (any_rep) {
        rsl[nsamp] = -1;
        rrs[nsamp] = 0;
        rrr[nsamp] = rir[nsamp] = 1.f;
        rst[nsamp] = nreptok;
        rnn[nsamp] = 0;
        // as above: a forced row is not touched and the device reads nothing for it; its
        // backlog (the forced token included, once known) goes with the next free sampling row
        if (s->repetitive() && s->pen_slot >= 0 && forced < 0 && !p.spec) {
          const int32_t from = s->rep_synced, upto = (int32_t)s->tokens.size();
          if (nreptok + (upto - from) > L.rep_cap)  // the planning above reserved this room
            throw std::logic_error("scheduler: repetition token region overflows");
          rsl[nsamp] = s->pen_slot;
          rrs[nsamp] = s->rep_fresh ? 1 : 0;
          rrr[nsamp] = s->repetition_penalty;
          rir[nsamp] = s->inv_repetition_penalty;
          rnn[nsamp] = upto - from;
          std::memcpy(rtk + nreptok, s->tokens.data() + from, sizeof(int32_t) * (size_t)(upto - from));
          nreptok += upto - from;
          s->rep_synced = upto;
          s->rep_fresh = false;
          ++nrep;
        }
      }
      if (any_shape) {
        // stateless: every sampling row of a shaped sequence carries the request's list and
        // min_p -- speculative rows and rows after a preemption alike; the device skips a
        // forced row by itself
        const int32_t nb = s->shaped() ? (int32_t)s->logit_bias.size() : 0;
        if (nbias + nb > L.bias_cap)  // max_seqs rows of at most LOGIT_BIAS_MAX entries each
          throw std::logic_error("scheduler: logit_bias region overflows");
        bst[nsamp] = nbias;
        bnn[nsamp] = nb;
        bmp[nsamp] = s->shaped() ? s->min_p : 0.f;
        bln[nsamp] = s->shaped() ? s->ln_min_p : 0.f;
        for (int32_t j = 0; j < nb; ++j) {
          btk[nbias + j] = s->logit_bias[j].first;
          bvl[nbias + j] = s->logit_bias[j].second;
        }
        nbias += nb;
      }
      ++nsamp;
    }
    // scoring rows: one per position >= score_from - 1 of the entry, each on that token's logit
    // row with the next prompt token as its target. For every other pass the row is inert: forced
    // to the target (the sampler emits it, the penalty / shaping / logprob passes skip it or write
    // a record nobody reads), greedy, no mask class, no slot, no bias.
    for (int32_t j = n - p.score_rows; j < n; ++j) {
      if (nsamp >= L.max_seqs)  // the planning above budgeted the rows
        throw std::logic_error("scheduler: scoring rows overflow max_num_seqs");
      const int32_t target = s->tokens[c0 + j + 1];
      lr[nsamp] = T + j;
      mc[nsamp] = -1;
      fc[nsamp] = target;
      off[nsamp] = c0 + j + 1;
      temp[nsamp] = 0.f;
      tk[nsamp] = 0;
      tp[nsamp] = 1.f;
      seeds[nsamp] = 0;
      lpn[nsamp] = s->score_n;
      stg[nsamp] = target;
      if (any_pen) {
        psl[nsamp] = -1;
        prs[nsamp] = 0;
        ppr[nsamp] = pfr[nsamp] = 0.f;
        pst[nsamp] = npair;
        pnn[nsamp] = 0;
      }
      if (any_rep) {
        rsl[nsamp] = -1;
        rrs[nsamp] = 0;
        rrr[nsamp] = rir[nsamp] = 1.f;
        rst[nsamp] = nreptok;
        rnn[nsamp] = 0;
      }
      if (any_shape) {
        bst[nsamp] = nbias;
        bnn[nsamp] = 0;
        bmp[nsamp] = bln[nsamp] = 0.f;
      }
      if (any_draft) {
        rfi[nsamp] = nsamp;
        rln[nsamp] = 1;
      }
      ++nsamp;
    }
    // attention work items (mirrors pilottai_amd/ops/attn_meta.py)
    if (n <= tpw) {
      const int32_t nparts = cfg_.split_decode ? std::max(1, (ctx + psz - 1) / psz) : 1;
      if (nparts > 1) {
        for (int32_t q = 0; q < nparts; ++q)
          dec.push_back({std::min(psz, ctx - q * psz), ns, 0, n | (q << 8) | (nparts << 20), pslot + q});
        ++nparted;  // merged in-kernel by the last partition (attention.hip)
        pslot += nparts;
      } else {
        dec.push_back({ctx, ns, 0, n | (1 << 20), 0});
      }
    }
    s->num_computed = ctx;
    p.end = ctx;
    ++s->inflight;
    if (p.spec) {
      s->spec_plan = plan_id;
      s->spec_entry = (int32_t)pi;
    }
    T += n;
    ++ns;
  }
  // split the longest wide prefill items (prefill_split_keys; slots after the decode partitions'
  // -- 8 partial slots per partition -- within the part_o / part_ml workspace of max_items slots)
  int32_t t_step_all = 0;
  for (const Planned& p : last_plan_) t_step_all += p.n;
  const int32_t G = std::max(1, cfg_.gqa_group);
  if (cfg_.prefill_split_keys > 0 && qtile * G > 32 && t_step_all > cfg_.small_step_tokens) {
    std::vector<ItemCost> split;
    int64_t n_items_total = (int64_t)pre.size() + (int64_t)dec.size();
    for (const ItemCost& c : pre) {
      const int32_t nq = c.c & 0xff;
      int32_t np = std::min<int32_t>(4, c.keys / cfg_.prefill_split_keys);
      if (nq > 32 / G && np >= 2 && pslot + 8 * np <= L.max_items && n_items_total + np - 1 <= L.max_items) {
        const int32_t tiles = (c.keys + 31) / 32;
        const int32_t per = ((tiles + np - 1) / np) * 32;
        for (int32_t q = 0; q < np; ++q)
          split.push_back({per, c.a, c.b, nq | (q << 8) | (np << 20), pslot + 8 * q});
        pslot += 8 * np;
        n_items_total += np - 1;
      } else {
        split.push_back(c);
      }
    }
    pre.swap(split);
  }
  std::stable_sort(pre.begin(), pre.end(), [](const ItemCost& x, const ItemCost& y) { return x.keys > y.keys; });
  for (const ItemCost& c : pre) {
    int32_t* it = items + 4 * nit++;
    it[0] = c.a; it[1] = c.b; it[2] = c.c; it[3] = c.d;
  }
  std::stable_sort(dec.begin(), dec.end(), [](const ItemCost& x, const ItemCost& y) { return x.keys > y.keys; });
  for (const ItemCost& c : dec) {
    int32_t* it = items + 4 * nit++;
    it[0] = c.a; it[1] = c.b; it[2] = c.c; it[3] = c.d;
  }
  // padding: tokens write no KV, sample rows are greedy on row 0
  for (int32_t t = T; t < L.max_tokens; ++t) {
    ids[t] = 0;
    pos[t] = 0;
    slots[t] = -1;
    er[t] = L.max_seqs;
  }
  for (int32_t r = nsamp; r < L.max_seqs; ++r) {
    lr[r] = 0;
    mc[r] = -1;
    fc[r] = -1;
    off[r] = 0;
    temp[r] = 0.f;
    tk[r] = 0;
    tp[r] = 1.f;
    seeds[r] = 0;
    lpn[r] = -1;
  }
  if (any_pen)
    for (int32_t r = nsamp; r < L.max_seqs; ++r) {
      psl[r] = -1;
      prs[r] = 0;
      ppr[r] = pfr[r] = 0.f;
      pst[r] = npair;
      pnn[r] = 0;
    }
  if (any_rep)
    for (int32_t r = nsamp; r < L.max_seqs; ++r) {
      rsl[r] = -1;
      rrs[r] = 0;
      rrr[r] = rir[r] = 1.f;
      rst[r] = nreptok;
      rnn[r] = 0;
    }
  if (any_shape)
    for (int32_t r = nsamp; r < L.max_seqs; ++r) {
      bst[r] = nbias;
      bnn[r] = 0;
      bmp[r] = bln[r] = 0.f;
    }
  if (any_score)
    for (int32_t r = nsamp; r < L.max_seqs; ++r) stg[r] = -1;
  for (int32_t r = ns; r < L.max_seqs; ++r) {
    qs[r] = T;
    ql[r] = 0;
    cl[r] = 0;
  }
  counts[0] = T;
  counts[1] = ns;
  counts[2] = nsamp;
  counts[3] = nit;
  counts[4] = nparted;
  counts[5] = pslot;
  counts[6] = ntrunc;  // rows that need the top-k / top-p threshold pass
  counts[7] = nembed;  // tokens whose hidden states are pooled (embedding requests)
  counts[8] = nlp;     // rows that need the log-probability pass
  counts[9] = npen > 0 ? 1 : 0;  // the step has a penalised sampling row (penalty pass)
  // ... a row with a repetition penalty (repetition pass): bit 1, the rep_tok words in use above it
  if (nrep > 0) counts[9] |= 2 | (nreptok << 2);
  if (any_score) counts[9] |= COUNTS9_SCORE_BIT;  // ... scoring rows (scoring pass): bit 30
  if (any_draft) {  // ... draft rows (the acceptance pass instead of the sampler's final merge): bit 29
    counts[9] |= COUNTS9_SPEC_BIT;
    for (int32_t r = nsamp; r < L.max_seqs; ++r) {
      rfi[r] = r;
      rln[r] = 1;
    }
    ++stat_draft_steps_;
  }
  if (nspan > 0) {  // ... span segments (span pooling pass): bit 28
    counts[9] |= COUNTS9_SPAN_BIT;
    buf[L.span_n] = nspan;
  }
  counts[10] = npair;            // words of the pair region those rows use
  counts[11] = any_shape ? 1 + nbias : 0;  // a shaped sampling row (logit_bias / min_p pass) + its bias words
  if (nit > L.max_items)  // by construction (psz guard above, max_items sizing) this cannot happen
    throw std::logic_error("scheduler: attention item list overflows max_items");
  buf[L.n_items] = nit;
  buf[L.n_copies] = ncopy;
  if (T > 0) {
    ++stat_steps_;
    plans_.push_back(Plan{next_plan_id_++, std::move(last_plan_)});
  }
  last_plan_.clear();
  return T;
}

bool Scheduler::predict(Sequence* s, Planned& e) const {
  // Mirrors commit() for the pending token (any token the row's mask allows, and for
  // string / list bodies one that neither closes nor separates; no EOS for free text):
  // false when the row could finish there, so it waits for the commit instead.
  const int32_t ng = s->num_generated + 1;
  const int32_t ntok = (int32_t)s->tokens.size() + 1;
  if (ng >= s->max_tokens || ntok >= cfg_.max_model_len) return false;
  // penalty counts are sent as known tokens: a penalised row waits for its commit
  if (s->needs_slot()) return false;
  // a drafting request's step may commit several tokens: nothing to continue from before that
  if (s->drafting()) return false;
  e.run.clear();
  if (!s->grammar) return true;
  const Grammar& g = *s->grammar;
  Grammar::Cursor c = g.cursor();
  int32_t cls, forced;
  g.next_at(c, &cls, &forced);
  g.advance_at(c, forced >= 0 ? forced : Grammar::GENERIC);
  if (g.done_at(c)) return false;
  const int32_t room = std::min(s->max_tokens - ng, cfg_.max_model_len - ntok);
  int32_t k = 0;
  while (k < room && !g.done_at(c)) {
    g.next_at(c, &cls, &forced);
    if (forced < 0) break;
    e.run.push_back(forced);
    g.advance_at(c, forced);
    ++k;
  }
  if (g.done_at(c) || ng + k >= s->max_tokens || ntok + k >= cfg_.max_model_len) return false;
  e.cur = c;
  return true;
}

SeqOutput Scheduler::finish(Sequence* s, int32_t reason, double now) {
  SeqOutput o;
  o.id = s->id;
  o.tokens.assign(s->tokens.begin() + s->prompt_len, s->tokens.end());
  o.finish_reason = reason;
  o.prompt_len = s->prompt_len;
  o.cached_prompt_tokens = std::max(0, s->cached_prompt_tokens);
  o.num_sampled = s->num_sampled;
  o.num_forced = s->num_forced;
  o.t_first_token = s->t_first_token;
  o.t_finish = now;
  o.embed_slot = s->embed_slot;  // FINISH_EMBED: read it; otherwise: clear it before reuse
  o.logprobs = s->logprobs;
  o.lp_records = std::move(s->lp_records);
  s->lp_records.clear();
  if (s->scoring()) --score_live_;
  if (s->drafting()) {
    --draft_live_;
    o.draft_proposed = s->draft_proposed;
    o.draft_accepted = s->draft_accepted;
    o.prediction_matched = s->prediction_matched;
    draft_counts_.push_back({s->id, s->draft_proposed, s->draft_accepted, s->prediction_matched});
    s->draft_len = 0;  // counted once
  }
  if (!s->span_slots.empty()) {
    // a caller that never takes the records loses the oldest instead of growing the list
    if (span_finishes_.size() >= kMaxSpanFinishes) span_finishes_.erase(span_finishes_.begin());
    span_finishes_.emplace_back(s->id, s->span_slots);
  }
  o.score_from = s->score_from;
  o.score_n = s->score_n;
  o.score_records = std::move(s->score_records);
  s->score_records.clear();
  if (s->pen_slot >= 0) {  // recycled by the next holder's reset flag
    pen_free_.push_back(s->pen_slot);
    s->pen_slot = -1;
  }
  free_seq(s);
  s->running = false;
  return o;
}

// One sampled token enters the sequence: the grammar advances, the stops and limits are checked,
// and the grammar's next forced run is appended (jump-forward). `lp`: the token's record, if the
// step computed one.
int32_t Scheduler::apply_token(Sequence* s, int32_t tok, const LogprobRecord* lp) {
  s->tokens.push_back(tok);
  ++s->num_generated;
  ++s->num_sampled;
  if (s->logprobs >= 0) {
    if (lp) {
      s->lp_records.push_back(*lp);
    } else {  // the step computed no records: keep the alignment with the tokens
      LogprobRecord r = forced_record(tok, 0);
      r.lp = NAN;
      s->lp_records.push_back(r);
    }
  }
  int32_t fin = NOT_FINISHED;
  if (s->grammar) {
    s->grammar->advance(tok);
    if (s->grammar->done()) fin = FINISH_STOP;
  } else if (!s->ignore_eos) {
    if (std::find(cfg_.eos_ids.begin(), cfg_.eos_ids.end(), tok) != cfg_.eos_ids.end() ||
        std::find(s->stop_ids.begin(), s->stop_ids.end(), tok) != s->stop_ids.end())
      fin = FINISH_STOP;
  }
  if (fin == NOT_FINISHED && s->num_generated >= s->max_tokens) fin = FINISH_LENGTH;
  if (fin == NOT_FINISHED && (int32_t)s->tokens.size() >= cfg_.max_model_len) fin = FINISH_LENGTH;
  if (fin == NOT_FINISHED && s->grammar) {
    const int32_t room = std::min(s->max_tokens - s->num_generated,
                                  cfg_.max_model_len - (int32_t)s->tokens.size());
    const int32_t k = s->grammar->take_forced_run(s->tokens, room);
    s->num_generated += k;
    s->num_forced += k;
    if (s->logprobs >= 0)
      for (int32_t j = k; j > 0; --j)
        s->lp_records.push_back(forced_record(s->tokens[s->tokens.size() - j], s->logprobs));
    if (s->grammar->done()) fin = FINISH_STOP;
    else if (s->num_generated >= s->max_tokens) fin = FINISH_LENGTH;
  }
  return fin;
}

std::vector<SeqOutput> Scheduler::commit(const int32_t* sampled, int32_t n, const LogprobRecord* lp,
                                         const ScoreRecord* sc, const int32_t* accept_len) {
  std::vector<SeqOutput> outs;
  if (plans_.empty()) return outs;
  Plan plan = std::move(plans_.front());
  plans_.pop_front();
  Plan* next = plans_.empty() ? nullptr : &plans_.front();  // the step still in flight, if any
  const double now = now_seconds();
  for (const Planned& p : plan.rows) --p.s->inflight;
  int32_t idx = 0;
  std::vector<Sequence*> done;
  for (const Planned& p : plan.rows) {
    Sequence* s = p.s;
    int32_t tok = -1;
    if (s->scoring()) {
      // the entry's rows hold its records; their sampled tokens (the forced targets) are ignored
      if (idx + p.score_rows > n) break;
      const int32_t first = idx;
      idx += p.score_rows;
      if (s->done || s->abort_pending) continue;
      for (int32_t j = 0; j < p.score_rows; ++j) {
        if (sc) {
          s->score_records.push_back(sc[first + j]);
        } else {  // the step computed no records: keep the alignment with the positions
          ScoreRecord r;
          r.lp = NAN;
          r.rank = 0;
          for (int32_t i = 0; i < LOGPROB_TOP; ++i) {
            r.ids[i] = -1;
            r.lps[i] = -INFINITY;
          }
          s->score_records.push_back(r);
        }
      }
      if (p.score_rows > 0 && s->t_first_token < 0) s->t_first_token = now;
      register_full_blocks(s);
      if (p.end == s->compute_len()) {
        outs.push_back(finish(s, FINISH_SCORE, now));
        done.push_back(s);
      }
      continue;
    }
    int32_t row0 = -1;
    if (p.sample) {
      if (idx >= n) break;
      row0 = idx;
      tok = sampled[idx++];
      idx += (int32_t)p.draft.size();  // a draft entry's other rows
    }
    if (p.voided || s->done || s->abort_pending) continue;
    if (!p.sample) {
      register_full_blocks(s);
      if (s->embed && p.end == (int32_t)s->tokens.size()) {
        outs.push_back(finish(s, FINISH_EMBED, now));  // frees the row: the caller reads it first
        done.push_back(s);
      }
      continue;
    }
    const int32_t before = (int32_t)s->tokens.size();
    if (s->t_first_token < 0) s->t_first_token = now;
    int32_t fin = NOT_FINISHED;
    if (p.draft.empty()) {
      fin = apply_token(s, tok, lp ? lp + row0 : nullptr);
      follow_prediction(s, (size_t)before);
    } else {
      // a run of 1 + k rows: y_0 .. y_a are committed one by one. The rows behind y_0 were
      // planned on a copy of the grammar cursor, so the forced run a token's commit appends
      // (jump-forward) is the run's own next tokens: those are skipped, not appended twice.
      const int32_t k = (int32_t)p.draft.size();
      const int32_t* ys = sampled + row0;
      int32_t a = accept_len ? std::max(0, std::min(accept_len[row0] - 1, k)) : 0;
      if (row0 + k >= n) a = 0;  // fewer rows than planned: trust the first only
      for (int32_t j = 0; j < a; ++j)  // the device's count, never past the first host mismatch
        if (ys[j] != p.draft[j]) a = j;
      int32_t j = 0;
      while (j <= a && fin == NOT_FINISHED) {
        const size_t at = s->tokens.size();
        fin = apply_token(s, ys[j], nullptr);
        const int32_t m = (int32_t)(s->tokens.size() - at) - 1;  // forced tokens behind y_j
        const int32_t use = std::min(m, a - j);
        if (!std::equal(ys + j + 1, ys + j + 1 + use, s->tokens.begin() + at + 1)) {
          a = j;  // cannot happen (same automaton, same tokens): keep what the grammar says
          break;
        }
        j += 1 + use;
      }
      // KV is valid for the run's inputs up to the last confirmed draft token; everything the
      // run wrote behind that is dead and is overwritten when those positions are computed
      // (a stop inside the run: every token committed before it was a confirmed draft token)
      const int32_t confirmed = std::min(a, (int32_t)s->tokens.size() - before);
      s->num_computed = std::min(p.end - k + confirmed, (int32_t)s->tokens.size() - 1);
      s->draft_accepted += confirmed;
      stat_draft_accepted_ += confirmed;
      if (confirmed == k) ++stat_draft_full_;
      const int32_t followed = follow_prediction(s, (size_t)before);
      s->prediction_matched += p.draft_pred ? followed : confirmed;
    }
    // check the speculative continuation the in-flight step holds for this row
    if (next && s->spec_plan == next->id) {
      Planned& e = next->rows[s->spec_entry];
      bool ok = fin == NOT_FINISHED &&
                (int32_t)s->tokens.size() == before + 1 + (int32_t)e.run.size() &&
                std::equal(e.run.begin(), e.run.end(), s->tokens.begin() + before + 1);
      if (ok && s->grammar) ok = s->grammar->cursor() == e.cur;
      if (!ok) {
        // drop the entry: its sample is discarded, and the row resumes from the
        // sampled token (recomputed next step: same KV, written again)
        e.voided = true;
        ++stat_spec_voided_;
        s->num_computed = before;
        s->pend_plan = -1;
      }
      s->spec_plan = -1;
    }
    register_full_blocks(s);
    if (fin != NOT_FINISHED) {
      outs.push_back(finish(s, fin, now));
      done.push_back(s);
    }
  }
  // rows aborted while listed by an in-flight step finish once no step lists them
  for (size_t i = 0; i < abort_wait_.size();) {
    Sequence* s = abort_wait_[i];
    if (s->inflight > 0) {
      ++i;
      continue;
    }
    aborted_.push_back(finish(s, FINISH_ABORT, now));
    done.push_back(s);
    abort_wait_.erase(abort_wait_.begin() + i);
  }
  if (!done.empty()) {
    running_.erase(std::remove_if(running_.begin(), running_.end(),
                                  [](Sequence* s) { return !s->running; }),
                   running_.end());
    for (Sequence* s : done) {
      s->done = true;
      auto it = seqs_.find(s->id);
      if (it == seqs_.end()) continue;
      if (s->inflight > 0) zombies_.push_back(std::move(it->second));  // a voided entry still lists it
      seqs_.erase(it);
    }
  }
  zombies_.erase(std::remove_if(zombies_.begin(), zombies_.end(),
                                [](const std::unique_ptr<Sequence>& z) { return z->inflight == 0; }),
                 zombies_.end());
  return outs;
}

bool Scheduler::abort(int64_t id) {
  auto it = seqs_.find(id);
  if (it == seqs_.end()) return false;
  Sequence* s = it->second.get();
  if (s->inflight > 0) {  // listed by an uncommitted step: finished at that step's commit
    if (!s->abort_pending) {
      s->abort_pending = true;
      abort_wait_.push_back(s);
    }
    return true;
  }
  waiting_.erase(std::remove(waiting_.begin(), waiting_.end(), s), waiting_.end());
  aborted_.push_back(finish(s, FINISH_ABORT, now_seconds()));
  running_.erase(std::remove(running_.begin(), running_.end(), s), running_.end());
  seqs_.erase(it);
  return true;
}

std::vector<SeqOutput> Scheduler::drain_aborted() {
  std::vector<SeqOutput> o;
  o.swap(aborted_);
  return o;
}

std::vector<Scheduler::SeqState> Scheduler::debug_state() const {
  std::vector<SeqState> out;
  for (const auto& kv : seqs_) {
    const Sequence* s = kv.second.get();
    out.push_back({s->id, s->running, s->embed, s->embed_slot, s->num_computed, (int32_t)s->tokens.size(),
                   (int32_t)s->blocks.size()});
  }
  return out;
}

std::vector<int32_t> Scheduler::take_embed_resets() {
  std::vector<int32_t> r;
  r.swap(embed_resets_);
  return r;
}

std::vector<Scheduler::DraftCounts> Scheduler::take_draft_counts() {
  std::vector<DraftCounts> r;
  r.swap(draft_counts_);
  return r;
}

std::vector<std::pair<int64_t, std::vector<int32_t>>> Scheduler::take_span_finishes() {
  std::vector<std::pair<int64_t, std::vector<int32_t>>> r;
  r.swap(span_finishes_);
  return r;
}

std::vector<int32_t> Scheduler::planned_draft(int64_t id) const {
  if (!plans_.empty())
    for (const Planned& p : plans_.back().rows)
      if (p.s->id == id && !p.s->done) return p.draft;
  return {};
}

Scheduler::KvMoves Scheduler::take_kv_moves() {
  KvMoves m;
  bm_.take_moves(m.spills, m.fills);
  return m;
}

std::vector<std::pair<int32_t, int32_t>> Scheduler::prefix_blocks(const std::vector<int32_t>& tokens) const {
  std::vector<std::pair<int32_t, int32_t>> out;
  const int32_t B = cfg_.block_size;
  uint64_t parent = 0;
  for (size_t b = 0; (b + 1) * B <= tokens.size(); ++b) {
    const int32_t* t = tokens.data() + b * B;
    const uint64_t h = hash_block(parent, t, B);
    int32_t id = bm_.peek(h, t);
    if (id >= 0) {
      out.emplace_back(0, id);
    } else if ((id = bm_.host_peek(h, t)) >= 0) {
      out.emplace_back(1, id);
    } else {
      break;
    }
    parent = h;
  }
  return out;
}

std::vector<int64_t> Scheduler::planned_ids() const {
  std::vector<int64_t> ids;
  if (!plans_.empty())
    for (const Planned& p : plans_.back().rows) ids.push_back(p.s->id);
  return ids;
}

void Scheduler::reset_prefix_cache() {
  if (running_.empty()) bm_.reset();
  else bm_.reset_host();
}

}  // namespace rt
