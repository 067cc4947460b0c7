// Stress driver for the prefix cache's host tier (block_manager.h "Host tier"), built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_host_tier_sanitizers.py.
//
// Drives a scheduler with a deliberately small pool (24 device blocks, 12 host slots) through a
// few thousand steps of prompts drawn from a handful of shared prefixes, with aborts and
// preemption, and models the memory the engine would move: one tag per (block, slot in block)
// and per (host slot, slot in block), the tag of a KV entry being the hash of the token prefix
// it belongs to. Every step applies, in the order of the engine's contract,
//   1. the spills, 2. the fills (take_kv_moves), 3. the step's partial-block copy list,
//   4. the step's own KV writes (the slot region),
// and then checks that every position below ctx_len of every sequence in the step reads the tag
// of its own prefix through its block table -- whatever interleaving of evictions, hits, releases
// and re-evictions the schedule() call went through. Exits non-zero on a violation, or when a run
// saw no spill, fill, host-slot eviction or preemption.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../block_manager.h"
#include "../scheduler.h"

using namespace rt;

#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

struct Req {
  std::vector<int32_t> toks;   // prompt, then every generated token the scheduler fed back
  std::vector<uint64_t> tags;  // tags[p]: the hash of toks[0 .. p]
  size_t prompt_len = 0;
  void put(size_t p, int32_t tok) {
    if (p < toks.size()) {
      CHECK(toks[p] == tok);  // a request's tokens never change, across preemption either
      return;
    }
    CHECK(p == toks.size());
    toks.push_back(tok);
    tags.push_back(hash_block(p ? tags[p - 1] : 0, &tok, 1));
  }
};

struct Totals {
  long long spills = 0, fills = 0, evicted = 0, preempt = 0, steps = 0, copies = 0, checked = 0;
};

static void run(uint32_t seed, Totals& tot) {
  std::mt19937 rng(seed);
  SchedulerConfig cfg;
  cfg.num_blocks = 24;
  cfg.host_slots = 12;
  cfg.host_cache_step_blocks = (seed % 3 == 0) ? 2 : 256;  // the cap ends chains early
  cfg.block_size = 16;
  cfg.max_num_seqs = 6;
  cfg.max_num_batched_tokens = 128;
  cfg.max_prefill_tokens = 128;
  cfg.max_model_len = 256;
  cfg.partial_block_reuse = true;
  cfg.same_step_prefix = seed % 2 == 0;
  cfg.token_align = 0;
  cfg.eos_ids = {2};
  const int32_t B = cfg.block_size;
  Scheduler sch(cfg);
  const StepLayout& L = sch.layout();
  std::vector<int32_t> buf(L.span_total + 16, 0);
  std::vector<uint64_t> dev((size_t)cfg.num_blocks * B, 0), host((size_t)cfg.host_slots * B, 0);

  std::vector<std::vector<int32_t>> prefixes;
  for (int i = 0; i < 5; ++i) {
    std::vector<int32_t> p;
    for (int j = 0, m = B * (2 + rng() % 4); j < m; ++j) p.push_back(10 + rng() % 900);
    prefixes.push_back(p);
  }
  std::map<int64_t, Req> reqs;
  std::set<int64_t> live;
  int64_t next_id = 1;
  const int64_t n_req = 600;
  int steps = 0;
  while (steps < 6000 && (next_id <= n_req || sch.has_work())) {
    for (int a = rng() % 3; a > 0 && next_id <= n_req; --a) {
      std::vector<int32_t> prompt = prefixes[rng() % prefixes.size()];
      if (rng() % 4 == 0) prompt.resize(1 + rng() % prompt.size());  // leaves the chain inside a block
      for (int j = 0, m = 1 + rng() % 30; j < m; ++j) prompt.push_back(10 + rng() % 900);
      Req r;
      r.prompt_len = prompt.size();
      for (size_t p = 0; p < prompt.size(); ++p) r.put(p, prompt[p]);
      reqs.emplace(next_id, std::move(r));
      sch.add_request(next_id, prompt, 0.7f, 1 + rng() % 40, next_id, rng() % 4 == 0, {3}, nullptr);
      live.insert(next_id++);
    }
    if (!live.empty() && rng() % 23 == 0) {
      auto it = live.begin();
      std::advance(it, rng() % live.size());
      sch.abort(*it);
    }
    for (const SeqOutput& o : sch.drain_aborted()) {
      CHECK(live.count(o.id));
      live.erase(o.id);
      reqs.erase(o.id);
    }
    const int32_t T = sch.schedule(buf.data(), (int32_t)buf.size() - 16);
    ++steps;
    // 1, 2: the moves of this call, a call without a step included
    const Scheduler::KvMoves mv = sch.take_kv_moves();
    for (const KvMove& m : mv.spills) {
      CHECK(m.block >= 0 && m.block < cfg.num_blocks && m.slot >= 0 && m.slot < cfg.host_slots);
      for (int32_t j = 0; j < B; ++j) host[(size_t)m.slot * B + j] = dev[(size_t)m.block * B + j];
    }
    for (const KvMove& m : mv.fills) {
      CHECK(m.block >= 0 && m.block < cfg.num_blocks && m.slot >= 0 && m.slot < cfg.host_slots);
      for (int32_t j = 0; j < B; ++j) dev[(size_t)m.block * B + j] = host[(size_t)m.slot * B + j];
    }
    CHECK((int32_t)mv.fills.size() <= cfg.host_cache_step_blocks);
    tot.spills += (long long)mv.spills.size();
    tot.fills += (long long)mv.fills.size();
    if (T == 0) continue;
    CHECK(T <= L.max_tokens);
    // 3: the partial-block copies
    const int32_t ncopy = buf[L.n_copies];
    CHECK(ncopy >= 0 && ncopy <= L.max_seqs);
    for (int32_t c = 0; c < ncopy; ++c) {
      const int32_t src = buf[L.copy_list + 3 * c], dst = buf[L.copy_list + 3 * c + 1],
                    j = buf[L.copy_list + 3 * c + 2];
      CHECK(src >= 0 && src < cfg.num_blocks && dst >= 0 && dst < cfg.num_blocks && src != dst && j > 0 && j < B);
      for (int32_t i = 0; i < j; ++i) dev[(size_t)dst * B + i] = dev[(size_t)src * B + i];
    }
    tot.copies += ncopy;
    // 4: the step's own KV writes
    const int32_t ns = buf[L.counts + 1], nsamp = buf[L.counts + 2];
    const std::vector<int64_t> ids = sch.planned_ids();
    CHECK((int32_t)ids.size() == ns && ns <= L.max_seqs);
    for (int32_t r = 0; r < ns; ++r) {
      auto it = reqs.find(ids[r]);
      CHECK(it != reqs.end());
      Req& q = it->second;
      const int32_t q0 = buf[L.q_start + r], qn = buf[L.q_len + r], ctx = buf[L.ctx_len + r];
      CHECK(qn > 0 && q0 >= 0 && q0 + qn <= T && ctx >= qn && ctx <= cfg.max_model_len);
      for (int32_t j = 0; j < qn; ++j) {
        const int32_t p = buf[L.positions + q0 + j], slot = buf[L.slots + q0 + j];
        CHECK(p == ctx - qn + j && slot >= 0 && slot < cfg.num_blocks * B);
        CHECK(slot == buf[L.block_table + (size_t)r * L.max_blocks + p / B] * B + p % B);
        q.put((size_t)p, buf[L.input_ids + q0 + j]);
        dev[slot] = q.tags[p];
      }
    }
    // every position of every sequence of the step reads the KV of its own prefix
    for (int32_t r = 0; r < ns; ++r) {
      const Req& q = reqs.find(ids[r])->second;
      const int32_t ctx = buf[L.ctx_len + r];
      CHECK((size_t)ctx <= q.tags.size());
      for (int32_t p = 0; p < ctx; ++p) {
        const int32_t blk = buf[L.block_table + (size_t)r * L.max_blocks + p / B];
        CHECK(blk >= 0 && blk < cfg.num_blocks);
        if (dev[(size_t)blk * B + p % B] != q.tags[p]) {
          std::fprintf(stderr, "seed %u step %d: request %lld position %d reads block %d slot %d: wrong KV\n", seed,
                       steps, (long long)ids[r], p, blk, p % B);
          std::exit(1);
        }
        ++tot.checked;
      }
    }
    std::vector<int32_t> sampled(nsamp);
    for (auto& s : sampled) s = (rng() % 25 == 0) ? 2 : (rng() % 40 == 0 ? 3 : 10 + (int32_t)(rng() % 900));
    for (const SeqOutput& o : sch.commit(sampled.data(), nsamp)) {
      CHECK(live.count(o.id));
      CHECK(o.cached_prompt_tokens >= 0 && o.cached_prompt_tokens <= o.prompt_len);
      live.erase(o.id);
      reqs.erase(o.id);
    }
  }
  CHECK(!sch.has_work() && live.empty());
  CHECK(sch.num_free_blocks() == cfg.num_blocks);
  CHECK(sch.num_host_cached() <= cfg.host_slots);
  const long long sp = sch.host_spilled_blocks(), hi = sch.host_hit_blocks(), ev = sch.host_evicted_blocks(),
                  pre = sch.total_preemptions();
  std::printf("host tier seed %u: %d steps, %lld spills, %lld fills, %lld host evictions, %lld preemptions, "
              "%lld cached prompt tokens\n", seed, steps, sp, hi, ev, pre, (long long)sch.total_cached_tokens());
  CHECK(sp > 0 && hi > 0 && ev > 0 && pre > 0);
  tot.evicted += ev;
  tot.preempt += pre;
  tot.steps += steps;
  sch.reset_prefix_cache();
  CHECK(sch.num_cached_blocks() == 0 && sch.num_host_cached() == 0);
}

int main(int argc, char** argv) {
  const int seeds = argc > 1 ? std::atoi(argv[1]) : 4;
  Totals tot;
  for (int s = 1; s <= seeds; ++s) run((uint32_t)s, tot);
  std::printf("host tier stress: %lld steps, %lld spills, %lld fills, %lld copies, %lld host evictions, "
              "%lld preemptions, %lld positions checked\n", tot.steps, tot.spills, tot.fills, tot.copies,
              tot.evicted, tot.preempt, tot.checked);
  if (tot.spills <= 0 || tot.fills <= 0 || tot.evicted <= 0 || tot.preempt <= 0) {
    std::fprintf(stderr, "host tier stress: a run without spills, fills, host evictions or preemptions\n");
    return 1;
  }
  std::printf("host tier stress: ok\n");
  return 0;
}
