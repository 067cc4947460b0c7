// Continuous-batching scheduler for the on-node inference engine
// (replaces the reference's bounded asyncio.Queue +
// LLMHandler Semaphore(5) — pilott/pilott.py:105,272-303, engine/llm.py:36).
//
// Every engine step runs ONE forward over a ragged token batch that mixes
//   * decode tokens of running sequences (1 token, or a jump-forward run of
//     grammar-forced tokens + the last sampled token),
//   * prefill chunks of newly admitted sequences (after prefix-cache reuse),
// bounded by max_num_batched_tokens / max_num_seqs. The scheduler writes the
// complete step description (token ids, positions, KV slots, per-sequence
// q/ctx lengths, block tables, attention work items, sampling parameters and
// grammar masks) straight into a caller-provided pinned int32 buffer with a fixed
// layout, so the Python side issues a single H2D copy and replays a hipGraph.
#pragma once
#include <cstdint>
#include <deque>
#include <memory>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "block_manager.h"
#include "grammar.h"

namespace rt {

struct SchedulerConfig {
  int32_t num_blocks = 1024;
  int32_t block_size = 16;
  int32_t max_num_seqs = 256;
  int32_t max_num_batched_tokens = 2048;
  int32_t max_prefill_tokens = 2048;  // per-step budget for new prompt tokens
  int32_t max_model_len = 8192;
  int32_t gqa_group = 4;               // query heads per KV head (attention work items)
  int32_t att_qcols = 128;             // MFMA columns (heads x tokens) per prefill attention item:
                                       // 128 = the LDS-staged 4-wave path, 32 = one wave per item
  int32_t att_wide_min_tokens = 2048;
  // wide prefill items whose causal key range reaches this many keys are cut into
  // min(4, keys / prefill_split_keys) partitions of whole 32-key tiles, merged in-kernel by the
  // last partition (attention.hip prefill_item_wg): the longest causal item stops being the
  // step's critical path. 0 = off (the default: measured no gain on the steps that take wide
  // items, profiles/r6_attention_split.md). Not on decode-sized (8-wave) steps.
  int32_t prefill_split_keys = 0;
  bool prefix_caching = true;
  // A request whose first two blocks are being prefilled right now by another sequence
  // (the calls of one agent task all start with the task text and arrive together)
  // waits up to max_prefix_defer steps for them and then reuses them from the prefix
  // cache instead of computing the same KV again.
  bool dedup_inflight_prefix = true;
  int32_t max_prefix_defer = 4;
  // ... unless the other sequence's chunk in this very step covers at least one full block of
  // the common prefix: then the request joins the step, its block table pointing at those blocks
  // (in every layer the step's K and V are in the paged cache before that layer's attention runs,
  // so its queries read them exactly as the other sequence's own queries do). Both prefix
  // switches below are off unless asked for; the engine asks for both (EngineConfig).
  bool same_step_prefix = false;
  // partial-block reuse: a prompt that leaves the cached hash chain inside a block copies the
  // common head (>= partial_block_min tokens) of the best cached block under the same parent
  // into its own next block (BlockManager::match_head; the step's copy list, StepLayout::copy_list)
  // instead of computing it. Applies only to steps whose buffer is stated to hold
  // layout().copy_total words (schedule()'s second argument).
  bool partial_block_reuse = false;
  int32_t partial_block_min = 1;
  // waiting embedding requests (memory lookups / write-backs encoded by the serving model)
  // are admitted before waiting generation requests: they are short and an agent's next
  // step waits on them, while a generation prompt behind them loses a few tokens of budget
  bool embed_first = true;
  // ... but never without bound: a preempted sequence (it already held KV) stays ahead of the
  // embeds, and a generation prompt passed over by embeds for embed_first_max_wait steps is
  // admitted in arrival order again (no starvation under a steady embed stream)
  int32_t embed_first_max_wait = 8;
  bool split_decode = true;            // flash-decoding partitions for long contexts
  // decode-sized steps (<= small_step_tokens tokens) with few decode partitions use
  // small_step_part-key partitions (0 = the general rule); the engine sets it when those
  // steps run 8-wave attention workgroups, which stream a whole context without a merge
  int32_t small_step_tokens = 0;
  int32_t small_step_part = 0;
  // > 0: steps above small_step_tokens size their decode partitions for about this many
  // (partition, KV head) workgroups: no split once the decode rows alone reach it, otherwise
  // equal partitions of the longest context (multiples of 32 keys, >= 128); 0 = the 512 / 256-key
  // rule
  int32_t decode_part_target = 0;
  // the same rule for the decode-sized steps that run 8-wave attention (small_step_part > 0,
  // t_step <= small_step_tokens; one 8-wave workgroup per CU): 0 = small_step_part
  int32_t small_step_target = 0;
  // GEMM-friendly step sizes: when a step has T > token_align tokens and
  // T % token_align <= align_slack, the tail of the multi-token chunks (prefill /
  // jump-forward) is deferred so that T is a multiple of token_align (library
  // GEMM cost jumps at each 256-row tile boundary). 0 disables.
  int32_t token_align = 0;
  int32_t kv_heads = 8;                // KV heads per rank (sizes the decode partitioning)
  int32_t align_slack = 96;
  // device slots for presence / frequency penalty counts (csrc/ops/penalties.hip) and the
  // repetition penalty's seen set (csrc/ops/repetition.hip): a request with either holds one
  // from admission to finish; min(max_num_seqs, penalty_slots) exist
  int32_t penalty_slots = 64;
  // device accumulator rows for span pooling (csrc/ops/span_pool.hip): an embedding request with
  // spans holds one per span from admission to finish
  int32_t embed_span_slots = 256;
  // host tier under the prefix cache (block_manager.h): slots of pinned host memory, one block
  // each; 0 = off, and then no code path changes. A prompt's chain may continue into the tier:
  // at most host_cache_step_blocks blocks are brought back per schedule() call (the rest of the
  // chain is computed), and the caller runs the moves of every call (take_kv_moves).
  int32_t host_slots = 0;
  int32_t host_cache_step_blocks = 256;
  std::vector<int32_t> eos_ids;
};

struct StepLayout {
  int32_t max_tokens, max_seqs, max_blocks, max_items;
  int32_t input_ids, positions, slots, q_start, q_len, ctx_len, logit_rows, mask_class, forced,
      offsets, temperature, top_k, top_p, seeds, items, n_items, part_size, counts, block_table, total;
  int32_t lp_n;        // [max_seqs]: alternatives asked per sampling row (log-probabilities), -1 = none
  int32_t embed_rows;  // [max_tokens]: pooling row of each token (embedding requests), max_seqs = none
  // presence / frequency penalties, after embed_rows: written and copied only by steps with a
  // penalised sampling row (counts[9] = 1; counts[10] = words of pair_tok in use)
  int32_t pen_slot;       // [max_seqs]: penalty slot of each sampling row, -1 = none
  int32_t pen_reset;      // [max_seqs]: 1 = the slot was just taken: clear it first
  int32_t pen_presence;   // [max_seqs]: fp32 bits
  int32_t pen_frequency;  // [max_seqs]: fp32 bits
  int32_t pair_start;     // [max_seqs]: the row's new generated tokens are
  int32_t pair_n;         // [max_seqs]:   pair_tok[pair_start : pair_start + pair_n]
  int32_t pair_tok;       // [pair_cap]
  int32_t pair_cap;       // max_tokens + max_model_len
  // logit_bias / min_p ("shaped" rows, csrc/ops/logit_shaping.hip), after the penalty regions:
  // written and copied only by steps with a shaped sampling row. counts[11] (the header's one
  // free word) = 0 in every other step, else 1 + the words of bias_tok / bias_val in use.
  int32_t bias_start;  // [max_seqs]: the row's bias list is entries
  int32_t bias_n;      // [max_seqs]:   [bias_start, bias_start + bias_n) of bias_tok / bias_val
  int32_t minp;        // [max_seqs]: fp32 bits of min_p, 0 = off
  int32_t ln_minp;     // [max_seqs]: fp32 bits of float32(ln min_p), as submitted
  int32_t bias_tok;    // [bias_cap]
  int32_t bias_val;    // [bias_cap]: fp32 bits
  int32_t bias_cap;    // max_seqs * LOGIT_BIAS_MAX: a step's lists always fit
  // repetition penalty (csrc/ops/repetition.hip), after the shaping regions and behind `total`:
  // written and copied only by steps with a sampling row that carries one. Such a step sets bit
  // 1 of counts[9] and puts the words of rep_tok in use into the bits above it:
  // counts[9] = [penalised row] | 2 | words << 2. `total` stays the extent of the regions above,
  // all a scheduler that is never given a repetition_penalty writes; rep_total is the whole
  // buffer, and schedule() refuses to write these regions into a buffer not stated to be that long.
  int32_t rep_slot;   // [max_seqs]: slot of each sampling row (the request's penalty slot), -1 = none
  int32_t rep_reset;  // [max_seqs]: 1 = the slot was just taken: clear its set first
  int32_t rep_r;      // [max_seqs]: fp32 bits of r
  int32_t rep_inv_r;  // [max_seqs]: fp32 bits of float32(1 / r), as submitted
  int32_t rep_start;  // [max_seqs]: the row's new tokens (prompt and generated) are
  int32_t rep_n;      // [max_seqs]:   rep_tok[rep_start : rep_start + rep_n]
  int32_t rep_tok;    // [rep_cap]
  int32_t rep_cap;    // max_tokens + max_model_len: one whole backlog always fits
  int32_t rep_total;
  // prompt scoring (csrc/ops/scoring.hip), behind rep_total: written and copied only by steps
  // with a scoring row, which set bit 30 of counts[9]. rep_total and everything before it keep
  // their values; score_total is the whole buffer, and schedule() refuses a scoring request
  // unless the buffer is stated to be that long.
  int32_t score_target;  // [max_seqs]: the token each row scores (tokens[p + 1]), -1 = not a scoring row
  int32_t score_total;
  // partial-block copies (csrc/ops/kv_copy.hip), behind score_total: n_copies is the word after
  // n_items (inside the header every step copies; 0 in a step without copies), copy_list holds
  // that many (donor block, new block, slots) triples and is written and copied only by steps
  // that have some. copy_total is the whole buffer; a scheduler whose buffer is not stated to be
  // that long plans no partial-block reuse.
  int32_t n_copies;
  int32_t copy_list;  // [3 * max_seqs]
  int32_t copy_total;
  // draft steps (predicted outputs / prompt-lookup drafts; csrc/ops/spec_verify.hip), behind
  // copy_total: written and copied only by steps in which a request owns draft rows, which set
  // bit 29 of counts[9]. Every sampling row r of such a step carries the run it belongs to:
  // rows [run_first[r], run_first[r] + run_len[r]) are one request's, a plain row is (r, 1).
  // copy_total and everything before it keep their values; spec_total is the whole buffer, and a
  // scheduler whose buffer is not stated to be that long plans no drafts.
  int32_t run_first;  // [max_seqs]
  int32_t run_len;    // [max_seqs]
  int32_t spec_total;
  // span pooling (embedding requests with spans; csrc/ops/span_pool.hip), behind spec_total:
  // written and copied only by steps in which a span has rows, which set bit 28 of counts[9].
  // span_n is the step's segment count, span_segs that many (first row of the step, rows, span
  // slot, init) quadruples: the rows of one scheduled chunk that lie inside one span, init = 1
  // when they start at the span's first token. A span contributes at most one segment per step,
  // so embed_span_slots quadruples always suffice. spec_total and everything before it keep their
  // values; span_total is the whole buffer, and schedule() refuses a request with spans unless
  // the buffer is stated to be that long.
  int32_t span_n;     // [1]
  int32_t span_segs;  // [4 * span_slots]
  int32_t span_slots;
  int32_t span_total;
};

constexpr int32_t COUNTS9_SCORE_BIT = 1 << 30;  // counts[9]: the step has scoring rows
constexpr int32_t COUNTS9_SPEC_BIT = 1 << 29;   // counts[9]: the step has draft rows (above the repetition words)
// counts[9]: the step has span segments. The repetition words above bit 1 count at most
// rep_cap = max_num_batched_tokens + max_model_len tokens: they stay below bit 28 while that is
// under 2^26, and add_request refuses spans on a scheduler configured beyond it.
constexpr int32_t COUNTS9_SPAN_BIT = 1 << 28;
constexpr int32_t MAX_DRAFT_LEN = 8;            // draft tokens of one run (add_request clamps draft_len)

constexpr int32_t LOGIT_BIAS_MAX = 300;  // entries of one request's logit_bias

enum FinishReason : int32_t {
  NOT_FINISHED = -1, FINISH_STOP = 0, FINISH_LENGTH = 1, FINISH_ABORT = 2,
  FINISH_EMBED = 3,  // embedding request: prompt fully prefilled, pooled hidden state ready
  FINISH_SCORE = 4   // scoring request: the last scored prompt position has its record
};

// Log-probability record of one generated token, as the device writes it per sampling row
// (csrc/ops/sampling.hip logprob_merge_kernel): the chosen token's logprob, then up to
// LOGPROB_TOP (token id, logprob) alternatives by descending logit (id -1 / -inf past the end).
constexpr int32_t LOGPROB_TOP = 20;
struct LogprobRecord {
  float lp;
  int32_t ids[LOGPROB_TOP];
  float lps[LOGPROB_TOP];
};
static_assert(sizeof(LogprobRecord) == 4 * (1 + 2 * LOGPROB_TOP), "LogprobRecord is 41 packed 32-bit words");

// Record of one scored prompt token, as the device writes it per scoring row (csrc/ops/scoring.hip
// score_merge_kernel): the token's logprob, its rank in the vocabulary (1 = most likely; larger
// logit first, equal logits by smaller id), then the alternatives as in LogprobRecord.
struct ScoreRecord {
  float lp;
  int32_t rank;
  int32_t ids[LOGPROB_TOP];
  float lps[LOGPROB_TOP];
};
static_assert(sizeof(ScoreRecord) == 4 * (2 + 2 * LOGPROB_TOP), "ScoreRecord is 42 packed 32-bit words");

struct SeqOutput {
  int64_t id;
  std::vector<int32_t> tokens;  // generated tokens (sampled + grammar-forced)
  int32_t finish_reason;
  int32_t prompt_len;
  int32_t cached_prompt_tokens;
  int32_t num_sampled;
  int32_t num_forced;
  double t_first_token;
  double t_finish;
  int32_t embed_slot = -1;  // pooling row of an embedding request (FINISH_EMBED: holds the sums)
  int32_t logprobs = -1;    // alternatives the request asked for (-1: it did not ask)
  std::vector<LogprobRecord> lp_records;  // logprobs >= 0: one per entry of `tokens`
  int32_t score_from = -1;  // scoring request: the first scored prompt position (-1: not one)
  int32_t score_n = 0;      // ... and the alternatives it asked for
  std::vector<ScoreRecord> score_records;  // FINISH_SCORE: prompt_len - score_from entries
  // drafting request: draft tokens proposed; those the sampler confirmed; and the tokens of draft
  // steps that moved the prediction cursor (confirmed prediction drafts, plus a run's own last
  // token when it equals the next prediction token) -- all 0 for any other request
  int32_t draft_proposed = 0, draft_accepted = 0, prediction_matched = 0;
};

struct Sequence {
  int64_t id;
  // embedding request pooled from its LAST token's final hidden state: the prompt may then
  // reuse cached prefix blocks (a token's hidden state depends only on its prefix)
  bool embed_last = false;
  std::vector<int32_t> tokens;
  int32_t prompt_len = 0;
  int32_t num_computed = 0;
  int32_t num_generated = 0;
  int32_t num_sampled = 0;
  int32_t num_forced = 0;
  int32_t cached_prompt_tokens = -1;
  std::vector<int32_t> blocks;
  std::vector<uint64_t> block_hashes;  // hash chain of registered leading blocks
  std::unique_ptr<Grammar> grammar;
  float temperature = 0.7f;
  int32_t top_k = 0;    // 0 = no top-k truncation
  float top_p = 1.0f;   // 1 = no nucleus truncation
  int32_t max_tokens = 256;
  int64_t seed = 0;
  int32_t logprobs = -1;  // >= 0: log-probability records are kept, with this many alternatives
  std::vector<LogprobRecord> lp_records;  // one per generated token (tokens[prompt_len:])
  // presence / frequency penalties: the device keeps the counts of tokens[prompt_len:] in
  // penalty slot pen_slot (held from admission to finish, across preemption); pen_synced of
  // those tokens have been sent to it; pen_fresh: the slot's old contents are not cleared yet
  float presence_penalty = 0.f, frequency_penalty = 0.f;
  int32_t pen_slot = -1;
  int32_t pen_synced = 0;
  bool pen_fresh = false;
  bool penalised() const { return !embed && (presence_penalty != 0.f || frequency_penalty != 0.f); }
  // logit_bias (unique token ids, non-zero values, at most LOGIT_BIAS_MAX) and min_p with the
  // float32(ln min_p) the host computed at submit: fixed for the life of the request, no
  // device state, so every sampling row of the sequence simply carries them
  std::vector<std::pair<int32_t, float>> logit_bias;
  float min_p = 0.f, ln_min_p = 0.f;
  bool shaped() const { return !embed && (!logit_bias.empty() || min_p > 0.f); }
  // repetition penalty r in (0, 2], 1 = off, with the float32(1 / r) the host computed at submit.
  // The device keeps the set of distinct ids of tokens[0:] -- the prompt too, whatever part of it
  // the prefix cache serves -- in the request's penalty slot (the same index as the additive
  // penalties' counts, separate arrays); rep_synced of those tokens have been sent to it;
  // rep_fresh: the slot's old set is not cleared yet
  float repetition_penalty = 1.f, inv_repetition_penalty = 1.f;
  int32_t rep_synced = 0;
  bool rep_fresh = false;
  bool repetitive() const { return !embed && repetition_penalty != 1.f; }
  bool needs_slot() const { return penalised() || repetitive(); }
  // scoring request (score_from = k >= 1): generates nothing. Positions k-1 .. len-2 are computed,
  // each with one row of the step whose target is the next prompt token; the last prompt token
  // predicts nothing and is not computed. score_records: one per scored position so far.
  int32_t score_from = -1;
  int32_t score_n = 0;
  std::vector<ScoreRecord> score_records;
  bool scoring() const { return score_from >= 0; }
  // tokens whose KV / logits the request still needs: all of them, or all but a scoring request's last
  int32_t compute_len() const { return (int32_t)tokens.size() - (scoring() ? 1 : 0); }
  // drafting request (draft_len > 0 and a draft source): when its decode row is planned, up to
  // draft_len tokens are proposed behind it and verified in the same step (Scheduler::propose).
  // pred_c: the prediction cursor; pred_synced: prediction[pred_c] is aligned with the next
  // token to generate (true at the start, kept while committed tokens follow the prediction,
  // regained by the n-gram resync)
  std::vector<int32_t> prediction;
  bool prompt_lookup = false;
  int32_t draft_len = 0;
  int32_t pred_c = 0;
  bool pred_synced = true;
  int32_t draft_proposed = 0, draft_accepted = 0, prediction_matched = 0;
  bool drafting() const { return draft_len > 0 && (!prediction.empty() || prompt_lookup); }
  bool ignore_eos = false;
  std::vector<int32_t> stop_ids;
  int64_t arrival = 0;
  double t_first_token = -1.0;
  bool running = false;
  // embedding request: the whole prompt is computed (no prefix-cache reuse: every token's
  // final hidden state is summed into pooling row embed_slot), nothing is sampled
  bool embed = false;
  int32_t embed_slot = -1;
  // spans [a, b) over the prompt, sorted by a (overlap allowed): every scheduled chunk lists, per
  // span, its rows inside the span as one segment for the span's slot. span_slots is empty until
  // admission and is kept across preemption: the request restarts at token 0, so every span meets
  // its first token -- and with it the segment that re-initialises the slot -- again.
  std::vector<std::pair<int32_t, int32_t>> spans;
  std::vector<int32_t> span_slots;
  // partial-block reuse: the first copy_j slots of block copy_dst (the sequence's own) come from
  // block copy_src, on which the sequence holds a reference until the step that first runs it
  // has listed the copy; copy_j = 0: none pending
  int32_t copy_src = -1, copy_dst = -1, copy_j = 0;
  bool tail_listed = false;  // the prompt's partly filled last block is in the donor index
  int32_t defer_count = 0;  // steps deferred waiting for an in-flight identical prefix
  int32_t embed_passed = 0; // steps an embed-first admission put embeds ahead of this prompt
  bool preempted = false;   // lost its KV to a preemption and waits to resume
  // pipelined steps (Scheduler "speculative rows"): plans not yet committed that list this
  // sequence; the plan (id) and row in which it last sampled; the plan and entry index of
  // its speculative continuation
  int32_t inflight = 0;
  int64_t pend_plan = -1;
  int32_t pend_idx = -1;
  int64_t spec_plan = -1;
  int32_t spec_entry = -1;
  bool done = false;           // finished while a later in-flight plan still lists it
  bool abort_pending = false;  // aborted while in flight: finished once no plan lists it
};

class Scheduler {
 public:
  explicit Scheduler(const SchedulerConfig& cfg);
  const StepLayout& layout() const { return lay_; }
  const SchedulerConfig& config() const { return cfg_; }

  void add_request(int64_t id, std::vector<int32_t> prompt, float temperature, int32_t max_tokens,
                   int64_t seed, bool ignore_eos, std::vector<int32_t> stop_ids,
                   std::unique_ptr<Grammar> grammar, int32_t top_k = 0, float top_p = 1.0f,
                   bool embed = false, bool embed_last = false, int32_t logprobs = -1,
                   float presence_penalty = 0.f, float frequency_penalty = 0.f,
                   std::vector<std::pair<int32_t, float>> logit_bias = {}, float min_p = 0.f,
                   float ln_min_p = 0.f, float repetition_penalty = 1.f,
                   float inv_repetition_penalty = 0.f,  // 0: float32(1 / r) is computed here
                   // k in [1, prompt_len - 1]: a scoring request over prompt positions k .. len-1
                   // (`logprobs` = its alternatives, 0..20; nothing is generated; grammar, penalties,
                   // logit_bias, min_p and embed are not allowed); anything else but -1 throws
                   int32_t score_from = -1,
                   // drafts (see Sequence): `prediction` token ids the reply is expected to repeat,
                   // `prompt_lookup` n-gram drafts from the request's own tokens, `draft_len` the
                   // tokens proposed per step (0 = off, at most MAX_DRAFT_LEN). A request with a
                   // draft source and draft_len > 0 takes no logprobs, penalties, score_from or embed
                   // (std::invalid_argument); without a source, or with draft_len 0, nothing changes
                   std::vector<int32_t> prediction = {}, bool prompt_lookup = false, int32_t draft_len = 0,
                   // token ranges [a, b) of an embedding request's prompt (mean pooling only), each
                   // pooled into a span slot of its own beside the whole-prompt row: 0 <= a < b <=
                   // prompt_len, sorted by a, at most embed_span_slots of them, a prompt shorter than
                   // max_model_len; anything else throws std::invalid_argument
                   std::vector<std::pair<int32_t, int32_t>> spans = {});
  bool abort(int64_t id);
  // Fill `buf` (layout()) for the next step. Returns the number of tokens in the
  // step (0 = nothing to run).
  //
  // Pipelined use: schedule() may be called again before the previous step is
  // committed (at most one uncommitted step). A row that samples in that in-flight step
  // is then planned speculatively: its unknown token enters the new step as input id
  // -(r + 1) (r = its sampling row in the in-flight step; the device replaces it from
  // that step's sampled tokens before the embedding lookup), followed by the grammar's
  // forced run where that run does not depend on the token. String and list bodies
  // assume a body token (not the closing / separator token), free-text rows assume no
  // EOS. commit() of the in-flight step checks the guess; a wrong guess voids the row's
  // speculative entry (its sample is dropped, its KV beyond the pending token is
  // recomputed) — only the sampled token's own KV is kept, and it is always right.
  //
  // `buf_words`: the size of `buf` in 32-bit words, 0 = not stated. layout().total covers every
  // region except the repetition penalty's, which lie behind it (layout().rep_total is the whole
  // buffer). Once a request with a repetition penalty has been added, schedule() throws
  // std::invalid_argument unless buf_words >= layout().rep_total, so a caller that sized its buffer by `total` and then adds a
  // request with a repetition penalty gets an error, never a write past its buffer.
  // The same holds one region further for scoring requests: once one has been added, schedule()
  // throws unless buf_words >= layout().score_total.
  // And one further for spans: once a request with spans has been added, schedule() throws unless
  // buf_words >= layout().span_total.
  // Drafts are planned only into a buffer stated to hold layout().spec_total words, and never
  // while a step is in flight (pipelined use): otherwise a drafting request decodes plainly.
  int32_t schedule(int32_t* buf, int32_t buf_words = 0);
  // Consume the sampled tokens of the oldest uncommitted step (one per sampling row).
  // `lp`: the step's log-probability records, one per sampling row (nullptr: the step computed
  // none); rows of requests that did not ask hold nothing meaningful and are not read.
  // `sc`: the step's score records, indexed by row like `sampled` (a scoring row counts as one of
  // the n rows; its sampled token is ignored); nullptr: the step computed none.
  // `accept_len`: the step's acceptance lengths, indexed by row like `sampled`
  // (csrc/ops/spec_verify.hip: a + 1 on the first row of a run). A run of 1 + k rows commits its
  // first a + 1 tokens, each exactly as a one-token commit would (grammar advance, stops,
  // jump-forward); a stop inside the run drops the rest. nullptr: every run commits one token.
  std::vector<SeqOutput> commit(const int32_t* sampled, int32_t n, const LogprobRecord* lp = nullptr,
                                const ScoreRecord* sc = nullptr, const int32_t* accept_len = nullptr);
  int32_t inflight_steps() const { return (int32_t)plans_.size(); }
  int64_t spec_rows() const { return stat_spec_rows_; }
  int64_t spec_voided() const { return stat_spec_voided_; }
  // drafts: tokens proposed, tokens the sampler confirmed, steps with draft rows, runs whose
  // whole draft was confirmed
  int64_t spec_draft_tokens() const { return stat_draft_tokens_; }
  int64_t spec_accepted_tokens() const { return stat_draft_accepted_; }
  int64_t spec_draft_steps() const { return stat_draft_steps_; }
  int64_t spec_runs_full() const { return stat_draft_full_; }
  // (id, proposed, accepted, prediction_matched) of the drafting requests finished since the
  // last call (the SeqOutput fields, for callers that read outputs as tuples)
  struct DraftCounts {
    int64_t id;
    int32_t proposed, accepted, matched;
  };
  std::vector<DraftCounts> take_draft_counts();
  // The finish records of span requests: (id, the accumulator row of each span in the request's
  // span order) of those finished or aborted since the last call. After FINISH_EMBED the rows
  // hold the sums: read them before the next step is scheduled. Take the records every step; the
  // list keeps the newest kMaxSpanFinishes.
  static constexpr size_t kMaxSpanFinishes = 4096;
  std::vector<std::pair<int64_t, std::vector<int32_t>>> take_span_finishes();
  // the draft of the request's entry in the step scheduled last (empty: none), for diagnostics
  std::vector<int32_t> planned_draft(int64_t id) const;
  // Finished-by-abort outputs are returned here as well.
  std::vector<SeqOutput> drain_aborted();

  int32_t num_running() const { return (int32_t)running_.size(); }
  int32_t num_waiting() const { return (int32_t)waiting_.size(); }
  int32_t num_free_blocks() const { return bm_.num_free(); }
  int32_t num_cached_blocks() const { return bm_.num_cached(); }
  int64_t total_prompt_tokens() const { return stat_prompt_tokens_; }
  int64_t total_cached_tokens() const { return stat_cached_tokens_; }
  int64_t total_preemptions() const { return stat_preemptions_; }
  int64_t steps() const { return stat_steps_; }
  int64_t aligned_steps() const { return stat_aligned_steps_; }
  int64_t prefix_defers() const { return stat_prefix_defers_; }
  int64_t partial_hit_tokens() const { return stat_partial_tokens_; }  // counted in total_cached_tokens too
  int64_t same_step_shares() const { return stat_same_step_; }         // requests that joined a prefix's own step
  int32_t num_donor_blocks() const { return bm_.num_donors(); }
  int32_t block_ref(int32_t block) const {
    return (block >= 0 && block < bm_.num_blocks()) ? bm_.ref_count(block) : -1;
  }
  bool has_work() const { return !running_.empty() || !waiting_.empty(); }
  void reset_prefix_cache();
  // Pooling rows whose embedding request was preempted in the last schedule() (it restarts
  // from token 0): the caller clears them before running the step.
  std::vector<int32_t> take_embed_resets();
  // The host tier's moves planned by the last schedule() call: spills (device block -> host slot)
  // and fills (host slot -> device block), each in planning order. The caller executes all
  // spills, then all fills, before the step runs -- after every schedule() call, one that
  // returned 0 tokens included. Both are empty without a host tier.
  struct KvMoves {
    std::vector<KvMove> spills, fills;
  };
  KvMoves take_kv_moves();
  int64_t host_hit_blocks() const { return bm_.host_hit_blocks(); }
  int64_t host_spilled_blocks() const { return bm_.host_spilled_blocks(); }
  int64_t host_evicted_blocks() const { return bm_.host_evicted_blocks(); }
  int32_t num_host_cached() const { return bm_.num_host_cached(); }
  // Where the leading full blocks of `tokens` are: (tier, id) per block of the hash chain, tier
  // 0 = device block, 1 = host slot, up to the first miss. No reference is taken and no LRU
  // order changes (diagnostics).
  std::vector<std::pair<int32_t, int32_t>> prefix_blocks(const std::vector<int32_t>& tokens) const;
  // the request of each row (sequence entry) of the step scheduled last, for diagnostics
  std::vector<int64_t> planned_ids() const;
  struct SeqState {
    int64_t id;
    bool running, embed;
    int32_t embed_slot, num_computed, num_tokens, num_blocks;
  };
  std::vector<SeqState> debug_state() const;  // every live sequence (diagnostics)
  int32_t num_free_embed_rows() const { return (int32_t)embed_free_.size(); }
  int32_t num_free_penalty_slots() const { return (int32_t)pen_free_.size(); }
  int32_t num_free_span_slots() const { return (int32_t)span_free_.size(); }

 private:
  bool ensure_blocks(Sequence* s, int32_t upto_tokens);
  void preempt(Sequence* s);
  void match_prefix(Sequence* s);
  // blocks of `r` (planned in the step being built, ending at r_end tokens) that `s` can share
  int32_t share_same_step(Sequence* s, const Sequence* r, int32_t r_end);
  void match_partial(Sequence* s);
  void count_cached(Sequence* s);
  void drop_copy(Sequence* s);
  void register_full_blocks(Sequence* s);
  SeqOutput finish(Sequence* s, int32_t reason, double now);
  void free_seq(Sequence* s, bool keep_embed_slot = false);

  SchedulerConfig cfg_;
  StepLayout lay_;
  BlockManager bm_;
  std::unordered_map<int64_t, std::unique_ptr<Sequence>> seqs_;
  std::deque<Sequence*> waiting_;
  std::vector<Sequence*> running_;
  struct Planned {
    Sequence* s;
    int32_t n;
    bool sample;
    int32_t end = 0;              // num_computed after this entry (its last token's position + 1)
    int32_t keep = 1;             // tokens the alignment trim must leave: another entry reads their blocks
    int32_t score_rows = 0;       // scoring request: rows of the step this entry owns (its last tokens)
    bool spec = false;            // speculative continuation of a row sampling in the previous plan
    bool voided = false;          // the speculation failed: nothing of this entry is committed
    int32_t src_idx = -1;         // spec: sampling row of the pending token in the previous plan
    std::vector<int32_t> run;     // spec: predicted forced tokens after the pending token
    Grammar::Cursor cur;          // spec: predicted automaton state before this entry's sample
    // draft entry: the last `draft.size()` of the n tokens are proposed, not yet real; the entry
    // owns 1 + draft.size() sampling rows, row j with the grammar's (class, forced) in row_gram[j]
    std::vector<int32_t> draft;
    std::vector<std::pair<int32_t, int32_t>> row_gram;
    bool draft_pred = false;      // the draft comes from the prediction (at pred_c), not from lookup
  };
  // up to k draft tokens for the decode row of `s` (empty: none); may move the prediction cursor
  std::vector<int32_t> propose(Sequence* s, int32_t k, bool* from_prediction) const;
  // one committed token: what a one-token commit applies. Returns the finish reason.
  int32_t apply_token(Sequence* s, int32_t tok, const LogprobRecord* lp);
  int32_t follow_prediction(Sequence* s, size_t from);  // -> tokens that were the prediction's next
  struct Plan {
    int64_t id;
    std::vector<Planned> rows;
  };
  bool predict(Sequence* s, Planned& e) const;
  std::vector<Planned> last_plan_;   // the plan being built by schedule()
  std::deque<Plan> plans_;           // scheduled, not yet committed (oldest first)
  int64_t next_plan_id_ = 0;
  std::vector<std::unique_ptr<Sequence>> zombies_;
  std::vector<Sequence*> abort_wait_;               // aborted while listed by an in-flight step  // finished, still listed by an in-flight plan
  int64_t stat_spec_rows_ = 0, stat_spec_voided_ = 0;
  std::vector<SeqOutput> aborted_;
  std::vector<int32_t> embed_free_;    // free pooling rows (0 .. max_seqs - 1)
  std::vector<int32_t> embed_resets_;  // rows of preempted embedding requests, to be cleared
  std::vector<int32_t> pen_free_;      // free penalty slots
  std::vector<int32_t> span_free_;     // free span slots
  bool span_requested_ = false;        // a request with spans was added: see schedule() (the buffer's size)
  std::vector<std::pair<int64_t, std::vector<int32_t>>> span_finishes_;
  bool rep_requested_ = false;         // a request with a repetition penalty was added: see schedule()
  bool score_requested_ = false;       // a scoring request was added: see schedule() (the buffer's size)
  int32_t score_live_ = 0;             // scoring requests not yet finished: the row budget applies
  int32_t draft_live_ = 0;             // drafting requests not yet finished: the row budget applies
  bool drafts_ok_ = false;             // the buffer of the schedule() call in progress holds the run regions
  int64_t stat_draft_tokens_ = 0, stat_draft_accepted_ = 0, stat_draft_steps_ = 0, stat_draft_full_ = 0;
  std::vector<DraftCounts> draft_counts_;
  int64_t arrival_counter_ = 0;
  int64_t stat_prompt_tokens_ = 0, stat_cached_tokens_ = 0, stat_preemptions_ = 0, stat_steps_ = 0;
  int64_t stat_aligned_steps_ = 0;
  int64_t stat_prefix_defers_ = 0;
  int64_t stat_partial_tokens_ = 0, stat_same_step_ = 0;
  bool copies_ok_ = false;  // the buffer of the schedule() call in progress holds the copy list
  int32_t fills_left_ = 0;  // host-tier fills the schedule() call in progress may still plan
  uint64_t prefix_key(const Sequence* s) const;
};

double now_seconds();

}  // namespace rt
