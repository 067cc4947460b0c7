// Python bindings for the CDNA4 kernels in csrc/ops/*.hip.
// Every entry point validates shapes/dtypes/devices on the host (so a bad call
// fails loudly instead of faulting the GPU) and launches on the caller's
// current HIP stream, which keeps them hipGraph-capturable.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>

extern "C" {
int pa_rmsnorm(void* out, const void* x, const void* w, int T, int D, float eps, hipStream_t st);
int pa_fused_add_rmsnorm(void* out, void* resid, const void* x, const void* w, int T, int D,
                         float eps, hipStream_t st);
int pa_rope_cache(void* q_out, void* k_cache, void* v_cache, const void* qkv, const int* positions,
                  const int* slot_mapping, const float* cos_sin, int T, int H, int KV, int ld,
                  int block_size, int apply_rope, hipStream_t st);
int pa_kv_copy(void* k_cache, void* v_cache, const int* n_copies, const int* copies, int max_copies,
               int layers, int num_blocks, int KV, long layer_stride, int block_size, hipStream_t st);
int pa_kv_gather_blocks(void* k_cache, void* v_cache, const int* ids, int n, void* stage, int layers,
                        int num_blocks, int KV, long layer_stride, int block_size, hipStream_t st);
int pa_kv_scatter_blocks(void* k_cache, void* v_cache, const int* ids, int n, void* stage, int layers,
                         int num_blocks, int KV, long layer_stride, int block_size, hipStream_t st);
int pa_span_pool(const void* hn, const int* n_seg, const int* segs, int cap, float* pool, int T, int d, int slots,
                 hipStream_t st);
int pa_silu_mul(void* out, const void* in, int T, int F, hipStream_t st);
int pa_paged_attention(void* out, float* part_o, float* part_ml, const void* q, const void* k_cache,
                       const void* v_cache, const int* items, const int* n_items, int max_items,
                       const int* part_size, int* counters, const int* q_start,
                       const int* q_len, const int* ctx_len, const int* block_table,
                       int max_blocks, int H, int KV, float scale_log2, int waves, int* pf_counters,
                       hipStream_t st);
int pa_sample_workspace_floats(int rows, int V);
int pa_patch_pending_ids(int* ids, const int* sampled, int T, int n_sampled, hipStream_t st);
int pa_sample(int* out_tokens, float* out_keys, float* workspace, const void* logits, int rows,
              int V, int ld, int vocab_offset, const float* temperature, const int* mask_class,
              const uint32_t* class_masks, int mask_words, const int64_t* seeds,
              const int* offsets, const int* forced, const float* tau, hipStream_t st);
int pa_sample_partials(float* workspace, const void* logits, int rows, int V, int ld, int vocab_offset,
                       const float* temperature, const int* mask_class, const uint32_t* class_masks,
                       int mask_words, const int64_t* seeds, const int* offsets, const float* tau,
                       hipStream_t st);
int pa_spec_verify(int* out_tokens, int* accept_len, const float* part_k, const int* part_i, const int* forced,
                   const int* input_ids, int n_ids, const int* logit_rows, const int* run_first,
                   const int* run_len, int rows, int nchunk, hipStream_t st);
int pa_logprob_workspace_floats(int rows, int V);
int pa_token_logprobs(float* out_lp, int out_stride, int* top_ids, float* top_lp, int top_stride, float* workspace,
                      const void* logits, int rows, int V, int ld, const int* tokens, const int* lp_n,
                      const int* forced, const int* mask_class, const uint32_t* class_masks, int mask_words,
                      hipStream_t st);
int pa_score_workspace_floats(int rows, int V);
int pa_score_tokens(float* out_lp, int* out_rank, int out_stride, int* top_ids, float* top_lp, int top_stride,
                    float* workspace, const void* logits, int rows, int V, int ld, const int* target,
                    const int* lp_n, hipStream_t st);
int pa_apply_penalties(void* logits, int rows, int V, int ld, int* counts, int* distinct, int* n_distinct,
                       int slots, int cap, const int* pen_slot, const int* pen_reset, const float* presence,
                       const float* frequency, const int* forced, const int* pair_start, const int* pair_n,
                       const int* pair_tok, int pair_len, hipStream_t st);
int pa_apply_repetition_penalty(void* logits, int rows, int V, int ld, uint32_t* seen, int words, int* list,
                                int* n_list, int slots, int cap, const int* rep_slot, const int* rep_reset,
                                const float* rep_r, const float* rep_inv_r, const int* forced,
                                const int* rep_start, const int* rep_n, const int* rep_tok, int tok_len,
                                hipStream_t st);
int pa_apply_logit_bias(void* logits, int rows, int V, int ld, const int* bias_start, const int* bias_n,
                        const int* bias_tok, const float* bias_val, int bias_len, const int* forced,
                        hipStream_t st);
int pa_minp_threshold(float* tau, int has_tau, const void* logits, int rows, int V, int ld,
                      const float* temperature, const float* min_p, const float* ln_min_p, const int* forced,
                      const int* mask_class, const uint32_t* class_masks, int mask_words, int n_classes,
                      hipStream_t st);
int pa_tp_topkp_phase(int phase, float* tau, float* ws, const void* logits, int rows, int v_local, int ld,
                      int vocab_offset, int V, const float* temperature, const int* top_k, const float* top_p,
                      const int* mask_class, const uint32_t* class_masks, int mask_words, hipStream_t st);
int pa_topkp_threshold(float* tau, const void* logits, int rows, int V, int ld, int shards,
                       long long shard_stride, const float* temperature, const int* top_k,
                       const float* top_p, const int* mask_class, const uint32_t* class_masks,
                       int mask_words, hipStream_t st);
void pa_skinny_set_variant(int v);
int pa_skinny_gemm(void* y, const void* x, const void* w, int M, int N, int K, int ldy, hipStream_t st);
void pa_decode_set_variant(int v);
void pa_handoff_set_acquire(int v);
void pa_handoff_set_modes(int gemm, int attn);
int pa_decode_gemm(void* y, const void* x, const void* wp, const void* resid, int M, int N, int K,
                   int ldx, int ldy, int ldr, int epi, int norm, float eps, int nt, int waves, int splits,
                   float* ws, long long ws_floats, int* counters, int n_counters, hipStream_t st);
int pa_decode_qkv_rope(const void* x, const void* wp, int M, int N, int K, int ldx, float eps, void* q_out,
                       void* k_cache, void* v_cache, const int* positions, const int* slots,
                       const float* cos_sin, int H, int KV, int nt, int waves, int splits, float* ws,
                       long long ws_floats, int* counters, int n_counters, hipStream_t st);
int pa_decode_gemm_fp8(void* y, const void* x, const void* wp8, const float* scale, const void* resid, int M, int N,
                       int K, int ldx, int ldy, int ldr, int epi, int norm, float eps, int nt, int waves,
                       int splits, float* ws, long long ws_floats, int* counters, int n_counters, hipStream_t st);
int pa_decode_qkv_rope_fp8(const void* x, const void* wp8, const float* scale, int M, int N, int K, int ldx,
                           float eps, void* q_out, void* k_cache, void* v_cache, const int* positions,
                           const int* slots, const float* cos_sin, int H, int KV, int nt, int waves, int splits,
                           float* ws, long long ws_floats, int* counters, int n_counters, hipStream_t st);
int pa_mid_gemm_plan(int M, int N, int K, int epi, int* fm, int* fn, int* S);
long long pa_mid_gemm_ws_floats(int M, int N, int K, int fm, int fn, int S);
int pa_mid_gemm(void* y, const void* x, const void* wp, const void* resid, float* ws, long long ws_floats,
                int* counters, int n_counters, int M, int N, int K, int ldx, int ldy, int ldr, int epi,
                const float* ss_in, float* ss_out, float* ss_zero, float eps, int fm, int fn, int splits,
                void* q_out, void* k_cache, void* v_cache, const int* positions, const int* slots,
                const float* cos_sin, int H, int KV, hipStream_t st);
int pa_row_sumsq(float* out, const void* x, int M, int K, int ldx, hipStream_t st);
int pa_timeline_marker(int id, hipStream_t st);
int pa_store_test(void* dst, long long n16, int mode, int grid, hipStream_t st);
long long pa_stream_gemm_ws_floats(int M, int N, int K, int mg, int rg, int tpw, int wt, int wk, int S);
void pa_stream_gemm_plan(int M, int N, int K, int epi, int* plan);
int pa_stream_gemm(void* y, const void* x, const void* wp, const void* resid, float* ws, long long ws_floats,
                   int* counters, int n_counters, int* err, int M, int N, int K, int ldx, int ldy, int ldr, int epi,
                   const float* ss_in, float* ss_out, float* ss_zero, float eps, const int* plan, void* q_out,
                   void* k_cache, void* v_cache, const int* positions, const int* slots, const float* cos_sin, int H,
                   int KV, int rel, unsigned long long* stamps, hipStream_t st);
void pa_prefill_gemm_plan(int M, int N, int K, int bn, int* full, int* S);
int pa_prefill_pick_bn(int M, int N);
void pa_prefill_set_variant(int v);
long long pa_prefill_gemm_ws_floats(int M, int N, int bn, int full, int S);
int pa_prefill_gemm(void* y, const void* x, const void* wp, const void* resid, float* ws, long long ws_floats,
                    int* counters, int n_counters, int M, int N, int K, int ldx, int ldy, int ldr, int epi,
                    const float* ss_in, float* ss_out, float* ss_zero, float eps, int full, int splits, int bn,
                    void* q_out, void* k_cache, void* v_cache, const int* positions, const int* slots,
                    const float* cos_sin, int H, int KV, int kernel_variant, hipStream_t st);
long long pa_cosine_topk_workspace_bytes(int Q, int N, int K);
int pa_cosine_topk(float* out_scores, int* out_rows, void* workspace, const void* queries,
                   const void* index, int Q, int N, int D, int K, const int* row_priority,
                   const uint64_t* row_tags, const float* row_expiry, const int* q_min_priority,
                   const uint64_t* q_tags, float now, int n_valid, hipStream_t st);
int pa_mmr_select_bf16(float* out_scores, int* out_rows, const int* rows, const float* scores, const void* packed,
                       const float* wr, const float* wd, int Q, int m, int K, int D, int nrows, hipStream_t st);
int pa_mmr_select_q16(float* out_scores, int* out_rows, const int* rows, const float* scores, const void* hi,
                      const void* lo, const float* rmeta, const float* wr, const float* wd, int Q, int m, int K,
                      int D, int nrows, hipStream_t st);
int pa_gather_rows_bf16(void* recs, const int* rows, const void* packed, long long n, int D, int nrows,
                        hipStream_t st);
int pa_gather_rows_q16(void* recs, const int* rows, const void* hi, const void* lo, const float* rmeta, long long n,
                       int D, int nrows, hipStream_t st);
int pa_mmr_select_rows_bf16(float* out_scores, int* out_pos, const void* recs, const int* slot, const float* scores,
                            const float* wr, const float* wd, int Q, int m, int K, int D, int nrecs, hipStream_t st);
int pa_mmr_select_rows_q16(float* out_scores, int* out_pos, const void* recs, const int* slot, const float* scores,
                           const float* wr, const float* wd, int Q, int m, int K, int D, int nrecs, hipStream_t st);
long long pa_q16_topk_workspace_bytes(int Q, int N);
int pa_q16_topk(float* out_scores, int* out_rows, int* unsafe, void* workspace, const void* queries_q,
                const float* qmeta, const void* hi, const void* lo, const float* rmeta, int Q, int N, int D, int K,
                const int* row_priority, const uint64_t* row_tags, const float* row_expiry,
                const int* q_min_priority, const uint64_t* q_tags, float now, int exact, hipStream_t st);
int pa_car_group();
long long pa_car_flag_bytes();
void* pa_car_alloc(long long bytes, void* handle_out);
void* pa_car_open(const void* handle);
int pa_car_close(void* p);
int pa_car_free(void* p);
int pa_car_collective(void* const* bases, int W, int rank0, int nranks_local, const void* const* ins,
                      void* const* outs, long long n4, long long cap_bytes, uint32_t* epochs, int* err, int op,
                      hipStream_t st);
int pa_car_all_reduce(void* const* bases, int W, int rank0, int nranks_local, const void* const* ins,
                      void* const* outs, long long nelem, long long cap_bytes, uint32_t* epochs, int* err,
                      int two_shot, const void* const* resids, float* const* ss, float* const* ss_zero,
                      int row_len, hipStream_t st);
}

namespace {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_gpu(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}
void check_dtype(const at::Tensor& t, at::ScalarType dt, const char* name) {
  TORCH_CHECK(t.scalar_type() == dt, name, " has dtype ", t.scalar_type(), ", expected ", dt);
}
void check_rc(int rc, const char* what) {
  TORCH_CHECK(rc == 0, what, " launch failed with code ", rc, " (",
              rc > 0 ? hipGetErrorString((hipError_t)rc) : "bad arguments", ")");
}

void rmsnorm(at::Tensor out, at::Tensor x, at::Tensor w, double eps) {
  check_gpu(out, "out"); check_gpu(x, "x"); check_gpu(w, "w");
  check_dtype(x, at::kBFloat16, "x"); check_dtype(out, at::kBFloat16, "out");
  check_dtype(w, at::kBFloat16, "w");
  const int D = x.size(-1);
  const int T = x.numel() / D;
  TORCH_CHECK(w.numel() == D && out.numel() == x.numel(), "rmsnorm shape mismatch");
  check_rc(pa_rmsnorm(out.data_ptr(), x.data_ptr(), w.data_ptr(), T, D, (float)eps, cur_stream()),
           "rmsnorm");
}

void fused_add_rmsnorm(at::Tensor out, at::Tensor resid, at::Tensor x, at::Tensor w, double eps) {
  check_gpu(out, "out"); check_gpu(resid, "resid"); check_gpu(x, "x"); check_gpu(w, "w");
  check_dtype(x, at::kBFloat16, "x"); check_dtype(resid, at::kBFloat16, "resid");
  check_dtype(out, at::kBFloat16, "out"); check_dtype(w, at::kBFloat16, "w");
  const int D = x.size(-1);
  const int T = x.numel() / D;
  TORCH_CHECK(w.numel() == D && out.numel() == x.numel() && resid.numel() == x.numel(),
              "fused_add_rmsnorm shape mismatch");
  check_rc(pa_fused_add_rmsnorm(out.data_ptr(), resid.data_ptr(), x.data_ptr(), w.data_ptr(), T,
                                D, (float)eps, cur_stream()),
           "fused_add_rmsnorm");
}

void rope_cache(at::Tensor q_out, at::Tensor k_cache, at::Tensor v_cache, at::Tensor qkv,
                at::Tensor positions, at::Tensor slot_mapping, at::Tensor cos_sin, int64_t H,
                int64_t KV, bool apply_rope) {
  check_gpu(q_out, "q_out"); check_gpu(k_cache, "k_cache"); check_gpu(v_cache, "v_cache");
  check_gpu(positions, "positions"); check_gpu(slot_mapping, "slot_mapping");
  check_gpu(cos_sin, "cos_sin");
  TORCH_CHECK(qkv.is_cuda() && qkv.stride(-1) == 1, "qkv must be a GPU tensor with unit inner stride");
  check_dtype(qkv, at::kBFloat16, "qkv"); check_dtype(q_out, at::kBFloat16, "q_out");
  check_dtype(k_cache, at::kBFloat16, "k_cache"); check_dtype(v_cache, at::kBFloat16, "v_cache");
  check_dtype(positions, at::kInt, "positions"); check_dtype(slot_mapping, at::kInt, "slot_mapping");
  check_dtype(cos_sin, at::kFloat, "cos_sin");
  const int T = qkv.size(0);
  TORCH_CHECK(qkv.size(1) >= (H + 2 * KV) * 128, "qkv too narrow");
  TORCH_CHECK(positions.numel() >= T && slot_mapping.numel() >= T, "positions/slots too short");
  TORCH_CHECK(k_cache.dim() == 5 && k_cache.size(1) == KV && k_cache.size(2) == 16 && k_cache.size(4) == 8,
              "k_cache must be [blocks, KV, 16, block, 8]");
  TORCH_CHECK(v_cache.dim() == 4 && v_cache.size(1) == KV && v_cache.size(2) == 128,
              "v_cache must be [blocks, KV, 128, block]");
  TORCH_CHECK(cos_sin.size(1) == 128, "cos_sin must be [max_pos, 128]");
  const int block = k_cache.size(3);
  check_rc(pa_rope_cache(q_out.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), qkv.data_ptr(),
                         positions.data_ptr<int>(), slot_mapping.data_ptr<int>(),
                         cos_sin.data_ptr<float>(), T, H, KV, qkv.stride(0), block,
                         apply_rope ? 1 : 0, cur_stream()),
           "rope_cache");
}

// k_cache [layers, blocks, KV, 16, 16, 8], v_cache [layers, blocks, KV, 128, 16] (one allocation each);
// n_copies: one device word; copies: device words (donor block, new block, j) x max_copies
void kv_copy(at::Tensor k_cache, at::Tensor v_cache, at::Tensor n_copies, at::Tensor copies) {
  check_gpu(k_cache, "k_cache"); check_gpu(v_cache, "v_cache");
  check_gpu(n_copies, "n_copies"); check_gpu(copies, "copies");
  check_dtype(k_cache, at::kBFloat16, "k_cache"); check_dtype(v_cache, at::kBFloat16, "v_cache");
  check_dtype(n_copies, at::kInt, "n_copies"); check_dtype(copies, at::kInt, "copies");
  TORCH_CHECK(k_cache.dim() == 6 && k_cache.size(3) == 16 && k_cache.size(4) == 16 && k_cache.size(5) == 8 &&
                  k_cache.is_contiguous(),
              "k_cache must be a contiguous [layers, blocks, KV, 16, 16, 8]");
  TORCH_CHECK(v_cache.dim() == 5 && v_cache.size(3) == 128 && v_cache.size(4) == 16 && v_cache.is_contiguous() &&
                  v_cache.size(0) == k_cache.size(0) && v_cache.size(1) == k_cache.size(1) &&
                  v_cache.size(2) == k_cache.size(2),
              "v_cache must be a contiguous [layers, blocks, KV, 128, 16] matching k_cache");
  TORCH_CHECK(n_copies.numel() >= 1, "n_copies: one int32 word");
  const int64_t max_copies = copies.numel() / 3;
  TORCH_CHECK(copies.is_contiguous() && max_copies >= 1 && max_copies <= 65535, "copies: 3 x [1, 65535] int32 words");
  const int64_t layers = k_cache.size(0), blocks = k_cache.size(1), KV = k_cache.size(2);
  TORCH_CHECK(layers * KV <= 65535 && blocks < (1ll << 31), "kv_copy: grid too large");
  check_rc(pa_kv_copy(k_cache.data_ptr(), v_cache.data_ptr(), n_copies.data_ptr<int>(), copies.data_ptr<int>(),
                      (int)max_copies, (int)layers, (int)blocks, (int)KV, (long)(blocks * KV * 2048), 16,
                      cur_stream()),
           "kv_copy");
}

// Host tier of the prefix cache (csrc/ops/kv_pages.hip): the pages of blocks ids[0:n] <-> records
// 0..n-1 of `stage` [records, layers * 2 * KV * 2048] bf16; caches as for kv_copy
static void kv_pages(at::Tensor& k_cache, at::Tensor& v_cache, at::Tensor& ids, int64_t n, at::Tensor& stage,
                     bool gather) {
  const char* name = gather ? "kv_gather_blocks" : "kv_scatter_blocks";
  check_gpu(k_cache, "k_cache"); check_gpu(v_cache, "v_cache"); check_gpu(ids, "ids"); check_gpu(stage, "stage");
  check_dtype(k_cache, at::kBFloat16, "k_cache"); check_dtype(v_cache, at::kBFloat16, "v_cache");
  check_dtype(ids, at::kInt, "ids"); check_dtype(stage, at::kBFloat16, "stage");
  TORCH_CHECK(k_cache.dim() == 6 && k_cache.size(3) == 16 && k_cache.size(4) == 16 && k_cache.size(5) == 8 &&
                  k_cache.is_contiguous(),
              "k_cache must be a contiguous [layers, blocks, KV, 16, 16, 8]");
  TORCH_CHECK(v_cache.dim() == 5 && v_cache.size(3) == 128 && v_cache.size(4) == 16 && v_cache.is_contiguous() &&
                  v_cache.size(0) == k_cache.size(0) && v_cache.size(1) == k_cache.size(1) &&
                  v_cache.size(2) == k_cache.size(2),
              "v_cache must be a contiguous [layers, blocks, KV, 128, 16] matching k_cache");
  const int64_t layers = k_cache.size(0), blocks = k_cache.size(1), KV = k_cache.size(2);
  const int64_t record = layers * 2 * KV * 2048;
  TORCH_CHECK(n >= 0 && n <= ids.numel() && ids.is_contiguous(), name, ": n must lie in [0, len(ids)]");
  TORCH_CHECK(stage.dim() == 2 && stage.size(1) == record && stage.is_contiguous() && n <= stage.size(0), name,
              ": stage must be a contiguous [>= n, layers * 2 * KV * 2048] bf16 tensor");
  TORCH_CHECK(layers * 2 <= 65535 && blocks < (1ll << 31) && n < (1ll << 31), name, ": grid too large");
  auto fn = gather ? pa_kv_gather_blocks : pa_kv_scatter_blocks;
  check_rc(fn(k_cache.data_ptr(), v_cache.data_ptr(), ids.data_ptr<int>(), (int)n, stage.data_ptr(), (int)layers,
              (int)blocks, (int)KV, (long)(blocks * KV * 2048), 16, cur_stream()),
           name);
}
void kv_gather_blocks(at::Tensor k_cache, at::Tensor v_cache, at::Tensor ids, int64_t n, at::Tensor stage) {
  kv_pages(k_cache, v_cache, ids, n, stage, true);
}
void kv_scatter_blocks(at::Tensor k_cache, at::Tensor v_cache, at::Tensor ids, int64_t n, at::Tensor stage) {
  kv_pages(k_cache, v_cache, ids, n, stage, false);
}

// hn [T, d] bf16; n_seg: one device word; segs: device words (first_row, n_rows, slot, init) x capacity;
// pool [slots, d] fp32 accumulators (csrc/ops/span_pool.hip)
void span_pool(at::Tensor hn, at::Tensor n_seg, at::Tensor segs, at::Tensor pool) {
  check_gpu(hn, "hn"); check_gpu(n_seg, "n_seg"); check_gpu(segs, "segs"); check_gpu(pool, "pool");
  check_dtype(hn, at::kBFloat16, "hn"); check_dtype(n_seg, at::kInt, "n_seg");
  check_dtype(segs, at::kInt, "segs"); check_dtype(pool, at::kFloat, "pool");
  TORCH_CHECK(hn.dim() == 2 && pool.dim() == 2, "span_pool: hn must be [T, d] and pool [slots, d]");
  const int64_t T = hn.size(0), d = hn.size(1), slots = pool.size(0);
  TORCH_CHECK_VALUE(d % 8 == 0, "span_pool: the row length ", d, " must be a multiple of 8 (16-byte loads)");
  TORCH_CHECK(pool.size(1) == d, "span_pool: pool rows have ", pool.size(1), " entries, hn rows ", d);
  TORCH_CHECK(n_seg.numel() >= 1, "n_seg: one int32 word");
  const int64_t cap = segs.numel() / 4;
  TORCH_CHECK(cap >= 1 && cap < (1ll << 31), "segs: 4 x [1, 2^31) int32 words");
  TORCH_CHECK(T < (1ll << 31) && slots < (1ll << 31) && d <= 65535ll * 1024, "span_pool: shape too large");
  TORCH_CHECK((uintptr_t)hn.data_ptr() % 16 == 0 && (uintptr_t)pool.data_ptr() % 16 == 0,
              "span_pool: hn and pool must be 16-byte aligned");
  check_rc(pa_span_pool(hn.data_ptr(), n_seg.data_ptr<int>(), segs.data_ptr<int>(), (int)cap, pool.data_ptr<float>(),
                        (int)T, (int)d, (int)slots, cur_stream()),
           "span_pool");
}

void silu_mul(at::Tensor out, at::Tensor in) {
  check_gpu(out, "out"); check_gpu(in, "in");
  check_dtype(out, at::kBFloat16, "out"); check_dtype(in, at::kBFloat16, "in");
  const int F = out.size(-1);
  const int T = out.numel() / F;
  TORCH_CHECK(in.size(-1) == 2 * F && in.numel() == 2 * out.numel(), "silu_mul shape mismatch");
  check_rc(pa_silu_mul(out.data_ptr(), in.data_ptr(), T, F, cur_stream()), "silu_mul");
}

void paged_attention(at::Tensor out, at::Tensor part_o, at::Tensor part_ml, at::Tensor q,
                     at::Tensor k_cache, at::Tensor v_cache, at::Tensor items, at::Tensor n_items,
                     at::Tensor counters, at::Tensor q_start, at::Tensor q_len,
                     at::Tensor ctx_len, at::Tensor block_table, double scale,
                     c10::optional<at::Tensor> part_size, int64_t waves) {
  for (auto* t : {&out, &part_o, &part_ml, &q, &k_cache, &v_cache, &items, &n_items, &counters,
                  &q_start, &q_len, &ctx_len, &block_table})
    check_gpu(*t, "paged_attention arg");
  check_dtype(q, at::kBFloat16, "q"); check_dtype(out, at::kBFloat16, "out");
  check_dtype(k_cache, at::kBFloat16, "k_cache"); check_dtype(v_cache, at::kBFloat16, "v_cache");
  check_dtype(part_o, at::kFloat, "part_o"); check_dtype(part_ml, at::kFloat, "part_ml");
  for (auto* t : {&items, &n_items, &counters, &q_start, &q_len, &ctx_len, &block_table})
    check_dtype(*t, at::kInt, "paged_attention int arg");
  TORCH_CHECK(q.dim() == 3 && q.size(2) == 128, "q must be [T, H, 128]");
  TORCH_CHECK(k_cache.dim() == 5 && k_cache.size(2) == 16 && k_cache.size(3) == 16 && k_cache.size(4) == 8,
              "k_cache must be [blocks, KV, 16, 16, 8]");
  TORCH_CHECK(v_cache.dim() == 4 && v_cache.size(2) == 128 && v_cache.size(3) == 16,
              "v_cache must be [blocks, KV, 128, 16]");
  const int H = q.size(1), KV = k_cache.size(1);
  TORCH_CHECK(items.dim() == 2 && items.size(1) == 4, "items must be [max_items, 4]");
  TORCH_CHECK(block_table.dim() == 2, "block_table must be [seqs, max_blocks]");
  const int max_items = items.size(0);
  TORCH_CHECK(part_o.numel() >= (int64_t)max_items * KV * 16 * 128, "part_o workspace too small");
  TORCH_CHECK(part_ml.numel() >= (int64_t)max_items * KV * 16 * 2, "part_ml workspace too small");
  TORCH_CHECK(counters.numel() >= block_table.size(0) * KV,
              "counters must hold one zero-initialised int per (sequence, KV head)");
  // split prefill items (attention.hip prefill_item_wg) take their tickets after the per-sequence
  // counters: one per (partial slot, KV head); without that room a split item computes its whole
  // key range (correct, only slower)
  int* pf_counters = counters.numel() >= (block_table.size(0) + (int64_t)max_items) * KV
                         ? counters.data_ptr<int>() + block_table.size(0) * KV
                         : nullptr;
  const float scale_log2 = (float)(scale * 1.4426950408889634);
  check_rc(pa_paged_attention(out.data_ptr(), part_o.data_ptr<float>(), part_ml.data_ptr<float>(),
                              q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                              items.data_ptr<int>(), n_items.data_ptr<int>(), max_items,
                              part_size.has_value() ? part_size->data_ptr<int>() : nullptr,
                              counters.data_ptr<int>(),
                              q_start.data_ptr<int>(), q_len.data_ptr<int>(),
                              ctx_len.data_ptr<int>(), block_table.data_ptr<int>(),
                              block_table.size(1), H, KV, scale_log2, (int)waves, pf_counters, cur_stream()),
           "paged_attention");
}

// y[M, N] = x[M, K] . w[N, K]^T for M <= 128; returns false if the shape is not handled.
bool skinny_gemm(at::Tensor y, at::Tensor x, at::Tensor w) {
  check_gpu(x, "x"); check_gpu(w, "w");
  TORCH_CHECK(y.is_cuda() && y.stride(-1) == 1, "y must be a GPU tensor with unit inner stride");
  check_dtype(x, at::kBFloat16, "x"); check_dtype(w, at::kBFloat16, "w"); check_dtype(y, at::kBFloat16, "y");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && y.dim() == 2, "skinny_gemm expects 2-D tensors");
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K && y.size(0) == M && y.size(1) == N, "skinny_gemm shape mismatch");
  const int rc = pa_skinny_gemm(y.data_ptr(), x.data_ptr(), w.data_ptr(), M, N, K, y.stride(0), cur_stream());
  TORCH_CHECK(rc >= 0, "skinny_gemm launch failed");
  return rc == 0;
}

// y = epi(rownorm(x) . W^T) on fragment-major packed weights wp [N/16, K/32, 64, 8]
// (csrc/ops/gemm_decode.hip). epi 0 plain, 1 silu(gate)*up (y has N/2 columns),
// 2 y = resid + acc. Returns false if the shape is not handled.
// With `scale` ([N] fp32, packed column order) wp holds e4m3 bytes in the same index layout
// (csrc/ops/gemm_decode_fp8.hip).
const float* fp8_scale(const at::Tensor& scale, int N) {
  check_gpu(scale, "scale");
  check_dtype(scale, at::kFloat, "scale");
  TORCH_CHECK(scale.dim() == 1 && scale.size(0) == N && scale.is_contiguous(), "scale must be contiguous [N = ", N, "]");
  return scale.data_ptr<float>();
}

bool decode_gemm_impl(at::Tensor y, at::Tensor x, at::Tensor wp, const at::Tensor* scale,
                      c10::optional<at::Tensor> resid, int64_t epi, bool norm, double eps, int64_t nt,
                      int64_t waves, int64_t splits, c10::optional<at::Tensor> ws,
                      c10::optional<at::Tensor> counters) {
  check_gpu(wp, "wp");
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.stride(1) == 1, "x must be a 2-D GPU tensor, unit inner stride");
  TORCH_CHECK(y.is_cuda() && y.dim() == 2 && y.stride(1) == 1, "y must be a 2-D GPU tensor, unit inner stride");
  check_dtype(x, at::kBFloat16, "x"); check_dtype(y, at::kBFloat16, "y");
  check_dtype(wp, scale ? at::kFloat8_e4m3fn : at::kBFloat16, "wp");
  TORCH_CHECK(wp.dim() == 4 && wp.size(2) == 64 && wp.size(3) == 8, "wp must be packed [N/16, K/32, 64, 8]");
  const int M = x.size(0), K = x.size(1), N = wp.size(0) * 16;
  TORCH_CHECK(wp.size(1) * 32 == K, "packed weight K ", wp.size(1) * 32, " != x K ", K);
  const float* sp = scale ? fp8_scale(*scale, N) : nullptr;
  TORCH_CHECK(x.stride(0) % 8 == 0 && K % 8 == 0, "x rows must be 16-byte aligned");
  const int NO = epi == 1 ? N / 2 : N;
  TORCH_CHECK(y.size(0) == M && y.size(1) == NO, "y shape [", y.size(0), ", ", y.size(1), "] != [", M, ", ", NO, "]");
  const void* rp = nullptr;
  int ldr = 0;
  if (epi == 2) {
    TORCH_CHECK(resid.has_value(), "epi=2 needs resid");
    const auto& r = *resid;
    TORCH_CHECK(r.is_cuda() && r.dim() == 2 && r.stride(1) == 1 && r.size(0) == M && r.size(1) == N,
                "resid must be [M, N] with unit inner stride");
    check_dtype(r, at::kBFloat16, "resid");
    rp = r.data_ptr();
    ldr = r.stride(0);
  }
  float* wsp = nullptr;
  long long wsn = 0;
  int* cp = nullptr;
  int cn = 0;
  if (ws.has_value() && counters.has_value()) {
    check_gpu(*ws, "ws"); check_gpu(*counters, "counters");
    check_dtype(*ws, at::kFloat, "ws"); check_dtype(*counters, at::kInt, "counters");
    wsp = ws->data_ptr<float>(); wsn = ws->numel(); cp = counters->data_ptr<int>(); cn = counters->numel();
  }
  const int rc =
      scale ? pa_decode_gemm_fp8(y.data_ptr(), x.data_ptr(), wp.data_ptr(), sp, rp, M, N, K, x.stride(0),
                                 y.stride(0), ldr, (int)epi, norm ? 1 : 0, (float)eps, (int)nt, (int)waves,
                                 (int)splits, wsp, wsn, cp, cn, cur_stream())
            : pa_decode_gemm(y.data_ptr(), x.data_ptr(), wp.data_ptr(), rp, M, N, K, x.stride(0), y.stride(0),
                             ldr, (int)epi, norm ? 1 : 0, (float)eps, (int)nt, (int)waves, (int)splits, wsp, wsn,
                             cp, cn, cur_stream());
  TORCH_CHECK(rc >= 0, "decode_gemm launch failed");
  return rc == 0;
}

bool decode_gemm(at::Tensor y, at::Tensor x, at::Tensor wp, c10::optional<at::Tensor> resid, int64_t epi,
                 bool norm, double eps, int64_t nt, int64_t waves, int64_t splits, c10::optional<at::Tensor> ws,
                 c10::optional<at::Tensor> counters) {
  return decode_gemm_impl(y, x, wp, nullptr, resid, epi, norm, eps, nt, waves, splits, ws, counters);
}

bool decode_gemm_fp8(at::Tensor y, at::Tensor x, at::Tensor wp8, at::Tensor scale, c10::optional<at::Tensor> resid,
                     int64_t epi, bool norm, double eps, int64_t nt, int64_t waves, int64_t splits,
                     c10::optional<at::Tensor> ws, c10::optional<at::Tensor> counters) {
  return decode_gemm_impl(y, x, wp8, &scale, resid, epi, norm, eps, nt, waves, splits, ws, counters);
}

// Decode QKV projection + RoPE + paged KV write (csrc/ops/gemm_decode.hip, EPI_ROPE).
void decode_qkv_rope_impl(at::Tensor x, at::Tensor wp, const at::Tensor* scale, double eps, at::Tensor q_out,
                          at::Tensor k_cache, at::Tensor v_cache, at::Tensor positions, at::Tensor slots,
                          at::Tensor cos_sin, int64_t H, int64_t KV, int64_t splits, c10::optional<at::Tensor> ws,
                          c10::optional<at::Tensor> counters) {
  check_gpu(wp, "wp"); check_gpu(q_out, "q_out"); check_gpu(k_cache, "k_cache"); check_gpu(v_cache, "v_cache");
  check_gpu(positions, "positions"); check_gpu(slots, "slots"); check_gpu(cos_sin, "cos_sin");
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.stride(1) == 1, "x must be a 2-D GPU tensor, unit inner stride");
  check_dtype(x, at::kBFloat16, "x"); check_dtype(q_out, at::kBFloat16, "q_out");
  check_dtype(wp, scale ? at::kFloat8_e4m3fn : at::kBFloat16, "wp");
  check_dtype(k_cache, at::kBFloat16, "k_cache"); check_dtype(v_cache, at::kBFloat16, "v_cache");
  check_dtype(positions, at::kInt, "positions"); check_dtype(slots, at::kInt, "slots");
  check_dtype(cos_sin, at::kFloat, "cos_sin");
  TORCH_CHECK(wp.dim() == 4 && wp.size(2) == 64 && wp.size(3) == 8, "wp must be packed [N/16, K/32, 64, 8]");
  const int M = x.size(0), K = x.size(1), N = wp.size(0) * 16;
  TORCH_CHECK(wp.size(1) * 32 == K, "packed weight K mismatch");
  const float* sp = scale ? fp8_scale(*scale, N) : nullptr;
  TORCH_CHECK(N == (H + 2 * KV) * 128, "packed QKV has ", N, " columns, expected (H + 2 KV) * 128");
  TORCH_CHECK(q_out.numel() >= (int64_t)M * H * 128, "q_out too small");
  TORCH_CHECK(positions.numel() >= M && slots.numel() >= M, "positions/slots shorter than x");
  TORCH_CHECK(cos_sin.dim() == 2 && cos_sin.size(1) == 128, "cos_sin must be [max_pos, 128]");
  TORCH_CHECK(k_cache.dim() == 5 && k_cache.size(1) == KV && k_cache.size(2) == 16 && k_cache.size(3) == 16 &&
                  k_cache.size(4) == 8, "k_cache must be [NB, KV, 16, 16, 8]");
  TORCH_CHECK(v_cache.dim() == 4 && v_cache.size(1) == KV && v_cache.size(2) == 128 && v_cache.size(3) == 16,
              "v_cache must be [NB, KV, 128, 16]");
  float* wsp = nullptr;
  long long wsn = 0;
  int* cp = nullptr;
  int cn = 0;
  if (ws.has_value() && counters.has_value()) {
    check_gpu(*ws, "ws"); check_gpu(*counters, "counters");
    check_dtype(*ws, at::kFloat, "ws"); check_dtype(*counters, at::kInt, "counters");
    wsp = ws->data_ptr<float>(); wsn = ws->numel(); cp = counters->data_ptr<int>(); cn = counters->numel();
  }
  const int rc =
      scale ? pa_decode_qkv_rope_fp8(x.data_ptr(), wp.data_ptr(), sp, M, N, K, x.stride(0), (float)eps,
                                     q_out.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                                     positions.data_ptr<int>(), slots.data_ptr<int>(), cos_sin.data_ptr<float>(),
                                     (int)H, (int)KV, 0, 0, (int)splits, wsp, wsn, cp, cn, cur_stream())
            : pa_decode_qkv_rope(x.data_ptr(), wp.data_ptr(), M, N, K, x.stride(0), (float)eps, q_out.data_ptr(),
                                 k_cache.data_ptr(), v_cache.data_ptr(), positions.data_ptr<int>(),
                                 slots.data_ptr<int>(), cos_sin.data_ptr<float>(), (int)H, (int)KV, 0, 0,
                                 (int)splits, wsp, wsn, cp, cn, cur_stream());
  check_rc(rc < 0 ? rc : (rc > 0 ? -1 : 0), "decode_qkv_rope");
}

void decode_qkv_rope(at::Tensor x, at::Tensor wp, double eps, at::Tensor q_out, at::Tensor k_cache,
                     at::Tensor v_cache, at::Tensor positions, at::Tensor slots, at::Tensor cos_sin, int64_t H,
                     int64_t KV, int64_t splits, c10::optional<at::Tensor> ws, c10::optional<at::Tensor> counters) {
  decode_qkv_rope_impl(x, wp, nullptr, eps, q_out, k_cache, v_cache, positions, slots, cos_sin, H, KV, splits, ws,
                       counters);
}

void decode_qkv_rope_fp8(at::Tensor x, at::Tensor wp8, at::Tensor scale, double eps, at::Tensor q_out,
                         at::Tensor k_cache, at::Tensor v_cache, at::Tensor positions, at::Tensor slots,
                         at::Tensor cos_sin, int64_t H, int64_t KV, int64_t splits, c10::optional<at::Tensor> ws,
                         c10::optional<at::Tensor> counters) {
  decode_qkv_rope_impl(x, wp8, &scale, eps, q_out, k_cache, v_cache, positions, slots, cos_sin, H, KV, splits, ws,
                       counters);
}

const float* opt_rows(const c10::optional<at::Tensor>& t, int M, const char* name) {
  if (!t.has_value()) return nullptr;
  check_gpu(*t, name);
  check_dtype(*t, at::kFloat, name);
  TORCH_CHECK(t->numel() >= M, name, " must hold >= M floats");
  return t->data_ptr<float>();
}

// y = epi(rowscale(x) . W^T) for mid-size token counts on packed weights (csrc/ops/gemm_mid.hip).
// epi 0 plain, 1 silu(gate)*up (y has N/2 columns), 2 resid + acc, 3 plain with the RoPE tile
// permutation undone. ss_in: [M] fp32 row sums of x^2 -> rows scaled by rsqrt(ss/K + eps) (the
// RMSNorm weight folded into W). ss_out (epi 2): [M] += row sums of y^2. ss_zero: [M] zeroed.
// Returns false if the shape/config is not handled.
bool mid_gemm(at::Tensor y, at::Tensor x, at::Tensor wp, c10::optional<at::Tensor> resid, at::Tensor ws,
              at::Tensor counters, int64_t epi, c10::optional<at::Tensor> ss_in, c10::optional<at::Tensor> ss_out,
              c10::optional<at::Tensor> ss_zero, double eps, int64_t fm, int64_t fn, int64_t splits) {
  check_gpu(wp, "wp"); check_gpu(ws, "ws"); check_gpu(counters, "counters");
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.stride(1) == 1, "x must be a 2-D GPU tensor, unit inner stride");
  TORCH_CHECK(y.is_cuda() && y.dim() == 2 && y.stride(1) == 1, "y must be a 2-D GPU tensor, unit inner stride");
  check_dtype(x, at::kBFloat16, "x"); check_dtype(wp, at::kBFloat16, "wp"); check_dtype(y, at::kBFloat16, "y");
  check_dtype(ws, at::kFloat, "ws"); check_dtype(counters, at::kInt, "counters");
  TORCH_CHECK(epi >= 0 && epi <= 3, "mid_gemm epi must be 0..3 (RoPE + KV write: mid_qkv_rope)");
  TORCH_CHECK(wp.dim() == 4 && wp.size(2) == 64 && wp.size(3) == 8, "wp must be packed [N/16, K/32, 64, 8]");
  const int M = x.size(0), K = x.size(1), N = wp.size(0) * 16;
  TORCH_CHECK(wp.size(1) * 32 == K, "packed weight K mismatch");
  TORCH_CHECK(x.stride(0) % 8 == 0 && y.stride(0) % 4 == 0, "x rows must be 16-byte, y rows 8-byte aligned");
  // the non-pair epilogues (plain, residual) of the ping-pong kernels store -- and read the
  // residual -- 16 B per lane (packed_epi.h store_pair_wide): y and resid rows 16-byte aligned
  const bool wide = epi == 0 || epi == 2;
  auto rows16 = [](const at::Tensor& t) { return t.stride(0) % 8 == 0 && ((uintptr_t)t.data_ptr() & 15) == 0; };
  TORCH_CHECK(!wide || rows16(y), "y rows must be 16-byte aligned for the plain / residual epilogue");
  TORCH_CHECK(((uintptr_t)y.data_ptr() & 7) == 0, "y must be 8-byte aligned");
  const int NO = epi == 1 ? N / 2 : N;
  TORCH_CHECK(y.size(0) == M && y.size(1) == NO, "y shape mismatch");
  const void* rp = nullptr;
  int ldr = 0;
  if (epi == 2) {
    TORCH_CHECK(resid.has_value(), "epi=2 needs resid");
    const auto& r = *resid;
    TORCH_CHECK(r.is_cuda() && r.dim() == 2 && r.stride(1) == 1 && r.size(0) == M && r.size(1) == N && rows16(r),
                "resid must be [M, N] with unit inner stride and 16-byte aligned rows");
    check_dtype(r, at::kBFloat16, "resid");
    rp = r.data_ptr();
    ldr = r.stride(0);
  }
  const int rc = pa_mid_gemm(y.data_ptr(), x.data_ptr(), wp.data_ptr(), rp, ws.data_ptr<float>(), ws.numel(),
                             counters.data_ptr<int>(), counters.numel(), M, N, K, x.stride(0), y.stride(0), ldr,
                             (int)epi, opt_rows(ss_in, M, "ss_in"), const_cast<float*>(opt_rows(ss_out, M, "ss_out")),
                             const_cast<float*>(opt_rows(ss_zero, M, "ss_zero")), (float)eps, (int)fm, (int)fn,
                             (int)splits, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, cur_stream());
  TORCH_CHECK(rc >= 0, "mid_gemm launch failed");
  return rc == 0;
}

// Mid-size QKV projection (RMSNorm folded into the rope-packed weights, row statistics
// ss_in) with RoPE and the paged KV write in the epilogue (csrc/ops/gemm_mid.hip, EP_ROPEKV).
bool mid_qkv_rope(at::Tensor x, at::Tensor wp, at::Tensor ss_in, double eps, at::Tensor q_out, at::Tensor k_cache,
                  at::Tensor v_cache, at::Tensor positions, at::Tensor slots, at::Tensor cos_sin, int64_t H,
                  int64_t KV, at::Tensor ws, at::Tensor counters, int64_t fm, int64_t fn, int64_t splits) {
  check_gpu(wp, "wp"); check_gpu(q_out, "q_out"); check_gpu(k_cache, "k_cache"); check_gpu(v_cache, "v_cache");
  check_gpu(positions, "positions"); check_gpu(slots, "slots"); check_gpu(cos_sin, "cos_sin");
  check_gpu(ws, "ws"); check_gpu(counters, "counters");
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.stride(1) == 1, "x must be a 2-D GPU tensor, unit inner stride");
  check_dtype(x, at::kBFloat16, "x"); check_dtype(wp, at::kBFloat16, "wp"); check_dtype(q_out, at::kBFloat16, "q_out");
  check_dtype(k_cache, at::kBFloat16, "k_cache"); check_dtype(v_cache, at::kBFloat16, "v_cache");
  check_dtype(positions, at::kInt, "positions"); check_dtype(slots, at::kInt, "slots");
  check_dtype(cos_sin, at::kFloat, "cos_sin");
  check_dtype(ws, at::kFloat, "ws"); check_dtype(counters, at::kInt, "counters");
  TORCH_CHECK(wp.dim() == 4 && wp.size(2) == 64 && wp.size(3) == 8, "wp must be packed [N/16, K/32, 64, 8]");
  const int M = x.size(0), K = x.size(1), N = wp.size(0) * 16;
  TORCH_CHECK(wp.size(1) * 32 == K, "packed weight K mismatch");
  TORCH_CHECK(x.stride(0) % 8 == 0, "x rows must be 16-byte aligned");
  TORCH_CHECK(N == (H + 2 * KV) * 128, "packed QKV has ", N, " columns, expected (H + 2 KV) * 128");
  TORCH_CHECK(q_out.numel() >= (int64_t)M * H * 128, "q_out too small");
  TORCH_CHECK(positions.numel() >= M && slots.numel() >= M, "positions/slots shorter than x");
  TORCH_CHECK(cos_sin.dim() == 2 && cos_sin.size(1) == 128, "cos_sin must be [max_pos, 128]");
  TORCH_CHECK(k_cache.dim() == 5 && k_cache.size(1) == KV && k_cache.size(2) == 16 && k_cache.size(3) == 16 &&
                  k_cache.size(4) == 8, "k_cache must be [NB, KV, 16, 16, 8]");
  TORCH_CHECK(v_cache.dim() == 4 && v_cache.size(1) == KV && v_cache.size(2) == 128 && v_cache.size(3) == 16,
              "v_cache must be [NB, KV, 128, 16]");
  const float* ssp = opt_rows(c10::optional<at::Tensor>(ss_in), M, "ss_in");
  const int rc = pa_mid_gemm(nullptr, x.data_ptr(), wp.data_ptr(), nullptr, ws.data_ptr<float>(), ws.numel(),
                             counters.data_ptr<int>(), counters.numel(), M, N, K, x.stride(0), 0, 0, 4, ssp, nullptr,
                             nullptr, (float)eps, (int)fm, (int)fn, (int)splits, q_out.data_ptr(), k_cache.data_ptr(),
                             v_cache.data_ptr(), positions.data_ptr<int>(), slots.data_ptr<int>(),
                             cos_sin.data_ptr<float>(), (int)H, (int)KV, cur_stream());
  TORCH_CHECK(rc >= 0, "mid_qkv_rope launch failed");
  return rc == 0;
}

// Weight-streaming projections for 16 < M <= 256 (csrc/ops/gemm_stream.hip): every epilogue
// (0 plain, 1 SwiGLU, 2 residual, 3 rope-perm, 4 RoPE + paged KV write). plan: 7 ints
// (mg, rg, tpw, wt, wk, S, D) or empty for the default decomposition.
bool stream_gemm(c10::optional<at::Tensor> y, at::Tensor x, at::Tensor wp, c10::optional<at::Tensor> resid,
                 at::Tensor ws, at::Tensor counters, at::Tensor err, int64_t epi, c10::optional<at::Tensor> ss_in,
                 c10::optional<at::Tensor> ss_out, c10::optional<at::Tensor> ss_zero, double eps,
                 std::vector<int64_t> plan, c10::optional<at::Tensor> q_out, c10::optional<at::Tensor> k_cache,
                 c10::optional<at::Tensor> v_cache, c10::optional<at::Tensor> positions,
                 c10::optional<at::Tensor> slots, c10::optional<at::Tensor> cos_sin, int64_t H, int64_t KV,
                 int64_t rel, c10::optional<at::Tensor> stamps) {
  check_gpu(wp, "wp"); check_gpu(ws, "ws"); check_gpu(counters, "counters"); check_gpu(err, "err");
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.stride(1) == 1, "x must be a 2-D GPU tensor, unit inner stride");
  check_dtype(x, at::kBFloat16, "x"); check_dtype(wp, at::kBFloat16, "wp");
  check_dtype(ws, at::kFloat, "ws"); check_dtype(counters, at::kInt, "counters"); check_dtype(err, at::kInt, "err");
  TORCH_CHECK(epi >= 0 && epi <= 4, "stream_gemm epi must be 0..4");
  TORCH_CHECK(wp.dim() == 4 && wp.size(2) == 64 && wp.size(3) == 8, "wp must be packed [N/16, K/32, 64, 8]");
  const int M = x.size(0), K = x.size(1), N = wp.size(0) * 16;
  TORCH_CHECK(wp.size(1) * 32 == K, "packed weight K mismatch");
  TORCH_CHECK(x.stride(0) % 8 == 0 && ((uintptr_t)x.data_ptr() & 15) == 0, "x rows must be 16-byte aligned");
  void* yp = nullptr;
  int ldy = 0;
  if (epi != 4) {
    TORCH_CHECK(y.has_value(), "stream_gemm needs y for epi ", epi);
    const auto& t = *y;
    TORCH_CHECK(t.is_cuda() && t.dim() == 2 && t.stride(1) == 1, "y must be a 2-D GPU tensor, unit inner stride");
    check_dtype(t, at::kBFloat16, "y");
    const int NO = epi == 1 ? N / 2 : N;
    TORCH_CHECK(t.size(0) == M && t.size(1) == NO, "y shape mismatch");
    TORCH_CHECK(t.stride(0) % 4 == 0 && ((uintptr_t)t.data_ptr() & 7) == 0, "y rows must be 8-byte aligned");
    yp = t.data_ptr();
    ldy = t.stride(0);
  }
  const void* rp = nullptr;
  int ldr = 0;
  if (epi == 2) {
    TORCH_CHECK(resid.has_value(), "epi=2 needs resid");
    const auto& r = *resid;
    TORCH_CHECK(r.is_cuda() && r.dim() == 2 && r.stride(1) == 1 && r.size(0) == M && r.size(1) == N &&
                    r.stride(0) % 4 == 0 && ((uintptr_t)r.data_ptr() & 7) == 0,
                "resid must be [M, N] with unit inner stride, 8-byte aligned rows");
    check_dtype(r, at::kBFloat16, "resid");
    rp = r.data_ptr();
    ldr = r.stride(0);
  }
  void *qp = nullptr, *kp = nullptr, *vp = nullptr;
  const int *pp = nullptr, *sp = nullptr;
  const float* cp = nullptr;
  if (epi == 4) {
    TORCH_CHECK(q_out && k_cache && v_cache && positions && slots && cos_sin, "epi=4 needs the RoPE / cache tensors");
    check_gpu(*q_out, "q_out"); check_gpu(*k_cache, "k_cache"); check_gpu(*v_cache, "v_cache");
    check_gpu(*positions, "positions"); check_gpu(*slots, "slots"); check_gpu(*cos_sin, "cos_sin");
    check_dtype(*q_out, at::kBFloat16, "q_out"); check_dtype(*k_cache, at::kBFloat16, "k_cache");
    check_dtype(*v_cache, at::kBFloat16, "v_cache"); check_dtype(*positions, at::kInt, "positions");
    check_dtype(*slots, at::kInt, "slots"); check_dtype(*cos_sin, at::kFloat, "cos_sin");
    TORCH_CHECK(N == (H + 2 * KV) * 128, "packed QKV has ", N, " columns, expected (H + 2 KV) * 128");
    TORCH_CHECK(q_out->numel() >= (int64_t)M * H * 128, "q_out too small");
    TORCH_CHECK(positions->numel() >= M && slots->numel() >= M, "positions/slots shorter than x");
    TORCH_CHECK(cos_sin->dim() == 2 && cos_sin->size(1) == 128, "cos_sin must be [max_pos, 128]");
    TORCH_CHECK(k_cache->dim() == 5 && k_cache->size(1) == KV && k_cache->size(2) == 16 && k_cache->size(3) == 16 &&
                    k_cache->size(4) == 8, "k_cache must be [NB, KV, 16, 16, 8]");
    TORCH_CHECK(v_cache->dim() == 4 && v_cache->size(1) == KV && v_cache->size(2) == 128 && v_cache->size(3) == 16,
                "v_cache must be [NB, KV, 128, 16]");
    qp = q_out->data_ptr(); kp = k_cache->data_ptr(); vp = v_cache->data_ptr();
    pp = positions->data_ptr<int>(); sp = slots->data_ptr<int>(); cp = cos_sin->data_ptr<float>();
  }
  int pl[7] = {0, 0, 0, 0, 0, 0, 0};
  if (!plan.empty()) {
    TORCH_CHECK(plan.size() == 7, "plan must be 7 ints (mg, rg, tpw, wt, wk, S, D)");
    for (int i = 0; i < 7; ++i) pl[i] = (int)plan[i];
  }
  const int rc = pa_stream_gemm(yp, x.data_ptr(), wp.data_ptr(), rp, ws.data_ptr<float>(), ws.numel(),
                                counters.data_ptr<int>(), counters.numel(), err.data_ptr<int>(), M, N, K, x.stride(0),
                                ldy, ldr, (int)epi, opt_rows(ss_in, M, "ss_in"),
                                const_cast<float*>(opt_rows(ss_out, M, "ss_out")),
                                const_cast<float*>(opt_rows(ss_zero, M, "ss_zero")), (float)eps, pl, qp, kp, vp, pp,
                                sp, cp, (int)H, (int)KV, (int)rel,
                                stamps ? reinterpret_cast<unsigned long long*>(stamps->data_ptr<int64_t>()) : nullptr,
                                cur_stream());
  TORCH_CHECK(rc >= 0, "stream_gemm launch failed");
  return rc == 0;
}

std::vector<int64_t> stream_gemm_plan(int64_t M, int64_t N, int64_t K, int64_t epi) {
  int p[7];
  pa_stream_gemm_plan((int)M, (int)N, (int)K, (int)epi, p);
  const long long ws = pa_stream_gemm_ws_floats((int)M, (int)N, (int)K, p[0], p[1], p[2], p[3], p[4], p[5]);
  return {p[0], p[1], p[2], p[3], p[4], p[5], p[6], (int64_t)ws};
}

// Large-M projections (csrc/ops/gemm_prefill.hip): 256x256 MFMA tiles on the packed
// weights with the same epilogues as mid_gemm (0 plain, 1 SwiGLU, 2 residual, 3 rope-perm).
bool prefill_gemm(at::Tensor y, at::Tensor x, at::Tensor wp, c10::optional<at::Tensor> resid, at::Tensor ws,
                  at::Tensor counters, int64_t epi, c10::optional<at::Tensor> ss_in, c10::optional<at::Tensor> ss_out,
                  c10::optional<at::Tensor> ss_zero, double eps, int64_t full, int64_t splits, int64_t bn,
                  int64_t variant) {
  check_gpu(wp, "wp"); check_gpu(ws, "ws"); check_gpu(counters, "counters");
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.stride(1) == 1, "x must be a 2-D GPU tensor, unit inner stride");
  TORCH_CHECK(y.is_cuda() && y.dim() == 2 && y.stride(1) == 1, "y must be a 2-D GPU tensor, unit inner stride");
  check_dtype(x, at::kBFloat16, "x"); check_dtype(wp, at::kBFloat16, "wp"); check_dtype(y, at::kBFloat16, "y");
  check_dtype(ws, at::kFloat, "ws"); check_dtype(counters, at::kInt, "counters");
  TORCH_CHECK(epi >= 0 && epi <= 3, "prefill_gemm epi must be 0..3 (RoPE + KV write: prefill_qkv_rope)");
  TORCH_CHECK(wp.dim() == 4 && wp.size(2) == 64 && wp.size(3) == 8, "wp must be packed [N/16, K/32, 64, 8]");
  const int M = x.size(0), K = x.size(1), N = wp.size(0) * 16;
  TORCH_CHECK(wp.size(1) * 32 == K, "packed weight K mismatch");
  TORCH_CHECK(x.stride(0) % 8 == 0 && y.stride(0) % 4 == 0, "x rows must be 16-byte, y rows 8-byte aligned");
  // the non-pair epilogues (plain, residual) of the ping-pong kernels store -- and read the
  // residual -- 16 B per lane (packed_epi.h store_pair_wide): y and resid rows 16-byte aligned
  const bool wide = epi == 0 || epi == 2;
  auto rows16 = [](const at::Tensor& t) { return t.stride(0) % 8 == 0 && ((uintptr_t)t.data_ptr() & 15) == 0; };
  TORCH_CHECK(!wide || rows16(y), "y rows must be 16-byte aligned for the plain / residual epilogue");
  TORCH_CHECK(((uintptr_t)y.data_ptr() & 7) == 0, "y must be 8-byte aligned");
  const int NO = epi == 1 ? N / 2 : N;
  TORCH_CHECK(y.size(0) == M && y.size(1) == NO, "y shape mismatch");
  const void* rp = nullptr;
  int ldr = 0;
  if (epi == 2) {
    TORCH_CHECK(resid.has_value(), "epi=2 needs resid");
    const auto& r = *resid;
    TORCH_CHECK(r.is_cuda() && r.dim() == 2 && r.stride(1) == 1 && r.size(0) == M && r.size(1) == N && rows16(r),
                "resid must be [M, N] with unit inner stride and 16-byte aligned rows");
    check_dtype(r, at::kBFloat16, "resid");
    rp = r.data_ptr();
    ldr = r.stride(0);
  }
  const int rc = pa_prefill_gemm(y.data_ptr(), x.data_ptr(), wp.data_ptr(), rp, ws.data_ptr<float>(), ws.numel(),
                                 counters.data_ptr<int>(), counters.numel(), M, N, K, x.stride(0), y.stride(0), ldr,
                                 (int)epi, opt_rows(ss_in, M, "ss_in"), const_cast<float*>(opt_rows(ss_out, M, "ss_out")),
                                 const_cast<float*>(opt_rows(ss_zero, M, "ss_zero")), (float)eps, (int)full,
                                 (int)splits, (int)bn, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0,
                                 (int)variant, cur_stream());
  TORCH_CHECK(rc >= 0, "prefill_gemm launch failed");
  return rc == 0;
}

bool prefill_qkv_rope(at::Tensor x, at::Tensor wp, at::Tensor ss_in, double eps, at::Tensor q_out, at::Tensor k_cache,
                      at::Tensor v_cache, at::Tensor positions, at::Tensor slots, at::Tensor cos_sin, int64_t H,
                      int64_t KV, at::Tensor ws, at::Tensor counters, int64_t full, int64_t splits, int64_t bn,
                      int64_t variant) {
  check_gpu(wp, "wp"); check_gpu(q_out, "q_out"); check_gpu(k_cache, "k_cache"); check_gpu(v_cache, "v_cache");
  check_gpu(positions, "positions"); check_gpu(slots, "slots"); check_gpu(cos_sin, "cos_sin");
  check_gpu(ws, "ws"); check_gpu(counters, "counters");
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.stride(1) == 1, "x must be a 2-D GPU tensor, unit inner stride");
  check_dtype(x, at::kBFloat16, "x"); check_dtype(wp, at::kBFloat16, "wp"); check_dtype(q_out, at::kBFloat16, "q_out");
  check_dtype(k_cache, at::kBFloat16, "k_cache"); check_dtype(v_cache, at::kBFloat16, "v_cache");
  check_dtype(positions, at::kInt, "positions"); check_dtype(slots, at::kInt, "slots");
  check_dtype(cos_sin, at::kFloat, "cos_sin");
  check_dtype(ws, at::kFloat, "ws"); check_dtype(counters, at::kInt, "counters");
  TORCH_CHECK(wp.dim() == 4 && wp.size(2) == 64 && wp.size(3) == 8, "wp must be packed [N/16, K/32, 64, 8]");
  const int M = x.size(0), K = x.size(1), N = wp.size(0) * 16;
  TORCH_CHECK(wp.size(1) * 32 == K, "packed weight K mismatch");
  TORCH_CHECK(x.stride(0) % 8 == 0, "x rows must be 16-byte aligned");
  TORCH_CHECK(N == (H + 2 * KV) * 128, "QKV width must be (H + 2 KV) * 128");
  TORCH_CHECK(q_out.numel() >= (int64_t)M * H * 128, "q_out too small");
  TORCH_CHECK(positions.numel() >= M && slots.numel() >= M, "positions/slots shorter than x");
  TORCH_CHECK(cos_sin.dim() == 2 && cos_sin.size(1) == 128, "cos_sin must be [max_pos, 128]");
  TORCH_CHECK(k_cache.dim() == 5 && k_cache.size(1) == KV && k_cache.size(2) == 16 && k_cache.size(3) == 16 &&
                  k_cache.size(4) == 8, "k_cache must be [NB, KV, 16, 16, 8]");
  TORCH_CHECK(v_cache.dim() == 4 && v_cache.size(1) == KV && v_cache.size(2) == 128 && v_cache.size(3) == 16,
              "v_cache must be [NB, KV, 128, 16]");
  TORCH_CHECK(ss_in.is_cuda() && ss_in.numel() >= M, "ss_in must hold M row statistics");
  check_dtype(ss_in, at::kFloat, "ss_in");
  const int rc = pa_prefill_gemm(nullptr, x.data_ptr(), wp.data_ptr(), nullptr, ws.data_ptr<float>(), ws.numel(),
                                 counters.data_ptr<int>(), counters.numel(), M, N, K, x.stride(0), 0, 0, 4,
                                 ss_in.data_ptr<float>(), nullptr, nullptr, (float)eps, (int)full, (int)splits,
                                 (int)bn, q_out.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), positions.data_ptr<int>(),
                                 slots.data_ptr<int>(), cos_sin.data_ptr<float>(), (int)H, (int)KV, (int)variant,
                                 cur_stream());
  TORCH_CHECK(rc >= 0, "prefill_qkv_rope launch failed");
  return rc == 0;
}

std::vector<int64_t> prefill_gemm_plan(int64_t M, int64_t N, int64_t K, int64_t bn) {
  int full, S;
  if (bn <= 0) bn = pa_prefill_pick_bn((int)M, (int)N);
  pa_prefill_gemm_plan((int)M, (int)N, (int)K, (int)bn, &full, &S);
  return {full, S, pa_prefill_gemm_ws_floats((int)M, (int)N, (int)bn, full, S), bn};
}

// out[m] = sum_k x[m, k]^2 (fp32)
void row_sumsq(at::Tensor out, at::Tensor x) {
  check_gpu(out, "out");
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.stride(1) == 1, "x must be a 2-D GPU tensor, unit inner stride");
  check_dtype(x, at::kBFloat16, "x"); check_dtype(out, at::kFloat, "out");
  TORCH_CHECK(out.numel() >= x.size(0), "out shorter than x");
  check_rc(pa_row_sumsq(out.data_ptr<float>(), x.data_ptr(), x.size(0), x.size(1), x.stride(0), cur_stream()),
           "row_sumsq");
}

std::vector<int64_t> mid_gemm_plan(int64_t M, int64_t N, int64_t K, int64_t epi) {
  int fm, fn, S;
  pa_mid_gemm_plan((int)M, (int)N, (int)K, (int)epi, &fm, &fn, &S);
  return {fm, fn, S, pa_mid_gemm_ws_floats((int)M, (int)N, (int)K, fm, fn, S)};
}

int64_t sample_workspace_floats(int64_t rows, int64_t V) {
  return pa_sample_workspace_floats(rows, V);
}

void patch_pending_ids(at::Tensor ids, at::Tensor sampled) {
  TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == at::kInt && ids.is_contiguous(), "ids: int32 device tensor");
  TORCH_CHECK(sampled.is_cuda() && sampled.scalar_type() == at::kInt && sampled.is_contiguous(),
              "sampled: int32 device tensor");
  check_rc(pa_patch_pending_ids(ids.data_ptr<int>(), sampled.data_ptr<int>(), (int)ids.numel(),
                                (int)sampled.numel(), cur_stream()),
           "patch_pending_ids");
}

void sample(at::Tensor out_tokens, c10::optional<at::Tensor> out_keys, at::Tensor workspace,
            at::Tensor logits, int64_t vocab_offset, at::Tensor temperature, at::Tensor mask_class,
            at::Tensor class_masks, at::Tensor seeds, at::Tensor offsets,
            c10::optional<at::Tensor> forced, c10::optional<at::Tensor> tau) {
  check_gpu(out_tokens, "out_tokens"); check_gpu(workspace, "workspace");
  check_gpu(temperature, "temperature"); check_gpu(mask_class, "mask_class");
  check_gpu(class_masks, "class_masks"); check_gpu(seeds, "seeds"); check_gpu(offsets, "offsets");
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.stride(1) == 1,
              "logits must be a 2-D GPU tensor with unit inner stride");
  check_dtype(logits, at::kBFloat16, "logits"); check_dtype(out_tokens, at::kInt, "out_tokens");
  check_dtype(workspace, at::kFloat, "workspace"); check_dtype(temperature, at::kFloat, "temperature");
  check_dtype(mask_class, at::kInt, "mask_class"); check_dtype(class_masks, at::kInt, "class_masks");
  check_dtype(seeds, at::kLong, "seeds"); check_dtype(offsets, at::kInt, "offsets");
  const int rows = logits.size(0), V = logits.size(1);
  TORCH_CHECK(out_tokens.numel() >= rows && temperature.numel() >= rows &&
                  mask_class.numel() >= rows && seeds.numel() >= rows && offsets.numel() >= rows,
              "per-row sampling parameter tensors too short");
  TORCH_CHECK(workspace.numel() >= pa_sample_workspace_floats(rows, V), "sample workspace too small");
  TORCH_CHECK(class_masks.dim() == 2, "class_masks must be [classes, words]");
  TORCH_CHECK(class_masks.size(1) * 32 >= vocab_offset + V, "class_masks too narrow for vocab");
  float* keys = nullptr;
  if (out_keys.has_value()) {
    check_gpu(*out_keys, "out_keys"); check_dtype(*out_keys, at::kFloat, "out_keys");
    keys = out_keys->data_ptr<float>();
  }
  const int* fp = nullptr;
  if (forced.has_value()) {
    check_gpu(*forced, "forced"); check_dtype(*forced, at::kInt, "forced");
    fp = forced->data_ptr<int>();
  }
  const float* tp = nullptr;
  if (tau.has_value()) {
    check_gpu(*tau, "tau"); check_dtype(*tau, at::kFloat, "tau");
    TORCH_CHECK(tau->numel() >= rows, "tau too short");
    tp = tau->data_ptr<float>();
  }
  check_rc(pa_sample(out_tokens.data_ptr<int>(), keys, workspace.data_ptr<float>(),
                     logits.data_ptr(), rows, V, logits.stride(0), vocab_offset,
                     temperature.data_ptr<float>(), mask_class.data_ptr<int>(),
                     reinterpret_cast<const uint32_t*>(class_masks.data_ptr<int>()),
                     class_masks.size(1), seeds.data_ptr<int64_t>(), offsets.data_ptr<int>(), fp,
                     tp, cur_stream()),
           "sample");
}

// The sampler's chunk pass alone (sampling.hip): fills the workspace's [rows, nchunk] partial keys
// and ids; spec_verify() merges them. Same checks as sample().
void sample_partials(at::Tensor workspace, at::Tensor logits, int64_t vocab_offset, at::Tensor temperature,
                     at::Tensor mask_class, at::Tensor class_masks, at::Tensor seeds, at::Tensor offsets,
                     c10::optional<at::Tensor> tau) {
  check_gpu(workspace, "workspace"); check_gpu(temperature, "temperature"); check_gpu(mask_class, "mask_class");
  check_gpu(class_masks, "class_masks"); check_gpu(seeds, "seeds"); check_gpu(offsets, "offsets");
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.stride(1) == 1,
              "logits must be a 2-D GPU tensor with unit inner stride");
  check_dtype(logits, at::kBFloat16, "logits"); check_dtype(workspace, at::kFloat, "workspace");
  check_dtype(temperature, at::kFloat, "temperature"); check_dtype(mask_class, at::kInt, "mask_class");
  check_dtype(class_masks, at::kInt, "class_masks"); check_dtype(seeds, at::kLong, "seeds");
  check_dtype(offsets, at::kInt, "offsets");
  const int rows = logits.size(0), V = logits.size(1);
  TORCH_CHECK(temperature.numel() >= rows && mask_class.numel() >= rows && seeds.numel() >= rows &&
                  offsets.numel() >= rows,
              "per-row sampling parameter tensors too short");
  TORCH_CHECK(workspace.is_contiguous() && workspace.numel() >= pa_sample_workspace_floats(rows, V),
              "sample workspace too small");
  TORCH_CHECK(class_masks.dim() == 2, "class_masks must be [classes, words]");
  TORCH_CHECK(class_masks.size(1) * 32 >= vocab_offset + V, "class_masks too narrow for vocab");
  const float* tp = nullptr;
  if (tau.has_value()) {
    check_gpu(*tau, "tau"); check_dtype(*tau, at::kFloat, "tau");
    TORCH_CHECK(tau->numel() >= rows, "tau too short");
    tp = tau->data_ptr<float>();
  }
  check_rc(pa_sample_partials(workspace.data_ptr<float>(), logits.data_ptr(), rows, V, logits.stride(0),
                              vocab_offset, temperature.data_ptr<float>(), mask_class.data_ptr<int>(),
                              reinterpret_cast<const uint32_t*>(class_masks.data_ptr<int>()),
                              class_masks.size(1), seeds.data_ptr<int64_t>(), offsets.data_ptr<int>(), tp,
                              cur_stream()),
           "sample_partials");
}

// Final merge + draft verification of a draft step (spec_verify.hip). part_k fp32 / part_i int32
// [rows, nchunk] contiguous; forced, logit_rows, run_first, run_len, out_tokens, accept_len hold
// at least `rows` int32 words; input_ids is the step's token ids.
void spec_verify(at::Tensor out_tokens, at::Tensor accept_len, at::Tensor part_k, at::Tensor part_i,
                 at::Tensor forced, at::Tensor input_ids, at::Tensor logit_rows, at::Tensor run_first,
                 at::Tensor run_len) {
  check_gpu(out_tokens, "out_tokens"); check_gpu(accept_len, "accept_len"); check_gpu(part_k, "part_k");
  check_gpu(part_i, "part_i"); check_gpu(forced, "forced"); check_gpu(input_ids, "input_ids");
  check_gpu(logit_rows, "logit_rows"); check_gpu(run_first, "run_first"); check_gpu(run_len, "run_len");
  check_dtype(out_tokens, at::kInt, "out_tokens"); check_dtype(accept_len, at::kInt, "accept_len");
  check_dtype(part_k, at::kFloat, "part_k"); check_dtype(part_i, at::kInt, "part_i");
  check_dtype(forced, at::kInt, "forced"); check_dtype(input_ids, at::kInt, "input_ids");
  check_dtype(logit_rows, at::kInt, "logit_rows"); check_dtype(run_first, at::kInt, "run_first");
  check_dtype(run_len, at::kInt, "run_len");
  TORCH_CHECK(part_k.dim() == 2 && part_i.dim() == 2 && part_k.sizes() == part_i.sizes() &&
                  part_k.is_contiguous() && part_i.is_contiguous() && part_k.size(1) >= 1,
              "part_k / part_i: contiguous [rows, nchunk] tensors of one shape");
  const int64_t rows = part_k.size(0), nchunk = part_k.size(1);
  TORCH_CHECK(rows * nchunk < (int64_t(1) << 31), "spec_verify: too many partials");
  for (const at::Tensor* t : {&out_tokens, &accept_len, &forced, &logit_rows, &run_first, &run_len})
    TORCH_CHECK(t->dim() == 1 && t->is_contiguous() && t->numel() >= rows,
                "spec_verify: per-row tensors must be contiguous 1-D with at least `rows` entries");
  TORCH_CHECK(input_ids.dim() == 1 && input_ids.is_contiguous() && input_ids.numel() < (int64_t(1) << 31),
              "input_ids: contiguous 1-D int32 tensor");
  check_rc(pa_spec_verify(out_tokens.data_ptr<int>(), accept_len.data_ptr<int>(), part_k.data_ptr<float>(),
                          part_i.data_ptr<int>(), forced.data_ptr<int>(), input_ids.data_ptr<int>(),
                          (int)input_ids.numel(), logit_rows.data_ptr<int>(), run_first.data_ptr<int>(),
                          run_len.data_ptr<int>(), (int)rows, (int)nchunk, cur_stream()),
           "spec_verify");
}

int64_t logprob_workspace_floats(int64_t rows, int64_t V) {
  return pa_logprob_workspace_floats(rows, V);
}

// Per-token log-probabilities behind sample() (sampling.hip logprob_*_kernel). out_lp [rows],
// top_ids / top_lp [rows, 20]: unit inner stride, any row stride (columns of one record buffer).
void token_logprobs(at::Tensor out_lp, at::Tensor top_ids, at::Tensor top_lp, at::Tensor workspace,
                    at::Tensor logits, at::Tensor tokens, at::Tensor lp_n, at::Tensor forced,
                    at::Tensor mask_class, at::Tensor class_masks) {
  check_gpu(workspace, "workspace"); check_gpu(tokens, "tokens"); check_gpu(lp_n, "lp_n");
  check_gpu(forced, "forced"); check_gpu(mask_class, "mask_class"); check_gpu(class_masks, "class_masks");
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.stride(1) == 1,
              "logits must be a 2-D GPU tensor with unit inner stride");
  check_dtype(logits, at::kBFloat16, "logits"); check_dtype(workspace, at::kFloat, "workspace");
  check_dtype(tokens, at::kInt, "tokens"); check_dtype(lp_n, at::kInt, "lp_n");
  check_dtype(forced, at::kInt, "forced"); check_dtype(mask_class, at::kInt, "mask_class");
  check_dtype(class_masks, at::kInt, "class_masks");
  check_dtype(out_lp, at::kFloat, "out_lp"); check_dtype(top_ids, at::kInt, "top_ids");
  check_dtype(top_lp, at::kFloat, "top_lp");
  const int64_t rows = logits.size(0), V = logits.size(1);
  TORCH_CHECK(out_lp.is_cuda() && out_lp.dim() == 1 && out_lp.size(0) >= rows, "out_lp: [rows] GPU tensor");
  TORCH_CHECK(top_ids.is_cuda() && top_ids.dim() == 2 && top_ids.size(0) >= rows && top_ids.size(1) == 20 &&
                  top_ids.stride(1) == 1,
              "top_ids: [rows, 20] GPU tensor with unit inner stride");
  TORCH_CHECK(top_lp.is_cuda() && top_lp.dim() == 2 && top_lp.size(0) >= rows && top_lp.size(1) == 20 &&
                  top_lp.stride(1) == 1 && top_lp.stride(0) == top_ids.stride(0),
              "top_lp: [rows, 20] GPU tensor laid out like top_ids");
  TORCH_CHECK(rows == 0 || (out_lp.stride(0) >= 1 && top_ids.stride(0) >= 20), "logprob outputs overlap");
  TORCH_CHECK(tokens.numel() >= rows && lp_n.numel() >= rows && forced.numel() >= rows &&
                  mask_class.numel() >= rows,
              "per-row logprob parameter tensors too short");
  const int64_t ld = rows > 1 ? logits.stride(0) : V;  // a one-row view's stride is arbitrary
  TORCH_CHECK(V > 0 && V % 8 == 0 && ld % 8 == 0 && ld >= V, "logits: V and the row stride must be multiples of 8");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(logits.data_ptr()) & 15) == 0,
              "logits must start 16-byte aligned (rows are read as 16-byte vectors)");
  TORCH_CHECK(V <= 64 * 4096, "token_logprobs supports vocabularies up to 262144 entries");
  TORCH_CHECK(workspace.numel() >= pa_logprob_workspace_floats(rows, V), "logprob workspace too small");
  TORCH_CHECK(class_masks.dim() == 2 && class_masks.is_contiguous(), "class_masks must be [classes, words]");
  TORCH_CHECK(class_masks.size(1) * 32 >= V, "class_masks too narrow for vocab");
  check_rc(pa_token_logprobs(out_lp.data_ptr<float>(), (int)out_lp.stride(0), top_ids.data_ptr<int>(),
                             top_lp.data_ptr<float>(), (int)top_ids.stride(0), workspace.data_ptr<float>(),
                             logits.data_ptr(), (int)rows, (int)V, (int)ld,
                             tokens.data_ptr<int>(), lp_n.data_ptr<int>(), forced.data_ptr<int>(),
                             mask_class.data_ptr<int>(),
                             reinterpret_cast<const uint32_t*>(class_masks.data_ptr<int>()),
                             (int)class_masks.size(1), cur_stream()),
             "token_logprobs");
}

int64_t score_workspace_floats(int64_t rows, int64_t V) { return pa_score_workspace_floats(rows, V); }

// Prompt scoring (scoring.hip): logprob, rank and top-20 of target[row] per logit row. out_lp /
// out_rank [rows] with one common stride, top_ids / top_lp [rows, 20]: unit inner stride, any
// row stride (columns of one record buffer). Rows with target < 0 are left untouched.
void score_tokens(at::Tensor out_lp, at::Tensor out_rank, at::Tensor top_ids, at::Tensor top_lp,
                  at::Tensor workspace, at::Tensor logits, at::Tensor target, at::Tensor lp_n) {
  check_gpu(workspace, "workspace"); check_gpu(target, "target"); check_gpu(lp_n, "lp_n");
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.stride(1) == 1,
              "logits must be a 2-D GPU tensor with unit inner stride");
  check_dtype(logits, at::kBFloat16, "logits"); check_dtype(workspace, at::kFloat, "workspace");
  check_dtype(target, at::kInt, "target"); check_dtype(lp_n, at::kInt, "lp_n");
  check_dtype(out_lp, at::kFloat, "out_lp"); check_dtype(out_rank, at::kInt, "out_rank");
  check_dtype(top_ids, at::kInt, "top_ids"); check_dtype(top_lp, at::kFloat, "top_lp");
  const int64_t rows = logits.size(0), V = logits.size(1);
  TORCH_CHECK(out_lp.is_cuda() && out_lp.dim() == 1 && out_lp.size(0) >= rows, "out_lp: [rows] GPU tensor");
  TORCH_CHECK(out_rank.is_cuda() && out_rank.dim() == 1 && out_rank.size(0) >= rows &&
                  (rows <= 1 || out_rank.stride(0) == out_lp.stride(0)),
              "out_rank: [rows] GPU tensor laid out like out_lp");
  TORCH_CHECK(top_ids.is_cuda() && top_ids.dim() == 2 && top_ids.size(0) >= rows && top_ids.size(1) == 20 &&
                  top_ids.stride(1) == 1,
              "top_ids: [rows, 20] GPU tensor with unit inner stride");
  TORCH_CHECK(top_lp.is_cuda() && top_lp.dim() == 2 && top_lp.size(0) >= rows && top_lp.size(1) == 20 &&
                  top_lp.stride(1) == 1 && top_lp.stride(0) == top_ids.stride(0),
              "top_lp: [rows, 20] GPU tensor laid out like top_ids");
  TORCH_CHECK(rows == 0 || (out_lp.stride(0) >= 1 && top_ids.stride(0) >= 20), "score outputs overlap");
  TORCH_CHECK(target.numel() >= rows && lp_n.numel() >= rows, "per-row score parameter tensors too short");
  TORCH_CHECK(target.is_contiguous() && lp_n.is_contiguous(), "target / lp_n must be contiguous");
  const int64_t ld = rows > 1 ? logits.stride(0) : V;  // a one-row view's stride is arbitrary
  TORCH_CHECK(V > 0 && V % 8 == 0 && ld % 8 == 0 && ld >= V, "logits: V and the row stride must be multiples of 8");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(logits.data_ptr()) & 15) == 0,
              "logits must start 16-byte aligned (rows are read as 16-byte vectors)");
  TORCH_CHECK(V <= 64 * 4096, "score_tokens supports vocabularies up to 262144 entries");
  TORCH_CHECK(workspace.numel() >= pa_score_workspace_floats(rows, V), "score workspace too small");
  TORCH_CHECK(workspace.is_contiguous(), "score workspace must be contiguous");
  check_rc(pa_score_tokens(out_lp.data_ptr<float>(), out_rank.data_ptr<int>(), (int)out_lp.stride(0),
                           top_ids.data_ptr<int>(), top_lp.data_ptr<float>(), (int)top_ids.stride(0),
                           workspace.data_ptr<float>(), logits.data_ptr(), (int)rows, (int)V, (int)ld,
                           target.data_ptr<int>(), lp_n.data_ptr<int>(), cur_stream()),
           "score_tokens");
}

// Presence / frequency penalties on the logits of the penalised sampling rows (penalties.hip):
// counts [slots, V], distinct [slots, cap], n_distinct [slots] are the per-slot device state.
void apply_penalties(at::Tensor logits, at::Tensor counts, at::Tensor distinct, at::Tensor n_distinct,
                     at::Tensor pen_slot, at::Tensor pen_reset, at::Tensor presence, at::Tensor frequency,
                     at::Tensor forced, at::Tensor pair_start, at::Tensor pair_n, at::Tensor pair_tok) {
  check_gpu(counts, "counts"); check_gpu(distinct, "distinct"); check_gpu(n_distinct, "n_distinct");
  check_gpu(pen_slot, "pen_slot"); check_gpu(pen_reset, "pen_reset"); check_gpu(presence, "presence");
  check_gpu(frequency, "frequency"); check_gpu(forced, "forced"); check_gpu(pair_start, "pair_start");
  check_gpu(pair_n, "pair_n"); check_gpu(pair_tok, "pair_tok");
  check_dtype(counts, at::kInt, "counts"); check_dtype(distinct, at::kInt, "distinct");
  check_dtype(n_distinct, at::kInt, "n_distinct"); check_dtype(pen_slot, at::kInt, "pen_slot");
  check_dtype(pen_reset, at::kInt, "pen_reset"); check_dtype(presence, at::kFloat, "presence");
  check_dtype(frequency, at::kFloat, "frequency"); check_dtype(forced, at::kInt, "forced");
  check_dtype(pair_start, at::kInt, "pair_start"); check_dtype(pair_n, at::kInt, "pair_n");
  check_dtype(pair_tok, at::kInt, "pair_tok");
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.scalar_type() == at::kBFloat16 &&
                  (logits.size(1) == 1 || logits.stride(1) == 1),
              "logits: [rows, V] bf16 GPU tensor with unit inner stride");
  const int64_t rows = logits.size(0), V = logits.size(1);
  TORCH_CHECK(counts.dim() == 2 && counts.size(1) == V, "counts must be [slots, V]");
  const int64_t slots = counts.size(0);
  TORCH_CHECK(distinct.dim() == 2 && distinct.size(0) == slots && distinct.size(1) >= 1,
              "distinct must be [slots, cap]");
  TORCH_CHECK(n_distinct.numel() == slots, "n_distinct must be [slots]");
  TORCH_CHECK(slots >= 1 && slots * V < (int64_t(1) << 40), "penalty state too large");
  TORCH_CHECK(pen_slot.numel() >= rows && pen_reset.numel() >= rows && presence.numel() >= rows &&
                  frequency.numel() >= rows && forced.numel() >= rows && pair_start.numel() >= rows &&
                  pair_n.numel() >= rows,
              "per-row penalty parameter tensors too short");
  const int64_t ld = rows > 1 ? logits.stride(0) : V;  // a one-row view's stride is arbitrary
  TORCH_CHECK(ld >= V && rows * ld < (int64_t(1) << 40) && pair_tok.numel() < (int64_t(1) << 31),
              "logits row stride / pair list out of range");
  check_rc(pa_apply_penalties(logits.data_ptr(), (int)rows, (int)V, (int)ld, counts.data_ptr<int>(),
                              distinct.data_ptr<int>(), n_distinct.data_ptr<int>(), (int)slots,
                              (int)distinct.size(1), pen_slot.data_ptr<int>(), pen_reset.data_ptr<int>(),
                              presence.data_ptr<float>(), frequency.data_ptr<float>(), forced.data_ptr<int>(),
                              pair_start.data_ptr<int>(), pair_n.data_ptr<int>(), pair_tok.data_ptr<int>(),
                              (int)pair_tok.numel(), cur_stream()),
           "apply_penalties");
}

// Repetition penalty on the logits of the sampling rows that carry one (repetition.hip): seen
// [slots, ceil(V / 32)] membership bits, seen_list [slots, cap], n_seen [slots] are the per-slot
// device state.
void apply_repetition_penalty(at::Tensor logits, at::Tensor seen, at::Tensor seen_list, at::Tensor n_seen,
                              at::Tensor rep_slot, at::Tensor rep_reset, at::Tensor rep_r, at::Tensor rep_inv_r,
                              at::Tensor forced, at::Tensor rep_start, at::Tensor rep_n, at::Tensor rep_tok) {
  check_gpu(seen, "seen"); check_gpu(seen_list, "seen_list"); check_gpu(n_seen, "n_seen");
  check_gpu(rep_slot, "rep_slot"); check_gpu(rep_reset, "rep_reset"); check_gpu(rep_r, "rep_r");
  check_gpu(rep_inv_r, "rep_inv_r"); check_gpu(forced, "forced"); check_gpu(rep_start, "rep_start");
  check_gpu(rep_n, "rep_n"); check_gpu(rep_tok, "rep_tok");
  check_dtype(seen, at::kInt, "seen"); check_dtype(seen_list, at::kInt, "seen_list");
  check_dtype(n_seen, at::kInt, "n_seen"); check_dtype(rep_slot, at::kInt, "rep_slot");
  check_dtype(rep_reset, at::kInt, "rep_reset"); check_dtype(rep_r, at::kFloat, "rep_r");
  check_dtype(rep_inv_r, at::kFloat, "rep_inv_r"); check_dtype(forced, at::kInt, "forced");
  check_dtype(rep_start, at::kInt, "rep_start"); check_dtype(rep_n, at::kInt, "rep_n");
  check_dtype(rep_tok, at::kInt, "rep_tok");
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.scalar_type() == at::kBFloat16 &&
                  (logits.size(1) == 1 || logits.stride(1) == 1),
              "logits: [rows, V] bf16 GPU tensor with unit inner stride");
  const int64_t rows = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V > 0 && V < (int64_t(1) << 31), "logits: vocabulary out of range");
  TORCH_CHECK(seen.dim() == 2 && seen.is_contiguous() && seen.size(1) == (V + 31) / 32,
              "seen must be [slots, ceil(V / 32)]");
  const int64_t slots = seen.size(0);
  TORCH_CHECK(seen_list.dim() == 2 && seen_list.is_contiguous() && seen_list.size(0) == slots &&
                  seen_list.size(1) >= 1 && seen_list.size(1) < (int64_t(1) << 31),
              "seen_list must be [slots, cap]");
  TORCH_CHECK(n_seen.numel() == slots && n_seen.is_contiguous(), "n_seen must be [slots]");
  TORCH_CHECK(slots >= 1 && slots < (int64_t(1) << 31), "repetition state: slots out of range");
  TORCH_CHECK(rep_slot.numel() >= rows && rep_reset.numel() >= rows && rep_r.numel() >= rows &&
                  rep_inv_r.numel() >= rows && forced.numel() >= rows && rep_start.numel() >= rows &&
                  rep_n.numel() >= rows,
              "per-row repetition parameter tensors too short");
  const int64_t ld = rows > 1 ? logits.stride(0) : V;  // a one-row view's stride is arbitrary
  TORCH_CHECK(ld >= V && rows * ld < (int64_t(1) << 40) && rep_tok.numel() < (int64_t(1) << 31),
              "logits row stride / token list out of range");
  check_rc(pa_apply_repetition_penalty(
               logits.data_ptr(), (int)rows, (int)V, (int)ld, reinterpret_cast<uint32_t*>(seen.data_ptr<int>()),
               (int)seen.size(1), seen_list.data_ptr<int>(), n_seen.data_ptr<int>(), (int)slots,
               (int)seen_list.size(1), rep_slot.data_ptr<int>(), rep_reset.data_ptr<int>(),
               rep_r.data_ptr<float>(), rep_inv_r.data_ptr<float>(), forced.data_ptr<int>(),
               rep_start.data_ptr<int>(), rep_n.data_ptr<int>(), rep_tok.data_ptr<int>(), (int)rep_tok.numel(),
               cur_stream()),
           "apply_repetition_penalty");
}

// logit_bias on the logits of the sampling rows (logit_shaping.hip): row r adds bias_val[i] to
// logit[bias_tok[i]] for i in [bias_start[r], bias_start[r] + bias_n[r]).
void apply_logit_bias(at::Tensor logits, at::Tensor bias_start, at::Tensor bias_n, at::Tensor bias_tok,
                      at::Tensor bias_val, at::Tensor forced) {
  check_gpu(bias_start, "bias_start"); check_gpu(bias_n, "bias_n"); check_gpu(bias_tok, "bias_tok");
  check_gpu(bias_val, "bias_val"); check_gpu(forced, "forced");
  check_dtype(bias_start, at::kInt, "bias_start"); check_dtype(bias_n, at::kInt, "bias_n");
  check_dtype(bias_tok, at::kInt, "bias_tok"); check_dtype(bias_val, at::kFloat, "bias_val");
  check_dtype(forced, at::kInt, "forced");
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.scalar_type() == at::kBFloat16 &&
                  (logits.size(1) == 1 || logits.stride(1) == 1),
              "logits: [rows, V] bf16 GPU tensor with unit inner stride");
  const int64_t rows = logits.size(0), V = logits.size(1);
  TORCH_CHECK(bias_start.numel() >= rows && bias_n.numel() >= rows && forced.numel() >= rows,
              "per-row bias parameter tensors too short");
  TORCH_CHECK(bias_val.numel() >= bias_tok.numel() && bias_tok.numel() < (int64_t(1) << 31),
              "bias_val must be as long as bias_tok");
  const int64_t ld = rows > 1 ? logits.stride(0) : V;  // a one-row view's stride is arbitrary
  TORCH_CHECK(V > 0 && V < (int64_t(1) << 31) && ld >= V && rows * ld < (int64_t(1) << 40),
              "logits row stride out of range");
  check_rc(pa_apply_logit_bias(logits.data_ptr(), (int)rows, (int)V, (int)ld, bias_start.data_ptr<int>(),
                               bias_n.data_ptr<int>(), bias_tok.data_ptr<int>(), bias_val.data_ptr<float>(),
                               (int)bias_tok.numel(), forced.data_ptr<int>(), cur_stream()),
           "apply_logit_bias");
}

// min_p threshold of the sampling rows (logit_shaping.hip): tau[r] = max(tau[r], tau_mp) when
// has_tau (tau holds the step's top-k / top-p thresholds), else tau[r] = tau_mp or -inf.
void minp_threshold(at::Tensor tau, bool has_tau, at::Tensor logits, at::Tensor temperature, at::Tensor min_p,
                    at::Tensor ln_min_p, at::Tensor forced, at::Tensor mask_class, at::Tensor class_masks) {
  for (auto* t : {&tau, &temperature, &min_p, &ln_min_p, &forced, &mask_class, &class_masks})
    check_gpu(*t, "minp_threshold arg");
  check_dtype(tau, at::kFloat, "tau"); check_dtype(logits, at::kBFloat16, "logits");
  check_dtype(temperature, at::kFloat, "temperature"); check_dtype(min_p, at::kFloat, "min_p");
  check_dtype(ln_min_p, at::kFloat, "ln_min_p"); check_dtype(forced, at::kInt, "forced");
  check_dtype(mask_class, at::kInt, "mask_class"); check_dtype(class_masks, at::kInt, "class_masks");
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && (logits.size(1) == 1 || logits.stride(1) == 1),
              "logits: [rows, V] bf16 GPU tensor with unit inner stride");
  const int64_t rows = logits.size(0), V = logits.size(1);
  TORCH_CHECK(tau.is_contiguous() && tau.numel() >= rows && temperature.numel() >= rows &&
                  min_p.numel() >= rows && ln_min_p.numel() >= rows && forced.numel() >= rows &&
                  mask_class.numel() >= rows,
              "per-row min_p parameter tensors too short");
  const int64_t ld = rows > 1 ? logits.stride(0) : V;  // a one-row view's stride is arbitrary
  TORCH_CHECK(V > 0 && V < (int64_t(1) << 31) && ld >= V && rows * ld < (int64_t(1) << 40),
              "logits row stride out of range");
  TORCH_CHECK(class_masks.dim() == 2 && class_masks.is_contiguous() && class_masks.size(1) * 32 >= V,
              "class_masks must be [classes, words] and cover the vocabulary");
  check_rc(pa_minp_threshold(tau.data_ptr<float>(), has_tau ? 1 : 0, logits.data_ptr(), (int)rows, (int)V,
                             (int)ld, temperature.data_ptr<float>(), min_p.data_ptr<float>(),
                             ln_min_p.data_ptr<float>(), forced.data_ptr<int>(), mask_class.data_ptr<int>(),
                             reinterpret_cast<const uint32_t*>(class_masks.data_ptr<int>()),
                             (int)class_masks.size(1), (int)class_masks.size(0), cur_stream()),
           "minp_threshold");
}

int64_t cosine_topk_workspace_bytes(int64_t Q, int64_t N, int64_t K) {
  return pa_cosine_topk_workspace_bytes(Q, N, K);
}

void cosine_topk(at::Tensor out_scores, at::Tensor out_rows, at::Tensor workspace,
                 at::Tensor queries, at::Tensor index, int64_t n_valid, int64_t K,
                 at::Tensor row_priority, at::Tensor row_tags, at::Tensor row_expiry,
                 at::Tensor q_min_priority, at::Tensor q_tags, double now) {
  for (auto* t : {&out_scores, &out_rows, &workspace, &queries, &index, &row_priority, &row_tags,
                  &row_expiry, &q_min_priority, &q_tags})
    check_gpu(*t, "cosine_topk arg");
  check_dtype(queries, at::kBFloat16, "queries"); check_dtype(index, at::kBFloat16, "index");
  check_dtype(out_scores, at::kFloat, "out_scores"); check_dtype(out_rows, at::kInt, "out_rows");
  check_dtype(row_priority, at::kInt, "row_priority"); check_dtype(row_tags, at::kLong, "row_tags");
  check_dtype(row_expiry, at::kFloat, "row_expiry");
  check_dtype(q_min_priority, at::kInt, "q_min_priority"); check_dtype(q_tags, at::kLong, "q_tags");
  TORCH_CHECK(index.dim() == 4 && index.size(2) == 64 && index.size(3) == 8,
              "index must be packed in 16-row tiles [N/16, D/32, 64, 8] (memory/semantic_index.py)");
  const int Q = queries.size(0), N = index.size(0) * 16, D = index.size(1) * 32;
  TORCH_CHECK(queries.dim() == 2 && queries.size(1) == D, "queries [Q, D] and the index must agree on D");
  TORCH_CHECK(Q <= 64, "cosine_topk takes at most 64 queries per call (ops.cosine_topk chunks larger batches)");
  TORCH_CHECK(n_valid <= N, "n_valid exceeds index rows");
  TORCH_CHECK(row_priority.numel() >= n_valid && row_tags.numel() >= n_valid && row_expiry.numel() >= n_valid,
              "row metadata shorter than n_valid");
  TORCH_CHECK(queries.is_contiguous(), "queries must be contiguous");
  TORCH_CHECK(out_scores.numel() >= (int64_t)Q * K && out_rows.numel() >= (int64_t)Q * K,
              "output too small");
  TORCH_CHECK(workspace.numel() * workspace.element_size() >=
                  pa_cosine_topk_workspace_bytes(Q, n_valid, K),
              "cosine_topk workspace too small");
  check_rc(pa_cosine_topk(out_scores.data_ptr<float>(), out_rows.data_ptr<int>(),
                          workspace.data_ptr(), queries.data_ptr(), index.data_ptr(), Q,
                          (int)n_valid, D, K, row_priority.data_ptr<int>(),
                          reinterpret_cast<const uint64_t*>(row_tags.data_ptr<int64_t>()),
                          row_expiry.data_ptr<float>(), q_min_priority.data_ptr<int>(),
                          reinterpret_cast<const uint64_t*>(q_tags.data_ptr<int64_t>()),
                          (float)now, (int)n_valid, cur_stream()),
           "cosine_topk");
}

int64_t q16_topk_workspace_bytes(int64_t Q, int64_t N) { return pa_q16_topk_workspace_bytes(Q, N); }

// Two-stage exact top-k over the 16-bit fixed-point index (csrc/ops/similarity_q16.hip).
void q16_topk(at::Tensor out_scores, at::Tensor out_rows, at::Tensor unsafe, at::Tensor workspace,
              at::Tensor queries_q, at::Tensor qmeta, at::Tensor hi, at::Tensor lo, at::Tensor rmeta, int64_t n_valid,
              int64_t K, at::Tensor row_priority, at::Tensor row_tags, at::Tensor row_expiry,
              at::Tensor q_min_priority, at::Tensor q_tags, double now, int64_t exact) {
  for (auto* t : {&out_scores, &out_rows, &unsafe, &workspace, &queries_q, &qmeta, &hi, &lo, &rmeta, &row_priority,
                  &row_tags, &row_expiry, &q_min_priority, &q_tags})
    check_gpu(*t, "q16_topk arg");
  check_dtype(queries_q, at::kChar, "queries_q"); check_dtype(hi, at::kChar, "hi"); check_dtype(lo, at::kChar, "lo");
  check_dtype(qmeta, at::kFloat, "qmeta"); check_dtype(rmeta, at::kFloat, "rmeta");
  check_dtype(out_scores, at::kFloat, "out_scores"); check_dtype(out_rows, at::kInt, "out_rows");
  check_dtype(unsafe, at::kInt, "unsafe");
  check_dtype(row_priority, at::kInt, "row_priority"); check_dtype(row_tags, at::kLong, "row_tags");
  check_dtype(row_expiry, at::kFloat, "row_expiry");
  check_dtype(q_min_priority, at::kInt, "q_min_priority"); check_dtype(q_tags, at::kLong, "q_tags");
  TORCH_CHECK(hi.dim() == 4 && hi.size(2) == 64 && hi.size(3) == 16 && lo.sizes() == hi.sizes(),
              "hi / lo must be int8 planes [N/16, D/64, 64, 16] (memory/semantic_index.py storage='q16')");
  const int64_t N = hi.size(0) * 16, D = hi.size(1) * 64;
  const int64_t Q = queries_q.size(0);
  TORCH_CHECK(queries_q.dim() == 3 && queries_q.size(1) == 2 && queries_q.size(2) == D, "queries_q [Q, 2, D]");
  TORCH_CHECK(Q <= 64, "q16_topk takes at most 64 queries per call");
  TORCH_CHECK(qmeta.numel() >= 2 * Q && rmeta.numel() >= 2 * n_valid, "qmeta [Q, 2] / rmeta [N, 2] too short");
  TORCH_CHECK(n_valid <= N, "n_valid exceeds index rows");
  TORCH_CHECK(row_priority.numel() >= n_valid && row_tags.numel() >= n_valid && row_expiry.numel() >= n_valid,
              "row metadata shorter than n_valid");
  TORCH_CHECK(out_scores.numel() >= Q * K && out_rows.numel() >= Q * K && unsafe.numel() >= Q, "output too small");
  TORCH_CHECK(workspace.numel() * workspace.element_size() >= pa_q16_topk_workspace_bytes(Q, n_valid),
              "q16_topk workspace too small");
  check_rc(pa_q16_topk(out_scores.data_ptr<float>(), out_rows.data_ptr<int>(), unsafe.data_ptr<int>(),
                       workspace.data_ptr(), queries_q.data_ptr(), qmeta.data_ptr<float>(), hi.data_ptr(),
                       lo.data_ptr(), rmeta.data_ptr<float>(), (int)Q, (int)n_valid, (int)D, (int)K,
                       row_priority.data_ptr<int>(), reinterpret_cast<const uint64_t*>(row_tags.data_ptr<int64_t>()),
                       row_expiry.data_ptr<float>(), q_min_priority.data_ptr<int>(),
                       reinterpret_cast<const uint64_t*>(q_tags.data_ptr<int64_t>()), (float)now, (int)exact,
                       cur_stream()),
           "q16_topk");
}

// MMR re-ranking of a scan's candidate lists (csrc/ops/similarity_mmr.hip). `planes`: the bf16
// index's packed tiles, or the q16 index's hi / lo planes with rmeta.
void mmr_check_lists(const at::Tensor& out_scores, const at::Tensor& out_rows, const at::Tensor& rows,
                     const at::Tensor& scores, const at::Tensor& wr, const at::Tensor& wd, int64_t K) {
  check_dtype(out_scores, at::kFloat, "out_scores"); check_dtype(out_rows, at::kInt, "out_rows");
  check_dtype(rows, at::kInt, "rows"); check_dtype(scores, at::kFloat, "scores");
  check_dtype(wr, at::kFloat, "wr"); check_dtype(wd, at::kFloat, "wd");
  TORCH_CHECK(rows.dim() == 2 && scores.sizes() == rows.sizes(), "rows / scores must be [Q, m]");
  TORCH_CHECK(rows.is_contiguous() && scores.is_contiguous() && out_scores.is_contiguous() &&
                  out_rows.is_contiguous() && wr.is_contiguous() && wd.is_contiguous(),
              "mmr_select tensors must be contiguous");
  const int64_t Q = rows.size(0), m = rows.size(1);
  TORCH_CHECK(m >= 1 && m <= 64 && K >= 1 && K <= 64, "mmr_select takes 1..64 candidates and picks per query");
  TORCH_CHECK(wr.numel() >= Q && wd.numel() >= Q, "wr / wd must be [Q]");
  TORCH_CHECK(out_scores.numel() >= Q * K && out_rows.numel() >= Q * K, "output too small");
}

void mmr_select_bf16(at::Tensor out_scores, at::Tensor out_rows, at::Tensor rows, at::Tensor scores,
                     at::Tensor packed, at::Tensor wr, at::Tensor wd, int64_t K) {
  for (auto* t : {&out_scores, &out_rows, &rows, &scores, &packed, &wr, &wd}) check_gpu(*t, "mmr_select_bf16 arg");
  mmr_check_lists(out_scores, out_rows, rows, scores, wr, wd, K);
  check_dtype(packed, at::kBFloat16, "packed");
  TORCH_CHECK(packed.dim() == 4 && packed.size(2) == 64 && packed.size(3) == 8 && packed.is_contiguous(),
              "packed must be bf16 tiles [N/16, D/32, 64, 8] (memory/semantic_index.py)");
  check_rc(pa_mmr_select_bf16(out_scores.data_ptr<float>(), out_rows.data_ptr<int>(), rows.data_ptr<int>(),
                              scores.data_ptr<float>(), packed.data_ptr(), wr.data_ptr<float>(),
                              wd.data_ptr<float>(), (int)rows.size(0), (int)rows.size(1), (int)K,
                              (int)(packed.size(1) * 32), (int)(packed.size(0) * 16), cur_stream()),
           "mmr_select_bf16");
}

void mmr_select_q16(at::Tensor out_scores, at::Tensor out_rows, at::Tensor rows, at::Tensor scores, at::Tensor hi,
                    at::Tensor lo, at::Tensor rmeta, at::Tensor wr, at::Tensor wd, int64_t K) {
  for (auto* t : {&out_scores, &out_rows, &rows, &scores, &hi, &lo, &rmeta, &wr, &wd})
    check_gpu(*t, "mmr_select_q16 arg");
  mmr_check_lists(out_scores, out_rows, rows, scores, wr, wd, K);
  check_dtype(hi, at::kChar, "hi"); check_dtype(lo, at::kChar, "lo"); check_dtype(rmeta, at::kFloat, "rmeta");
  TORCH_CHECK(hi.dim() == 4 && hi.size(2) == 64 && hi.size(3) == 16 && lo.sizes() == hi.sizes() &&
                  hi.is_contiguous() && lo.is_contiguous(),
              "hi / lo must be int8 planes [N/16, D/64, 64, 16] (memory/semantic_index.py storage='q16')");
  TORCH_CHECK(rmeta.dim() == 2 && rmeta.size(1) == 2 && rmeta.is_contiguous(), "rmeta must be [N, 2]");
  // a row id is followed only if both its tile and its scale exist
  const int64_t nrows = std::min<int64_t>(hi.size(0) * 16, rmeta.size(0));
  check_rc(pa_mmr_select_q16(out_scores.data_ptr<float>(), out_rows.data_ptr<int>(), rows.data_ptr<int>(),
                             scores.data_ptr<float>(), hi.data_ptr(), lo.data_ptr(), rmeta.data_ptr<float>(),
                             wr.data_ptr<float>(), wd.data_ptr<float>(), (int)rows.size(0), (int)rows.size(1), (int)K,
                             (int)(hi.size(1) * 64), (int)nrows, cur_stream()),
           "mmr_select_q16");
}

// Exchange records of stored rows (csrc/ops/similarity_mmr_rows.hip): recs [n, rowbytes] uint8,
// rowbytes = 2 D (bf16) or 2 D + 16 (q16). `rows` come from another rank: any value is allowed,
// ids outside the planes give zero records.
void gather_check(const at::Tensor& recs, const at::Tensor& rows, int64_t rowbytes) {
  check_dtype(recs, at::kByte, "recs"); check_dtype(rows, at::kInt, "rows");
  TORCH_CHECK(rows.dim() == 1 && rows.is_contiguous(), "rows must be a contiguous [n] int32 tensor");
  TORCH_CHECK(recs.dim() == 2 && recs.is_contiguous() && recs.size(0) == rows.size(0) && recs.size(1) == rowbytes,
              "recs must be a contiguous [n, ", rowbytes, "] uint8 tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(recs.data_ptr()) % 16 == 0, "recs must be 16-byte aligned");
}

void gather_rows_bf16(at::Tensor recs, at::Tensor rows, at::Tensor packed) {
  for (auto* t : {&recs, &rows, &packed}) check_gpu(*t, "gather_rows_bf16 arg");
  check_dtype(packed, at::kBFloat16, "packed");
  TORCH_CHECK(packed.dim() == 4 && packed.size(2) == 64 && packed.size(3) == 8 && packed.is_contiguous(),
              "packed must be bf16 tiles [N/16, D/32, 64, 8] (memory/semantic_index.py)");
  const int64_t D = packed.size(1) * 32;
  gather_check(recs, rows, 2 * D);
  TORCH_CHECK(packed.size(0) * 16 <= INT32_MAX, "index too large for int32 row ids");
  check_rc(pa_gather_rows_bf16(recs.data_ptr(), rows.data_ptr<int>(), packed.data_ptr(), (long long)rows.size(0),
                               (int)D, (int)(packed.size(0) * 16), cur_stream()),
           "gather_rows_bf16");
}

void gather_rows_q16(at::Tensor recs, at::Tensor rows, at::Tensor hi, at::Tensor lo, at::Tensor rmeta) {
  for (auto* t : {&recs, &rows, &hi, &lo, &rmeta}) check_gpu(*t, "gather_rows_q16 arg");
  check_dtype(hi, at::kChar, "hi"); check_dtype(lo, at::kChar, "lo"); check_dtype(rmeta, at::kFloat, "rmeta");
  TORCH_CHECK(hi.dim() == 4 && hi.size(2) == 64 && hi.size(3) == 16 && lo.sizes() == hi.sizes() &&
                  hi.is_contiguous() && lo.is_contiguous(),
              "hi / lo must be int8 planes [N/16, D/64, 64, 16] (memory/semantic_index.py storage='q16')");
  TORCH_CHECK(rmeta.dim() == 2 && rmeta.size(1) == 2 && rmeta.is_contiguous(), "rmeta must be [N, 2]");
  const int64_t D = hi.size(1) * 64;
  gather_check(recs, rows, 2 * D + 16);
  // a row id is followed only if both its tile and its scale exist
  const int64_t nrows = std::min<int64_t>(hi.size(0) * 16, rmeta.size(0));
  TORCH_CHECK(nrows <= INT32_MAX, "index too large for int32 row ids");
  check_rc(pa_gather_rows_q16(recs.data_ptr(), rows.data_ptr<int>(), hi.data_ptr(), lo.data_ptr(),
                              rmeta.data_ptr<float>(), (long long)rows.size(0), (int)D, (int)nrows, cur_stream()),
           "gather_rows_q16");
}

// MMR re-ranking over exchange records: slot [Q, m] indexes recs [R, rowbytes]; out_pos are list
// positions. q16 is told from bf16 by the caller (the record does not carry its format).
void mmr_select_rows(at::Tensor out_scores, at::Tensor out_pos, at::Tensor recs, at::Tensor slot, at::Tensor scores,
                     at::Tensor wr, at::Tensor wd, int64_t K, bool q16) {
  for (auto* t : {&out_scores, &out_pos, &recs, &slot, &scores, &wr, &wd}) check_gpu(*t, "mmr_select_rows arg");
  mmr_check_lists(out_scores, out_pos, slot, scores, wr, wd, K);
  check_dtype(recs, at::kByte, "recs");
  TORCH_CHECK(recs.dim() == 2 && recs.is_contiguous(), "recs must be a contiguous [R, rowbytes] uint8 tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(recs.data_ptr()) % 16 == 0, "recs must be 16-byte aligned");
  const int64_t rb = recs.size(1), D = (rb - (q16 ? 16 : 0)) / 2, slab = q16 ? 64 : 32;
  TORCH_CHECK(D >= slab && D % slab == 0 && 2 * D + (q16 ? 16 : 0) == rb && (!q16 || D <= 1024),
              "recs rows of ", rb, " bytes are not ", q16 ? "q16 records (2 D + 16, D a multiple of 64, <= 1024)"
                                                          : "bf16 records (2 D, D a multiple of 32)");
  TORCH_CHECK(recs.size(0) <= INT32_MAX, "too many records for int32 slots");
  auto fn = q16 ? pa_mmr_select_rows_q16 : pa_mmr_select_rows_bf16;
  check_rc(fn(out_scores.data_ptr<float>(), out_pos.data_ptr<int>(), recs.data_ptr(), slot.data_ptr<int>(),
              scores.data_ptr<float>(), wr.data_ptr<float>(), wd.data_ptr<float>(), (int)slot.size(0),
              (int)slot.size(1), (int)K, (int)D, (int)recs.size(0), cur_stream()),
           "mmr_select_rows");
}

}  // namespace

// One phase of the vocab-parallel top-k / top-p threshold (sampling.hip tp_topkp_kernel):
// logits [rows, v_local] is this rank's slice; ws [ceil4(rows) + rows * 1028] fp32 holds
// mx | h0 | h1 | st.
void tp_topkp_phase(int64_t phase, at::Tensor tau, at::Tensor ws, at::Tensor logits, int64_t vocab_offset,
                    int64_t V, at::Tensor temperature, at::Tensor top_k, at::Tensor top_p, at::Tensor mask_class,
                    at::Tensor class_masks) {
  for (auto* t : {&tau, &ws, &temperature, &top_k, &top_p, &mask_class, &class_masks})
    check_gpu(*t, "tp_topkp_phase arg");
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.stride(1) == 1, "logits: [rows, v_local] GPU");
  check_dtype(tau, at::kFloat, "tau"); check_dtype(ws, at::kFloat, "ws"); check_dtype(logits, at::kBFloat16, "logits");
  check_dtype(temperature, at::kFloat, "temperature"); check_dtype(top_k, at::kInt, "top_k");
  check_dtype(top_p, at::kFloat, "top_p"); check_dtype(mask_class, at::kInt, "mask_class");
  check_dtype(class_masks, at::kInt, "class_masks");
  const int rows = logits.size(0), vl = logits.size(1);
  TORCH_CHECK(ws.numel() >= (int64_t)((rows + 3) & ~3) + (int64_t)rows * 1028,
              "ws must hold ceil4(rows) + rows * 1028 floats");
  TORCH_CHECK(tau.numel() >= rows && temperature.numel() >= rows && top_k.numel() >= rows &&
                  top_p.numel() >= rows && mask_class.numel() >= rows, "per-row tensors too short");
  TORCH_CHECK(class_masks.dim() == 2 && class_masks.size(1) * 32 >= V && vocab_offset + vl <= V,
              "class_masks / vocab slice");
  check_rc(pa_tp_topkp_phase((int)phase, tau.data_ptr<float>(), ws.data_ptr<float>(), logits.data_ptr(), rows, vl,
                             logits.stride(0), (int)vocab_offset, (int)V, temperature.data_ptr<float>(),
                             top_k.data_ptr<int>(), top_p.data_ptr<float>(), mask_class.data_ptr<int>(),
                             reinterpret_cast<const uint32_t*>(class_masks.data_ptr<int>()), class_masks.size(1),
                             cur_stream()),
           "tp_topkp_phase");
}

// tau[r] = top-k / top-p logit threshold of row r. `logits` is [rows, V] or a TP
// all-gather [shards, rows, V/shards] (then V is the full vocabulary).
void topkp_threshold(at::Tensor tau, at::Tensor logits, int64_t V, at::Tensor temperature,
                     at::Tensor top_k, at::Tensor top_p, at::Tensor mask_class, at::Tensor class_masks) {
  for (auto* t : {&tau, &logits, &temperature, &top_k, &top_p, &mask_class, &class_masks})
    check_gpu(*t, "topkp_threshold arg");
  check_dtype(tau, at::kFloat, "tau"); check_dtype(logits, at::kBFloat16, "logits");
  check_dtype(temperature, at::kFloat, "temperature"); check_dtype(top_k, at::kInt, "top_k");
  check_dtype(top_p, at::kFloat, "top_p"); check_dtype(mask_class, at::kInt, "mask_class");
  check_dtype(class_masks, at::kInt, "class_masks");
  int shards = 1, rows, ld;
  long long sstride = 0;
  if (logits.dim() == 3) {
    shards = logits.size(0); rows = logits.size(1); ld = logits.stride(1); sstride = logits.stride(0);
    TORCH_CHECK(logits.size(2) * shards == V, "gathered logits do not cover the vocabulary");
  } else {
    TORCH_CHECK(logits.dim() == 2 && logits.size(1) == V, "logits must be [rows, V]");
    rows = logits.size(0); ld = logits.stride(0);
  }
  TORCH_CHECK(logits.stride(-1) == 1, "logits need unit inner stride");
  TORCH_CHECK(tau.numel() >= rows && temperature.numel() >= rows && top_k.numel() >= rows &&
                  top_p.numel() >= rows && mask_class.numel() >= rows, "per-row tensors too short");
  TORCH_CHECK(class_masks.dim() == 2 && class_masks.size(1) * 32 >= V, "class_masks too narrow");
  check_rc(pa_topkp_threshold(tau.data_ptr<float>(), logits.data_ptr(), rows, V, ld, shards, sstride,
                              temperature.data_ptr<float>(), top_k.data_ptr<int>(), top_p.data_ptr<float>(),
                              mask_class.data_ptr<int>(),
                              reinterpret_cast<const uint32_t*>(class_masks.data_ptr<int>()),
                              class_masks.size(1), cur_stream()),
           "topkp_threshold");
}

// ---- custom P2P all-reduce (csrc/ops/custom_ar.hip) ----
py::tuple car_alloc(int64_t bytes) {
  char h[64];
  void* p = pa_car_alloc(bytes, h);
  TORCH_CHECK(p != nullptr, "car_alloc: uncached IPC allocation of ", bytes, " bytes failed");
  return py::make_tuple((int64_t)(uintptr_t)p, py::bytes(h, 64));
}

int64_t car_open(py::bytes handle) {
  std::string h = handle;
  TORCH_CHECK(h.size() == 64, "car_open: IPC handle must be 64 bytes");
  void* p = pa_car_open(h.data());
  TORCH_CHECK(p != nullptr, "car_open: hipIpcOpenMemHandle failed");
  return (int64_t)(uintptr_t)p;
}

void car_all_reduce(std::vector<int64_t> bases, int64_t rank0, std::vector<at::Tensor> ins,
                    std::vector<at::Tensor> outs, int64_t cap_bytes, at::Tensor epochs, at::Tensor err,
                    bool two_shot, std::vector<at::Tensor> resids, std::vector<at::Tensor> ss,
                    std::vector<at::Tensor> ss_zero, int64_t row_len) {
  const int W = (int)bases.size();
  const int nl = (int)ins.size();
  TORCH_CHECK(W >= 2 && W <= 8, "custom all-reduce supports 2..8 ranks");
  TORCH_CHECK(nl >= 1 && (int)outs.size() == nl && rank0 >= 0 && rank0 + nl <= W, "bad rank range");
  const int64_t n = ins[0].numel();
  std::vector<void*> b(W), ip(nl), op(nl);
  for (int i = 0; i < W; ++i) b[i] = (void*)(uintptr_t)bases[i];
  for (int i = 0; i < nl; ++i) {
    check_gpu(ins[i], "in"); check_gpu(outs[i], "out");
    check_dtype(ins[i], at::kBFloat16, "in"); check_dtype(outs[i], at::kBFloat16, "out");
    TORCH_CHECK(ins[i].numel() == n && outs[i].numel() == n, "all-reduce tensors differ in size");
    TORCH_CHECK(((uintptr_t)ins[i].data_ptr() & 15) == 0 && ((uintptr_t)outs[i].data_ptr() & 15) == 0,
                "all-reduce tensors must be 16-byte aligned");
    ip[i] = ins[i].data_ptr(); op[i] = outs[i].data_ptr();
  }
  TORCH_CHECK(n % 8 == 0 && n * 2 <= cap_bytes, "message of ", n, " bf16 does not fit the custom all-reduce");
  check_gpu(epochs, "epochs"); check_dtype(epochs, at::kInt, "epochs");
  TORCH_CHECK(epochs.numel() >= (int64_t)nl * pa_car_group(), "epochs too short");
  check_gpu(err, "err"); check_dtype(err, at::kInt, "err");
  // fused residual epilogue: out = resid + sum, ss[row] += sum(out^2), ss_zero <- 0
  std::vector<const void*> rp;
  std::vector<float*> sp, zp;
  const bool fused = !resids.empty();
  if (fused) {
    TORCH_CHECK((int)resids.size() == nl, "one resid per local rank");
    TORCH_CHECK(row_len > 0 && n % row_len == 0 && (row_len / 8) % 256 == 0 && row_len % 8 == 0,
                "fused all-reduce needs whole rows of a multiple of 2048 elements");
    const int64_t rows = n / row_len;
    for (int i = 0; i < nl; ++i) {
      check_gpu(resids[i], "resid"); check_dtype(resids[i], at::kBFloat16, "resid");
      TORCH_CHECK(resids[i].numel() == n && resids[i].is_contiguous() && ((uintptr_t)resids[i].data_ptr() & 15) == 0,
                  "resid must match the message, contiguous and 16-byte aligned");
      rp.push_back(resids[i].data_ptr());
    }
    TORCH_CHECK(ss.empty() || (int)ss.size() == nl, "one ss per local rank");
    TORCH_CHECK(ss_zero.empty() || (int)ss_zero.size() == nl, "one ss_zero per local rank");
    for (auto& t : ss) {
      check_gpu(t, "ss"); check_dtype(t, at::kFloat, "ss");
      TORCH_CHECK(t.numel() >= rows, "ss shorter than the message's rows");
      sp.push_back(t.data_ptr<float>());
    }
    for (auto& t : ss_zero) {
      check_gpu(t, "ss_zero"); check_dtype(t, at::kFloat, "ss_zero");
      TORCH_CHECK(t.numel() >= rows, "ss_zero shorter than the message's rows");
      zp.push_back(t.data_ptr<float>());
    }
  }
  check_rc(pa_car_all_reduce(b.data(), W, (int)rank0, nl, ip.data(), op.data(), n, cap_bytes,
                             reinterpret_cast<uint32_t*>(epochs.data_ptr<int>()), err.data_ptr<int>(),
                             two_shot ? 1 : 0, fused ? rp.data() : nullptr, sp.empty() ? nullptr : sp.data(),
                             zp.empty() ? nullptr : zp.data(), (int)row_len, cur_stream()),
           "custom all-reduce");
}

// Small collectives over the custom all-reduce buffers (custom_ar.hip co_kernel): op 0 = SUM
// and 1 = MAX of fp32 (outs may alias ins), 2 = all-gather of any 4-byte dtype (outs[i] holds
// W x n elements, rank-major). n % 4 == 0, 16-byte aligned tensors.
void car_collective(std::vector<int64_t> bases, int64_t rank0, std::vector<at::Tensor> ins,
                    std::vector<at::Tensor> outs, int64_t cap_bytes, at::Tensor epochs, at::Tensor err, int64_t op) {
  const int W = (int)bases.size();
  const int nl = (int)ins.size();
  TORCH_CHECK(W >= 2 && W <= 8, "custom collectives support 2..8 ranks");
  TORCH_CHECK(nl >= 1 && (int)outs.size() == nl && rank0 >= 0 && rank0 + nl <= W, "bad rank range");
  TORCH_CHECK(op >= 0 && op <= 2, "op: 0 sum, 1 max, 2 gather");
  const int64_t n = ins[0].numel();
  std::vector<void*> b(W), ip(nl), opp(nl);
  for (int i = 0; i < W; ++i) b[i] = (void*)(uintptr_t)bases[i];
  for (int i = 0; i < nl; ++i) {
    check_gpu(ins[i], "in"); check_gpu(outs[i], "out");
    TORCH_CHECK(ins[i].element_size() == 4 && outs[i].element_size() == 4, "4-byte elements");
    if (op < 2) {
      check_dtype(ins[i], at::kFloat, "in"); check_dtype(outs[i], at::kFloat, "out");
    }
    TORCH_CHECK(ins[i].numel() == n && outs[i].numel() == (op == 2 ? n * W : n), "collective tensor sizes");
    TORCH_CHECK(((uintptr_t)ins[i].data_ptr() & 15) == 0 && ((uintptr_t)outs[i].data_ptr() & 15) == 0,
                "collective tensors must be 16-byte aligned");
    ip[i] = ins[i].data_ptr(); opp[i] = outs[i].data_ptr();
  }
  TORCH_CHECK(n % 4 == 0 && n * 4 <= cap_bytes, "message of ", n, " x 4 B does not fit the custom buffers");
  check_gpu(epochs, "epochs"); check_dtype(epochs, at::kInt, "epochs");
  TORCH_CHECK(epochs.numel() >= (int64_t)nl * pa_car_group(), "epochs too short");
  check_gpu(err, "err"); check_dtype(err, at::kInt, "err");
  check_rc(pa_car_collective(b.data(), W, (int)rank0, nl, ip.data(), opp.data(), n, cap_bytes,
                             reinterpret_cast<uint32_t*>(epochs.data_ptr<int>()), err.data_ptr<int>(), (int)op,
                             cur_stream()),
           "custom collective");
}

// ---- uncached device memory (in-launch hand-off workspaces) ----
// Split-K slabs and attention partials are written by one workgroup and read by another
// inside the same launch. In uncached memory (MTYPE UC: no L1/L2 copy of any line) a reader
// can never see a stale copy held by its own CU or XCD, whatever the placement, so the
// hand-off needs no L2 write-back on the producer side.
at::Tensor empty_uncached(int64_t numel, at::ScalarType dtype, int64_t device) {
  TORCH_CHECK(numel > 0, "empty_uncached: numel must be positive");
  const int64_t bytes = numel * (int64_t)c10::elementSize(dtype);
  int prev = 0;
  TORCH_CHECK(hipGetDevice(&prev) == hipSuccess, "hipGetDevice failed");
  TORCH_CHECK(hipSetDevice((int)device) == hipSuccess, "hipSetDevice failed");
  void* p = nullptr;
  const hipError_t e = hipExtMallocWithFlags(&p, (size_t)bytes, hipDeviceMallocUncached);
  if (e == hipSuccess) (void)hipMemset(p, 0, (size_t)bytes);
  (void)hipSetDevice(prev);
  TORCH_CHECK(e == hipSuccess && p != nullptr, "empty_uncached: hipExtMallocWithFlags(", bytes,
              " bytes, uncached) failed");
  TORCH_CHECK(hipDeviceSynchronize() == hipSuccess, "empty_uncached: memset failed");
  auto opts = at::TensorOptions().dtype(dtype).device(at::Device(at::kCUDA, (int)device));
  return torch::from_blob(p, {numel}, [](void* q) { (void)hipFree(q); }, opts);
}

PYBIND11_MODULE(_C, m) {
  m.def("store_test", [](at::Tensor dst, int64_t mode, int64_t grid) {
    check_gpu(dst, "dst");
    TORCH_CHECK(dst.is_contiguous() && dst.nbytes() % 16 == 0, "dst: contiguous, a multiple of 16 bytes");
    check_rc(pa_store_test(dst.data_ptr(), (long long)(dst.nbytes() / 16), (int)mode, (int)grid, cur_stream()),
             "store_test");
  }, py::arg("dst"), py::arg("mode"), py::arg("grid") = 256, "diagnostics: fill dst with one store form");
  m.def("timeline_marker", [](int64_t id) { check_rc(pa_timeline_marker((int)id, cur_stream()), "timeline_marker"); },
        "empty marker kernel (0 = begin, 1 = end of a timed region) for profile cutting");
  m.def("empty_uncached", &empty_uncached, py::arg("numel"), py::arg("dtype"), py::arg("device"),
        "zero-filled device tensor in uncached memory (hipDeviceMallocUncached)");
  m.doc() = "pilottai_amd CDNA4 (gfx950) HIP kernels";
  m.def("rmsnorm", &rmsnorm);
  m.def("fused_add_rmsnorm", &fused_add_rmsnorm);
  m.def("rope_cache", &rope_cache);
  m.def("silu_mul", &silu_mul);
  m.def("skinny_gemm", &skinny_gemm);
  m.def("skinny_set_variant", [](int v) { pa_skinny_set_variant(v); });
  m.def("decode_set_variant", [](int v) { pa_decode_set_variant(v); });
  m.def("handoff_set_acquire", [](int v) { pa_handoff_set_acquire(v); },
        "protocol of every in-launch hand-off (diagnostics): 0 sc1 only, 1 acquire, 2 release + acquire");
  m.def("handoff_set_modes", [](int gemm, int attn) { pa_handoff_set_modes(gemm, attn); },
        "hand-off protocols of the GEMM split-K slabs and of the attention merge (defaults 2, 1)");
  m.def("decode_gemm", &decode_gemm, py::arg("y"), py::arg("x"), py::arg("wp"), py::arg("resid") = py::none(),
        py::arg("epi") = 0, py::arg("norm") = false, py::arg("eps") = 1e-5, py::arg("nt") = 0,
        py::arg("waves") = 0, py::arg("splits") = 0, py::arg("ws") = py::none(), py::arg("counters") = py::none());
  m.def("decode_qkv_rope", &decode_qkv_rope, py::arg("x"), py::arg("wp"), py::arg("eps"), py::arg("q_out"),
        py::arg("k_cache"), py::arg("v_cache"), py::arg("positions"), py::arg("slots"), py::arg("cos_sin"),
        py::arg("H"), py::arg("KV"), py::arg("splits") = 0, py::arg("ws") = py::none(),
        py::arg("counters") = py::none());
  m.def("decode_gemm_fp8", &decode_gemm_fp8, py::arg("y"), py::arg("x"), py::arg("wp8"), py::arg("scale"),
        py::arg("resid") = py::none(), py::arg("epi") = 0, py::arg("norm") = false, py::arg("eps") = 1e-5,
        py::arg("nt") = 0, py::arg("waves") = 0, py::arg("splits") = 0, py::arg("ws") = py::none(),
        py::arg("counters") = py::none());
  m.def("decode_qkv_rope_fp8", &decode_qkv_rope_fp8, py::arg("x"), py::arg("wp8"), py::arg("scale"), py::arg("eps"),
        py::arg("q_out"), py::arg("k_cache"), py::arg("v_cache"), py::arg("positions"), py::arg("slots"),
        py::arg("cos_sin"), py::arg("H"), py::arg("KV"), py::arg("splits") = 0, py::arg("ws") = py::none(),
        py::arg("counters") = py::none());
  m.def("mid_gemm", &mid_gemm, py::arg("y"), py::arg("x"), py::arg("wp"), py::arg("resid"), py::arg("ws"),
        py::arg("counters"), py::arg("epi") = 0, py::arg("ss_in") = py::none(), py::arg("ss_out") = py::none(),
        py::arg("ss_zero") = py::none(), py::arg("eps") = 1e-5, py::arg("fm") = 0, py::arg("fn") = 0,
        py::arg("splits") = 0);
  m.def("mid_qkv_rope", &mid_qkv_rope, py::arg("x"), py::arg("wp"), py::arg("ss_in"), py::arg("eps"),
        py::arg("q_out"), py::arg("k_cache"), py::arg("v_cache"), py::arg("positions"), py::arg("slots"),
        py::arg("cos_sin"), py::arg("H"), py::arg("KV"), py::arg("ws"), py::arg("counters"), py::arg("fm") = 0,
        py::arg("fn") = 0, py::arg("splits") = 0);
  m.def("prefill_gemm", &prefill_gemm, py::arg("y"), py::arg("x"), py::arg("wp"), py::arg("resid"), py::arg("ws"),
        py::arg("counters"), py::arg("epi") = 0, py::arg("ss_in") = py::none(), py::arg("ss_out") = py::none(),
        py::arg("ss_zero") = py::none(), py::arg("eps") = 1e-5, py::arg("full") = -1, py::arg("splits") = 0,
        py::arg("bn") = 0, py::arg("variant") = -1);
  m.def("prefill_qkv_rope", &prefill_qkv_rope, py::arg("x"), py::arg("wp"), py::arg("ss_in"), py::arg("eps"),
        py::arg("q_out"), py::arg("k_cache"), py::arg("v_cache"), py::arg("positions"), py::arg("slots"),
        py::arg("cos_sin"), py::arg("H"), py::arg("KV"), py::arg("ws"), py::arg("counters"), py::arg("full") = -1,
        py::arg("splits") = 0, py::arg("bn") = 0, py::arg("variant") = -1);
  m.def("prefill_set_variant", [](int v) { pa_prefill_set_variant(v); });
  m.def("prefill_gemm_plan", &prefill_gemm_plan, py::arg("M"), py::arg("N"), py::arg("K"), py::arg("bn") = 0,
        "default (full tiles, splits, workspace floats, tile width) of prefill_gemm");
  m.def("row_sumsq", &row_sumsq, py::arg("out"), py::arg("x"));
  m.def("stream_gemm", &stream_gemm, py::arg("y"), py::arg("x"), py::arg("wp"), py::arg("resid"), py::arg("ws"),
        py::arg("counters"), py::arg("err"), py::arg("epi"), py::arg("ss_in"), py::arg("ss_out"), py::arg("ss_zero"),
        py::arg("eps"), py::arg("plan"), py::arg("q_out") = py::none(), py::arg("k_cache") = py::none(),
        py::arg("v_cache") = py::none(), py::arg("positions") = py::none(), py::arg("slots") = py::none(),
        py::arg("cos_sin") = py::none(), py::arg("H") = 0, py::arg("KV") = 0, py::arg("rel") = 0,
        py::arg("stamps") = py::none());
  m.def("stream_gemm_plan", &stream_gemm_plan,
        "default (mg, rg, tpw, wt, wk, S, D, workspace floats) of stream_gemm");
  m.def("mid_gemm_plan", &mid_gemm_plan, "default (fm, fn, splits, workspace floats) of mid_gemm");
  m.def("paged_attention", &paged_attention, py::arg("out"), py::arg("part_o"), py::arg("part_ml"), py::arg("q"),
        py::arg("k_cache"), py::arg("v_cache"), py::arg("items"), py::arg("n_items"), py::arg("counters"),
        py::arg("q_start"), py::arg("q_len"), py::arg("ctx_len"), py::arg("block_table"), py::arg("scale"),
        py::arg("part_size") = py::none(), py::arg("waves") = 4);
  m.def("sample_workspace_floats", &sample_workspace_floats);
  m.def("patch_pending_ids", &patch_pending_ids);
  m.def("kv_copy", &kv_copy);
  m.def("kv_gather_blocks", &kv_gather_blocks);
  m.def("kv_scatter_blocks", &kv_scatter_blocks);
  m.def("span_pool", &span_pool);
  m.def("sample_partials", &sample_partials, py::arg("workspace"), py::arg("logits"), py::arg("vocab_offset"),
        py::arg("temperature"), py::arg("mask_class"), py::arg("class_masks"), py::arg("seeds"),
        py::arg("offsets"), py::arg("tau") = py::none());
  m.def("spec_verify", &spec_verify, py::arg("out_tokens"), py::arg("accept_len"), py::arg("part_k"),
        py::arg("part_i"), py::arg("forced"), py::arg("input_ids"), py::arg("logit_rows"),
        py::arg("run_first"), py::arg("run_len"));
  m.def("sample", &sample, py::arg("out_tokens"), py::arg("out_keys"), py::arg("workspace"),
        py::arg("logits"), py::arg("vocab_offset"), py::arg("temperature"), py::arg("mask_class"),
        py::arg("class_masks"), py::arg("seeds"), py::arg("offsets"), py::arg("forced"),
        py::arg("tau") = py::none());
  m.def("topkp_threshold", &topkp_threshold);
  m.def("logprob_workspace_floats", &logprob_workspace_floats);
  m.def("token_logprobs", &token_logprobs, py::arg("out_lp"), py::arg("top_ids"), py::arg("top_lp"),
        py::arg("workspace"), py::arg("logits"), py::arg("tokens"), py::arg("lp_n"), py::arg("forced"),
        py::arg("mask_class"), py::arg("class_masks"));
  m.def("score_workspace_floats", &score_workspace_floats);
  m.def("score_tokens", &score_tokens, py::arg("out_lp"), py::arg("out_rank"), py::arg("top_ids"),
        py::arg("top_lp"), py::arg("workspace"), py::arg("logits"), py::arg("target"), py::arg("lp_n"));
  m.def("apply_penalties", &apply_penalties, py::arg("logits"), py::arg("counts"), py::arg("distinct"),
        py::arg("n_distinct"), py::arg("pen_slot"), py::arg("pen_reset"), py::arg("presence"),
        py::arg("frequency"), py::arg("forced"), py::arg("pair_start"), py::arg("pair_n"), py::arg("pair_tok"));
  m.def("apply_repetition_penalty", &apply_repetition_penalty, py::arg("logits"), py::arg("seen"),
        py::arg("seen_list"), py::arg("n_seen"), py::arg("rep_slot"), py::arg("rep_reset"), py::arg("rep_r"),
        py::arg("rep_inv_r"), py::arg("forced"), py::arg("rep_start"), py::arg("rep_n"), py::arg("rep_tok"));
  m.def("apply_logit_bias", &apply_logit_bias, py::arg("logits"), py::arg("bias_start"), py::arg("bias_n"),
        py::arg("bias_tok"), py::arg("bias_val"), py::arg("forced"));
  m.def("minp_threshold", &minp_threshold, py::arg("tau"), py::arg("has_tau"), py::arg("logits"),
        py::arg("temperature"), py::arg("min_p"), py::arg("ln_min_p"), py::arg("forced"),
        py::arg("mask_class"), py::arg("class_masks"));
  m.def("tp_topkp_phase", &tp_topkp_phase);
  m.def("cosine_topk_workspace_bytes", &cosine_topk_workspace_bytes);
  m.def("cosine_topk", &cosine_topk);
  m.def("q16_topk_workspace_bytes", &q16_topk_workspace_bytes);
  m.def("q16_topk", &q16_topk);
  m.def("mmr_select_bf16", &mmr_select_bf16);
  m.def("mmr_select_q16", &mmr_select_q16);
  m.def("gather_rows_bf16", &gather_rows_bf16);
  m.def("gather_rows_q16", &gather_rows_q16);
  m.def("mmr_select_rows", &mmr_select_rows);
  m.def("car_alloc", &car_alloc);
  m.def("car_open", &car_open);
  m.def("car_close", [](int64_t p) { return pa_car_close((void*)(uintptr_t)p); });
  m.def("car_free", [](int64_t p) { return pa_car_free((void*)(uintptr_t)p); });
  m.def("car_all_reduce", &car_all_reduce, py::arg("bases"), py::arg("rank0"), py::arg("ins"), py::arg("outs"),
        py::arg("cap_bytes"), py::arg("epochs"), py::arg("err"), py::arg("two_shot"),
        py::arg("resids") = std::vector<at::Tensor>(), py::arg("ss") = std::vector<at::Tensor>(),
        py::arg("ss_zero") = std::vector<at::Tensor>(), py::arg("row_len") = 0);
  m.def("car_collective", &car_collective, py::arg("bases"), py::arg("rank0"), py::arg("ins"), py::arg("outs"),
        py::arg("cap_bytes"), py::arg("epochs"), py::arg("err"), py::arg("op"));
  m.def("car_group", &pa_car_group);
  m.def("car_flag_bytes", &pa_car_flag_bytes);
  m.attr("ATT_PART") = 512;
  m.attr("SAMPLE_CHUNK") = 4096;
}
