// Decode-step projections on pre-packed bf16 weights: the entry points of the kernel in
// gemm_decode.h (design notes there), and the switches shared with its FP8 sibling
// (gemm_decode_fp8.hip) and the other split-K GEMMs.
#include "gemm_decode.h"

namespace pa {

// bit 0: non-temporal weight loads (default on: the weight stream is read once per step by one
// wave, so it should not displace x and the KV cache in L2 / MALL; 5-9 % faster on every
// projection at M = 8-32, 8-token decode steps 3.49 -> 3.33 ms: profiles/r2_decode_nt_ab.jsonl)
int g_dg_variant = 1;

// protocol of the in-launch hand-offs, common.h handoff_last (tools/splitk_check.py: fresh
// inputs, NaN-poisoned slabs and outputs; tools/handoff_cost.py; profiles/r3_splitk_handoff.md):
//   GEMM split-K slabs (decode / wide / mid / prefill): 2 = producer agent release + last-arriver
//     agent acquire. Decode qkv_rope at M = 9 with 3 K-slices mismatched in 46 of 3,000 runs
//     with the round-2 sc1-only form (mode 0) and in 4 of 10,000 with the acquire alone
//     (mode 1); none with mode 2 (+2-3 us per split launch). Round 4: with the slabs in
//     uncached memory (ops.empty_handoff) mode 1 still mismatched 5 of 10,000 (finite values),
//     so the cause is not a stale L2 copy of the slab; mode 2 stays
//     (profiles/r4_handoff_uncached.md).
//   attention partition merge: 1 = last-arriver agent acquire on uncached partials: 0 bad runs
//     in 10,000 poisoned repetitions for each of ten 256/512-key, 4/8-wave cases (round 4); the
//     release costs +77 us at 64 rows x 1,000 keys there (it writes back every dirty L2 line of
//     the XCD, and this launch leaves many).
int g_handoff_acquire = 2;
int g_handoff_attn = 1;

}  // namespace pa

// Returns 1 if the shape/config is not handled, 0 on success, -2 on a launch error.
// epi: 0 plain, 1 silu(gate)*up over interleaved tile pairs, 2 residual add.
// nt/waves/splits <= 0 pick the defaults; ws/counters: split-K slabs and zeroed tickets.
extern "C" void pa_decode_set_variant(int v) { pa::g_dg_variant = v; }
extern "C" void pa_handoff_set_acquire(int v) { pa::g_handoff_acquire = pa::g_handoff_attn = v; }
extern "C" void pa_handoff_set_modes(int gemm, int attn) {
  pa::g_handoff_acquire = gemm;
  pa::g_handoff_attn = attn;
}

extern "C" int pa_decode_gemm(void* y, const void* x, const void* wp, const void* resid, int M, int N, int K,
                              int ldx, int ldy, int ldr, int epi, int norm, float eps, int nt, int waves,
                              int splits, float* ws, long long ws_floats, int* counters, int n_counters,
                              hipStream_t st) {
  using namespace pa;
  if (epi == EPI_ROPE) return 1;
  DgArgs a{(bf16*)y, (const bf16*)x, wp, nullptr, (const bf16*)resid, M, N, K, ldx, ldy, ldr, eps, RopeArgs{},
           1, ws, counters};
  return dispatch<false>(a, epi, norm, nt, waves, splits, ws_floats, n_counters, st);
}

// QKV projection (RMSNorm folded, rope-permuted packed weights) + RoPE + paged KV
// write: q -> q_out [M, H, 128], k/v -> the layer's cache pages at slots[m].
extern "C" int pa_decode_qkv_rope(const void* x, const void* wp, int M, int N, int K, int ldx, float eps,
                                  void* q_out, void* k_cache, void* v_cache, const int* positions,
                                  const int* slots, const float* cos_sin, int H, int KV, int nt, int waves,
                                  int splits, float* ws, long long ws_floats, int* counters, int n_counters,
                                  hipStream_t st) {
  using namespace pa;
  if (N != (H + 2 * KV) * 128) return 1;
  DgArgs a{nullptr, (const bf16*)x, wp, nullptr, nullptr, M, N, K, ldx, 0, 0, eps,
           RopeArgs{(bf16*)q_out, (bf16*)k_cache, (bf16*)v_cache, positions, slots, cos_sin, H, KV},
           1, ws, counters};
  return dispatch<false>(a, EPI_ROPE, 1, nt, waves, splits, ws_floats, n_counters, st);
}
