// Decode-step projections on FP8 (OCP e4m3) packed weights: the W8 instantiation of the
// kernel in gemm_decode.h. wp8 is the fragment-major layout with 1-byte elements
// ([N/16][K/32][64 lanes][8], ops.pack_decode_weight_fp8), scale [N] the per-column
// power-of-two scales in PACKED column order. Same arguments, return codes, refused shapes
// and (nt, waves, splits) as pa_decode_gemm / pa_decode_qkv_rope; the K split and the
// reduction order are those of the bf16 instantiation by construction, so the result equals
// the bf16 kernel on the dequantised weights bit for bit.
#include "gemm_decode.h"

extern "C" int pa_decode_gemm_fp8(void* y, const void* x, const void* wp8, const float* scale, const void* resid,
                                  int M, int N, int K, int ldx, int ldy, int ldr, int epi, int norm, float eps,
                                  int nt, int waves, int splits, float* ws, long long ws_floats, int* counters,
                                  int n_counters, hipStream_t st) {
  using namespace pa;
  if (epi == EPI_ROPE) return 1;
  DgArgs a{(bf16*)y, (const bf16*)x, wp8, scale, (const bf16*)resid, M, N, K, ldx, ldy, ldr, eps, RopeArgs{},
           1, ws, counters};
  return dispatch<true>(a, epi, norm, nt, waves, splits, ws_floats, n_counters, st);
}

extern "C" int pa_decode_qkv_rope_fp8(const void* x, const void* wp8, const float* scale, int M, int N, int K,
                                      int ldx, float eps, void* q_out, void* k_cache, void* v_cache,
                                      const int* positions, const int* slots, const float* cos_sin, int H, int KV,
                                      int nt, int waves, int splits, float* ws, long long ws_floats,
                                      int* counters, int n_counters, hipStream_t st) {
  using namespace pa;
  if (N != (H + 2 * KV) * 128) return 1;
  DgArgs a{nullptr, (const bf16*)x, wp8, scale, nullptr, M, N, K, ldx, 0, 0, eps,
           RopeArgs{(bf16*)q_out, (bf16*)k_cache, (bf16*)v_cache, positions, slots, cos_sin, H, KV},
           1, ws, counters};
  return dispatch<true>(a, EPI_ROPE, 1, nt, waves, splits, ws_floats, n_counters, st);
}
