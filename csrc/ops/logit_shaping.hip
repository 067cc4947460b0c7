// Stateless logit shaping on the LM-head logits of the sampling rows, behind the penalty pass
// and ahead of the grammar mask, the top-k / top-p threshold's consumer (the sampler) and the
// log-probability pass:
//
//   logit_bias   for each (t, b) of the row's list:  logit[t] <- bf16(float(logit[t]) + b)
//                (one fp32 add, one round-to-nearest-even conversion; nothing else is touched)
//   min_p        m = the largest logit among the tokens the row's mask class allows;
//                tau_mp = fadd_rn(m, fmul_rn(T, L)),  L = float32(ln p) computed on the host;
//                tau[row] = max(tau[row], tau_mp): the sampler keeps {allowed i : logit_i >= tau},
//                i.e. the tokens whose probability at temperature T is >= p * the largest one.
//
// Both are functions of the row alone (its list is fixed for the life of the request, the
// threshold depends only on the row's logits): no device state, no hand-off between workgroups.
#include "common.h"

namespace pa {

constexpr int BIAS_THREADS = 256;
constexpr int MINP_THREADS = 1024;

// One workgroup per sampling row; the row's entries carry unique token ids (submit()
// guarantees it), so every rewritten logit is read and written by one thread only.
__global__ __launch_bounds__(BIAS_THREADS) void apply_logit_bias_kernel(
    bf16* __restrict__ logits, int V, int ld, const int* __restrict__ bias_start,
    const int* __restrict__ bias_n, const int* __restrict__ bias_tok,
    const float* __restrict__ bias_val, int bias_len, const int* __restrict__ forced) {
  const int row = blockIdx.x;
  const int n = bias_n[row];
  if (n <= 0 || forced[row] >= 0) return;  // uniform per workgroup
  const int start = bias_start[row];
  if (start < 0 || start > bias_len - n) return;  // a list that leaves the region: not read
  bf16* lr = logits + (size_t)row * ld;
  for (int i = threadIdx.x; i < n; i += BIAS_THREADS) {
    const int t = bias_tok[start + i];
    if (t < 0 || t >= V) continue;
    lr[t] = f2bf(__fadd_rn(bf2f(lr[t]), bias_val[start + i]));
  }
}

// the 16-bit order key of sampling.hip's radix select: monotone in the bf16 value
__device__ __forceinline__ uint32_t shp_order_key(uint32_t b) {
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
__device__ __forceinline__ float shp_key_value(uint32_t k) {
  const uint32_t b = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
  return __uint_as_float(b << 16);
}

// One workgroup per sampling row, one pass over the row: the maximum is taken on the order
// keys (integers: no floating-point comparison is involved). Key 0 (a negative NaN
// pattern) stands for "nothing allowed". has_tau = 0: the step ran no top-k / top-p pass, so
// tau holds nothing yet and rows this kernel skips get "no truncation" (-inf, as
// topkp_threshold_kernel writes it).
__global__ __launch_bounds__(MINP_THREADS) void minp_threshold_kernel(
    float* __restrict__ tau, int has_tau, const uint16_t* __restrict__ logits, int V, int ld,
    const float* __restrict__ temperature, const float* __restrict__ min_p,
    const float* __restrict__ ln_min_p, const int* __restrict__ forced,
    const int* __restrict__ mask_class, const uint32_t* __restrict__ class_masks, int mask_words,
    int n_classes) {
  const int row = blockIdx.x;
  const float p = min_p[row];
  const float T = temperature[row];
  const int mc = mask_class[row];
  if (!(p > 0.f) || !(T > 0.f) || forced[row] >= 0 || mc >= n_classes) {  // uniform per workgroup
    if (!has_tau && threadIdx.x == 0) tau[row] = -INFINITY;
    return;
  }
  const uint16_t* lr = logits + (size_t)row * ld;
  const uint32_t* mrow = mc >= 0 ? class_masks + (size_t)mc * mask_words : nullptr;
  // whole 16-byte vectors inside [0, V) when the row starts 16-byte aligned; the remainder
  // (and an unaligned row) entry by entry, so nothing at or beyond V is ever loaded
  const int nvec = ((reinterpret_cast<uintptr_t>(lr) & 15) == 0) ? V / 8 : 0;
  uint32_t best = 0;
  for (int v = threadIdx.x; v < nvec; v += MINP_THREADS) {
    const int i0 = v * 8;
    const u32x4 w = *reinterpret_cast<const u32x4*>(lr + i0);
    const uint32_t bits = mrow ? (mrow[i0 >> 5] >> (i0 & 31)) : 0xffu;  // 8 | 32: one mask word
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t b = (j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xffffu);
      const uint32_t k = shp_order_key(b);
      best = ((bits >> j) & 1u) ? max(best, k) : best;
    }
  }
  for (int i = nvec * 8 + threadIdx.x; i < V; i += MINP_THREADS) {
    if (mrow && !((mrow[i >> 5] >> (i & 31)) & 1u)) continue;
    best = max(best, shp_order_key(lr[i]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o, 64));
  __shared__ uint32_t red[MINP_THREADS / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < MINP_THREADS / 64; ++w) best = max(best, red[w]);
    if (best == 0) {  // the mask allows nothing: the row is left to the sampler's fallback
      if (!has_tau) tau[row] = -INFINITY;
      return;
    }
    // two separately rounded fp32 operations, as the host computes them: the product goes
    // through an opaque register so that it cannot be contracted into an fma with the sum
    float prod = __fmul_rn(T, ln_min_p[row]);
    asm volatile("" : "+v"(prod));
    const float t_mp = __fadd_rn(shp_key_value(best), prod);
    tau[row] = has_tau ? fmaxf(tau[row], t_mp) : t_mp;
  }
}

}  // namespace pa

// logits [rows, ld] bf16 (V <= ld: the padding is not touched); per-row arrays of >= rows
// entries; bias_tok / bias_val [bias_len].
extern "C" int pa_apply_logit_bias(void* logits, int rows, int V, int ld, const int* bias_start,
                                   const int* bias_n, const int* bias_tok, const float* bias_val,
                                   int bias_len, const int* forced, hipStream_t st) {
  if (rows <= 0) return 0;
  if (V <= 0 || ld < V || bias_len < 0) return -1;
  hipLaunchKernelGGL(pa::apply_logit_bias_kernel, dim3(rows), dim3(pa::BIAS_THREADS), 0, st,
                     (pa::bf16*)logits, V, ld, bias_start, bias_n, bias_tok, bias_val, bias_len, forced);
  return (int)hipGetLastError();
}

// tau [rows] fp32, updated in place (has_tau != 0) or written (has_tau == 0); class_masks
// [n_classes, mask_words] with mask_words * 32 >= V.
extern "C" int pa_minp_threshold(float* tau, int has_tau, const void* logits, int rows, int V, int ld,
                                 const float* temperature, const float* min_p, const float* ln_min_p,
                                 const int* forced, const int* mask_class, const uint32_t* class_masks,
                                 int mask_words, int n_classes, hipStream_t st) {
  if (rows <= 0) return 0;
  if (V <= 0 || ld < V || (long long)mask_words * 32 < V || n_classes < 0) return -1;
  hipLaunchKernelGGL(pa::minp_threshold_kernel, dim3(rows), dim3(pa::MINP_THREADS), 0, st, tau, has_tau,
                     (const uint16_t*)logits, V, ld, temperature, min_p, ln_min_p, forced, mask_class,
                     class_masks, mask_words, n_classes);
  return (int)hipGetLastError();
}
