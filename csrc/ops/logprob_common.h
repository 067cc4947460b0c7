// Device helpers shared by the passes that read whole logit rows in 4096-entry chunks: the
// sampler and the log-probability pass (sampling.hip) and the scoring pass (scoring.hip).
//
// Conventions (the files that include this are compiled with -ffast-math, i.e. no-infs): inside
// the kernels a masked / absent entry is the finite LP_NEG, every test is a finite or an integer
// comparison, and the -inf of the outputs is stored as its bit pattern.
#pragma once
#include "common.h"

namespace pa {

constexpr int SMP_CHUNK = 4096;  // vocab entries per workgroup (256 threads x 16)

struct KeyIdx {
  float k;
  int i;
};

__device__ __forceinline__ KeyIdx better(KeyIdx a, KeyIdx b) {
  // larger key wins; ties -> smaller index (deterministic)
  if (b.k > a.k || (b.k == a.k && b.i < a.i)) return b;
  return a;
}

// bf16 values map to a monotone 16-bit order key (radix select, log-probability lists, ranks)
__device__ __forceinline__ uint32_t bf16_order_key(uint16_t b) {
  return (b & 0x8000u) ? (~(uint32_t)b & 0xffffu) : ((uint32_t)b | 0x8000u);
}
__device__ __forceinline__ float order_key_value(uint32_t k) {
  const uint16_t b = (k & 0x8000u) ? (uint16_t)(k & 0x7fffu) : (uint16_t)(~k & 0xffffu);
  return __uint_as_float((uint32_t)b << 16);
}

constexpr float LP_NEG = -3.0e38f;      // masked / absent entry (below every bf16 logit in use)
constexpr float LP_LIVE = -1.0e38f;     // x > LP_LIVE: a real logit
constexpr int LP_NEG_INF_BITS = (int)0xff800000u;
__device__ __forceinline__ void store_neg_inf(float* p) { *reinterpret_cast<int*>(p) = LP_NEG_INF_BITS; }

constexpr int LP_MAX = 20;              // alternatives per token (the OpenAI API's limit)
constexpr int LP_WS = 2 + 2 * LP_MAX;   // floats per (row, chunk): max, sum, 20 logits, 20 ids
constexpr int LP_MAX_CHUNKS = 64;       // one lane of the merge wave per chunk (V <= 262144)

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ KeyIdx wave_best(KeyIdx b) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    KeyIdx other{__shfl_xor(b.k, o, 64), __shfl_xor(b.i, o, 64)};
    b = better(b, other);
  }
  return b;
}

// Merge sorted (logit, id) lists into the first n entries of their union, one list per owning
// lane (`owner`; ids are unique over all lists; a list ends at id < 0 or after `len` entries).
// Every lane of the wave calls it; lane 0 writes out_k[k] = logit - sub, out_i[k] = id, and
// (-inf, -1) from the end of the merged list up to `pad` entries.
__device__ __forceinline__ void lp_merge_lists(const float* lk, const int* li, int len, bool owner, int n,
                                               float* out_k, int* out_i, int pad, float sub) {
  const int lane = threadIdx.x & 63;
  int p = 0, k = 0;
  for (; k < n; ++k) {
    KeyIdx h{LP_NEG, 0x7fffffff};
    if (owner && p < len) {
      const int id = li[p];
      if (id >= 0) h = KeyIdx{lk[p], id};
    }
    const KeyIdx w = wave_best(h);
    if (w.i == 0x7fffffff) break;  // every list is exhausted (wave-uniform)
    if (h.i == w.i) ++p;
    if (lane == 0) {
      out_k[k] = w.k - sub;
      out_i[k] = w.i;
    }
  }
  if (lane == 0)
    for (; k < pad; ++k) {
      store_neg_inf(out_k + k);
      out_i[k] = -1;
    }
}

// One chunk of a row, held in the registers of a 256-thread workgroup: v[j] is the logit (LP_NEG
// when masked or -inf), key[j] its rank inside the chunk as one unsigned number, the bf16 order
// key above (4095 - index in the chunk), 0 = masked (keys are unique inside a chunk). Writes the
// chunk's fp32 (max, sum exp(x - max)) to w[0:2] and its top-n as (logit, id) lists to
// w[2 : 2 + LP_MAX] / w[2 + LP_MAX : LP_WS] (sorted; -inf / -1 past the end, n entries written).
// Every thread of the workgroup calls it; `key` is consumed.
__device__ __forceinline__ void lp_chunk_reduce(const float (&v)[16], uint32_t (&key)[16], int n, int chunk,
                                                float* w) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __shared__ float s_red[8];
  __shared__ uint32_t s_key[4][LP_MAX];
  // the chunk's normaliser: max, then sum exp(x - max)
  float m = v[0];
#pragma unroll
  for (int j = 1; j < 16; ++j) m = fmaxf(m, v[j]);
  m = wave_max(m);
  if (lane == 0) s_red[wid] = m;
  __syncthreads();
  m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  float s = 0.f;
  if (m > LP_LIVE) {
#pragma unroll
    for (int j = 0; j < 16; ++j) s += v[j] > LP_LIVE ? __expf(v[j] - m) : 0.f;
  }
  s = wave_sum(s);
  if (lane == 0) s_red[4 + wid] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    w[0] = m;
    w[1] = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);
  }
  if (n == 0) return;
  // this wave's top-n: n rounds of (thread best over its registers, wave argmax, the owner
  // retires the winner)
  int it = 0;
  for (; it < n; ++it) {
    uint32_t b = key[0];
#pragma unroll
    for (int j = 1; j < 16; ++j) b = max(b, key[j]);
    const uint32_t win = wave_max_u32(b);
    if (win == 0u) break;  // nothing allowed is left in this wave (wave-uniform)
    if (lane == 0) s_key[wid][it] = win;
#pragma unroll
    for (int j = 0; j < 16; ++j) key[j] = key[j] == win ? 0u : key[j];
  }
  if (lane == 0)
    for (; it < n; ++it) s_key[wid][it] = 0u;
  __syncthreads();
  // wave 0 merges the four sorted lists (lane l < 4 holds the head of wave l's list)
  if (wid != 0) return;
  float* out_k = w + 2;
  int* out_i = reinterpret_cast<int*>(w + 2 + LP_MAX);
  int p = 0, k = 0;
  for (; k < n; ++k) {
    const uint32_t h = (lane < 4 && p < n) ? s_key[lane & 3][p] : 0u;
    const uint32_t win = wave_max_u32(h);
    if (win == 0u) break;  // wave-uniform
    if (h == win) ++p;
    if (lane == 0) {
      out_k[k] = order_key_value(win >> 12);
      out_i[k] = chunk * SMP_CHUNK + 4095 - (int)(win & 4095u);
    }
  }
  if (lane == 0)
    for (; k < n; ++k) {
      store_neg_inf(out_k + k);
      out_i[k] = -1;
    }
}

}  // namespace pa
