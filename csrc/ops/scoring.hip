// Prompt scoring: log-probability, vocabulary rank and top-n alternatives of a GIVEN token per
// logit row (the engine's scoring requests: "how likely is this text I already have").
//
// For row r with target t = target[r] >= 0 and x = the row's bf16 logits:
//   logprob  float(x[t]) - lse(x): natural log over the whole vocabulary at temperature 1, no
//            grammar mask, the fp32 chunked log-sum-exp of the log-probability pass
//            (sampling.hip); a logit of -inf gives -inf
//   rank     1 + #{ i : key(x[i]) > key(x[t]) or (key(x[i]) == key(x[t]) and i < t) }, key = the
//            16-bit bf16 order key: integer comparisons only, so exact ("larger logit first,
//            equal logits by smaller id", the order of the lists; -0 ranks below +0)
//   top-n    the n = lp_n[r] (0..20) most likely tokens with their logprobs, ordered and padded
//            like the log-probability pass (id -1 / -inf past the end, -inf logits never listed)
// Two plain launches, no flags or atomics between workgroups:
//   score_chunk_kernel  grid (nchunk, rows), 256 threads: the chunk's 4096 entries are read once
//       as 16-byte vectors; fp32 (max, sum exp) and top-n of the chunk (lp_chunk_reduce), and the
//       number of the chunk's entries that beat the target. The target's 16 bits are fetched
//       once per workgroup (one 2-byte load at a workgroup-uniform address).
//   score_merge_kernel  one wave per row: combines the normalisers, the lists, the counts (an
//       integer sum) and the target's logit, writes the record.
// Rows with target < 0 are skipped (nothing read, nothing written). A target >= V writes logprob
// -inf and rank 0 and reads nothing out of bounds. Compiled with -ffast-math: see logprob_common.h.
#include "common.h"
#include "logprob_common.h"

namespace pa {

constexpr int SC_WS = LP_WS + 2;  // words per (row, chunk): the logprob pass's 42, the count, one pad

__global__ __launch_bounds__(256) void score_chunk_kernel(float* __restrict__ ws,
                                                          const bf16* __restrict__ logits, int V, int ld,
                                                          const int* __restrict__ target,
                                                          const int* __restrict__ lp_n, int nchunk) {
  const int row = blockIdx.y, chunk = blockIdx.x;
  const int t = target[row];
  if (t < 0) return;  // the whole workgroup
  const int n = min(max(lp_n[row], 0), LP_MAX);
  const bf16* lr = logits + (size_t)row * ld;
  const bool t_ok = t < V;
  // the target's order key, one load per workgroup (every thread asks for the same two bytes)
  const uint32_t tkey = t_ok ? bf16_order_key(reinterpret_cast<const uint16_t*>(lr)[t]) : 0xffffffffu;
  const int base = chunk * SMP_CHUNK + threadIdx.x * 8;
  float v[16];
  uint32_t key[16];
  int beat = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i0 = base + h * 2048;
    if (i0 < V) {  // V % 8 == 0: a vector is inside the row or past it as a whole
      const u32x4 raw = *reinterpret_cast<const u32x4*>(lr + i0);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t b16 = (raw[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
        const float x = __uint_as_float(b16 << 16);
        const bool live = x > LP_LIVE;  // a logit of -inf is never listed and adds nothing to the sum
        const uint32_t local = (uint32_t)(threadIdx.x * 8 + h * 2048 + j);
        const uint32_t ok = bf16_order_key((uint16_t)b16);
        v[h * 8 + j] = live ? x : LP_NEG;
        key[h * 8 + j] = live ? ((ok << 12) | (4095u - local)) : 0u;
        // (key, inverted global index) compared as one number; every entry counts, -inf included
        beat += (ok > tkey || (ok == tkey && i0 + j < t)) ? 1 : 0;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[h * 8 + j] = LP_NEG;
        key[h * 8 + j] = 0u;
      }
    }
  }
  float* w = ws + ((size_t)row * nchunk + chunk) * SC_WS;
  __shared__ int s_beat[4];
  beat = wave_sum_i32(beat);
  if ((threadIdx.x & 63) == 0) s_beat[threadIdx.x >> 6] = beat;
  __syncthreads();
  if (threadIdx.x == 0) reinterpret_cast<int*>(w)[LP_WS] = (s_beat[0] + s_beat[1]) + (s_beat[2] + s_beat[3]);
  lp_chunk_reduce(v, key, n, chunk, w);
}

__global__ __launch_bounds__(64) void score_merge_kernel(float* __restrict__ out_lp, int* __restrict__ out_rank,
                                                         int out_stride, int* __restrict__ top_ids,
                                                         float* __restrict__ top_lp, int top_stride,
                                                         const float* __restrict__ ws,
                                                         const bf16* __restrict__ logits, int V, int ld,
                                                         const int* __restrict__ target,
                                                         const int* __restrict__ lp_n, int nchunk) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const int t = target[row];
  if (t < 0) return;
  const int n = min(max(lp_n[row], 0), LP_MAX);
  int* ti = top_ids + (size_t)row * top_stride;
  float* tl = top_lp + (size_t)row * top_stride;
  float* ol = out_lp + (size_t)row * out_stride;
  int* orank = out_rank + (size_t)row * out_stride;
  const float* w = ws + ((size_t)row * nchunk + min(lane, nchunk - 1)) * SC_WS;
  const bool owner = lane < nchunk;
  const float m = owner ? w[0] : LP_NEG;
  const float M = wave_max(m);
  const int beat = wave_sum_i32(owner ? reinterpret_cast<const int*>(w)[LP_WS] : 0);
  if (lane == 0) *orank = t < V ? 1 + beat : 0;
  if (!(M > LP_LIVE)) {  // every logit is -inf
    if (lane < LP_MAX) {
      ti[lane] = -1;
      store_neg_inf(tl + lane);
    }
    if (lane == 0) store_neg_inf(ol);
    return;
  }
  const float S = wave_sum(m > LP_LIVE ? w[1] * __expf(m - M) : 0.f);
  const float lse = M + logf(S);
  if (lane == 0) {
    store_neg_inf(ol);  // a target outside the vocabulary, or a logit of -inf
    if (t < V) {
      const float x = bf2f(logits[(size_t)row * ld + t]);
      if (x > LP_LIVE) *ol = x - lse;
    }
  }
  lp_merge_lists(w + 2, reinterpret_cast<const int*>(w + 2 + LP_MAX), n, owner, n, tl, ti, LP_MAX, lse);
}

}  // namespace pa

extern "C" int pa_score_workspace_floats(int rows, int V) {
  const int nchunk = (V + pa::SMP_CHUNK - 1) / pa::SMP_CHUNK;
  return rows * nchunk * pa::SC_WS;
}

// out_lp / out_rank [row * out_stride]; top_ids / top_lp [row * top_stride + 0..19] (the four may
// be columns of one record buffer). workspace: pa_score_workspace_floats(rows, V) floats.
extern "C" int pa_score_tokens(float* out_lp, int* out_rank, int out_stride, int* top_ids, float* top_lp,
                               int top_stride, float* workspace, const void* logits, int rows, int V, int ld,
                               const int* target, const int* lp_n, hipStream_t st) {
  if (rows <= 0) return 0;
  if (V <= 0 || V % 8 != 0 || ld % 8 != 0 || ld < V || top_stride < pa::LP_MAX || out_stride < 1) return -1;
  const int nchunk = (V + pa::SMP_CHUNK - 1) / pa::SMP_CHUNK;
  if (nchunk > pa::LP_MAX_CHUNKS) return -1;
  hipLaunchKernelGGL(pa::score_chunk_kernel, dim3(nchunk, rows), dim3(256), 0, st, workspace,
                     (const pa::bf16*)logits, V, ld, target, lp_n, nchunk);
  hipLaunchKernelGGL(pa::score_merge_kernel, dim3(rows), dim3(64), 0, st, out_lp, out_rank, out_stride, top_ids,
                     top_lp, top_stride, workspace, (const pa::bf16*)logits, V, ld, target, lp_n, nchunk);
  return (int)hipGetLastError();
}
