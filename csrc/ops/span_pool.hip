// Span pooling for document chunk embeddings ("late chunking": runtime/scheduler.h span region).
//
// An embedding request may name token ranges of its prompt; each range reports the mean of the
// final-norm hidden rows of its tokens. The scheduler cuts every range into the pieces that lie
// in the step's rows and lists them as segments (first_row, n_rows, slot, init); this kernel adds
// the rows of each segment into the segment's fp32 accumulator row:
//   pool[slot][j] = (init ? +0 : pool[slot][j]) + hn[first_row][j] + ... + hn[first_row + n_rows - 1][j]
// evaluated left to right, one round-to-nearest fp32 add of the exactly converted bf16 value per
// row. That order is the specification: the sum of a range is then the same bits whatever prefill
// chunks the prompt was cut into, and the same bits from run to run.
//
// So a thread owns 8 neighbouring dimensions of one segment for all of the segment's rows: no
// atomics, no cross-lane reduction, nothing that could reorder the adds. The row loads are
// independent of each other and SP_UNROLL of them (16 bytes each) are in flight per thread; only
// the adds are a chain. The adds are written as v_add_f32 instructions: the file is built with the
// op library's common flags, under which the compiler may reassociate an fp32 expression, and a
// sum whose order is its contract must not depend on that. There is no multiply anywhere, so no
// fused multiply-add can form.
//
// The segment count is read from device memory and the grid is (segment capacity, column groups),
// the same in every step (hipGraph capture); workgroups at or beyond the count exit at once.
// Two segments of one launch never name the same slot (the scheduler emits at most one segment
// per range and step, and a range owns its slot); they may share rows (overlapping ranges).
#include "common.h"

namespace pa {

constexpr int SP_THREADS = 128;           // 2 waves; 8 dimensions per thread
constexpr int SP_COLS = SP_THREADS * 8;   // dimensions per column group
constexpr int SP_UNROLL = 8;              // row loads in flight per thread

__device__ __forceinline__ float sp_add(float a, float b) {
  float r;
  asm("v_add_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// acc[0..7] += the 8 bf16 values of `v`, exactly converted (bf16 is the top half of an fp32)
__device__ __forceinline__ void sp_add_row(float (&acc)[8], const uint4& v) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc[2 * i] = sp_add(acc[2 * i], __uint_as_float(w[i] << 16));
    acc[2 * i + 1] = sp_add(acc[2 * i + 1], __uint_as_float(w[i] & 0xffff0000u));
  }
}

// grid (cap, ceil(d / SP_COLS)), SP_THREADS threads. hn [T, d] bf16 as 16-byte vectors (d % 8 == 0),
// pool [slots, d] fp32. A segment whose rows leave [0, T), with n_rows <= 0, or whose slot leaves
// [0, slots) is skipped: nothing of it is read or written.
__global__ __launch_bounds__(SP_THREADS) void span_pool_kernel(const uint4* __restrict__ hn,
                                                               const int* __restrict__ n_seg,
                                                               const int* __restrict__ segs, int cap,
                                                               float* __restrict__ pool, int T, int d, int slots) {
  const int seg = blockIdx.x;
  if (seg >= min(*n_seg, cap)) return;
  const int first = segs[4 * seg], n = segs[4 * seg + 1], slot = segs[4 * seg + 2], init = segs[4 * seg + 3];
  if (n <= 0 || first < 0 || first > T - n || (unsigned)slot >= (unsigned)slots) return;
  const int col = (blockIdx.y * SP_THREADS + threadIdx.x) * 8;
  if (col >= d) return;
  float4* dst = reinterpret_cast<float4*>(pool + (size_t)slot * d + col);
  float acc[8];
  if (init) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  } else {
    const float4 a = dst[0], b = dst[1];
    acc[0] = a.x; acc[1] = a.y; acc[2] = a.z; acc[3] = a.w;
    acc[4] = b.x; acc[5] = b.y; acc[6] = b.z; acc[7] = b.w;
  }
  const size_t ld = (size_t)(d >> 3);  // 16-byte vectors per row
  const uint4* src = hn + (size_t)first * ld + (col >> 3);
  int r = 0;
  for (; r + SP_UNROLL <= n; r += SP_UNROLL) {
    uint4 v[SP_UNROLL];
#pragma unroll
    for (int u = 0; u < SP_UNROLL; ++u) v[u] = src[(size_t)(r + u) * ld];
#pragma unroll
    for (int u = 0; u < SP_UNROLL; ++u) sp_add_row(acc, v[u]);
  }
  for (; r < n; ++r) sp_add_row(acc, src[(size_t)r * ld]);
  dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
  dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

}  // namespace pa

// hn: [T, d] bf16; n_seg: one device word; segs: device words (first_row, n_rows, slot, init) x cap;
// pool: [slots, d] fp32. -1: bad arguments (d % 8, sizes).
extern "C" int pa_span_pool(const void* hn, const int* n_seg, const int* segs, int cap, float* pool, int T, int d,
                            int slots, hipStream_t st) {
  if (cap <= 0 || T <= 0 || slots <= 0) return 0;
  if (d <= 0 || d % 8 != 0) return -1;
  const int groups = (d + pa::SP_COLS - 1) / pa::SP_COLS;
  if (groups > 65535) return -1;
  hipLaunchKernelGGL(pa::span_pool_kernel, dim3(cap, groups), dim3(pa::SP_THREADS), 0, st,
                     reinterpret_cast<const uint4*>(hn), n_seg, segs, cap, pool, T, d, slots);
  return (int)hipGetLastError();
}
