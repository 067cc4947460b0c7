// Cross-shard MMR re-ranking (memory/node_store.py, ShardedSemanticIndex): the candidates of a
// query sit on up to W shards, so their stored rows travel as exchange RECORDS and the
// selection runs where the query was asked.
//
// Record = one stored row, rowbytes a multiple of 16:
//     bf16 index: the row's D bf16 values, row-major                        (2 D bytes)
//     q16 index:  D int8 hi, D int8 lo, the row's fp32 scale, 12 zero bytes (2 D + 16 bytes)
// The all-zero record stands for "no row" (scale 0: every s_ij is 0).
//
// gather_rows_kernel (owner side): recs[i] = the record of local row rows[i]. One thread per
// 16-byte piece: piece p of row r is plane[r / 16][p / 4][16 (p % 4) + r % 16] of the
// fragment-major tiles (one 16-byte load, one 16-byte store). An id outside [0, nrows) -- the
// ids come from another rank -- writes zeros and never forms an address.
//
// mmr_rows_kernel (requester side): mmr_kernel (similarity_mmr.hip) with its operands taken from
// the records: slot [Q, m] indexes recs [R_total, rowbytes], the first entry that is negative or
// >= R_total ends the list and is never dereferenced. Lane (g, c) loads for slab s the 16 bytes
// rec + 64 s + 16 g of candidate 16 b + c (q16: the lo plane D bytes further on), which is
// exactly the fragment the tile kernel loads from plane[row / 16][s][16 g + row % 16]; the same
// MFMAs run in the same slab order, then the same select(). The picks are reported as list
// POSITIONS (the kernel never sees row ids), -1 past them.
#include "common.h"
#include "mmr_common.h"
#include "q16_exact.h"

namespace pa {
namespace mmr {

template <bool Q16>
__global__ __launch_bounds__(THREADS) void gather_rows_kernel(
    i32x4* __restrict__ recs, const int* __restrict__ rows, const i32x4* __restrict__ plane_a,
    const i32x4* __restrict__ plane_b, const float* __restrict__ rmeta, long long total, int ppr, int D,
    int nrows) {
  const long long idx = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= total) return;
  const long long i = idx / ppr;
  const int p = (int)(idx - i * ppr);
  const int r = rows[i];
  i32x4 v = i32x4{0, 0, 0, 0};
  if (r >= 0 && r < nrows) {
    const int pp = Q16 ? D / 16 : D / 8;  // pieces of one plane's row; 4 per k-slab
    const size_t tile = (size_t)(r >> 4) * pp * 16;  // pieces before the row's tile
    if (!Q16 || p < 2 * pp) {
      const i32x4* plane = (Q16 && p >= pp) ? plane_b : plane_a;
      const int e = (Q16 && p >= pp) ? p - pp : p;
      v = plane[tile + (size_t)(e >> 2) * 64 + 16 * (e & 3) + (r & 15)];
    } else {
      v[0] = __float_as_int(rmeta[2 * (size_t)r]);
    }
  }
  recs[idx] = v;
}

template <bool Q16>
__global__ __launch_bounds__(THREADS) void mmr_rows_kernel(
    float* __restrict__ out_s, int* __restrict__ out_p, const char* __restrict__ recs,
    const int* __restrict__ slot, const float* __restrict__ scores, const float* __restrict__ wr,
    const float* __restrict__ wd, int m, int K, int D, int nrecs) {
  __shared__ __attribute__((aligned(16))) float sim[MAXM * SLD];
  const int q = blockIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int g = lane >> 4, col = lane & 15;
  const size_t rowbytes = 2 * (size_t)D + (Q16 ? 16 : 0);
  const int sl = lane < m ? slot[(size_t)q * m + lane] : -1;
  const int n = list_len(sl, nrecs);
  const int nb = (n + 15) >> 4;  // groups that hold a candidate
  // candidate 16 b + col of every group; a lane without one loads candidate 0's fragment
  // (listed whenever a wave computes) and zeroes it
  const int sl0 = __shfl(sl, 0, 64);
  int cs[NG];
  bool cok[NG];
#pragma unroll
  for (int b = 0; b < NG; ++b) {
    const int r = __shfl(sl, 16 * b + col, 64);
    cok[b] = 16 * b + col < n;
    cs[b] = cok[b] ? r : sl0;
  }
  if (wid < nb) {  // wave-uniform
    const int S = D / (Q16 ? 64 : 32);  // k-slabs; 64 bytes of a record (plane) each
    size_t off[NG];                     // byte offset of this lane's 16 B in slab 0 of its record
#pragma unroll
    for (int b = 0; b < NG; ++b) off[b] = (size_t)cs[b] * rowbytes + 16 * g;
    f32x4 out[NG];
    if constexpr (Q16) {
      constexpr int KB = 2;  // slabs per load batch
      const char* hi = recs;
      const char* lo = recs + D;
      i32x4 hh[NG], hl[NG], lh[NG], ll[NG];
#pragma unroll
      for (int b = 0; b < NG; ++b) hh[b] = hl[b] = lh[b] = ll[b] = i32x4{0, 0, 0, 0};
      for (int s0 = 0; s0 < S; s0 += KB) {
        i32x4 fh[KB][NG], fl[KB][NG];
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          const size_t so = (size_t)min(s0 + u, S - 1) * 64;  // past D: re-read, never used
#pragma unroll
          for (int b = 0; b < NG; ++b) {
            const i32x4 zero = i32x4{0, 0, 0, 0};
            if (b < nb) {
              const i32x4 xh = *reinterpret_cast<const i32x4*>(hi + off[b] + so);
              const i32x4 xl = *reinterpret_cast<const i32x4*>(lo + off[b] + so);
              fh[u][b] = cok[b] ? xh : zero;
              fl[u][b] = cok[b] ? xl : zero;
            } else {
              fh[u][b] = fl[u][b] = zero;
            }
          }
        }
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          if (s0 + u >= S) break;
          const i32x4 ah = pick_group(fh[u], wid), al = pick_group(fl[u], wid);
#pragma unroll
          for (int b = 0; b < NG; ++b) {
            if (b < nb) {
              hh[b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, fh[u][b], hh[b], 0, 0, 0);
              hl[b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, fl[u][b], hl[b], 0, 0, 0);
              lh[b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, fh[u][b], lh[b], 0, 0, 0);
              ll[b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, fl[u][b], ll[b], 0, 0, 0);
            }
          }
        }
      }
      // lane holds (candidate i = 16 wid + 4 g + r, candidate j = 16 b + col); their row scales
      const float sc = lane < n ? *reinterpret_cast<const float*>(recs + (size_t)sl * rowbytes + 2 * (size_t)D) : 0.f;
      float si[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) si[r] = __shfl(sc, 16 * wid + 4 * g + r, 64);
#pragma unroll
      for (int b = 0; b < NG; ++b) {
        const float sj = __shfl(sc, 16 * b + col, 64);
#pragma unroll
        for (int r = 0; r < 4; ++r) out[b][r] = q16::exact_score(hh[b][r], hl[b][r], lh[b][r], ll[b][r], si[r], sj);
      }
    } else {
      constexpr int KB = 4;
#pragma unroll
      for (int b = 0; b < NG; ++b) out[b] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int s0 = 0; s0 < S; s0 += KB) {
        bf16x8 f[KB][NG];
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          const size_t so = (size_t)min(s0 + u, S - 1) * 64;
#pragma unroll
          for (int b = 0; b < NG; ++b) {
            const bf16x8 zero = bf16x8{};
            if (b < nb) {
              const bf16x8 x = *reinterpret_cast<const bf16x8*>(recs + off[b] + so);
              f[u][b] = cok[b] ? x : zero;
            } else {
              f[u][b] = zero;
            }
          }
        }
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          if (s0 + u >= S) break;
          const bf16x8 a = pick_group(f[u], wid);
#pragma unroll
          for (int b = 0; b < NG; ++b)
            if (b < nb) out[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, f[u][b], out[b], 0, 0, 0);
        }
      }
    }
    // C layout: register r of lane (g, col) is (i = 16 wid + 4 g + r, j = 16 b + col) -> sim[j][i..i+3]
#pragma unroll
    for (int b = 0; b < NG; ++b)
      if (b < nb) *reinterpret_cast<f32x4*>(sim + (16 * b + col) * SLD + 16 * wid + 4 * g) = out[b];
  }
  __syncthreads();
  if (wid == 0) {
    const float rel = lane < n ? scores[(size_t)q * m + lane] : 0.f;
    select(out_s + (size_t)q * K, out_p + (size_t)q * K, sim, rel, lane, n, K, wr[q], wd[q]);
  }
}

template <bool Q16>
int launch_gather(void* recs, const int* rows, const void* a, const void* b, const float* rmeta, long long n, int D,
                  int nrows, hipStream_t st) {
  const int ppr = Q16 ? D / 8 + 1 : D / 8;  // 16-byte pieces per record
  const long long total = n * ppr;
  const long long blocks = (total + THREADS - 1) / THREADS;
  if (blocks > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL(gather_rows_kernel<Q16>, dim3((unsigned)blocks), dim3(THREADS), 0, st,
                     reinterpret_cast<i32x4*>(recs), rows, reinterpret_cast<const i32x4*>(a),
                     reinterpret_cast<const i32x4*>(b), rmeta, total, ppr, D, nrows);
  return (int)hipGetLastError();
}

}  // namespace mmr
}  // namespace pa

// recs [n][2 D] bytes, rows [n], packed: bf16 tiles [nrows/16][D/32][64][8]. Returns 0, -1 for an
// unsupported shape, or a HIP error.
extern "C" int pa_gather_rows_bf16(void* recs, const int* rows, const void* packed, long long n, int D, int nrows,
                                   hipStream_t st) {
  if (n <= 0) return 0;
  if (D < 32 || D % 32 != 0 || nrows < 0) return -1;
  return pa::mmr::launch_gather<false>(recs, rows, packed, nullptr, nullptr, n, D, nrows, st);
}

// recs [n][2 D + 16] bytes; hi / lo: int8 planes [nrows/16][D/64][64][16], rmeta [nrows][2].
extern "C" int pa_gather_rows_q16(void* recs, const int* rows, const void* hi, const void* lo, const float* rmeta,
                                  long long n, int D, int nrows, hipStream_t st) {
  if (n <= 0) return 0;
  if (D < 64 || D % 64 != 0 || nrows < 0) return -1;
  return pa::mmr::launch_gather<true>(recs, rows, hi, lo, rmeta, n, D, nrows, st);
}

// recs [nrecs][2 D] bytes (16-byte aligned), slot / scores [Q][m], wr / wd [Q]; outputs [Q][K].
extern "C" int pa_mmr_select_rows_bf16(float* out_scores, int* out_pos, const void* recs, const int* slot,
                                       const float* scores, const float* wr, const float* wd, int Q, int m, int K,
                                       int D, int nrecs, hipStream_t st) {
  using namespace pa::mmr;
  if (Q <= 0) return 0;
  if (bad_shape(m, K, D, 32) || nrecs < 0) return -1;
  hipLaunchKernelGGL(mmr_rows_kernel<false>, dim3(Q), dim3(THREADS), 0, st, out_scores, out_pos,
                     reinterpret_cast<const char*>(recs), slot, scores, wr, wd, m, K, D, nrecs);
  return (int)hipGetLastError();
}

// recs [nrecs][2 D + 16] bytes; D <= 1024 (int32 sums).
extern "C" int pa_mmr_select_rows_q16(float* out_scores, int* out_pos, const void* recs, const int* slot,
                                      const float* scores, const float* wr, const float* wd, int Q, int m, int K,
                                      int D, int nrecs, hipStream_t st) {
  using namespace pa::mmr;
  if (Q <= 0) return 0;
  if (bad_shape(m, K, D, 64) || D > 1024 || nrecs < 0) return -1;
  hipLaunchKernelGGL(mmr_rows_kernel<true>, dim3(Q), dim3(THREADS), 0, st, out_scores, out_pos,
                     reinterpret_cast<const char*>(recs), slot, scores, wr, wd, m, K, D, nrecs);
  return (int)hipGetLastError();
}
