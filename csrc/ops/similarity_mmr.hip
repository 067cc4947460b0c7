// Diversity-aware re-ranking of a semantic-search candidate list: maximal marginal relevance
// (MMR) over the HBM-resident index (memory/semantic_index.py search(diversity=)).
//
// Input per query: the filtered top-m of the scan (similarity.hip / similarity_q16.hip), best
// first: rows [Q, m] int32 (-1 past the hits), scores [Q, m] fp32 (rel_i, the cosine of row i
// and the query), and the weights wr = float32(1 - d), wd = float32(d) of the query's diversity
// d. Output: the k rows picked greedily,
//     pick = argmax over the open candidates of   (wr * rel_i) - (wd * M_i),
//     M_i  = max of s_ij over the candidates j picked so far (first step: the subtrahend is 0),
// three separately rounded fp32 operations (no fma), ties (with -0 == +0) to the smaller list
// position; each pick is reported with its cosine rel, entries past the picks are (-inf, -1).
// s_ij is the similarity of the STORED rows i and j:
//     bf16 index: the dot product of the two bf16 rows, accumulated in fp32 by the MFMA;
//     q16 index:  exact_score of the two fixed-point rows (q16_exact.h) -- exact integer dot
//                 products, so the kernel and ops/reference.py agree bit for bit.
// Scores must be finite (they are cosines).
//
// One 4-wave workgroup per query (grid = Q, any Q). The <= 64 candidates form four groups of
// 16. For every k-slab (32 dims bf16, 64 dims q16) lane (g = l >> 4, c = l & 15) gathers the
// 16 bytes of candidate 16 b + c straight from the fragment-major tile of its row,
//     plane[row / 16][slab][16 g + row % 16],
// which is that candidate's piece of an A operand of v_mfma_f32_16x16x32_bf16 /
// v_mfma_i32_16x16x64_i8 -- and, the layouts being the same, of a B operand. Wave w multiplies
// group w (A) by groups 0..3 (B): the Gram blocks (w, 0..3), accumulated over all slabs in
// registers (q16: hh / hl / lh / ll int32 sums, exact for D <= 1024 as in the scan). Nothing is
// staged per dimension in LDS, so every D the scans accept works. The 64 x 64 fp32 matrix goes
// to LDS; wave 0 then selects with one lane per candidate (M_i in a register, wave argmax by
// max + ballot, the winner's column read from LDS). Lanes past the list and lists' -1 entries
// never form an address from their row id: they read a listed row's fragment and zero it.
#include "common.h"
#include "mmr_common.h"
#include "q16_exact.h"

namespace pa {
namespace mmr {

template <bool Q16>
__global__ __launch_bounds__(THREADS) void mmr_kernel(
    float* __restrict__ out_s, int* __restrict__ out_r, const int* __restrict__ rows,
    const float* __restrict__ scores, const void* __restrict__ plane_a, const void* __restrict__ plane_b,
    const float* __restrict__ rmeta, const float* __restrict__ wr, const float* __restrict__ wd, int m, int K,
    int D, int nrows) {
  __shared__ __attribute__((aligned(16))) float sim[MAXM * SLD];
  const int q = blockIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int row = lane < m ? rows[(size_t)q * m + lane] : -1;
  const int n = list_len(row, nrows);
  const int nb = (n + 15) >> 4;  // groups that hold a candidate
  // candidate 16 b + col of every group; a lane without one gathers candidate 0's fragment
  // (listed whenever a wave computes) and zeroes it
  const int row0 = __shfl(row, 0, 64);
  int crow[NG];
  bool cok[NG];
#pragma unroll
  for (int b = 0; b < NG; ++b) {
    const int r = __shfl(row, 16 * b + col, 64);
    cok[b] = 16 * b + col < n;
    crow[b] = cok[b] ? r : row0;
  }
  if (wid < nb) {  // wave-uniform
    const int S = D / (Q16 ? 64 : 32);  // k-slabs; 1 KiB of a tile each
    size_t off[NG];                     // byte offset of this lane's 16 B in slab 0 of its row's tile
#pragma unroll
    for (int b = 0; b < NG; ++b)
      off[b] = ((size_t)(crow[b] >> 4) * S * 64 + 16 * g + (crow[b] & 15)) * 16;
    f32x4 out[NG];
    if constexpr (Q16) {
      constexpr int KB = 2;  // slabs per load batch
      const char* hi = reinterpret_cast<const char*>(plane_a);
      const char* lo = reinterpret_cast<const char*>(plane_b);
      i32x4 hh[NG], hl[NG], lh[NG], ll[NG];
#pragma unroll
      for (int b = 0; b < NG; ++b) hh[b] = hl[b] = lh[b] = ll[b] = i32x4{0, 0, 0, 0};
      for (int s0 = 0; s0 < S; s0 += KB) {
        i32x4 fh[KB][NG], fl[KB][NG];
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          const size_t so = (size_t)min(s0 + u, S - 1) * 1024;  // past D: re-read, never used
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
      const float sc = lane < n ? rmeta[2 * (size_t)row] : 0.f;
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
      const char* pk = reinterpret_cast<const char*>(plane_a);
#pragma unroll
      for (int b = 0; b < NG; ++b) out[b] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int s0 = 0; s0 < S; s0 += KB) {
        bf16x8 f[KB][NG];
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          const size_t so = (size_t)min(s0 + u, S - 1) * 1024;
#pragma unroll
          for (int b = 0; b < NG; ++b) {
            const bf16x8 zero = bf16x8{};
            if (b < nb) {
              const bf16x8 x = *reinterpret_cast<const bf16x8*>(pk + off[b] + so);
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
    select(out_s + (size_t)q * K, out_r + (size_t)q * K, sim, rel, row, n, K, wr[q], wd[q]);
  }
}

}  // namespace mmr
}  // namespace pa

// rows / scores [Q][m] (the scan's output for K = m), packed: bf16 tiles [nrows/16][D/32][64][8];
// wr / wd [Q]; outputs [Q][K]. Returns 0, -1 for an unsupported shape, or a HIP error.
extern "C" int pa_mmr_select_bf16(float* out_scores, int* out_rows, const int* rows, const float* scores,
                                  const void* packed, const float* wr, const float* wd, int Q, int m, int K, int D,
                                  int nrows, hipStream_t st) {
  using namespace pa::mmr;
  if (Q <= 0) return 0;
  if (bad_shape(m, K, D, 32)) return -1;
  hipLaunchKernelGGL(mmr_kernel<false>, dim3(Q), dim3(THREADS), 0, st, out_scores, out_rows, rows, scores, packed,
                     (const void*)nullptr, (const float*)nullptr, wr, wd, m, K, D, nrows);
  return (int)hipGetLastError();
}

// hi / lo: int8 planes [nrows/16][D/64][64][16], rmeta [nrows][2] (s_r, .); D <= 1024 (int32 sums).
extern "C" int pa_mmr_select_q16(float* out_scores, int* out_rows, const int* rows, const float* scores,
                                 const void* hi, const void* lo, const float* rmeta, const float* wr, const float* wd,
                                 int Q, int m, int K, int D, int nrows, hipStream_t st) {
  using namespace pa::mmr;
  if (Q <= 0) return 0;
  if (bad_shape(m, K, D, 64) || D > 1024) return -1;
  hipLaunchKernelGGL(mmr_kernel<true>, dim3(Q), dim3(THREADS), 0, st, out_scores, out_rows, rows, scores, hi, lo,
                     rmeta, wr, wd, m, K, D, nrows);
  return (int)hipGetLastError();
}
