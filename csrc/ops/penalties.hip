// Presence / frequency penalties (OpenAI semantics) on the LM-head logits, before the
// top-k / top-p threshold, the sampler and the log-probability pass read them:
//
//     logit[t] <- bf16( float(logit[t]) - (presence * [c_t > 0] + frequency * c_t) )
//
// c_t = occurrences of token t among the request's GENERATED tokens so far. The counts live
// in a per-request "penalty slot" on the device and are kept in step by deltas: each step the
// scheduler sends a sampling row only the generated tokens it has not sent yet (the pair
// region of the step buffer), so the pass touches a handful of new tokens plus the slot's
// distinct tokens and never a whole 128K-entry row.
//
// State per slot: counts int32 [V], distinct int32 [cap] (the tokens with a non-zero count, in
// arrival order), n_distinct int32. One workgroup per sampling row; a slot appears in at most
// one row of a step, so no state is shared between workgroups of a launch.
//
// Memory model: every access to the three state arrays is an agent-scope atomic (performed at
// L2), so a count added in phase (b) by one wave is what phase (c) of another wave reads after
// the workgroup barrier -- no per-CU L1 line of the state is ever read. The logits are written
// by an earlier kernel and each rewritten entry is read and written by one thread only.
#include "common.h"

namespace pa {

constexpr int PEN_THREADS = 256;

#define PEN_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// all earlier state atomics of this workgroup are complete before any later one is issued
__device__ __forceinline__ void pen_phase_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

__global__ __launch_bounds__(PEN_THREADS) void apply_penalties_kernel(
    bf16* __restrict__ logits, int V, int ld, int* __restrict__ counts, int* __restrict__ distinct,
    int* __restrict__ n_distinct, int slots, int cap, const int* __restrict__ pen_slot,
    const int* __restrict__ pen_reset, const float* __restrict__ presence,
    const float* __restrict__ frequency, const int* __restrict__ forced,
    const int* __restrict__ pair_start, const int* __restrict__ pair_n,
    const int* __restrict__ pair_tok, int pair_len) {
  const int row = blockIdx.x;
  const int slot = pen_slot[row];
  if (slot < 0 || slot >= slots || forced[row] >= 0) return;  // uniform per workgroup
  int* cnt = counts + (size_t)slot * V;
  int* lst = distinct + (size_t)slot * cap;
  int* nd = n_distinct + slot;
  const int tid = threadIdx.x;

  // (a) recycle the slot: zero the counts its old list names
  if (pen_reset[row] != 0) {
    const int n_old = min(max(__hip_atomic_load(nd, PEN_RLX), 0), cap);
    for (int i = tid; i < n_old; i += PEN_THREADS) {
      const int t = __hip_atomic_load(lst + i, PEN_RLX);
      if (t >= 0 && t < V) __hip_atomic_store(cnt + t, 0, PEN_RLX);
    }
    pen_phase_barrier();  // every thread has read n_distinct
    if (tid == 0) __hip_atomic_store(nd, 0, PEN_RLX);
    pen_phase_barrier();
  }

  // (b) count the row's new tokens; the thread that takes a count from 0 appends the token
  int start = pair_start[row], n_new = pair_n[row];
  if (start < 0 || n_new < 0 || start > pair_len - n_new) n_new = 0;
  for (int i = tid; i < n_new; i += PEN_THREADS) {
    const int t = pair_tok[start + i];
    if (t < 0 || t >= V) continue;
    if (__hip_atomic_fetch_add(cnt + t, 1, PEN_RLX) == 0) {
      const int at = __hip_atomic_fetch_add(nd, 1, PEN_RLX);
      if (at >= 0 && at < cap) __hip_atomic_store(lst + at, t, PEN_RLX);
    }
  }
  pen_phase_barrier();

  // (c) rewrite the logits of the distinct tokens (each listed once: one thread per logit)
  const float a = presence[row], b = frequency[row];
  const int n = min(max(__hip_atomic_load(nd, PEN_RLX), 0), cap);
  bf16* lr = logits + (size_t)row * ld;
  for (int i = tid; i < n; i += PEN_THREADS) {
    const int t = __hip_atomic_load(lst + i, PEN_RLX);
    if (t < 0 || t >= V) continue;
    const int c = __hip_atomic_load(cnt + t, PEN_RLX);
    if (c <= 0) continue;
    // separately rounded fp32 operations (no contraction), then one RNE conversion
    const float pen = __fadd_rn(a, __fmul_rn(b, (float)c));
    lr[t] = f2bf(__fsub_rn(bf2f(lr[t]), pen));
  }
}

}  // namespace pa

// logits [rows, ld] bf16 (V <= ld: the padding is not touched); counts [slots, V], distinct
// [slots, cap], n_distinct [slots]; per-row arrays of >= rows entries; pair_tok [pair_len].
extern "C" int pa_apply_penalties(void* logits, int rows, int V, int ld, int* counts, int* distinct,
                                  int* n_distinct, int slots, int cap, const int* pen_slot,
                                  const int* pen_reset, const float* presence, const float* frequency,
                                  const int* forced, const int* pair_start, const int* pair_n,
                                  const int* pair_tok, int pair_len, hipStream_t st) {
  if (rows <= 0) return 0;
  if (V <= 0 || ld < V || slots <= 0 || cap <= 0 || pair_len < 0) return -1;
  hipLaunchKernelGGL(pa::apply_penalties_kernel, dim3(rows), dim3(pa::PEN_THREADS), 0, st, (pa::bf16*)logits,
                     V, ld, counts, distinct, n_distinct, slots, cap, pen_slot, pen_reset, presence,
                     frequency, forced, pair_start, pair_n, pair_tok, pair_len);
  return (int)hipGetLastError();
}
