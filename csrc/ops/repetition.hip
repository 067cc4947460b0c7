// Repetition penalty (the HF / vLLM rule, with 1/r rounded once to fp32 on the host) on the raw
// LM-head logits, before the presence / frequency pass, logit_bias, the grammar mask, the
// thresholds, the sampler and the log-probability pass read them:
//
//     x = float(logit[t]);  logit[t] <- bf16( x > 0 ? x * inv_r : x * r )      for every t in S
//
// S = the distinct token ids of the request so far, prompt included (also the part of the prompt
// the prefix cache served: the scheduler keeps the ids). Each product is one correctly rounded
// fp32 multiplication (no division on the device: this library is built with -ffast-math) and
// one RNE conversion, so the pass agrees with the CPU reference bit for bit.
//
// The set lives in a per-request slot on the device and is kept in step by deltas: each step
// the scheduler sends a sampling row only the tokens it has not sent yet (the rep_tok region of
// the step buffer) -- the whole prompt once, a handful of tokens afterwards -- so the pass
// touches the new tokens plus |S| entries and never a whole 128K-entry row.
//
// State per slot: seen uint32 [words = ceil(V / 32)] (bit t & 31 of word t >> 5 = t is in S),
// list int32 [cap] (the members of S, each once, in arrival order), n_list int32. One workgroup
// per sampling row; a slot appears in at most one row of a step, so no state is shared between
// workgroups of a launch.
//
// Memory model: as in penalties.hip, every access to the three state arrays is an agent-scope
// atomic (performed at L2), so a bit set or an entry appended in phase (b) by one wave is what
// phase (c) of another wave reads after the workgroup barrier. The logits are written by an
// earlier kernel and each rewritten entry is read and written by one thread only.
#include "common.h"

namespace pa {

constexpr int REP_THREADS = 256;
constexpr int REP_UNROLL = 4;  // membership atomics in flight per thread while a backlog is inserted

#define REP_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// all earlier state atomics of this workgroup are complete before any later one is issued
__device__ __forceinline__ void rep_phase_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

__global__ __launch_bounds__(REP_THREADS) void apply_repetition_kernel(
    bf16* __restrict__ logits, int V, int ld, uint32_t* __restrict__ seen, int words, int* __restrict__ list,
    int* __restrict__ n_list, int slots, int cap, const int* __restrict__ rep_slot,
    const int* __restrict__ rep_reset, const float* __restrict__ rep_r, const float* __restrict__ rep_inv_r,
    const int* __restrict__ forced, const int* __restrict__ rep_start, const int* __restrict__ rep_n,
    const int* __restrict__ rep_tok, int tok_len) {
  const int row = blockIdx.x;
  const int slot = rep_slot[row];
  if (slot < 0 || slot >= slots || forced[row] >= 0) return;  // uniform per workgroup
  uint32_t* bits = seen + (size_t)slot * words;
  int* lst = list + (size_t)slot * cap;
  int* nl = n_list + slot;
  const int tid = threadIdx.x;

  // (a) recycle the slot: zero the membership words its old list names
  if (rep_reset[row] != 0) {
    const int n_old = min(max(__hip_atomic_load(nl, REP_RLX), 0), cap);
    for (int i = tid; i < n_old; i += REP_THREADS) {
      const int t = __hip_atomic_load(lst + i, REP_RLX);
      if (t >= 0 && t < V) __hip_atomic_store(bits + (t >> 5), 0u, REP_RLX);
    }
    rep_phase_barrier();  // every thread has read n_list
    if (tid == 0) __hip_atomic_store(nl, 0, REP_RLX);
    rep_phase_barrier();
  }

  // (b) insert the row's new tokens; the thread that flips a token's bit appends the token
  int start = rep_start[row], n_new = rep_n[row];
  if (start < 0 || n_new < 0 || start > tok_len - n_new) n_new = 0;
  for (int i0 = 0; i0 < n_new; i0 += REP_THREADS * REP_UNROLL) {
    int t[REP_UNROLL];
    uint32_t old[REP_UNROLL];
#pragma unroll
    for (int u = 0; u < REP_UNROLL; ++u) {
      const int i = i0 + u * REP_THREADS + tid;
      t[u] = i < n_new ? rep_tok[start + i] : -1;
      if (t[u] >= V) t[u] = -1;
    }
#pragma unroll
    for (int u = 0; u < REP_UNROLL; ++u)
      old[u] = t[u] >= 0 ? __hip_atomic_fetch_or(bits + (t[u] >> 5), 1u << (t[u] & 31), REP_RLX) : ~0u;
#pragma unroll
    for (int u = 0; u < REP_UNROLL; ++u) {
      if (t[u] < 0 || ((old[u] >> (t[u] & 31)) & 1u)) continue;
      const int at = __hip_atomic_fetch_add(nl, 1, REP_RLX);
      if (at >= 0 && at < cap) __hip_atomic_store(lst + at, t[u], REP_RLX);
    }
  }
  rep_phase_barrier();

  // (c) rewrite the logits of the listed tokens (each listed once: one thread per logit)
  const float r = rep_r[row], inv_r = rep_inv_r[row];
  const int n = min(max(__hip_atomic_load(nl, REP_RLX), 0), cap);
  bf16* lr = logits + (size_t)row * ld;
  for (int i = tid; i < n; i += REP_THREADS) {
    const int t = __hip_atomic_load(lst + i, REP_RLX);
    if (t < 0 || t >= V) continue;
    const float x = bf2f(lr[t]);
    // one correctly rounded fp32 product, then one RNE conversion
    lr[t] = f2bf(__fmul_rn(x, x > 0.f ? inv_r : r));
  }
}

}  // namespace pa

// logits [rows, ld] bf16 (V <= ld: the padding is not touched); seen [slots, words] with
// words * 32 >= V, list [slots, cap], n_list [slots]; per-row arrays of >= rows entries;
// rep_tok [tok_len].
extern "C" int pa_apply_repetition_penalty(void* logits, int rows, int V, int ld, uint32_t* seen, int words,
                                           int* list, int* n_list, int slots, int cap, const int* rep_slot,
                                           const int* rep_reset, const float* rep_r, const float* rep_inv_r,
                                           const int* forced, const int* rep_start, const int* rep_n,
                                           const int* rep_tok, int tok_len, hipStream_t st) {
  if (rows <= 0) return 0;
  if (V <= 0 || ld < V || slots <= 0 || cap <= 0 || tok_len < 0 || (int64_t)words * 32 < V) return -1;
  hipLaunchKernelGGL(pa::apply_repetition_kernel, dim3(rows), dim3(pa::REP_THREADS), 0, st, (pa::bf16*)logits,
                     V, ld, seen, words, list, n_list, slots, cap, rep_slot, rep_reset, rep_r, rep_inv_r,
                     forced, rep_start, rep_n, rep_tok, tok_len);
  return (int)hipGetLastError();
}
