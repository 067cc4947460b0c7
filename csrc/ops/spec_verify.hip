// Acceptance pass of a draft step (predicted outputs / prompt-lookup drafts).
//
// A drafting request enters a step with the run [last real token, d_0 .. d_{k-1}] and owns
// 1 + k consecutive sampling rows; row j holds the logits behind the first j draft tokens. The
// sampler's noise is keyed on (seed, position, vocab index), so row j samples exactly the token
// y_j a one-token decode step would sample at that position -- provided the draft tokens before
// it were right. Verification is therefore plain equality: a = the number of leading j < k with
// y_j == d_j, and the step emits y_0 .. y_a.
//
// This kernel is the sampler's final merge (sample_final_kernel, sampling.hip) plus that check,
// in one launch that takes sample_final_kernel's place in the draft-step graphs:
//   merge    out_tokens[row] = forced[row] >= 0 ? forced[row] : the id of the best of the row's
//            nchunk partial (key, id) pairs -- larger key first, equal keys by smaller id; a row
//            with no allowed token (every id 0x7fffffff) gives 0.
//   accept   d_j = input_ids[logit_rows[first + j + 1]], the input token of the run's next row.
//   write    accept_len[first row of a run] = a + 1, every other row 0; a plain row is a run of
//            length 1 and gets 1.
//
// Work split, chosen for robustness over the last microsecond (the launch reads a few hundred
// partials per run): one 64-lane workgroup per ROW merges that row and writes its token, so every
// row is written whatever the run descriptors say; the workgroup of a run's FIRST row then walks
// the run's rows in order, merging each again (nchunk / 64 strided loads and one wave reduction
// per row, <= 9 rows) until the first mismatch. No workgroup reads what another one writes, so
// nothing depends on dispatch order, and there are no flags or atomics.
//
// The run descriptors come from a host buffer: a pair that is not a valid run of this launch
// (first outside [0, row], row outside the run, the run past `rows`, length < 1) makes the row a
// run of its own; a logit row outside [0, n_ids) ends the acceptance there. Nothing is read or
// written out of range for any descriptor contents.
//
// Compiled with -ffast-math (no-infs) like the sampler: keys are compared as integers (the usual
// monotone map of the float bits, -0 folded into +0), which orders -inf partials exactly too.
#include "common.h"

namespace pa {

__device__ __forceinline__ int sv_order(float k) {
  int b = __float_as_int(k);
  if (b == (int)0x80000000u) b = 0;           // -0 == +0
  return b >= 0 ? b : (b ^ 0x7fffffff);       // monotone: float order == signed int order
}

// the row's token: every lane of the wave calls it, every lane gets the result
__device__ __forceinline__ int sv_merge_row(const float* __restrict__ part_k, const int* __restrict__ part_i,
                                            const int* __restrict__ forced, int row, int nchunk) {
  int bk = (int)0x80000000u, bi = 0x7fffffff;  // below every key
  const size_t base = (size_t)row * nchunk;
  for (int c = threadIdx.x; c < nchunk; c += 64) {
    const int k = sv_order(part_k[base + c]);
    const int i = part_i[base + c];
    if (k > bk || (k == bk && i < bi)) { bk = k; bi = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int k = __shfl_xor(bk, o, 64), i = __shfl_xor(bi, o, 64);
    if (k > bk || (k == bk && i < bi)) { bk = k; bi = i; }
  }
  const int f = forced[row];
  return f >= 0 ? f : (bi == 0x7fffffff ? 0 : bi);
}

__global__ __launch_bounds__(64) void spec_verify_kernel(
    int* __restrict__ out_tokens, int* __restrict__ accept_len, const float* __restrict__ part_k,
    const int* __restrict__ part_i, const int* __restrict__ forced, const int* __restrict__ input_ids,
    int n_ids, const int* __restrict__ logit_rows, const int* __restrict__ run_first,
    const int* __restrict__ run_len, int rows, int nchunk) {
  const int row = blockIdx.x;
  if (row >= rows) return;
  const int y = sv_merge_row(part_k, part_i, forced, row, nchunk);
  int first = run_first[row], len = run_len[row];
  if (first < 0 || first > row || len < 1 || len > rows - first || row - first >= len) {
    first = row;  // not a run of this launch: the row stands alone
    len = 1;
  }
  if (first != row) {  // uniform over the workgroup
    if (threadIdx.x == 0) {
      out_tokens[row] = y;
      accept_len[row] = 0;
    }
    return;
  }
  // first row of a run: y_j against the input token of row j + 1, in order
  int a = 0, yj = y;
  while (a + 1 < len) {
    const int lr = logit_rows[row + a + 1];  // row + a + 1 < first + len <= rows
    if (lr < 0 || lr >= n_ids || input_ids[lr] != yj) break;
    ++a;
    yj = sv_merge_row(part_k, part_i, forced, row + a, nchunk);
  }
  if (threadIdx.x == 0) {
    out_tokens[row] = y;
    accept_len[row] = a + 1;
  }
}

}  // namespace pa

// part_k / part_i: [rows, nchunk] as sample_chunk_kernel leaves them; forced, logit_rows,
// run_first, run_len, out_tokens, accept_len: [rows]; input_ids: [n_ids].
extern "C" int pa_spec_verify(int* out_tokens, int* accept_len, const float* part_k, const int* part_i,
                              const int* forced, const int* input_ids, int n_ids, const int* logit_rows,
                              const int* run_first, const int* run_len, int rows, int nchunk,
                              hipStream_t st) {
  if (rows <= 0) return 0;
  if (nchunk < 1 || n_ids < 0) return -1;
  hipLaunchKernelGGL(pa::spec_verify_kernel, dim3(rows), dim3(64), 0, st, out_tokens, accept_len, part_k,
                     part_i, forced, input_ids, n_ids, logit_rows, run_first, run_len, rows, nchunk);
  return (int)hipGetLastError();
}
