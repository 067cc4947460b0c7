// The exact score of two 16-bit fixed-point vectors (csrc/ops/similarity_q16.hip header): shared
// by the q16 scan (row x query) and the MMR re-ranking pass (row x row, similarity_mmr.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace pa {
namespace q16 {

// the exact score (see the header); the ONLY place the integer sums become a float
__device__ __forceinline__ float exact_score(int hh, int hl, int lh, int ll, float sr, float sq) {
  const long long I = (long long)hh * 65536 + ((long long)hl + (long long)lh) * 256 + (long long)ll;
  return (float)((double)I * ((double)sr * (double)sq));
}

}  // namespace q16
}  // namespace pa
