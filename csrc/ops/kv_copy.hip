// Partial-block KV copy for the prefix cache (runtime/block_manager.h "donor index").
//
// A prompt that matches a cached block only in its first j < 16 tokens takes those j key slots
// from the cached ("donor") block instead of computing them again: the scheduler lists
// (donor block, new block, j) triples for the step, and this kernel -- the first node of every
// step graph, before layer 0 writes any KV -- copies the slots in every layer and KV head. A
// later copy of the list may read what an earlier one wrote only across launches: the
// scheduler never lists a block as donor and as destination in one step.
//   K page [16 dim chunks][16 slots][8]: slots 0..j-1 of a chunk are one run of j x 16 B
//   V page [128 dims][16 slots]:        slots 0..j-1 of a dim are j x 2 B
// (layouts: rope_cache.hip). The copy count is read from device memory, so the launch has the
// same shape in every step (hipGraph capture); a step without copies exits at once. Slots at or
// beyond j of the new block are not touched.
#include "common.h"

namespace pa {

constexpr int KVC_BLK = 16;                  // slots per page
constexpr int KVC_PAGE = 128 * KVC_BLK;      // bf16 elements of one (block, KV head) page

// grid (layers * KV), 256 threads: one workgroup per (layer, KV head) walks the step's copies
// (a step has a handful at most; 256 workgroups that find a zero count cost a step nothing)
__global__ __launch_bounds__(256) void kv_copy_kernel(bf16* __restrict__ k_cache, bf16* __restrict__ v_cache,
                                                      const int* __restrict__ n_copies,
                                                      const int* __restrict__ copies, int max_copies,
                                                      int num_blocks, int KV, long layer_stride) {
  const int n = min(*n_copies, max_copies);
  if (n <= 0) return;
  const int layer = blockIdx.x / KV, h = blockIdx.x % KV;
  const size_t base = (size_t)layer * layer_stride;
  const int t = threadIdx.x;
  for (int c = 0; c < n; ++c) {
    const int src = copies[3 * c], dst = copies[3 * c + 1];
    const int j = min(copies[3 * c + 2], KVC_BLK);
    if (j <= 0 || src == dst || (unsigned)src >= (unsigned)num_blocks || (unsigned)dst >= (unsigned)num_blocks)
      continue;
    const size_t so = base + ((size_t)src * KV + h) * KVC_PAGE, dof = base + ((size_t)dst * KV + h) * KVC_PAGE;
    // K: thread = (chunk, slot), one 16-byte vector each
    if ((t & 15) < j) {
      const uint4* ks = reinterpret_cast<const uint4*>(k_cache + so);
      uint4* kd = reinterpret_cast<uint4*>(k_cache + dof);
      kd[t] = ks[t];
    }
    // V: thread = (dim, half row of 8 slots): one 16-byte load, the first j slots stored one by one
    const int half = t & 1;
    if (half * 8 < j) {
      const uint4 raw = reinterpret_cast<const uint4*>(v_cache + so)[t];
      const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
      unsigned short* vd = reinterpret_cast<unsigned short*>(v_cache + dof) + (size_t)t * 8;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (half * 8 + i < j) vd[i] = (unsigned short)(w[i >> 1] >> ((i & 1) * 16));
    }
  }
}

}  // namespace pa

// k_cache / v_cache: [layers][num_blocks][KV][page]; n_copies: one device word; copies: device
// words (src, dst, j) x max_copies. layer_stride in elements.
extern "C" int pa_kv_copy(void* k_cache, void* v_cache, const int* n_copies, const int* copies,
                          int max_copies, int layers, int num_blocks, int KV, long layer_stride,
                          int block_size, hipStream_t st) {
  if (max_copies <= 0 || layers <= 0 || KV <= 0) return 0;
  if (block_size != pa::KVC_BLK) return -1;
  hipLaunchKernelGGL(pa::kv_copy_kernel, dim3(layers * KV), dim3(256), 0, st, (pa::bf16*)k_cache,
                     (pa::bf16*)v_cache, n_copies, copies, max_copies, num_blocks, KV, layer_stride);
  return (int)hipGetLastError();
}
