// Whole-block KV moves for the prefix cache's host tier (runtime/block_manager.h "Host tier").
//
// An evicted block is spilled to pinned host memory and a later prompt whose hash chain reaches
// it gets it back instead of computing it again. The host copies are plain async memcpys of
// whole records; these two launches pack the pages of the listed blocks -- strided over layers
// and the K / V pools -- into contiguous records of a device staging buffer, and unpack them:
//   record i = [layer][K|V][KV][page], page = 2048 bf16 (4 KiB)    (layers x 2 x KV x 4 KiB)
// (cache layouts: kv_copy.hip). One workgroup per (record, layer, K|V) moves KV x 4 KiB that is
// contiguous on both sides, 16 bytes per lane and access, PG_INFLIGHT loads in flight before
// their stores. Every byte is touched once: the staging side is read / written non-temporally.
// The block list is device memory, its length a plain launch argument (these launches run
// between steps, never inside a captured graph); an id outside [0, num_blocks) skips its
// record, as kv_copy skips a copy.
#include "common.h"

namespace pa {

constexpr int PG_PAGE = 128 * 16;  // bf16 elements of one (block, KV head) page
constexpr int PG_VEC = PG_PAGE / 8;  // 16-byte vectors of a page
constexpr int PG_THREADS = 256;
constexpr int PG_INFLIGHT = 4;

// grid (n, layers * 2), 256 threads. GATHER: cache -> stage; else stage -> cache.
template <bool GATHER>
__global__ __launch_bounds__(PG_THREADS) void kv_pages_kernel(bf16* __restrict__ k_cache, bf16* __restrict__ v_cache,
                                                              const int* __restrict__ ids, bf16* __restrict__ stage,
                                                              int num_blocks, int KV, int layers, long layer_stride) {
  const int rec = blockIdx.x;
  const int layer = blockIdx.y >> 1, sel = blockIdx.y & 1;
  const int blk = ids[rec];
  if ((unsigned)blk >= (unsigned)num_blocks) return;
  bf16* cache = sel ? v_cache : k_cache;
  u32x4* cp = reinterpret_cast<u32x4*>(cache + (size_t)layer * layer_stride + (size_t)blk * KV * PG_PAGE);
  u32x4* sp = reinterpret_cast<u32x4*>(stage + (((size_t)rec * layers + layer) * 2 + sel) * (size_t)KV * PG_PAGE);
  // a page is PG_THREADS vectors, so the workgroup moves KV whole passes of one vector per thread:
  // rounds of PG_INFLIGHT passes with every load issued unconditionally before the first store,
  // then the KV % PG_INFLIGHT passes that are left, one at a time
  const int nvec = KV * PG_VEC;
  int i = threadIdx.x;
  for (; i + (PG_INFLIGHT - 1) * PG_THREADS < nvec; i += PG_INFLIGHT * PG_THREADS) {
    u32x4 x[PG_INFLIGHT];
#pragma unroll
    for (int u = 0; u < PG_INFLIGHT; ++u)
      x[u] = GATHER ? cp[i + u * PG_THREADS] : __builtin_nontemporal_load(sp + i + u * PG_THREADS);
#pragma unroll
    for (int u = 0; u < PG_INFLIGHT; ++u) {
      if (GATHER) __builtin_nontemporal_store(x[u], sp + i + u * PG_THREADS);
      else cp[i + u * PG_THREADS] = x[u];
    }
  }
  for (; i < nvec; i += PG_THREADS) {
    const u32x4 x = GATHER ? cp[i] : __builtin_nontemporal_load(sp + i);
    if (GATHER) __builtin_nontemporal_store(x, sp + i);
    else cp[i] = x;
  }
}
static_assert(PG_VEC == PG_THREADS, "one vector of a page per thread and pass");

template <bool GATHER>
static int kv_pages_launch(void* k_cache, void* v_cache, const int* ids, int n, void* stage, int layers,
                           int num_blocks, int KV, long layer_stride, int block_size, hipStream_t st) {
  if (n <= 0 || layers <= 0 || KV <= 0) return 0;
  if (block_size != 16 || layers * 2 > 65535) return -1;
  hipLaunchKernelGGL(kv_pages_kernel<GATHER>, dim3(n, layers * 2), dim3(PG_THREADS), 0, st, (bf16*)k_cache,
                     (bf16*)v_cache, ids, (bf16*)stage, num_blocks, KV, layers, layer_stride);
  return (int)hipGetLastError();
}

}  // namespace pa

// k_cache / v_cache: [layers][num_blocks][KV][page]; ids: n device words; stage: n records.
// layer_stride in elements.
extern "C" int pa_kv_gather_blocks(void* k_cache, void* v_cache, const int* ids, int n, void* stage, int layers,
                                   int num_blocks, int KV, long layer_stride, int block_size, hipStream_t st) {
  return pa::kv_pages_launch<true>(k_cache, v_cache, ids, n, stage, layers, num_blocks, KV, layer_stride,
                                   block_size, st);
}

extern "C" int pa_kv_scatter_blocks(void* k_cache, void* v_cache, const int* ids, int n, void* stage, int layers,
                                    int num_blocks, int KV, long layer_stride, int block_size, hipStream_t st) {
  return pa::kv_pages_launch<false>(k_cache, v_cache, ids, n, stage, layers, num_blocks, KV, layer_stride,
                                    block_size, st);
}
