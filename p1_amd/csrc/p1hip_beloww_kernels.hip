// p1hip_beloww_kernels.hip -- the fifth gfx950 code object of libp1hip.so: the
// filter kernel of p1hip_scan_below_batch_wide (hard-target searches that share
// k_scan launches).
//
// It hashes nothing: it reads the partials k_scan and k_batch_scan left on the
// device, so it compiles in a second and needs no tools/isa_post.py pass; it is
// built device-only, linked into build/p1hip_beloww.hsaco and embedded by
// p1hip_beloww_blob.S after the other four objects, which stay as they are.
// The ABI with the host runtime is beloww_abi.hpp.
#include <hip/hip_runtime.h>

#include "beloww_abi.hpp"

using namespace p1;

// One workgroup per request: an order-preserving compaction of the request's
// candidate tiles.  It walks the request's ranges in table order and each range
// in chunks of kBlock tiles, one partial per thread (beloww_thread).  Per
// chunk: the wave's ballot of the flags, the lane's rank from the popcount of
// the lower lanes, the four wave totals through LDS, and `base`, the
// candidates of all earlier chunks.  The range bounds, the slot bounds and the
// target depend on blockIdx alone (scalar loads), and `base` is computed by
// every thread from the same LDS values, so the trip counts are uniform: the
// barrier inside the loop is reached by the whole workgroup.  A flagged tile
// whose rank is below the request's slot count writes its index in the partial
// array to its slot, so the indices come out in table order and nothing past
// the request's slots is written.  The loop does not end once the slots are
// full: count[r] is the total, which tells the host that it has to look at
// the partials itself.  No atomics, no memset; nothing one workgroup writes is
// read by another; every store is an ordinary vector store.
//
// The LDS totals are double-buffered: chunk i + 2 rewrites what chunk i read,
// and the barrier of chunk i + 1 lies between the two.
extern "C" __global__ __launch_bounds__(kBlock) void k_beloww_filter(const Key* __restrict__ part,
                                                                     const WideRange* __restrict__ ranges,
                                                                     const uint32_t* __restrict__ req_range0,
                                                                     const uint64_t* __restrict__ targets,
                                                                     const uint32_t* __restrict__ req_slot0,
                                                                     uint32_t* __restrict__ cand,
                                                                     uint32_t* __restrict__ count) {
  constexpr uint32_t kWaves = kBlock / 64;
  __shared__ uint32_t wave_sum[2][kWaves];
  const uint32_t r = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t j0 = req_range0[r], j1 = req_range0[r + 1];
  const uint32_t s0 = req_slot0[r], slots = req_slot0[r + 1] - s0;
  const uint64_t target = targets[r];
  const uint64_t lower_lanes = (1ull << lane) - 1u;
  uint32_t base = 0, buf = 0;
  for (uint32_t j = j0; j < j1; ++j) {
    const WideRange R = ranges[j];
    for (uint32_t c0 = 0; c0 < R.ntiles; c0 += kBlock, buf ^= 1u) {
      uint32_t tile;
      const bool hit = beloww_thread(part, R, c0, tid, target, &tile);  // the last chunk may be ragged
      const uint64_t word = __ballot(hit);
      if (lane == 0) wave_sum[buf][wave] = (uint32_t)__popcll(word);
      __syncthreads();
      uint32_t before = 0, total = 0;
      for (uint32_t i = 0; i < kWaves; ++i) {
        const uint32_t s = wave_sum[buf][i];
        if (i < wave) before += s;
        total += s;
      }
      const uint32_t rank = base + before + (uint32_t)__popcll(word & lower_lanes);
      if (hit && rank < slots) cand[s0 + rank] = tile;
      base += total;
    }
  }
  if (tid == 0) count[r] = base;
}
