// p1hip_belowb_kernels.hip -- the fourth gfx950 code object of libp1hip.so:
// the two kernels of p1hip_scan_below_batch (many target searches in one
// launch pair).
//
// Only the generic per-thread path (scan_core.hpp generic_thread), so it
// compiles in seconds and needs no tools/isa_post.py pass; it is built
// device-only, linked into build/p1hip_belowb.hsaco and embedded by
// p1hip_belowb_blob.S after the other three objects, which stay as they are.
// The ABI with the host runtime is belowb_abi.hpp.
#include <hip/hip_runtime.h>

#include "belowb_abi.hpp"

using namespace p1;

// k_below_mark with the target of the tile's request: the workgroup finds its
// piece by binary search on block0 and loads targets[S.req], both uniform
// (scalar loads).  One ballot word per wave, stored by lane 0 with an ordinary
// vector store; every word of the launch's tiles is written by exactly one
// wave, so there is no memset, no atomic and nothing that waits.
extern "C" __global__ __launch_bounds__(kBlock) void k_belowb_mark(const BatchSeg* __restrict__ segs, uint32_t nseg,
                                                                   const uint64_t* __restrict__ targets,
                                                                   uint64_t* __restrict__ marks) {
  const uint32_t b = blockIdx.x;
  const BatchSeg& S = segs[batch_find_seg(segs, nseg, b)];
  // The target waits in a VGPR pair, as k_below_mark's does: the piece's 48
  // uniform words fill the SGPR file.
  uint64_t t = targets[S.req];
  asm volatile("" : "+v"(t));
  const bool hit = below_thread(S.ga, (uint64_t)(b - S.block0) * kBlock + threadIdx.x, t);
  const uint64_t word = __ballot(hit);
  if ((threadIdx.x & 63u) == 0) marks[(uint64_t)b * kBelowWordsPerTile + (threadIdx.x >> 6)] = word;
}

// One workgroup per request: an order-preserving compaction of the request's
// mark words, a chunk of kBlock words at a time, one word per thread.  Per
// chunk: the popcount of the thread's word, an inclusive prefix sum across the
// wave's 64 lanes (__shfl_up), the four wave totals through LDS, and `base`,
// the set bits of all earlier chunks.  `base` is computed by every thread from
// the same LDS values, so it is the same in all of them and the loop's trip
// count is uniform: the barrier inside it is reached by the whole workgroup.
// A thread whose word starts below the request's slot count expands it
// (belowb_expand_word) into the slots from its exclusive prefix on, so the
// indices come out in increasing word and bit order and nothing past the
// request's slots is written.  The loop ends once the slots are full.  No
// atomics, no memset; nothing one workgroup writes is read by another.
//
// The LDS totals are double-buffered: chunk i + 2 rewrites what chunk i read,
// and the barrier of chunk i + 1 lies between the two.
extern "C" __global__ __launch_bounds__(kBlock) void k_belowb_collect(const uint64_t* __restrict__ marks,
                                                                      const uint32_t* __restrict__ req_tile0,
                                                                      const uint32_t* __restrict__ req_hit0,
                                                                      uint32_t* __restrict__ idx,
                                                                      uint32_t* __restrict__ count) {
  constexpr uint32_t kWaves = kBlock / 64;
  __shared__ uint32_t wave_sum[2][kWaves];
  const uint32_t r = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t w0 = req_tile0[r] * kBelowWordsPerTile, w1 = req_tile0[r + 1] * kBelowWordsPerTile;
  const uint32_t s0 = req_hit0[r], slots = req_hit0[r + 1] - s0;
  uint32_t base = 0, buf = 0;
  for (uint32_t c0 = w0; c0 < w1 && base < slots; c0 += kBlock, buf ^= 1u) {
    const uint32_t w = c0 + tid;
    const uint64_t word = w < w1 ? marks[w] : 0;  // the last chunk may be ragged
    const uint32_t c = (uint32_t)__popcll(word);
    uint32_t incl = c;
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[buf][wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t i = 0; i < kWaves; ++i) {
      const uint32_t s = wave_sum[buf][i];
      if (i < wave) before += s;
      total += s;
    }
    const uint32_t excl = base + before + (incl - c);
    if (c != 0 && excl < slots) belowb_expand_word(word, w, slots - excl, idx + s0 + excl);
    base += total;
  }
  if (tid == 0) count[r] = base < slots ? base : slots;
}
