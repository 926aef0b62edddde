// p1hip_batch_kernels.hip -- the second gfx950 code object of libp1hip.so:
// the kernels of p1hip_scan_batch (many small requests in one launch pair)
// and the per-request fold of p1hip_scan_batch_wide (k_wide_reduce).
//
// Only the generic per-thread path (scan_core.hpp generic_thread), so it
// compiles in seconds and needs no tools/isa_post.py pass; it is built
// device-only, linked into build/p1hip_batch.hsaco and embedded by
// p1hip_batch_blob.S after the scan object.  The ABI with the host runtime is
// batch_abi.hpp.
#include <hip/hip_runtime.h>

#include "batch_abi.hpp"

using namespace p1;

#include "argmin_dev.hpp"

// ----------------------------------------------------------------------------
// Kernels
// ----------------------------------------------------------------------------
// One tile per workgroup: the grid IS the tiles (no work queue: these launches
// are short, and the per-XCD clock skew the queue of k_scan absorbs does not
// matter to them).  The workgroup finds its piece by binary search on block0
// (uniform: scalar loads), runs one nonce per thread and writes one partial.
// Threads past the piece's last nonce contribute the identity key.
extern "C" __global__ __launch_bounds__(kBlock) void k_batch_scan(const BatchSeg* __restrict__ segs, uint32_t nseg,
                                                                  Key* __restrict__ part) {
  const uint32_t b = blockIdx.x;
  const BatchSeg& S = segs[batch_find_seg(segs, nseg, b)];
  const Key k = generic_thread(S.ga, (uint64_t)(b - S.block0) * kBlock + threadIdx.x);
  block_min_store<kBlock>(k, part + b);
}

// One workgroup per request: folds the request's partials, which the kernel
// boundary on the stream has made visible (no fence, no atomics).  A request
// of at most kBatchMaxNonces nonces has at most kSmallMaxBlocks = 262 tiles:
// two loads per thread at the most.
extern "C" __global__ __launch_bounds__(kBlock) void k_batch_reduce(const Key* __restrict__ part,
                                                                    const uint32_t* __restrict__ req_tile0,
                                                                    Key* __restrict__ out) {
  const uint32_t r = blockIdx.x;
  const uint32_t t1 = req_tile0[r + 1];
  Key m = {~0ull, ~0ull};
  for (uint32_t i = req_tile0[r] + threadIdx.x; i < t1; i += kBlock) m = key_min(m, part[i]);
  block_min_store<kBlock>(m, out + r);
}

// p1hip_scan_batch_wide: one workgroup per request folds the request's
// ranges of the device's partial array (batch_abi.hpp WideRange: one range
// per k_scan segment of the request, one for its generic tiles).  The range
// table is indexed by the workgroup's request, so its loads are wave-uniform;
// the partials were written by earlier kernels on the stream (no fence, no
// atomics).  A range of a 2^24-nonce request has at most 6554 tiles.
extern "C" __global__ __launch_bounds__(kBlock) void k_wide_reduce(const Key* __restrict__ part,
                                                                   const WideRange* __restrict__ ranges,
                                                                   const uint32_t* __restrict__ req_range0,
                                                                   Key* __restrict__ out) {
  const uint32_t r = blockIdx.x;
  const uint32_t j1 = req_range0[r + 1];
  Key m = {~0ull, ~0ull};
  for (uint32_t j = req_range0[r]; j < j1; ++j) {
    const uint32_t t0 = ranges[j].tile0, nt = ranges[j].ntiles;
    for (uint32_t i = threadIdx.x; i < nt; i += kBlock) m = key_min(m, part[t0 + i]);
  }
  block_min_store<kBlock>(m, out + r);
}
