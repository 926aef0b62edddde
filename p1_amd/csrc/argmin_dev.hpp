// argmin_dev.hpp -- the wave / workgroup argmin both device code objects end
// their kernels with (p1hip_kernels.hip, p1hip_batch_kernels.hip).  Device
// only; included after `using namespace p1;` (Key, key_lt: scan_core.hpp).
#pragma once

// ----------------------------------------------------------------------------
// Wave / workgroup argmin over Key = (hash, nonce), lexicographic.
// ----------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}

template <int CTRL>
__device__ __forceinline__ Key key_dpp(const Key& k) {
  Key o;
  o.h = ((uint64_t)dpp<CTRL>((uint32_t)(k.h >> 32)) << 32) | dpp<CTRL>((uint32_t)k.h);
  o.n = ((uint64_t)dpp<CTRL>((uint32_t)(k.n >> 32)) << 32) | dpp<CTRL>((uint32_t)k.n);
  return o;
}

__device__ __forceinline__ uint32_t swz_xor16(uint32_t v) {
  // ds_swizzle bit-mask mode: and 0x1f, or 0, xor 0x10 (within 32 lanes)
  return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);
}

__device__ __forceinline__ Key key_min(const Key& a, const Key& b) { return key_lt(b, a) ? b : a; }

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}

// All 64 lanes must be active.  Returns the wave minimum (wave-uniform).
__device__ __forceinline__ Key wave_min(Key k) {
  k = key_min(k, key_dpp<0xB1>(k));   // quad_perm [1,0,3,2]  (xor 1)
  k = key_min(k, key_dpp<0x4E>(k));   // quad_perm [2,3,0,1]  (xor 2)
  k = key_min(k, key_dpp<0x124>(k));  // row_ror:4
  k = key_min(k, key_dpp<0x128>(k));  // row_ror:8  -> every lane holds its row min
  Key o;
  o.h = ((uint64_t)swz_xor16((uint32_t)(k.h >> 32)) << 32) | swz_xor16((uint32_t)k.h);
  o.n = ((uint64_t)swz_xor16((uint32_t)(k.n >> 32)) << 32) | swz_xor16((uint32_t)k.n);
  k = key_min(k, o);                  // halves of 32 lanes
  Key a, b;
  a.h = readlane64(k.h, 0);  a.n = readlane64(k.n, 0);
  b.h = readlane64(k.h, 32); b.n = readlane64(k.n, 32);
  return key_min(a, b);
}

template <int NT>
__device__ __forceinline__ void block_min_store(Key k, Key* out) {
  __shared__ Key sk[NT / 64];
  k = wave_min(k);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) sk[wid] = k;
  __syncthreads();
  if (threadIdx.x == 0) {
    Key b = sk[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) b = key_min(b, sk[w]);
    *out = b;
  }
}
