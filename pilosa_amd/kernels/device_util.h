// Device-side helpers shared by every kernel file: one definition each of the
// small pieces a new kernel would otherwise copy from its neighbour.  Include
// after kernels.h.  Everything is __device__ __forceinline__, so the header
// needs no anonymous namespace and defines nothing with external linkage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace pk {

__device__ __forceinline__ int wave_lane() { return threadIdx.x & 63; }

__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Wave-wide sums through DPP row ops (ockl), not __shfl_xor: the latter is six
// dependent ds_bpermute round trips through the LDS pipe per call.
extern "C" __device__ int __ockl_wfred_add_i32(int);
extern "C" __device__ long __ockl_wfred_add_i64(long);
__device__ __forceinline__ int wave_sum(int v) { return __ockl_wfred_add_i32(v); }
__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) { return int64_t(__ockl_wfred_add_i64(long(v))); }

// inclusive prefix sum over the wave's 64 lanes (all lanes active)
__device__ __forceinline__ int wave_scan_incl(int v) {
  const int lane = wave_lane();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

// broadcast lane `src` (wave-uniform) with scalar readlanes, no LDS pipe
__device__ __forceinline__ uint64_t rl_u64(uint64_t v, int src) {
  return (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(v >> 32), src))) << 32) |
         uint32_t(__builtin_amdgcn_readlane(int(v), src));
}
__device__ __forceinline__ int64_t rl_i64(int64_t v, int src) { return int64_t(rl_u64(uint64_t(v), src)); }

// Bijective XCD-aware block remap: hardware block ids b, b + 8, b + 16, ...
// (one XCD) get consecutive logical ids, so consecutive logical units -- the
// same shard or (shard, key) under different queries, chunks or rows, i.e. the
// same hot containers, colptr and slot lists -- run on one XCD and share its L2.
__device__ __forceinline__ uint32_t xcd_remap(uint32_t bid, uint32_t nblk) {
  const uint32_t nx = 8;
  const uint32_t xcd = bid % nx, loc = bid / nx;
  const uint32_t q = nblk / nx, r = nblk % nx;
  const uint32_t base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + loc;
}

// Payload/meta pointers live in ViewDev as generic pointers; casting them to
// the global address space gives global_load (vmcnt only) instead of
// flat_load, which also counts against lgkmcnt and so serialises with LDS.
// (The host compilation pass parses these bodies too, without address spaces.)
#if defined(__HIP_DEVICE_COMPILE__)
#define PK_GLOBAL __attribute__((address_space(1)))
#else
#define PK_GLOBAL
#endif
template <class T>
__device__ __forceinline__ const PK_GLOBAL T* gp(const T* p) {
  return (const PK_GLOBAL T*)(p);
}

// first u16 of the container described by meta word m
__device__ __forceinline__ const uint16_t* payload_of(const ViewDev& v, int64_t m) {
  return v.payload + meta_off16(m) * 8;
}

// the k-th of the eight u16 values of one 16-byte payload load
__device__ __forceinline__ uint32_t val8(const uint4& q, int k) {
  const uint32_t w = k < 2 ? q.x : (k < 4 ? q.y : (k < 6 ? q.z : q.w));
  return (w >> ((k & 1) * 16)) & 0xffff;
}

// Two per-thread lookups of a dense row's containers in shard s.  row_keys:
// all keys of the row at once -- the presence mask plus the first container's
// index, from which key j's container is lo + popcount of the lower mask bits;
// d < 0 (empty row) is allowed.  find_container: one key j of a row that
// exists (d >= 0), when nothing else of the row is wanted.

// Key-presence mask and absolute first-container index of dense row d in shard s.
__device__ __forceinline__ uint32_t row_keys(const ViewDev& v, int s, int64_t d, int64_t& lo) {
  lo = 0;
  if (d < 0) return 0;
  const auto rp = gp(v.rowptr + int64_t(s) * (v.D + 1));
  const uint32_t r0 = rp[d];
  lo = gp(v.shard_base)[s] + r0;
  // the view's mask table: one 2-byte load instead of the row's metas
  if (v.keymask) return gp(v.keymask)[int64_t(s) * v.D + d];
  const uint32_t r1 = rp[d + 1];
  const int n = int(r1 - r0);
  if (n == 16) return 0xffffu;
  uint32_t pres = 0;
#pragma unroll
  for (int k = 0; k < 16; k++)
    if (k < n) pres |= 1u << meta_j(gp(v.meta)[lo + k]);
  return pres;
}

// Absolute meta index of dense row d's key-j container in shard s, -1 = none.
__device__ __forceinline__ int64_t find_container(const ViewDev& v, int s, int64_t d, int j) {
  const auto rp = gp(v.rowptr + int64_t(s) * (v.D + 1));
  const uint32_t r0 = rp[d];
  const int64_t lo = gp(v.shard_base)[s] + r0;
  if (v.keymask) {
    const uint32_t pres = gp(v.keymask)[int64_t(s) * v.D + d];
    return ((pres >> j) & 1) ? lo + __popc(pres & ((1u << j) - 1)) : -1;
  }
  const int n = min(int(rp[d + 1] - r0), 16);
  for (int k = 0; k < n; k++) {
    const int jj = meta_j(gp(v.meta)[lo + k]);
    if (jj == j) return lo + k;
    if (jj > j) break;   // a row's containers are sorted by key
  }
  return -1;
}

}  // namespace pk
