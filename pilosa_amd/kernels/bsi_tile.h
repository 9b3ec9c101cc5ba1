// Per-(shard, key) access to the rows of a BSI view as register tiles: the
// container lookups and tile loads shared by the BSI kernels (bsi_kernels.hip),
// the Distinct kernel (distinct_kernels.hip) and the Extract kernel
// (extract_kernels.hip), and the slice-wise staging the latter two share.
// Include after expr_tile.h.
#pragma once
#include "expr_tile.h"

namespace pk {

struct BsiCtx {
  const BsiArgs& bsi;
  const ViewDev& bv;
  int s;
  int j;
  int64_t base;
  const uint32_t* rp;
  uint64_t* lb;
  // lane i < depth (<= 63): container of bit plane i at key j (-1 = absent),
  // resolved once, in parallel, by plane_index().
  int64_t planes = -1;
};

// Every lane resolves one BSI row's container at (s, j): the plane loops then
// broadcast it with readlanes instead of a dependent ballot walk per plane.
__device__ __forceinline__ void plane_index(BsiCtx& c) {
  const int lane = wave_lane();
  const int64_t d = lane < c.bsi.depth ? c.bsi.bit_row[lane] : -1;
  int64_t found = -1;
  if (d >= 0) {
    const int64_t lo = c.base + c.rp[d], hi = c.base + c.rp[d + 1];
    if (hi - lo == 16) {   // every key present (dense planes): no meta walk
      c.planes = lo + c.j;
      return;
    }
    for (int64_t ci = lo; ci < hi; ci++)
      if (meta_j(c.bv.meta[ci]) == c.j) {
        found = ci;
        break;
      }
  }
  c.planes = found;
}

// container index of dense row d at key j in shard s (wave-uniform, -1 absent)
__device__ __forceinline__ int64_t bsi_find(const BsiCtx& c, int64_t d) {
  if (d < 0) return -1;
  const int lane = wave_lane();
  const int64_t lo = c.rp[d], hi = c.rp[d + 1];
  int64_t found = -1;
  if (lane < hi - lo && meta_j(c.bv.meta[c.base + lo + lane]) == c.j) found = c.base + lo + lane;
  const uint64_t b = __ballot(found >= 0);
  if (!b) return -1;
  return rl_i64(found, int(__builtin_ctzll(b)));
}

__device__ __forceinline__ void bsi_row(const BsiCtx& c, int64_t d, Tile& t) {
  const int64_t ci = bsi_find(c, d);
  if (ci < 0) tile_zero(t);
  else tile_load(t, c.bv.payload, c.bv.meta[ci], c.lb);
}

__device__ __forceinline__ void bsi_plane(const BsiCtx& c, int lane_slot, Tile& t) {
  const int64_t ci = rl_i64(c.planes, lane_slot);
  if (ci < 0) tile_zero(t);
  else tile_load(t, c.bv.payload, c.bv.meta[ci], c.lb);
}

__device__ __forceinline__ void bsi_bit(const BsiCtx& c, int i, Tile& t) {
  if (i < 0 || i >= c.bsi.depth) tile_zero(t);
  else bsi_plane(c, i, t);
}

// (a native 16-byte vector, moved as ds_*_b128: see bsi_group_sum_kernel)
typedef uint64_t dq_u64x2 __attribute__((ext_vector_type(2)));

// f(i, word pair) for the slots i in [slot0, slot0 + n) of container m, as the
// calling lane holds them in a Tile.  i is a constant after unrolling.  A
// bitmap container loads only those slots; arrays and runs go through lb.
template <class F>
__device__ __forceinline__ void slice_each(const uint16_t* payload, int64_t m, uint64_t* lb, int slot0, int n,
                                           F&& f) {
  const int lane = wave_lane();
  if (meta_type(m) == CT_BITMAP) {
    const ulong2* p = reinterpret_cast<const ulong2*>(payload + meta_off16(m) * 8);
#pragma unroll
    for (int i = 0; i < 8; i++)
      if (i >= slot0 && i < slot0 + n) f(i, p[i * 64 + lane]);
  } else {
    lds_expand(lb, payload, m);
    const ulong2* l2 = reinterpret_cast<const ulong2*>(lb);
#pragma unroll
    for (int i = 0; i < 8; i++)
      if (i >= slot0 && i < slot0 + n) f(i, l2[i * 64 + lane]);
    lds_fence();
  }
}

}  // namespace pk
