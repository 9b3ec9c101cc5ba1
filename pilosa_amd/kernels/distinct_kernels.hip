// CDNA4 (gfx950) kernel K26: Distinct(field=) -- which values occur in a
// bit-sliced (BSI) int field over exists & filter.
//
// Every other BSI kernel (bsi_kernels.hip) treats a bit plane as a set of
// columns and never forms the value of a column.  This one transposes: the
// plane words of 32 columns become 32 per-column magnitudes (bit_transpose.h),
// and each magnitude is marked in one of two device bitmaps of 2^depth bits,
// pos or neg by the column's sign bit.  The host reads back only the non-zero
// words of the two bitmaps.
//
// Work unit, slab layout and stages 1 and 2 are those of bsi_slab.h, shared
// with K27 and K29: one workgroup of four waves owns one (arena shard, key,
// slice of n tile slots).
//
//   1. Every wave resolves the containers of exists, sign and the planes at
//      the key (BsiCtx, bsi_tile.h) and evaluates the slice of consider =
//      exists & filter (slab_consider).  A key without an exists container, or
//      an empty consider slice, ends the workgroup here: every wave computes
//      the same, so both exits are block-uniform, and they come before the
//      barrier.
//   2. Staging (slab_stage): the waves take the sign row and the planes
//      round-robin and store the slice's slots into the slab.  One
//      __syncthreads().
//   3. Transpose: a slot is 256 words of 32 columns, one per thread; a thread
//      skips a word whose consider word is 0, else reads the <= 32 plane words
//      (absent planes are zero), transposes them in registers and marks the
//      magnitude of every considered column.
//
// Marking reads the bitmap word with a plain load and issues the atomic OR only
// when the bit is missing: a low-cardinality field would otherwise send every
// column's atomic to the same few L2 words (the failure kth_block_add's comment
// records for counters).  A stale read costs one redundant OR -- OR is
// idempotent -- so no fence or protocol is needed, and no launch reads what it
// wrote.  MARK selects the variants measured in profiles/distinct/README.md:
// 0 = always OR, 1 = test first (shipped), 2 = test first and skip a value
// equal to the thread's previous one.
//
// Slab: DISTINCT_FIXED_TILES + depth tiles (consider, sign, planes).
//
// Resource usage (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage), see profiles/distinct/resource_usage.txt:
//   MARK 0, 1: 214 VGPRs, 0 AGPRs, 106 SGPRs (63 spilled to VGPR lanes), scratch 0,
//              static LDS 40960 B, occupancy 2 waves/SIMD by registers
//   MARK 2:    215 VGPRs, 0 AGPRs, 106 SGPRs (72 spilled to VGPR lanes), scratch 0,
//              static LDS 40960 B, occupancy 2 waves/SIMD
// The SGPR pressure is BsiArgs passed by value (134 dwords of kernel
// arguments); the spills go to VGPR lanes, not to memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "expr_tile.h"
#include "bsi_tile.h"
#include "bit_transpose.h"
#include "bsi_slab.h"

namespace pk {

template <int MARK>
__device__ __forceinline__ void distinct_mark(uint32_t* __restrict__ bm, uint32_t mag) {
  uint32_t* w = bm + (mag >> 5);
  const uint32_t bit = 1u << (mag & 31);
  if (MARK == 0 || !(*w & bit)) atomicOr(w, bit);
}

template <int MARK>
__global__ __launch_bounds__(256) void bsi_distinct_kernel(const QueryProg* __restrict__ progs,
                                                           const ViewDev* __restrict__ views, int S, BsiArgs bsi,
                                                           int n, uint32_t* __restrict__ pos,
                                                           uint32_t* __restrict__ neg) {
  __shared__ WaveScratch scratch[WAVES_PER_BLOCK];
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const SlabUnit u = slab_unit(n);
  const int s = u.s, j = u.j, slot0 = u.slot0;
  if (s >= S) return;
  const ViewDev& bv = views[bsi.view];
  WaveScratch& ws = scratch[wave];
  BsiCtx c{bsi, bv, s, j, bv.shard_base[s], bv.rowptr + int64_t(s) * (bv.D + 1), ws.lb};
  const int depth = bsi.depth;  // <= 32 (launcher)

  // ---- 1. consider slice, in every wave (block-uniform exits, no barrier yet: see bsi_slab.h)
  const int64_t ce = bsi_find(c, bsi.row_exists);
  if (ce < 0) return;
  if (!slab_consider(progs[0], views, bv, ce, s, j, ws, slot0, n, wave, lane)) return;

  // ---- 2. staging: tile 1 = sign, tile 2 + p = plane p
  const int64_t cs = bsi_find(c, bsi.row_sign);
  plane_index(c);
  const uint64_t present = slab_present(c, depth);
  slab_stage(bv, ws, slot0, n, wave, lane, DISTINCT_FIXED_TILES + depth,
             [&](int t) { return t == 1 ? cs : rl_i64(c.planes, t - 2); });
  __syncthreads();

  // ---- 3. transpose and mark: thread tid owns 32-column word tid of each slot
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(bsi_slab);
  const int tid = threadIdx.x;
  uint32_t prev = 0;  // MARK 2: the thread's last marked (magnitude, sign)
  bool prev_neg = false, have_prev = false;
  for (int k = 0; k < n; k++) {
    const uint32_t cw = s32[k * 256 + tid];
    if (!cw) continue;
    const uint32_t sw = cs >= 0 ? s32[(n + k) * 256 + tid] : 0u;
    uint32_t a[32];
#pragma unroll
    for (int p = 0; p < 32; p++)
      a[p] = (p < depth && ((present >> p) & 1)) ? s32[((DISTINCT_FIXED_TILES + p) * n + k) * 256 + tid] : 0u;
    bit_transpose32(a);
#pragma unroll
    for (int col = 0; col < 32; col++) {
      if (!((cw >> col) & 1)) continue;
      const bool ng = (sw >> col) & 1;
      if (MARK == 2) {
        if (have_prev && a[col] == prev && ng == prev_neg) continue;
        prev = a[col];
        prev_neg = ng;
        have_prev = true;
      }
      distinct_mark<MARK>(ng ? neg : pos, a[col]);
    }
  }
}

// ------------------------------------------------------------ launcher

int launch_bsi_distinct(const QueryProg* progs, const ViewDev* views, int S, BsiArgs bsi, int slots, int mark,
                        uint32_t* pos, uint32_t* neg, hipStream_t st) {
  if (bsi.depth < 0 || bsi.depth > DISTINCT_MAX_PLANES) return -1;
  const int n = distinct_slots(bsi.depth, slots);
  if (S <= 0) return n;
  const int64_t blocks = slab_blocks(S, n);
  if (blocks >= (int64_t(1) << 31)) return -1;
  const int lds = slab_lds_bytes(DISTINCT_FIXED_TILES, bsi.depth, n);
  if (mark == 0) slab_launch(bsi_distinct_kernel<0>, blocks, lds, st, progs, views, S, bsi, n, pos, neg);
  else if (mark == 2) slab_launch(bsi_distinct_kernel<2>, blocks, lds, st, progs, views, S, bsi, n, pos, neg);
  else slab_launch(bsi_distinct_kernel<1>, blocks, lds, st, progs, views, S, bsi, n, pos, neg);
  return n;
}

}  // namespace pk
