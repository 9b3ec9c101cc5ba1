// CDNA4 (gfx950) kernel K27: Extract(filter, Rows(field=)) for a bit-sliced
// (BSI) int field -- the value of every column of the filter, in column order.
//
// bsi_distinct_kernel (K26) forms the value of a column and then forgets which
// column held it.  This kernel keeps it: the output is three parallel vectors,
// columns[o] / values[o] / valid[o], compacted (one entry per column of the
// filter) and ascending by column.  Compaction needs the position of every
// column, and that is a prefix sum over the whole index.  It is split so that
// no workgroup waits for another:
//
//   * across (shard, key) units: an expr_count launch of the filter program has
//     left the count of every unit, the host's cumsum turned them into
//     exclusive offsets unit_off[s * 16 + j]; the launch boundary is the only
//     global ordering.  An offset of -1 marks a unit that is empty or lies
//     entirely beyond the request's window (offset + limit): its workgroups
//     leave at once.
//   * inside a unit, before the slice: every wave holds the whole filter tile
//     of the key anyway, so the slice's base is the popcount of the tile's
//     earlier slots (one wave reduction, no load).
//   * inside the slice: a block-wide exclusive scan of the 256 threads' word
//     popcounts per slot -- a wave scan plus four wave totals through LDS.
//
// Work unit, slab layout, staging and the block scan are those of bsi_slab.h,
// shared with K26 and K29: one workgroup of four waves owns one (arena shard,
// key, slice of n tile slots).
//
//   1. Every wave evaluates the filter tile of the key.  consider = the filter
//      alone: a column without a value is still a row of the answer, so tile 0
//      is written here and not by slab_consider, which also would not count
//      the columns before the slice.  An empty slice ends the workgroup here,
//      block-uniformly, before any barrier.
//   2. Staging (slab_stage): exists, the sign row and the planes go round-robin
//      over the waves into the slab.  exists is one more tile: it becomes the
//      validity bit.  One __syncthreads().
//   3. Scan (slab_scan_totals): thread tid owns 32-column word tid of each
//      slot.  Wave totals per slot go to LDS (the expansion bitmap of wave 0,
//      free after the barrier); one more __syncthreads(); every thread then
//      knows the output position of its first column (slab_scan_pos).
//   4. Transpose and write: a thread skips a zero consider word, else reads the
//      <= 32 plane words, transposes them in registers (bit_transpose.h) and,
//      for every set bit in ascending order, stores the global column id, the
//      value (sign ? -mag : mag) + base (0 where exists is clear) and the
//      validity byte at its position.  Plain vector stores at unique indices:
//      no atomics, no grid-wide barrier, no spin, no cooperative launch.  Every
//      store is bounds-checked against the buffers' length, so data that
//      changed between the count pass and this one cannot write outside them.
//
// Several int fields of one request share unit_off and the column vector; only
// the launch that is given a columns pointer writes it.
//
// Slab: EXTRACT_FIXED_TILES + depth tiles (consider, exists, sign, planes).
//
// Resource usage (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage), see profiles/extract/resource_usage.txt:
//   216 VGPRs, 0 AGPRs, 106 SGPRs (104 spilled to VGPR lanes), scratch 0,
//   static LDS 40960 B, occupancy 2 waves/SIMD by registers
// The SGPR pressure is BsiArgs passed by value (134 dwords of kernel
// arguments); the spills go to VGPR lanes, not to memory: ScratchSize is 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "expr_tile.h"
#include "bsi_tile.h"
#include "bit_transpose.h"
#include "bsi_slab.h"

namespace pk {

__global__ __launch_bounds__(256) void bsi_extract_kernel(const QueryProg* __restrict__ progs,
                                                          const ViewDev* __restrict__ views, int S, BsiArgs bsi, int n,
                                                          const int64_t* __restrict__ unit_off,
                                                          const int64_t* __restrict__ col_base, int64_t base,
                                                          int64_t cap, uint64_t* __restrict__ columns,
                                                          int64_t* __restrict__ values, uint8_t* __restrict__ valid) {
  __shared__ WaveScratch scratch[WAVES_PER_BLOCK];
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const SlabUnit u = slab_unit(n);
  const int s = u.s, j = u.j, slot0 = u.slot0;
  if (s >= S) return;
  const int64_t uo = unit_off[int64_t(s) * 16 + j];
  if (uo < 0) return;  // empty, or beyond the window (block-uniform)
  const ViewDev& bv = views[bsi.view];
  WaveScratch& ws = scratch[wave];
  BsiCtx c{bsi, bv, s, j, bv.shard_base[s], bv.rowptr + int64_t(s) * (bv.D + 1), ws.lb};
  const int depth = bsi.depth;  // <= 32 (launcher)

  // ---- 1. the filter tile, in every wave (block-uniform exits, no barrier yet)
  const QueryProg& qp = progs[0];
  if (!qp.nprog) return;
  uint32_t mask[MAXLEAF];
  build_slots(qp, views, s, ws, mask);
  if (!((candidate_mask(qp, mask) >> j) & 1)) return;
  Tile f;
  eval_tile(qp, views, s, j, ws, f);
  uint64_t any = 0;
  int before = 0;  // the filter's columns in the key's slots below the slice (this lane's words)
#pragma unroll
  for (int i = 0; i < 8; i++) {
    if (i < slot0) before += __popcll(f.w[i].x) + __popcll(f.w[i].y);
    if (i >= slot0 && i < slot0 + n) {
      any |= f.w[i].x | f.w[i].y;
      if (wave == 0) bsi_slab[(i - slot0) * 64 + lane] = dq_u64x2{f.w[i].x, f.w[i].y};
    }
  }
  if (!__ballot(any != 0)) return;
  const int64_t slice_base = uo + wave_sum(before);

  // ---- 2. staging: tile 1 = exists, 2 = sign, 3 + p = plane p
  const int64_t ce = bsi_find(c, bsi.row_exists);
  const int64_t cs = bsi_find(c, bsi.row_sign);
  plane_index(c);
  const uint64_t present = slab_present(c, depth);
  slab_stage(bv, ws, slot0, n, wave, lane, EXTRACT_FIXED_TILES + depth,
             [&](int t) { return t == 1 ? ce : t == 2 ? cs : rl_i64(c.planes, t - 3); });
  __syncthreads();

  // ---- 3. block scan: wave totals per slot through LDS (wave 0's lb is free now)
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(bsi_slab);
  int* part = reinterpret_cast<int*>(scratch[0].lb);  // [n][WAVES_PER_BLOCK]
  const int tid = threadIdx.x;
  for (int k = 0; k < n; k++) slab_scan_totals(part, k, wave, lane, __popc(s32[k * 256 + tid]));
  __syncthreads();

  // ---- 4. transpose and write: thread tid owns 32-column word tid of each slot
  const uint64_t col0 = uint64_t(col_base[s]) + uint64_t(j) * 65536u + uint64_t(tid) * 32u;
  int64_t run = slice_base;  // output position of the slot's first column
  for (int k = 0; k < n; k++) {
    const uint32_t cw = s32[k * 256 + tid];
    int64_t o = slab_scan_pos(part, k, wave, __popc(cw), run);
    if (cw) {
      const uint32_t ew = ce >= 0 ? s32[(n + k) * 256 + tid] : 0u;
      const uint32_t sw = cs >= 0 ? s32[(2 * n + k) * 256 + tid] : 0u;
      uint32_t a[32];
#pragma unroll
      for (int p = 0; p < 32; p++)
        a[p] = (p < depth && ((present >> p) & 1)) ? s32[((EXTRACT_FIXED_TILES + p) * n + k) * 256 + tid] : 0u;
      bit_transpose32(a);
      const uint64_t colk = col0 + uint64_t(slot0 + k) * 8192u;
#pragma unroll
      for (int col = 0; col < 32; col++) {
        if (!((cw >> col) & 1)) continue;
        if (o >= 0 && o < cap) {
          const bool ok = (ew >> col) & 1;
          const int64_t mag = int64_t(a[col]);
          if (columns) columns[o] = colk + uint64_t(col);
          values[o] = ok ? (((sw >> col) & 1) ? -mag : mag) + base : 0;
          valid[o] = ok ? 1 : 0;
        }
        o++;
      }
    }
  }
}

// ------------------------------------------------------------ launcher

int launch_bsi_extract(const QueryProg* progs, const ViewDev* views, int S, BsiArgs bsi, int slots,
                       const int64_t* unit_off, const int64_t* col_base, int64_t base, int64_t cap, uint64_t* columns,
                       int64_t* values, uint8_t* valid, hipStream_t st) {
  if (bsi.depth < 0 || bsi.depth > EXTRACT_MAX_PLANES || cap < 0) return -1;
  const int n = extract_slots(bsi.depth, slots);
  if (S <= 0 || cap == 0) return n;
  const int64_t blocks = slab_blocks(S, n);
  if (blocks >= (int64_t(1) << 31)) return -1;
  slab_launch(bsi_extract_kernel, blocks, slab_lds_bytes(EXTRACT_FIXED_TILES, bsi.depth, n), st, progs, views, S, bsi, n,
              unit_off, col_base, base, cap, columns, values, valid);
  return n;
}

}  // namespace pk
