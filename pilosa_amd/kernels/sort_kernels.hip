// CDNA4 (gfx950) kernel K29: Sort(<filter>, field=, limit=, offset=, sort-desc=)
// for a bit-sliced (BSI) int field -- the selection pass: the (column, value)
// pairs of the k = offset + limit smallest (or largest) values of exists &
// filter over all local shards, in column order.  The k selected entries are
// then put in answer order by one stable sort on the device (GpuEngine.bsi_sort).
//
// The global rank descent (bsi_kth_*, bsi_kernels.hip) has left a threshold T,
// the k-th value in the requested direction.  The selected set is every column
// whose value sorts strictly before T plus the first m columns, in column order
// over all shards, whose value is T (m = k - |before|): ties go by column id.
// That needs two prefix sums over the whole index, and they are split as in
// K27 so that no workgroup waits for another:
//
//   mode 1 (count): every workgroup writes how many of its columns are before T
//     and how many equal T, one int32 pair at its unit index.  Workgroup (unit)
//     order is column order; xcd_remap permutes only which block runs which
//     unit.  The caller's cumsums turn the pairs into before_off[w] and
//     eq_before[w], and the total of `before` into m (all on the device).
//   mode 2 (fill): same grid, same n, same staging and comparator.  A
//     workgroup's output base is before_off[w] + min(eq_before[w], m); a
//     thread's selected word is before | (the first q set bits of equal), q the
//     tie quota left at that word; positions inside the workgroup come from two
//     block scans per slot (equal, then selected): a wave scan plus four wave
//     totals through LDS.  The launch boundary is the only global ordering: no
//     atomics on the output, no grid-wide barrier, no spin, no cooperative
//     launch.
//
// Work unit, slab layout, stages 1 and 2 and the block scans are those of
// bsi_slab.h, shared with K26 and K27: one workgroup of four waves owns one
// (arena shard, key, slice of n tile slots).
//
//   1. Every wave evaluates the slice of consider = exists & filter
//      (slab_consider).  A key without an exists container, or an empty slice,
//      ends the workgroup here, block-uniformly, before any barrier (its count
//      pair stays 0).
//   2. Staging (slab_stage): the sign row and the planes go round-robin over
//      the waves into the slab.  One __syncthreads().
//   3. Compare: thread tid owns 32-column word tid of each slot and runs the
//      bit-sliced comparator (sort_select.h) MSB first over the staged plane
//      words: a `before` word and an `equal` word, no transpose.  select_all
//      (k >= N, or no limit): before = consider, equal = 0, T is not read.
//   4. mode 1: block sum of the two popcounts, one plain store of the pair.
//      mode 2: the scans above; only a thread whose selected word is non-zero
//      reads the <= 32 plane words again and transposes them in registers
//      (bit_transpose.h); for every selected bit in ascending order it stores
//      the global column id and the real value (sign ? -mag : mag) + base at
//      its position.  Plain vector stores at unique indices, each
//      bounds-checked against the buffers' length, so data that changed between
//      the two launches cannot write outside them; the caller initialises the
//      column vector to -1, so a slot the fill did not reach is recognisable.
//
// Slab: SORT_FIXED_TILES + depth tiles (consider, sign, planes).
//
// Resource usage (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage), see profiles/sort/resource_usage.txt:
//   215 VGPRs, 0 AGPRs, 106 SGPRs (88 spilled to VGPR lanes), scratch 0,
//   static LDS 40960 B, occupancy 2 waves/SIMD by registers
// As for K27 the SGPR pressure is BsiArgs passed by value; the spills go to
// VGPR lanes, not to memory: ScratchSize is 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "expr_tile.h"
#include "bsi_tile.h"
#include "bit_transpose.h"
#include "bsi_slab.h"
#include "sort_select.h"

namespace pk {

__global__ __launch_bounds__(256) void bsi_sort_select_kernel(
    const QueryProg* __restrict__ progs, const ViewDev* __restrict__ views, int S, BsiArgs bsi, int n, int mode,
    int select_all, int desc, int t_neg, uint32_t t_mag, int32_t* __restrict__ counts,
    const int64_t* __restrict__ before_off, const int64_t* __restrict__ eq_before, const int64_t* __restrict__ m_ptr,
    const int64_t* __restrict__ col_base, int64_t base, int64_t cap, int64_t* __restrict__ columns,
    int64_t* __restrict__ values) {
  __shared__ WaveScratch scratch[WAVES_PER_BLOCK];
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const SlabUnit u = slab_unit(n);
  const uint32_t unit = u.unit;
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
  slab_stage(bv, ws, slot0, n, wave, lane, SORT_FIXED_TILES + depth,
             [&](int t) { return t == 1 ? cs : rl_i64(c.planes, t - 2); });
  __syncthreads();

  // ---- 3. compare: thread tid owns 32-column word tid of each slot
  uint32_t* s32 = reinterpret_cast<uint32_t*>(bsi_slab);
  int* part = reinterpret_cast<int*>(scratch[0].lb);  // wave totals (wave 0's lb is free after the barrier)
  const int tid = threadIdx.x;
  auto compare = [&](int k, uint32_t cw) -> SortWords {
    if (select_all) return SortWords{cw, 0u};
    const uint32_t sw = cs >= 0 ? s32[(n + k) * 256 + tid] : 0u;
    const SortWords r = sort_compare32(
        [&](int p) { return ((present >> p) & 1) ? s32[((2 + p) * n + k) * 256 + tid] : 0u; }, depth, sw,
        t_neg != 0, t_mag, desc != 0);
    return SortWords{r.before & cw, r.equal & cw};
  };

  if (mode == 1) {
    // ---- 4a. count: the workgroup's (before, equal) pair, one plain store each
    int nb = 0, ne = 0;
    for (int k = 0; k < n; k++) {
      const uint32_t cw = s32[k * 256 + tid];
      if (!cw) continue;
      const SortWords r = compare(k, cw);
      nb += __popc(r.before);
      ne += __popc(r.equal);
    }
    nb = wave_sum(nb);
    ne = wave_sum(ne);
    if (lane == 0) {
      part[wave * 2] = nb;
      part[wave * 2 + 1] = ne;
    }
    __syncthreads();
    if (tid == 0) {
      int tb = 0, te = 0;
#pragma unroll
      for (int w = 0; w < WAVES_PER_BLOCK; w++) {
        tb += part[w * 2];
        te += part[w * 2 + 1];
      }
      counts[int64_t(unit) * 2] = tb;
      counts[int64_t(unit) * 2 + 1] = te;
    }
    return;
  }

  // ---- 4b. fill.  Pass A: the equal words' wave totals per slot; the before word replaces the consider word
  // in the slab (each thread owns its words: no other thread reads them), the equal word goes to eqs
  int* part_eq = part;                             // [n][WAVES_PER_BLOCK]
  int* part_sel = part + 8 * WAVES_PER_BLOCK;      // [n][WAVES_PER_BLOCK]
  uint32_t* eqs = reinterpret_cast<uint32_t*>(scratch[1].lb);  // [n][256] equal words (8 KiB: wave 1's lb, free too)
  for (int k = 0; k < n; k++) {
    const uint32_t cw = s32[k * 256 + tid];
    SortWords r{0u, 0u};
    if (cw) r = compare(k, cw);
    eqs[k * 256 + tid] = r.equal;
    s32[k * 256 + tid] = r.before;
    slab_scan_totals(part_eq, k, wave, lane, __popc(r.equal));
  }
  __syncthreads();

  // Pass B: the tie quota at every word -> the selected word (kept in the slab) and its wave totals
  const int64_t m = m_ptr[0];
  const int64_t eqb = eq_before[unit];
  int64_t eq_run = eqb;  // equal columns before the slot, over all shards
  for (int k = 0; k < n; k++) {
    const uint32_t ew = eqs[k * 256 + tid];
    const int ec = __popc(ew);
    const int64_t prior = slab_scan_pos(part_eq, k, wave, ec, eq_run);
    const int64_t left = m - prior;
    const int q = left <= 0 ? 0 : left >= ec ? ec : int(left);
    const uint32_t sel = s32[k * 256 + tid] | (q == ec ? ew : first_set_bits32(ew, q));
    s32[k * 256 + tid] = sel;
    slab_scan_totals(part_sel, k, wave, lane, __popc(sel));
  }
  __syncthreads();

  // Pass C: transpose and write
  const uint64_t col0 = uint64_t(col_base[s]) + uint64_t(j) * 65536u + uint64_t(tid) * 32u;
  int64_t run = before_off[unit] + (eqb < m ? eqb : (m > 0 ? m : 0));  // output position of the slot's first column
  for (int k = 0; k < n; k++) {
    const uint32_t sel = s32[k * 256 + tid];
    int64_t o = slab_scan_pos(part_sel, k, wave, __popc(sel), run);
    if (sel) {
      const uint32_t sw = cs >= 0 ? s32[(n + k) * 256 + tid] : 0u;
      uint32_t a[32];
#pragma unroll
      for (int p = 0; p < 32; p++)
        a[p] = (p < depth && ((present >> p) & 1)) ? s32[((SORT_FIXED_TILES + p) * n + k) * 256 + tid] : 0u;
      bit_transpose32(a);
      const uint64_t colk = col0 + uint64_t(slot0 + k) * 8192u;
#pragma unroll
      for (int col = 0; col < 32; col++) {
        if (!((sel >> col) & 1)) continue;
        if (o >= 0 && o < cap) {
          const int64_t mag = int64_t(a[col]);
          columns[o] = int64_t(colk + uint64_t(col));
          values[o] = (((sw >> col) & 1) ? -mag : mag) + base;
        }
        o++;
      }
    }
  }
}

// ------------------------------------------------------------ launcher

int launch_bsi_sort_select(int mode, const QueryProg* progs, const ViewDev* views, int S, BsiArgs bsi, int slots,
                           int select_all, int desc, int64_t T, int32_t* counts, const int64_t* before_off,
                           const int64_t* eq_before, const int64_t* m, const int64_t* col_base, int64_t base,
                           int64_t cap, int64_t* columns, int64_t* values, hipStream_t st) {
  if (bsi.depth < 0 || bsi.depth > SORT_MAX_PLANES || cap < 0 || (mode != 1 && mode != 2)) return -1;
  const uint64_t mag = T < 0 ? uint64_t(-T) : uint64_t(T);
  if (!select_all && (mag >> 32)) return -1;
  const int n = sort_slots(bsi.depth, slots);
  if (S <= 0 || (mode == 2 && cap == 0)) return n;
  const int64_t blocks = sort_blocks(S, n);
  if (blocks >= (int64_t(1) << 30)) return -1;
  slab_launch(bsi_sort_select_kernel, blocks, slab_lds_bytes(SORT_FIXED_TILES, bsi.depth, n), st, progs, views, S, bsi,
              n, mode, select_all, desc, int(T < 0), uint32_t(mag), counts, before_off, eq_before, m, col_base, base, cap,
              columns, values);
  return n;
}

}  // namespace pk
