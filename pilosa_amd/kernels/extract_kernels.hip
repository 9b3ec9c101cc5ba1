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
// Work unit, stages 1 and 2 as in K26: one workgroup of four waves owns one
// (arena shard, key, slice); a slice is n of the key's 8 tile slots (8192
// columns each; n is 1, 2, 4 or 8).
//
//   1. Every wave evaluates the filter tile of the key.  consider = the filter
//      alone: a column without a value is still a row of the answer.  An empty
//      slice ends the workgroup here, block-uniformly, before any barrier.
//   2. Staging: exists, the sign row and the planes go round-robin over the
//      waves into the block-shared LDS slab ([tile][slot][lane], 16 bytes per
//      lane; slice_each, bsi_tile.h).  exists is one more tile: it becomes the
//      validity bit.  One __syncthreads().
//   3. Scan: thread tid owns 32-column word tid of each slot.  Wave totals per
//      slot go to LDS (the expansion bitmap of wave 0, free after the barrier);
//      one more __syncthreads(); every thread then knows the output position of
//      its first column.
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
// LDS: four WaveScratch (40 KiB, static) + (3 + depth) * n KiB dynamic
// (consider, exists, sign, planes); the launcher clamps n to what fits 160 KiB.
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

namespace pk {

__global__ __launch_bounds__(256) void bsi_extract_kernel(const QueryProg* __restrict__ progs,
                                                          const ViewDev* __restrict__ views, int S, BsiArgs bsi, int n,
                                                          const int64_t* __restrict__ unit_off,
                                                          const int64_t* __restrict__ col_base, int64_t base,
                                                          int64_t cap, uint64_t* __restrict__ columns,
                                                          int64_t* __restrict__ values, uint8_t* __restrict__ valid) {
  __shared__ WaveScratch scratch[WAVES_PER_BLOCK];
  extern __shared__ dq_u64x2 ex_slab[];  // [3 + depth][n][64]: consider, exists, sign, planes; slots of the slice
  const uint32_t unit = xcd_remap(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const uint32_t nsl = 8u / uint32_t(n);
  const int slot0 = int(unit % nsl) * n;
  const int j = int((unit / nsl) & 15);
  const int s = int(unit / (nsl * 16));
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
      if (wave == 0) ex_slab[(i - slot0) * 64 + lane] = dq_u64x2{f.w[i].x, f.w[i].y};
    }
  }
  if (!__ballot(any != 0)) return;
  const int64_t slice_base = uo + wave_sum(before);

  // ---- 2. staging: tile 1 = exists, 2 = sign, 3 + p = plane p, round-robin over the waves
  const int64_t ce = bsi_find(c, bsi.row_exists);
  const int64_t cs = bsi_find(c, bsi.row_sign);
  plane_index(c);
  const uint64_t present = __ballot(c.planes >= 0) & ((1ull << depth) - 1);  // (depth <= 32)
  for (int t = 1 + wave; t < 3 + depth; t += WAVES_PER_BLOCK) {
    const int64_t ci = t == 1 ? ce : t == 2 ? cs : rl_i64(c.planes, t - 3);
    if (ci < 0) continue;  // absent: never read back
    dq_u64x2* dst = ex_slab + t * n * 64 + lane;
    slice_each(bv.payload, bv.meta[ci], ws.lb, slot0, n,
               [&](int i, ulong2 e) { dst[(i - slot0) * 64] = dq_u64x2{e.x, e.y}; });
  }
  __syncthreads();

  // ---- 3. block scan: wave totals per slot through LDS (wave 0's lb is free now)
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(ex_slab);
  int* part = reinterpret_cast<int*>(scratch[0].lb);  // [n][WAVES_PER_BLOCK]
  const int tid = threadIdx.x;
  for (int k = 0; k < n; k++) {
    const int incl = wave_scan_incl(__popc(s32[k * 256 + tid]));
    if (lane == 63) part[k * WAVES_PER_BLOCK + wave] = incl;
  }
  __syncthreads();

  // ---- 4. transpose and write: thread tid owns 32-column word tid of each slot
  const uint64_t col0 = uint64_t(col_base[s]) + uint64_t(j) * 65536u + uint64_t(tid) * 32u;
  int64_t run = slice_base;  // output position of the slot's first column
  for (int k = 0; k < n; k++) {
    const uint32_t cw = s32[k * 256 + tid];
    const int cnt = __popc(cw);
    int64_t o = run + (wave_scan_incl(cnt) - cnt);
#pragma unroll
    for (int w = 0; w < WAVES_PER_BLOCK; w++) {
      const int p = part[k * WAVES_PER_BLOCK + w];
      if (w < wave) o += p;
      run += p;
    }
    if (cw) {
      const uint32_t ew = ce >= 0 ? s32[(n + k) * 256 + tid] : 0u;
      const uint32_t sw = cs >= 0 ? s32[(2 * n + k) * 256 + tid] : 0u;
      uint32_t a[32];
#pragma unroll
      for (int p = 0; p < 32; p++)
        a[p] = (p < depth && ((present >> p) & 1)) ? s32[((3 + p) * n + k) * 256 + tid] : 0u;
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

int extract_slots(int depth, int want) {
  int n = 8;
  // four WaveScratch + (consider, exists, sign, planes) * n KiB inside the CU's 160 KiB
  while (n > 1 && int64_t(sizeof(WaveScratch)) * WAVES_PER_BLOCK + int64_t(3 + depth) * n * 1024 > 160 * 1024) n >>= 1;
  if (want >= 1 && want < n) {
    int w = 1;
    while (w * 2 <= want) w <<= 1;  // round down to a power of two
    n = w;
  }
  return n;
}

int launch_bsi_extract(const QueryProg* progs, const ViewDev* views, int S, BsiArgs bsi, int slots,
                       const int64_t* unit_off, const int64_t* col_base, int64_t base, int64_t cap, uint64_t* columns,
                       int64_t* values, uint8_t* valid, hipStream_t st) {
  if (bsi.depth < 0 || bsi.depth > EXTRACT_MAX_PLANES || cap < 0) return -1;
  const int n = extract_slots(bsi.depth, slots);
  if (S <= 0 || cap == 0) return n;
  const int64_t blocks = int64_t(S) * 16 * (8 / n);
  if (blocks >= (int64_t(1) << 31)) return -1;
  const int lds = (3 + bsi.depth) * n * 1024;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(bsi_extract_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL(bsi_extract_kernel, dim3(unsigned(blocks)), dim3(64 * WAVES_PER_BLOCK), lds, st, progs, views, S,
                     bsi, n, unit_off, col_base, base, cap, columns, values, valid);
  return n;
}

}  // namespace pk
