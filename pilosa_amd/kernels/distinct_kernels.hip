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
// Work unit: one workgroup of four waves owns one (arena shard, key, slice);
// a slice is n of the 8 tile slots of the key (slot i of a Tile is the
// contiguous column range [8192 i, 8192 (i + 1)), so n is 1, 2, 4 or 8).
//
//   1. Every wave resolves the containers of exists, sign and the planes at
//      the key (BsiCtx, bsi_tile.h) and evaluates the slice of consider =
//      exists & filter (eval_tile, as bsi_kth_init_kernel does).  A key
//      without an exists container, or an empty consider slice, ends the
//      workgroup here: every wave computes the same, so both exits are
//      block-uniform, and they come before the barrier.
//   2. Staging: the waves take the sign row and the planes round-robin and
//      store the slice's slots into a block-shared LDS slab, in the per-lane
//      16-byte layout of bsi_group_sum_kernel ([tile][slot][lane]).  Array and
//      run containers are expanded once through the wave's lb; a bitmap
//      container loads only the slice's slots.  One __syncthreads().
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
// LDS: four WaveScratch (40 KiB, static) + (2 + depth) * n KiB dynamic
// (consider, sign, planes); the launcher clamps n to what fits in 160 KiB.
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
  extern __shared__ dq_u64x2 dq_slab[];  // [2 + depth][n][64]: consider, sign, planes; slots of the slice
  const uint32_t unit = xcd_remap(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const uint32_t nsl = 8u / uint32_t(n);
  const int slot0 = int(unit % nsl) * n;
  const int j = int((unit / nsl) & 15);
  const int s = int(unit / (nsl * 16));
  if (s >= S) return;
  const ViewDev& bv = views[bsi.view];
  WaveScratch& ws = scratch[wave];
  BsiCtx c{bsi, bv, s, j, bv.shard_base[s], bv.rowptr + int64_t(s) * (bv.D + 1), ws.lb};
  const int depth = bsi.depth;  // <= 32 (launcher)

  // ---- 1. consider slice, in every wave (block-uniform exits, no barrier yet)
  const int64_t ce = bsi_find(c, bsi.row_exists);
  if (ce < 0) return;
  const QueryProg& qp = progs[0];
  uint64_t any = 0;
  if (qp.nprog) {
    uint32_t mask[MAXLEAF];
    build_slots(qp, views, s, ws, mask);
    if (!((candidate_mask(qp, mask) >> j) & 1)) return;
    Tile f;
    eval_tile(qp, views, s, j, ws, f);
    slice_each(bv.payload, bv.meta[ce], ws.lb, slot0, n, [&](int i, ulong2 e) {
      const dq_u64x2 v{e.x & f.w[i].x, e.y & f.w[i].y};
      any |= v.x | v.y;
      if (wave == 0) dq_slab[(i - slot0) * 64 + lane] = v;
    });
  } else {
    slice_each(bv.payload, bv.meta[ce], ws.lb, slot0, n, [&](int i, ulong2 e) {
      any |= e.x | e.y;
      if (wave == 0) dq_slab[(i - slot0) * 64 + lane] = dq_u64x2{e.x, e.y};
    });
  }
  if (!__ballot(any != 0)) return;

  // ---- 2. staging: tile 1 = sign, tile 2 + p = plane p, round-robin over the waves
  const int64_t cs = bsi_find(c, bsi.row_sign);
  plane_index(c);
  const uint64_t present = __ballot(c.planes >= 0) & ((1ull << depth) - 1);  // (depth <= 32)
  for (int t = 1 + wave; t < 2 + depth; t += WAVES_PER_BLOCK) {
    const int64_t ci = t == 1 ? cs : rl_i64(c.planes, t - 2);
    if (ci < 0) continue;  // absent: never read back
    dq_u64x2* dst = dq_slab + t * n * 64 + lane;
    slice_each(bv.payload, bv.meta[ci], ws.lb, slot0, n,
               [&](int i, ulong2 e) { dst[(i - slot0) * 64] = dq_u64x2{e.x, e.y}; });
  }
  __syncthreads();

  // ---- 3. transpose and mark: thread tid owns 32-column word tid of each slot
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(dq_slab);
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
      a[p] = (p < depth && ((present >> p) & 1)) ? s32[((2 + p) * n + k) * 256 + tid] : 0u;
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

int distinct_slots(int depth, int want) {
  int n = 8;
  // four WaveScratch + (consider, sign, planes) * n KiB inside the CU's 160 KiB
  while (n > 1 && int64_t(sizeof(WaveScratch)) * WAVES_PER_BLOCK + int64_t(2 + depth) * n * 1024 > 160 * 1024) n >>= 1;
  if (want >= 1 && want < n) {
    int w = 1;
    while (w * 2 <= want) w <<= 1;  // round down to a power of two
    n = w;
  }
  return n;
}

int launch_bsi_distinct(const QueryProg* progs, const ViewDev* views, int S, BsiArgs bsi, int slots, int mark,
                        uint32_t* pos, uint32_t* neg, hipStream_t st) {
  if (bsi.depth < 0 || bsi.depth > DISTINCT_MAX_PLANES) return -1;
  const int n = distinct_slots(bsi.depth, slots);
  if (S <= 0) return n;
  const int64_t blocks = int64_t(S) * 16 * (8 / n);
  if (blocks >= (int64_t(1) << 31)) return -1;
  const int lds = (2 + bsi.depth) * n * 1024;
  const dim3 grid{unsigned(blocks)}, block(64 * WAVES_PER_BLOCK);
#define PK_DISTINCT(M)                                                                                   \
  {                                                                                                      \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(bsi_distinct_kernel<M>),                     \
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);                          \
    hipLaunchKernelGGL(bsi_distinct_kernel<M>, grid, block, lds, st, progs, views, S, bsi, n, pos, neg); \
  }
  if (mark == 0) PK_DISTINCT(0)
  else if (mark == 2) PK_DISTINCT(2)
  else PK_DISTINCT(1)
#undef PK_DISTINCT
  return n;
}

}  // namespace pk
