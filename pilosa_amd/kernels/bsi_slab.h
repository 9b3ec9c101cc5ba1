// The slab scaffolding shared by the kernels that form per-column values of a
// BSI field: Distinct (distinct_kernels.hip, K26), Extract
// (extract_kernels.hip, K27) and Sort (sort_kernels.hip, K29).  Include after
// bsi_tile.h and bit_transpose.h.
//
// One workgroup of four waves owns one (arena shard, key, slice); a slice is n
// of the key's 8 tile slots (slot i of a Tile is the contiguous column range
// [8192 i, 8192 (i + 1)), so n is 1, 2, 4 or 8).  The slice's rows are staged
// into a block-shared LDS slab of `tiles` tiles, [tile][slot][lane] with 16
// bytes per lane (the layout of bsi_group_sum_kernel): tile 0 is the consider
// slice, then the kernel's fixed rows (sign; Extract: exists, sign), then one
// tile per bit plane.  After one __syncthreads() thread tid owns the 32-column
// word tid of every slot: 32-bit word (t * n + k) * 256 + tid of tile t, slot k.
//
// Every return before that barrier must be block-uniform: a wave that skips a
// barrier the others reach hangs the workgroup.  s >= S, an absent exists
// container, the candidate mask and the __ballot(any) exit depend only on
// (s, j, slot0) and on memory every wave reads alike, so they are.  The helpers
// never return from the kernel themselves: slab_consider() hands back a bool
// that the kernel acts on.
//
// LDS: four WaveScratch (40 KiB, static) + tiles * n KiB dynamic;
// slab_slots() (kernels.h) clamps n to what fits in the CU's 160 KiB.
#pragma once
#include "bsi_tile.h"
#include "bit_transpose.h"

namespace pk {

static_assert(sizeof(WaveScratch) * WAVES_PER_BLOCK == SLAB_STATIC_LDS, "slab_slots() assumes four WaveScratch");

// The workgroup's slab, [tiles][n][64]: all of its dynamic LDS.  The helpers
// address it by name, not through a pointer argument: with a pointer the
// compiler forms the lane-relative index of every slot in vector registers (32
// s_sub_i32 become v_subrev_u32 + v_mov_b32 per kernel).
extern __shared__ dq_u64x2 bsi_slab[];

// the workgroup's (arena shard, key, first slot of the slice); unit = its index in column order
struct SlabUnit {
  uint32_t unit;
  int s, j, slot0;
};

__device__ __forceinline__ SlabUnit slab_unit(int n) {
  const uint32_t unit = xcd_remap(blockIdx.x, gridDim.x);
  const uint32_t nsl = 8u / uint32_t(n);
  const int slot0 = int(unit % nsl) * n;
  const int j = int((unit / nsl) & 15);
  const int s = int(unit / (nsl * 16));
  return SlabUnit{unit, s, j, slot0};
}

// Tile 0 = the slice of consider = exists (container ce) & filter (qp; nprog ==
// 0: exists alone), evaluated in every wave and stored by wave 0.  false = the
// key is no candidate of the filter or the slice is empty: block-uniform.
__device__ __forceinline__ bool slab_consider(const QueryProg& qp, const ViewDev* __restrict__ views, const ViewDev& bv,
                                              int64_t ce, int s, int j, WaveScratch& ws, int slot0, int n, int wave,
                                              int lane) {
  uint64_t any = 0;
  if (qp.nprog) {
    uint32_t mask[MAXLEAF];
    build_slots(qp, views, s, ws, mask);
    if (!((candidate_mask(qp, mask) >> j) & 1)) return false;
    Tile f;
    eval_tile(qp, views, s, j, ws, f);
    slice_each(bv.payload, bv.meta[ce], ws.lb, slot0, n, [&](int i, ulong2 e) {
      const dq_u64x2 v{e.x & f.w[i].x, e.y & f.w[i].y};
      any |= v.x | v.y;
      if (wave == 0) bsi_slab[(i - slot0) * 64 + lane] = v;
    });
  } else {
    slice_each(bv.payload, bv.meta[ce], ws.lb, slot0, n, [&](int i, ulong2 e) {
      any |= e.x | e.y;
      if (wave == 0) bsi_slab[(i - slot0) * 64 + lane] = dq_u64x2{e.x, e.y};
    });
  }
  return __ballot(any != 0) != 0;
}

// Tiles [1, tiles), round-robin over the waves: ci_of(t) = the container of
// tile t, -1 = absent (its tile is never read back).  Array and run containers
// are expanded once through the wave's lb; a bitmap container loads only the
// slice's slots.  The caller's __syncthreads() follows.
template <class F>
__device__ __forceinline__ void slab_stage(const ViewDev& bv, WaveScratch& ws, int slot0, int n, int wave, int lane,
                                           int tiles, F&& ci_of) {
  for (int t = 1 + wave; t < tiles; t += WAVES_PER_BLOCK) {
    const int64_t ci = ci_of(t);
    if (ci < 0) continue;  // absent: never read back
    dq_u64x2* dst = bsi_slab + t * n * 64 + lane;
    slice_each(bv.payload, bv.meta[ci], ws.lb, slot0, n,
               [&](int i, ulong2 e) { dst[(i - slot0) * 64] = dq_u64x2{e.x, e.y}; });
  }
}

// lanes' plane containers -> the mask of the planes present at the key (depth <= 32)
__device__ __forceinline__ uint64_t slab_present(const BsiCtx& c, int depth) {
  return __ballot(c.planes >= 0) & ((1ull << depth) - 1);
}

// The gather of a word's <= 32 plane words through `present` (absent planes are
// zero) before bit_transpose32() stays written out in the three kernels: behind
// any function boundary the compiler allocates the SGPRs of that loop
// differently and every kernel's text moves by about 2 %
// (profiles/bsi_slab/README.md).

// Block-wide exclusive scan of one count per thread and slot, in two steps with
// a __syncthreads() between them: the waves' totals of slot k go to
// part[k][WAVES_PER_BLOCK] (LDS), then every thread adds the totals of the waves
// below it to its wave scan.  run = the position of the slot's first column; it
// advances by the slot's total.
__device__ __forceinline__ void slab_scan_totals(int* part, int k, int wave, int lane, int cnt) {
  const int incl = wave_scan_incl(cnt);
  if (lane == 63) part[k * WAVES_PER_BLOCK + wave] = incl;
}

__device__ __forceinline__ int64_t slab_scan_pos(const int* part, int k, int wave, int cnt, int64_t& run) {
  int64_t o = run + (wave_scan_incl(cnt) - cnt);
#pragma unroll
  for (int w = 0; w < WAVES_PER_BLOCK; w++) {
    const int p = part[k * WAVES_PER_BLOCK + w];
    if (w < wave) o += p;
    run += p;
  }
  return o;
}

// One workgroup of four waves per unit, lds bytes of dynamic LDS for the slab.
template <class K, class... A>
void slab_launch(K kernel, int64_t blocks, int lds, hipStream_t st, A... args) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL(kernel, dim3(unsigned(blocks)), dim3(64 * WAVES_PER_BLOCK), lds, st, args...);
}

}  // namespace pk
