// CDNA4 (gfx950) kernels for the bitmap index hot path: the expression
// evaluator (expr_count, union_count*, expr_materialize, expr_dense).  The
// kernels over bit-sliced int fields, built on the same tiles, have their own
// file.
//
// Reference hot loops replaced here:
//   K1/K2 popcountAndSlice / intersectionCount  roaring/roaring.go:3078-3215,5061-5072
//   K3-K6 intersect/union/difference/xor        roaring/roaring.go:3217-4344
//   K8    count/countRange                      roaring/roaring.go:2000-2110
//   K10   OffsetRange row extraction             roaring/roaring.go:535-558
//   K17/K21 TopN / GroupBy intersection counts  fragment.go:1568-1700, executor.go:3060-3230
//
// Execution model (ours): a whole batch of queries is evaluated over ALL local
// shards in one launch.  One 64-lane wave owns one (query, shard) work item
// and walks the <=16 container keys of the row in that shard, holding each
// container as a register tile and interpreting the query's postfix program
// over the tiles (expr_tile.h).
// Fast paths: Count(Row) sums container cardinalities from the metadata only;
// Count(Intersect(a,b)) dispatches on the container type pair
// (bitmap&bitmap popcount, array->bitmap probe, array->LDS-bitmap probe).
//
// Workgroups are remapped XCD-aware (xcd_remap, device_util.h): consecutive
// logical blocks (same shard, different queries -> the same hot containers)
// are kept on one XCD so they share its L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "expr_tile.h"

namespace pk {

// |A ∩ B| for two containers with a type-pair dispatch (no full tiles for arrays).
__device__ __forceinline__ int and2_count(const ViewDev& va, int64_t ma, const ViewDev& vb, int64_t mb,
                                          uint64_t* lb) {
  const int lane = wave_lane();
  const int ta = meta_type(ma), tb = meta_type(mb);
  int c = 0;
  if (ta == CT_BITMAP && tb == CT_BITMAP) {
    const ulong2* pa = reinterpret_cast<const ulong2*>(payload_of(va, ma));
    const ulong2* pb = reinterpret_cast<const ulong2*>(payload_of(vb, mb));
    ulong2 x[8], y[8];
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = pa[i * 64 + lane];
#pragma unroll
    for (int i = 0; i < 8; i++) y[i] = pb[i * 64 + lane];
#pragma unroll
    for (int i = 0; i < 8; i++) c += __popcll(x[i].x & y[i].x) + __popcll(x[i].y & y[i].y);
    return c;
  }
  if (ta == CT_RUN || tb == CT_RUN) {
    Tile a, b;
    tile_load(a, va.payload, ma, lb);
    tile_load(b, vb.payload, mb, lb);
    tile_op<OP_AND>(a, b);
    return tile_popc(a);
  }
  if (ta == CT_BITMAP || tb == CT_BITMAP) {
    // probe the bitmap with the array values; large arrays first stage the
    // 8 KiB bitmap into LDS with coalesced 16 B loads (random 8 B global
    // probes would touch every line anyway).
    const bool abit = ta == CT_BITMAP;
    const uint64_t* bw = reinterpret_cast<const uint64_t*>((abit ? va.payload : vb.payload) +
                                                           meta_off16(abit ? ma : mb) * 8);
    const int64_t am = abit ? mb : ma;
    const uint16_t* arr = (abit ? vb.payload : va.payload) + meta_off16(am) * 8;
    const int n = meta_n(am);
    const uint64_t* probe = bw;
    if (n >= 256) {
      const ulong2* src = reinterpret_cast<const ulong2*>(bw);
      ulong2* l2 = reinterpret_cast<ulong2*>(lb);
      ulong2 t[8];
#pragma unroll
      for (int i = 0; i < 8; i++) t[i] = src[i * 64 + lane];
#pragma unroll
      for (int i = 0; i < 8; i++) l2[i * 64 + lane] = t[i];
      lds_fence();
      probe = lb;
    }
    c = probe_array(probe, arr, n);
    if (n >= 256) lds_fence();
    return c;
  }
  // array & array: scatter the larger into LDS, probe with the smaller
  const bool abig = meta_n(ma) >= meta_n(mb);
  const int64_t mbig = abig ? ma : mb, msmall = abig ? mb : ma;
  const ViewDev& vbig = abig ? va : vb;
  const ViewDev& vsmall = abig ? vb : va;
  lds_expand(lb, vbig.payload, mbig);
  c = probe_array(lb, payload_of(vsmall, msmall), meta_n(msmall));
  lds_fence();
  return c;
}

// Count kernel: out[q] += |program(q)| over all local shards.
// MODE 1 (fast) handles only Count(Row) and Count(Intersect(a,b)) programs
// (no register tile stack -> far fewer VGPRs, higher occupancy); MODE 2
// (flat) handles left folds "l0 l1 op l2 op ..." (Union/Intersect/Difference/
// Xor of leaves, time-range view unions, Not) with one accumulator tile and
// one load tile; MODE 0 interprets any program with the 4-deep tile stack.
template <int MODE>
__global__ __launch_bounds__(256, MODE == 0 ? 1 : 4) void expr_count_kernel(const QueryProg* __restrict__ progs, int Q,
                                                         const ViewDev* __restrict__ views, int S,
                                                         unsigned long long* __restrict__ out,
                                                         int32_t* __restrict__ per_key,
                                                         int64_t* __restrict__ per_shard) {
  __shared__ WaveScratch scratch[WAVES_PER_BLOCK];
  const uint32_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const int64_t item = int64_t(blk) * WAVES_PER_BLOCK + wave;
  if (item >= int64_t(Q) * S) return;
  const int q = int(item % Q);
  const int s = int(item / Q);
  const QueryProg& qp = progs[q];
  WaveScratch& ws = scratch[wave];
  uint32_t mask[MAXLEAF];
  build_slots(qp, views, s, ws, mask);
  const uint32_t cand = candidate_mask(qp, mask);
  int64_t total = 0;
  if (cand) {
    if (qp.nprog == 1) {
      // Count(Row): metadata only
      if (lane < 16 && ((cand >> lane) & 1)) {
        const int n = meta_n(ws.meta[0][lane]);
        total = n;
        if (per_key) per_key[(int64_t(q) * S + s) * 16 + lane] = n;
      }
    } else if (MODE == 1) {
      // Count(Intersect(leaf0, leaf1)) with a container type-pair dispatch
      const ViewDev& va = views[qp.leaf_view[0]];
      const ViewDev& vb = views[qp.leaf_view[1]];
      for (uint32_t cm = cand; cm; cm &= cm - 1) {
        const int j = __builtin_ctz(cm);
        const int64_t ma = ws.meta[0][j];
        const int64_t mb = ws.meta[1][j];
        total += and2_count(va, ma, vb, mb, ws.lb);
      }
    } else {
      for (uint32_t cm = cand; cm; cm &= cm - 1) {
        const int j = __builtin_ctz(cm);
        Tile acc;
        if (MODE == 2) eval_flat(qp, views, s, j, ws, acc);
        else eval_tile(qp, views, s, j, ws, acc);
        int c = tile_popc(acc);
        if (per_key) {
          const int64_t cj = wave_sum_i64(c);
          if (lane == 0) per_key[(int64_t(q) * S + s) * 16 + j] = int32_t(cj);
        }
        total += c;
      }
    }
  }
  total = wave_sum_i64(total);
  if (lane == 0 && total && out) atomicAdd(out + q, (unsigned long long)total);
  if (lane == 0 && per_shard) per_shard[int64_t(q) * S + s] = total;
}

// Union count (MODE 3 of launch_expr_count): Count(Union(l0, l1, ...)) of
// plain leaves, e.g. the covering time views of Row(t=r, from, to)
// (reference executeRowShard unions the views, executor.go:1444-1533).  Per
// key the wave clears one LDS bitmap and ORs every leaf container into it
// with returning LDS atomics; a bit counts when its OR flips it
// (popcount(mask & ~old)), so no tile is expanded, combined or read back --
// for the small arrays of time views that is most of the work.
__global__ __launch_bounds__(256) void union_count_kernel(const QueryProg* __restrict__ progs, int Q,
                                                          const ViewDev* __restrict__ views, int S,
                                                          unsigned long long* __restrict__ out) {
  __shared__ WaveScratch scratch[WAVES_PER_BLOCK];
  const uint32_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const int64_t item = int64_t(blk) * WAVES_PER_BLOCK + wave;
  if (item >= int64_t(Q) * S) return;
  const int q = int(item % Q);
  const int s = int(item / Q);
  const QueryProg& qp = progs[q];
  WaveScratch& ws = scratch[wave];
  uint32_t mask[MAXLEAF];
  build_slots(qp, views, s, ws, mask);
  uint32_t cand = 0;
  for (int k = 0; k < qp.nleaf; k++) cand |= mask[k];
  unsigned long long* lb64 = reinterpret_cast<unsigned long long*>(ws.lb);
  uint32_t* lb32 = reinterpret_cast<uint32_t*>(ws.lb);
  int64_t total = 0;
  for (uint32_t cm = cand; cm; cm &= cm - 1) {
    const int j = __builtin_ctz(cm);
    ulong2* l2 = reinterpret_cast<ulong2*>(ws.lb);
#pragma unroll
    for (int i = 0; i < 8; i++) l2[i * 64 + lane] = make_ulong2(0, 0);
    lds_fence();
    for (int k = 0; k < qp.nleaf; k++) {
      const int64_t m = ws.meta[k][j];
      if (m < 0) continue;
      const ViewDev& v = views[qp.leaf_view[k]];
      const uint16_t* p = payload_of(v, m);
      const int type = meta_type(m);
      if (type == CT_BITMAP) {
        const ulong2* g = reinterpret_cast<const ulong2*>(p);
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const ulong2 w = g[i * 64 + lane];
          const int wi = 2 * (i * 64 + lane);
          const unsigned long long ox = atomicOr(lb64 + wi, (unsigned long long)w.x);
          const unsigned long long oy = atomicOr(lb64 + wi + 1, (unsigned long long)w.y);
          total += __popcll(w.x & ~ox) + __popcll(w.y & ~oy);
        }
      } else if (type == CT_ARRAY) {
        const int n = meta_n(m);
        const uint4* p4 = reinterpret_cast<const uint4*>(p);
        for (int e8 = lane; e8 < ((n + 7) >> 3); e8 += 64) {
          const uint4 v4 = p4[e8];
          const uint32_t w4[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
          for (int t = 0; t < 8; t++) {
            if (e8 * 8 + t < n) {
              const uint32_t x = (w4[t >> 1] >> ((t & 1) * 16)) & 0xffff;
              const uint32_t bit = 1u << (x & 31);
              total += (atomicOr(lb32 + (x >> 5), bit) & bit) ? 0 : 1;
            }
          }
        }
      } else {
        const int nr = p[0];
        for (int r = lane; r < nr; r += 64) {
          const uint32_t st = p[8 + 2 * r], e = uint32_t(p[9 + 2 * r]) + 1;
          for (uint32_t w = st >> 6; w <= (e - 1) >> 6; w++) {
            uint64_t mk = ~0ull;
            if (w == (st >> 6)) mk &= ~0ull << (st & 63);
            if (w == ((e - 1) >> 6) && (e & 63)) mk &= (1ull << (e & 63)) - 1;
            total += __popcll(mk & ~atomicOr(lb64 + w, (unsigned long long)mk));
          }
        }
      }
    }
    lds_fence();
  }
  total = wave_sum_i64(total);
  if (lane == 0 && total) atomicAdd(out + q, (unsigned long long)total);
}

// Union count v2 (MODE 4, the default for Count(Union(leaves))).  v1 above
// walks the leaves of a key one after the other: slot (LDS) -> meta (global)
// -> payload (global) -> returning LDS atomics, i.e. two dependent global
// round trips per (leaf, key), ~7x16 of them in series per (query, shard) for
// a YMDH time range.  Here
//   * the metas of every (leaf, key) are fetched in one parallel round trip
//     (lane = (leaf, container) pair) into a wave-private LDS table;
//   * per key, the present leaves' payloads are walked as ONE flat list of
//     16-byte chunks (array: 8 values, bitmap: 2 words), so the loads of all
//     leaves are in flight together (4 per lane per step); a lane finds its
//     chunk's leaf by comparing with the leaves' chunk prefix (scalar
//     readlanes) and fetches the leaf's meta / payload pointer with bpermutes;
//   * values are OR-ed into the LDS bitmap with NON-returning ds_or, and the
//     key's union is counted by one popcount pass that also re-zeroes it;
//   * a key present in one leaf only is counted from its metadata.
// Run containers (rare in time views) are OR-ed in a second, per-run loop.
__device__ __forceinline__ int shfl_i32(int v, int src) { return __shfl(v, src); }
__device__ __forceinline__ int64_t shfl_i64(int64_t v, int src) {
  const int lo = __shfl(int(uint64_t(v)), src), hi = __shfl(int(uint64_t(v) >> 32), src);
  return int64_t((uint64_t(uint32_t(hi)) << 32) | uint32_t(lo));
}

__global__ __launch_bounds__(256) void union_count2_kernel(const QueryProg* __restrict__ progs, int Q,
                                                           const ViewDev* __restrict__ views, int S,
                                                           unsigned long long* __restrict__ out) {
  __shared__ uint32_t lbits[WAVES_PER_BLOCK][2048];
  __shared__ int64_t lmeta[WAVES_PER_BLOCK][MAXLEAF * 16];
  const uint32_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const int64_t item = int64_t(blk) * WAVES_PER_BLOCK + wave;
  if (item >= int64_t(Q) * S) return;
  const int q = int(item % Q);
  const int s = int(item / Q);
  const QueryProg& qp = progs[q];
  const int nleaf = qp.nleaf;
  uint32_t* lb = lbits[wave];
  int64_t* mt = lmeta[wave];
  for (int t = lane; t < MAXLEAF * 16; t += 64) mt[t] = -1;
  {
    uint4* lb4 = reinterpret_cast<uint4*>(lb);
#pragma unroll
    for (int i = 0; i < 8; i++) lb4[i * 64 + lane] = make_uint4(0, 0, 0, 0);
  }
  lds_fence();
  // (leaf, container) metas: lane -> leaf k0 + lane/16, container lane%16
#pragma unroll
  for (int k0 = 0; k0 < MAXLEAF; k0 += 4) {
    const int k = k0 + (lane >> 4), idx = lane & 15;
    if (k0 < nleaf && k < nleaf) {
      const int64_t d = qp.leaf_row[k];
      if (d >= 0) {
        const ViewDev& v = views[qp.leaf_view[k]];
        const uint32_t* rp = v.rowptr + int64_t(s) * (v.D + 1);
        const int64_t base = v.shard_base[s];
        const int64_t lo = base + rp[d], hi = base + rp[d + 1];
        if (idx < hi - lo) {
          const int64_t m = v.meta[lo + idx];
          mt[k * 16 + meta_j(m)] = m;
        }
      }
    }
  }
  lds_fence();
  bool has = false;
  if (lane < 16)
    for (int k = 0; k < nleaf; k++) has |= mt[k * 16 + lane] >= 0;
  const uint32_t cand = uint32_t(__ballot(has) & 0xffff);
  // per-leaf payload base pointer (lane k < nleaf)
  const uint16_t* lpay = lane < nleaf ? views[qp.leaf_view[lane]].payload : nullptr;
  int64_t total = 0;
  unsigned long long* lb64 = reinterpret_cast<unsigned long long*>(lb);
  for (uint32_t cm = cand; cm; cm &= cm - 1) {
    const int j = __builtin_ctz(cm);
    const int64_t m = lane < nleaf ? mt[lane * 16 + j] : -1;
    const uint64_t pres = __ballot(m >= 0);
    if (__popcll(pres) == 1) {  // one leaf holds this key: its cardinality
      if (lane == __builtin_ctzll(pres)) total += meta_n(m);
      continue;
    }
    const int type = m >= 0 ? meta_type(m) : -1;
    const int cnt = type == CT_ARRAY ? (meta_n(m) + 7) >> 3 : (type == CT_BITMAP ? 512 : 0);
    // inclusive scan of chunk counts over lanes 0..15
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
      const int t = __shfl_up(incl, d);
      if ((lane & 15) >= d) incl += t;
    }
    const int pre = incl - cnt;
    const int tot = __builtin_amdgcn_readlane(incl, 15);
    const uint16_t* lptr = (m >= 0) ? lpay + meta_off16(m) * 8 : nullptr;
    for (int c0 = 0; c0 < tot; c0 += 256) {
      int c[4], leaf[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { c[u] = c0 + u * 64 + lane; leaf[u] = 0; }
      for (int k = 1; k < nleaf; k++) {
        const int pk = __builtin_amdgcn_readlane(pre, k);
#pragma unroll
        for (int u = 0; u < 4; u++) leaf[u] += c[u] >= pk;
      }
      uint4 v[4];
      int64_t mm[4];
      int loc[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        mm[u] = shfl_i64(m, leaf[u]);
        loc[u] = c[u] - shfl_i32(pre, leaf[u]);
        const uint4* p = reinterpret_cast<const uint4*>(shfl_i64(int64_t(lptr), leaf[u]));
        if (c[u] < tot) v[u] = p[loc[u]];
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if (c[u] >= tot) continue;
        if (meta_type(mm[u]) == CT_BITMAP) {
          atomicOr(lb64 + 2 * loc[u], (unsigned long long)(uint64_t(v[u].y) << 32 | v[u].x));
          atomicOr(lb64 + 2 * loc[u] + 1, (unsigned long long)(uint64_t(v[u].w) << 32 | v[u].z));
        } else {
          const int n = meta_n(mm[u]);
          const uint32_t w4[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
          for (int t = 0; t < 8; t++) {
            const uint32_t x = (w4[t >> 1] >> ((t & 1) * 16)) & 0xffff;
            if (loc[u] * 8 + t < n) atomicOr(lb + (x >> 5), 1u << (x & 31));
          }
        }
      }
    }
    // run containers of this key
    uint64_t runs = __ballot(type == CT_RUN);
    for (; runs; runs &= runs - 1) {
      const int k = __builtin_ctzll(runs);
      const uint16_t* p = reinterpret_cast<const uint16_t*>(shfl_i64(int64_t(lptr), k));
      const int nr = p[0];
      for (int r = lane; r < nr; r += 64) {
        const uint32_t st = p[8 + 2 * r], e = uint32_t(p[9 + 2 * r]) + 1;
        for (uint32_t w = st >> 6; w <= (e - 1) >> 6; w++) {
          uint64_t mk = ~0ull;
          if (w == (st >> 6)) mk &= ~0ull << (st & 63);
          if (w == ((e - 1) >> 6) && (e & 63)) mk &= (1ull << (e & 63)) - 1;
          atomicOr(lb64 + w, (unsigned long long)mk);
        }
      }
    }
    lds_fence();
    uint4* lb4 = reinterpret_cast<uint4*>(lb);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint4 w = lb4[i * 64 + lane];
      total += __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);
      lb4[i * 64 + lane] = make_uint4(0, 0, 0, 0);
    }
    lds_fence();
  }
  total = wave_sum_i64(total);
  if (lane == 0 && total) atomicAdd(out + q, (unsigned long long)total);
}

// Materialize kernel: writes result containers for every (q, s, j) with
// counts[q,s,j] > 0 at u16 offset offs[q,s,j]; array if n <= 4096 else bitmap.
__global__ __launch_bounds__(256) void expr_materialize_kernel(const QueryProg* __restrict__ progs, int Q,
                                                               const ViewDev* __restrict__ views, int S,
                                                               const int32_t* __restrict__ counts,
                                                               const int64_t* __restrict__ offs,
                                                               uint16_t* __restrict__ outp) {
  __shared__ WaveScratch scratch[WAVES_PER_BLOCK];
  const uint32_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const int64_t item = int64_t(blk) * WAVES_PER_BLOCK + wave;
  if (item >= int64_t(Q) * S) return;
  const int q = int(item % Q);
  const int s = int(item / Q);
  const QueryProg& qp = progs[q];
  WaveScratch& ws = scratch[wave];
  uint32_t mask[MAXLEAF];
  build_slots(qp, views, s, ws, mask);
  const uint32_t cand = candidate_mask(qp, mask);
  for (uint32_t cm = cand; cm; cm &= cm - 1) {
    const int j = __builtin_ctz(cm);
    const int64_t key = (int64_t(q) * S + s) * 16 + j;
    const int n = counts[key];
    if (n <= 0) continue;
    Tile acc;
    eval_tile(qp, views, s, j, ws, acc);
    uint16_t* dst = outp + offs[key];
    if (n > ARRAY_MAX) {
      ulong2* d2 = reinterpret_cast<ulong2*>(dst);
#pragma unroll
      for (int i = 0; i < 8; i++) d2[i * 64 + lane] = acc.w[i];
    } else {
      // ordered compaction: chunk i covers words [128i, 128i+128), lane l owns
      // words 128i+2l, 128i+2l+1 -> exclusive wave scan of per-lane popcounts.
      int base = 0;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const uint64_t x = acc.w[i].x, y = acc.w[i].y;
        const int c = __popcll(x) + __popcll(y);
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_up(incl, o, 64);
          if (lane >= o) incl += t;
        }
        int pos = base + incl - c;
        const int wbase = 128 * i + 2 * lane;
        for (uint64_t b = x; b; b &= b - 1) dst[pos++] = uint16_t(wbase * 64 + __builtin_ctzll(b));
        for (uint64_t b = y; b; b &= b - 1) dst[pos++] = uint16_t((wbase + 1) * 64 + __builtin_ctzll(b));
        base += __shfl(incl, 63, 64);
      }
    }
  }
}

// Dense evaluation: every (q, s, j) result tile is written as a bitmap
// container at the fixed u16 offset ((q*S + s)*16 + j) * 4096 of `outp`, with
// its metadata word (key j, bitmap, n, offset) in out_meta.  The result is a
// one-row device view per query whose shard layout matches the inputs; Shift
// (row_kernels.hip) reads it back word-addressed.
__global__ __launch_bounds__(256) void expr_dense_kernel(const QueryProg* __restrict__ progs, int Q,
                                                         const ViewDev* __restrict__ views, int S,
                                                         uint16_t* __restrict__ outp, int64_t* __restrict__ out_meta) {
  __shared__ WaveScratch scratch[WAVES_PER_BLOCK];
  const uint32_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const int64_t item = int64_t(blk) * WAVES_PER_BLOCK + wave;
  if (item >= int64_t(Q) * S) return;
  const int q = int(item % Q);
  const int s = int(item / Q);
  const QueryProg& qp = progs[q];
  WaveScratch& ws = scratch[wave];
  uint32_t mask[MAXLEAF];
  build_slots(qp, views, s, ws, mask);
  const uint32_t cand = candidate_mask(qp, mask);
  for (int j = 0; j < 16; j++) {
    const int64_t key = (int64_t(q) * S + s) * 16 + j;
    Tile acc;
    if ((cand >> j) & 1) eval_tile(qp, views, s, j, ws, acc);
    else tile_zero(acc);
    ulong2* d2 = reinterpret_cast<ulong2*>(outp + key * 4096);
#pragma unroll
    for (int i = 0; i < 8; i++) d2[i * 64 + lane] = acc.w[i];
    const int64_t n = wave_sum_i64(tile_popc(acc));
    if (lane == 0) out_meta[key] = int64_t(j) | (int64_t(CT_BITMAP) << 4) | (n << 6) | ((key * 512) << 23);
  }
}

// ------------------------------------------------------------ launchers

void launch_expr_count(const QueryProg* progs, int Q, const ViewDev* views, int S, unsigned long long* out,
                       int32_t* per_key, int64_t* per_shard, int mode, hipStream_t st) {
  const int64_t items = int64_t(Q) * S;
  if (items == 0) return;
  const dim3 grid(grid_for(items)), block(64 * WAVES_PER_BLOCK);
  if (mode == 4 && per_key == nullptr && per_shard == nullptr)
    hipLaunchKernelGGL(union_count2_kernel, grid, block, 0, st, progs, Q, views, S, out);
  else if (mode == 3 && per_key == nullptr && per_shard == nullptr)
    hipLaunchKernelGGL(union_count_kernel, grid, block, 0, st, progs, Q, views, S, out);
  else if (mode == 1 && per_key == nullptr)
    hipLaunchKernelGGL(expr_count_kernel<1>, grid, block, 0, st, progs, Q, views, S, out, per_key, per_shard);
  else if (mode == 2 || mode == 3 || mode == 4)
    hipLaunchKernelGGL(expr_count_kernel<2>, grid, block, 0, st, progs, Q, views, S, out, per_key, per_shard);
  else
    hipLaunchKernelGGL(expr_count_kernel<0>, grid, block, 0, st, progs, Q, views, S, out, per_key, per_shard);
}

void launch_expr_materialize(const QueryProg* progs, int Q, const ViewDev* views, int S, const int32_t* counts,
                             const int64_t* offs, uint16_t* outp, hipStream_t st) {
  const int64_t items = int64_t(Q) * S;
  if (items == 0) return;
  hipLaunchKernelGGL(expr_materialize_kernel, dim3(grid_for(items)), dim3(64 * WAVES_PER_BLOCK), 0, st, progs,
                     Q, views, S, counts, offs, outp);
}

void launch_expr_dense(const QueryProg* progs, int Q, const ViewDev* views, int S, uint16_t* outp, int64_t* out_meta,
                       hipStream_t st) {
  const int64_t items = int64_t(Q) * S;
  if (items == 0) return;
  hipLaunchKernelGGL(expr_dense_kernel, dim3(grid_for(items)), dim3(64 * WAVES_PER_BLOCK), 0, st, progs, Q, views, S,
                     outp, out_meta);
}

}  // namespace pk
