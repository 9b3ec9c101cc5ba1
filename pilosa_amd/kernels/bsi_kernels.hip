// CDNA4 (gfx950) kernels over bit-sliced (BSI) int fields: Sum, Sum per group,
// range predicates, Min / Max and the k-th value (Percentile).
//
// Reference hot loops replaced here:
//   K13   BSI sum                                fragment.go:1109-1141
//         BSI range comparators                  fragment.go:1271-1534
//         BSI min / max                          fragment.go:1145-1225
//
// A BSI view holds row 0 (exists), row 1 (sign) and rows 2+i (bit plane i); the
// host resolves them to dense row indices (BsiArgs: row_exists / row_sign /
// bit_row[i], -1 = absent).  One 64-lane wave owns one (shard, key) item (times
// a query or group for the sums) and combines the planes' containers as
// register tiles; filters are ordinary expression programs evaluated through
// the same tiles (expr_tile.h).  Workgroups are remapped XCD-aware (xcd_remap,
// device_util.h) so the items that read the same planes share an L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "expr_tile.h"
#include "bsi_tile.h"

namespace pk {

// BSI sum over bit-sliced rows (fragment.go:1109-1141):
//   consider = exists & filter ; count = |consider|
//   sum = Σ_i 2^i (|B_i & consider & ~sign| - |B_i & consider & sign|)
//
// Key-parallel: one wave per (shard, key, query), the
// queries of one (shard, key) on consecutive waves of one XCD so the bit
// planes they all read are shared through its L2.  Lanes first resolve the
// container of every bit plane at this key in parallel (lane i: plane i), so
// the plane loop issues its tile loads without a dependent metadata walk.
// FMODE: 0 no filter, 1 flat-fold filter (two tiles), 2 any program (tile stack).
template <int FMODE>
__global__ __launch_bounds__(256) void bsi_sum_keys_kernel(const QueryProg* __restrict__ progs, int Q,
                                                           const ViewDev* __restrict__ views, int S, BsiArgs bsi,
                                                           unsigned long long* __restrict__ out_sum,
                                                           unsigned long long* __restrict__ out_cnt) {
  __shared__ WaveScratch scratch[WAVES_PER_BLOCK];
  const uint32_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const int64_t item = int64_t(blk) * WAVES_PER_BLOCK + wave;
  const bool live = item < int64_t(Q) * S * 16;
  const int q = live ? int(item % Q) : -1;
  // the wave's (sum, count); the block folds its waves' results into one
  // atomic pair per query: 15k waves hitting the same two words serialise
  // at one L2 channel
  int64_t tsum = 0, tcnt = 0;
  auto work = [&]() {
    const int j = int((item / Q) & 15);
    const int s = int(item / (int64_t(Q) * 16));
    const QueryProg& qp = progs[q];
    WaveScratch& ws = scratch[wave];
    const ViewDev& bv = views[bsi.view];
    const uint32_t* rp = bv.rowptr + int64_t(s) * (bv.D + 1);
    const int64_t base = bv.shard_base[s];
    // container index of dense row d at key j (or -1), evaluated per lane
    auto lane_find = [&](int64_t d) -> int64_t {
      if (d < 0) return -1;
      const int64_t lo = base + rp[d], hi = base + rp[d + 1];
      if (hi - lo == 16) return lo + j;   // every key present (dense planes): no meta walk
      for (int64_t c = lo; c < hi; c++)
        if (meta_j(bv.meta[c]) == j) return c;
      return -1;
    };
    // lane i < depth (<= 63): bit plane i; lanes 0 / 1 then resolve exists /
    // sign in a second parallel lookup
    const int64_t mine = lane < bsi.depth ? lane_find(bsi.bit_row[lane]) : -1;
    const int64_t extra = lane == 0 ? lane_find(bsi.row_exists) : (lane == 1 ? lane_find(bsi.row_sign) : -1);
    const int64_t ce = rl_i64(extra, 0);
    if (ce < 0) return;
    Tile consider, sign, bits;
    tile_load(consider, bv.payload, bv.meta[ce], ws.lb);
    if (FMODE != 0 && qp.nprog) {
      uint32_t mask[MAXLEAF];
      build_slots(qp, views, s, ws, mask);
      if (!((candidate_mask(qp, mask) >> j) & 1)) return;
      Tile f;
      if (FMODE == 1) eval_flat(qp, views, s, j, ws, f);
      else eval_tile(qp, views, s, j, ws, f);
      tile_op<OP_AND>(consider, f);
    }
    const int64_t acc_cnt = tile_popc(consider);
    const int64_t cs = rl_i64(extra, 1);
    if (cs >= 0) tile_load(sign, bv.payload, bv.meta[cs], ws.lb);
    else tile_zero(sign);
    // consider splits into its non-negative and negative columns once per key
    // (consider <- consider & ~sign, sign <- consider & sign); a key with no
    // negative column (the usual case: the sign row is sparse) then counts one
    // AND + popcount per plane word instead of two
    uint64_t anyneg = 0;
  #pragma unroll
    for (int w = 0; w < 8; w++) {
      const ulong2 c = consider.w[w], g = sign.w[w];
      consider.w[w] = make_ulong2(c.x & ~g.x, c.y & ~g.y);
      sign.w[w] = make_ulong2(c.x & g.x, c.y & g.y);
      anyneg |= sign.w[w].x | sign.w[w].y;
    }
    const bool neg = __ballot(anyneg != 0) != 0;
    int64_t acc_sum = 0;
    // planes double-buffered: the next present plane's tile is in flight
    // while the current one is counted (one load round trip per plane, not
    // a wait before every plane)
    const uint64_t present = __ballot(mine >= 0) & (bsi.depth >= 64 ? ~0ull : ((1ull << bsi.depth) - 1));
    auto count_plane = [&](const Tile& t, int i) {
      int pc = 0, nc = 0;
  #pragma unroll
      for (int w = 0; w < 8; w++) pc += __popcll(t.w[w].x & consider.w[w].x) + __popcll(t.w[w].y & consider.w[w].y);
      if (neg) {
  #pragma unroll
        for (int w = 0; w < 8; w++) nc += __popcll(t.w[w].x & sign.w[w].x) + __popcll(t.w[w].y & sign.w[w].y);
      }
      acc_sum += int64_t(uint64_t(int64_t(pc - nc)) << i);
    };
    Tile bits2;
    uint64_t left = present;
    int cur = left ? __builtin_ctzll(left) : -1;
    if (cur >= 0) {
      left &= left - 1;
      tile_load(bits, bv.payload, bv.meta[rl_i64(mine, cur)], ws.lb);
    }
    while (cur >= 0) {
      int nxt = left ? __builtin_ctzll(left) : -1;
      if (nxt >= 0) {
        left &= left - 1;
        tile_load(bits2, bv.payload, bv.meta[rl_i64(mine, nxt)], ws.lb);
      }
      count_plane(bits, cur);
      cur = nxt;
      if (cur < 0) break;
      nxt = left ? __builtin_ctzll(left) : -1;
      if (nxt >= 0) {
        left &= left - 1;
        tile_load(bits, bv.payload, bv.meta[rl_i64(mine, nxt)], ws.lb);
      }
      count_plane(bits2, cur);
      cur = nxt;
    }
    tsum = wave_sum_i64(acc_sum);
    tcnt = wave_sum_i64(acc_cnt);
  };
  if (live) work();
  __shared__ long long red_s[WAVES_PER_BLOCK], red_c[WAVES_PER_BLOCK];
  __shared__ int red_q[WAVES_PER_BLOCK];
  if (lane == 0) {
    red_s[wave] = tsum;
    red_c[wave] = tcnt;
    red_q[wave] = q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < WAVES_PER_BLOCK; w++) {
      const int qw = red_q[w];
      if (qw < 0) continue;
      long long ss = red_s[w], cc = red_c[w];
      for (int w2 = w + 1; w2 < WAVES_PER_BLOCK; w2++)
        if (red_q[w2] == qw) {
          ss += red_s[w2];
          cc += red_c[w2];
          red_q[w2] = -1;
        }
      if (ss) atomicAdd(out_sum + qw, (unsigned long long)ss);
      if (cc) atomicAdd(out_cnt + qw, (unsigned long long)cc);
    }
  }
}

// BSI sum per group (GroupBy(..., aggregate=Sum(field=))): G filter programs
// -- one per group, the GroupBy filter followed by the group's rows as a left
// AND-fold -- over one BSI field.  bsi_sum_keys_kernel gives every (shard,
// key, group) wave its own pass over all depth+2 plane tiles and decodes array
// and run planes through LDS each time.  Here one workgroup owns one (shard,
// key, plane slab, chunk of groups): its four waves stage exists, sign and the
// slab's planes once into a block-shared LDS slab, in the per-lane Tile layout
// (ulong2 at [i*64 + lane], so a read-back is eight conflict-free 16-byte LDS
// reads), then stream the chunk's groups past them round-robin.  A group that
// misses a leaf at this key costs no tile; one that is empty after the AND
// with exists costs no plane.  The only barrier is the __syncthreads() after
// staging; a workgroup whose key has no exists container leaves before it
// (wave- and block-uniform).  Every wave adds its (group, unit) result with
// one 64-bit atomic per output word, out_cnt from slab 0 only; zeros are
// skipped.
//
// Measured (profiles/groupby_sum/README.md: 64 shards, depth 20, bitmap planes)
// it moves 59 times fewer plane tiles than bsi_sum_keys_kernel at 1,024 groups
// and still takes 1.2 - 1.3 times as long at 8, 32 and 1,024 groups: one
// workgroup per CU and an unoverlapped chain of dependent loads per group,
// repeated per slab.  GpuExecutor therefore routes to it only on request
// (PILOSA_GROUPSUM_MIN_GROUPS).
//
// LDS: four WaveScratch (40 KiB, static) + (2 + planes) * 8 KiB dynamic; the
// 160 KiB of a CU bound planes at GS_MAX_PLANES = 13 (one workgroup per CU), 3
// planes still fit two workgroups.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage):
//   FMODE 1 (flat folds):  172 VGPRs, 0 AGPRs, 84 SGPRs, scratch 0, static LDS
//                          40960 B, occupancy 2 waves/SIMD by registers
//   FMODE 2 (any program): 256 VGPRs, 38 AGPRs, 84 SGPRs, scratch 0, static LDS
//                          40960 B, occupancy 1 wave/SIMD
// The slab is a native 16-byte vector (u64x2, moved as ds_*_b128), not ulong2:
// copying Tile words to LDS as HIP vector structs left the staged tile in
// 144 B/lane of scratch.
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

template <int FMODE>
__global__ __launch_bounds__(256) void bsi_group_sum_kernel(const QueryProg* __restrict__ progs, int G,
                                                            const ViewDev* __restrict__ views, int S, BsiArgs bsi,
                                                            int planes, int nslab, int gchunk, int nchunk,
                                                            unsigned long long* __restrict__ out_sum,
                                                            unsigned long long* __restrict__ out_cnt) {
  __shared__ WaveScratch scratch[WAVES_PER_BLOCK];
  extern __shared__ u64x2 gs_slab[];  // [2 + planes][512]: exists, sign, planes of the slab
  const uint32_t unit = xcd_remap(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const int chunk = int(unit % uint32_t(nchunk));
  const int slab = int((unit / uint32_t(nchunk)) % uint32_t(nslab));
  const int j = int((unit / (uint32_t(nchunk) * uint32_t(nslab))) & 15);
  const int s = int(unit / (uint32_t(nchunk) * uint32_t(nslab) * 16));
  if (s >= S) return;
  WaveScratch& ws = scratch[wave];
  const ViewDev& bv = views[bsi.view];
  const uint32_t* rp = bv.rowptr + int64_t(s) * (bv.D + 1);
  const int64_t base = bv.shard_base[s];
  // container index of dense row d at key j (or -1), evaluated per lane
  auto lane_find = [&](int64_t d) -> int64_t {
    if (d < 0) return -1;
    const int64_t lo = base + rp[d], hi = base + rp[d + 1];
    if (hi - lo == 16) return lo + j;   // every key present (dense planes): no meta walk
    for (int64_t c = lo; c < hi; c++)
      if (meta_j(bv.meta[c]) == j) return c;
    return -1;
  };
  // every wave resolves the same containers (lane i: plane i; then lanes 0 / 1:
  // exists / sign), so the staging split needs no exchange between waves
  const int p0 = slab * planes;
  const int np = min(planes, bsi.depth - p0);  // planes of this slab (<= 0: none, depth 0)
  const int64_t mine = (lane >= p0 && lane < p0 + np) ? lane_find(bsi.bit_row[lane]) : -1;
  const int64_t extra = lane == 0 ? lane_find(bsi.row_exists) : (lane == 1 ? lane_find(bsi.row_sign) : -1);
  const int64_t ce = rl_i64(extra, 0);
  if (ce < 0) return;
  const int64_t cs = rl_i64(extra, 1);
  const uint64_t present = __ballot(mine >= 0);
  // stage: wave w decodes tiles w, w+4, ... (0 exists, 1 sign, 2+p plane p0+p)
  for (int t = wave; t < 2 + np; t += WAVES_PER_BLOCK) {
    const int64_t ci = t == 0 ? ce : (t == 1 ? cs : rl_i64(mine, p0 + t - 2));
    if (ci < 0) continue;  // absent: never read back
    Tile tl;
    tile_load(tl, bv.payload, bv.meta[ci], ws.lb);
#pragma unroll
    for (int i = 0; i < 8; i++) gs_slab[t * 512 + i * 64 + lane] = u64x2{tl.w[i].x, tl.w[i].y};
  }
  __syncthreads();
  const int g1 = min(G, (chunk + 1) * gchunk);
  for (int g = chunk * gchunk + wave; g < g1; g += WAVES_PER_BLOCK) {
    const QueryProg& qp = progs[g];
    Tile consider;
    if (qp.nprog) {
      uint32_t mask[MAXLEAF];
      build_slots(qp, views, s, ws, mask);
      if (!candidate_at(qp, ws, j)) continue;
      if (FMODE == 1) eval_flat(qp, views, s, j, ws, consider);
      else eval_tile(qp, views, s, j, ws, consider);
      uint64_t any = 0;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const u64x2 e = gs_slab[i * 64 + lane];
        consider.w[i].x &= e.x;
        consider.w[i].y &= e.y;
        any |= consider.w[i].x | consider.w[i].y;
      }
      if (!__ballot(any != 0)) continue;
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const u64x2 e = gs_slab[i * 64 + lane];
        consider.w[i] = make_ulong2(e.x, e.y);
      }
    }
    const int64_t acc_cnt = slab == 0 ? tile_popc(consider) : 0;
    // split once by sign (consider <- non-negative, sign <- negative columns);
    // a key without a negative column counts one AND + popcount per plane word
    Tile sign;
    bool neg = false;
    if (cs >= 0 && np > 0) {
      uint64_t anyneg = 0;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const ulong2 c = consider.w[i];
        const u64x2 sg = gs_slab[512 + i * 64 + lane];
        consider.w[i] = make_ulong2(c.x & ~sg.x, c.y & ~sg.y);
        sign.w[i] = make_ulong2(c.x & sg.x, c.y & sg.y);
        anyneg |= sign.w[i].x | sign.w[i].y;
      }
      neg = __ballot(anyneg != 0) != 0;
    }
    int64_t acc_sum = 0;
    for (int p = 0; p < np; p++) {
      if (!((present >> (p0 + p)) & 1)) continue;
      const u64x2* pl = gs_slab + (2 + p) * 512 + lane;
      int pc = 0, nc = 0;
      if (neg) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const u64x2 b = pl[i * 64];
          pc += __popcll(b.x & consider.w[i].x) + __popcll(b.y & consider.w[i].y);
          nc += __popcll(b.x & sign.w[i].x) + __popcll(b.y & sign.w[i].y);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const u64x2 b = pl[i * 64];
          pc += __popcll(b.x & consider.w[i].x) + __popcll(b.y & consider.w[i].y);
        }
      }
      acc_sum += int64_t(uint64_t(int64_t(pc - nc)) << (p0 + p));
    }
    const int64_t tsum = wave_sum_i64(acc_sum);
    const int64_t tcnt = wave_sum_i64(acc_cnt);
    if (lane == 0) {
      if (tsum) atomicAdd(out_sum + g, (unsigned long long)tsum);
      if (tcnt) atomicAdd(out_cnt + g, (unsigned long long)tcnt);
    }
  }
}

// ---------------------------------------------------------------- BSI range
// Bit-sliced comparators (O'Neil), reference fragment.go:1271-1534, with the
// exact control flow of pilosa_amd/models/fragment.py (_range_eq/_lt/_gt/
// _between).  One wave per (shard, key): the predicate result of that
// container is built in registers from the exists/sign/bit-slice tiles and
// written as a bitmap container of a temporary device view, which ordinary
// expression programs then consume as a leaf (Count(Intersect(Row(f=1),
// Row(v > 10))) = one range launch + one count launch).

// filt = filt & ~(filt & ~r & ~keep)   (reference: filt.Difference(filt.Difference(row).Difference(keep)))
__device__ __forceinline__ void keep_set_bits(Tile& f, const Tile& r, const Tile& k) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    f.w[i].x &= ~(f.w[i].x & ~r.w[i].x & ~k.w[i].x);
    f.w[i].y &= ~(f.w[i].y & ~r.w[i].y & ~k.w[i].y);
  }
}

// filt = filt & ~(r & ~keep)
__device__ __forceinline__ void drop_set_bits(Tile& f, const Tile& r, const Tile& k) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    f.w[i].x &= ~(r.w[i].x & ~k.w[i].x);
    f.w[i].y &= ~(r.w[i].y & ~k.w[i].y);
  }
}

__device__ void bsi_lt_unsigned(const BsiCtx& c, Tile& filt, int depth, uint64_t pred, bool allow_eq) {
  Tile keep, r;
  tile_zero(keep);
  bool leading = true;
  for (int i = depth - 1; i >= 0; i--) {
    bsi_bit(c, i, r);
    const int bit = int((pred >> i) & 1);
    if (leading) {
      if (bit == 0) {
        tile_op<OP_ANDNOT>(filt, r);
        continue;
      }
      leading = false;
    }
    if (i == 0 && !allow_eq) {
      if (bit == 0) {
        filt = keep;
        return;
      }
      drop_set_bits(filt, r, keep);
      return;
    }
    if (bit == 0) {
      drop_set_bits(filt, r, keep);
      continue;
    }
    if (i > 0) {
#pragma unroll
      for (int w = 0; w < 8; w++) {
        keep.w[w].x |= filt.w[w].x & ~r.w[w].x;
        keep.w[w].y |= filt.w[w].y & ~r.w[w].y;
      }
    }
  }
}

__device__ void bsi_gt_unsigned(const BsiCtx& c, Tile& filt, int depth, uint64_t pred, bool allow_eq) {
  Tile keep, r;
  tile_zero(keep);
  for (int i = depth - 1; i >= 0; i--) {
    bsi_bit(c, i, r);
    const int bit = int((pred >> i) & 1);
    if (i == 0 && !allow_eq) {
      if (bit == 1) {
        filt = keep;
        return;
      }
      keep_set_bits(filt, r, keep);
      return;
    }
    if (bit == 1) {
      keep_set_bits(filt, r, keep);
      continue;
    }
    if (i > 0) {
#pragma unroll
      for (int w = 0; w < 8; w++) {
        keep.w[w].x |= filt.w[w].x & r.w[w].x;
        keep.w[w].y |= filt.w[w].y & r.w[w].y;
      }
    }
  }
}

__device__ void bsi_between_unsigned(const BsiCtx& c, Tile& filt, int depth, uint64_t pmin, uint64_t pmax) {
  Tile keep1, keep2, r;
  tile_zero(keep1);
  tile_zero(keep2);
  for (int i = depth - 1; i >= 0; i--) {
    bsi_bit(c, i, r);
    const int b1 = int((pmin >> i) & 1), b2 = int((pmax >> i) & 1);
    if (b1 == 1) {
      keep_set_bits(filt, r, keep1);
    } else if (i > 0) {
#pragma unroll
      for (int w = 0; w < 8; w++) {
        keep1.w[w].x |= filt.w[w].x & r.w[w].x;
        keep1.w[w].y |= filt.w[w].y & r.w[w].y;
      }
    }
    if (b2 == 0) {
      drop_set_bits(filt, r, keep2);
    } else if (i > 0) {
#pragma unroll
      for (int w = 0; w < 8; w++) {
        keep2.w[w].x |= filt.w[w].x & ~r.w[w].x;
        keep2.w[w].y |= filt.w[w].y & ~r.w[w].y;
      }
    }
  }
}

// op: 0 EQ, 1 NEQ, 2 LT, 3 LTE, 4 GT, 5 GTE, 6 BETWEEN(p1..p2), 7 NOT NULL
// OPC: the comparison as a template constant, so each instantiation keeps only
// its own path's tiles live (the runtime switch over every op held 256 VGPRs,
// one wave per SIMD).  ``op_rt`` is unused (kept for the launcher's signature).
template <int OPC>
__global__ __launch_bounds__(256, 2) void bsi_range_kernel(const ViewDev* __restrict__ views, int S, BsiArgs bsi,
                                                        int op_rt, int64_t p1, int64_t p2,
                                                        uint16_t* __restrict__ out_payload,
                                                        int64_t* __restrict__ out_meta,
                                                        unsigned long long* __restrict__ out_count) {
  __shared__ WaveScratch scratch[WAVES_PER_BLOCK];
  const uint32_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const int64_t item = int64_t(blk) * WAVES_PER_BLOCK + wave;
  const bool live = item < int64_t(S) * 16;
  if (!live && !out_count) return;  // (the count path's block barrier needs every wave)
  const int64_t it = live ? item : 0;
  const int s = int(it >> 4), j = int(it & 15);
  const ViewDev& bv = views[bsi.view];
  BsiCtx c{bsi, bv, s, j, bv.shard_base[s], bv.rowptr + int64_t(s) * (bv.D + 1), scratch[wave].lb};
  plane_index(c);
  const int depth = bsi.depth;
  constexpr int op = OPC;
  (void)op_rt;
  Tile b, sign, res;
  bsi_row(c, bsi.row_exists, b);
  bsi_row(c, bsi.row_sign, sign);
  if (op == 7) {
    res = b;
  } else if (op == 0 || op == 1) {
    Tile eq = b, r;
    const uint64_t up = uint64_t(p1 < 0 ? -p1 : p1);
    if (p1 < 0) tile_op<OP_AND>(eq, sign);
    else tile_op<OP_ANDNOT>(eq, sign);
    for (int i = depth - 1; i >= 0; i--) {
      bsi_bit(c, i, r);
      if ((up >> i) & 1) tile_op<OP_AND>(eq, r);
      else tile_op<OP_ANDNOT>(eq, r);
    }
    res = b;
    if (op == 1) tile_op<OP_ANDNOT>(res, eq);
    else res = eq;
  } else if (op == 2 || op == 3) {
    const bool allow = op == 3;
    const uint64_t up = uint64_t(p1 < 0 ? -p1 : p1);
    if ((p1 >= 0 && allow) || (p1 >= -1 && !allow)) {
      Tile pos = b;
      tile_op<OP_ANDNOT>(pos, sign);
      bsi_lt_unsigned(c, pos, depth, up, allow);
      res = sign;
      tile_or(res, pos);
    } else {
      res = b;
      tile_op<OP_AND>(res, sign);
      bsi_gt_unsigned(c, res, depth, up, allow);
    }
  } else if (op == 4 || op == 5) {
    const bool allow = op == 5;
    const uint64_t up = uint64_t(p1 < 0 ? -p1 : p1);
    if ((p1 >= 0 && allow) || (p1 >= -1 && !allow)) {
      res = b;
      tile_op<OP_ANDNOT>(res, sign);
      bsi_gt_unsigned(c, res, depth, up, allow);
    } else {
      Tile neg = b;
      tile_op<OP_AND>(neg, sign);
      res = b;   // the positives, taken before the descent so b and sign are dead during it
      tile_op<OP_ANDNOT>(res, sign);
      bsi_lt_unsigned(c, neg, depth, up, allow);
      tile_or(res, neg);
    }
  } else {  // between
    const uint64_t umin = uint64_t(p1 < 0 ? -p1 : p1), umax = uint64_t(p2 < 0 ? -p2 : p2);
    if (p1 >= 0) {
      res = b;
      tile_op<OP_ANDNOT>(res, sign);
      bsi_between_unsigned(c, res, depth, umin, umax);
    } else if (p2 < 0) {
      res = b;
      tile_op<OP_AND>(res, sign);
      bsi_between_unsigned(c, res, depth, umax, umin);
    } else {
      Tile pos = b, neg = b;
      tile_op<OP_ANDNOT>(pos, sign);
      tile_op<OP_AND>(neg, sign);
      bsi_lt_unsigned(c, pos, depth, umax, true);
      bsi_lt_unsigned(c, neg, depth, umin, true);
      res = pos;
      tile_or(res, neg);
    }
  }
  const int64_t n = wave_sum_i64(tile_popc(res));
  if (out_count) {  // Count(Row(v <op> x)): no predicate view is written
    // the block's waves fold into one atomic: every wave of the launch
    // adding to the same word serialises at one L2 channel
    // (through each wave's own scratch word 0, free by now: no extra LDS)
    if (lane == 0) scratch[wave].lb[0] = live ? uint64_t(n) : 0ull;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long t = 0;
      for (int w = 0; w < WAVES_PER_BLOCK; w++) t += scratch[w].lb[0];
      if (t) atomicAdd(out_count, t);
    }
    return;
  }
  ulong2* dst = reinterpret_cast<ulong2*>(out_payload + item * 4096);
#pragma unroll
  for (int i = 0; i < 8; i++) dst[i * 64 + lane] = res.w[i];
  if (lane == 0) out_meta[item] = int64_t(j) | (int64_t(CT_BITMAP) << 4) | (n << 6) | ((item * 512) << 23);
}

// ---------------------------------------------------------------- BSI min/max
// Per (shard, key) MSB-first descents (reference fragment.go:1145-1225):
// consider = exists & filter; for Min the max-magnitude negative and the
// unsigned minimum of the positives, for Max the unsigned maximum of the
// positives and the minimum magnitude of the negatives.  out[item] = 4 x
// (value, count); the host folds keys into shard results exactly as one
// shard-wide descent would (the key sets partition the shard).  WHICH = 1
// (Min) runs only maxU(neg) / minU(pos), 2 (Max) only maxU(pos) / minU(neg):
// half the tiles, popcounts and wave reductions per bit (0 = all four).
template <int WHICH, int MINW = 2>
__global__ __launch_bounds__(256, MINW) void bsi_minmax_kernel(const QueryProg* __restrict__ progs,
                                                         const ViewDev* __restrict__ views, int S, BsiArgs bsi,
                                                         int64_t* __restrict__ out) {
  __shared__ WaveScratch scratch[WAVES_PER_BLOCK];
  const uint32_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const int64_t item = int64_t(blk) * WAVES_PER_BLOCK + wave;
  if (item >= int64_t(S) * 16) return;
  const int s = int(item >> 4), j = int(item & 15);
  const ViewDev& bv = views[bsi.view];
  WaveScratch& ws = scratch[wave];
  BsiCtx c{bsi, bv, s, j, bv.shard_base[s], bv.rowptr + int64_t(s) * (bv.D + 1), ws.lb};
  plane_index(c);
  const int depth = bsi.depth;
  const QueryProg& qp = progs[0];
  Tile pos, neg;
  bsi_row(c, bsi.row_exists, pos);
  if (qp.nprog) {
    uint32_t mask[MAXLEAF];
    build_slots(qp, views, s, ws, mask);
    Tile f;
    if ((candidate_mask(qp, mask) >> j) & 1) eval_tile(qp, views, s, j, ws, f);
    else tile_zero(f);
    tile_op<OP_AND>(pos, f);
  }
  {
    Tile sign;
    bsi_row(c, bsi.row_sign, sign);
    neg = pos;
    tile_op<OP_AND>(neg, sign);
    tile_op<OP_ANDNOT>(pos, sign);
  }
  // counted first, so pos / neg are dead once the descents' tiles take them
  const int64_t npos = wave_sum_i64(tile_popc(pos)), nneg = wave_sum_i64(tile_popc(neg));
  // four descents share each bit-slice load: maxU(neg), minU(pos), maxU(pos), minU(neg)
  Tile fmaxn = neg, fminp = pos, fmaxp = pos, fminn = neg, r;
  int64_t vmaxn = 0, vminp = 0, vmaxp = 0, vminn = 0;
  int64_t cmaxn = 0, cminp = 0, cmaxp = 0, cminn = 0;
  for (int i = depth - 1; i >= 0; i--) {
    bsi_bit(c, i, r);
    Tile t;
    int64_t k;
    if (WHICH != 2) {  // maxU(neg)
      t = fmaxn;
      tile_op<OP_AND>(t, r);
      k = wave_sum_i64(tile_popc(t));
      if (k > 0) { vmaxn |= int64_t(1) << i; fmaxn = t; cmaxn = k; }
      else if (i == 0) cmaxn = wave_sum_i64(tile_popc(fmaxn));
    }
    if (WHICH != 1) {  // maxU(pos)
      t = fmaxp;
      tile_op<OP_AND>(t, r);
      k = wave_sum_i64(tile_popc(t));
      if (k > 0) { vmaxp |= int64_t(1) << i; fmaxp = t; cmaxp = k; }
      else if (i == 0) cmaxp = wave_sum_i64(tile_popc(fmaxp));
    }
    if (WHICH != 2) {  // minU(pos)
      t = fminp;
      tile_op<OP_ANDNOT>(t, r);
      k = wave_sum_i64(tile_popc(t));
      if (k > 0) { fminp = t; cminp = k; }
      else { vminp += int64_t(1) << i; if (i == 0) cminp = wave_sum_i64(tile_popc(fminp)); }
    }
    if (WHICH != 1) {  // minU(neg)
      t = fminn;
      tile_op<OP_ANDNOT>(t, r);
      k = wave_sum_i64(tile_popc(t));
      if (k > 0) { fminn = t; cminn = k; }
      else { vminn += int64_t(1) << i; if (i == 0) cminn = wave_sum_i64(tile_popc(fminn)); }
    }
  }
  if (lane == 0) {
    int64_t* o = out + item * 10;
    o[0] = vmaxn; o[1] = cmaxn; o[2] = vminp; o[3] = cminp;
    o[4] = vmaxp; o[5] = cmaxp; o[6] = vminn; o[7] = cminn;
    o[8] = npos; o[9] = nneg;
  }
}

// ---------------------------------------------------------------- BSI k-th value
// Percentile(field=, nth=): the k-th smallest value of exists & filter, exact.
// An MSB-first descent like Min / Max, but the branch taken at each bit
// depends on the counts of ALL (shard, key) items, so it is one launch per
// bit: the launch boundary is the grid-wide barrier.  One wave owns one item;
// its candidate container lives between launches in a dense buffer
// cand[S*16][1024].  No launch reads a word it writes: the step for bit i adds
// to cnt1[i] only and reads cnt1[depth-1 .. i+1], which earlier launches of
// the same stream finished.

// the block's four waves fold into one atomic per counter (every wave of the
// launch adding to one word serialises at one L2 channel); slot: a free LDS
// word per wave.  Every wave of the block must call it.
__device__ __forceinline__ void kth_block_add(uint64_t* slot, int stride, uint64_t v0, uint64_t v1,
                                              unsigned long long* out0, unsigned long long* out1) {
  if (wave_lane() == 0) {
    slot[0] = v0;
    slot[1] = v1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t a = 0, b = 0;
    const uint64_t* base = slot;  // wave 0's slot
    for (int w = 0; w < WAVES_PER_BLOCK; w++) {
      a += base[w * stride];
      b += base[w * stride + 1];
    }
    if (a) atomicAdd(out0, (unsigned long long)a);
    if (b && out1) atomicAdd(out1, (unsigned long long)b);
  }
}

__global__ __launch_bounds__(256, 2) void bsi_kth_init_kernel(const QueryProg* __restrict__ progs,
                                                              const ViewDev* __restrict__ views, int S, BsiArgs bsi,
                                                              uint64_t* __restrict__ cand,
                                                              unsigned long long* __restrict__ cnt) {
  __shared__ WaveScratch scratch[WAVES_PER_BLOCK];
  const uint32_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const int64_t item = int64_t(blk) * WAVES_PER_BLOCK + wave;
  const bool live = item < int64_t(S) * 16;  // (the block barrier below needs every wave)
  uint64_t n = 0, nneg = 0;
  if (live) {
    const int s = int(item >> 4), j = int(item & 15);
    const ViewDev& bv = views[bsi.view];
    WaveScratch& ws = scratch[wave];
    BsiCtx c{bsi, bv, s, j, bv.shard_base[s], bv.rowptr + int64_t(s) * (bv.D + 1), ws.lb};
    const QueryProg& qp = progs[0];
    Tile t;
    bsi_row(c, bsi.row_exists, t);
    if (qp.nprog) {
      uint32_t mask[MAXLEAF];
      build_slots(qp, views, s, ws, mask);
      Tile f;
      if ((candidate_mask(qp, mask) >> j) & 1) eval_tile(qp, views, s, j, ws, f);
      else tile_zero(f);
      tile_op<OP_AND>(t, f);
    }
    ulong2* dst = reinterpret_cast<ulong2*>(cand + item * 1024);
#pragma unroll
    for (int i = 0; i < 8; i++) dst[i * 64 + lane] = t.w[i];
    n = uint64_t(wave_sum_i64(tile_popc(t)));
    Tile sign;
    bsi_row(c, bsi.row_sign, sign);
    tile_op<OP_AND>(t, sign);
    nneg = uint64_t(wave_sum_i64(tile_popc(t)));
  }
  kth_block_add(scratch[wave].lb, int(sizeof(WaveScratch) / sizeof(uint64_t)), n, nneg, cnt, cnt + 1);
}

__global__ __launch_bounds__(256) void bsi_kth_step_kernel(const ViewDev* __restrict__ views, int S, BsiArgs bsi,
                                                           uint64_t* __restrict__ cand, unsigned long long* cnt,
                                                           int i, uint64_t r, uint64_t tot, int largest_first) {
  __shared__ uint64_t lbs[WAVES_PER_BLOCK][1024];
  const uint32_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int lane = wave_lane();
  const int64_t item = int64_t(blk) * WAVES_PER_BLOCK + wave;
  const bool live = item < int64_t(S) * 16;
  const int depth = bsi.depth;
  uint64_t c1 = 0;
  if (live) {
    const int s = int(item >> 4), j = int(item & 15);
    const ViewDev& bv = views[bsi.view];
    // (only planes i and i + 1 are read: each is found as bsi_row finds the
    // exists row, without plane_index's walk over every plane)
    BsiCtx c{bsi, bv, s, j, bv.shard_base[s], bv.rowptr + int64_t(s) * (bv.D + 1), lbs[wave]};
    ulong2* cp = reinterpret_cast<ulong2*>(cand + item * 1024);
    Tile t, p;
#pragma unroll
    for (int w = 0; w < 8; w++) t.w[w] = cp[w * 64 + lane];
    if (i == depth - 1) {
      bsi_row(c, bsi.row_sign, p);
      if (largest_first) tile_op<OP_AND>(t, p);
      else tile_op<OP_ANDNOT>(t, p);
    } else {
      // the decision on bit i + 1: the chain over the counts of the finished launches
      int bit = 0;
      for (int b = depth - 1; b > i; b--) bit = kth_chain(largest_first, cnt[2 + b], r, tot);
      bsi_row(c, bsi.bit_row[i + 1], p);
      if (bit) tile_op<OP_AND>(t, p);
      else tile_op<OP_ANDNOT>(t, p);
    }
    if (i > 0) {  // (nothing reads the candidates after the last bit's step)
#pragma unroll
      for (int w = 0; w < 8; w++) cp[w * 64 + lane] = t.w[w];
    }
    bsi_row(c, bsi.bit_row[i], p);
    tile_op<OP_AND>(t, p);
    c1 = uint64_t(wave_sum_i64(tile_popc(t)));
  }
  kth_block_add(lbs[wave], 1024, c1, 0, cnt + 2 + i, nullptr);
}

// Fold of the per-key descents into the call's ONE (value, count), on the
// device (one small D2H instead of the [S, 16, 10] table): per fragment (its
// G = 16 * sub-shards keys) fragment.min/max's sign rules -- Min: the largest
// |negative| if any negative, else the smallest positive; Max: the largest
// positive if any, else the smallest |negative| (fragment.go:1145-1225) --
// with the counts of every key holding that value summed; across fragments
// the extreme, counted in the FIRST fragment holding it (executor.go
// ValCount.Smaller / Larger keep the earlier shard's).  One 1024-thread block;
// out = {value, count, found}.
constexpr int FOLD_THREADS = 1024;
// GT: the keys per fragment as a compile-time constant (16: every key's
// loads issue together -- the runtime-G loop serialised them, 44 us per call)
// or 0 (runtime G, wide shards)
template <int GT>
__global__ __launch_bounds__(FOLD_THREADS) void bsi_minmax_fold_kernel(const int64_t* __restrict__ o, int F, int Grt,
                                                                      int is_min, int64_t* __restrict__ out) {
  const int G = GT > 0 ? GT : Grt;
  __shared__ int64_t sv[FOLD_THREADS / 64];
  __shared__ int sf[FOLD_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t BIG = 0x7fffffffffffffffLL;
  // this thread's best (value, fragment) over its fragments; key = value
  // for Min, -value for Max (smaller key wins; ties: lower fragment)
  int64_t bkey = BIG, bval = 0, bcnt = 0;
  int bfrag = 0x7fffffff;
  if (GT == 16) {
    // 16 lanes per fragment, lane g on key g: its 10 words are 5 coalesced
    // 16-byte loads (a thread per fragment striding 80 bytes per key touched
    // 64 cache lines per load instruction: 47 us per call), two fragments
    // per group in flight; the group's extreme and count by shuffles
    const int g = tid & 15;
    auto fold = [&](const longlong2 w0, const longlong2 w1, const longlong2 w2, const longlong2 w3,
                    const longlong2 w4, const int f) {
      const bool live = f < F;
      const bool anyp = (uint64_t(__ballot(live && w4.x > 0)) >> (lane & 48)) & 0xFFFFu;
      const bool anyn = (uint64_t(__ballot(live && w4.y > 0)) >> (lane & 48)) & 0xFFFFu;
      if (!anyp && !anyn) return;  // group-uniform
      const bool use_neg = is_min ? anyn : !anyp;
      const int vc = is_min ? (anyn ? 0 : 2) : (anyp ? 4 : 6);
      const bool largest = vc == 0 || vc == 4;
      const bool valid = (use_neg ? w4.y : w4.x) > 0;
      const longlong2 xc = vc == 0 ? w0 : vc == 2 ? w1 : vc == 4 ? w2 : w3;  // (value, count)
      int64_t best = valid ? int64_t(xc.x) : (largest ? int64_t(-1) : BIG);
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) {
        const int64_t b2 = __shfl_xor(best, off, 64);
        best = largest ? (b2 > best ? b2 : best) : (b2 < best ? b2 : best);
      }
      int64_t cnt = valid && int64_t(xc.x) == best ? int64_t(xc.y) : 0;
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
      const int64_t val = use_neg ? -best : best;
      const int64_t key = is_min ? val : -val;
      if (g == 0 && (key < bkey || (key == bkey && f < bfrag))) { bkey = key; bval = val; bcnt = cnt; bfrag = f; }
    };
    const int grp = tid >> 4;  // 64 groups
    for (int f0 = grp; f0 < F; f0 += 2 * (FOLD_THREADS / 16)) {
      const int f1 = f0 + FOLD_THREADS / 16;
      const longlong2* e0 = reinterpret_cast<const longlong2*>(o + (int64_t(f0) * 16 + g) * 10);
      const longlong2* e1 = reinterpret_cast<const longlong2*>(o + (int64_t(f1 < F ? f1 : f0) * 16 + g) * 10);
      const longlong2 a0 = e0[0], a1 = e0[1], a2 = e0[2], a3 = e0[3], a4 = e0[4];
      const longlong2 b0 = e1[0], b1 = e1[1], b2 = e1[2], b3 = e1[3], b4 = e1[4];
      fold(a0, a1, a2, a3, a4, f0);
      fold(b0, b1, b2, b3, b4, f1);
    }
  } else
  for (int f = tid; f < F; f += FOLD_THREADS) {
    const int64_t* e = o + int64_t(f) * G * 10;
    bool anyp = false, anyn = false;
#pragma unroll
    for (int g = 0; g < G; g++) {
      anyp |= e[g * 10 + 8] > 0;
      anyn |= e[g * 10 + 9] > 0;
    }
    if (!anyp && !anyn) continue;
    // column pair and sign of the fragment's candidate: Min: neg -> max |neg| (0/1),
    // else min pos (2/3); Max: pos -> max pos (4/5), else min |neg| (6/7)
    const bool use_neg = is_min ? anyn : !anyp;
    const int vc = is_min ? (anyn ? 0 : 2) : (anyp ? 4 : 6);
    const bool largest = vc == 0 || vc == 4;
    const int mcol = use_neg ? 9 : 8;
    int64_t best = largest ? -1 : BIG, cnt = 0;
#pragma unroll
    for (int g = 0; g < G; g++) {
      if (e[g * 10 + mcol] <= 0) continue;
      const int64_t v = e[g * 10 + vc];
      if (largest ? v > best : v < best) { best = v; cnt = 0; }
      if (v == best) cnt += e[g * 10 + vc + 1];
    }
    const int64_t val = use_neg ? -best : best;
    const int64_t key = is_min ? val : -val;
    if (key < bkey || (key == bkey && f < bfrag)) { bkey = key; bval = val; bcnt = cnt; bfrag = f; }
  }
  // block argmin of (key, fragment): wave shuffles, then LDS across waves
  int64_t k = bkey;
  int fr = bfrag;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int64_t k2 = __shfl_xor(k, off, 64);
    const int f2 = __shfl_xor(fr, off, 64);
    if (k2 < k || (k2 == k && f2 < fr)) { k = k2; fr = f2; }
  }
  if (lane == 0) { sv[wave] = k; sf[wave] = fr; }
  __syncthreads();
  if (wave == 0) {
    k = lane < FOLD_THREADS / 64 ? sv[lane] : BIG;
    fr = lane < FOLD_THREADS / 64 ? sf[lane] : 0x7fffffff;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int64_t k2 = __shfl_xor(k, off, 64);
      const int f2 = __shfl_xor(fr, off, 64);
      if (k2 < k || (k2 == k && f2 < fr)) { k = k2; fr = f2; }
    }
    if (lane == 0) { sv[0] = k; sf[0] = fr; }
  }
  __syncthreads();
  // the owner of the winning fragment writes it (vector stores)
  if (sf[0] == bfrag && bfrag != 0x7fffffff && sv[0] == bkey) {
    out[0] = bval;
    out[1] = bcnt;
    out[2] = 1;
  } else if (tid == 0 && sf[0] == 0x7fffffff) {
    out[0] = 0;
    out[1] = 0;
    out[2] = 0;
  }
}

// Multi-block fold (16 keys per fragment): block b takes fragments
// 64 b .. 64 b + 63, one per 16-lane group (the same per-fragment rules as
// bsi_minmax_fold_kernel), and writes its winner as part[4 b ..] = {key,
// value, count, fragment} (key = value for Min, -value for Max; BIG = none).
__global__ __launch_bounds__(FOLD_THREADS) void bsi_minmax_fold_part_kernel(const int64_t* __restrict__ o, int F,
                                                                           int is_min, int64_t* __restrict__ part) {
  __shared__ int64_t sv[FOLD_THREADS / 64];
  __shared__ int sf[FOLD_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = tid & 15;
  const int64_t BIG = 0x7fffffffffffffffLL;
  const int f = int(blockIdx.x) * (FOLD_THREADS / 16) + (tid >> 4);
  const longlong2* e = reinterpret_cast<const longlong2*>(o + (int64_t(f < F ? f : 0) * 16 + g) * 10);
  const longlong2 w0 = e[0], w1 = e[1], w2 = e[2], w3 = e[3], w4 = e[4];
  const bool live = f < F;
  const bool anyp = (uint64_t(__ballot(live && w4.x > 0)) >> (lane & 48)) & 0xFFFFu;
  const bool anyn = (uint64_t(__ballot(live && w4.y > 0)) >> (lane & 48)) & 0xFFFFu;
  int64_t key = BIG, val = 0, cnt = 0;
  if (anyp || anyn) {  // group-uniform
    const bool use_neg = is_min ? anyn : !anyp;
    const int vc = is_min ? (anyn ? 0 : 2) : (anyp ? 4 : 6);
    const bool largest = vc == 0 || vc == 4;
    const bool valid = (use_neg ? w4.y : w4.x) > 0;
    const longlong2 xc = vc == 0 ? w0 : vc == 2 ? w1 : vc == 4 ? w2 : w3;
    int64_t best = valid ? int64_t(xc.x) : (largest ? int64_t(-1) : BIG);
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
      const int64_t b2 = __shfl_xor(best, off, 64);
      best = largest ? (b2 > best ? b2 : best) : (b2 < best ? b2 : best);
    }
    int64_t c = valid && int64_t(xc.x) == best ? int64_t(xc.y) : 0;
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    val = use_neg ? -best : best;
    key = is_min ? val : -val;
    cnt = c;
  }
  // block argmin of (key, fragment) over the groups' lane 0
  int64_t k = g == 0 ? key : BIG;
  int fr = g == 0 && key != BIG ? f : 0x7fffffff;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int64_t k2 = __shfl_xor(k, off, 64);
    const int f2 = __shfl_xor(fr, off, 64);
    if (k2 < k || (k2 == k && f2 < fr)) { k = k2; fr = f2; }
  }
  if (lane == 0) { sv[wave] = k; sf[wave] = fr; }
  __syncthreads();
  if (wave == 0) {
    k = lane < FOLD_THREADS / 64 ? sv[lane] : BIG;
    fr = lane < FOLD_THREADS / 64 ? sf[lane] : 0x7fffffff;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int64_t k2 = __shfl_xor(k, off, 64);
      const int f2 = __shfl_xor(fr, off, 64);
      if (k2 < k || (k2 == k && f2 < fr)) { k = k2; fr = f2; }
    }
    if (lane == 0) { sv[0] = k; sf[0] = fr; }
  }
  __syncthreads();
  int64_t* pb = part + int64_t(blockIdx.x) * 4;
  if (sf[0] == 0x7fffffff) {
    if (tid == 0) { pb[0] = BIG; pb[1] = 0; pb[2] = 0; pb[3] = 0x7fffffff; }
  } else if (g == 0 && f == sf[0] && key == sv[0]) {
    pb[0] = key; pb[1] = val; pb[2] = cnt; pb[3] = f;
  }
}

// The blocks' winners -> out = {value, count, found}: smallest key, ties to
// the lower fragment (the first shard holding the extreme).
__global__ __launch_bounds__(256) void bsi_minmax_fold_final_kernel(const int64_t* __restrict__ part, int nb,
                                                                   int64_t* __restrict__ out) {
  __shared__ int64_t sk[4], sv[4], sc[4];
  __shared__ int sfr[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t BIG = 0x7fffffffffffffffLL;
  int64_t k = BIG, v = 0, c = 0;
  int fr = 0x7fffffff;
  for (int b = tid; b < nb; b += 256) {
    const int64_t k2 = part[int64_t(b) * 4], f2 = part[int64_t(b) * 4 + 3];
    if (k2 < k || (k2 == k && int(f2) < fr)) {
      k = k2; fr = int(f2); v = part[int64_t(b) * 4 + 1]; c = part[int64_t(b) * 4 + 2];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int64_t k2 = __shfl_xor(k, off, 64), v2 = __shfl_xor(v, off, 64), c2 = __shfl_xor(c, off, 64);
    const int f2 = __shfl_xor(fr, off, 64);
    if (k2 < k || (k2 == k && f2 < fr)) { k = k2; fr = f2; v = v2; c = c2; }
  }
  if (lane == 0) { sk[wave] = k; sv[wave] = v; sc[wave] = c; sfr[wave] = fr; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; w++)
      if (sk[w] < k || (sk[w] == k && sfr[w] < fr)) { k = sk[w]; fr = sfr[w]; v = sv[w]; c = sc[w]; }
    const bool found = fr != 0x7fffffff;
    out[0] = found ? v : 0;
    out[1] = found ? c : 0;
    out[2] = found ? 1 : 0;
  }
}

// ------------------------------------------------------------ launchers

void launch_bsi_range(const ViewDev* views, int S, BsiArgs bsi, int op, int64_t p1, int64_t p2, uint16_t* out_payload,
                      int64_t* out_meta, unsigned long long* out_count, hipStream_t st) {
  const int64_t items = int64_t(S) * 16;
  if (items == 0) return;
  const dim3 grid(grid_for(items)), block(64 * WAVES_PER_BLOCK);
#define PK_RANGE(OPV)                                                                                       \
  case OPV:                                                                                                 \
    hipLaunchKernelGGL(bsi_range_kernel<OPV>, grid, block, 0, st, views, S, bsi, op, p1, p2, out_payload,  \
                       out_meta, out_count);                                                                \
    break;
  switch (op) {
    PK_RANGE(0) PK_RANGE(1) PK_RANGE(2) PK_RANGE(3) PK_RANGE(4) PK_RANGE(5) PK_RANGE(6) PK_RANGE(7)
    default: break;
  }
#undef PK_RANGE
}

void launch_bsi_minmax(const QueryProg* progs, const ViewDev* views, int S, BsiArgs bsi, int64_t* out,
                       hipStream_t st, int which) {
  const int64_t items = int64_t(S) * 16;
  if (items == 0) return;
  const dim3 grid(grid_for(items)), block(64 * WAVES_PER_BLOCK);
  // 2 waves per SIMD; 3 (168 VGPRs, 224 B of spills) measured the same
  // (1.29 vs 1.31 ms per Min, profiles/r04_u/)
  if (which == 1)
    hipLaunchKernelGGL((bsi_minmax_kernel<1, 2>), grid, block, 0, st, progs, views, S, bsi, out);
  else if (which == 2)
    hipLaunchKernelGGL((bsi_minmax_kernel<2, 2>), grid, block, 0, st, progs, views, S, bsi, out);
  else
    hipLaunchKernelGGL((bsi_minmax_kernel<0, 2>), grid, block, 0, st, progs, views, S, bsi, out);
}

void launch_bsi_kth_init(const QueryProg* progs, const ViewDev* views, int S, BsiArgs bsi, uint64_t* cand,
                         unsigned long long* cnt, hipStream_t st) {
  const int64_t items = int64_t(S) * 16;
  if (items == 0) return;
  hipLaunchKernelGGL(bsi_kth_init_kernel, dim3(grid_for(items)), dim3(64 * WAVES_PER_BLOCK), 0, st, progs, views, S,
                     bsi, cand, cnt);
}

void launch_bsi_kth_step(const ViewDev* views, int S, BsiArgs bsi, uint64_t* cand, unsigned long long* cnt, int i,
                         uint64_t r, uint64_t tot, int largest_first, hipStream_t st) {
  const int64_t items = int64_t(S) * 16;
  if (items == 0 || i < 0 || i >= bsi.depth) return;
  hipLaunchKernelGGL(bsi_kth_step_kernel, dim3(grid_for(items)), dim3(64 * WAVES_PER_BLOCK), 0, st, views, S, bsi,
                     cand, cnt, i, r, tot, largest_first);
}

void launch_bsi_minmax_fold(const int64_t* o, int F, int G, int is_min, int64_t* out, int64_t* part,
                            hipStream_t st) {
  if (G == 16 && part && F > FOLD_THREADS / 16) {
    // one fragment per 16-lane group over ceil(F / 64) blocks, then the
    // blocks' winners (one load round trip each instead of ~8 in one block)
    const int nb = (F + FOLD_THREADS / 16 - 1) / (FOLD_THREADS / 16);
    hipLaunchKernelGGL(bsi_minmax_fold_part_kernel, dim3(nb), dim3(FOLD_THREADS), 0, st, o, F, is_min, part);
    hipLaunchKernelGGL(bsi_minmax_fold_final_kernel, dim3(1), dim3(256), 0, st, part, nb, out);
  } else if (G == 16) {
    hipLaunchKernelGGL(bsi_minmax_fold_kernel<16>, dim3(1), dim3(FOLD_THREADS), 0, st, o, F, G, is_min, out);
  } else {
    hipLaunchKernelGGL(bsi_minmax_fold_kernel<0>, dim3(1), dim3(FOLD_THREADS), 0, st, o, F, G, is_min, out);
  }
}

void launch_bsi_sum(const QueryProg* progs, int Q, const ViewDev* views, int S, BsiArgs bsi,
                    unsigned long long* out_sum, unsigned long long* out_cnt, int fmode, hipStream_t st) {
  const int64_t items = int64_t(Q) * S * 16;
  if (items == 0) return;
  const dim3 grid(grid_for(items)), block(64 * WAVES_PER_BLOCK);
  if (fmode == 0)
    hipLaunchKernelGGL(bsi_sum_keys_kernel<0>, grid, block, 0, st, progs, Q, views, S, bsi, out_sum, out_cnt);
  else if (fmode == 1)
    hipLaunchKernelGGL(bsi_sum_keys_kernel<1>, grid, block, 0, st, progs, Q, views, S, bsi, out_sum, out_cnt);
  else
    hipLaunchKernelGGL(bsi_sum_keys_kernel<2>, grid, block, 0, st, progs, Q, views, S, bsi, out_sum, out_cnt);
}

int launch_bsi_group_sum(const QueryProg* progs, int G, const ViewDev* views, int S, BsiArgs bsi, int planes,
                         int gchunk, int fmode, unsigned long long* out_sum, unsigned long long* out_cnt,
                         hipStream_t st) {
  if (G <= 0 || S <= 0) return 0;
  planes = planes < 1 ? 1 : (planes > GS_MAX_PLANES ? GS_MAX_PLANES : planes);
  if (bsi.depth < 1) planes = 1;
  else if (planes > bsi.depth) planes = bsi.depth;
  const int nslab = bsi.depth > 0 ? (bsi.depth + planes - 1) / planes : 1;
  gchunk = gchunk < 1 ? 1 : gchunk;
  const int nchunk = (G + gchunk - 1) / gchunk;
  const int64_t blocks = int64_t(S) * 16 * nslab * nchunk;
  if (blocks >= (int64_t(1) << 31)) return -1;
  const int lds = (2 + planes) * 8192;
  const dim3 grid{unsigned(blocks)}, block(64 * WAVES_PER_BLOCK);
  if (fmode == 1) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(bsi_group_sum_kernel<1>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(bsi_group_sum_kernel<1>, grid, block, lds, st, progs, G, views, S, bsi, planes, nslab, gchunk,
                       nchunk, out_sum, out_cnt);
  } else {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(bsi_group_sum_kernel<2>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(bsi_group_sum_kernel<2>, grid, block, lds, st, progs, G, views, S, bsi, planes, nslab, gchunk,
                       nchunk, out_sum, out_cnt);
  }
  return nslab;
}

}  // namespace pk
