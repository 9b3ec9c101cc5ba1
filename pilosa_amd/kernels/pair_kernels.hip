// Count(Intersect(Row(a), Row(b))) for a batch of queries, organised around
// container keys instead of (query, shard) work items.
//
// Why a separate path: in the headline workload ~70 % of container pairs are
// array&array (~1.1k values each), 26 % array&bitmap.  The generic kernel
// walks the <=16 keys of one (query, shard) sequentially, so every container
// costs two dependent global round trips (meta -> payload) and a wave never
// has more than one container in flight; it also streams each row once per
// query, although in a Zipf batch every hot row is read by many queries.
//
// Here the work is split in two launches:
//   K1 pair_build   one thread per (shard, query): resolves both rows' CSR
//                   ranges, derives the key-presence masks (no meta loads for
//                   full rows) and writes the matching container index pair
//                   for every key j to pairs[(s*16 + j) * Q + q].
//   K2 and2_pairs   one wave per (shard, key, chunk of CQ queries).  The
//                   batch is sorted on the host by (hot row, other row), so
//                   consecutive queries in a chunk usually share row a: the
//                   wave stages a's container ONCE into its 8 KiB LDS bitmap
//                   and only streams b's container per query.  Waves of one
//                   (shard, key) unit are consecutive and XCD-remapped onto
//                   one XCD, so the unit's containers (~1.3 MB) live in that
//                   XCD's 4 MB L2 while all its chunks run.
// Per-(unit, query) counts go to an int32 partial buffer that torch reduces
// (deterministic, no contended atomics).
//
// The kernel is v6: one wave per workgroup (LDS bitmap at address 0), the
// next pair's B head prefetched while the current pair is counted.  It is built
// in three shapes: plain (variant 6), with batched array staging for
// serving-size batches (BST, variant 39) and with bitmap twins (TWN, variant
// 63).  Per 4096-query batch on the 954-shard index (profiles/r02_pairs/,
// r03_pairs/): round 1 29.4 ms; branch-free 8-probe chunks 21.7 ms; 1 wave per
// workgroup 18.1 ms; + B-head prefetch 16.9 ms.  Occupancy: 20 waves/CU (8 KiB
// LDS and 84 VGPRs per wave); padding LDS to 16 / 12 waves/CU measured 17.9 /
// 23.3 ms against 16.7 (profiles/r03_occ/), so sharing one bitmap between two
// waves to reach 32 waves/CU would buy well under the 12->16 step.
// Per-pair budget at that occupancy, from cost-isolation skeletons
// (profiles/r05_pairs/): control 13 %, wave_sum 5 %, B-head loads 27 %,
// staging 19 %, counting 38 %; the control skeleton alone spends 4.6 of its
// 7.5 ms waiting on the B heads.
//
// History: measured and rejected.  None of this code is in the file any more;
// all of it is in git history before the commit that retired it (until then
// the kernel carried a template flag per experiment -- APF, DBG, SB, PD, ONE,
// SHD, ROT, UNS -- and the variants were built into the PK_KBENCH module).
// Numbers are ms per 4096-query headline batch against the v6 of their day
// (16.7-16.9, later 16.3) unless they say otherwise.
//   v2/v3 register-pipelined operands, v1/v4/v5 multi-wave workgroups.
//   v7 size-class lane groups with per-run staging: 18.5 (lower occupancy,
//     probes unchanged).
//   v8 lane-interleaved u16 probes: 24.0 (5x the load instructions although
//     LDS conflicts fell from 0.52 to 0.33 of the LDS cycles).
//   XOR-swizzled LDS bitmap (dword w at w ^ (((w >> 5) & 7) << 2), behind
//     lds_swz* hooks that were left as identities): 18.8 vs 16.8
//     (profiles/r03_pairs/): the extra address VALU per probe costs more than
//     the conflicts it removes, whose pattern on real data is close to random.
//   v9 every load of a container issued before any of it is consumed: 20.9
//     (profiles/r03_v9/); one-ahead prefetch in the multi-chunk array walks:
//     23.5 (profiles/r03_pf/).  The chunked walk is not latency-bound: issuing
//     the array loads earlier made the kernel slower both times.
//   v10-v12 a run of queries sharing A counted as one flat stream of 16-byte
//     chunks (wave scan, lane->pair map by popcount), chunk prefetch depth
//     1-3: 18.2-18.5; its skeletons 21-24: no probes 14.6, no staging 16.5, no
//     loads 15.6, no singletons 16.9 (profiles/r04_pairs/).
//   13 (APF) the next pair's A chunk prefetched when it is an array of <= 512
//     values: 17.7 (profiles/r04_f/).
//   14 one-op LDS word addressing per probe half through an inline-asm mask
//     (28 instead of 32 VALU per 8 probes): 17.2, the asm stopped the probe
//     loop's unroll; 32 / 16 queries per wave 17.5 / 19.9 (profiles/r04_l/).
//   Non-temporal loads for B containers whose row occurs once in the batch:
//     17.4 (profiles/r04_o/).
//   16/17 (SB) the <= 32 / 16-value B arrays of A's run counted lane-parallel
//     in one pass, 18-20 (PD) B-head prefetch depth 2-4, 31-37 (DBG) the
//     cost-isolation skeletons behind the budget above: all slower or wrong
//     by construction (profiles/r05_pairs/).
//   38/40 (ONE) one-off pairs probe a bitmap A in place and stage the smaller
//     of two arrays: at 8 queries per wave 0.554 / 1.019 / 1.353 ms at 32 /
//     64 / 128 queries, against 0.437 / 0.794 / 1.225 for 39
//     (profiles/r05_serve/, r06_serve/): the in-place probes cost more than
//     they save.  39 at 4096 queries: 17.2.
//   41/42 (SHD) dense bitmap shadows of the 256 hottest rows in HBM, staged by
//     one copy or read in place (DeviceView.ensure_shadow, PILOSA_SHADOW):
//     16.66 vs 16.45, serving 61.5k vs 69.3k req/s (profiles/r05_shadow/,
//     r05_serve/): the hot A rows are mostly bitmaps already.  Its build
//     kernel lives on as twin_build_kernel.
//   50/51 (ROT) each lane's 16-byte chunk rotated by (lane & 3) dwords to
//     spread the probes' banks: conflict ratio 0.516 -> 0.529, 24 % slower
//     (profiles/r06_pairs/): the conflicts are random gathers.
//   64/65 (UNS) un-staging, zero only the dwords a <= 512-value array set
//     instead of the 8 KiB clear: 16.73 vs 16.30 alone, 15.42 vs 15.05 on top
//     of the twins (8 predicated, conflicting ds_write_b32 and 8 more VGPRs
//     against 8 b128 stores); 61 / 62 twinned A only / B only at T = 2048:
//     16.16 / 15.40 (profiles/pairs_twin/).
//
// Bitmap twins (TWN, variant 63, 64 queries per wave): the dense array
// containers (n > T) of up to 64 mostly-array rows also live in HBM as bitmaps
// and either side of a pair reads its twin, so a dense B is 8 ds_read_b128
// ANDs instead of n ds_read_b32 gathers and a dense A stages by one copy.
// kbench, min of 10 (profiles/pairs_twin/): plain v6 16.29-16.30 ms (five
// alternated repeats); T = 3072 / 2730 / 2048: 15.86 / 15.59 / 15.05 ms with
// 12 / 19 / 35 twin rows (1.4 / 2.2 / 4.1 GiB, built in 1.4 ms).  LDS
// instructions -27 %, VALU -17 %, fetched bytes +12 %.
// Hot-pair table (profiles/hot_pairs/): six rounds inside the kernel left half
// of its time as fixed per-pair cost, so the lever is the number of pairs.
// Rows are queried by the Zipf law that fills them: most queries name two hot
// rows, whose per-shard intersection counts change only when they are written.
// Each view keeps int32 hot_counts[S][H][H] for its H = 512 rows of most bits
// (DeviceView.ensure_hot: densify + the MFMA bitgemm with one K-split per
// shard, 0.47 s and 954 MiB on the headline index; a written shard's slice is
// masked out by hot_valid[s] until it is recomputed).  pair_build answers a
// query whose two rows both have a slot from the table: key 0's entry carries
// {PRECOUNTED, count}, keys 1-15 NONE, no metas are loaded; the pair kernel's
// prologue copies the count into its partial.  kbench, min of 10, variant 63
// alternated three times: no table 15.12-15.15 ms; H = 128 / 256 / 512: 9.95 /
// 8.08 / 6.46 ms with 28 / 44 / 59 % of the (shard, query) entries precounted.
// Compaction (profiles/pair_compact/): those precounted queries kept their
// lanes of the grid -- 16 pairs entries each per shard, a partial, and with
// 26.9 live lanes per 64-query wave almost no wave was skipped.  For batches
// above the serving sizes pair_split_kernel now partitions the programs on the
// device into the live ones and the ones a table answers in EVERY shard;
// hot_pair_sum_kernel sums the latter from the table and pair_build, the pair
// kernel (template flag DQ) and the scatter run over the live count, which they
// read from device memory: 27 waves per (shard, key) unit instead of 62 on the
// headline batch, 0.42 of the pairs / partial columns.  The PRECOUNTED entries
// remain for serving-size batches, the per-shard route and views with a
// written shard's slice masked.
//
// Reference hot loops replaced: roaring/roaring.go:3078-3215 intersectionCount*
// and executor.go:1230-1290 (executeCount over executeIntersect).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "device_util.h"

namespace pk {
namespace {

constexpr uint32_t NONE = 0xffffffffu;
// pairs entry of a query pair_build answered from the view's hot-pair table:
// x = PRECOUNTED, y = the shard's count (key 0's entry; keys 1-15 hold NONE).
// Container indices stay below it (the engine takes the pair path only for
// views of fewer than 0xffffffff containers).
constexpr uint32_t PRECOUNTED = 0xfffffffeu;

// keymask[s][d] = row_keys() of every (shard, dense row): built once per view
// generation (DeviceView.ensure_keymask), it turns pair_build's up-to-16
// scattered meta loads per row into one 2-byte load (1.4 ms of a 4096-query
// Count(Intersect) batch on the headline index was pair_build).
__global__ __launch_bounds__(256) void keymask_build_kernel(ViewDev v, int S, uint16_t* __restrict__ out) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= int64_t(S) * v.D) return;
  const int s = int(t / v.D);
  const int64_t d = t - int64_t(s) * v.D;
  v.keymask = nullptr;
  int64_t lo;
  out[t] = uint16_t(row_keys(v, s, d, lo));
}

__device__ __forceinline__ void pair_build_body(const QueryProg* __restrict__ progs, int Q,
                                                const ViewDev* __restrict__ views, int S,
                                                uint2* __restrict__ pairs, int hot) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= int64_t(Q) * S) return;
  const int s = int(t / Q), q = int(t % Q);
  const QueryProg& qp = progs[q];
  uint2* dst = pairs + int64_t(s) * 16 * Q + q;
  // hot-pair table: both rows are hot rows of one view whose slice of this
  // shard is valid -> the shard's count rides in key 0's entry, no metas
  if (hot && qp.leaf_view[0] == qp.leaf_view[1] && qp.leaf_row[0] >= 0 && qp.leaf_row[1] >= 0) {
    const ViewDev& hv = views[qp.leaf_view[0]];
    if (hv.hot_counts != nullptr && gp(hv.hot_valid)[s]) {
      const int sa = gp(hv.hot_slot)[qp.leaf_row[0]], sb = gp(hv.hot_slot)[qp.leaf_row[1]];
      if (sa >= 0 && sb >= 0) {
        const int64_t h = hv.hot_h;
        const uint32_t c = uint32_t(gp(hv.hot_counts)[(int64_t(s) * h + min(sa, sb)) * h + max(sa, sb)]);
        dst[0] = make_uint2(PRECOUNTED, c);
#pragma unroll
        for (int j = 1; j < 16; j++) dst[int64_t(j) * Q] = make_uint2(NONE, NONE);
        return;
      }
    }
  }
  int64_t loa, lob;
  const uint32_t pa = row_keys(views[qp.leaf_view[0]], s, qp.leaf_row[0], loa);
  const uint32_t pb = row_keys(views[qp.leaf_view[1]], s, qp.leaf_row[1], lob);
  const uint32_t both = pa & pb;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    uint2 e = make_uint2(NONE, NONE);
    if ((both >> j) & 1) {
      const uint32_t below = (1u << j) - 1;
      e.x = uint32_t(loa + __popc(pa & below));
      e.y = uint32_t(lob + __popc(pb & below));
    }
    dst[int64_t(j) * Q] = e;
  }
}

__global__ __launch_bounds__(256) void pair_build_kernel(const QueryProg* __restrict__ progs, int Q,
                                                         const ViewDev* __restrict__ views, int S,
                                                         uint2* __restrict__ pairs, int hot) {
  pair_build_body(progs, Q, views, S, pairs, hot);
}

// The compacted route (pair_split_kernel below): the query count *nq is only
// known on the device.  The grid is sized by the host's count; threads past
// *nq * S exit before anything is divided by it (*nq may be 0).
__global__ __launch_bounds__(256) void pair_build_dq_kernel(const QueryProg* __restrict__ progs,
                                                            const int32_t* __restrict__ nq,
                                                            const ViewDev* __restrict__ views, int S,
                                                            uint2* __restrict__ pairs, int hot) {
  pair_build_body(progs, *nq, views, S, pairs, hot);
}

// ---- container primitives (wave-cooperative, lb = wave-private 1024-word LDS bitmap)

__device__ __forceinline__ void lds_clear(uint64_t* lb) {
  ulong2* l2 = reinterpret_cast<ulong2*>(lb);
  const int lane = wave_lane();
#pragma unroll
  for (int i = 0; i < 8; i++) l2[i * 64 + lane] = make_ulong2(0, 0);
}

// Stage a container of any type into lb as a bitmap.  BST
// (batched staging): an array's chunks are all loaded (4 per lane per round
// trip) before the LDS clear and the scatter, instead of one dependent load
// per 512 values -- a 4096-value array was 8 serial round trips, and staging
// was ~60 % of a 32-query batch's pair-kernel time (profiles/r05_serve/).
template <bool BST = false>
__device__ __forceinline__ void stage(uint64_t* lb, const uint16_t* p, int64_t m) {
  const int lane = wave_lane();
  const int type = meta_type(m);
  ulong2* l2 = reinterpret_cast<ulong2*>(lb);
  if (type == CT_BITMAP) {
    const auto g = gp(reinterpret_cast<const ulong2*>(p));
    ulong2 t[8];
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = g[i * 64 + lane];
#pragma unroll
    for (int i = 0; i < 8; i++) l2[i * 64 + lane] = t[i];
    lds_fence();
    return;
  }
  uint32_t* l32 = reinterpret_cast<uint32_t*>(lb);
  if (BST && type == CT_ARRAY) {
    const int n = meta_n(m);
    const auto p4 = gp(reinterpret_cast<const uint4*>(p));
    const int n8 = (n + 7) >> 3;
    bool cleared = false;
    for (int b = 0; b < n8; b += 4 * 64) {
      uint4 v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int e8 = b + k * 64 + lane;
        v[k] = make_uint4(0, 0, 0, 0);
        if (e8 < n8) v[k] = p4[e8];
      }
      if (!cleared) {   // the clear overlaps the first round of loads
        lds_clear(lb);
        lds_fence();
        cleared = true;
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int e8 = b + k * 64 + lane;
        const uint32_t w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
        const int rem = n - e8 * 8;
#pragma unroll
        for (int t = 0; t < 8; t++) {
          const uint32_t x = (w[t >> 1] >> ((t & 1) * 16)) & 0xffff;
          const bool ok = t < rem;
          if (e8 < n8) atomicOr(l32 + (x >> 5), ok ? (1u << (x & 31)) : 0u);
        }
      }
    }
    if (!cleared) {
      lds_clear(lb);
    }
    lds_fence();
    return;
  }
  lds_clear(lb);
  lds_fence();
  if (type == CT_ARRAY) {
    const int n = meta_n(m);
    const auto p4 = gp(reinterpret_cast<const uint4*>(p));
    const int n8 = (n + 7) >> 3;
    for (int e8 = lane; e8 < n8; e8 += 64) {
      const uint4 v4 = p4[e8];
      const uint32_t w[4] = {v4.x, v4.y, v4.z, v4.w};
      const int rem = n - e8 * 8;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint32_t v = (w[k >> 1] >> ((k & 1) * 16)) & 0xffff;
        const bool ok = k < rem;
        atomicOr(l32 + (v >> 5), ok ? (1u << (v & 31)) : 0u);
      }
    }
  } else {
    const auto pr = gp(p);
    const int nr = pr[0];
    for (int r = lane; r < nr; r += 64) {
      const uint32_t s = pr[8 + 2 * r], e = uint32_t(pr[9 + 2 * r]) + 1;
      const uint32_t ws = s >> 6, we = (e - 1) >> 6;
      if (ws == we) {
        const uint64_t mk = (e - s == 64) ? ~0ull : (((1ull << (e - s)) - 1) << (s & 63));
        atomicOr(reinterpret_cast<unsigned long long*>(&lb[ws]), mk);
      } else {
        atomicOr(reinterpret_cast<unsigned long long*>(&lb[ws]), ~0ull << (s & 63));
        for (uint32_t w = ws + 1; w < we; w++) lb[w] = ~0ull;
        const uint32_t hb = e & 63;
        atomicOr(reinterpret_cast<unsigned long long*>(&lb[we]), hb ? ((1ull << hb) - 1) : ~0ull);
      }
    }
  }
  lds_fence();
}

// Dword of value v's bit in a 1024-word bitmap (the staged one in LDS, or a
// container in global memory: BM's address space says which).
template <class BM>
__device__ __forceinline__ uint32_t bm_word(BM bm, uint32_t v) {
  return bm[v >> 5];
}

// Probe the 8 values packed in one 16-byte chunk against a 1024-word bitmap.
// Branch-free: all 8 word reads are issued before any is consumed (one
// lgkmcnt wait per chunk instead of one per value).  Pad values are 0 and are
// probed too; the caller subtracts their hits once per array (pad_hits()).
// v_bfe_u32 only uses bits 4:0 of its offset operand, so the value itself is
// the offset (no `& 31`).
template <class BM>
__device__ __forceinline__ int probe8(BM bm, const uint4 v4) {
  const uint32_t w[4] = {v4.x, v4.y, v4.z, v4.w};
  uint32_t x[8];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    x[2 * k] = bm_word(bm, w[k] & 0xffffu);
    x[2 * k + 1] = bm_word(bm, w[k] >> 16);
  }
  int c = 0;
#pragma unroll
  for (int k = 0; k < 4; k++)
    c += int(__builtin_amdgcn_ubfe(x[2 * k], w[k], 1u)) + int(__builtin_amdgcn_ubfe(x[2 * k + 1], w[k] >> 16, 1u));
  return c;
}

// Hits of `slots - n` zero-valued pad probes: bit 0 of the bitmap times the
// number of probed slots that were not array values (counted on lane 0 only,
// so the wave sum subtracts it once).
template <class BM>
__device__ __forceinline__ int pad_hits(BM bm, int slots, int n) {
  return wave_lane() == 0 ? int(bm[0] & 1u) * (slots - n) : 0;
}

// Whole-array probe with the next chunk's load issued before the current
// chunk's LDS probes (2-deep register pipeline); lanes past the array hold zero
// chunks; every lane probes 8 slots per iteration.
template <class BM>
__device__ __forceinline__ int probe_pipe(BM bm, const uint16_t* arr, int n) {
  const int lane = wave_lane();
  const auto p4 = gp(reinterpret_cast<const uint4*>(arr));
  const int n8 = (n + 7) >> 3;
  const int iters = (n8 + 63) >> 6;
  int c = 0;
  int e8 = lane;
  uint4 cur = make_uint4(0, 0, 0, 0);
  if (e8 < n8) cur = p4[e8];
#pragma unroll 2
  for (int it = 0; it < iters; it++) {
    const int ne8 = e8 + 64;
    uint4 nxt = make_uint4(0, 0, 0, 0);
    if (ne8 < n8) nxt = p4[ne8];
    c += probe8(bm, cur);
    cur = nxt;
    e8 = ne8;
  }
  return c - pad_hits(bm, iters * 512, n);
}

// |staged ∩ B| for a bitmap B in global memory 
__device__ __forceinline__ int and_lds_bitmap(const uint64_t* lb, const uint64_t* y) {
  const int lane = wave_lane();
  const ulong2* a = reinterpret_cast<const ulong2*>(lb);
  const auto b = gp(reinterpret_cast<const ulong2*>(y));
  int c = 0;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    ulong2 u[4], v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = b[(h * 4 + i) * 64 + lane];
#pragma unroll
    for (int i = 0; i < 4; i++) u[i] = a[(h * 4 + i) * 64 + lane];
#pragma unroll
    for (int i = 0; i < 4; i++) c += __popcll(u[i].x & v[i].x) + __popcll(u[i].y & v[i].y);
  }
  return c;
}

// |A ∩ B| of two bitmaps in global memory
__device__ __forceinline__ int and_global_bitmaps(const uint64_t* x, const uint64_t* y) {
  const int lane = wave_lane();
  const auto a = gp(reinterpret_cast<const ulong2*>(x));
  const auto b = gp(reinterpret_cast<const ulong2*>(y));
  int c = 0;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    ulong2 u[4], v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) u[i] = a[(h * 4 + i) * 64 + lane];
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = b[(h * 4 + i) * 64 + lane];
#pragma unroll
    for (int i = 0; i < 4; i++) c += __popcll(u[i].x & v[i].x) + __popcll(u[i].y & v[i].y);
  }
  return c;
}

// Count bits of a run container inside the staged bitmap.
__device__ __forceinline__ int runs_in_lds(const uint64_t* lb, const uint16_t* p) {
  const int lane = wave_lane();
  const auto pr = gp(p);
  const int nr = pr[0];
  int c = 0;
  for (int r = lane; r < nr; r += 64) {
    const uint32_t s = pr[8 + 2 * r], e = uint32_t(pr[9 + 2 * r]) + 1;
    const uint32_t ws = s >> 6, we = (e - 1) >> 6;
    for (uint32_t w = ws; w <= we; w++) {
      uint64_t mk = ~0ull;
      if (w == ws) mk &= ~0ull << (s & 63);
      if (w == we && (e & 63)) mk &= (1ull << (e & 63)) - 1;
      c += __popcll(lb[w] & mk);
    }
  }
  return c;
}

// Small arrays (n <= SMALL_ARRAY_N, the Zipf tail rows): one value per lane
// and iteration, all loads issued before the probes (probe8 would run 8 LDS
// probe instructions on a few lanes for a 20-value array).
#ifndef SMALL_ARRAY_N
#define SMALL_ARRAY_N 256
#endif
static_assert(SMALL_ARRAY_N % 64 == 0 && SMALL_ARRAY_N > 0, "SMALL_ARRAY_N must be a positive multiple of 64");
constexpr int SMALL_ITERS = SMALL_ARRAY_N / 64;
template <class BM>
__device__ __forceinline__ int probe_small(BM bm, const uint16_t* arr, int n) {
  const int lane = wave_lane();
  const auto p = gp(arr);
  if (n <= 64) {  // one value per lane, one probe (wave-uniform branch)
    const uint32_t v = lane < n ? uint32_t(p[lane]) : 0u;
    return int(__builtin_amdgcn_ubfe(bm_word(bm, v), v, 1u)) - pad_hits(bm, 64, n);
  }
  uint32_t v[SMALL_ITERS];
#pragma unroll
  for (int k = 0; k < SMALL_ITERS; k++) v[k] = lane + 64 * k < n ? uint32_t(p[lane + 64 * k]) : 0u;
  uint32_t x[SMALL_ITERS];
#pragma unroll
  for (int k = 0; k < SMALL_ITERS; k++) x[k] = bm_word(bm, v[k]);
  int c = 0;
#pragma unroll
  for (int k = 0; k < SMALL_ITERS; k++) c += int(__builtin_amdgcn_ubfe(x[k], v[k], 1u));
  return c - pad_hits(bm, 64 * SMALL_ITERS, n);
}

// |B ∩ staged| for any B container type (staged in lb)
__device__ __forceinline__ int count_vs_lds(const uint64_t* lb, const uint16_t* p, int64_t m) {
  const int type = meta_type(m);
  if (type == CT_BITMAP) return and_lds_bitmap(lb, reinterpret_cast<const uint64_t*>(p));
  if (type == CT_ARRAY) {
    const uint32_t* bm = reinterpret_cast<const uint32_t*>(lb);
    if (meta_n(m) <= SMALL_ARRAY_N) return probe_small(bm, p, meta_n(m));
    return probe_pipe(bm, p, meta_n(m));
  }
  return runs_in_lds(lb, p);
}

__device__ __forceinline__ int popc_and4(const uint4 a, const uint4 b) {
  return __popc(a.x & b.x) + __popc(a.y & b.y) + __popc(a.z & b.z) + __popc(a.w & b.w);
}

// ---- v6: one wave per workgroup (LDS bitmap at address 0) + the next pair's
// B head prefetched while the current pair is counted.
//
// Per pair, before anything of the current pair waits, ONE load is issued for
// the next valid pair's B: its whole array when n <= 64 (one value per lane),
// else its first 16 B per lane (all of an array of <= 512 values, chunk 0 of a
// bitmap / bigger array).  The current pair's head arrived during the previous
// pair, so a tail pair (most pairs) waits for nothing; the in-order vmcnt wait
// for anything loaded later also covers the prefetch, which by then has had
// the previous pair's work to arrive.
__device__ __forceinline__ uint4 load_bhead(const uint16_t* p, int64_t m) {
  const int lane = wave_lane();
  const int t = meta_type(m);
  if (t == CT_ARRAY && meta_n(m) <= 64) {
    const uint32_t v = uint32_t(gp(p)[min(lane, meta_n(m) - 1)]);
    return make_uint4(v, 0, 0, 0);
  }
  const int last = t == CT_BITMAP ? 511 : (t == CT_ARRAY ? ((meta_n(m) + 7) >> 3) - 1 : 0);
  return gp(reinterpret_cast<const uint4*>(p))[min(lane, last)];
}

// |B & staged| with B's head (load_bhead) already in registers
__device__ __forceinline__ int count_vs_head(const uint64_t* lb, const uint16_t* p, int64_t m, const uint4 head) {
  const int lane = wave_lane();
  const int t = meta_type(m);
  const uint32_t* bm = reinterpret_cast<const uint32_t*>(lb);
  if (t == CT_ARRAY) {
    const int n = meta_n(m);
    if (n <= 64) {
      const uint32_t v = lane < n ? head.x : 0u;
      return int(__builtin_amdgcn_ubfe(bm_word(bm, v), v, 1u)) - pad_hits(bm, 64, n);
    }
    const int n8 = (n + 7) >> 3;
    if (n <= 512) {
      const uint4 h = lane < n8 ? head : make_uint4(0, 0, 0, 0);
      return probe8(bm, h) - pad_hits(bm, 512, n);
    }
    // bigger arrays: chunk `lane` is the head, the rest pipelined as probe_pipe
    const auto p4 = gp(reinterpret_cast<const uint4*>(p));
    const int iters = (n8 + 63) >> 6;
    int c = 0;
    int e8 = lane;
    uint4 cur = head;  // n8 > 64: every lane's head chunk is real
#pragma unroll 2
    for (int it = 0; it < iters; it++) {
      const int ne8 = e8 + 64;
      uint4 nxt = make_uint4(0, 0, 0, 0);
      if (ne8 < n8) nxt = p4[ne8];
      c += probe8(bm, cur);
      cur = nxt;
      e8 = ne8;
    }
    return c - pad_hits(bm, iters * 512, n);
  }
  if (t == CT_BITMAP) {
    const auto g = gp(reinterpret_cast<const uint4*>(p));
    const uint4* l4 = reinterpret_cast<const uint4*>(lb);
    int c = popc_and4(l4[lane], head);
    {
      uint4 b[4], x[4];
#pragma unroll
      for (int k = 0; k < 4; k++) b[k] = g[(1 + k) * 64 + lane];
#pragma unroll
      for (int k = 0; k < 4; k++) x[k] = l4[(1 + k) * 64 + lane];
#pragma unroll
      for (int k = 0; k < 4; k++) c += popc_and4(x[k], b[k]);
    }
    {
      uint4 b[3], x[3];
#pragma unroll
      for (int k = 0; k < 3; k++) b[k] = g[(5 + k) * 64 + lane];
#pragma unroll
      for (int k = 0; k < 3; k++) x[k] = l4[(5 + k) * 64 + lane];
#pragma unroll
      for (int k = 0; k < 3; k++) c += popc_and4(x[k], b[k]);
    }
    return c;
  }
  return runs_in_lds(lb, p);
}

// twin[r][s][j]: row rows[r]'s key-j container of shard s as a bitmap (zeros
// where absent).  One wave per (r, s, j): built in LDS by stage(), copied out.
__global__ __launch_bounds__(64) void twin_build_kernel(ViewDev v, int S, const int32_t* __restrict__ rows, int R,
                                                        uint64_t* __restrict__ twin) {
  __shared__ uint64_t lb[1024];
  const int64_t w = int64_t(blockIdx.x) + int64_t(blockIdx.y) * 65535;
  if (w >= int64_t(R) * S * 16) return;
  const int j = int(w & 15);
  const int64_t rs = w >> 4;
  const int s = int(rs % S);
  const int r = int(rs / S);
  const int lane = wave_lane();
  ulong2* dst = reinterpret_cast<ulong2*>(twin + w * 1024);
  const int64_t d = rows[r];
  int64_t c = -1;
  if (d >= 0) {
    int64_t lo;
    const uint32_t pres = row_keys(v, s, d, lo);
    if ((pres >> j) & 1) c = lo + __popc(pres & ((1u << j) - 1));
  }
  if (c < 0) {
#pragma unroll
    for (int i = 0; i < 8; i++) dst[i * 64 + lane] = make_ulong2(0, 0);
    return;
  }
  const int64_t m = gp(v.meta)[c];
  stage<true>(lb, payload_of(v, m), m);
  const ulong2* l2 = reinterpret_cast<const ulong2*>(lb);
#pragma unroll
  for (int i = 0; i < 8; i++) dst[i * 64 + lane] = l2[i * 64 + lane];
}

// ---- bitmap twins (TWN): the dense ARRAY containers (n > the view's
// twin_cutoff) of the rows DeviceView.ensure_twin picked also exist as
// 1024-word bitmaps in HBM.  The prologue swaps such an operand's payload
// pointer for its twin and rewrites the lane's meta type to CT_BITMAP, on
// side A (TWN & 1), side B (TWN & 2) or both; everything after the prologue
// then takes its bitmap path: a twinned B is 8 conflict-free ds_read_b128
// ANDs instead of n ds_read_b32 gathers, a twinned A stages by one copy with
// no clear and no ds_or scatter.  Costs 8 KiB of reads instead of 2 n bytes.
__device__ __forceinline__ int64_t meta_as_bitmap(int64_t m) {
  return (m & ~(int64_t(3) << 4)) | (int64_t(CT_BITMAP) << 4);
}

__device__ __forceinline__ void twin_swap(const ViewDev& v, int64_t d, int S, int64_t u, int64_t& m, uint64_t& pl) {
  if (v.twin_slot == nullptr || meta_type(m) != CT_ARRAY || meta_n(m) <= v.twin_cutoff) return;
  const int sl = gp(v.twin_slot)[d];
  if (sl < 0) return;
  pl = reinterpret_cast<uint64_t>(v.twin + ((int64_t(sl) * S + (u >> 4)) * 16 + (u & 15)) * 1024);
  m = meta_as_bitmap(m);
}

// The pair kernel's query count: an int by value, as the kernel has always
// taken it (same kernel arguments, same code), or with DQ read from device
// memory.
template <bool DQ>
struct QCount {
  int q;
  __device__ __forceinline__ int get() const { return q; }
};
template <>
struct QCount<true> {
  const int32_t* q;
  __device__ __forceinline__ int get() const { return *q; }
};

// ---- v6: one wave per (shard, key, chunk of CQ queries).  BST = batched
// array staging (stage(), the serving variant 39); TWN = bitmap twins on side
// A (1), side B (2) or both (3, variant 63).  DQ = the query count is read from
// device memory (the compacted route): the grid is sized by the host's count,
// which is not smaller; the workgroups past the live ones exit first thing and
// the XCD remap runs over the live ones only (over the whole grid it would
// hand all live units to the first few XCDs).
template <int CQ, bool BST = false, int TWN = 0, bool DQ = false>
__global__ __launch_bounds__(64, 5) void and2_pairs_v6_kernel(const QueryProg* __restrict__ progs, QCount<DQ> qc,
                                                             const ViewDev* __restrict__ views, int S,
                                                             const uint2* __restrict__ pairs,
                                                             int32_t* __restrict__ partial) {
  __shared__ uint64_t lb[1024];
  const int lane = wave_lane();
  const int Q = qc.get();
  uint32_t nblk = gridDim.x;
  if (DQ) {
    const int64_t live = int64_t(S) * 16 * ((Q + CQ - 1) / CQ);   // *nq == 0: every workgroup exits
    if (int64_t(blockIdx.x) >= live) return;
    nblk = uint32_t(live);
  }
  const int64_t gw = int64_t(xcd_remap(blockIdx.x, nblk));
  const int nch = (Q + CQ - 1) / CQ;
  const int64_t u = gw / nch;
  if (u >= int64_t(S) * 16) return;
  const int q0 = int(gw % nch) * CQ;
  const int nq = min(CQ, Q - q0);

  uint32_t ea = NONE;
  int vai = -1;
  int64_t ma = 0, mb = 0;
  uint64_t pal = 0, pbl = 0;
  int mine = 0;
  if (lane < nq) {
    const uint2 e = pairs[u * Q + q0 + lane];
    if (e.x == PRECOUNTED) {
      mine = int(e.y);   // answered by pair_build from the hot-pair table
    } else if (e.x != NONE) {
      ea = e.x;
      vai = progs[q0 + lane].leaf_view[0];
      const int vbi = progs[q0 + lane].leaf_view[1];
      ma = gp(views[vai].meta)[e.x];
      mb = gp(views[vbi].meta)[e.y];
      pal = reinterpret_cast<uint64_t>(payload_of(views[vai], ma));
      pbl = reinterpret_cast<uint64_t>(payload_of(views[vbi], mb));
      if (TWN & 1) twin_swap(views[vai], progs[q0 + lane].leaf_row[0], S, u, ma, pal);
      if (TWN & 2) twin_swap(views[vbi], progs[q0 + lane].leaf_row[1], S, u, mb, pbl);
    }
  }
  uint64_t todo = __ballot(ea != NONE);
  if (todo) {
    uint32_t cached = NONE;
    int cached_v = -1;
    int i = __builtin_ctzll(todo);
    todo &= todo - 1;
    // head of pair i's B; inside the loop, of the pair after the current one
    uint4 pf = load_bhead(reinterpret_cast<const uint16_t*>(rl_u64(pbl, i)), rl_i64(mb, i));
    for (;;) {
      const uint32_t a = __builtin_amdgcn_readlane(ea, i);
      const int va = __builtin_amdgcn_readlane(vai, i);
      const int64_t mA = rl_i64(ma, i), mB = rl_i64(mb, i);
      const uint16_t* pA = reinterpret_cast<const uint16_t*>(rl_u64(pal, i));
      const uint16_t* pB = reinterpret_cast<const uint16_t*>(rl_u64(pbl, i));
      const int tA = meta_type(mA), tB = meta_type(mB);
      const int j = todo ? __builtin_ctzll(todo) : -1;
      const uint4 head = pf;
      if (j >= 0) pf = load_bhead(reinterpret_cast<const uint16_t*>(rl_u64(pbl, j)), rl_i64(mb, j));
      int c = 0;
      if (a == cached && va == cached_v) {
        c = count_vs_head(lb, pB, mB, head);
      } else {
        const bool next_same = j >= 0 && __builtin_amdgcn_readlane(ea, j) == a &&
                               __builtin_amdgcn_readlane(vai, j) == va;
        if (!next_same && tA == CT_BITMAP && tB == CT_BITMAP) {
          c = and_global_bitmaps(reinterpret_cast<const uint64_t*>(pA), reinterpret_cast<const uint64_t*>(pB));
        } else if (!next_same && tA == CT_ARRAY && tB == CT_BITMAP && meta_n(mA) <= SMALL_ARRAY_N) {
          c = probe_small(gp(reinterpret_cast<const uint32_t*>(pB)), pA, meta_n(mA));
        } else if (!next_same && tA == CT_ARRAY && tB == CT_BITMAP) {
          lds_fence();
          stage<BST>(lb, pB, mB);
          cached = NONE;
          cached_v = -1;
          c = count_vs_lds(lb, pA, mA);
        } else {
          lds_fence();  // previous readers of lb are done before it is rewritten
          stage<BST>(lb, pA, mA);
          cached = a;
          cached_v = va;
          c = count_vs_head(lb, pB, mB, head);
        }
      }
      c = wave_sum(c);
      if (lane == i) mine = c;
      if (j < 0) break;
      i = j;
      todo &= todo - 1;
    }
  }
  if (lane < nq) partial[u * Q + q0 + lane] = mine;
}

// ---- compaction: the queries a hot-pair table answers in every shard leave
// the pair grid.  pair_split_kernel partitions the sorted KIND_AND2 programs on
// the device (so every prepare route, the mesh and the alias dedupe get it
// unchanged and no host copy of the slot map has to follow the writes) into
//   live  compact copies of the programs the pair kernels still count (order
//         kept: runs of equal leaf 0 stay contiguous) + their submission indices
//   hot   {view, min slot, max slot, query} of the table-answered ones, summed
//         over the shards by hot_pair_sum_kernel, one wave each
// and leaves both counts in cnt[0] / cnt[1] for the kernels behind it (DQ).
// A query is table-answered when its rows are two slotted rows of one view
// whose table is valid in EVERY shard; with any shard masked by a write the
// view's queries stay live and pair_build's PRECOUNTED branch serves the valid
// shards as it does on the per-shard route and for small batches.
constexpr int SPLIT_T = 1024, SPLIT_W = SPLIT_T / 64, SPLIT_MAXV = 64;

__global__ __launch_bounds__(SPLIT_T) void pair_split_kernel(const QueryProg* __restrict__ progs, int Q,
                                                             const ViewDev* __restrict__ views, int V, int S,
                                                             const int64_t* __restrict__ ti,
                                                             QueryProg* __restrict__ lprogs,
                                                             int64_t* __restrict__ lti, int4* __restrict__ hotl,
                                                             int32_t* __restrict__ cnt) {
  __shared__ int vok[SPLIT_MAXV];
  __shared__ int wl[SPLIT_W], wh[SPLIT_W];
  __shared__ int dst[SPLIT_T];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // views past SPLIT_MAXV: their queries stay live
  const int nv = min(V, SPLIT_MAXV);
  if (tid < nv)
    vok[tid] = views[tid].hot_counts != nullptr && views[tid].hot_slot != nullptr && views[tid].hot_valid != nullptr;
  __syncthreads();
  for (int v = 0; v < nv; v++) {
    if (!vok[v]) continue;   // only ever cleared below: a stale 1 costs a redundant look
    const auto hv = gp(views[v].hot_valid);
    for (int s = tid; s < S; s += SPLIT_T)
      if (!hv[s]) vok[v] = 0;
  }
  __syncthreads();
  int lbase = 0, hbase = 0;
  for (int q0 = 0; q0 < Q; q0 += SPLIT_T) {
    const int q = q0 + tid;
    bool hot = false;
    int4 he = make_int4(0, 0, 0, 0);
    if (q < Q) {
      const QueryProg& qp = progs[q];
      const int va = qp.leaf_view[0];
      const int64_t ra = qp.leaf_row[0], rb = qp.leaf_row[1];
      if (va == qp.leaf_view[1] && va >= 0 && va < nv && vok[va] && ra >= 0 && rb >= 0) {
        const auto hs = gp(views[va].hot_slot);
        const int sa = hs[ra], sb = hs[rb];
        if (sa >= 0 && sb >= 0) {
          hot = true;
          he = make_int4(va, min(sa, sb), max(sa, sb), q);
        }
      }
    }
    const bool live = q < Q && !hot;
    const uint64_t bl = __ballot(live), bh = __ballot(hot);
    if (lane == 0) {
      wl[wv] = __popcll(bl);
      wh[wv] = __popcll(bh);
    }
    __syncthreads();
    int pl = 0, ph = 0, tl = 0, th = 0;
#pragma unroll
    for (int w = 0; w < SPLIT_W; w++) {
      pl += w < wv ? wl[w] : 0;
      ph += w < wv ? wh[w] : 0;
      tl += wl[w];
      th += wh[w];
    }
    const uint64_t below = (1ull << lane) - 1;
    int d = -1;
    if (live) {
      d = lbase + pl + __popcll(bl & below);
      lti[d] = ti[q];
    }
    if (hot) hotl[hbase + ph + __popcll(bh & below)] = he;
    dst[tid] = d;
    __syncthreads();
    // the tile's live programs, 16 B per thread and step
    const uint4* src = reinterpret_cast<const uint4*>(progs + q0);
    uint4* out = reinterpret_cast<uint4*>(lprogs);
    const int n16 = min(SPLIT_T, Q - q0) * int(sizeof(QueryProg) / 16);
    for (int i = tid; i < n16; i += SPLIT_T) {
      const int dq = dst[i >> 4];
      if (dq >= 0) out[int64_t(dq) * 16 + (i & 15)] = src[i];
    }
    __syncthreads();   // dst, wl, wh are rewritten by the next tile
    lbase += tl;
    hbase += th;
  }
  if (tid == 0) {
    cnt[0] = lbase;
    cnt[1] = hbase;
  }
}
static_assert(sizeof(QueryProg) == 16 * 16, "pair_split_kernel copies a program as 16 uint4");

// One wave per table-answered query: out[ti[query]] += the table's count of
// its slot pair summed over the shards.  Grid sized by the host's query count.
__global__ __launch_bounds__(256) void hot_pair_sum_kernel(const ViewDev* __restrict__ views, int S,
                                                           const int4* __restrict__ hotl,
                                                           const int32_t* __restrict__ cnt,
                                                           const int64_t* __restrict__ ti,
                                                           unsigned long long* __restrict__ out, int64_t nout) {
  const int w = int(blockIdx.x) * 4 + int(threadIdx.x >> 6);
  if (w >= cnt[1]) return;
  const int lane = wave_lane();
  const int4 e = hotl[w];
  const ViewDev& hv = views[e.x];
  const int64_t h = hv.hot_h;
  const auto hc = gp(hv.hot_counts) + int64_t(e.y) * h + e.z;
  int64_t a = 0;
#pragma unroll 4
  for (int s = lane; s < S; s += 64) a += uint32_t(hc[int64_t(s) * h * h]);
  a = wave_sum_i64(a);
  const int64_t o = ti[e.w];
  if (lane == 0 && a && o >= 0 && o < nout) atomicAdd(out + o, (unsigned long long)a);
}
}  // namespace

void launch_twin_build(const ViewDev& v, int S, const int32_t* rows, int R, uint64_t* twin, hipStream_t st) {
  const int64_t w = int64_t(R) * S * 16;
  if (w <= 0) return;
  const dim3 grid(unsigned(w < 65535 ? w : 65535), unsigned((w + 65534) / 65535));
  hipLaunchKernelGGL(twin_build_kernel, grid, dim3(64), 0, st, v, S, rows, R, twin);
}

void launch_keymask_build(const ViewDev& v, int S, uint16_t* out, hipStream_t st) {
  const int64_t n = int64_t(S) * v.D;
  if (n == 0) return;
  hipLaunchKernelGGL(keymask_build_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, v, S, out);
}

template <int CQ, bool BST, int TWN>
void launch_v6(const QueryProg* progs, int Q, const ViewDev* views, int S, const uint2* pairs, int32_t* partial,
               hipStream_t st) {
  const int64_t wv = int64_t(S) * 16 * ((Q + CQ - 1) / CQ);
  hipLaunchKernelGGL((and2_pairs_v6_kernel<CQ, BST, TWN>), dim3(unsigned(wv)), dim3(64), 0, st, progs, QCount<false>{Q},
                     views, S, pairs, partial);
}

// the same over *nq <= Q queries (and2_pairs_v6_kernel, DQ)
template <int CQ, int TWN>
void launch_v6_dq(const QueryProg* progs, int Q, const int32_t* nq, const ViewDev* views, int S, const uint2* pairs,
                  int32_t* partial, hipStream_t st) {
  const int64_t wv = int64_t(S) * 16 * ((Q + CQ - 1) / CQ);
  hipLaunchKernelGGL((and2_pairs_v6_kernel<CQ, false, TWN, true>), dim3(unsigned(wv)), dim3(64), 0, st, progs,
                     QCount<true>{nq}, views, S, pairs, partial);
}

// pair_build then the pair kernel.  `variant`: 63 = bitmap twins (64 queries
// per wave only; any other chunk size falls back to 6), 6 = plain v6, which
// for serving-size batches (Q <= 128, almost every pair one-off) picks 39 =
// batched array staging at 4 queries per wave up to 32 queries, 32 up to 64,
// 16 up to 128 (0.437 / 0.794 / 1.225 ms at 32 / 64 / 128 queries,
// profiles/r06_serve/kbench_b*.log).  Any other id runs plain v6, and only 6,
// 39 and 63 are handed entries answered from the hot-pair table.  `cq` =
// queries per wave (4 / 8 / 16 / 32 / 64; <= 0 picks by batch size: 8 for
// Q <= 128, 32 for Q <= 2048, 64 above).
void launch_and2_pairs(const QueryProg* progs, int Q, const ViewDev* views, int S, uint2* pairs, int32_t* partial,
                       int cq, int variant, hipStream_t st) {
  const int64_t items = int64_t(Q) * S;
  if (items == 0) return;
  const bool twin = variant == 63 && (cq > 0 ? cq == 64 : Q > 2048);
  if (variant == 63 && !twin) variant = 6;
  if (variant == 6 && cq <= 0 && Q <= 128) {
    variant = 39;
    cq = Q <= 32 ? 4 : (Q <= 64 ? 32 : 16);
  }
  if (cq <= 0) cq = Q <= 128 ? 8 : (Q <= 2048 ? 32 : 64);
  const int hot = variant == 6 || variant == 39 || variant == 63;
  hipLaunchKernelGGL(pair_build_kernel, dim3(unsigned((items + 255) / 256)), dim3(256), 0, st, progs, Q, views, S,
                     pairs, hot);
#define PK_LAUNCH(CQV)                                                         \
  if (variant == 39)                                                           \
    launch_v6<CQV, true, 0>(progs, Q, views, S, pairs, partial, st);           \
  else                                                                         \
    launch_v6<CQV, false, 0>(progs, Q, views, S, pairs, partial, st);          \
  break;
  switch (twin ? 0 : cq) {
    case 0: launch_v6<64, false, 3>(progs, Q, views, S, pairs, partial, st); break;
    case 4: PK_LAUNCH(4)
    case 8: PK_LAUNCH(8)
    case 16: PK_LAUNCH(16)
    case 32: PK_LAUNCH(32)
    default: PK_LAUNCH(64)
  }
#undef PK_LAUNCH
}

// Column sums of the pair kernel's per-(unit, query) partials (int32[U][n])
// scattered straight into the batch result: out[ti[q]] += sum_u partial[u][q].
// Replaces a strided torch reduction (~67 us for a 36-query serving batch,
// profiles/r05_serve/) plus an index_copy.  Block = 64 columns x 4 row lanes
// over a 128-row chunk; one int64 atomic per (block, column).
__device__ __forceinline__ void partial_sum_scatter_body(const int32_t* __restrict__ partial, int64_t U, int n,
                                                         const int64_t* __restrict__ ti,
                                                         unsigned long long* __restrict__ out, int64_t nout) {
  __shared__ long long acc[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int q = int(blockIdx.x) * 64 + tx;
  const int64_t r0 = int64_t(blockIdx.y) * 128;
  const int64_t r1 = r0 + 128 < U ? r0 + 128 : U;
  long long a = 0;
  if (q < n) {
#pragma unroll 8
    for (int64_t r = r0 + ty; r < r1; r += 4) a += partial[r * n + q];
  }
  acc[ty][tx] = a;
  __syncthreads();
  if (ty == 0 && q < n) {
    const long long t = acc[0][tx] + acc[1][tx] + acc[2][tx] + acc[3][tx];
    const int64_t o = ti[q];
    if (t && o >= 0 && o < nout) atomicAdd(out + o, (unsigned long long)t);
  }
}

__global__ __launch_bounds__(256) void partial_sum_scatter_kernel(const int32_t* __restrict__ partial, int64_t U,
                                                                  int n, const int64_t* __restrict__ ti,
                                                                  unsigned long long* __restrict__ out,
                                                                  int64_t nout) {
  partial_sum_scatter_body(partial, U, n, ti, out, nout);
}

// n = *nq columns (the compacted route); workgroups of columns past it exit whole
__global__ __launch_bounds__(256) void partial_sum_scatter_dq_kernel(const int32_t* __restrict__ partial, int64_t U,
                                                                     const int32_t* __restrict__ nq,
                                                                     const int64_t* __restrict__ ti,
                                                                     unsigned long long* __restrict__ out,
                                                                     int64_t nout) {
  const int n = *nq;
  if (int(blockIdx.x) * 64 >= n) return;
  partial_sum_scatter_body(partial, U, n, ti, out, nout);
}

void launch_partial_sum_scatter(const int32_t* partial, int64_t U, int n, const int64_t* ti, int64_t* out,
                                int64_t nout, hipStream_t st) {
  if (U <= 0 || n <= 0) return;
  const dim3 grid(unsigned((n + 63) / 64), unsigned((U + 127) / 128));
  hipLaunchKernelGGL(partial_sum_scatter_kernel, grid, dim3(256), 0, st, partial, U, n, ti,
                     reinterpret_cast<unsigned long long*>(out), nout);
}

// Count(Intersect) totals of a sorted KIND_AND2 part with the table-answered
// queries compacted out of the pair grid: split -> hot sum -> pair_build ->
// pair kernel -> scatter, the last three over the live count in work.
// Variant and queries per wave follow the host's Q as in launch_and2_pairs
// (the host does not know the live count); only the 32- and 64-query shapes
// of variants 6 and 63 exist with a device count.  false: nothing launched
// (serving-size batch, or a shape that is not built).
bool launch_and2_total(const QueryProg* progs, int Q, const ViewDev* views, int V, int S, const int64_t* ti,
                       int64_t* out, int64_t nout, uint2* pairs, int32_t* partial, uint8_t* work, int cq,
                       int variant, hipStream_t st) {
  if (Q <= 128 || S <= 0 || V <= 0) return false;
  const bool twin = variant == 63 && (cq > 0 ? cq == 64 : Q > 2048);
  if (variant == 63 && !twin) variant = 6;
  if (variant != 6 && !twin) return false;
  if (cq <= 0) cq = Q <= 2048 ? 32 : 64;
  if (cq != 32 && cq != 64) return false;
  int32_t* cnt = reinterpret_cast<int32_t*>(work);
  QueryProg* lprogs = reinterpret_cast<QueryProg*>(work + AND2_WORK_HEAD);
  int4* hotl = reinterpret_cast<int4*>(work + AND2_WORK_HEAD + int64_t(Q) * sizeof(QueryProg));
  int64_t* lti = reinterpret_cast<int64_t*>(work + AND2_WORK_HEAD + int64_t(Q) * (sizeof(QueryProg) + 16));
  unsigned long long* o64 = reinterpret_cast<unsigned long long*>(out);
  hipLaunchKernelGGL(pair_split_kernel, dim3(1), dim3(SPLIT_T), 0, st, progs, Q, views, V, S, ti, lprogs, lti, hotl,
                     cnt);
  hipLaunchKernelGGL(hot_pair_sum_kernel, dim3(unsigned((Q + 3) / 4)), dim3(256), 0, st, views, S, hotl, cnt, ti,
                     o64, nout);
  const int64_t items = int64_t(Q) * S;
  hipLaunchKernelGGL(pair_build_dq_kernel, dim3(unsigned((items + 255) / 256)), dim3(256), 0, st, lprogs, cnt, views,
                     S, pairs, 1);
  if (twin)
    launch_v6_dq<64, 3>(lprogs, Q, cnt, views, S, pairs, partial, st);
  else if (cq == 64)
    launch_v6_dq<64, 0>(lprogs, Q, cnt, views, S, pairs, partial, st);
  else
    launch_v6_dq<32, 0>(lprogs, Q, cnt, views, S, pairs, partial, st);
  const int64_t U = int64_t(S) * 16;
  const dim3 grid(unsigned((Q + 63) / 64), unsigned((U + 127) / 128));
  hipLaunchKernelGGL(partial_sum_scatter_dq_kernel, grid, dim3(256), 0, st, partial, U, cnt, lti, o64, nout);
  return true;
}

}  // namespace pk
