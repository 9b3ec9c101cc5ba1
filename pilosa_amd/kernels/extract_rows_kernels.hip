// CDNA4 (gfx950) kernel K28: Extract(filter, Rows(field=)) for a set, time,
// mutex or bool field -- for every column of the filter, the rows of the
// field's standard view that hold it.
//
// K25 (row_filter_counts_kernel) stages one filter container per (shard, key)
// in LDS and streams every row of a field past it, but only counts.  K27
// (bsi_extract_kernel) knows where every column of the filter lands in the
// output: unit_off[s * 16 + j] of its (shard, key) unit plus the column's rank
// inside the unit.  This kernel joins the two: for every hit of a row on the
// staged filter it records which row, at which output position.
//
// Work unit, as in K25: one workgroup of four waves per (arena shard s, key j,
// chunk of dense rows of the field's view), XCD-remapped so that the chunks of
// one (s, j) share an L2.  A unit leaves block-uniformly, before any barrier,
// when unit_off[s * 16 + j] < 0 (empty, or beyond the window: K27's marking)
// or when the filter tile of the key is empty.
//
//   1. Filter and rank.  The filter is a program (build_slots / candidate_mask
//      / eval_tile, expr_tile.h), evaluated by every wave as in K27.  The
//      waves share the staging: wave w writes tile slots w and w + 4 into the
//      8 KiB LDS bitmap and, next to it, their part of the rank table -- the
//      exclusive popcount prefix per 32-bit word, 2,048 u16 entries.  A slot
//      is 256 words, four per lane: a wave scan (wave_scan_incl) gives the
//      prefix inside the slot, and since every wave holds the whole tile the
//      columns of the slots below are one wave reduction away -- no totals
//      travel through LDS and the scan needs no barrier of its own.  One
//      __syncthreads() after staging.  The output position of filter column x
//      is fr_pos() (filter_rank.h): unit_off + rank[x >> 5] + the popcount of
//      the word's lower bits.
//   2. Columns (any mode, chunk 0, only when a column vector is passed): the
//      set bits of the staged filter, ascending, at their positions.  A
//      request without an int field gets its column vector here, not from a
//      K27 launch.
//   3. Stream, as in K25: each wave takes rows_per_wave dense rows at a time,
//      one per lane; the row's key-j container comes from the key-presence
//      table or the walk of at most 16 metas (find_container).  Arrays of at
//      most 32 values are enumerated by the lane that found them; larger
//      arrays, bitmaps and runs by the whole wave, one container after the
//      other (filter_rank.h holds the per-lane enumerations).  Every hit -- a
//      column of the row's container whose filter bit is set -- at a position
//      pos < cap (the window's length) is emitted as (pos, dense row d).
//
// What "emitted" means is the mode:
//   count   wg_hits[blockIdx.x] = the workgroup's hits: a block reduction (one
//           more barrier) and one plain store per workgroup.  The host's
//           cumsum turns them into each workgroup's base and the total T.
//   fill    the same traversal again; keys[wg_base[blockIdx.x] + slot] =
//           pos * D + d, slot from a workgroup-local LDS cursor (an LDS
//           atomic; the compiler aggregates it per wave).  Every store is
//           bounds-checked against T, so data that changed between the two
//           passes cannot write outside the buffer.  The host sorts the keys:
//           ascending by column, then by dense row = by row id.
//   scalar  (mutex, bool) one pass, no count and no sort: atomicMin(first +
//           pos, row id) on a vector initialised to all ones.  The addresses
//           are unique while the mutex invariant holds; the minimum is the
//           host's "first row" even on a fragment that breaks it.
// No global atomics in the list modes, no grid-wide barrier, no spin, no
// cooperative launch in any mode.
//
// LDS (static): four WaveScratch 40,960 B + bitmap 8,192 B + rank 4,096 B (the
// 12 KiB) + the fill cursor (8 B) or the count's wave totals (32 B): at most
// 53,280 B, three workgroups per CU.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage), see
// profiles/extract_rows/resource_usage.txt:
//   count:  212 VGPRs, 0 AGPRs, 66 SGPRs, scratch 0, LDS 53,280 B
//   fill:   212 VGPRs, 0 AGPRs, 72 SGPRs, scratch 0, LDS 53,256 B
//   scalar: 212 VGPRs, 0 AGPRs, 66 SGPRs, scratch 0, LDS 53,248 B
//   no spills; occupancy 2 waves/SIMD in every mode, by registers (the four
//   tiles of eval_tile's stack, as in K27) -- the LDS would admit three
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"
#include "expr_tile.h"
#include "filter_rank.h"

namespace pk {
namespace {

constexpr int RX_THREADS = 64 * WAVES_PER_BLOCK;
constexpr int RX_OWNED_N = 32;  // arrays up to this size are enumerated by one lane
constexpr int RX_COUNT = 1, RX_FILL = 2, RX_SCALAR = 3;

// what a launch writes; the pointers of the other modes are null
struct RowsExtractOut {
  uint64_t* columns;            // any mode: the column vector [>= cap], or nullptr
  unsigned long long* wg_hits;  // count: hits per workgroup [grid]
  const int64_t* wg_base;       // fill: exclusive cumsum of wg_hits [grid]
  int64_t* keys;                // fill: pos * D + d per hit [T]
  int64_t T;
  const uint64_t* row_ids;      // scalar: the view's row directory [D]
  unsigned long long* first;    // scalar: smallest row id per position [cap], all ones = none
};

template <int MODE>
__global__ __launch_bounds__(RX_THREADS) void rows_extract_kernel(const QueryProg* __restrict__ progs,
                                                                  const ViewDev* __restrict__ views, int S, int fview,
                                                                  int64_t D, int nchunk, int64_t rows_per_block,
                                                                  int rows_per_wave,
                                                                  const int64_t* __restrict__ unit_off,
                                                                  const int64_t* __restrict__ col_base, int64_t cap,
                                                                  RowsExtractOut out) {
  __shared__ WaveScratch scratch[WAVES_PER_BLOCK];
  __shared__ __attribute__((aligned(16))) uint64_t fb[1024];      // the filter tile of (s, j) as a bitmap
  __shared__ __attribute__((aligned(16))) uint16_t rank[FR_WORDS];  // columns below each 32-bit word
  __shared__ unsigned long long cursor;                           // fill: next slot of the workgroup
  __shared__ unsigned long long wave_hits[WAVES_PER_BLOCK];       // count: the waves' totals
  const uint32_t unit = xcd_remap(blockIdx.x, gridDim.x);
  const int chunk = int(unit % uint32_t(nchunk));
  const uint32_t sj = unit / uint32_t(nchunk);
  const int j = int(sj & 15), s = int(sj >> 4);
  if (s >= S) return;
  const int64_t uo = unit_off[int64_t(s) * 16 + j];
  if (uo < 0) return;  // empty, or beyond the window (block-uniform)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  WaveScratch& ws = scratch[wave];

  // ---- 1. the filter tile, in every wave (block-uniform exits, no barrier yet)
  const QueryProg& qp = progs[0];
  if (!qp.nprog) return;
  uint32_t mask[MAXLEAF];
  build_slots(qp, views, s, ws, mask);
  if (!((candidate_mask(qp, mask) >> j) & 1)) return;
  Tile f;
  eval_tile(qp, views, s, j, ws, f);
  uint64_t any = 0;
  int below0 = 0, below1 = 0;  // this lane's columns in the slots below slot `wave` / slot `wave + 4`
#pragma unroll
  for (int i = 0; i < 8; i++) {
    any |= f.w[i].x | f.w[i].y;
    const int c = __popcll(f.w[i].x) + __popcll(f.w[i].y);
    if (i < wave) below0 += c;
    if (i < wave + 4) below1 += c;
  }
  if (!__ballot(any != 0)) return;
  const int base0 = wave_sum(below0), base1 = wave_sum(below1);
  // staging: wave w owns slots w and w + 4; lane l of slot i holds 32-bit words 4 * (64 * i + l) + {0, 1, 2, 3}
#pragma unroll
  for (int i = 0; i < 8; i++) {
    if ((i & 3) != wave) continue;  // wave-uniform
    const ulong2 t = f.w[i];
    reinterpret_cast<ulong2*>(fb)[i * 64 + lane] = t;
    const int c0 = __popc(uint32_t(t.x)), c1 = __popc(uint32_t(t.x >> 32)), c2 = __popc(uint32_t(t.y));
    const int c = c0 + c1 + c2 + __popc(uint32_t(t.y >> 32));
    const int e = (i < 4 ? base0 : base1) + wave_scan_incl(c) - c;  // <= 65,504 before the last word
    reinterpret_cast<ushort4*>(rank)[i * 64 + lane] =
        make_ushort4(uint16_t(e), uint16_t(e + c0), uint16_t(e + c0 + c1), uint16_t(e + c0 + c1 + c2));
  }
  if (MODE == RX_FILL && tid == 0) cursor = 0;
  __syncthreads();
  const uint32_t* fw = reinterpret_cast<const uint32_t*>(fb);

  // ---- 2. the column vector, by the first chunk's workgroup
  if (out.columns != nullptr && chunk == 0) {
    const uint64_t col0 = uint64_t(col_base[s]) + uint64_t(j) * 65536u;
    for (int w = tid; w < FR_WORDS; w += RX_THREADS) {
      int64_t o = uo + int64_t(rank[w]);
      fr_word_hits(uint32_t(w), fw[w], [&](uint32_t x) {
        if (o < cap) out.columns[o] = col0 + x;
        o++;
      });
    }
  }

  // ---- 3. stream the rows of this chunk past the filter, rows_per_wave per wave and step
  const ViewDev fv = views[fview];
  const int64_t Dv = min(fv.D, D);
  const int64_t d0 = rows_per_block > 0 ? int64_t(chunk) * rows_per_block : 0;
  const int64_t d1 = rows_per_block > 0 ? min(Dv, d0 + rows_per_block) : Dv;
  const int64_t wbase = MODE == RX_FILL ? out.wg_base[blockIdx.x] : 0;
  unsigned long long nh = 0;
  auto hit = [&](uint32_t x, int64_t d, uint64_t rid) {
    const int64_t pos = fr_pos(uo, rank, fw, x);
    if (pos >= cap) return;
    if (MODE == RX_COUNT) {
      nh++;
    } else if (MODE == RX_FILL) {
      const int64_t idx = wbase + int64_t(atomicAdd(&cursor, 1ull));
      if (idx >= 0 && idx < out.T) out.keys[idx] = pos * D + d;
    } else {
      atomicMin(out.first + pos, (unsigned long long)rid);
    }
  };
  for (int64_t db = d0 + int64_t(wave) * rows_per_wave; db < d1; db += int64_t(WAVES_PER_BLOCK) * rows_per_wave) {
    const int64_t d = db + lane;
    int64_t m = 0;
    if (lane < rows_per_wave && d < d1) {
      const int64_t c = find_container(fv, s, d, j);
      if (c >= 0) m = gp(fv.meta)[c];
    }
    const int n = meta_n(m);
    const int t = meta_type(m);
    const bool live = n > 0 && (t == CT_ARRAY || t == CT_BITMAP || t == CT_RUN);
    const bool owned = live && t == CT_ARRAY && n <= RX_OWNED_N;
    if (owned) {
      const uint64_t rid = MODE == RX_SCALAR ? gp(out.row_ids)[d] : 0;
      const auto p4 = gp(reinterpret_cast<const uint4*>(payload_of(fv, m)));
      for (int e = 0; e < ((n + 7) >> 3); e++) {
        const uint4 q = p4[e];
        fr_array_chunk_hits(fw, q.x, q.y, q.z, q.w, n - e * 8, [&](uint32_t x) { hit(x, d, rid); });
      }
    }
    uint64_t coop = __ballot(live && !owned);
    while (coop) {
      const int src = __builtin_ctzll(coop);
      coop &= coop - 1;
      const int64_t cm = rl_i64(m, src);
      const int64_t cd = db + src;
      const uint64_t rid = MODE == RX_SCALAR ? gp(out.row_ids)[cd] : 0;
      const uint16_t* p = payload_of(fv, cm);
      const int ct = meta_type(cm);
      auto emit = [&](uint32_t x) { hit(x, cd, rid); };
      if (ct == CT_BITMAP) {
        const auto g2 = gp(reinterpret_cast<const ulong2*>(p));
#pragma unroll 2
        for (int i = 0; i < 8; i++) {
          const ulong2 a = g2[i * 64 + lane];
          const uint32_t wi = 2u * uint32_t(i * 64 + lane);
          fr_bitmap_word_hits(fw, wi, a.x, emit);
          fr_bitmap_word_hits(fw, wi + 1u, a.y, emit);
        }
      } else if (ct == CT_ARRAY) {
        const int cn = meta_n(cm);
        const auto p4 = gp(reinterpret_cast<const uint4*>(p));
        for (int e = lane; e < ((cn + 7) >> 3); e += 64) {
          const uint4 q = p4[e];
          fr_array_chunk_hits(fw, q.x, q.y, q.z, q.w, cn - e * 8, emit);
        }
      } else {
        const int nr = gp(p)[0];
        const auto r32 = gp(reinterpret_cast<const uint32_t*>(p)) + 4;  // (start, last) pairs
        for (int r = lane; r < nr; r += 64) {
          const uint32_t ab = r32[r];
          const uint32_t a = ab & 0xffff, b = ab >> 16;
          if (b >= a) fr_run_hits(fw, a, b, emit);
        }
      }
    }
  }

  if (MODE == RX_COUNT) {
    const int64_t wt = wave_sum_i64(int64_t(nh));
    if (lane == 0) wave_hits[wave] = (unsigned long long)wt;
    __syncthreads();
    if (tid == 0) {
      unsigned long long tot = 0;
#pragma unroll
      for (int w = 0; w < WAVES_PER_BLOCK; w++) tot += wave_hits[w];
      out.wg_hits[blockIdx.x] = tot;
    }
  }
}

}  // namespace

// ------------------------------------------------------------ launcher

int64_t rows_extract_blocks(int S, int64_t D, int64_t rows_per_block) {
  if (S <= 0 || D < 0 || rows_per_block < 0) return 0;
  const int64_t nchunk = rows_per_block > 0 ? std::max<int64_t>(1, (D + rows_per_block - 1) / rows_per_block) : 1;
  const int64_t blocks = int64_t(S) * 16 * nchunk;
  return blocks >= (int64_t(1) << 31) ? -1 : blocks;
}

int64_t launch_rows_extract(int mode, const QueryProg* progs, const ViewDev* views, int S, int fview, int64_t D,
                            int64_t rows_per_block, int rows_per_wave, const int64_t* unit_off,
                            const int64_t* col_base, int64_t cap, uint64_t* columns, int64_t* wg, int64_t* keys,
                            int64_t T, const uint64_t* row_ids, uint64_t* first, hipStream_t st) {
  const int64_t blocks = rows_extract_blocks(S, D, rows_per_block);
  if (blocks < 0 || cap < 0 || mode < RX_COUNT || mode > RX_SCALAR) return -1;
  if (blocks == 0 || cap == 0) return 0;
  const int64_t nchunk = blocks / (int64_t(S) * 16);
  const int64_t chunk_rows = nchunk > 1 ? rows_per_block : D;
  if (rows_per_wave != 16 && rows_per_wave != 32 && rows_per_wave != 64)
    rows_per_wave = chunk_rows >= 256 ? 64 : (chunk_rows >= 128 ? 32 : 16);  // as launch_row_filter_counts
  RowsExtractOut out{};
  out.columns = columns;
  const dim3 grid{unsigned(blocks)}, block{RX_THREADS};
  if (mode == RX_COUNT) {
    out.wg_hits = reinterpret_cast<unsigned long long*>(wg);
    hipLaunchKernelGGL(rows_extract_kernel<RX_COUNT>, grid, block, 0, st, progs, views, S, fview, D, int(nchunk),
                       rows_per_block, rows_per_wave, unit_off, col_base, cap, out);
  } else if (mode == RX_FILL) {
    out.wg_base = wg;
    out.keys = keys;
    out.T = T;
    hipLaunchKernelGGL(rows_extract_kernel<RX_FILL>, grid, block, 0, st, progs, views, S, fview, D, int(nchunk),
                       rows_per_block, rows_per_wave, unit_off, col_base, cap, out);
  } else {
    out.row_ids = row_ids;
    out.first = reinterpret_cast<unsigned long long*>(first);
    hipLaunchKernelGGL(rows_extract_kernel<RX_SCALAR>, grid, block, 0, st, progs, views, S, fview, D, int(nchunk),
                       rows_per_block, rows_per_wave, unit_off, col_base, cap, out);
  }
  return blocks;
}

}  // namespace pk
