// K25: exact row counts of a whole field under one filter, TopK(field=, k=).
//
// TopK ranks every row of a field by |row ∩ filter| summed over all shards.
// The only other device route to those numbers is one Op("and", (filter,
// Leaf(field, row))) program per row through expr_count, which re-evaluates the
// filter once per (row, shard, key).  A field's arena already holds every
// row's containers sorted by (shard, dense row, key), so here the filter is
// staged once and all rows stream past it:
//
//   * one workgroup (4 waves) per (arena shard s, key j, chunk of dense rows);
//     consecutive units share (s, j) and, after the XCD remap, an L2.  With
//     rows_per_block = 0 the chunk is the whole field (one workgroup per
//     (s, j));
//   * the workgroup decodes the filter row's key-j container of shard s -- an
//     array, a bitmap or a run -- into an 8 KiB LDS bitmap.  No container at
//     (s, j), or an empty one: the workgroup leaves before any barrier (the
//     test depends on s and j alone, so the exit is block-uniform);
//   * each wave takes 64 dense rows at a time, one per lane (16 or 32 where the
//     workgroup has fewer than 256 rows, so that all four waves work): the
//     row's key-j container comes from keymask[s][d] (bit j, index
//     rowptr[s][d] + popcount of the lower bits) or, for a view without the
//     table, from a walk of the row's at most 16 meta words;
//   * arrays of at most RFC_OWNED_N values are counted by the lane that found
//     them (16-byte loads, one LDS bit test per value): the tail of a Zipf
//     field is such arrays and a wave per container would leave 60 lanes
//     idle.  Everything else is counted by the whole wave, one container
//     after the other: bitmaps by coalesced 16-byte loads AND the LDS words,
//     arrays eight values per lane and load, runs one run per lane with
//     masked popcounts of the LDS words they cover;
//   * one 64-bit atomicAdd into out[d] per non-zero (s, j, d).
//
// Without a filter row_card_all_kernel sums the metadata counts and reads no
// payload.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage):
//   row_filter_counts_kernel: 60 VGPRs, 0 AGPRs, 60 SGPRs, scratch 0, LDS
//                             8192 B, occupancy 8 waves/SIMD (neither
//                             registers nor LDS limit it)
//   row_card_all_kernel:      15 VGPRs, 37 SGPRs, scratch 0, LDS 0, occupancy 8
// Measurements against the per-row programs route: profiles/topk/README.md.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"
#include "device_util.h"

namespace pk {
namespace {

constexpr int RFC_THREADS = 256;
constexpr int RFC_OWNED_N = 32;   // arrays up to this size are counted by one lane

// bits of the staged filter inside [a, b] (a <= b < 65536)
__device__ __forceinline__ int popc_range(const uint64_t* fb, uint32_t a, uint32_t b) {
  const uint32_t wa = a >> 6, wb = b >> 6;
  const uint64_t first = ~0ull << (a & 63);
  const uint64_t last = ~0ull >> (63 - (b & 63));
  if (wa == wb) return __popcll(fb[wa] & first & last);
  int c = __popcll(fb[wa] & first) + __popcll(fb[wb] & last);
  for (uint32_t w = wa + 1; w < wb; w++) c += __popcll(fb[w]);
  return c;
}

__global__ __launch_bounds__(RFC_THREADS) void row_filter_counts_kernel(ViewDev fv, ViewDev xv, int64_t xd, int S,
                                                                        int nchunk, int64_t rows_per_block,
                                                                        int rows_per_wave,
                                                                        unsigned long long* __restrict__ out) {
  __shared__ uint64_t fb[1024];   // the filter's (s, j) container as a bitmap
  const uint32_t unit = xcd_remap(blockIdx.x, gridDim.x);
  const int chunk = int(unit % uint32_t(nchunk));
  const uint32_t sj = unit / uint32_t(nchunk);
  const int j = int(sj & 15), s = int(sj >> 4);
  if (s >= S) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // ---- stage the filter (block-uniform exits before the first barrier)
  const int64_t xc = find_container(xv, s, xd, j);
  if (xc < 0) return;
  const int64_t xm = gp(xv.meta)[xc];
  if (meta_n(xm) == 0) return;
  const int xt = meta_type(xm);
  const uint16_t* xp = payload_of(xv, xm);
  {
    ulong2* l2 = reinterpret_cast<ulong2*>(fb);
    if (xt == CT_BITMAP) {
      const auto g2 = gp(reinterpret_cast<const ulong2*>(xp));
      for (int i = tid; i < 512; i += RFC_THREADS) l2[i] = g2[i];
    } else {
      for (int i = tid; i < 512; i += RFC_THREADS) l2[i] = make_ulong2(0, 0);
    }
  }
  __syncthreads();
  if (xt == CT_ARRAY) {
    uint32_t* f32 = reinterpret_cast<uint32_t*>(fb);
    const int n = meta_n(xm);
    const auto p4 = gp(reinterpret_cast<const uint4*>(xp));
    for (int e = tid; e < ((n + 7) >> 3); e += RFC_THREADS) {
      const uint4 q = p4[e];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint32_t x = val8(q, k);
        if (e * 8 + k < n) atomicOr(&f32[x >> 5], 1u << (x & 31));
      }
    }
  } else if (xt == CT_RUN) {
    uint32_t* f32 = reinterpret_cast<uint32_t*>(fb);
    const int nr = gp(xp)[0];
    const auto r32 = gp(reinterpret_cast<const uint32_t*>(xp)) + 4;   // (start, last) pairs
    for (int r = tid; r < nr; r += RFC_THREADS) {
      const uint32_t ab = r32[r];
      const uint32_t a = ab & 0xffff, b = ab >> 16;
      if (b < a) continue;
      const uint32_t wa = a >> 5, wb = b >> 5;
      const uint32_t first = ~0u << (a & 31), last = ~0u >> (31 - (b & 31));
      if (wa == wb) {
        atomicOr(&f32[wa], first & last);
      } else {
        atomicOr(&f32[wa], first);
        for (uint32_t w = wa + 1; w < wb; w++) atomicOr(&f32[w], ~0u);
        atomicOr(&f32[wb], last);
      }
    }
  }
  __syncthreads();

  // ---- stream the rows of this chunk past it, rows_per_wave per wave and step
  const uint32_t* f32 = reinterpret_cast<const uint32_t*>(fb);
  const int64_t d0 = rows_per_block > 0 ? int64_t(chunk) * rows_per_block : 0;
  const int64_t d1 = rows_per_block > 0 ? min(fv.D, d0 + rows_per_block) : fv.D;
  for (int64_t db = d0 + int64_t(wave) * rows_per_wave; db < d1; db += 4 * rows_per_wave) {
    const int64_t d = db + lane;
    int64_t m = 0;
    if (lane < rows_per_wave && d < d1) {
      const int64_t c = find_container(fv, s, d, j);
      if (c >= 0) m = gp(fv.meta)[c];
    }
    const int n = meta_n(m);
    const int t = meta_type(m);
    const bool live = n > 0 && (t == CT_ARRAY || t == CT_BITMAP || t == CT_RUN);
    const bool owned = live && t == CT_ARRAY && n <= RFC_OWNED_N;
    if (owned) {
      const auto p4 = gp(reinterpret_cast<const uint4*>(payload_of(fv, m)));
      int cnt = 0;
      for (int e = 0; e < ((n + 7) >> 3); e++) {
        const uint4 q = p4[e];
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const uint32_t x = val8(q, k);
          if (e * 8 + k < n) cnt += int((f32[x >> 5] >> (x & 31)) & 1);
        }
      }
      if (cnt) atomicAdd(out + d, (unsigned long long)cnt);
    }
    uint64_t coop = __ballot(live && !owned);
    while (coop) {
      const int src = __builtin_ctzll(coop);
      coop &= coop - 1;
      const int64_t cm = rl_i64(m, src);
      const uint16_t* p = payload_of(fv, cm);
      const int ct = meta_type(cm);
      int cnt = 0;
      if (ct == CT_BITMAP) {
        const auto g2 = gp(reinterpret_cast<const ulong2*>(p));
        const ulong2* l2 = reinterpret_cast<const ulong2*>(fb);
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const ulong2 a = g2[i * 64 + lane];
          const ulong2 b = l2[i * 64 + lane];
          cnt += __popcll(a.x & b.x) + __popcll(a.y & b.y);
        }
      } else if (ct == CT_ARRAY) {
        const int cn = meta_n(cm);
        const auto p4 = gp(reinterpret_cast<const uint4*>(p));
        for (int e = lane; e < ((cn + 7) >> 3); e += 64) {
          const uint4 q = p4[e];
#pragma unroll
          for (int k = 0; k < 8; k++) {
            const uint32_t x = val8(q, k);
            if (e * 8 + k < cn) cnt += int((f32[x >> 5] >> (x & 31)) & 1);
          }
        }
      } else {
        const int nr = gp(p)[0];
        const auto r32 = gp(reinterpret_cast<const uint32_t*>(p)) + 4;
        for (int r = lane; r < nr; r += 64) {
          const uint32_t ab = r32[r];
          const uint32_t a = ab & 0xffff, b = ab >> 16;
          if (b >= a) cnt += popc_range(fb, a, b);
        }
      }
      const int total = wave_sum(cnt);
      if (lane == 0 && total) atomicAdd(out + db + src, (unsigned long long)total);
    }
  }
}

// No filter: out[d] += the metadata counts of row d's containers in every
// shard; no payload is read.  Grid-stride over (shard, dense row), d fastest.
__global__ __launch_bounds__(256) void row_card_all_kernel(ViewDev v, int S, unsigned long long* __restrict__ out) {
  const int64_t total = int64_t(S) * v.D;
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += int64_t(gridDim.x) * blockDim.x) {
    const int s = int(t / v.D);
    const int64_t d = t - int64_t(s) * v.D;
    const auto rp = gp(v.rowptr + int64_t(s) * (v.D + 1));
    const int64_t sb = gp(v.shard_base)[s];
    const uint32_t r0 = rp[d], r1 = rp[d + 1];
    unsigned long long n = 0;
    for (uint32_t c = r0; c < r1; c++) n += unsigned(meta_n(gp(v.meta)[sb + c]));
    if (n) atomicAdd(out + d, n);
  }
}

}  // namespace

int64_t launch_row_filter_counts(const ViewDev& fv, const ViewDev* xv, int64_t xd, int S, int64_t rows_per_block,
                                 int rows_per_wave, unsigned long long* out, hipStream_t st) {
  if (S <= 0 || fv.D <= 0) return 0;
  if (xv == nullptr) {
    const int64_t total = int64_t(S) * fv.D;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, int64_t(1) << 20);
    hipLaunchKernelGGL(row_card_all_kernel, dim3(unsigned(blocks)), dim3(256), 0, st, fv, S, out);
    return blocks;
  }
  if (xd < 0 || xd >= xv->D) return 0;   // the filter row has no container here
  const int64_t nchunk = rows_per_block > 0 ? (fv.D + rows_per_block - 1) / rows_per_block : 1;
  const int64_t blocks = int64_t(S) * 16 * nchunk;
  if (blocks >= (int64_t(1) << 31)) return -1;
  // rows a wave looks up per step: a workgroup with few rows spreads them over
  // its four waves (the cooperative containers of a wave are counted one after
  // the other, so 64 dense rows on one wave are a chain of 64 dependent passes)
  const int64_t chunk_rows = nchunk > 1 ? rows_per_block : fv.D;
  if (rows_per_wave != 16 && rows_per_wave != 32 && rows_per_wave != 64)
    rows_per_wave = chunk_rows >= 256 ? 64 : (chunk_rows >= 128 ? 32 : 16);
  hipLaunchKernelGGL(row_filter_counts_kernel, dim3(unsigned(blocks)), dim3(RFC_THREADS), 0, st, fv, *xv, xd, S,
                     int(nchunk), rows_per_block, rows_per_wave, out);
  return blocks;
}

}  // namespace pk
