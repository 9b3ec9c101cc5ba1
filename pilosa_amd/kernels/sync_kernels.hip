// Anti-entropy read path (gfx950): block checksums and block data straight
// from an HBM arena, so a sync pass never materialises a cold fragment.
//
//   K22  fragment block checksums   fragment.go:1776-1854 (Blocks),
//        fragment.go:2811-2825 (blockHasher); block data: fragment.go:1856-1871
//
// A block is 100 consecutive row ids of one fragment; its checksum is XXH64
// (seed 0) over the block's set positions row * ShardWidth + column in
// ascending order, each written as 8 big-endian bytes.
//
// One 256-thread workgroup per unit = (fragment, block).  The host turns the
// sorted row directory into a dense-row range [d0, d1) per block; the
// workgroup walks dense rows ascending, the fragment's M arena sub-shards
// (shards wider than 2^20 columns), the row's containers (ascending slot j;
// type-0 metadata words are dead slots left by device clears and compaction)
// and their values ascending.  An array container's values are copied to an
// LDS staging buffer as they are; a bitmap or run container is expanded into
// an 8 KiB LDS bitmap (as container_merge does) and enumerated 256 words at a
// time by a popcount prefix scan.  Staged values are the low 16 bits; the
// position is base | low with base = row << e | m << 20 | j << 16.
//
//   hash: lanes 0..3 own one XXH64 accumulator each and consume one 32-byte
//         stripe (4 positions) per step from the staging buffer.  The 0..3
//         positions left over after the last whole stripe carry over to the
//         next container (a stripe may straddle a container, row or sub-shard
//         boundary); lane 0 finalises (kernels/xxh64_state.h).
//   dump: every thread writes staged positions to out[] in stream order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"
#include "xxh64_state.h"

namespace pk {

namespace {

constexpr int WG = 256;                // 4 waves of 64
constexpr int SEG_WORDS = WG;          // bitmap words enumerated per pass: one per thread
constexpr int STAGE = SEG_WORDS * 64;  // staged values per pass

struct WalkLds {
  uint64_t bm[1024];
  uint16_t stg[STAGE];
  uint64_t carry[4];
  uint64_t accs[4];
  int32_t wtot[WG / 64];
};

// OR a bitmap or run container into the (cleared) LDS bitmap.
__device__ __forceinline__ void expand_container(uint64_t* bm, const uint16_t* p, int type) {
  const int tid = threadIdx.x;
  if (type == CT_BITMAP) {
    const uint64_t* w = reinterpret_cast<const uint64_t*>(p);
    for (int i = tid; i < 1024; i += WG) bm[i] = w[i];
    return;
  }
  for (int i = tid; i < 1024; i += WG) bm[i] = 0;
  __syncthreads();
  const int nr = p[0];  // runs [start, last] at p[8 + 2r], p[9 + 2r]
  for (int r = tid; r < nr; r += WG) {
    const uint32_t s = p[8 + 2 * r], l = p[9 + 2 * r];
    if (s > l) continue;
    const uint32_t ws = s >> 6, we = l >> 6;
    for (uint32_t w = ws; w <= we; w++) {
      const uint32_t lo = w == ws ? (s & 63) : 0, hi = w == we ? (l & 63) + 1 : 64;
      const uint64_t mk = (hi - lo == 64) ? ~0ull : (((1ull << (hi - lo)) - 1) << lo);
      atomicOr(reinterpret_cast<unsigned long long*>(&bm[w]), mk);
    }
  }
}

// One unit's walk state: positions seen, the hash lanes' accumulator (threads
// 0..3) and the number of carried positions (uniform over the workgroup).
struct Walk {
  uint64_t total;
  uint64_t acc;
  int cn;
};

// The T values staged in L.stg (positions base | stg[i]) join the stream.
template <bool DUMP>
__device__ __forceinline__ void consume(WalkLds& L, Walk& w, uint64_t base, int T, uint64_t* __restrict__ out,
                                        uint64_t cap) {
  const int tid = threadIdx.x;
  if (DUMP) {
    for (int i = tid; i < T; i += WG)
      if (w.total + i < cap) out[w.total + i] = base | L.stg[i];
    w.total += T;
    __syncthreads();   // stg is rewritten by the next pass
    return;
  }
  // the stream seen here: carry[0 .. cn) then stg[0 .. T)
  const int avail = w.cn + T;
  const int stripes = avail >> 2, rem = avail & 3;
  uint64_t keep = 0;
  if (tid < 4) {
    uint64_t acc = w.acc;
    for (int i = 0; i < stripes; i++) {
      const int idx = 4 * i + tid;
      const uint64_t pos = idx < w.cn ? L.carry[idx] : (base | L.stg[idx - w.cn]);
      acc = xxh::round(acc, xxh::bswap(pos));
    }
    w.acc = acc;
    const int idx = 4 * stripes + tid;
    if (tid < rem) keep = idx < w.cn ? L.carry[idx] : (base | L.stg[idx - w.cn]);
  }
  __syncthreads();     // every carry read is done
  if (tid < rem) L.carry[tid] = keep;
  w.cn = rem;
  w.total += T;
  __syncthreads();
}

template <bool DUMP>
__device__ __forceinline__ void walk_container(WalkLds& L, Walk& w, const uint16_t* __restrict__ payload, int64_t m,
                                               uint64_t base, uint64_t* __restrict__ out, uint64_t cap) {
  const int tid = threadIdx.x;
  const int type = meta_type(m);
  const uint16_t* p = payload + meta_off16(m) * 8;
  if (type == CT_ARRAY) {
    const int n = meta_n(m);
    for (int c0 = 0; c0 < n; c0 += STAGE) {
      const int T = min(STAGE, n - c0);
      for (int i = tid; i < T; i += WG) L.stg[i] = p[c0 + i];
      __syncthreads();
      consume<DUMP>(L, w, base, T, out, cap);
    }
    return;
  }
  expand_container(L.bm, p, type);
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  for (int seg = 0; seg < 1024 / SEG_WORDS; seg++) {
    uint64_t x = L.bm[seg * SEG_WORDS + tid];
    const int c = __popcll(x);
    int incl = c;
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(incl, o, 64);
      if (lane >= o) incl += y;
    }
    if (lane == 63) L.wtot[wave] = incl;
    __syncthreads();
    int at = incl - c, T = 0;
    for (int k = 0; k < WG / 64; k++) {
      if (k < wave) at += L.wtot[k];
      T += L.wtot[k];
    }
    const int vbase = (seg * SEG_WORDS + tid) * 64;
    while (x) {
      L.stg[at++] = uint16_t(vbase + __ffsll(static_cast<long long>(x)) - 1);
      x &= x - 1;
    }
    __syncthreads();   // stg written, wtot read
    if (T) consume<DUMP>(L, w, base, T, out, cap);
  }
}

// units[u] = {first arena shard of the fragment, d0, d1}; rows[d] = row id of
// dense row d; e = shard width exponent.  Hash: out_n[u] positions, out_h[u]
// their XXH64.  Dump (one unit): positions to out[0 .. cap).
template <bool DUMP>
__global__ __launch_bounds__(WG) void block_walk_kernel(ViewDev v, const int32_t* __restrict__ units, int M, int e,
                                                        const int64_t* __restrict__ rows,
                                                        int64_t* __restrict__ out_n, uint64_t* __restrict__ out_h,
                                                        uint64_t* __restrict__ out, uint64_t cap) {
  __shared__ WalkLds L;
  const int tid = threadIdx.x;
  const int64_t u = blockIdx.x;
  const int s0 = units[3 * u], d0 = units[3 * u + 1], d1 = units[3 * u + 2];
  Walk w;
  w.total = 0;
  w.cn = 0;
  w.acc = xxh::acc_init(tid & 3);
  for (int d = d0; d < d1; d++) {
    const uint64_t rbase = uint64_t(rows[d]) << e;
    for (int m = 0; m < M; m++) {
      const int s = s0 + m;
      const uint32_t* rp = v.rowptr + int64_t(s) * (v.D + 1);
      const int64_t sb = v.shard_base[s];
      const int64_t lo = sb + rp[d], hi = sb + rp[d + 1];
      for (int64_t ci = lo; ci < hi; ci++) {
        const int64_t mw = v.meta[ci];
        if (meta_type(mw) == 0 || meta_n(mw) == 0) continue;
        const uint64_t base = rbase | (uint64_t(m) << 20) | (uint64_t(meta_j(mw)) << 16);
        walk_container<DUMP>(L, w, v.payload, mw, base, out, cap);
      }
    }
  }
  if (DUMP) return;
  if (tid < 4) L.accs[tid] = w.acc;
  __syncthreads();
  if (tid == 0) {
    uint64_t left[3];
    for (int i = 0; i < w.cn; i++) left[i] = xxh::bswap(L.carry[i]);
    out_n[u] = int64_t(w.total);
    out_h[u] = xxh::finalise(L.accs, left, w.total);
  }
}

}  // namespace

void launch_block_hash(const ViewDev& v, const int32_t* units, int64_t U, int M, int e, const int64_t* rows,
                       int64_t* out_n, uint64_t* out_h, hipStream_t st) {
  constexpr int64_t CHUNK = 1 << 16;   // units per launch
  for (int64_t u0 = 0; u0 < U; u0 += CHUNK) {
    const int64_t n = std::min<int64_t>(CHUNK, U - u0);
    hipLaunchKernelGGL((block_walk_kernel<false>), dim3(unsigned(n)), dim3(WG), 0, st, v, units + 3 * u0, M, e, rows,
                       out_n + u0, out_h + u0, static_cast<uint64_t*>(nullptr), uint64_t(0));
  }
}

void launch_block_dump(const ViewDev& v, const int32_t* unit, int M, int e, const int64_t* rows, uint64_t* out,
                       int64_t cap, hipStream_t st) {
  if (cap <= 0) return;
  hipLaunchKernelGGL((block_walk_kernel<true>), dim3(1), dim3(WG), 0, st, v, unit, M, e, rows,
                     static_cast<int64_t*>(nullptr), static_cast<uint64_t*>(nullptr), out, uint64_t(cap));
}

}  // namespace pk
