// ConstRow(columns=[...]) on the device (gfx950).
//
//   K30 const_row_kernel   a literal row, given by its column ids, as a dense
//                          one-row view (Pilosa added the call after v1.3)
//
// The host maps every listed column to a location `si << 20 | x` (si = index
// of its device shard in the view's shard list, x = offset in that shard),
// drops the columns of shards the view does not hold, sorts the locations and
// uploads them as one int64 vector (GpuEngine.const_row_view).  The kernel
// writes the layout of bsi_range_kernel / shift_dense_kernel: one 8 KiB bitmap
// per unit u = si * 16 + key at payload + u * 4096 (uint16 units) and
// meta[u] = key | CT_BITMAP << 4 | card << 6 | (u * 512) << 23.  Every unit of
// every shard is written in full, the all-zero ones too, so no reader sees
// uninitialised memory and the host runs no separate clearing pass.
//
// Shape chosen: one wave per unit, four units per 256-thread workgroup, a
// wave-private 8 KiB LDS tile and no __syncthreads() (the alternative, a
// workgroup per unit with two barriers, puts four times the workgroups behind
// the mostly empty units of a short list and buys nothing for a full one: a
// wave ORs 64 columns per instruction and a unit holds at most 65,536).  The
// 32 KiB of LDS per workgroup admit five workgroups of a CU's 160 KiB, 20
// waves, at 21 VGPRs each: the kernel is a store stream, bound by the 128 KiB
// + 128 B it writes per shard, not by occupancy.
//
// Per unit:
//   1. lanes 0 and 1 find the unit's range [lo, hi) of the location vector by
//      a lower-bound search each (const_row.h), broadcast by readlane;
//   2. an empty range (wave-uniform branch): 128 bytes of zeros per lane;
//   3. otherwise: zero the tile, OR the bits in with non-returning LDS
//      atomics (duplicates cost nothing), copy the tile out with 16-byte
//      stores, counting the bits on the way;
//   4. wave_sum of the counts, lane 0 stores the meta word.
// Plain stores and vector LDS atomics only: no global atomics, no spin, no
// cooperative launch.  The searches stay inside [0, n] and a bit's tile word
// is masked to the tile whatever the vector holds, so a malformed vector
// gives a wrong row, never an access outside the buffers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "device_util.h"
#include "const_row.h"

namespace pk {

namespace {

constexpr int CR_WAVES = 4;          // units per workgroup
constexpr int CR_TILE_WORDS = 2048;  // 8 KiB as 32-bit words

__global__ __launch_bounds__(CR_WAVES * 64) void const_row_kernel(const int64_t* __restrict__ loc, int64_t n, int S,
                                                                  uint16_t* __restrict__ payload,
                                                                  int64_t* __restrict__ meta) {
  __shared__ __attribute__((aligned(16))) uint32_t tiles[CR_WAVES][CR_TILE_WORDS];
  const int lane = wave_lane();
  const int wave = threadIdx.x >> 6;
  const int64_t u = int64_t(blockIdx.x) * CR_WAVES + wave;
  if (u >= int64_t(S) * 16) return;  // whole waves leave; nothing below waits for another wave
  const auto lp = gp(loc);
  // lane 0: the unit's first location, lane 1: the next unit's (odd lanes repeat lane 1)
  const int64_t b = const_row_lower_bound(lp, n, const_row_unit_start(u + (lane & 1)));
  const int64_t lo = rl_i64(b, 0), hi = rl_i64(b, 1);
  uint4* dst = reinterpret_cast<uint4*>(payload + u * 4096);
  int c = 0;
  if (lo >= hi) {
#pragma unroll
    for (int i = 0; i < 8; i++) dst[i * 64 + lane] = make_uint4(0, 0, 0, 0);
  } else {
    uint32_t* tile = tiles[wave];
    uint4* t4 = reinterpret_cast<uint4*>(tile);
#pragma unroll
    for (int i = 0; i < 8; i++) t4[i * 64 + lane] = make_uint4(0, 0, 0, 0);
    lds_fence();
    for (int64_t i = lo + lane; i < hi; i += 64) {
      const ConstRowBit p = const_row_split(lp[i]);
      atomicOr(&tile[p.word & (CR_TILE_WORDS - 1)], 1u << p.bit);
    }
    lds_fence();
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint4 q = t4[i * 64 + lane];
      c += __popc(q.x) + __popc(q.y) + __popc(q.z) + __popc(q.w);
      dst[i * 64 + lane] = q;
    }
  }
  const int64_t card = wave_sum_i64(c);
  if (lane == 0) meta[u] = const_row_meta(u, card);
}

}  // namespace

void launch_const_row(const int64_t* loc, int64_t n, int S, uint16_t* payload, int64_t* meta, hipStream_t st) {
  const int64_t units = int64_t(S) * 16;
  if (units <= 0 || n < 0) return;
  hipLaunchKernelGGL(const_row_kernel, dim3(unsigned((units + CR_WAVES - 1) / CR_WAVES)), dim3(CR_WAVES * 64), 0, st,
                     loc, n, S, payload, meta);
}

}  // namespace pk
