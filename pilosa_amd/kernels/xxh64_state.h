// XXH64 (seed 0) as four state functions -- round, merge, tail, finalise --
// shared by the block-checksum kernel (sync_kernels.hip) and the stand-alone
// host self-test (native/selftest/block_hash_selftest.cpp), so the host
// program exercises exactly the code the kernel runs.
//
// The input is always a whole number of 8-byte words (block checksums hash
// positions, fragment.go:2811-2825), so of XXH64's finalisation only these
// cases exist: fewer than 4 words (no accumulators, seed + PRIME5), the
// 4-accumulator merge, 0..3 8-byte tail rounds, and the avalanche.  Words are
// the little-endian reads of the byte stream: a position written as 8
// big-endian bytes enters as bswap64(position).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XXH_HD __host__ __device__ __forceinline__
#else
#define XXH_HD inline
#endif

namespace xxh {

constexpr uint64_t P1 = 0x9E3779B185EBCA87ull;
constexpr uint64_t P2 = 0xC2B2AE3D27D4EB4Full;
constexpr uint64_t P3 = 0x165667B19E3779F9ull;
constexpr uint64_t P4 = 0x85EBCA77C2B2AE63ull;
constexpr uint64_t P5 = 0x27D4EB2F165667C5ull;

XXH_HD uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

// Initial value of accumulator k (0..3), seed 0.
XXH_HD uint64_t acc_init(int k) {
  return k == 0 ? P1 + P2 : k == 1 ? P2 : k == 2 ? 0ull : 0ull - P1;
}

// One accumulator consumes one word of its stripe.
XXH_HD uint64_t round(uint64_t acc, uint64_t w) { return rotl(acc + w * P2, 31) * P1; }

XXH_HD uint64_t merge_round(uint64_t h, uint64_t v) { return (h ^ round(0, v)) * P1 + P4; }

// The four accumulators after the last whole stripe -> one hash value.
XXH_HD uint64_t merge(uint64_t v0, uint64_t v1, uint64_t v2, uint64_t v3) {
  uint64_t h = rotl(v0, 1) + rotl(v1, 7) + rotl(v2, 12) + rotl(v3, 18);
  h = merge_round(h, v0);
  h = merge_round(h, v1);
  h = merge_round(h, v2);
  return merge_round(h, v3);
}

// One 8-byte tail round.
XXH_HD uint64_t tail(uint64_t h, uint64_t w) { return rotl(h ^ round(0, w), 27) * P1 + P4; }

XXH_HD uint64_t avalanche(uint64_t h) {
  h ^= h >> 33;
  h *= P2;
  h ^= h >> 29;
  h *= P3;
  return h ^ (h >> 32);
}

// Hash of n words: v[0..3] = the accumulators after n / 4 whole stripes
// (unused when n < 4), left[0 .. n % 4) the words after the last stripe.
XXH_HD uint64_t finalise(const uint64_t* v, const uint64_t* left, uint64_t n) {
  uint64_t h = n >= 4 ? merge(v[0], v[1], v[2], v[3]) : P5;
  h += n * 8;
  const int rem = int(n & 3);
  for (int i = 0; i < rem; i++) h = tail(h, left[i]);
  return avalanche(h);
}

XXH_HD uint64_t bswap(uint64_t x) { return __builtin_bswap64(x); }

}  // namespace xxh
