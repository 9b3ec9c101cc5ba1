// 32 x 32 bit-matrix transpose in registers, host and device: the primitive
// that turns 32 bit-plane words of a BSI field (row p = plane p, bit c =
// column c) into 32 per-column magnitudes (row c = column c, bit p = plane p).
// Plain C++ with no HIP dependency, so the host compiler can build and test it
// on its own (native/selftest/bit_transpose_selftest.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PK_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define PK_HOST_DEVICE inline
#endif

namespace pk {

// In place: afterwards bit p of a[c] is bit c of the old a[p] (bit 0 = LSB).
// Five rounds of block swaps (Hacker's Delight 7-3, LSB-first): round j swaps
// the j x j blocks above and below the diagonal of every 2j x 2j block, 16
// three-XOR swaps of word pairs each, 80 in all.  Both loops have constant
// trip counts and constant indices once unrolled, so a[] stays in registers.
PK_HOST_DEVICE void bit_transpose32(uint32_t (&a)[32]) {
#pragma unroll
  for (int r = 0; r < 5; r++) {
    const int j = 16 >> r;
    const uint32_t m = r == 0 ? 0x0000ffffu : r == 1 ? 0x00ff00ffu : r == 2 ? 0x0f0f0f0fu
                     : r == 3 ? 0x33333333u : 0x55555555u;
#pragma unroll
    for (int k = 0; k < 32; k++) {
      if (k & j) continue;
      const uint32_t t = ((a[k] >> j) ^ a[k + j]) & m;
      a[k + j] ^= t;
      a[k] ^= t << j;
    }
  }
}

}  // namespace pk
