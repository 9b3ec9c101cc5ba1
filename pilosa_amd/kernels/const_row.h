// Pieces of ConstRow(columns=[...]) (const_row_kernels.hip, K30), host and
// device: where a unit's columns lie in the sorted location vector, how one
// location splits into (unit, word, bit), and the meta word of a written unit.
// Plain C++ with no HIP dependency, so the host compiler can build and test it
// on its own (native/selftest/const_row_selftest.cpp).
//
// A location is `si << 20 | x`: si the index of the column's device shard in
// the view's shard list, x its offset in that shard.  A unit is one (shard,
// key) container, u = si * 16 + key = loc >> 16; the vector is ascending, so
// a unit's columns are one contiguous range of it.
#pragma once
#include <stdint.h>

#include "bit_transpose.h"  // PK_HOST_DEVICE

namespace pk {

// First index i in [0, n] with loc[i] >= key (n when there is none).  The
// result stays inside [0, n] whatever loc holds.  `Ptr` is anything indexable
// that yields int64_t: the kernel passes its global-address-space pointer, the
// host test a plain one, so both run this loop.
template <class Ptr>
PK_HOST_DEVICE int64_t const_row_lower_bound(Ptr loc, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (loc[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The first location that belongs to unit u or a later one.  The range of
// unit u is [lower_bound(start(u)), lower_bound(start(u + 1))).
PK_HOST_DEVICE int64_t const_row_unit_start(int64_t u) { return u << 16; }

struct ConstRowBit {
  int64_t unit;   // si * 16 + key
  uint32_t word;  // 32-bit word of the unit's 8 KiB bitmap, 0 .. 2047
  uint32_t bit;   // bit of that word, 0 .. 31
};

PK_HOST_DEVICE ConstRowBit const_row_split(int64_t loc) {
  const uint32_t x = uint32_t(loc) & 0xffffu;
  return ConstRowBit{loc >> 16, x >> 5, x & 31u};
}

// Meta word of unit u written as a bitmap container of `card` columns at
// payload + u * 4096 (uint16 units): key | CT_BITMAP << 4 | card << 6 |
// (u * 512) << 23, the offset in 16-byte units.  card <= 65536 fits the 17
// bits of meta_n.
PK_HOST_DEVICE int64_t const_row_meta(int64_t u, int64_t card) {
  return (u & 15) | (int64_t(2) << 4) | (card << 6) | ((u * 512) << 23);
}

}  // namespace pk
