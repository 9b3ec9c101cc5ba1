// Word-level pieces of Sort(field=, limit=) (sort_kernels.hip, K29), host and
// device: the bit-sliced comparator that classifies the 32 columns of a word
// against a threshold value without transposing the planes, and the "first q
// set bits of a word" cut of a tie group.  Plain C++ with no HIP dependency,
// so the host compiler can build and test it on its own
// (native/selftest/sort_select_selftest.cpp).
#pragma once
#include <stdint.h>

#include "bit_transpose.h"  // PK_HOST_DEVICE

namespace pk {

struct SortWords {
  uint32_t before;  // columns whose value sorts strictly before T
  uint32_t equal;   // columns whose value is T
};

// Columns of one 32-column word against the threshold T = (t_neg ? -t_mag :
// t_mag).  plane(p) is the word of bit plane p (0 where the plane is absent),
// p < depth <= 32; sign the word of the sign row.  A column's value is
// sign ? -magnitude : magnitude, so a set sign bit over magnitude 0 is the
// value 0.  "Before" is < ascending and > with desc.  MSB first: a column
// still equal to T on the planes above p is decided at p when its bit differs
// from T's.  The result is not masked: the caller ANDs it with the considered
// columns.
template <class Plane>
PK_HOST_DEVICE SortWords sort_compare32(Plane&& plane, int depth, uint32_t sign, bool t_neg, uint32_t t_mag,
                                        bool desc) {
  uint32_t eq = ~0u, lt = 0, gt = 0, nz = 0;
  if (depth < 32 && (uint64_t(t_mag) >> depth)) {  // |T| beyond the planes: every magnitude is smaller
    lt = ~0u;
    eq = 0;
    for (int p = depth - 1; p >= 0; p--) nz |= plane(p);
  } else {
    for (int p = depth - 1; p >= 0; p--) {
      const uint32_t w = plane(p);
      const uint32_t tb = ((t_mag >> p) & 1) ? ~0u : 0u;
      nz |= w;
      lt |= eq & ~w & tb;
      gt |= eq & w & ~tb;
      eq &= ~(w ^ tb);
    }
  }
  const uint32_t neg = sign & nz;  // really negative columns
  uint32_t less, same, more;
  if (t_neg && t_mag) {
    less = neg & gt;
    same = neg & eq;
    more = ~neg | lt;
  } else {
    less = neg | lt;
    same = ~neg & eq;
    more = ~neg & gt;
  }
  return SortWords{desc ? more : less, same};
}

// The q lowest set bits of w (all of w when q >= popcount, none when q <= 0).
PK_HOST_DEVICE uint32_t first_set_bits32(uint32_t w, int q) {
  uint32_t rest = w;  // w without its lowest min(q, popcount) set bits
#pragma unroll
  for (int i = 0; i < 32; i++)
    if (i < q) rest &= rest - 1;
  return w & ~rest;
}

}  // namespace pk
