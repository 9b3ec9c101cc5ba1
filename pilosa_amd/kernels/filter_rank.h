// The pure pieces of rows_extract_kernel (K28, extract_rows_kernels.hip), host
// and device: where a column of a staged filter lands in the output, and which
// values of a row's container hit the filter.  The filter of one (shard, key)
// is 2,048 32-bit words fw[] (bit b of word w = column 32 * w + b of the key)
// next to rank[], the exclusive popcount prefix per word (the prefix before
// the last word is at most 65,504, so u16 holds it).  Plain C++ with no HIP
// dependency and no LDS or wave intrinsic, so the host compiler can build and
// test it on its own (native/selftest/filter_rank_selftest.cpp).
//
// Every enumeration calls emit(x) once per hit, x = the column's offset inside
// the key (0 .. 65535), in ascending order of x.
#pragma once
#include <stdint.h>

#ifndef PK_HOST_DEVICE
#if defined(__HIPCC__)
#define PK_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define PK_HOST_DEVICE inline
#endif
#endif

namespace pk {

constexpr int FR_WORDS = 2048;  // 32-bit words of one key's filter

// Output position of filter column x (its bit must be set): the unit's offset,
// the columns in the words below x's and the columns below x in its word.
PK_HOST_DEVICE int64_t fr_pos(int64_t unit_off, const uint16_t* rank, const uint32_t* fw, uint32_t x) {
  const uint32_t w = x >> 5;
  return unit_off + int64_t(rank[w]) + int64_t(__builtin_popcount(fw[w] & ((1u << (x & 31)) - 1u)));
}

// The set bits of h, a container word already ANDed with filter word w.
template <class E>
PK_HOST_DEVICE void fr_word_hits(uint32_t w, uint32_t h, E&& emit) {
  while (h) {
    emit(w * 32u + uint32_t(__builtin_ctz(h)));
    h &= h - 1u;
  }
}

// One 16-byte chunk of an array container: eight u16 values in q0 .. q3 (low
// half first), of which the first nvalid (0 .. 8) belong to the array.
template <class E>
PK_HOST_DEVICE void fr_array_chunk_hits(const uint32_t* fw, uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3,
                                        int nvalid, E&& emit) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 8; k++) {
    const uint32_t q = k < 2 ? q0 : (k < 4 ? q1 : (k < 6 ? q2 : q3));
    const uint32_t x = (q >> ((k & 1) * 16)) & 0xffffu;
    if (k < nvalid && ((fw[x >> 5] >> (x & 31)) & 1u)) emit(x);
  }
}

// 64-bit word wi (0 .. 1023) of a bitmap container.
template <class E>
PK_HOST_DEVICE void fr_bitmap_word_hits(const uint32_t* fw, uint32_t wi, uint64_t bits, E&& emit) {
  fr_word_hits(2u * wi, uint32_t(bits) & fw[2u * wi], emit);
  fr_word_hits(2u * wi + 1u, uint32_t(bits >> 32) & fw[2u * wi + 1u], emit);
}

// The run [a, b] (a <= b <= 65535) across the words it covers: the first and
// the last word are masked, the words between are taken whole.
template <class E>
PK_HOST_DEVICE void fr_run_hits(const uint32_t* fw, uint32_t a, uint32_t b, E&& emit) {
  const uint32_t wa = a >> 5, wb = b >> 5;
  const uint32_t first = ~0u << (a & 31), last = ~0u >> (31u - (b & 31));
  if (wa == wb) {
    fr_word_hits(wa, fw[wa] & first & last, emit);
    return;
  }
  fr_word_hits(wa, fw[wa] & first, emit);
  for (uint32_t w = wa + 1; w < wb; w++) fr_word_hits(w, fw[w], emit);
  fr_word_hits(wb, fw[wb] & last, emit);
}

}  // namespace pk
