// Stand-alone check of kernels/bit_transpose.h (the register transpose of the
// Distinct kernel, K26) on the host: build with -fsanitize=address,undefined
// and run directly.  Every case compares bit_transpose32 with the naive bit
// loop: random matrices, all-zero, all-one, every single-bit matrix, single
// rows, single columns, and the BSI use (row p = plane p of 32 column values).
// stderr ends with "<n> cases, <f> failures"; exit status 1 on any failure.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../kernels/bit_transpose.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd32() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return uint32_t((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static void naive(const uint32_t (&in)[32], uint32_t (&out)[32]) {
  for (int c = 0; c < 32; c++) {
    out[c] = 0;
    for (int p = 0; p < 32; p++) out[c] |= ((in[p] >> c) & 1u) << p;
  }
}

static int cases = 0, failures = 0;

static void check(const uint32_t (&in)[32], const char* what) {
  uint32_t want[32], got[32];
  naive(in, want);
  memcpy(got, in, sizeof(got));
  pk::bit_transpose32(got);
  cases++;
  if (memcmp(want, got, sizeof(got)) != 0) {
    failures++;
    fprintf(stderr, "FAIL %s\n", what);
    return;
  }
  pk::bit_transpose32(got);  // an involution
  if (memcmp(in, got, sizeof(got)) != 0) {
    failures++;
    fprintf(stderr, "FAIL %s (twice is not the identity)\n", what);
  }
}

int main() {
  uint32_t m[32];
  memset(m, 0, sizeof(m));
  check(m, "all zero");
  memset(m, 0xff, sizeof(m));
  check(m, "all one");
  for (int p = 0; p < 32; p++)
    for (int c = 0; c < 32; c++) {
      memset(m, 0, sizeof(m));
      m[p] = 1u << c;
      check(m, "single bit");
    }
  for (int p = 0; p < 32; p++) {
    memset(m, 0, sizeof(m));
    m[p] = 0xffffffffu;
    check(m, "single row");
    for (int q = 0; q < 32; q++) m[q] = 1u << p;
    check(m, "single column");
  }
  for (int i = 0; i < 2000; i++) {
    for (int p = 0; p < 32; p++) m[p] = rnd32();
    check(m, "random");
  }
  for (int i = 0; i < 200; i++) {  // sparse and dense
    for (int p = 0; p < 32; p++) m[p] = rnd32() & rnd32() & rnd32();
    check(m, "sparse");
    for (int p = 0; p < 32; p++) m[p] = rnd32() | rnd32() | rnd32();
    check(m, "dense");
  }
  // the kernel's use: plane p of 32 column values -> the values back
  for (int i = 0; i < 200; i++) {
    uint32_t vals[32], planes[32];
    const int depth = 1 + int(rnd32() % 32);
    for (int c = 0; c < 32; c++) vals[c] = depth == 32 ? rnd32() : (rnd32() & ((1u << depth) - 1));
    for (int p = 0; p < 32; p++) {
      planes[p] = 0;
      for (int c = 0; c < 32; c++) planes[p] |= ((vals[c] >> p) & 1u) << c;
    }
    check(planes, "planes");
    pk::bit_transpose32(planes);
    cases++;
    if (memcmp(planes, vals, sizeof(vals)) != 0) {
      failures++;
      fprintf(stderr, "FAIL planes -> values\n");
    }
  }
  fprintf(stderr, "%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
