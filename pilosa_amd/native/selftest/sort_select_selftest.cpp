// Stand-alone check of kernels/sort_select.h (the word comparator and the tie
// cut of the Sort kernel, K29) on the host: build with
// -fsanitize=address,undefined and run directly.  Every case compares
// sort_compare32 / first_set_bits32 with a naive per-column loop: random,
// all-zero and all-one planes and sign words; thresholds 0, +-1, +- the largest
// magnitude of depths 1, 11 and 32, values taken from the word itself and
// random ones; both directions; q from 0 to 32 and beyond.
// stderr ends with "<n> cases, <f> failures"; exit status 1 on any failure.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "../../kernels/sort_select.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd32() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return uint32_t((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static int cases = 0, failures = 0;

static int64_t value_of(const uint32_t* planes, int depth, uint32_t sign, int col) {
  int64_t mag = 0;
  for (int p = 0; p < depth; p++) mag |= int64_t((planes[p] >> col) & 1u) << p;
  return ((sign >> col) & 1u) ? -mag : mag;
}

static void check_compare(const uint32_t* planes, int depth, uint32_t sign, int64_t T, const char* what) {
  for (int desc = 0; desc < 2; desc++) {
    uint32_t before = 0, equal = 0;
    for (int col = 0; col < 32; col++) {
      const int64_t v = value_of(planes, depth, sign, col);
      if (desc ? v > T : v < T) before |= 1u << col;
      if (v == T) equal |= 1u << col;
    }
    const uint64_t mag = T < 0 ? uint64_t(-T) : uint64_t(T);
    const pk::SortWords got =
        pk::sort_compare32([&](int p) { return planes[p]; }, depth, sign, T < 0, uint32_t(mag), desc != 0);
    cases++;
    if (got.before != before || got.equal != equal) {
      failures++;
      fprintf(stderr, "FAIL compare %s depth %d T %lld desc %d: before %08x want %08x, equal %08x want %08x\n", what,
              depth, (long long)T, desc, got.before, before, got.equal, equal);
    }
  }
}

static void check_word(const uint32_t* planes, int depth, uint32_t sign, const char* what) {
  const int64_t top = depth == 0 ? 0 : (int64_t(1) << depth) - 1;
  const int64_t fixed[] = {0, 1, -1, top, -top, top - 1, -(top - 1), top / 2, -(top / 2)};
  for (int64_t T : fixed)
    if (T >= -top && T <= top) check_compare(planes, depth, sign, T, what);
  for (int col = 0; col < 32; col += 5) check_compare(planes, depth, sign, value_of(planes, depth, sign, col), what);
  for (int i = 0; i < 4; i++) {
    const int64_t mag = depth == 0 ? 0 : int64_t(((uint64_t(rnd32()) << 32) | rnd32()) & uint64_t(top));
    check_compare(planes, depth, sign, (rnd32() & 1u) ? -mag : mag, what);
  }
}

static void check_first(uint32_t w) {
  for (int q = -1; q <= 34; q++) {
    uint32_t want = 0;
    int left = q;
    for (int b = 0; b < 32 && left > 0; b++)
      if ((w >> b) & 1u) {
        want |= 1u << b;
        left--;
      }
    const uint32_t got = pk::first_set_bits32(w, q);
    cases++;
    if (got != want) {
      failures++;
      fprintf(stderr, "FAIL first_set_bits32(%08x, %d) = %08x want %08x\n", w, q, got, want);
    }
  }
}

int main() {
  uint32_t planes[32];
  const int depths[] = {0, 1, 2, 11, 21, 31, 32};
  for (int depth : depths) {
    for (uint32_t fill : {0u, 0xffffffffu}) {
      for (int p = 0; p < 32; p++) planes[p] = fill;
      for (uint32_t sign : {0u, 0xffffffffu, 0xaaaa5555u})
        check_word(planes, depth, sign, fill ? "all one" : "all zero");
    }
    for (int i = 0; i < 200; i++) {
      for (int p = 0; p < 32; p++) planes[p] = rnd32();
      check_word(planes, depth, rnd32(), "random");
      for (int p = 0; p < 32; p++) planes[p] = rnd32() & rnd32() & rnd32();
      check_word(planes, depth, rnd32() & rnd32(), "sparse");
      // few distinct values: ties with T are common
      const uint32_t a = rnd32(), b = rnd32();
      for (int p = 0; p < 32; p++) planes[p] = (rnd32() & 1u) ? a : (rnd32() & 1u) ? b : ~a;
      check_word(planes, depth, (rnd32() & 1u) ? a : b, "tied");
    }
  }
  // a threshold whose magnitude needs more planes than the field has
  for (int p = 0; p < 32; p++) planes[p] = rnd32();
  for (int64_t T : {int64_t(2048), int64_t(-2048), int64_t(0xffffffffll), -int64_t(0xffffffffll)})
    check_compare(planes, 11, rnd32(), T, "beyond the planes");
  check_first(0u);
  check_first(0xffffffffu);
  check_first(1u);
  check_first(0x80000000u);
  for (int i = 0; i < 300; i++) {
    check_first(rnd32());
    check_first(rnd32() & rnd32() & rnd32());
  }
  fprintf(stderr, "%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
