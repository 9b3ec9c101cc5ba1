// Stand-alone check of kernels/filter_rank.h (the pure pieces of
// rows_extract_kernel, K28) on the host: build with
// -fsanitize=address,undefined and run directly.  Every case compares the
// output position (fr_pos) and a hit enumeration (array chunks, bitmap words,
// runs) with a naive bit loop over one key's 65,536 columns, on random, empty,
// full and single-bit filters.  The filter words and the rank table live in
// exactly sized heap blocks, so an index past either is an ASan report.
// stderr ends with "<n> cases, <f> failures"; exit status 1 on any failure.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../kernels/filter_rank.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd32() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return uint32_t((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static int cases = 0, failures = 0;

static void fail(const char* filter, const char* what) {
  failures++;
  fprintf(stderr, "FAIL %s: %s\n", filter, what);
}

struct Filter {
  std::vector<uint32_t> fw;    // FR_WORDS words
  std::vector<uint16_t> rank;  // exclusive popcount prefix per word, as the kernel builds it
  std::vector<int> naive_pos;  // per column: its position among the filter's columns, -1 = not in the filter
  const char* name;

  Filter(const char* n) : fw(pk::FR_WORDS, 0u), rank(pk::FR_WORDS, 0), naive_pos(65536, -1), name(n) {}

  void finish() {
    uint32_t run = 0;
    for (int w = 0; w < pk::FR_WORDS; w++) {
      rank[w] = uint16_t(run);
      if (w == pk::FR_WORDS - 1 && run > 65504) fail(name, "prefix before the last word beyond u16's use");
      run += uint32_t(__builtin_popcount(fw[w]));
    }
    int p = 0;
    for (uint32_t x = 0; x < 65536; x++)
      if ((fw[x >> 5] >> (x & 31)) & 1u) naive_pos[x] = p++;
  }
};

static const int64_t UNIT_OFF = (int64_t(1) << 33) + 12345;  // positions are 64-bit

// the hits an enumeration reported against the naive loop over `member`
// (which columns the container holds): same columns, ascending, right positions
static void compare(const Filter& f, const std::vector<uint8_t>& member, const std::vector<uint32_t>& got,
                    const char* what) {
  cases++;
  std::vector<uint32_t> want;
  for (uint32_t x = 0; x < 65536; x++)
    if (member[x] && f.naive_pos[x] >= 0) want.push_back(x);
  if (want != got) return fail(f.name, what);
  for (size_t i = 0; i < got.size(); i++)
    if (pk::fr_pos(UNIT_OFF, f.rank.data(), f.fw.data(), got[i]) != UNIT_OFF + f.naive_pos[got[i]])
      return fail(f.name, "position of a hit");
}

static void check_positions(const Filter& f) {
  cases++;
  for (uint32_t x = 0; x < 65536; x++)
    if (f.naive_pos[x] >= 0 && pk::fr_pos(UNIT_OFF, f.rank.data(), f.fw.data(), x) != UNIT_OFF + f.naive_pos[x])
      return fail(f.name, "fr_pos");
}

// an ascending array of n distinct values through 16-byte chunks, as a lane
// (all chunks) or a wave (chunks strided over 64 lanes: the union is the same)
static void check_array(const Filter& f, int n, int mode) {
  std::vector<uint8_t> member(65536, 0);
  std::vector<uint16_t> vals;
  if (mode == 0) {  // scattered
    while (int(vals.size()) < n) {
      const uint32_t x = rnd32() & 0xffff;
      if (!member[x]) { member[x] = 1; vals.push_back(0); }
    }
  } else {  // packed at the top: the last value is 65535
    for (int i = 0; i < n; i++) { member[65535 - i] = 1; vals.push_back(0); }
  }
  vals.clear();
  for (uint32_t x = 0; x < 65536; x++)
    if (member[x]) vals.push_back(uint16_t(x));
  // the payload is padded to a multiple of 8 values; the pad holds values that would hit (0xffff, 0)
  std::vector<uint16_t> padded(vals);
  while (padded.size() % 8) padded.push_back(padded.size() % 2 ? 0xffff : 0);
  std::vector<uint32_t> got;
  for (int e = 0; e < (n + 7) / 8; e++) {
    uint32_t q[4];
    memcpy(q, padded.data() + e * 8, 16);
    pk::fr_array_chunk_hits(f.fw.data(), q[0], q[1], q[2], q[3], n - e * 8, [&](uint32_t x) { got.push_back(x); });
  }
  compare(f, member, got, "array chunks");
}

static void check_bitmap(const Filter& f, int density) {
  std::vector<uint8_t> member(65536, 0);
  std::vector<uint32_t> got;
  for (uint32_t wi = 0; wi < 1024; wi++) {
    uint64_t bits = (uint64_t(rnd32()) << 32) | rnd32();
    if (density == 0) bits &= (uint64_t(rnd32()) << 32) | rnd32();
    if (density == 2) bits = ~0ull;
    if (density == 3) bits = wi % 7 ? 0 : (1ull << 63) | 1ull;
    for (int b = 0; b < 64; b++) member[wi * 64 + b] = uint8_t((bits >> b) & 1);
    pk::fr_bitmap_word_hits(f.fw.data(), wi, bits, [&](uint32_t x) { got.push_back(x); });
  }
  compare(f, member, got, "bitmap words");
}

static void check_run(const Filter& f, uint32_t a, uint32_t b) {
  std::vector<uint8_t> member(65536, 0);
  for (uint32_t x = a; x <= b; x++) member[x] = 1;
  std::vector<uint32_t> got;
  pk::fr_run_hits(f.fw.data(), a, b, [&](uint32_t x) { got.push_back(x); });
  compare(f, member, got, "run");
}

static void check_filter(const Filter& f) {
  check_positions(f);
  for (int mode = 0; mode < 2; mode++)
    for (int n : {0, 1, 8, 9, 4096}) check_array(f, n, mode);
  for (int density = 0; density < 4; density++) check_bitmap(f, density);
  // runs inside one word, ending on bit 31 or 63, spanning many words, the whole key
  const uint32_t runs[][2] = {{5, 5},       {0, 0},         {65535, 65535}, {3, 17},      {32, 63},   {40, 63},
                              {0, 31},      {7, 31},        {64, 95},       {31, 32},     {63, 64},   {30, 33},
                              {100, 4000},  {0, 65535},     {1, 65534},     {4095, 8192}, {65504, 65535},
                              {65503, 65535}, {2016, 2047}, {2047, 2048}};
  for (const auto& r : runs) check_run(f, r[0], r[1]);
  for (int i = 0; i < 40; i++) {
    uint32_t a = rnd32() & 0xffff, b = rnd32() & 0xffff;
    if (a > b) { const uint32_t t = a; a = b; b = t; }
    check_run(f, a, b);
  }
}

int main() {
  {
    Filter f("empty");
    f.finish();
    check_filter(f);
  }
  {
    Filter f("full");
    for (auto& w : f.fw) w = ~0u;
    f.finish();
    check_filter(f);
  }
  for (int i = 0; i < 6; i++) {
    Filter f("random");
    for (auto& w : f.fw) w = i < 2 ? rnd32() : (i < 4 ? rnd32() & rnd32() & rnd32() : rnd32() | rnd32());
    f.finish();
    check_filter(f);
  }
  for (uint32_t x : {0u, 31u, 32u, 63u, 4095u, 32768u, 65504u, 65535u}) {
    Filter f("single bit");
    f.fw[x >> 5] = 1u << (x & 31);
    f.finish();
    check_filter(f);
  }
  fprintf(stderr, "%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
