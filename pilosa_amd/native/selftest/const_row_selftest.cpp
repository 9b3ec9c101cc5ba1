// Stand-alone check of kernels/const_row.h (the unit range search, the
// location split and the meta word of const_row_kernel, K30) on the host:
// build with -fsanitize=address,undefined and run directly.  Every case
// compares the header with a naive loop over the whole vector: random vectors
// (with duplicates), the empty one, a single element, every column in one
// unit, and a unit whose range ends exactly at the vector's end.  The vectors
// are heap blocks of exactly n elements, so a search that reads loc[n] or
// loc[-1] is an AddressSanitizer error.
// stderr ends with "<n> cases, <f> failures"; exit status 1 on any failure.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../kernels/const_row.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd64() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545f4914f6cdd1dull;
}

static int cases = 0, failures = 0;

// Unit u of the ascending vector v over S shards, the naive way: its range,
// its bitmap as 2048 words, its cardinality.
static void check_unit(const std::vector<int64_t>& v, int64_t u, const char* what) {
  const int64_t n = int64_t(v.size());
  int64_t* heap = new int64_t[size_t(n) + (n == 0)];  // exactly n readable elements (1 when n == 0, never read)
  std::copy(v.begin(), v.end(), heap);
  int64_t lo = 0;
  while (lo < n && (v[size_t(lo)] >> 16) < u) lo++;
  int64_t hi = lo;
  while (hi < n && (v[size_t(hi)] >> 16) == u) hi++;
  const int64_t glo = pk::const_row_lower_bound(heap, n, pk::const_row_unit_start(u));
  const int64_t ghi = pk::const_row_lower_bound(heap, n, pk::const_row_unit_start(u + 1));
  cases++;
  if (glo != lo || ghi != hi) {
    failures++;
    fprintf(stderr, "FAIL range %s n %lld unit %lld: [%lld, %lld) want [%lld, %lld)\n", what, (long long)n,
            (long long)u, (long long)glo, (long long)ghi, (long long)lo, (long long)hi);
  }
  // the bits the kernel would set, through the split, against the naive bitmap
  std::vector<uint32_t> got(2048, 0), want(2048, 0);
  for (int64_t i = glo; i < ghi; i++) {
    const pk::ConstRowBit p = pk::const_row_split(heap[i]);
    cases++;
    if (p.unit != u || p.word >= 2048 || p.bit >= 32) {
      failures++;
      fprintf(stderr, "FAIL split %s loc %lld: unit %lld word %u bit %u\n", what, (long long)heap[i],
              (long long)p.unit, p.word, p.bit);
      continue;
    }
    got[p.word] |= 1u << p.bit;
  }
  int64_t card = 0;
  for (int64_t i = 0; i < n; i++) {
    if ((v[size_t(i)] >> 16) != u) continue;
    const int64_t x = v[size_t(i)] % 65536;
    if (!((want[size_t(x / 32)] >> (x % 32)) & 1u)) card++;
    want[size_t(x / 32)] |= 1u << (x % 32);
  }
  cases++;
  if (got != want) {
    failures++;
    fprintf(stderr, "FAIL bitmap %s n %lld unit %lld\n", what, (long long)n, (long long)u);
  }
  // the meta word: key, type 2 (bitmap), cardinality, offset in 16-byte units
  const int64_t m = pk::const_row_meta(u, card);
  cases++;
  if ((m & 15) != u % 16 || ((m >> 4) & 3) != 2 || ((m >> 6) & 0x1ffff) != card ||
      int64_t(uint64_t(m) >> 23) != u * 512) {
    failures++;
    fprintf(stderr, "FAIL meta %s unit %lld card %lld: %llx\n", what, (long long)u, (long long)card, (long long)m);
  }
  delete[] heap;
}

static void check_vector(std::vector<int64_t> v, int S, const char* what) {
  std::sort(v.begin(), v.end());
  for (int64_t u = 0; u < int64_t(S) * 16; u++) check_unit(v, u, what);
}

int main() {
  // the empty vector
  check_vector({}, 3, "empty");
  // a single element: first unit, a middle one, the last column of the last unit
  check_vector({0}, 2, "single first");
  check_vector({(int64_t(1) << 20) | (7 << 16) | 31}, 3, "single middle");
  check_vector({(int64_t(2) << 20) | 0xfffff}, 3, "single last");
  // every column in one unit: word and key boundaries, a full container, duplicates
  {
    std::vector<int64_t> v;
    for (int64_t x : {0, 31, 32, 63, 64, 65535}) v.push_back((int64_t(1) << 20) | (5 << 16) | x);
    check_vector(v, 3, "one unit boundaries");
    v.clear();
    for (int64_t x = 0; x < 65536; x++) v.push_back((3 << 16) | x);
    check_vector(v, 1, "one unit full");
    for (int64_t x = 0; x < 65536; x += 3) v.push_back((3 << 16) | x);
    check_vector(v, 1, "one unit full with duplicates");
  }
  // a unit whose range ends exactly at the vector's end: the last unit of the
  // last shard, and a middle unit with nothing after it
  {
    std::vector<int64_t> v;
    for (int i = 0; i < 100; i++) v.push_back(int64_t(rnd64() % (3 << 20)));
    for (int64_t x : {0, 1, 65535}) v.push_back((int64_t(2) << 20) | (15 << 16) | x);
    check_vector(v, 3, "range ends at the end, last unit");
    v.clear();
    for (int64_t x : {5, 6, 7}) v.push_back((int64_t(1) << 20) | (2 << 16) | x);
    check_vector(v, 3, "range ends at the end, middle unit");
  }
  // key and shard boundaries
  check_vector({65535, 65536, (1 << 20) - 1, 1 << 20}, 2, "key and shard boundaries");
  // random vectors, sparse to dense, with duplicates
  for (int round = 0; round < 40; round++) {
    const int S = 1 + int(rnd64() % 4);
    const int64_t n = round < 10 ? int64_t(rnd64() % 8) : int64_t(rnd64() % 20000);
    std::vector<int64_t> v;
    for (int64_t i = 0; i < n; i++) {
      const int64_t loc = int64_t(rnd64() % (uint64_t(S) << 20));
      v.push_back(loc);
      if (rnd64() % 8 == 0) v.push_back(loc);
    }
    check_vector(v, S, "random");
  }
  fprintf(stderr, "%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
