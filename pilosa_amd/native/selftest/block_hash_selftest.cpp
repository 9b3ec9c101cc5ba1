// Stand-alone check of kernels/xxh64_state.h, the XXH64 state functions the
// block-checksum kernel (kernels/sync_kernels.hip) calls.  Built with
// -fsanitize=address,undefined by tests/test_block_hash_host.py and run
// directly.
//
// stdin: cases of "n digest piece" followed by n words, all hexadecimal except
// n and piece.  The words are the stream's positions; each enters the hash as
// bswap64(position), i.e. as 8 big-endian bytes.  They are fed the way the
// kernel feeds them: in pieces (piece sizes cycle through a fixed pattern
// starting at index `piece`), four accumulators taking word 4i + k of every
// whole stripe, the 0..3 words after the last whole stripe carried into the
// next piece, then finalise().  Every digest must equal the expected one.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../kernels/xxh64_state.h"

namespace {

const int PIECES[] = {3, 2, 1, 6, 5, 4096, 7, 4, 0, 16384, 1};

uint64_t hash_in_pieces(const std::vector<uint64_t>& pos, int piece) {
  uint64_t acc[4], carry[4], next[4];
  for (int k = 0; k < 4; k++) acc[k] = xxh::acc_init(k);
  int cn = 0;
  size_t at = 0;
  while (at < pos.size()) {
    size_t T = size_t(PIECES[piece++ % int(sizeof(PIECES) / sizeof(PIECES[0]))]);
    if (T > pos.size() - at) T = pos.size() - at;
    const uint64_t* stg = pos.data() + at;
    const int avail = cn + int(T), stripes = avail >> 2, rem = avail & 3;
    for (int k = 0; k < 4; k++) {        // lane k of the kernel
      for (int i = 0; i < stripes; i++) {
        const int idx = 4 * i + k;
        acc[k] = xxh::round(acc[k], xxh::bswap(idx < cn ? carry[idx] : stg[idx - cn]));
      }
      const int idx = 4 * stripes + k;
      if (k < rem) next[k] = idx < cn ? carry[idx] : stg[idx - cn];
    }
    for (int k = 0; k < rem; k++) carry[k] = next[k];
    cn = rem;
    at += T;
  }
  uint64_t left[3] = {0, 0, 0};
  for (int i = 0; i < cn; i++) left[i] = xxh::bswap(carry[i]);
  return xxh::finalise(acc, left, pos.size());
}

}  // namespace

int main() {
  int cases = 0, failures = 0;
  unsigned long long n;
  uint64_t want;
  int piece;
  while (std::scanf("%llu %" SCNx64 " %d", &n, &want, &piece) == 3) {
    std::vector<uint64_t> pos(n);
    for (auto& p : pos)
      if (std::scanf("%" SCNx64, &p) != 1) {
        std::fprintf(stderr, "case %d: truncated input\n", cases);
        return 2;
      }
    const uint64_t got = hash_in_pieces(pos, piece);
    if (got != want) {
      failures++;
      std::fprintf(stderr, "case %d (n=%llu piece=%d): got %016" PRIx64 " want %016" PRIx64 "\n", cases, n, piece,
                   got, want);
    }
    cases++;
  }
  std::fprintf(stderr, "%d cases, %d failures\n", cases, failures);
  return failures ? 1 : (cases ? 0 : 2);
}
