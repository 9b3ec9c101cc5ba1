// Shared host/device declarations for the gfx950 bitmap kernels.
// The byte layouts of QueryProg / ViewDev / BsiArgs are mirrored by numpy
// structured dtypes in pilosa_amd/ops/device.py (static_asserts below pin them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pk {

constexpr int MAXLEAF = 16;
constexpr int MAXPROG = 32;
constexpr int ARRAY_MAX = 4096;
constexpr int RUN_MAX = 2048;
constexpr int CT_ARRAY = 1, CT_BITMAP = 2, CT_RUN = 3;
// opcodes: 0..MAXLEAF-1 push leaf k; then binary ops
constexpr int OP_AND = 32, OP_OR = 33, OP_XOR = 34, OP_ANDNOT = 35;

// container metadata word (see pilosa_amd/native/pyroaring.cpp)
__host__ __device__ __forceinline__ int meta_j(int64_t m) { return int(m & 15); }
__host__ __device__ __forceinline__ int meta_type(int64_t m) { return int((m >> 4) & 3); }
__host__ __device__ __forceinline__ int meta_n(int64_t m) { return int((m >> 6) & 0x1ffff); }
__host__ __device__ __forceinline__ int64_t meta_off16(int64_t m) { return int64_t(uint64_t(m) >> 23); }

struct QueryProg {
  int32_t nleaf;
  int32_t nprog;
  int32_t leaf_view[MAXLEAF];
  int64_t leaf_row[MAXLEAF];  // dense row index in the view, -1 = empty row
  uint8_t prog[MAXPROG];
  int64_t pad[3];
};
static_assert(sizeof(QueryProg) == 256, "QueryProg layout");

struct ViewDev {
  const uint32_t* rowptr;      // [S][D+1]
  const int64_t* shard_base;   // [S+1]
  const int64_t* meta;         // [C]
  const uint16_t* payload;     // [P]
  int64_t D;
  const uint16_t* keymask;     // [S][D] key-presence mask per (shard, row); nullptr = derive from meta
  // unused, always zero: they keep the offsets of the fields below
  uint64_t reserved0;
  uint64_t reserved1;
  // bitmap twins of the view's dense ARRAY rows (pair kernels, TWN): row d's
  // key-j container in shard s as a 1024-word bitmap at
  // twin + ((twin_slot[d] * S + s) * 16 + j) * 1024; nullptr / -1 = none; used
  // for a container only while it is an array of more than twin_cutoff values
  const uint64_t* twin;
  const int32_t* twin_slot;    // [D]
  int64_t twin_cutoff;
  // hot-pair table (pair_build): the per-shard intersection counts of the
  // view's hot_h hottest rows with each other, hot_counts[(s * hot_h + i) *
  // hot_h + j], read at (min, max) of the two slots: the build skips whole
  // 128 x 128 tiles strictly below the diagonal (they stay zero), so entries
  // with i > j exist only inside diagonal tiles (all of them for hot_h <= 128);
  // hot_slot[d] = slot of dense row d or -1; hot_valid[s] = 0 while shard s's
  // slice is stale.  nullptr / 0 = no table
  const int32_t* hot_counts;
  const int32_t* hot_slot;     // [D]
  const uint8_t* hot_valid;    // [S]
  int64_t hot_h;
};
static_assert(sizeof(ViewDev) == 120, "ViewDev layout");

struct BsiArgs {
  int32_t view;
  int32_t depth;
  int64_t row_exists;
  int64_t row_sign;
  int64_t bit_row[64];
};

void launch_expr_count(const QueryProg* progs, int Q, const ViewDev* views, int S, unsigned long long* out,
                       int32_t* per_key, int64_t* per_shard, int mode, hipStream_t st);
void launch_expr_materialize(const QueryProg* progs, int Q, const ViewDev* views, int S, const int32_t* counts,
                             const int64_t* offs, uint16_t* outp, hipStream_t st);
// Count(Intersect(a, b)) via key-major pair kernels (pair_kernels.hip):
// pairs = uint2[S*16*Q] scratch, partial = int32[S*16*Q] per-(shard,key,query) counts.
// out[ti[q]] += sum over the U rows of partial[U][n] (pair-kernel partials)
void launch_partial_sum_scatter(const int32_t* partial, int64_t U, int n, const int64_t* ti, int64_t* out,
                                int64_t nout, hipStream_t st);
// A query whose two rows both have a slot in their view's hot-pair table is
// answered by pair_build from the table (shipped variants 6 / 39 / 63 only).
void launch_and2_pairs(const QueryProg* progs, int Q, const ViewDev* views, int S, uint2* pairs, int32_t* partial,
                       int cq, int variant, hipStream_t st);
// The same batch summed into out[ti[q]], with the queries a table answers in
// every shard taken out of the pair grid on the device (pair_split_kernel).
// progs: the sorted KIND_AND2 part, ti its submission indices, views[V].
// work: and2_work_bytes(Q) bytes of 256-byte aligned scratch = counters
// {live, table-answered} | live programs | table-answered list | live ti.
// false = nothing launched: Q <= 128 or a variant / cq with no device-count
// instantiation (built: variants 6 and 63 at 32 / 64 queries per wave).
constexpr int64_t AND2_WORK_HEAD = 256;
inline int64_t and2_work_bytes(int64_t Q) { return AND2_WORK_HEAD + Q * int64_t(sizeof(QueryProg) + 16 + 8); }
bool launch_and2_total(const QueryProg* progs, int Q, const ViewDev* views, int V, int S, const int64_t* ti,
                       int64_t* out, int64_t nout, uint2* pairs, int32_t* partial, uint8_t* work, int cq,
                       int variant, hipStream_t st);
// BSI predicate -> one bitmap container per (shard, key): payload u16[S*16*4096], meta int64[S*16].
// op: 0 EQ, 1 NEQ, 2 LT, 3 LTE, 4 GT, 5 GTE, 6 BETWEEN, 7 NOT NULL (values are base-relative).
// out_count != nullptr: only add the matching column count (no view is written).
void launch_bsi_range(const ViewDev* views, int S, BsiArgs bsi, int op, int64_t p1, int64_t p2, uint16_t* out_payload,
                      int64_t* out_meta, unsigned long long* out_count, hipStream_t st);
// BSI min/max descents per (shard, key): out int64[S*16*10] (see bsi_kernels.hip).
// the [F fragments x G keys x 10] descents -> out int64[3] {value, count, found}
// part: int64[4 * ceil(F / 64)] scratch of the multi-block fold (G == 16), or nullptr
void launch_bsi_minmax_fold(const int64_t* o, int F, int G, int is_min, int64_t* out, int64_t* part,
                            hipStream_t st);
void launch_bsi_minmax(const QueryProg* progs, const ViewDev* views, int S, BsiArgs bsi, int64_t* out,
                       hipStream_t st, int which = 0);
// Percentile(field=, nth=): exact rank selection by an MSB-first descent whose
// branch at each bit is global (bsi_kernels.hip bsi_kth_*).  One step of
// the chain, shared by the step kernel (every wave replays the bits already
// decided) and the host (the final replay): the current candidate set holds
// ``tot`` values of which ``c1`` have the bit set, ``r`` is the 0-based rank
// sought inside it -- counted from the smallest magnitude (largest_first = 0,
// non-negative answers) or from the largest (1, negative answers).  Returns
// the bit and narrows (r, tot) to the branch taken.
__host__ __device__ inline int kth_chain(int largest_first, uint64_t c1, uint64_t& r, uint64_t& tot) {
  const uint64_t c0 = tot - c1;
  if (largest_first) {
    if (r < c1) { tot = c1; return 1; }
    r -= c1; tot = c0; return 0;
  }
  if (r < c0) { tot = c0; return 0; }
  r -= c0; tot = c1; return 1;
}
constexpr int KTH_CNT = 2 + 64;  // cnt[0] = N, cnt[1] = Nneg, cnt[2 + i] = cnt1[i]
// init: cand[S*16][1024] = exists & filter per (shard, key); cnt[0] += |cand|, cnt[1] += |cand & sign|
void launch_bsi_kth_init(const QueryProg* progs, const ViewDev* views, int S, BsiArgs bsi, uint64_t* cand,
                         unsigned long long* cnt, hipStream_t st);
// step for bit i (depth-1 .. 0): narrow cand by the decision on bit i+1 (the
// sign restriction at i == depth-1), cnt[2 + i] += |cand & plane i|
void launch_bsi_kth_step(const ViewDev* views, int S, BsiArgs bsi, uint64_t* cand, unsigned long long* cnt, int i,
                         uint64_t r, uint64_t tot, int largest_first, hipStream_t st);
// fmode: 0 no filters, 1 flat-fold filter programs, 2 any program.
void launch_bsi_sum(const QueryProg* progs, int Q, const ViewDev* views, int S, BsiArgs bsi,
                    unsigned long long* out_sum, unsigned long long* out_cnt, int fmode, hipStream_t st);
// GroupBy(..., aggregate=Sum(field=)): out_sum[g] / out_cnt[g] += the BSI sum
// (base-relative) / column count of group program g, G programs past LDS-staged
// planes (bsi_group_sum_kernel).  planes = bit planes per LDS slab (clamped to
// 1 .. GS_MAX_PLANES and to the depth), gchunk = groups per workgroup, fmode
// 1 = every program is a flat fold, 2 = any program.  Returns the slabs run,
// -1 when the grid would not fit.
constexpr int GS_MAX_PLANES = 13;
int launch_bsi_group_sum(const QueryProg* progs, int G, const ViewDev* views, int S, BsiArgs bsi, int planes,
                         int gchunk, int fmode, unsigned long long* out_sum, unsigned long long* out_cnt,
                         hipStream_t st);

// The slab kernels K26 / K27 / K29 below (bsi_slab.h): one workgroup per (arena
// shard, key, slice of n tile slots), the slice staged into fixed_tiles + depth
// LDS tiles of n KiB next to the four WaveScratch.  slab_slots() = the tile
// slots per workgroup: the largest of 8, 4, 2, 1 that fits the CU's 160 KiB at
// this depth, or want rounded down to a power of two where that is smaller
// (want < 1: no wish).
constexpr int64_t SLAB_STATIC_LDS = 40960;  // four WaveScratch (bsi_slab.h asserts it)
inline int slab_slots(int fixed_tiles, int depth, int want) {
  int n = 8;
  while (n > 1 && SLAB_STATIC_LDS + int64_t(fixed_tiles + depth) * n * 1024 > 160 * 1024) n >>= 1;
  if (want >= 1 && want < n) {
    int w = 1;
    while (w * 2 <= want) w <<= 1;  // round down to a power of two
    n = w;
  }
  return n;
}
inline int64_t slab_blocks(int S, int n) { return int64_t(S) * 16 * (8 / n); }
inline int slab_lds_bytes(int fixed_tiles, int depth, int n) { return (fixed_tiles + depth) * n * 1024; }

// Distinct(field=) (distinct_kernels.hip, K26): bit v of pos / neg |= 1 for
// every column of exists & filter (progs[0]; nprog == 0: no filter) holding the
// base-relative value +v / -v; pos and neg hold 2^depth bits each (at least one
// 32-bit word), zeroed by the caller.  depth <= DISTINCT_MAX_PLANES.  slots =
// tile slots per workgroup (1, 2, 4 or 8; anything else: the largest that
// fits), clamped by distinct_slots() = slab_slots() to what the 160 KiB of LDS
// hold at this depth.  mark: 0 always OR, 1 test the bit first, 2 also skip a repeat of the
// thread's previous value.  Returns the slots used, -1 when nothing was launched
// (depth out of range, grid too large).
constexpr int DISTINCT_MAX_PLANES = 32;
constexpr int DISTINCT_FIXED_TILES = 2;  // consider, sign
inline int distinct_slots(int depth, int want) { return slab_slots(DISTINCT_FIXED_TILES, depth, want); }
int launch_bsi_distinct(const QueryProg* progs, const ViewDev* views, int S, BsiArgs bsi, int slots, int mark,
                        uint32_t* pos, uint32_t* neg, hipStream_t st);

// Extract(filter, Rows(field=)) (extract_kernels.hip, K27): for every column of
// the filter progs[0] (nprog >= 1), in ascending column order, columns[o] = the
// global column id (col_base[s] + the column's offset in arena shard s),
// values[o] = its real value in the BSI field (base applied; 0 without one),
// valid[o] = 1 when it has one.  unit_off[s * 16 + j] = the output position of
// the first column of (shard, key), an exclusive prefix sum of the filter's
// per-unit counts; -1 = skip the unit.  cap = the length of the output vectors:
// no store goes past it.  columns == nullptr: leave the column vector alone.
// depth <= EXTRACT_MAX_PLANES.  slots as for launch_bsi_distinct, clamped by
// extract_slots().  Returns the slots used, -1 when nothing was launched.
constexpr int EXTRACT_MAX_PLANES = 32;
constexpr int EXTRACT_FIXED_TILES = 3;  // consider, exists, sign
inline int extract_slots(int depth, int want) { return slab_slots(EXTRACT_FIXED_TILES, depth, want); }
int launch_bsi_extract(const QueryProg* progs, const ViewDev* views, int S, BsiArgs bsi, int slots,
                       const int64_t* unit_off, const int64_t* col_base, int64_t base, int64_t cap, uint64_t* columns,
                       int64_t* values, uint8_t* valid, hipStream_t st);

// Sort(<filter>, field=, limit=) (sort_kernels.hip, K29): the selection pass
// over consider = exists & progs[0] (nprog == 0: exists alone).  The selected
// columns are those whose base-relative value sorts before T (< T, or > T with
// desc) and the first m[0] columns, in column order, whose value is T;
// select_all != 0 selects every considered column and ignores T.  One
// workgroup per (arena shard, key, slice of n tile slots), sort_blocks(S, n) of
// them, in column order; both modes must run with the same slots.
//   mode 1 (count): counts[2 w] / counts[2 w + 1] = workgroup w's columns
//     before T / equal to T (int32; zeroed by the caller: an empty workgroup
//     stores nothing).  The other pointers are not read.
//   mode 2 (fill): before_off / eq_before = the exclusive prefix sums of the
//     two counts over the workgroups, m = one int64 on the device.  For every
//     selected column, in ascending column order, columns[o] = its global
//     column id (col_base[s] + the column's offset in arena shard s) and
//     values[o] = its real value (base applied).  cap = the length of both
//     vectors: no store goes past it.
// depth <= SORT_MAX_PLANES and |T| < 2^32.  slots as for launch_bsi_distinct,
// clamped by sort_slots().  Returns the slots used, -1 when nothing was
// launched.
constexpr int SORT_MAX_PLANES = 32;
constexpr int SORT_FIXED_TILES = 2;  // consider, sign
inline int sort_slots(int depth, int want) { return slab_slots(SORT_FIXED_TILES, depth, want); }
inline int64_t sort_blocks(int S, int n) { return slab_blocks(S, n); }
int launch_bsi_sort_select(int mode, const QueryProg* progs, const ViewDev* views, int S, BsiArgs bsi, int slots,
                           int select_all, int desc, int64_t T, int32_t* counts, const int64_t* before_off,
                           const int64_t* eq_before, const int64_t* m, const int64_t* col_base, int64_t base,
                           int64_t cap, int64_t* columns, int64_t* values, hipStream_t st);

// Extract(filter, Rows(field=)) for a set-like field (extract_rows_kernels.hip,
// K28): every hit of a dense row d < D of views[fview] on the filter progs[0]
// at an output position pos < cap (unit_off / col_base / the positions as for
// launch_bsi_extract; cap = the window's length).  One workgroup per (shard,
// key, chunk of rows_per_block rows; 0 = all rows), rows_per_wave as for
// launch_row_filter_counts; rows_extract_blocks() is the grid, which the two
// list passes must share.  mode 1 (count): wg[block] = the workgroup's hits
// (zeroed by the caller).  mode 2 (fill): wg = the exclusive cumsum of the
// counts, keys[base + slot] = pos * D + d, no store at or past T.  mode 3
// (scalar): first[pos] = min(first[pos], row_ids[d]), first[cap] initialised
// to all ones.  columns != nullptr: the launch also writes the column vector
// (>= cap entries).  Returns the workgroups launched, -1 when nothing was
// launched (grid too large, bad mode).
int64_t rows_extract_blocks(int S, int64_t D, int64_t rows_per_block);
int64_t launch_rows_extract(int mode, const QueryProg* progs, const ViewDev* views, int S, int fview, int64_t D,
                            int64_t rows_per_block, int rows_per_wave, const int64_t* unit_off,
                            const int64_t* col_base, int64_t cap, uint64_t* columns, int64_t* wg, int64_t* keys,
                            int64_t T, const uint64_t* row_ids, uint64_t* first, hipStream_t st);

// TopK(field=, k=) (topk_kernels.hip, K25): out[d] +=|row d ∩ filter| over
// the S arena shards for every dense row d of ``fv``; the filter is dense row
// ``xd`` of ``*xv`` (same shard list), staged once per (shard, key) in LDS.
// xv == nullptr: no filter, out[d] += |row d| from the metadata alone.
// rows_per_block > 0 splits the rows of a (shard, key) over several
// workgroups, 0 = one workgroup per (shard, key); rows_per_wave = rows a wave
// looks up per step (16, 32 or 64; anything else: chosen from the rows of a
// workgroup).  out must hold fv.D words.
// Returns the workgroups launched, -1 when the grid would not fit.
int64_t launch_row_filter_counts(const ViewDev& fv, const ViewDev* xv, int64_t xd, int S, int64_t rows_per_block,
                                 int rows_per_wave, unsigned long long* out, hipStream_t st);

// Device TopN slot index (topn_kernels.hip): pass 1 counts cached-row bits per
// column into colcnt[S*2^20]; pass 2 (fill) scatters cache slots behind the
// per-shard exclusive scan colptr[S][2^20+1] (colcnt reused as cursors).
void launch_topn_index(const ViewDev& v, int S, int K, int k0, const int32_t* cache_dense, uint32_t* colcnt,
                       const uint32_t* colptr, const int64_t* entbase, uint16_t* slots, bool fill, hipStream_t st);
// Arguments of the src-TopN kernel.  Rows are addressed in an "acc space" of
// A sorted row ids (identical on every rank of a node).
struct TopNLaunch {
  ViewDev v;                      // the TopN field's view (fallback probes)
  int Q, S, K;                     // queries, shards (fragments), cache slots
  int H32, H16;                   // counter tiers: u32 < H32 <= u16 < H16 <= u8
  int64_t A;                      // acc-space size
  const int32_t* src_counts;      // [Q*S*16] materialised src containers
  const int64_t* src_offs;        // [Q*S*16] u16 offsets into src_vals
  const uint16_t* src_vals;       // array (n <= 4096) or bitmap (4096 u16)
  const uint32_t* colptr;         // [S][2^20+1] per-shard entry offsets
  const int64_t* entbase;         // [S] first slot entry of each shard
  const uint16_t* slots;          // cache slot per (column, cached row)
  int64_t slots_n;                // entries allocated (>= used + 16, multiple of 8)
  const int32_t* cache_cnt;       // [S][K] cached counts (desc), 0 = empty
  const int32_t* cache_acc;       // [S][K] acc index of each slot's row
  const int32_t* slotmap;         // [S][A] cache slot of each acc row, -1
  const int32_t* a2dense;         // [A] dense row in v, -1 = absent here
  const int32_t* ns;              // [Q] n (0 = unlimited)
  const int32_t* min_threshold;   // [Q]
  int32_t* acc;                   // mode 1: [Q][A] summed pushed counts
  const int64_t* pair_off;        // mode 2: [Q+1]
  const int32_t* pair_idx;        // mode 2: [P] acc index of each id
  unsigned long long* out;        // mode 2/3: [P] summed counts >= threshold
  uint32_t* hist_out;             // mode 1 (optional): [Q*S][words] kept histograms
  const uint32_t* hist_in;        // mode 3: histograms kept by mode 1
  int R;                          // hot ranks [0, R) counted by mode 4; slot index / histogram cover [R, K)
  const int32_t* hot_meta;        // [S][16][R] key-j container of each hot row (meta index in shard), -1
  const int32_t* hot_split;       // [S][16][2] ranks before [0] hold containers over the lane-owned bound,
                                  // before [1] the cooperative ones (bitmaps, runs, arrays > HOT_MID_N)
  uint32_t* hot_cnt;              // [S][Q][R] src counts of the hot ranks (mode 4 writes, 1-3 read)
  int32_t* tail_built;            // [Q*S] mode 1: 1 = unit's tail histogram built (kept), 0 = skipped
  const int32_t* cache_dense;     // [S][K] dense row of each cache slot (mode 3 exact probes)
  int M;                          // arena sub-shards per fragment (S fragments, S*M device shards: src, colptr,
                                  // entbase, slots, hot_meta/split are per sub-shard; mode 4 runs with S*M, M=1)
  int tbuild_min;                 // mode 4: bitmap srcs of >= this many bits build the table by transpose
  int dbg;                        // PILOSA_TOPN_DBG cost isolation: 1 skip histogram, 2 skip walk, 8 skip small hot rows,
                                  // 16 skip big hot rows, 32 skip their bitmaps, 64 skip their arrays,
                                  // 256 no lane-owned / mid atomics, 512 table skips bitmap srcs, 1024
                                  // bitmap srcs by LDS atomics (not the transposed build), 2048 skip mid-size rows, 4096
                                  // lane-owned rows load but do not count, 8192 phase 1 adds nothing to acc
                                  // (answers then wrong, except 1024)
};
// LDS bytes of the (query, shard) slot histogram (u32 / u16 / u8 tiers).
int topn_lds_bytes(int K, int H32, int H16);
// mode 1: phase-1 heap walk -> acc[Q][A] (+ hist_out); mode 2: ids= re-count
// -> out[P] (rebuilds the histograms); mode 3: ids= re-count from hist_in.
// mode 4: hot-rank count matrix hot_cnt (row-major over the batch).
void launch_topn_src(const TopNLaunch& a, int mode, hipStream_t st);
// Src containers (counts / u16 offsets into the arena payload) of plain
// rows; *has_run set when a run container needs materialising.
void launch_leaf_src(const ViewDev& v, const int64_t* rows, int Q, int S, int32_t* counts, int64_t* offs,
                     int32_t* has_run, hipStream_t st);
// twin[r][s][j] = row rows[r]'s key-j container of shard s as a bitmap
void launch_twin_build(const ViewDev& v, int S, const int32_t* rows, int R, uint64_t* twin, hipStream_t st);
void launch_keymask_build(const ViewDev& v, int S, uint16_t* out, hipStream_t st);
// Row counts of (shard, dense row) entries -> out[N] (device rank caches).
void launch_row_counts(const ViewDev& v, const int32_t* shard_of, const int32_t* dense, int64_t N, int32_t* out,
                       hipStream_t st);
// out[p] = sum over shards of row dense[p]'s count where >= threshold[p] (ids= re-count, no src).
void launch_row_counts_sum(const ViewDev& v, int S, const int32_t* dense, const int32_t* threshold, int P,
                           unsigned long long* out, hipStream_t st);
// Cache-only TopN: cm[j*S + s] = candidate u[j]'s count in shard s (memoised per rank-cache prefix).
void launch_topn_cache_counts(const ViewDev& v, int S, const int32_t* u, int U, int32_t* cm, hipStream_t st);
// Cache-only TopN batch: membership, per-threshold totals and per-query top-n
// (prm = lim[Q] | mt[Q] | tsel[Q] | nq[Q] | th[T]; out[Q, KK+1], column 0 = rows kept or -2 on overflow).
void launch_topn_cache_batch(const int32_t* cnt, int K, int S, int nmax, const int32_t* inv, const int32_t* u,
                             const int32_t* cm, const int32_t* prm, int Q, int T, int U, int KK, uint8_t* member,
                             long long* tot, long long* out, hipStream_t st, int nlim = 0, int mark = 0);
// Mesh cache-only TopN: one rank's buffer [member bytes | int32 totals[T, U] | flags[2]] (cleared here;
// flags = this rank's [stale, declined] vote, which rides in the batch's one all-reduce) and the front
// end's select over the reduced buffer (out[q, 0] = -3 / -4 when some rank was stale / declined).
void launch_topn_cache_partial(const int32_t* cnt, int K, int S, int nmax, int nlim, const int32_t* inv,
                               const int32_t* cm, const int32_t* prm, int Q, int T, int U, uint8_t* member,
                               int32_t* tot, int32_t* flags, int stale, int declined, hipStream_t st);
void launch_topn_cache_select32(const uint8_t* member, const int32_t* tot, const int32_t* ids, const int32_t* prm,
                                int Q, int U, int KK, long long* out, const int32_t* flags, hipStream_t st);
void launch_topn_hot_meta(const ViewDev& v, int S, int K, int R, const int32_t* cache_dense, int32_t* hot_meta,
                          int32_t* hot_split, hipStream_t st);

// Row-pair intersection count matrix C[M][N] (int32, atomically accumulated)
// of dense bit rows A[M][KW] and B[N][KW] (u64 words), bitgemm.hip.
// mode 1: i8 MFMA (v_mfma_i32_32x32x32_i8), mode 0: VALU popcount.
// c_split_stride > 0: K-split y adds into C + y * c_split_stride instead (one
// matrix per split; with KW / splits = 16384 words of densify output, one per
// shard).  skip_lower: tiles strictly below the diagonal are not computed
// (A and B the same rows: C is symmetric, read it at (min, max)).  With a
// split stride every entry of a computed tile is stored, not added (C needs no
// clearing; skipped tiles are left as they are).
void launch_bitgemm(const uint64_t* A, const uint64_t* B, int M, int N, int64_t KW, int splits, int mode,
                    int32_t* C, hipStream_t st, int64_t c_split_stride = 0, bool skip_lower = false);
// K-splits launch_bitgemm runs for these arguments (rows of a per-split C).
int bitgemm_splits(int64_t KW, int splits, int mode);
// Dense bit rows of an arena: out[R][(s1-s0) * 16384] u64 for dense rows `rows`.
void launch_densify(const ViewDev& v, const int64_t* rows, int R, int s0, int s1, uint64_t* out, hipStream_t st);

// Dense one-row result views: container (q, s, j) is a bitmap at u16 offset
// ((q*S + s)*16 + j) * 4096 of outp; out_meta[(q*S + s)*16 + j] its metadata.
void launch_expr_dense(const QueryProg* progs, int Q, const ViewDev* views, int S, uint16_t* outp, int64_t* out_meta,
                       hipStream_t st);
// Shift a dense view (u64[S][16384]) up by n (0 < n < 2^20) columns per shard:
// main_out = bits that stay in the shard, spill_out = bits carried into the
// next shard (both dense, with metadata like launch_expr_dense).
void launch_shift_dense(const uint64_t* src, int S, int M, int64_t n, int64_t row_words, uint64_t* main_out,
                        int64_t* main_meta, uint64_t* spill_out, int64_t* spill_meta, hipStream_t st);
// ConstRow (const_row_kernels.hip, K30): the columns at the ascending
// locations loc[0, n) (si << 20 | offset) as a dense one-row view, one bitmap
// and one meta word per (shard, key) unit, every unit written.
void launch_const_row(const int64_t* loc, int64_t n, int S, uint16_t* payload, int64_t* meta, hipStream_t st);
// Rows listing: flags[d] = 1 for dense rows with a non-empty container in
// shards [s0, s0 + ns) (j >= 0: only rows whose key-j container holds col16).
void launch_rows(const ViewDev& v, int s0, int ns, int j, uint32_t col16, uint8_t* flags, hipStream_t st);

// Device write path (write_kernels.hip).  merge: one workgroup per touched
// container u -> scratch[u][1024] u64 bitmap + card[u]; mode 0 applies sorted
// u16 lows dlows[dstart[u], dstart[u+1]), mode 1 the delta container dmeta[u]
// (arena metadata into dpayload, -1 none); old_meta[u] = -1 for a new
// container; nruns[u] = its number of runs.  emit: final container u at u16
// offset off16[u]*8 of payload, encoded by the reference's Optimize rule
// (run / array / bitmap), and its metadata word (-1 if empty).
void launch_container_merge(const int64_t* old_meta, const uint16_t* payload, int64_t U, const int32_t* dstart,
                            const uint16_t* dlows, const int64_t* dmeta, const uint16_t* dpayload, int mode,
                            bool clear, uint64_t* scratch, int32_t* card, int32_t* nruns, hipStream_t st);
// Copy every live container (meta type != 0) of size size16[c] 16-byte units
// from src to new_off16[c] of dst (payload compaction).
void launch_payload_compact(const int64_t* meta, int64_t C, const int64_t* new_off16, const int64_t* size16,
                            const uint16_t* src, uint16_t* dst, hipStream_t st);
void launch_container_emit(const uint64_t* scratch, const int32_t* card, const int32_t* nruns, const int64_t* off16,
                           const int32_t* jkey, int64_t U, uint16_t* payload, int64_t* meta_out, hipStream_t st);

// Anti-entropy read path (sync_kernels.hip).  units[u] = {first arena shard of
// the fragment, d0, d1}: the dense rows [d0, d1) of one 100-row block over the
// fragment's M sub-shards; rows[D] = the view's row directory; e = the shard
// width exponent.  block_hash: out_n[u] = set positions of unit u (0 = no
// block), out_h[u] = XXH64 over them as big-endian u64 in ascending order
// (launched in chunks of 2^16 units).  block_dump: one unit's positions
// row << e | column in that order into out[0 .. cap).
void launch_block_hash(const ViewDev& v, const int32_t* units, int64_t U, int M, int e, const int64_t* rows,
                       int64_t* out_n, uint64_t* out_h, hipStream_t st);
void launch_block_dump(const ViewDev& v, const int32_t* unit, int M, int e, const int64_t* rows, uint64_t* out,
                       int64_t cap, hipStream_t st);

}  // namespace pk
