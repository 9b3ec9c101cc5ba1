// Wave-cooperative tile machinery of the expression evaluator, shared by the
// count / materialize kernels (bitmap_kernels.hip) and the BSI kernels
// (bsi_kernels.hip).  Include after kernels.h.
//
// One 64-lane wave owns one work item and walks the <=16 container keys of a
// row in a shard.  A container is held as a register "tile": 1024 u64 words
// spread over the wave, lane l owns words {128*i + 2*l + h | i<8, h<2} so every
// tile load is eight fully coalesced 1 KiB global_load_dwordx4
// wave-instructions.  Array and run containers are expanded into a
// wave-private 8 KiB LDS bitmap (ds_or_b64 scatter) and read back in the same
// layout.  Boolean query trees are compiled on the host to a tiny postfix
// program (<=32 ops, <=16 leaves) that the wave interprets with a 4-deep
// register stack (static register moves, no scratch).
#pragma once
#include "device_util.h"

namespace pk {

// one wave per work item, four to a workgroup
constexpr int WAVES_PER_BLOCK = 4;

static inline unsigned grid_for(int64_t items) {
  return unsigned((items + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK);
}

struct Tile {
  ulong2 w[8];
};

__device__ __forceinline__ void tile_zero(Tile& t) {
#pragma unroll
  for (int i = 0; i < 8; i++) t.w[i] = make_ulong2(0, 0);
}

__device__ __forceinline__ int tile_popc(const Tile& t) {
  int c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) c += __popcll(t.w[i].x) + __popcll(t.w[i].y);
  return c;
}

// Expand an array / run container into the wave-private LDS bitmap `lb`
// (1024 u64).  Caller reads it back.
__device__ __forceinline__ void lds_expand(uint64_t* lb, const uint16_t* payload, int64_t m) {
  const int lane = wave_lane();
  ulong2* l2 = reinterpret_cast<ulong2*>(lb);
#pragma unroll
  for (int i = 0; i < 8; i++) l2[i * 64 + lane] = make_ulong2(0, 0);
  lds_fence();
  const int type = meta_type(m);
  const uint16_t* p = payload + meta_off16(m) * 8;
  if (type == CT_ARRAY) {
    // 16-byte loads: 8 values per lane per instruction (payload is 16B aligned,
    // padded to a multiple of 8 values; the tail is masked by index).
    const int n = meta_n(m);
    const uint4* p4 = reinterpret_cast<const uint4*>(p);
    const int n8 = (n + 7) >> 3;
    for (int e8 = lane; e8 < n8; e8 += 64) {
      const uint4 v4 = p4[e8];
      const uint32_t w[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint32_t v = (w[k >> 1] >> ((k & 1) * 16)) & 0xffff;  // (val8() here changes the code)
        if (e8 * 8 + k < n) atomicOr(reinterpret_cast<unsigned long long*>(&lb[v >> 6]), 1ull << (v & 63));
      }
    }
  } else {  // run
    const int nr = p[0];
    for (int r = lane; r < nr; r += 64) {
      uint32_t s = p[8 + 2 * r], e = uint32_t(p[9 + 2 * r]) + 1;  // [s,e)
      uint32_t ws = s >> 6, we = (e - 1) >> 6;
      if (ws == we) {
        uint64_t mk = (e - s == 64) ? ~0ull : (((1ull << (e - s)) - 1) << (s & 63));
        atomicOr(reinterpret_cast<unsigned long long*>(&lb[ws]), mk);
      } else {
        atomicOr(reinterpret_cast<unsigned long long*>(&lb[ws]), ~0ull << (s & 63));
        for (uint32_t w = ws + 1; w < we; w++) lb[w] = ~0ull;
        uint32_t hb = e & 63;
        atomicOr(reinterpret_cast<unsigned long long*>(&lb[we]), hb ? ((1ull << hb) - 1) : ~0ull);
      }
    }
  }
  lds_fence();
}

__device__ __forceinline__ void tile_load(Tile& t, const uint16_t* payload, int64_t m, uint64_t* lb) {
  const int lane = wave_lane();
  if (meta_type(m) == CT_BITMAP) {
    const ulong2* p = reinterpret_cast<const ulong2*>(payload + meta_off16(m) * 8);
#pragma unroll
    for (int i = 0; i < 8; i++) t.w[i] = p[i * 64 + lane];
  } else {
    lds_expand(lb, payload, m);
    const ulong2* l2 = reinterpret_cast<const ulong2*>(lb);
#pragma unroll
    for (int i = 0; i < 8; i++) t.w[i] = l2[i * 64 + lane];
    lds_fence();
  }
}

template <int OP>
__device__ __forceinline__ void tile_op(Tile& a, const Tile& b) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    if (OP == OP_AND) { a.w[i].x &= b.w[i].x; a.w[i].y &= b.w[i].y; }
    if (OP == OP_OR) { a.w[i].x |= b.w[i].x; a.w[i].y |= b.w[i].y; }
    if (OP == OP_XOR) { a.w[i].x ^= b.w[i].x; a.w[i].y ^= b.w[i].y; }
    if (OP == OP_ANDNOT) { a.w[i].x &= ~b.w[i].x; a.w[i].y &= ~b.w[i].y; }
  }
}

__device__ __forceinline__ void tile_or(Tile& a, const Tile& b) { tile_op<OP_OR>(a, b); }

// Per-wave scratch in LDS.
struct WaveScratch {
  uint64_t lb[1024];          // 8 KiB expansion bitmap
  int64_t meta[MAXLEAF][16];  // container meta word per (leaf, j), -1 absent
};

// Build the (leaf, key) meta table for query `qp` in shard `s`; returns the
// presence mask of each leaf in `mask[]` (wave-uniform).  Lanes take
// (leaf, container) pairs -- 4 leaves per pass, passes unrolled -- so the
// rowptr and meta loads of all leaves are in flight together instead of one
// leaf's dependent chain after the other's; the key loops then read metas
// from LDS, not global memory.
__device__ __forceinline__ void build_slots(const QueryProg& qp, const ViewDev* views, int s, WaveScratch& ws,
                                            uint32_t* mask) {
  const int lane = wave_lane();
  for (int t = lane; t < MAXLEAF * 16; t += 64) (&ws.meta[0][0])[t] = -1;
  lds_fence();
  const int nleaf = qp.nleaf;
#pragma unroll
  for (int k0 = 0; k0 < MAXLEAF; k0 += 4) {
    const int k = k0 + (lane >> 4), idx = lane & 15;
    if (k0 < nleaf && k < nleaf) {
      const int64_t d = qp.leaf_row[k];
      if (d >= 0) {
        const ViewDev& v = views[qp.leaf_view[k]];
        const uint32_t* rp = v.rowptr + int64_t(s) * (v.D + 1);
        const int64_t base = v.shard_base[s];
        const int64_t lo = base + rp[d], hi = base + rp[d + 1];
        if (idx < hi - lo) {
          const int64_t m = v.meta[lo + idx];
          ws.meta[k][meta_j(m)] = m;
        }
      }
    }
  }
  lds_fence();
  for (int k0 = 0; k0 < MAXLEAF; k0 += 4) {
    const int k = k0 + (lane >> 4);
    const bool has = ws.meta[k][lane & 15] >= 0;
    const uint64_t b = __ballot(has);
#pragma unroll
    for (int i = 0; i < 4; i++) mask[k0 + i] = uint32_t((b >> (16 * i)) & 0xffff);
  }
}

// Candidate keys: evaluate the program over presence masks.
__device__ __forceinline__ uint32_t candidate_mask(const QueryProg& qp, const uint32_t* mask) {
  uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;  // s0 = top
  for (int pc = 0; pc < qp.nprog; pc++) {
    const int op = qp.prog[pc];
    if (op < OP_AND) {
      s3 = s2; s2 = s1; s1 = s0; s0 = mask[op];
    } else {
      uint32_t r;
      if (op == OP_AND) r = s1 & s0;
      else if (op == OP_ANDNOT) r = s1;
      else r = s1 | s0;  // OR, XOR
      s0 = r; s1 = s2; s2 = s3; s3 = 0;
    }
  }
  return s0;
}

// Evaluate the program for key j into `acc`.
__device__ __forceinline__ void eval_tile(const QueryProg& qp, const ViewDev* views, int s, int j, WaveScratch& ws,
                                          Tile& acc) {
  Tile t1, t2, t3;
  tile_zero(acc);
  tile_zero(t1);
  tile_zero(t2);
  tile_zero(t3);
  for (int pc = 0; pc < qp.nprog; pc++) {
    const int op = qp.prog[pc];
    if (op < OP_AND) {
      t3 = t2; t2 = t1; t1 = acc;
      const int64_t m = ws.meta[op][j];
      if (m < 0) tile_zero(acc);
      else tile_load(acc, views[qp.leaf_view[op]].payload, m, ws.lb);
    } else {
      // acc = t1 OP acc
      if (op == OP_AND) { tile_op<OP_AND>(t1, acc); }
      else if (op == OP_OR) { tile_op<OP_OR>(t1, acc); }
      else if (op == OP_XOR) { tile_op<OP_XOR>(t1, acc); }
      else { tile_op<OP_ANDNOT>(t1, acc); }
      acc = t1; t1 = t2; t2 = t3; tile_zero(t3);
    }
  }
}

// Count array values whose bit is set in the 1024-word bitmap `bm` (global or
// LDS); 16-byte loads of 8 values per lane.
__device__ __forceinline__ int probe_array(const uint64_t* bm, const uint16_t* arr, int n) {
  const int lane = wave_lane();
  const uint4* p4 = reinterpret_cast<const uint4*>(arr);
  const int n8 = (n + 7) >> 3;
  int c = 0;
  for (int e8 = lane; e8 < n8; e8 += 64) {
    const uint4 v4 = p4[e8];
    const uint32_t w[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint32_t v = (w[k >> 1] >> ((k & 1) * 16)) & 0xffff;
      const int hit = int((bm[v >> 6] >> (v & 63)) & 1);
      c += (e8 * 8 + k < n) ? hit : 0;
    }
  }
  return c;
}

// Flat fold: acc = l0; acc = acc op_i l_i.
__device__ __forceinline__ void load_leaf(const QueryProg& qp, const ViewDev* views, int s, int j, WaveScratch& ws,
                                          int k, Tile& t) {
  const int64_t m = ws.meta[k][j];
  if (m < 0) tile_zero(t);
  else tile_load(t, views[qp.leaf_view[k]].payload, m, ws.lb);
}

__device__ __forceinline__ void eval_flat(const QueryProg& qp, const ViewDev* views, int s, int j, WaveScratch& ws,
                                          Tile& acc) {
  load_leaf(qp, views, s, j, ws, qp.prog[0], acc);
  for (int pc = 1; pc + 1 < qp.nprog; pc += 2) {
    Tile t;
    load_leaf(qp, views, s, j, ws, qp.prog[pc], t);
    const int op = qp.prog[pc + 1];
    if (op == OP_AND) tile_op<OP_AND>(acc, t);
    else if (op == OP_OR) tile_op<OP_OR>(acc, t);
    else if (op == OP_XOR) tile_op<OP_XOR>(acc, t);
    else tile_op<OP_ANDNOT>(acc, t);
  }
}

// candidate_mask for the one key j, read from the meta table build_slots left
// in LDS: inside a loop over groups the mask[] array it indexes by opcode
// would live in scratch memory
__device__ __forceinline__ bool candidate_at(const QueryProg& qp, const WaveScratch& ws, int j) {
  bool s0 = false, s1 = false, s2 = false, s3 = false;  // s0 = top
  for (int pc = 0; pc < qp.nprog; pc++) {
    const int op = qp.prog[pc];
    if (op < OP_AND) {
      s3 = s2; s2 = s1; s1 = s0; s0 = ws.meta[op][j] >= 0;
    } else {
      bool r;
      if (op == OP_AND) r = s1 && s0;
      else if (op == OP_ANDNOT) r = s1;
      else r = s1 || s0;  // OR, XOR
      s0 = r; s1 = s2; s2 = s3; s3 = false;
    }
  }
  return s0;
}

}  // namespace pk
