// Poseidon2 Merkle tree kernels (see merkle.h).  MerkleTree::new [p3-recalled]:
//   leaf i  = sponge(row i of every tallest matrix, concatenated in commit order)
//   node j  = compress(left, right); if matrices of height == this layer exist,
//             node = compress(node, sponge(row j of those matrices))
// One thread per row/node (16 lanes per row/node in short trees and layers); leaf rows are read
// column by column so every load of a wave is a contiguous 256-byte segment.  Any number of
// matrices at any heights: a launch's columns travel in the kernel arguments up to MAXSEG
// matrices, else in the tree's column table.
#include <algorithm>

#include "merkle.h"
#include "poseidon2.h"

// (Throughput Poseidon2 kernels at 7 or 8 waves per SIMD ran within noise of the compiler's
// 5-6: profiles/r03/ab_p2_occupancy.txt.)

namespace bfz {

using namespace kb;

// The columns hashed by one launch: matrices ("segments", merkle.h ColSeg) in commit order, each
// with at least one column.  Up to MAXSEG of them travel in the kernel arguments (ColList); a
// longer list is a range of the tree's table in device memory (ColTable), read by the `_tab`
// form of each kernel.  Both forms share every kernel body (templates over the list type).
constexpr int MAXSEG = 16;
struct ColList {
  ColSeg seg[MAXSEG];
  int nseg;
  int n;  // columns of all segments
};
struct ColTable {
  const ColSeg* seg;  // the range's first segment (MerkleTree::col_table + its index)
  int nseg;
  int n;
};
__device__ __forceinline__ ColSeg seg_at(const ColList& cl, int i) { return cl.seg[i]; }
// No kernel writes the table: it is read through the constant address space, where a uniform
// index gives scalar loads.
__device__ __forceinline__ ColSeg seg_at(const ColTable& ct, int i) {
  const auto* s = (const __attribute__((address_space(4))) ColSeg*)ct.seg + i;
  return ColSeg{s->base, s->stride, s->n};
}

// A walk over a list's columns in order.  The walk is wave-uniform and the list sits in the
// kernarg segment, or is read through a uniform address, so its state lives in SGPRs: a step to
// the next column is a scalar add, and only a segment's end loads anything (the next segment's
// base / stride / count, by scalar loads in either form).
template <class CL>
struct ColWalk {
  const uint32_t* p;  // the next column
  size_t stride;
  int left;           // columns left in segment s, p's included
  int s;
  __device__ __forceinline__ void enter(const CL& cl, int seg) {
    s = seg;
    p = nullptr;
    stride = 0;
    left = 0;
    if (seg < cl.nseg) {
      const ColSeg g = seg_at(cl, seg);
      p = g.base;
      stride = g.stride;
      left = g.n;
    }
  }
  // Past the list's last column the walk stays on it: a caller may always load through the
  // returned pointer (a short chunk's surplus loads re-read that column and are not used).
  __device__ __forceinline__ const uint32_t* next(const CL& cl) {
    const uint32_t* r = p;
    if (left > 1) {
      left--;
      p += stride;
    } else if (s + 1 < cl.nseg) {
      enter(cl, s + 1);
    }
    return r;
  }
  // k steps of next() at once (a list with at least one column): one multiply-add per segment
  // passed; past the list's end the walk stays on its last column, as next() does.
  __device__ __forceinline__ void skip(const CL& cl, int k) {
    while (k > 0) {
      if (left > k) {
        left -= k;
        p += (size_t)k * stride;
        return;
      }
      if (s + 1 >= cl.nseg) {
        p += (size_t)(left - 1) * stride;
        left = 1;
        return;
      }
      k -= left;
      enter(cl, s + 1);
    }
  }
  // Lane mode: the next m <= 8 columns, lane k < m getting column k's pointer (one multiply-add
  // per segment the chunk touches, no per-lane search).
  __device__ __forceinline__ const uint32_t* next_lanes(const CL& cl, int m, int lane) {
    const uint32_t* r = nullptr;
    for (int k0 = 0; k0 < m && left > 0;) {
      const int take = m - k0 < left ? m - k0 : left;
      const int k = lane - k0;
      if (k >= 0 && k < take) r = p + (size_t)k * stride;
      k0 += take;
      if (left > take) {
        left -= take;
        p += (size_t)take * stride;
      } else {
        enter(cl, s + 1);
      }
    }
    return r;
  }
};

// Word `off4 / 4` of a column.  A 32-bit byte offset keeps the address a scalar base plus one
// VGPR (make_cols refuses columns longer than 4 GiB).
__device__ __forceinline__ uint32_t ld_col(const uint32_t* col, uint32_t off4) {
  // (a column pointer read from a table has lost its address space: see kb.h ld_global)
  return *(const __attribute__((address_space(1))) uint32_t*)(
      (const __attribute__((address_space(1))) char*)col + off4);
}

// The next 8 columns' words of one row (a list with at least one column; see ColWalk::next for
// the list's end).  Straight-line: eight loads in flight together.
template <class CL>
__device__ __forceinline__ void load_chunk(uint32_t nx[8], ColWalk<CL>& w, const CL& cl,
                                           uint32_t off4) {
#pragma unroll
  for (int k = 0; k < 8; k++) nx[k] = ld_col(w.next(cl), off4);
}

// Overwrite-mode absorb: st[0..m) = nx[0..m).
__device__ __forceinline__ void take_chunk(uint32_t st[16], const uint32_t nx[8], int m) {
  if (m == 8) {
#pragma unroll
    for (int k = 0; k < 8; k++) st[k] = nx[k];
  } else {
#pragma unroll
    for (int k = 0; k < 7; k++) st[k] = k < m ? nx[k] : st[k];
  }
}

// PaddingFreeSponge of one row over the list's columns, st zero on entry; only st[0..8) (the
// digest) is finished on return.  The first permutation starts from a zero capacity, one that
// a full chunk follows leaves st[0..8) unfinished (overwritten unread), the last one st[8..16).
// (Issuing a chunk's loads before the previous chunk's permutation, 8 more VGPRs, was no
// faster in either kernel, and holding them to the old 6 / 5 waves per SIMD was slower:
// profiles/r07/ab_merkle_ends.txt.)
template <class CL>
__device__ __forceinline__ void sponge_cols(uint32_t st[16], const CL& cl, uint32_t off4) {
  ColWalk<CL> w;
  w.enter(cl, 0);
  bool first = true;
  for (int rest = cl.n; rest > 0; first = false) {
    const int m = rest < 8 ? rest : 8;
    uint32_t nx[8];
    load_chunk(nx, w, cl, off4);
    take_chunk(st, nx, m);
    rest -= m;
    poseidon2_permute_ends(st, first, rest < 8, rest > 0);
  }
}

// Rows [r0, r0 + count) (a shard's range; the whole matrix when unsharded).
template <class CL>
__device__ __forceinline__ void hash_leaves(const CL& cl, size_t r0, size_t count,
                                            uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const size_t r = r0 + i;
  uint32_t st[16];
#pragma unroll
  for (int i = 0; i < 16; i++) st[i] = 0;
  sponge_cols(st, cl, (uint32_t)r * 4u);
  uint4* o = reinterpret_cast<uint4*>(out + 8 * r);
  o[0] = make_uint4(st[0], st[1], st[2], st[3]);
  o[1] = make_uint4(st[4], st[5], st[6], st[7]);
}
__global__ __launch_bounds__(256) void k_hash_leaves(ColList cl, size_t r0, size_t count,
                                                     uint32_t* __restrict__ out) {
  hash_leaves(cl, r0, count, out);
}
__global__ __launch_bounds__(256) void k_hash_leaves_tab(ColTable cl, size_t r0, size_t count,
                                                         uint32_t* __restrict__ out) {
  hash_leaves(cl, r0, count, out);
}

// Leaves of a short tree (at most LANE_LAYER_MAX rows) in lane mode: the thread kernel above is
// then a few waves, each paying the single-thread permutation latency once per chunk.  A block
// of 1024 threads owns LEAF_ROWS = 64 consecutive rows, 16 lanes per row (lane l holds word l of
// the row's sponge state), so a chunk costs one lane-mode permutation latency.
// Data movement: the 16 lanes of a row do not gather their chunk from 8 columns (a wave would
// fetch 4-row, 16-byte pieces from 8 places).  The block stages column tiles in LDS instead:
// wave w of the 16 loads rows [0, 64) of column 16 * round + w, one contiguous 256-byte
// segment, so a round brings 16 columns = two chunks.  The loaded word waits in a register while
// the previous round's two chunks are permuted, and lands in the other of two tiles, so one
// barrier per round is enough.  The consumer reads tile[column][row]; a wave reads rows
// 4w .. 4w + 3 of 8 columns, and a column stride of 64 + 4 words puts those 32 words into 32
// different banks (word address 4 * column + row mod 32; the LDS of gfx950 has 64 banks).
constexpr int LEAF_ROWS = 64;
constexpr int LEAF_TILE_STRIDE = LEAF_ROWS + 4;
template <class CL>
__device__ __forceinline__ void hash_leaves_lanes(const CL& cl, size_t r0, size_t count,
                                                  uint32_t* __restrict__ out) {
  __shared__ uint32_t tile[2][16][LEAF_TILE_STRIDE];
  const int lane = threadIdx.x & 15, row = threadIdx.x >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lr = threadIdx.x & 63;
  const size_t b0 = (size_t)blockIdx.x * LEAF_ROWS;  // the block's first row of the range
  // a partial block (fewer than 64 rows) keeps every thread: the barriers need all of them and
  // DPP whole 16-lane rows; a surplus thread loads the range's last row and stores nothing
  const size_t lrow = b0 + lr < count ? b0 + lr : count - 1;
  const uint32_t off4 = (uint32_t)(r0 + lrow) * 4u;
  const LaneConsts kc = lane_consts(lane);
  ColWalk<CL> w;  // wave-uniform: this wave's column of the round
  w.enter(cl, 0);
  if (cl.n > 0) w.skip(cl, wave);
  uint32_t x = cl.n > 0 ? ld_col(w.p, off4) : 0u;
  uint32_t h = 0;
  // chunk c is columns [8c, 8c + 8): the even chunks open a round
  for (int c = 0, rest = cl.n; rest > 0; c++, rest -= 8) {
    const uint32_t(*t)[LEAF_TILE_STRIDE] = tile[(c >> 1) & 1];
    if (!(c & 1)) {
      tile[(c >> 1) & 1][wave][lr] = x;
      if (rest > 16) {  // the next round's load, in flight over this round's permutations
        w.skip(cl, 16);
        x = ld_col(w.p, off4);
      }
      __syncthreads();
    }
    const int m = rest < 8 ? rest : 8;
    if (lane < m) h = t[8 * (c & 1) + lane][row];  // overwrite mode: the other lanes keep the state
    h = poseidon2_permute_lane(h, lane, kc);
  }
  if (lane < 8 && b0 + row < count) out[8 * (r0 + b0 + row) + lane] = h;
}
__global__ __launch_bounds__(1024) void k_hash_leaves_lanes(ColList cl, size_t r0, size_t count,
                                                            uint32_t* __restrict__ out) {
  hash_leaves_lanes(cl, r0, count, out);
}
__global__ __launch_bounds__(1024) void k_hash_leaves_lanes_tab(ColTable cl, size_t r0,
                                                                size_t count,
                                                                uint32_t* __restrict__ out) {
  hash_leaves_lanes(cl, r0, count, out);
}

// Merkle node from its two children already in st[0..16]:
//   compress(children), then with injected columns: compress(node, sponge(the node's row)).
// The steps share ONE permutation call site, so the kernel holds a single inlined copy of
// the (~27 KB) permutation core instead of three; each step picks its ends (both compressions
// and the sponge's last permutation are read in [0..8) only).
template <class CL>
__device__ __forceinline__ void merkle_node(uint32_t st[16], const CL& cl, uint32_t off4) {
  const int nchunks = (cl.n + 7) >> 3;
  const int nsteps = nchunks ? nchunks + 2 : 1;
  ColWalk<CL> w;
  w.enter(cl, 0);
  uint32_t d[8];
  int rest = cl.n;
  for (int step = 0; step < nsteps; step++) {
    bool lo = true, hi = false;
    if (step == 1) {
#pragma unroll
      for (int i = 0; i < 8; i++) d[i] = st[i];
#pragma unroll
      for (int i = 0; i < 16; i++) st[i] = 0;
    }
    if (step >= 1 && step <= nchunks) {
      const int m = rest < 8 ? rest : 8;
      uint32_t nx[8];
      load_chunk(nx, w, cl, off4);
      take_chunk(st, nx, m);
      rest -= m;
      if (rest > 0) {  // another chunk follows
        lo = rest < 8;
        hi = true;
      }
    }
    if (nchunks && step == nchunks + 1) {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        st[8 + i] = st[i];
        st[i] = d[i];
      }
    }
    poseidon2_permute_ends(st, step == 1, lo, hi);
  }
}

__device__ __forceinline__ void load16(uint32_t st[16], const uint32_t* p) {
  const uint4* in = reinterpret_cast<const uint4*>(p);
  const uint4 a = in[0], b = in[1], c = in[2], d = in[3];
  st[0] = a.x; st[1] = a.y; st[2] = a.z; st[3] = a.w;
  st[4] = b.x; st[5] = b.y; st[6] = b.z; st[7] = b.w;
  st[8] = c.x; st[9] = c.y; st[10] = c.z; st[11] = c.w;
  st[12] = d.x; st[13] = d.y; st[14] = d.z; st[15] = d.w;
}

__device__ __forceinline__ void store8(uint32_t* p, const uint32_t st[16]) {
  uint4* o = reinterpret_cast<uint4*>(p);
  o[0] = make_uint4(st[0], st[1], st[2], st[3]);
  o[1] = make_uint4(st[4], st[5], st[6], st[7]);
}

// Nodes [j0, j0 + count) of a layer.
template <class CL>
__device__ __forceinline__ void compress(const uint32_t* __restrict__ prev, size_t j0,
                                         size_t count, uint32_t* __restrict__ out, const CL& inj) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const size_t j = j0 + i;
  uint32_t st[16];
  load16(st, prev + 16 * j);
  merkle_node(st, inj, (uint32_t)j * 4u);
  store8(out + 8 * j, st);
}
__global__ __launch_bounds__(256) void k_compress(const uint32_t* __restrict__ prev, size_t j0,
                                                  size_t count, uint32_t* __restrict__ out,
                                                  ColList inj) {
  compress(prev, j0, count, out, inj);
}
__global__ __launch_bounds__(256) void k_compress_tab(const uint32_t* __restrict__ prev, size_t j0,
                                                      size_t count, uint32_t* __restrict__ out,
                                                      ColTable inj) {
  compress(prev, j0, count, out, inj);
}

// Merkle node j in lane mode (see poseidon2_permute_lane): lane l of the node's 16-lane row
// holds word l of the state; the digest ends up in lanes 0..7.  The injected columns are the
// nc columns from segment s0 on.
template <class CL>
__device__ __forceinline__ uint32_t merkle_node_lane(uint32_t v, const CL& cl, int s0, int nc,
                                                     size_t j, int lane, const LaneConsts& kc) {
  ColWalk<CL> w;
  w.enter(cl, s0);
  v = poseidon2_permute_lane(v, lane, kc);
  if (nc > 0) {
    const uint32_t d = v;
    uint32_t h = 0;
    for (int rest = nc; rest > 0; rest -= 8) {  // PaddingFreeSponge, overwrite mode
      const int m = rest < 8 ? rest : 8;
      const uint32_t* col = w.next_lanes(cl, m, lane);
      if (lane < m && col) h = ld_global(col, j);
      h = poseidon2_permute_lane(h, lane, kc);
    }
    const uint32_t hs = dpp<DPP_ROR8>(h);  // lanes 8..15 <- h[0..7]
    v = poseidon2_permute_lane(lane < 8 ? d : hs, lane, kc);
  }
  return v;
}

// Subtree layers in lane mode (16 lanes per node: the permutation latency, not throughput,
// is the cost here).  Block b owns TOP_NODES consecutive nodes of the first layer and
// computes their subtree up to its root: up to TOP_LAYERS layers, every layer but the first
// read from LDS, every digest written to HBM (query paths need every layer).  (A variant that
// let the last block to finish build the rest of the tree in the same launch was no faster:
// the cross-XCD release/acquire cost what the launch boundary did, profiles/r02/ab_merkle_top.txt.)
// (32- and 16-node subtrees, i.e. 512- and 256-thread blocks with one wave per SIMD from the
// first layer on, left k_compress_top's time unchanged within 3%: a layer costs one lane-mode
// permutation latency whatever the occupancy, profiles/r03/ab_open_and_tops.txt)
constexpr int TOP_NODES = 64;   // fills a 1024-thread block in one lane-mode pass
constexpr int TOP_LAYERS = 7;   // 64 nodes -> 1
// Medium layers (TOP_NODES < nodes <= LANE_LAYER_MAX) go to lane mode: a single-lane launch
// of this size is one permutation latency long (~12 us) while 16 lanes per node finish sooner.
// (2^12, 2^13, 2^15, 2^16: slower, profiles/r02/ab_merkle_top.txt, profiles/r04/ab_lane_layer_threshold.txt)
constexpr size_t LANE_LAYER_MAX = (size_t)1 << 14;
// Leaves of at most LANE_LAYER_MAX rows go to k_hash_leaves_lanes from this many columns on
// Single launches of both kernels, alternating, 20 each (profiles/r18/merkle_wide.json; median
// (min-max) us, lane kernel against thread kernel): from 64 columns on the lane kernel's whole
// range lies below the thread kernel's minimum, at 2^11 and at 2^14 rows -- 64 columns 36.3
// (36.2-36.6) against 56.6 (56.5-61.4), 2^11 x 544 in 8 segments 280 (278-284) against 455
// (451-458).  Below that its median is lower as well (8 columns 8.6 against 11.2, 2^14 x 31 23.5
// against 31.4), but one launch in twenty runs 10-20 us late in either kernel, and over five
// sessions most shapes of 8 to 31 columns had a session in which such a launch put the lane
// kernel's maximum above the thread kernel's (2^14 x 31: 42.4 against 37.6 in one of five), so
// trees below 64 columns stay with the thread kernel.
constexpr int LANE_LEAF_MIN_COLS = 64;
constexpr int MAXTOP = TOP_LAYERS;
struct TopLayers {
  uint32_t* out[MAXTOP];
  int s0[MAXTOP], nc[MAXTOP];  // a layer injects nc columns, from segment s0 of the list on
  int n;  // layers in this launch
};

// base: the first node of the launch's first layer (a rank's subtree of a sharded tree; 0 else)
template <class CL>
__device__ __forceinline__ void compress_top(const uint32_t* __restrict__ prev, size_t nlen,
                                             const CL& inj, const TopLayers& tl,
                                             const RootChallenge& rc, size_t base) {
  __shared__ uint32_t buf[2][TOP_NODES * 8];
  const size_t per = nlen < (size_t)TOP_NODES ? nlen : (size_t)TOP_NODES;
  const size_t g0 = base + (size_t)blockIdx.x * per;  // first-layer node of this block
  const int lane = threadIdx.x & 15;
  const LaneConsts kc = lane_consts(lane);
  for (int l = 0; l < tl.n; l++) {
    const size_t m = per >> l, g = g0 >> l;
    const uint32_t* src = buf[(l - 1) & 1];
    uint32_t* dst = buf[l & 1];
    // whole 16-lane rows are active together (DPP needs all of them); the first layer is read
    // from HBM, the rest from LDS (one pointer for both would compile to flat loads)
    for (size_t j = threadIdx.x >> 4; j < m; j += blockDim.x >> 4) {
      const uint32_t x = l == 0 ? ld_global(prev, 16 * (g + j) + lane) : src[16 * j + lane];
      const uint32_t v = merkle_node_lane(x, inj, tl.s0[l], tl.nc[l], g + j, lane, kc);
      if (lane < 8) {
        tl.out[l][8 * (g + j) + lane] = v;
        dst[8 * j + lane] = v;
      }
    }
    __syncthreads();
  }
  // FRI transcript step on the finished root (the root's block only): observe the root,
  // duplex, beta = the last 4 outputs popped in reverse (as k_fri_challenge)
  if (rc.state && threadIdx.x < 64) {
    const uint32_t* root = buf[(tl.n - 1) & 1];
    uint32_t v = lane < 8 ? root[lane] : ld_global(rc.state, lane);
    v = poseidon2_permute_lane(v, lane, kc);
    if (threadIdx.x < 16) {
      rc.state[lane] = v;
      if (lane >= 4 && lane < 8) rc.beta->c[7 - lane] = v;
    }
  }
}
__global__ __launch_bounds__(1024) void k_compress_top(const uint32_t* __restrict__ prev,
                                                       size_t nlen, ColList inj, TopLayers tl,
                                                       RootChallenge rc, size_t base) {
  compress_top(prev, nlen, inj, tl, rc, base);
}
__global__ __launch_bounds__(1024) void k_compress_top_tab(const uint32_t* __restrict__ prev,
                                                           size_t nlen, ColTable inj, TopLayers tl,
                                                           RootChallenge rc, size_t base) {
  compress_top(prev, nlen, inj, tl, rc, base);
}

// Medium layers in lane mode (see LANE_LAYER_MAX).
template <class CL>
__device__ __forceinline__ void compress_lanes(const uint32_t* __restrict__ prev, size_t j0,
                                               size_t count, uint32_t* __restrict__ out,
                                               const CL& inj) {
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const int lane = threadIdx.x & 15;
  if (i >= count) return;
  const size_t j = j0 + i;
  const uint32_t v = merkle_node_lane(prev[16 * j + lane], inj, 0, inj.n, j, lane, lane_consts(lane));
  if (lane < 8) out[8 * j + lane] = v;
}
__global__ __launch_bounds__(256) void k_compress_lanes(const uint32_t* __restrict__ prev,
                                                        size_t j0, size_t count,
                                                        uint32_t* __restrict__ out, ColList inj) {
  compress_lanes(prev, j0, count, out, inj);
}
__global__ __launch_bounds__(256) void k_compress_lanes_tab(const uint32_t* __restrict__ prev,
                                                            size_t j0, size_t count,
                                                            uint32_t* __restrict__ out,
                                                            ColTable inj) {
  compress_lanes(prev, j0, count, out, inj);
}

__global__ __launch_bounds__(256) void k_hash_rows8_lanes(const uint32_t* __restrict__ rows,
                                                          size_t r0, size_t count,
                                                          uint32_t* __restrict__ out) {
  const size_t i = r0 + (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  const int lane = threadIdx.x & 15;
  if (i >= r0 + count) return;
  const uint32_t v = poseidon2_permute_lane(lane < 8 ? rows[8 * i + lane] : 0u, lane);
  if (lane < 8) out[8 * i + lane] = v;
}

// Lane-mode batch permutation (bfz_poseidon2_permute_small): 16 lanes per state.
__global__ __launch_bounds__(256) void k_permute_lanes(uint32_t* __restrict__ s, size_t n) {
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const int lane = threadIdx.x & 15;
  if (i >= n) return;
  s[16 * i + lane] = poseidon2_permute_lane(s[16 * i + lane], lane);
}

__global__ __launch_bounds__(256) void k_permute_batch(uint32_t* __restrict__ s, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t st[16];
#pragma unroll
  for (int k = 0; k < 16; k++) st[k] = s[16 * i + k];
  poseidon2_permute(st);
#pragma unroll
  for (int k = 0; k < 16; k++) s[16 * i + k] = st[k];
}

__global__ __launch_bounds__(256) void k_hash_rows8(const uint32_t* __restrict__ rows, size_t r0,
                                                    size_t count, uint32_t* __restrict__ out) {
  const size_t i = r0 + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r0 + count) return;
  uint32_t st[16];
  const uint4* in = reinterpret_cast<const uint4*>(rows + 8 * i);
  uint4 a = in[0], b = in[1];
  st[0] = a.x; st[1] = a.y; st[2] = a.z; st[3] = a.w;
  st[4] = b.x; st[5] = b.y; st[6] = b.z; st[7] = b.w;
#pragma unroll
  for (int k = 8; k < 16; k++) st[k] = 0;
  poseidon2_permute(st);
  uint4* o = reinterpret_cast<uint4*>(out + 8 * i);
  o[0] = make_uint4(st[0], st[1], st[2], st[3]);
  o[1] = make_uint4(st[4], st[5], st[6], st[7]);
}

// A tree's columns on the host: its matrices by descending height (the order they are hashed
// in) and their segments.  A matrix without columns has no segment (ColWalk: a segment has at
// least one column).
struct TreeCols {
  std::vector<const MatRef*> sorted;
  std::vector<ColSeg> seg;
  std::vector<int> seg_of{0};        // sorted[i]'s segment; seg_of[sorted.size()] = seg.size()
  const ColSeg* table = nullptr;     // the tree's col_table when it has one
};

// Sorts the tree's matrices and, for a tree with more than MAXSEG segments (only then can a
// launch's list exceed the kernel arguments), fills its device table: one upload on the tree's
// stream, ahead of every launch, through the pinned staging arena as the chip programs' code and
// list buffers go (the host vector need not outlive this call).
static TreeCols tree_cols(const std::vector<MatRef>& mats, MerkleTree& t, hipStream_t st,
                          bool always_table = false) {
  TreeCols tc;
  for (const MatRef& m : mats) tc.sorted.push_back(&m);
  std::stable_sort(tc.sorted.begin(), tc.sorted.end(),
                   [](const MatRef* a, const MatRef* b) { return a->height > b->height; });
  tc.seg_of.clear();
  for (const MatRef* m : tc.sorted) {
    tc.seg_of.push_back((int)tc.seg.size());
    if (m->width <= 0) continue;
    // ld_col addresses a column's words by a 32-bit byte offset
    if (m->height > ((size_t)1 << 30)) throw std::runtime_error("merkle: matrix taller than 2^30");
    tc.seg.push_back(ColSeg{m->base, m->stride ? m->stride : m->height, m->width});
  }
  tc.seg_of.push_back((int)tc.seg.size());
  t.col_table.free();
  if (tc.seg.size() > (size_t)MAXSEG || (always_table && !tc.seg.empty())) {
    t.col_table.reset(tc.seg.size());
    upload_async(t.col_table.p, tc.seg.data(), tc.seg.size() * sizeof(ColSeg), st);
    tc.table = t.col_table.p;
  }
  return tc;
}

// The columns of one launch, sorted[a, b): in the kernel arguments when they fit (every
// built-in proof's launches do), else as a range of the tree's table for the `_tab` kernels.
struct Cols {
  ColList arg;
  ColTable tab;
  int n;         // columns
  bool in_args;
};
static Cols launch_cols(const TreeCols& tc, size_t a, size_t b) {
  Cols c{};
  const int s0 = tc.seg_of[a], nseg = tc.seg_of[b] - s0;
  c.in_args = nseg <= MAXSEG;
  for (int i = 0; i < nseg; i++) {
    c.n += tc.seg[s0 + i].n;
    if (c.in_args) c.arg.seg[i] = tc.seg[s0 + i];
  }
  c.arg.nseg = c.in_args ? nseg : 0;
  c.arg.n = c.in_args ? c.n : 0;
  c.tab = ColTable{tc.table ? tc.table + s0 : nullptr, nseg, c.n};
  return c;
}

// One layer's nodes [j0, j0 + count) from prev into out (lane mode for small launches).
static void launch_layer(const uint32_t* prev, uint32_t* out, size_t j0, size_t count,
                         const Cols& c, hipStream_t st) {
  if (count <= LANE_LAYER_MAX) {
    const dim3 grid(ceil_div(16 * count, 256));
    if (c.in_args)
      hipLaunchKernelGGL(k_compress_lanes, grid, dim3(256), 0, st, prev, j0, count, out, c.arg);
    else
      hipLaunchKernelGGL(k_compress_lanes_tab, grid, dim3(256), 0, st, prev, j0, count, out, c.tab);
  } else {
    KernelProbe& probe = p2_probe();
    hipEvent_t ev0 = probe.on ? probe.begin(st) : nullptr;
    const dim3 grid(ceil_div(count, 256));
    if (c.in_args)
      hipLaunchKernelGGL(k_compress, grid, dim3(256), 0, st, prev, j0, count, out, c.arg);
    else
      hipLaunchKernelGGL(k_compress_tab, grid, dim3(256), 0, st, prev, j0, count, out, c.tab);
    // one compression, plus the injected rows' sponge and one more compression if any
    if (probe.on)
      probe.end(ev0, st, (double)count * (c.n ? 2 + (c.n + 7) / 8 : 1), c.n ? "k_compress+inject" : "k_compress");
  }
  KCHECK();
}

// Leaf digests of rows [r0, r0 + count): lane mode (k_hash_leaves_lanes) or one thread per row.
static void launch_leaves(const Cols& c, size_t r0, size_t count, uint32_t* out, bool lanes,
                          hipStream_t st) {
  if (lanes) {
    const dim3 grid(ceil_div(count, LEAF_ROWS)), block(16 * LEAF_ROWS);
    if (c.in_args)
      hipLaunchKernelGGL(k_hash_leaves_lanes, grid, block, 0, st, c.arg, r0, count, out);
    else
      hipLaunchKernelGGL(k_hash_leaves_lanes_tab, grid, block, 0, st, c.tab, r0, count, out);
  } else {
    KernelProbe& probe = p2_probe();
    hipEvent_t ev0 = probe.on ? probe.begin(st) : nullptr;
    const dim3 grid(ceil_div(count, 256));
    if (c.in_args)
      hipLaunchKernelGGL(k_hash_leaves, grid, dim3(256), 0, st, c.arg, r0, count, out);
    else
      hipLaunchKernelGGL(k_hash_leaves_tab, grid, dim3(256), 0, st, c.tab, r0, count, out);
    if (probe.on) probe.end(ev0, st, (double)count * ((c.n + 7) / 8), "k_hash_leaves");
  }
  KCHECK();
}

// The matrices of height nlen from sorted[next] on: returns the index past them.
static size_t height_end(const TreeCols& tc, size_t next, size_t nlen) {
  while (next < tc.sorted.size() && tc.sorted[next]->height == nlen) next++;
  return next;
}

// One k_compress_top launch: tl.n layers from layers[L - 1] (`first` nodes in the launch's first
// layer, `base` the first of them), injecting sorted[next..] by height; returns the index past
// the injected matrices.  The launch's list holds the matrices of all its layers; a layer
// injects tl.nc[l] columns from segment tl.s0[l] of it on.
static size_t launch_top(MerkleTree& t, int L, TopLayers tl, size_t nlen, size_t first, size_t base,
                         const TreeCols& tc, size_t next, RootChallenge rc, hipStream_t st) {
  const size_t a = next;
  for (int l = 0; l < tl.n; l++, nlen >>= 1) {
    const size_t e = height_end(tc, next, nlen);
    tl.s0[l] = tc.seg_of[next] - tc.seg_of[a];
    tl.nc[l] = 0;
    for (; next < e; next++) tl.nc[l] += tc.sorted[next]->width;
    t.layers[L + l].reset(8 * nlen);
    tl.out[l] = t.layers[L + l].p;
  }
  const Cols c = launch_cols(tc, a, next);
  const unsigned blocks = first > (size_t)TOP_NODES ? (unsigned)(first / TOP_NODES) : 1u;
  const uint32_t* prev = t.layers[L - 1].p;
  if (c.in_args)
    hipLaunchKernelGGL(k_compress_top, dim3(blocks), dim3(16 * TOP_NODES), 0, st, prev, first,
                       c.arg, tl, rc, base);
  else
    hipLaunchKernelGGL(k_compress_top_tab, dim3(blocks), dim3(16 * TOP_NODES), 0, st, prev, first,
                       c.tab, tl, rc, base);
  KCHECK();
  return next;
}

// Layers L0..nl with layers[L0-1] (len nodes) complete; sorted[next..] are the matrices
// still to inject (heights descending).  Big layers get one launch each; the rest go to
// k_compress_top in one launch.
static void build_layers(MerkleTree& t, int L0, size_t len, const TreeCols& tc,
                         size_t next, hipStream_t st, bool fetch_root = true,
                         RootChallenge rc = {}) {
  const int nl = (int)t.layers.size() - 1;
  int L = L0;
  for (; L <= nl && (len >> 1) > LANE_LAYER_MAX; L++) {  // throughput layers
    const size_t nlen = len >> 1;
    const size_t e = height_end(tc, next, nlen);
    t.layers[L].reset(8 * nlen);
    launch_layer(t.layers[L - 1].p, t.layers[L].p, 0, nlen, launch_cols(tc, next, e), st);
    next = e;
    len = nlen;
  }
  while (L <= nl) {  // subtree launches
    const size_t first = len >> 1;
    const int sub = first > (size_t)TOP_NODES ? TOP_LAYERS : log2i(first) + 1;
    TopLayers tl{};
    tl.n = std::min(sub, nl - L + 1);
    const bool root_launch = L + tl.n > nl;
    next = launch_top(t, L, tl, first, first, 0, tc, next, root_launch ? rc : RootChallenge{}, st);
    L += tl.n;
    len = first >> (tl.n - 1);
  }
  if (next != tc.sorted.size()) throw std::runtime_error("merkle: non power-of-two heights");
  if (!fetch_root) return;
  fetch(t.root, t.layers[nl].p, 32, st);
}

// ------------------------------------------------------------------ sharded trees
ShardCtx*& shard_ctx() {
  static ShardCtx* c = nullptr;
  return c;
}

static bool shard_tree(size_t h0) {
  const ShardCtx* c = shard_ctx();
  return c && c->world > 1 && h0 >= (size_t)c->world * SHARD_MIN_LEAVES;
}

// Rank k owns nodes [k len / G, (k+1) len / G) of every layer with len >= G nodes (one
// subtree, injected rows included); the layer of G nodes is all-gathered and the layers above
// it are built redundantly by every rank.  leaves(r0, count) hashes the rank's own rows.
template <class Leaves>
static void build_sharded(MerkleTree& t, size_t h0, const TreeCols& tc,
                          size_t next, Leaves leaves, hipStream_t st, bool fetch_root,
                          RootChallenge rc = {}) {
  const ShardCtx& c = *shard_ctx();
  const size_t G = (size_t)c.world, k = (size_t)c.rank;
  const int nl = log2i(h0), lg = log2i(G);
  t.sharded_below = nl - lg;  // layers [0, nl - lg) hold only this rank's range
  t.shard_log = lg;
  leaves(k * (h0 / G), h0 / G);
  size_t len = h0;
  int L = 1;
  for (; L <= nl - lg && (len >> 1) / G > LANE_LAYER_MAX; L++) {  // throughput layers
    const size_t nlen = len >> 1;
    const size_t e = height_end(tc, next, nlen);
    t.layers[L].reset(8 * nlen);
    launch_layer(t.layers[L - 1].p, t.layers[L].p, k * (nlen / G), nlen / G,
                 launch_cols(tc, next, e), st);
    next = e;
    len = nlen;
  }
  // the rank's subtree below the shard level: up to TOP_LAYERS layers per k_compress_top launch
  // (a layer per launch made the small shares of a many-rank proof launch-bound)
  while (L <= nl - lg) {
    const size_t first = (len >> 1) / G;  // this rank's nodes of the launch's first layer
    const int sub = first > (size_t)TOP_NODES ? TOP_LAYERS : log2i(first) + 1;
    TopLayers tl{};
    tl.n = std::min(sub, nl - lg - L + 1);
    next = launch_top(t, L, tl, len >> 1, first, k * first, tc, next, RootChallenge{}, st);
    L += tl.n;
    len >>= tl.n;
  }
  // layer nl - lg has G nodes; node k is ours: all-gather them device to device
  DBuf<uint32_t>& lay = t.layers[nl - lg];
  DBuf<uint32_t> all(8 * G);
  coll_sync(st);
  c.allgather(lay.p + 8 * k, 32, all.p);
  HIP_CHECK(hipMemcpyAsync(lay.p, all.p, 32 * G, hipMemcpyDeviceToDevice, st));
  build_layers(t, nl - lg + 1, G, tc, next, st, fetch_root, rc);
}

void merkle_build(const std::vector<MatRef>& mats, MerkleTree& t, hipStream_t st, bool fetch_root) {
  if (mats.empty()) throw std::runtime_error("merkle: no matrices");
  t.mats = mats;
  const TreeCols tc = tree_cols(mats, t, st);
  const size_t h0 = tc.sorted[0]->height;
  t.layers.clear();
  t.layers.resize(log2i(h0) + 1);
  t.sharded_below = 0;
  const size_t next = height_end(tc, 0, h0);
  t.layers[0].reset(8 * h0);
  const Cols cl = launch_cols(tc, 0, next);
  auto leaves = [&](size_t r0, size_t count) {
    launch_leaves(cl, r0, count, t.layers[0].p,
                  count <= LANE_LAYER_MAX && cl.n >= LANE_LEAF_MIN_COLS, st);
  };
  if (shard_tree(h0)) {
    build_sharded(t, h0, tc, next, leaves, st, fetch_root);
    return;
  }
  leaves(0, h0);
  build_layers(t, 1, h0, tc, next, st, fetch_root);
}

static void hash_rows8_range(const uint32_t* rows, size_t r0, size_t count, uint32_t* digests,
                             hipStream_t st) {
  if (count <= LANE_LAYER_MAX)
    hipLaunchKernelGGL(k_hash_rows8_lanes, dim3(ceil_div(16 * count, 256)), dim3(256), 0, st, rows,
                       r0, count, digests);
  else {
    KernelProbe& probe = p2_probe();
    hipEvent_t ev0 = probe.on ? probe.begin(st) : nullptr;
    hipLaunchKernelGGL(k_hash_rows8, dim3(ceil_div(count, 256)), dim3(256), 0, st, rows, r0, count,
                       digests);
    if (probe.on) probe.end(ev0, st, (double)count, "k_hash_rows8");
  }
  KCHECK();
}

void merkle_from_rows8(MerkleTree& t, const uint32_t* rows, size_t h, hipStream_t st,
                       bool fetch_root, RootChallenge rc, bool allow_shard,
                       const std::function<void(size_t, size_t, uint32_t*)>& fused) {
  t.mats = {MatRef{rows, h, 8}};
  t.layers.clear();
  t.layers.resize(log2i(h) + 1);
  t.layers[0].reset(8 * h);
  t.sharded_below = 0;
  auto leaves = [&](size_t r0, size_t count) {
    if (fused) fused(r0, count, t.layers[0].p);
    else hash_rows8_range(rows, r0, count, t.layers[0].p, st);
  };
  if (h < 2) throw std::runtime_error("merkle: rows8 tree needs two leaves");
  if (allow_shard && shard_tree(h)) {
    build_sharded(t, h, TreeCols{}, 0, leaves, st, fetch_root, rc);
    return;
  }
  leaves(0, h);
  build_layers(t, 1, h, TreeCols{}, 0, st, fetch_root, rc);
}

void poseidon2_batch(uint32_t* states, size_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_permute_batch, dim3(ceil_div(n, 256)), dim3(256), 0, st, states, n);
  KCHECK();
}

void poseidon2_batch_small(uint32_t* states, size_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_permute_lanes, dim3(ceil_div(16 * n, 256)), dim3(256), 0, st, states, n);
  KCHECK();
}

__global__ void k_fill_cells(uint32_t* __restrict__ p, size_t n, uint64_t seed) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = (uint32_t)(((i + seed) * 0x9E3779B97F4A7C15ull) >> 33) % P;
}

void merkle_time(size_t rows, const int* widths, size_t nmats, int kind_a, int kind_b, int runs,
                 float* ms_a, float* ms_b) {
  if (rows < 1 || (rows & (rows - 1)) || rows > ((size_t)1 << 24))
    throw std::runtime_error("merkle_time: rows not a power of two in [1, 2^24]");
  if (!widths || !nmats || !ms_a || !ms_b || runs < 1 || kind_a < 0 || kind_a > 5 || kind_b < 0 ||
      kind_b > 5 || (kind_a >= 4) != (kind_b >= 4))
    throw std::runtime_error("merkle_time: bad argument (kinds 0..5, both leaves or both layers)");
  hipStream_t st = stream();
  auto filled = [&](size_t n, uint64_t seed) {
    DBuf<uint32_t> d(n);
    hipLaunchKernelGGL(k_fill_cells, dim3(ceil_div(n, 256)), dim3(256), 0, st, d.p, n, seed);
    KCHECK();
    return d;
  };
  std::vector<DBuf<uint32_t>> cells;
  std::vector<MatRef> mats;
  for (size_t i = 0; i < nmats; i++) {
    if (widths[i] < 1 || widths[i] > 4096) throw std::runtime_error("merkle_time: width out of range");
    cells.push_back(filled(rows * widths[i], i << 40));
    mats.push_back(MatRef{cells[i].p, rows, widths[i]});
  }
  MerkleTree t;
  const TreeCols tc = tree_cols(mats, t, st, true);
  const Cols c = launch_cols(tc, 0, nmats);
  const DBuf<uint32_t> prev = filled(16 * rows, (uint64_t)1 << 60);
  DBuf<uint32_t> out[2] = {DBuf<uint32_t>(8 * rows), DBuf<uint32_t>(8 * rows)};
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  auto run = [&](int kind, uint32_t* o) {
    Cols k = c;
    if (kind & 1) k.in_args = false;
    else if (!c.in_args) throw std::runtime_error("merkle_time: the list does not fit the kernel arguments");
    HIP_CHECK(hipEventRecord(e0, st));
    if (kind >> 1 == 2) launch_layer(prev.p, o, 0, rows, k, st);
    else launch_leaves(k, 0, rows, o, kind >> 1 == 1, st);
    HIP_CHECK(hipEventRecord(e1, st));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    return ms;
  };
  run(kind_a, out[0].p);  // one warm-up of each
  run(kind_b, out[1].p);
  for (int i = 0; i < runs; i++) {
    ms_a[i] = run(kind_a, out[0].p);
    ms_b[i] = run(kind_b, out[1].p);
  }
  HIP_CHECK(hipEventDestroy(e0));
  HIP_CHECK(hipEventDestroy(e1));
  std::vector<uint32_t> ha(8 * rows), hb(8 * rows);
  HIP_CHECK(hipMemcpyAsync(ha.data(), out[0].p, ha.size() * 4, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(hb.data(), out[1].p, hb.size() * 4, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  if (ha != hb) throw std::runtime_error("merkle_time: the two kernels' digests differ");
}

// kernels a proof launches (gpu.h PreloadKernels)
static PreloadKernels preload_merkle{
    (const void*)&k_hash_leaves,
    (const void*)&k_hash_leaves_tab,
    (const void*)&k_hash_leaves_lanes,
    (const void*)&k_hash_leaves_lanes_tab,
    (const void*)&k_compress,
    (const void*)&k_compress_tab,
    (const void*)&k_compress_top,
    (const void*)&k_compress_top_tab,
    (const void*)&k_compress_lanes,
    (const void*)&k_compress_lanes_tab,
    (const void*)&k_hash_rows8_lanes,
    (const void*)&k_hash_rows8};

}  // namespace bfz
