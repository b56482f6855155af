// Device NTT / coset LDE (see ntt.hip).
#pragma once
#include <algorithm>
#include <functional>
#include <utility>
#include <vector>

#include "gpu.h"

namespace bfz {

// All device work of a proof is ordered on one stream (bfz::stream()); pooled buffers released
// on the host may be reused immediately by later work on that stream.

// In-place/out-of-place radix-2 passes over `ncols` columns of size 2^L.
// dif=false: inverse DIT (bit-reversed in -> natural out, twiddles w^-1, no 1/n scaling)
// dif=true : forward DIF (natural in -> bit-reversed out)
void ntt_passes(const uint32_t* src, uint32_t* dst, size_t src_stride, size_t dst_stride, int ncols,
                int L, bool dif, hipStream_t st);

// evals: column-major, bit-reversed rows (n x w).  lde: column-major 2n x w, bit-reversed
// rows = evaluations of the interpolant on shift * H_2n (shift = GENERATOR / domain shift).
// Builds (once per process) the twiddle and coset-power tables a proof's LDEs of height 2^L use,
// so no proof builds a table between its launches (bfz_record_* call it for the record's heights).
void prepare_lde_tables(int L);
void coset_lde(const uint32_t* evals, size_t n, int w, uint32_t shift, uint32_t* lde,
               hipStream_t st);
// The same with the input columns at stride src_stride, and only_half = 0 / 1: write only
// LDE rows [0, n) / [n, 2n) of each column (the other half is left untouched -- a quotient
// chunk's own domain is that half, so the caller has its values already; -1: both halves).
void coset_lde_ex(const uint32_t* evals, size_t src_stride, size_t n, int w, uint32_t shift,
                  uint32_t* lde, int only_half, hipStream_t st, int tiny = -1);
// tiny: heights up to 2^8 in one launch (k_lde_tiny): 1 / 0, -1 = BFZ_LDE_TINY (default on).

// Sharded LDE.  lde_coefficients: coef = n * (coefficients of the interpolant
// over H_n), natural order (the iDFT alone).  coset_residue: the rank shard of the coset LDE
// on shift * H_2n for G = 2^logG ranks and residue r = bitrev_G(rank): bit-reversed positions
// [rank m, (rank+1) m), m = 2n / G, column-major (m x w) -- word-for-word the same rows as
// coset_lde's.
void lde_coefficients(const uint32_t* evals, size_t n, int w, uint32_t* coef, hipStream_t st);
void coset_residue(const uint32_t* coef, size_t n, int w, uint32_t shift, int logG, int r,
                   uint32_t* out, hipStream_t st);
// The same for the listed columns only (out column y = coefficient column cols[y]).
void coset_residue_cols(const uint32_t* coef, size_t n, const std::vector<int>& cols,
                        uint32_t shift, int logG, int r, uint32_t* out, hipStream_t st);

// The same in one pass over the coefficients (k_coef_fold): the iDFT's second pass keeps each
// column's coefficients in registers, writes coef only for [j0, j0 + len) (column stride n; the
// first pass runs into coef, so its other words are left holding that pass's intermediate) and
// folds them into out (residue r, m x w, m = 2n / G) and, with next_cols, into nxt (residue r2,
// the listed columns) -- natural order; residue_dft then finishes each (the forward DFT).
// Returns false (nothing launched) where it does not apply (log n <= 14 or > 23, G > 32);
// else *dft_low is what residue_dft has left to do for out and nxt alike: -1 = the whole DFT,
// s >= 0 = only its stages [0, s) (2, 4 and 8 ranks: at 2 ranks without a next residue out is
// k_lde_mid's half r, at 4 and 8 the fold kernel continues with the strided DIF stages).
bool coef_fold_residues(const uint32_t* evals, size_t n, int w, uint32_t* coef, size_t j0,
                        size_t len, uint32_t shift, int logG, int r, uint32_t* out,
                        const std::vector<int>* next_cols, int r2, uint32_t* nxt, int* dft_low,
                        hipStream_t st, int ab = -1);
void residue_dft(uint32_t* out, size_t m, int w, int dft_low, hipStream_t st);
// ab: the A/B switches of this call as LDE_AB_* bits; -1 = the environment's (BFZ_FUSED_RESIDUE,
// BFZ_MID_HALF, BFZ_FUSED_DIF, each on unless "0").
enum : int { LDE_AB_UNFUSED = 1, LDE_AB_NO_MID_HALF = 2, LDE_AB_NO_FUSED_DIF = 4 };

// One rank's sharded LDE, the dispatch of a sharded proof (prover.hip lde_into):
// coef_fold_residues then residue_dft of out and nxt, else lde_coefficients then
// coset_residue[_cols].  next_cols null or empty: no next-row residue.  *folded, if given, runs
// between the two phases (the timed proof's event).  Returns dft_low of the fused path, -2 for
// the unfused one.
int lde_shard(const uint32_t* evals, size_t n, int w, uint32_t* coef, size_t j0, size_t len,
              uint32_t shift, int logG, int r, uint32_t* out, const std::vector<int>* next_cols,
              int r2, uint32_t* nxt, hipStream_t st, int ab = -1,
              const std::function<void()>* folded = nullptr);

// Which kernel families the calling thread has launched since the last call (test hooks).
enum : uint32_t {
  NTT_PASS_DIT = 1u << 0, NTT_PASS_DIF = 1u << 1, NTT_R16_DIT = 1u << 2, NTT_R16_DIF = 1u << 3,
  NTT_TILE_DIT_DIN = 1u << 4, NTT_TILE_DIT = 1u << 5, NTT_TILE_DIF = 1u << 6,
  NTT_LDE_TINY = 1u << 7, NTT_SCALE_SPLIT = 1u << 8, NTT_MID_FULL = 1u << 9,
  NTT_MID_HALF = 1u << 10, NTT_MID_SHARD = 1u << 11, NTT_COEF_FOLD_R0 = 1u << 12,
  NTT_COEF_FOLD_R2 = 1u << 13, NTT_COEF_FOLD_R3 = 1u << 14, NTT_FOLD_RESIDUE = 1u << 15,
  NTT_TILE_B8 = 1u << 16,  // << (B - 8): the tile sizes 2^8 .. 2^14 launched
};
uint32_t ntt_paths_take();

// Row-major natural-order host layout -> column-major bit-reversed device layout.
void transpose_bitrev(const uint32_t* rowmajor, size_t n, int w, uint32_t* colmajor,
                      hipStream_t st);

// Number of waves that saw a word >= p in d[0..n) (0 iff every word is canonical); syncs st.
size_t count_noncanonical(const uint32_t* d, size_t n, hipStream_t st);

// Column-major (H x w) -> row-major, row order unchanged.
void transpose_to_rowmajor(const uint32_t* colmajor, size_t H, int w, uint32_t* rowmajor,
                           hipStream_t st);

}  // namespace bfz
