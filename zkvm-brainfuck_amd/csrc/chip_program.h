// A caller-defined chip of a machine: its AIR as a constraint program (air_program.h, optional --
// Program, Memory and Byte are lookup-only chips) paired with its sends and receives as an
// interaction program (lookup_program.h).  What Chip::eval does for any chip
// (crates/stark/src/chip.rs:222-228: the AIR, then eval_permutation_constraints,
// permutation.rs:157-272) is done here for the pair:
//   chip_compile      both programs validated on their own and against each other, the shape.
//   chip_check_host   debug_constraints (debug.rs:24-105) of one chip, single-threaded: air_run,
//                     then a loop over the compiled list.
//   check_chip_prog_device / quotient_chip_prog (chip_program.hip)
//                     the row check on the trace domain and the machine quotient of the chip
//                     (quotient_values, quotient.rs:18-165) on 3 H_2n, one kernel each.
// Constraint order, as debug_check.h's header: the K_air AIR constraints, one LogUp constraint
// per batch, then the running sum's first-row, transition and last-row constraints.
#pragma once
#include "air_program.h"
#include "debug_check.h"
#include "lookup_program.h"
#include "quotient.h"

namespace bfz {

struct ChipProgram {
  bool has_air = false;
  AirProgram air;
  LookupProgram lk;
  int air_constraints() const { return has_air ? air.num_constraints : 0; }
  int num_constraints() const { return air_constraints() + lk.batches() + 3; }  // K
  int perm_width() const { return lk.perm_width(); }                            // EF columns
  // chip.rs:82-87: a chip with an interaction has degree max(AIR degree, 3) and log quotient
  // degree log2_ceil(degree - 1): 1 up to degree 3, 2 for 4 and 5, 3 for 6 to 9
  int degree() const { return has_air && air.degree > 3 ? air.degree : 3; }
  int log_quotient_degree() const { return chip_lqd_of_degree(degree()); }
  int chunks() const { return 1 << log_quotient_degree(); }  // D
  static int chip_lqd_of_degree(int d) {
    int l = 1;
    while ((1 << l) < d - 1) l++;
    return l;
  }
};

// The largest AIR degree a chip program may have (bfz_set_chip_max_degree): 3 unless raised, 9 at
// most.  Process-wide and independent of air_max_degree().  A program compiled under a higher cap
// is refused again where it is used (chip_cap_or_throw: machine_prove, machine_verify).
int chip_max_degree();
void set_chip_max_degree(int degree);  // 0 = the default; throws outside {0, 3..9}
void chip_cap_or_throw(const ChipProgram& p);
// A chip of log quotient degree l takes heights up to 2^(24 - l) (3 H_(D n) must exist); at l = 1
// the bound is the 2^23 of every trace.
inline size_t chip_max_height(const ChipProgram& p) {
  return (size_t)1 << (p.log_quotient_degree() > 1 ? 24 - p.log_quotient_degree() : 23);
}

// air = nullptr / air_len = 0: a lookup-only chip.  Throws std::runtime_error naming what is
// wrong: either program's own refusal, a width mismatch, no interaction, an AIR degree above
// chip_max_degree().
ChipProgram chip_compile(const uint8_t* air, size_t air_len, const uint8_t* lookups,
                         size_t lookups_len);

// Host path: row-major natural-order traces of canonical words; perm = h x 4 * perm_width().
// out.chip = -1; per_row (optional, h entries): the first failing index or -1.
void chip_check_host(const ChipProgram& p, const uint32_t* main, const uint32_t* prep,
                     const uint32_t* perm, size_t h, const PermChallenges& ch, const kb::EF& cumsum,
                     ChipCheck& out, int32_t* per_row);
// The same check with the constraint profile (ProfileAcc, as profile_air_host): every constraint
// of every row is evaluated; counts[k] = the rows on which constraint k is not zero, first_rows[k]
// = the smallest of them or -1 (K entries each); out is chip_check_host's summary.
void chip_profile_host(const ChipProgram& p, const uint32_t* main, const uint32_t* prep,
                       const uint32_t* perm, size_t h, const PermChallenges& ch, const kb::EF& cumsum,
                       ChipCheck& out, uint64_t* counts, int64_t* first_rows);

// ---- device side (chip_program.hip).  The lists in device memory; code is nullptr / ncode 0 for
// a lookup-only chip (the kernels' HAS_AIR = 0 instantiation, which has no slot file).
struct ChipLists {
  const uint32_t* code;  // AirProgram::code
  int ncode;
  const uint32_t* list;  // LookupProgram::list
  int air_constraints, num_constraints;
};
// The chip's quotient on 3 H_2n: mainc / prepc / permc = the LDEs (column-major, bit-reversed,
// 2^logN rows; prepc may be nullptr without preprocessed columns; permc = 4 * perm_width
// columns).  Of qp everything is read: the LogUp challenges, the cumulative sum, alpha_pows
// (num_constraints powers, alpha^(K-1-k)) and the domain's fields.  Output as quotient_into.
void quotient_chip_prog(const ChipLists& cl, const uint32_t* mainc, const uint32_t* prepc,
                        const uint32_t* permc, int logN, const QuotParams& qp,
                        const QuotParams* qp_dev, const QuotOut& out, hipStream_t st);
// Its launch alone (quotient_chip_prog, beside quotient_prog in quotient.hip, adds the tables).
void launch_quotient_chip_prog(const ChipLists& cl, const uint32_t* mainc, const uint32_t* prepc,
                               const uint32_t* permc, int logN, const QuotParams* qp_dev,
                               const uint32_t* twf, const uint32_t* sel_inv, const QuotOut& qo,
                               hipStream_t st);
// A chip of D = 2^lqd = 4 or 8 chunks: its quotient on coset slab S_r = 3 g^r H_2n, r >= 1, of
// 3 H_(D n) (air_program.h SlabParams).  slab_quot_params turns qp's domain fields (shift, Z_H
// values and inverses) into the slab's and leaves the challenges, the cumulative sum and
// alpha_pows.  quotient_chip_slab (machine_program.hip) is k_quotient_machine_coset over a
// one-segment table: mainc / prepc / permc = the LDEs on the slab, out.chunk[0] / [1] = where
// chunks r / r + D/2 go.
void slab_quot_params(QuotParams& qp, size_t n, int lqd, int r);
void quotient_chip_slab(const ChipLists& cl, const uint32_t* mainc, const uint32_t* prepc,
                        const uint32_t* permc, int logN, const QuotParams& slab_qp,
                        const QuotOut& out, hipStream_t st);
// The row check of column-major bit-reversed traces of h rows, as check_chip_device: res =
// {min(row * K + index) or ~0, failing rows}; per_row_dev (optional) by storage position.
void check_chip_prog_device(const ChipLists& cl, const uint32_t* mainc, const uint32_t* prepc,
                            const uint32_t* permc, size_t h, const PermChallenges* ch_dev,
                            const kb::EF* cumsum_dev, unsigned long long* res_dev,
                            int32_t* per_row_dev, hipStream_t st);

}  // namespace bfz
