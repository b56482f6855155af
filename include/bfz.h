/*
 * bfz — C ABI of the MI355X core-proof prover for the felicityin/zkvm-brainfuck zkVM.
 *
 * This is the drop-in boundary.  Each entry point replaces one reference interface
 * (paths relative to the reference repository):
 *
 *   bfz_execute      ProverClient::execute().run()        crates/sdk/src/lib.rs:57-59,
 *                    -> BfProver::execute                 crates/prover/src/lib.rs:60-65
 *   bfz_setup        ProverClient::setup / MachineProver::setup
 *                                                         crates/sdk/src/lib.rs:133-135,
 *                                                         crates/stark/src/prover.rs:49,197,
 *                                                         crates/stark/src/machine.rs:154-224
 *   bfz_prove        ProverClient::prove().run() / MachineProver::prove
 *                                                         crates/sdk/src/action.rs:58-61,
 *                                                         crates/stark/src/prover.rs:112,560-582
 *   bfz_verify       ProverClient::verify / StarkMachine::verify
 *                                                         crates/sdk/src/lib.rs:110-116,
 *                                                         crates/stark/src/machine.rs:258-284
 *   bfz_commit       MachineProver::commit -> Pcs::commit (coset LDE + MerkleTreeMmcs)
 *                                                         crates/stark/src/prover.rs:209-236
 *   bfz_coset_lde    Radix2DitParallel::coset_lde_batch + bit_reverse_rows (inside
 *                    TwoAdicFriPcs::commit, called at prover.rs:227,334,411)
 *   bfz_poseidon2_permute  Poseidon2KoalaBear<16> (kb31_poseidon2.rs:35-50)
 *   bfz_uni_prove    utils::uni_stark_prove -> p3_uni_stark::prove
 *                                                         crates/core/machine/src/utils/prove.rs:97-127
 *   bfz_uni_verify   utils::uni_stark_verify -> p3_uni_stark::verify
 *                                                         crates/core/machine/src/utils/prove.rs:129-159
 *   bfz_uni_check    the row check of p3_uni_stark::prove in a debug build (Air<DebugConstraintBuilder>)
 *                                                         crates/core/machine/src/utils/prove.rs:97-112,
 *                                                         crates/stark/src/debug.rs:43-94
 *   bfz_record_uni_prove   uni_stark_prove on a chip trace the device generated
 *                                                         crates/core/machine/src/utils/prove.rs:97-127
 *   bfz_uni_verify_batch   uni_stark_verify of many proofs, query phase on the device
 *                                                         crates/core/machine/src/utils/prove.rs:129-159
 *
 * Conventions: field elements are uint32_t in MONTGOMERY form (x * 2^32 mod p), i.e.
 * byte-identical to a Rust `[KoalaBear]` slice; matrices are row-major.  Every function
 * returns 0 on success and a negative status on failure (bfz_last_error() describes it);
 * the Rust wrapper panics on a non-zero status, matching the reference (which unwraps).
 * Calls are serialized internally (one mutex); one process drives ONE GPU: bfz_init binds
 * the device on first use and fails if a later call names another one.  The stream,
 * allocator pool, twiddle/selector caches and pinned staging are process-wide, so ranks are
 * separate processes (one per GPU), never threads of one process -- the sharded entry points
 * hold the mutex while they run the caller's collective callbacks.
 * Proofs are byte strings in the BFZ1 normal form described in DESIGN.md.
 */
#ifndef BFZ_H
#define BFZ_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bfz_pk bfz_pk;         /* device-resident proving key (DeviceProvingKey) */
typedef struct bfz_record bfz_record; /* executed record with traces resident in HBM  */
/* ShardMainData<SC, DeviceMatrix, DeviceProverData> (crates/stark/src/types.rs:13-18): the main
 * traces' evaluations, their coset LDEs and Merkle tree, resident in HBM from bfz_main_commit
 * until bfz_main_data_free. */
typedef struct bfz_main_data bfz_main_data;
/* p3 DuplexChallenger<KoalaBear, Poseidon2KoalaBear<16>, 16, 8> (kb31_poseidon2.rs:31) as plain
 * data, words in Montgomery form (the in-memory MontyField31 value): sponge_state, then
 * input_buffer[0..n_input) and output_buffer[0..n_output) exactly as the Rust Vecs hold them
 * (samples pop from the end of output_buffer). */
typedef struct {
  uint32_t sponge_state[16];
  uint32_t input_buffer[8];
  uint32_t n_input;
  uint32_t output_buffer[8];
  uint32_t n_output;
} bfz_challenger;

typedef struct {
  double trace_ms, main_commit_ms, perm_ms, quotient_ms, open_ms, fri_ms, total_ms;
  double lde_ms, lde_bytes; /* whole coset LDEs: 12*n*w algorithmic bytes per call */
  int lde_calls;
  double ntt_kernel_ms, ntt_kernel_bytes; /* NTT pass kernel, per-launch events, 8 B/element */
  int ntt_kernel_launches;
  double p2_kernel_ms, p2_perms; /* Poseidon2 leaf/compress kernels: time and permutations */
  int p2_launches;
  double lde_elem_stages; /* radix-2 element-stages of the coset LDEs: 3*n*log2(n)*w per call */
  /* Openings (k_open_partial_batch: 4*n*w + 16*n*points B per matrix, the low coset) and reduced
   * openings (k_reduce: 4*H*w + 16*H*(2 or 3) B per LDE height): per-launch events, algorithmic
   * bytes. */
  double open_kernel_ms, open_kernel_bytes;
  int open_kernel_launches;
  double reduce_kernel_ms, reduce_kernel_bytes;
  int reduce_kernel_launches;
  /* The LogUp stage (perm_ms, prover.rs:280-334) in parts: permutation rows + cumulative-sum scan
   * (replicated on every rank of a sharded proof), iDFT of the permutation columns (replicated;
   * 0 unsharded), fold + forward DFT (this rank's residue and its next-residue shards when
   * sharded; the whole coset LDE unsharded), Merkle hashing (split). */
  double perm_rows_ms, perm_idft_ms, perm_dft_ms, perm_hash_ms;
  /* The main commit (main_commit_ms, prover.rs:209-236) in the same parts: iDFT of the main
   * columns (replicated when sharded; 0 unsharded), fold + forward DFT, Merkle hashing. */
  double main_idft_ms, main_dft_ms, main_hash_ms;
  /* Base-field cells (sum of height x width) of the main and permutation traces. */
  double main_cells, perm_cells;
} bfz_timings;

/* Binds the process to `device` and looks up every kernel a proof launches (code objects and
 * launch objects, ~5 ms), so none of that runs between the first proof's launches. */
int bfz_init(int device);
const char* bfz_last_error(void);
/* Hash of the sources the library was built from (bfz/srchash.py); bfz/_lib.py refuses a
 * library whose hash differs from the sources beside it. */
const char* bfz_build_id(void);
int bfz_device_name(char* buf, size_t cap);
void bfz_free(void* p);
int bfz_synchronize(void); /* hipDeviceSynchronize on the bound device */
/* Host-only self-tests of the boundary's own bookkeeping (no device needed): "emit_rollback" =
 * a batch hand-over that fails part-way releases the proofs already handed out. 0 = passed. */
int bfz_selftest(const char* name);

int bfz_execute(const char* elf, const uint8_t* stdin_data, size_t nin, uint8_t* out,
                size_t out_cap, size_t* out_len, uint64_t* cycles);

/* MachineProver::generate_traces (crates/stark/src/prover.rs:58-81) after
 * generate_dependencies (machine.rs:228-248): row-major Montgomery trace of one chip
 * (chip index in BfAir::chips() order, brainfuck/mod.rs:53-81; prep != 0 selects the
 * preprocessed trace).  *out is malloc'd (bfz_free).  Returns 1 if the chip is not
 * included in the record. */
int bfz_trace(const char* elf, const uint8_t* stdin_data, size_t nin, int chip, int prep,
              uint32_t** out, size_t* height, size_t* width);

/* Diagnostic: the executor's event stream (Executor::run + emit_events, crates/core/executor/src/
 * executor.rs:71-326) serialized field by field: executor 0 = the record executor (bfz_trace,
 * oracle-checked traces), 1 = the prover pipeline's executor (bfz_record_new, bfz_prove,
 * bfz_prove_batch).  Host only; *out is malloc'd (bfz_free). */
int bfz_execute_events(const char* elf, const uint8_t* stdin_data, size_t nin, int executor,
                       uint8_t** out, size_t* out_len);

/* generate_permutation_trace (crates/stark/src/permutation.rs:75-148, called at
 * prover.rs:280-296) of one chip on the device: main (and, for Program/Byte, prep) are
 * row-major Montgomery traces of `height` rows, alpha/beta the LogUp challenges (EF,
 * Montgomery).  *out (malloc'd, bfz_free) = the permutation trace flattened to base
 * (flatten_to_base, prover.rs:318-334), row-major height x *width; cumsum = its last row's
 * running sum.  Diagnostic entry (the prover keeps the trace in HBM). */
int bfz_perm_trace(int chip, const uint32_t* main, const uint32_t* prep, size_t height,
                   const uint32_t alpha[4], const uint32_t beta[4], uint32_t** out, size_t* width,
                   uint32_t cumsum[4]);

/* Same trace generated on the device from the uploaded events (the prover's own path),
 * returned row-major in natural row order for comparison. */
int bfz_trace_device(const char* elf, const uint8_t* stdin_data, size_t nin, int chip,
                     uint32_t** out, size_t* height, size_t* width);

/* The preprocessed commit is made once per program text and cached (16 most recent programs):
 * a repeated setup of the same ELF returns a handle to the same device-resident key. */
int bfz_setup(const char* elf, bfz_pk** pk, uint32_t vk_commit[8]);
void bfz_pk_free(bfz_pk* pk);

/* MachineProver::pk_to_device (crates/stark/src/prover.rs:52,201-203): the device key of a
 * StarkProvingKey kept on the host.  BfProver::setup keeps only pk_to_host(pk)
 * (crates/prover/src/lib.rs:51) and BfProver::prove rebuilds the device key from it on every
 * proof (:76).  Arguments are the key's preprocessed traces (StarkProvingKey::traces,
 * machine.rs:49-60, in the key's order): chips[i] the chip id (BfAir::chips() order) of
 * traces[i], a row-major Montgomery heights[i] x widths[i] matrix, and the key's commit.
 * The program is recovered from the Program chip's preprocessed trace (pc, opcode, op_a bytes;
 * program/mod.rs:66-94); both traces must be exactly that program's (machine.rs:154-224), and
 * the device commitment of them must equal commit, or the call fails.  The device key is the
 * per-program setup cache's (a cache hit costs the trace comparison only). */
int bfz_pk_from_host(const int* chips, const uint32_t* const* traces, const size_t* heights,
                     const size_t* widths, size_t n, const uint32_t commit[8], bfz_pk** pk);
/* The preprocessed commitment of a device key (StarkProvingKey::commit / vk.commit). */
int bfz_pk_commit(const bfz_pk* pk, uint32_t commit[8]);

/* The split MachineProver surface, for a Rust HipProver:
 *   bfz_main_commit         MachineProver::commit (crates/stark/src/prover.rs:209-236): host
 *                           row-major main traces (as bfz_prove_traces) -> LDE + MerkleTreeMmcs
 *                           commit in HBM; root = main_commit (8 Montgomery words, as vk_commit).
 *                           pk may be NULL (the trait's commit takes no key); if given, bfz_open
 *                           refuses the data for any other key.
 *   bfz_record_main_commit  the same from a device-resident record (traces generated on device).
 *   bfz_challenger_observe_pk  MachineProvingKey::observe_into (prover.rs:595-601).
 *   bfz_open                MachineProver::open (prover.rs:242-553) on the challenger state
 *                           after observe_into.  Like the trait method (which takes the
 *                           challenger &mut), ch is advanced: on success it holds the state
 *                           after the whole opening (PCS open, FRI commit phase, grind, query
 *                           sampling).  MachineProver::prove opens on a clone (prover.rs:578):
 *                           pass a copy to keep the caller's state.  Output = the same BFZ1
 *                           proof bfz_prove* returns.  The main data stays valid (it may be
 *                           opened again).
 *   bfz_main_data_free      drops ShardMainData (frees its HBM). */
int bfz_main_commit(const bfz_pk* pk, const int* chips, const uint32_t* const* traces,
                    const size_t* heights, const size_t* widths, size_t nchips, bfz_main_data** out,
                    uint32_t root[8]);
int bfz_record_main_commit(const bfz_pk* pk, const bfz_record* rec, bfz_main_data** out,
                           uint32_t root[8]);
int bfz_challenger_observe_pk(const bfz_pk* pk, bfz_challenger* ch);
int bfz_open(const bfz_pk* pk, bfz_main_data* data, bfz_challenger* ch, uint8_t** proof,
             size_t* proof_len);
void bfz_main_data_free(bfz_main_data* data);

int bfz_prove(const bfz_pk* pk, const uint8_t* stdin_data, size_t nin, uint8_t** proof,
              size_t* proof_len);
/* MachineProver::prove from host traces (crates/stark/src/prover.rs:560-582 after
 * generate_dependencies + generate_traces, prover.rs:58-81): chips[i] is the chip index in
 * BfAir::chips() order, traces[i] its row-major Montgomery main trace (heights[i] x
 * widths[i], height a power of two).  Preprocessed traces come from the proving key. */
int bfz_prove_traces(const bfz_pk* pk, const int* chips, const uint32_t* const* traces,
                     const size_t* heights, const size_t* widths, size_t nchips, uint8_t** proof,
                     size_t* proof_len);
int bfz_verify(const char* elf, const uint32_t vk_commit[8], const uint8_t* proof,
               size_t proof_len);

/* StarkMachine::verify (crates/stark/src/machine.rs:258-284) of n proofs of one program.
 * on_device = 0: the host verifier, proof by proof.  1: the query phase of all n proofs (the
 * Merkle openings of the four input rounds and of every FRI commit-phase step, the reduced
 * openings and the fold chain: nearly all of a verification's Poseidon2 permutations) in one
 * batched device pass; decoding, the transcript replay, the PoW check, the out-of-domain check
 * and the cumulative-sum check stay on the host.  Both give the same outcome for the same bytes:
 * `why` is the host verifier's reason (truncated to 119 characters), the first failure in its
 * order.  Returns 0 whenever the check RAN (as the constraint checker does), whatever the
 * outcomes; negative for a real error (NULL arguments, no device bound with on_device = 1, a
 * device error).  n = 0 is a successful no-op.  Honours bfz_set_num_queries and
 * bfz_set_pcs_variant exactly as bfz_verify does. */
typedef struct {
  int32_t ok;    /* 1 accepted, 0 rejected */
  int32_t query; /* the query whose check failed first, -1 if the rejection is not a query's */
  char why[120]; /* "" when ok; otherwise the host verifier's reason string */
} bfz_verify_outcome;
int bfz_verify_batch(const char* elf, const uint32_t vk_commit[8], const uint8_t* const* proofs,
                     const size_t* lens, size_t n, int on_device, bfz_verify_outcome* out);

/* Pipelined proofs of one program over many inputs (the reference's execute-then-prove loop,
 * crates/core/machine/src/utils/prove.rs:23-66, with execution off the critical path):
 * exec_threads host threads run the executor into pinned memory, a copy stream uploads job
 * k+1's events while the GPU proves job k.  proofs[i] (malloc'd, bfz_free) is byte-identical to
 * bfz_prove(pk, stdins[i]).  exec_threads <= 0: environment BFZ_EXEC_THREADS or 3.
 * stats (optional): wall time of the batch and per-stage sums over jobs. */
typedef struct {
  double wall_ms, exec_ms, upload_ms, prove_ms;
  int exec_threads;
} bfz_batch_stats;
int bfz_prove_batch(const bfz_pk* pk, const uint8_t* const* stdins, const size_t* nins,
                    size_t njobs, int exec_threads, uint8_t** proofs, size_t* proof_lens,
                    bfz_batch_stats* stats);

/* Split prove: bfz_record_new executes the program and copies its events to HBM (the
 * proof's inputs); bfz_record_prove generates every chip trace on the device
 * (generate_dependencies + generate_traces, prover.rs:58-81) and proves. */
int bfz_record_new(const bfz_pk* pk, const uint8_t* stdin_data, size_t nin, bfz_record** rec,
                   uint64_t* cycles);
int bfz_record_prove(const bfz_pk* pk, const bfz_record* rec, uint8_t** proof, size_t* proof_len,
                     bfz_timings* timings);
void bfz_record_free(bfz_record* rec);

/* The reference's ExecutionRecord (crates/core/executor/src/record.rs:15-34) as plain arrays,
 * one C struct per event type of crates/core/executor/src/events (explicit padding, no
 * compiler-inserted gaps; opcodes are the Opcode discriminants of opcode.rs:13-30).
 * bfz_memory_access is Option<MemoryRecordEnum> (events/memory.rs:31-79): kind 0 = None,
 * 1 = Read (prev_value unused), 2 = Write. */
typedef struct {
  uint8_t kind, value, prev_value, _pad;
  uint32_t timestamp, prev_timestamp;
} bfz_memory_access;
typedef struct { /* CpuEvent, events/cpu.rs */
  uint32_t clk, pc, next_pc, mp, next_mp;
  uint8_t mv, next_mv, _pad[2];
  bfz_memory_access mv_access, next_mv_access;
} bfz_cpu_event;
typedef struct { /* AluEvent, events/instr.rs */
  uint32_t pc;
  uint8_t opcode, next_mv, mv, _pad;
} bfz_alu_event;
typedef struct { /* JumpEvent */
  uint32_t pc, next_pc;
  uint8_t opcode, _pad[3];
  uint32_t dst;
  uint8_t mv, _pad2[3];
} bfz_jump_event;
typedef struct { /* MemInstrEvent */
  uint32_t clk, pc;
  uint8_t opcode, _pad[3];
  uint32_t mp, next_mp;
} bfz_mem_instr_event;
typedef struct { /* IoEvent */
  uint32_t pc;
  uint8_t opcode, _pad[3];
  uint32_t mp;
  uint8_t mv, _pad2[3];
} bfz_io_event;
typedef struct { /* MemoryEvent: addr, initial_mem_access, final_mem_access (events/memory.rs:6-13) */
  uint32_t addr, initial_timestamp, final_timestamp;
  uint8_t initial_value, final_value, _pad[2];
} bfz_memory_event;
typedef struct {
  const bfz_cpu_event* cpu;                 size_t n_cpu;          /* cpu_events */
  const bfz_alu_event* add;                 size_t n_add;          /* add_events */
  const bfz_alu_event* sub;                 size_t n_sub;          /* sub_events */
  const bfz_jump_event* jump;               size_t n_jump;         /* jump_events */
  const bfz_io_event* io;                   size_t n_io;           /* io_events */
  const bfz_mem_instr_event* memory_instr;  size_t n_memory_instr; /* memory_instr_events */
  const bfz_memory_event* memory;           size_t n_memory;       /* cpu_memory_access */
} bfz_events;
/* A device record from the reference's own events (the record utils::prove hands to
 * MachineProver::prove, crates/core/machine/src/utils/prove.rs:38-44): the arrays go to HBM
 * (add_events then sub_events as one AddSub stream, alu/mod.rs:72), the memory events are put
 * in the normal form (sorted by address; the reference drains a HashMap, executor.rs:74), and
 * bfz_record_prove / bfz_record_main_commit then generate every chip trace and the byte-lookup
 * multiplicities on the device (generate_dependencies + generate_traces, prover.rs:58-81,
 * machine.rs:228-248).  The program is pk's.  Events are validated (pc inside the program,
 * opcodes, access kinds, unique memory addresses, at least one cycle) before any kernel reads
 * them.  Host pointers (pageable is fine). */
int bfz_record_from_events(const bfz_pk* pk, const bfz_events* events, bfz_record** rec);

/* The same record from a compact hand-over: one 16-byte bfz_cycle per CpuEvent (in
 * record.cpu_events order) plus cpu_memory_access.  Everything else in the record is a function
 * of these and the program: clk = 2 i (executor.rs:131), next_pc / next_mp = the next cycle's pc
 * / mp (the last cycle's next_pc is the program length, its next_mp follows its opcode),
 * next_mv and both access records follow the opcode (executor.rs:140-205: the read at clk + 1,
 * the ALU write at clk + 2), and every add/jump/memory_instr/io event is the cycle's own fields
 * (emit_events, executor.rs:196-239) -- so the device rebuilds them (tracegen.hip
 * expand_cycles) instead of receiving ~64 B per cycle.  Cycles that no reference record holds
 * (pc outside the program, an access on a memory step, prev_timestamp >= clk + 1, prev_value
 * outside an Input, nonzero padding, a successor pc / mp the executor would not step to, a last
 * cycle that does not leave the program) are refused before any trace kernel runs. */
typedef struct {
  uint32_t pc;         /* CpuEvent::pc */
  uint32_t mp;         /* CpuEvent::mp */
  uint32_t prev_ts;    /* mv_access's prev_timestamp; 0 when mv_access is None (memory steps) */
  uint8_t mv;          /* CpuEvent::mv */
  uint8_t prev_value;  /* Input (mv_access is a Write): its prev_value; 0 otherwise */
  uint8_t _pad[2];
} bfz_cycle;
int bfz_record_from_cycles(const bfz_pk* pk, const bfz_cycle* cycles, size_t n_cycles,
                           const bfz_memory_event* memory, size_t n_memory, bfz_record** rec);

/* The same hand-over in chunks, so the host conversion of record.cpu_events overlaps the DMA:
 * bfz_cycles_begin announces n_cycles; each bfz_cycles_push queues one converted chunk
 * (cycles[first, first + n)) on a copy stream and returns at once -- from page-locked
 * (bfz_host_alloc) memory the copy is a DMA that runs while the caller converts the next chunk,
 * and the chunk must then stay unchanged until bfz_cycles_finish returns; chunks may come from
 * several threads, in any order.  bfz_cycles_finish checks that every cycle was pushed exactly
 * once, then validates and expands them exactly as bfz_record_from_cycles (same record, same
 * proof) and consumes the handle, also on error; bfz_cycles_abort drops an unfinished one.
 * Replaces the single-array call of HipProver::prove (crates/bf-hip-prover) with a pipelined
 * CycleArrays::new; the reference hands the record over in memory (utils/prove.rs:44-46). */
typedef struct bfz_cycle_upload bfz_cycle_upload;
int bfz_cycles_begin(const bfz_pk* pk, size_t n_cycles, bfz_cycle_upload** up);
int bfz_cycles_push(bfz_cycle_upload* up, size_t first, const bfz_cycle* cycles, size_t n);
int bfz_cycles_finish(bfz_cycle_upload* up, const bfz_memory_event* memory, size_t n_memory,
                      bfz_record** rec);
void bfz_cycles_abort(bfz_cycle_upload* up);

/* Page-locked host memory for the hand-over arrays (the Rust CycleArrays builds its bfz_cycle
 * vector in it): bfz_record_from_cycles / bfz_record_from_events then DMA straight from the
 * caller's array instead of staging it through the library's pinned chunks (PCIe-bound: ~60 GB/s
 * against ~35-40 GB/s staged).  Any host memory is still accepted; this only makes the upload
 * faster.  Pairs with bfz_host_free (not bfz_free); freed blocks are kept page-locked for reuse
 * (up to 8 GiB), so a per-proof allocation of the same size does not pin memory again.  Host-side replacement of the reference's
 * Vec allocation in ExecutionRecord hand-off (crates/core/machine/src/utils/prove.rs:44-46). */
int bfz_host_alloc(size_t bytes, void** out);
void bfz_host_free(void* p);

/* One proof sharded over `world` GPUs (one process per GPU, every rank calls this with the
 * same record): each rank computes its residue-class row shard of every large LDE, hashes its
 * subtree of every large Merkle tree, evaluates the quotient at its points and computes its
 * slice of the openings, reduced openings and large FRI rounds (the commits, quotient and
 * open of crates/stark/src/prover.rs:209-236,344-470); the ranks exchange subtree roots,
 * quotient values, opened-value slices, one FRI layer and the query openings through the
 * callbacks (torch.distributed / RCCL on the host side).  Every rank returns the same proof,
 * byte-identical to bfz_record_prove's.  The
 * callbacks return 0 on success.  Their buffers (send / recv / data) are DEVICE pointers on the
 * rank's GPU: ncclAllGather / ncclAllReduce run on them directly.  When a callback is entered the
 * send data is complete; the library's stream is drained first except at the two quotient
 * all-gathers, where later GPU work is already queued to run beside the collective (a callback
 * that synchronizes the whole device waits for that work too, which is correct).  The received
 * data must be in place when the callback returns. */
typedef int (*bfz_allgather_fn)(void* ctx, const void* send, size_t bytes, void* recv);
typedef int (*bfz_allreduce_u32_fn)(void* ctx, uint32_t* data, size_t n);
/* `count` proofs of one record back to back with `inflight` (1..4) of them in flight, each on
 * its own stream, pool and pinned mailboxes ("lane", one host thread each): one proof's
 * latency-bound launches (Merkle tree tops, the FRI tail, the transcript steps) then run beside
 * the other's bulk hashing.  Every proof must be byte-identical to the first (an error
 * otherwise); *proof receives the first; wall_ms (optional) the whole run.  The steady-state
 * throughput of the bfz_record_prove loop; the reference proves one shard at a time
 * (utils/prove.rs:38-66). */
int bfz_record_prove_repeat(const bfz_pk* pk, const bfz_record* rec, int count, int inflight,
                            uint8_t** proof, size_t* len, double* wall_ms);

int bfz_record_prove_sharded(const bfz_pk* pk, const bfz_record* rec, int rank, int world,
                             bfz_allgather_fn allgather, bfz_allreduce_u32_fn allreduce_sum,
                             void* ctx, uint8_t** proof, size_t* proof_len, bfz_timings* timings);

/* Timing of ONE rank's share of a world-rank sharded proof, run alone on this GPU: the same
 * kernels and sizes bfz_record_prove_sharded runs on rank `rank`, with every exchange a no-op
 * (receive buffers keep whatever they hold, so the result is not a proof and is discarded;
 * the FRI final-constant check is skipped).  Stage times and kernel counters go to *timings;
 * timings == NULL runs the share without stage events or per-launch kernel probes (the caller
 * times it on the wall clock, as the single-GPU headline is timed).  Predicts the per-rank
 * critical path of an N-GPU proof without N GPUs. */
int bfz_record_prove_shard_solo(const bfz_pk* pk, const bfz_record* rec, int rank, int world,
                                bfz_timings* timings);

/* The collectives of the last bfz_record_prove_shard_solo run, in call order: kinds[i] = 0 for an
 * all-gather (bytes[i] = this rank's contribution; it receives world - 1 times that), 1 for a sum
 * all-reduce of u32 words (bytes[i] = the vector's size).  *n = the number of collectives; at most
 * cap entries are written.  Feeds bench.py's collective-time model of the N-GPU curve; the
 * reference has no multi-GPU prover. */
int bfz_shard_solo_exchanges(int* kinds, uint64_t* bytes, size_t cap, size_t* n);

/* For the same collectives: ms[i] = GPU milliseconds of the work this rank has queued to run
 * while collective i is in flight (the sharded prover issues the quotient exchange in two
 * all-gathers, each after the work it overlaps is queued), 0 where nothing overlaps.  Measured
 * only by a bfz_record_prove_shard_solo run WITH timings (0 otherwise).  bench.py's collective
 * model charges max(0, collective time - ms[i]). */
int bfz_shard_solo_overlaps(double* ms, size_t cap, size_t* n);

/* Device memory held by proof lane `lane`'s buffer pool (0..3, the lanes of
 * bfz_record_prove_repeat / bfz_prove_batch; 0 = the default
 * lane): every buffer a proof on that lane allocated, in use or cached for the next proof -- the
 * resident set of one proof in flight (bench.py reports it beside the lanes' throughput).  The
 * process-wide device data -- twiddle, power and selector tables, proving keys, the records'
 * device events -- lives in a separate resident pool and is not included.  0 for a lane never
 * used. */
int bfz_device_pool_bytes(int lane, uint64_t* bytes);

/* Column-sharded PCS commit + FRI commit phase of a synthetic trace (BASELINE.json configs 4
 * and 5).  Replaces, for one n x (world * w_local) trace, TwoAdicFriPcs::commit
 * (crates/stark/src/prover.rs:209-236: coset LDE with shift GENERATOR, bit-reversed rows,
 * MerkleTreeMmcs) followed by the FRI commit phase of fri::prover (prover.rs:460-470) on the
 * batched column sum_c alpha^c col_c.  Rank r passes its columns [r w_local, (r+1) w_local) as a
 * DEVICE buffer d_cols (column-major, bit-reversed rows, Montgomery form, n = 2^log_n) and two
 * device exchange buffers of 2n * w_local words; alltoall(ctx) must exchange equal blocks of
 * d_send into d_recv (block j to rank j, e.g. ncclAllToAll / torch all_to_all_single), and
 * allgather is as above.  out receives [root (8) | FRI roots (8 per round) | final value (4)]
 * (*nwords words, identical on every rank and to world = 1).  cap = capacity of out in words.
 * As above, the allgather buffers are device pointers. */
typedef int (*bfz_alltoall_fn)(void* ctx);
int bfz_commit_fri_sharded(const uint32_t* d_cols, int log_n, size_t w_local, int rank, int world,
                           uint32_t* d_send, uint32_t* d_recv, bfz_alltoall_fn alltoall,
                           bfz_allgather_fn allgather, void* ctx, uint32_t* out, size_t cap,
                           size_t* nwords);

/* ---- Constraint checker: the reference's `--features debug` mode, on the device ----
 * Replaces debug_constraints (crates/stark/src/debug.rs:24-105), StarkMachine::debug_constraints
 * (crates/stark/src/machine.rs:288-387) and the per-kind interaction balance of
 * debug_interactions_with_all_chips (crates/stark/src/lookup/debug.rs:59-196); its per-key
 * result is bfz_record_debug_interactions / bfz_debug_interactions_traces further down.
 *
 * Every row i of a chip's trace is checked against Chip::eval (chip.rs:222-228) with row
 * (i + 1) mod height as the next row, is_first = [i == 0], is_last = [i == height - 1] and
 * is_transition = 1 - is_last (debug.rs:43-94; a 1-row trace is its own next row).  A constraint
 * is named by its 0-based position in the emission order of Chip::eval: the chip's AIR
 * constraints, then one LogUp constraint per batch of two interactions, then the first-row,
 * transition and last-row constraints of the running sum (permutation.rs:157-272).  AddSub has
 * num_constraints = 14: 0-7 AIR, 8-10 batches, 11 first-row, 12 transition, 13 last-row.
 *
 * The reference stops the process at the first failing row (debug.rs:98-103) or panics on an
 * unbalanced sum (machine.rs:337-349).  A library must not: these calls return 0 whenever the
 * check RAN, whether or not the constraints hold, and report the outcome in `ok` /
 * `failing_rows`; a negative status is a real error (bad shapes, a device error). */
#define BFZ_NUM_CHIPS 8
#define BFZ_NUM_KINDS 8 /* LookupKind argument index 1..7 (lookup/lookup.rs:17-42); 0 unused */
typedef struct {
  int32_t chip;             /* chip index, BfAir::chips() order */
  int32_t num_constraints;  /* K: constraints Chip::eval emits for this chip */
  uint64_t height;
  uint64_t failing_rows;    /* rows with at least one non-zero constraint */
  int64_t first_row;        /* the smallest failing row, -1 if none */
  int32_t first_constraint; /* the first failing index at first_row, -1 if none */
  int32_t num_batches;      /* LogUp batch constraints: indices [K - 3 - num_batches, K - 3) */
  uint32_t cumulative_sum[4];
} bfz_chip_check;
typedef struct {
  int32_t ok;            /* 1: every row of every chip holds and the total cumulative sum is 0 */
  int32_t n_chips;       /* included chips; chips[0..n_chips) in machine order */
  int32_t balance_valid; /* 1: the kind_* tables below were computed */
  int32_t _pad;
  uint32_t alpha[4], beta[4]; /* the LogUp challenges sampled from the challenger */
  uint32_t cumulative_sum[4]; /* sum of the chips' cumulative sums (machine.rs:337) */
  bfz_chip_check chips[BFZ_NUM_CHIPS];
  /* Per LookupKind and chip index, over the rows' interactions with a non-zero multiplicity
   * (lookup/debug.rs:79-116): kind_sum = sum of +-mult / (alpha + kind + sum_v beta^(v+1) val_v)
   * (a chip's sum over kinds is its cumulative sum; a balanced kind sums to 0 over the chips),
   * kind_net = sum of the signed multiplicities, sends positive, in the reference's field_to_int
   * form (lookup/debug.rs:46-54: an integer in (-p/2, p/2]), kind_count = their number. */
  uint32_t kind_sum[BFZ_NUM_KINDS][BFZ_NUM_CHIPS][4];
  int32_t kind_net[BFZ_NUM_KINDS][BFZ_NUM_CHIPS];
  uint32_t kind_count[BFZ_NUM_KINDS][BFZ_NUM_CHIPS];
} bfz_debug_report;

/* debug_constraints (debug.rs:24-105) of ONE chip, a diagnostic like bfz_perm_trace: main, prep
 * (Program / Byte, else NULL) and perm are row-major Montgomery matrices of `height` rows, perm
 * the flattened permutation trace exactly as bfz_perm_trace returns it; alpha, beta, cumsum as
 * there.  on_device = 0 runs the checker's host path (the same templates, single-threaded, no
 * device needed); 1 uploads the traces and runs the check kernel.  first_fail_per_row (optional,
 * `height` entries) receives each row's first failing index, or -1. */
int bfz_check_chip(int chip, const uint32_t* main, const uint32_t* prep, const uint32_t* perm,
                   size_t height, const uint32_t alpha[4], const uint32_t beta[4],
                   const uint32_t cumsum[4], int on_device, bfz_chip_check* out,
                   int32_t* first_fail_per_row);
/* StarkMachine::debug_constraints (machine.rs:288-387) on a device record: every chip trace is
 * generated on the device as bfz_record_prove does, alpha then beta are sampled from ch (two
 * sample_ext_element, machine.rs:300-303; ch is advanced, as in bfz_open), the permutation traces
 * are generated (machine.rs:319-335), their cumulative sums added (:337) and every included chip
 * checked (:369-384).  No LDE, no commit, no Merkle tree.  The kind_* balance table is computed
 * when the total sum is not zero (machine.rs:338-349) or when flags bit 0 is set. */
int bfz_record_debug_constraints(const bfz_pk* pk, const bfz_record* rec, bfz_challenger* ch,
                                 unsigned flags, bfz_debug_report* out);
/* The same from host main traces: arguments and validation of bfz_prove_traces, preprocessed
 * traces from the key (machine.rs:309-312). */
int bfz_debug_constraints_traces(const bfz_pk* pk, const int* chips, const uint32_t* const* traces,
                                 const size_t* heights, const size_t* widths, size_t nchips,
                                 bfz_challenger* ch, unsigned flags, bfz_debug_report* out);

/* ---- Per-key lookup discrepancies: the rest of debug_interactions_with_all_chips ----
 * Which call covers which part of crates/stark/src/lookup/debug.rs: the kind_* table of
 * bfz_debug_report above is the per-KIND balance under the LogUp challenges (what tells that
 * "Byte is off by -1"); the calls below are the per-KEY result the reference prints
 * (lookup/debug.rs:59-196): for every lookup tuple "{kind} (v0, v1, ...)" (:100) with a non-zero
 * multiplicity (:94) the sends minus the receives over all chips (:109-114,148-149), each chip's
 * share of it (:151), the chips' distinct-key counts (:153) and the verdict (:175-195).  The
 * multiset does not depend on alpha or beta, so it also shows keys that differ while the totals
 * match (:188-191).
 *
 * Records come in ascending order of (kind, then the values' canonical integers,
 * lexicographically).  This is deliberately NOT the reference's order, which sorts the keys as
 * strings (BTreeMap<String, ..>, where "10" comes before "9").  Field words are Montgomery form.
 * Every interaction is counted once: for each record the sum of chip_net is congruent to net
 * mod p. */
#define BFZ_LOOKUP_MAX_VALUES 7
typedef struct {
  int32_t kind;  /* LookupKind 1..7 */
  int32_t nvals;
  uint32_t values[BFZ_LOOKUP_MAX_VALUES]; /* Montgomery; unused entries 0 */
  int32_t net;                       /* field_to_int(sends - receives) over all chips, != 0 */
  int32_t chip_net[BFZ_NUM_CHIPS];   /* field_to_int per chip index (lookup/debug.rs:151) */
  uint32_t chip_count[BFZ_NUM_CHIPS]; /* non-zero-multiplicity interactions with this key */
  int32_t first_chip;                /* witness: the smallest (chip, row, interaction) */
  int32_t first_interaction;         /* index in sends-then-receives chain order (lookup/debug.rs:80) */
  int64_t first_row;                 /* natural row order */
} bfz_lookup_discrepancy;
typedef struct {
  int32_t balanced;         /* the reference's return value: 1 = no key with a non-zero net */
  int32_t total_net;        /* field_to_int of the sum over all keys (lookup/debug.rs:150,180) */
  uint64_t interactions;    /* non-zero-multiplicity interactions of the selected kinds */
  uint64_t distinct_keys;
  uint64_t unbalanced_keys; /* may exceed cap */
  uint64_t chip_distinct[BFZ_NUM_CHIPS]; /* "{} chip has {} distinct events" (lookup/debug.rs:153) */
  uint32_t n_written;       /* min(unbalanced_keys, cap) */
  uint32_t rounds, tag_collisions; /* diagnostics of the device path, 0 on the host path */
  uint64_t table_bytes;            /* device memory of the aggregation, 0 on the host path */
} bfz_lookup_report;

/* debug_interactions_with_all_chips on a device record (traces generated on the device as
 * bfz_record_prove does).  kinds_mask: bit k selects LookupKind k (the reference's
 * interaction_kinds); 0 or a bit outside 1..7 is an error.  out receives the first
 * min(unbalanced_keys, cap) records (cap > 0 needs out).  Returns 0 whenever the check ran; a
 * negative status is a real error: bad shapes, a bad mask, a device error, or not enough device
 * memory for the aggregation (the message names the bytes needed). */
int bfz_record_debug_interactions(const bfz_pk* pk, const bfz_record* rec, unsigned kinds_mask,
                                  bfz_lookup_report* report, bfz_lookup_discrepancy* out,
                                  size_t cap);
/* The same from host main traces (arguments and validation of bfz_debug_constraints_traces,
 * preprocessed traces from the key, machine.rs:309-312).  on_device = 0 runs the host path: the
 * same Lookup tables single-threaded over an ordered map, no device needed. */
int bfz_debug_interactions_traces(const bfz_pk* pk, const int* chips, const uint32_t* const* traces,
                                  const size_t* heights, const size_t* widths, size_t nchips,
                                  unsigned kinds_mask, int on_device, bfz_lookup_report* report,
                                  bfz_lookup_discrepancy* out, size_t cap);
/* A key that holds the program only (no preprocessed commit, no device data), for the host paths:
 * bfz_debug_interactions_traces with on_device = 0 accepts it on a machine without a GPU.  Every
 * call that needs the device key refuses it with an error. */
int bfz_setup_host(const char* elf, bfz_pk** pk);

/* ---- Per-chip uni-STARK proofs: utils::uni_stark_prove / uni_stark_verify ----
 * Replaces bf_core_machine::utils::{uni_stark_prove, uni_stark_verify}
 * (crates/core/machine/src/utils/prove.rs:97-159): p3_uni_stark::{prove, verify} of ONE chip's
 * AIR over one trace, with the machine prover's PCS and challenger, no public values
 * (utils/prove.rs:111), no LogUp and no other chip -- what the reference's chip tests run
 * (alu/mod.rs:221-245 AddSub, jump/mod.rs:34-52 Jump, memory/instructions/mod.rs:21-37
 * MemoryInstrs).  Under the uni-STARK builders a chip's send / receive are no-ops
 * (air/builder.rs:232-239,273-275), so exactly the chip's AIR constraints are proven.
 *
 * chip is one of Cpu 0, AddSub 2, Jump 3, MemoryInstrs 6, IO 7.  Program 1, Memory 4 and Byte 5
 * have no AIR constraints of their own or need a preprocessed trace, which p3_uni_stark does not
 * take: every call refuses them with a negative status.
 *
 *   bfz_uni_info    host only: the constraints the chip's AIR emits, their maximal degree and
 *                   log_quotient_degree = log2_ceil(degree - 1) (crates/stark/src/chip.rs:82-87,
 *                   without its floor of 3 for chips with interactions: there are none here),
 *                   all computed from the AIR itself.  Any output pointer may be NULL.
 *   bfz_uni_prove   trace = row-major Montgomery height x width, height a power of two in
 *                   [1, 2^23], width the chip's main width.  ch is advanced as by bfz_open (pass
 *                   a copy to keep the caller's state).  *proof (bfz_free) is the BFU1 normal
 *                   form of DESIGN.md; the same inputs give the same bytes.  A trace that
 *                   violates the AIR still proves; the verifier rejects that proof, and
 *                   bfz_uni_check (below) names the row and the constraint.  timings
 *                   (optional): main_commit_ms, quotient_ms, open_ms, fri_ms, total_ms.
 *   bfz_uni_verify  host only.  Returns 0 whenever the check RAN, like bfz_verify_batch: out->ok,
 *                   out->why ("" when ok, else the reason in the host verifier's style, e.g.
 *                   "OOD evaluation mismatch on chip AddSub"); negative for a real error (NULL
 *                   arguments, a refused chip).  ch is advanced; after an accepted proof it is
 *                   the prover's final state.
 * bfz_uni_prove and bfz_uni_verify honour bfz_set_num_queries and bfz_set_pcs_variant;
 * BFZ_UNI_OBSERVE_DEGREE=0 drops the log degree from the transcript head (decision U1 of
 * DESIGN.md §2). */
int bfz_uni_info(int chip, int* num_constraints, int* degree, int* log_quotient_degree);
int bfz_uni_prove(int chip, const uint32_t* trace, size_t height, size_t width, bfz_challenger* ch,
                  uint8_t** proof, size_t* proof_len, bfz_timings* timings);
int bfz_uni_verify(int chip, bfz_challenger* ch, const uint8_t* proof, size_t proof_len,
                   bfz_verify_outcome* out);

/* The debug half of uni_stark_prove.  In a debug build the reference's uni_stark_prove requires
 * Air<DebugConstraintBuilder> (crates/core/machine/src/utils/prove.rs:97-112): p3_uni_stark::prove
 * [p3-recalled] checks every row of the trace against the AIR and panics at the first failing
 * constraint.  bfz_uni_check is that check with the row semantics of crates/stark/src/debug.rs:43-94
 * (row i local, row (i + 1) mod height next, is_first = [i == 0], is_last = [i == height - 1],
 * is_transition = 1 - is_last; a 1-row trace is its own next row).  Only the chip's own AIR
 * constraints are evaluated -- no LogUp constraint, so no permutation trace, challenge or
 * cumulative sum is needed (bfz_check_chip is the check that has them) -- and a constraint is named
 * by its 0-based position among them, 0 .. K-1 with the K of bfz_uni_info (for AddSub the indices
 * 0-7 of bfz_chip_check's numbering).  Like the other checks it returns 0 whenever the check RAN
 * and reports the outcome in failing_rows; chips, arguments, refusals and their messages are
 * bfz_uni_prove's (a wrong width, a height that is no power of two, a word >= p: negative status).
 *   bfz_uni_check         trace as for bfz_uni_prove.  on_device = 0 runs the same row function on
 *                         the host, single-threaded, no device needed; 1 uploads the trace and runs
 *                         the check kernel.  first_fail_per_row (optional, `height` entries, natural
 *                         row order) receives each row's first failing index, or -1.
 *   bfz_record_uni_check  the chip's trace of a device record, generated on the device as
 *                         bfz_record_prove does and checked where it is.  Returns 1 when the record
 *                         does not include the chip (as bfz_trace). */
typedef struct {
  int32_t chip, num_constraints;   /* K of bfz_uni_info: the AIR's constraints only */
  uint64_t height, failing_rows;
  int64_t first_row;               /* smallest failing row, natural order; -1 if none */
  int32_t first_constraint, _pad;  /* first failing index at first_row, in eval_air's emission order */
} bfz_uni_check_result;
int bfz_uni_check(int chip, const uint32_t* trace, size_t height, size_t width, int on_device,
                  bfz_uni_check_result* out, int32_t* first_fail_per_row /* optional, natural order */);
int bfz_record_uni_check(const bfz_record* rec, int chip, bfz_uni_check_result* out);

/* uni_stark_prove (crates/core/machine/src/utils/prove.rs:97-127) of one chip of a device record:
 * the record's traces are generated on the device as bfz_record_prove does (all chips; one is
 * used) and the chip's evaluations are proven where they are -- no upload, no transpose, no copy.
 * The proof is byte-identical to bfz_uni_prove on the same chip's host trace (bfz_trace), and ch
 * ends in the same state.  Returns 1 when the record does not include the chip.  timings
 * (optional): trace_ms (the trace generation) and the stages of bfz_uni_prove. */
int bfz_record_uni_prove(const bfz_record* rec, int chip, bfz_challenger* ch,
                         uint8_t** proof, size_t* proof_len, bfz_timings* timings);

/* uni_stark_verify (crates/core/machine/src/utils/prove.rs:129-159) of n proofs with
 * bfz_verify_batch's contract: proof i is of chip chips[i] and is checked against its own
 * challenger chs[i], which is advanced as by bfz_uni_verify.  Returns 0 whenever the check RAN
 * (n = 0 is a no-op); negative for a real error (NULL arguments, a refused chip, on_device = 1
 * without a bound device).  on_device = 0 is bfz_uni_verify proof by proof; on_device = 1 runs
 * everything before and after the query loops on the host and all the proofs' query loops in one
 * batched device pass (the kernels of bfz_verify_batch, two input rounds per proof), with the same
 * (ok, query, why) and the same ending challengers for the same bytes.  Honours
 * bfz_set_num_queries, bfz_set_pcs_variant, BFZ_UNI_OBSERVE_DEGREE and fault-injection bit 1. */
int bfz_uni_verify_batch(const int* chips, bfz_challenger* chs, const uint8_t* const* proofs,
                         const size_t* lens, size_t n, int on_device, bfz_verify_outcome* out);

/* ---- Caller-defined AIRs as constraint programs ----
 * utils::uni_stark_prove / uni_stark_verify are generic over A: Air
 * (crates/core/machine/src/utils/prove.rs:97-159); the bfz_uni_* calls above take the five chips
 * compiled into the library.  Here the AIR arrives as data, so a new chip, or one changed
 * constraint, is proven, row-checked and verified without rebuilding the library.  As above,
 * send / receive are no-ops (air/builder.rs:232-239,273-275): no preprocessed columns, no public
 * values, no extension-field columns.
 *
 * The program format "BFA1": little-endian u32 words, field constants as Montgomery words.
 *     "BFA1" | width | n_nodes | n_constraints
 *     n_nodes x (op, a, b)
 *     n_constraints x node index          -- emission order (acc = acc * alpha + c)
 *   op 0 CONST (a = a word < p), 1 LOCAL (a = column), 2 NEXT (a = column), 3 IS_FIRST_ROW,
 *   4 IS_LAST_ROW, 5 IS_TRANSITION, 6 ADD, 7 SUB, 8 MUL, 9 NEG (a only).  Unused operands are 0;
 *   the operands of ops 6-9 are indices of EARLIER nodes (p3's SymbolicExpression [p3-recalled]
 *   written flat, already in topological order).
 * A constraint's degree follows SymbolicExpression::degree_multiple: a trace variable 1, a
 * constant 0, is_first_row / is_last_row 1, is_transition 0, add / sub the maximum, mul the sum,
 * neg the identity; the AIR's degree is the maximum, log_quotient_degree = log2_ceil(degree - 1).
 * Every call validates the program first (a malformed one: negative status, the message names the
 * word offset) and refuses a degree above 3 and a program whose compiled instruction list keeps
 * more than BFZ_AIR_MAX_LIVE values live at once (the message names the count).
 *
 *   bfz_air_export  host only: the BFA1 program of a built-in chip's AIR (the chips of
 *                   bfz_uni_info, the same refusals); *prog is freed with bfz_free.  Proofs and
 *                   checks made from it equal the compiled chip's byte for byte.
 *   bfz_air_info    host only: validates, and reports the shape and the compiled list's size.
 *   bfz_air_eval    host only: the K constraint values over extension-field rows.  local / next:
 *                   width x 4 Montgomery words; the selectors 4 words each; out: K x 4.
 *   bfz_air_check   bfz_uni_check for a program: out->chip = -1; first_fail_per_row optional,
 *                   natural order.
 *   bfz_air_prove   bfz_uni_prove's contract: the same refusals for height, width and words >= p,
 *                   ch is advanced, a trace that violates the AIR still proves, and it honours
 *                   bfz_set_num_queries, bfz_set_pcs_variant and BFZ_UNI_OBSERVE_DEGREE.  The proof
 *                   is BFU1 with the chip word BFZ_AIR_CHIP, a label outside the transcript.  Like
 *                   p3_uni_stark, the AIR itself is NOT bound into the transcript: a verifier must
 *                   know which program a proof is for.
 *   bfz_air_verify  bfz_uni_verify's contract; returns 0 whenever the check RAN.  The AIR is the
 *                   caller's program, so the proof's chip word is not interpreted, and the chip
 *                   name in a reason reads "custom" ("OOD evaluation mismatch on chip custom").
 * bfz_uni_verify rejects a BFZ_AIR_CHIP proof with "proof is for another chip". */
#define BFZ_AIR_MAX_WIDTH 64        /* the library's column maps are 64 wide */
#define BFZ_AIR_MAX_NODES 4096
#define BFZ_AIR_MAX_CONSTRAINTS 512
#define BFZ_AIR_MAX_LIVE 32         /* the interpreter's slot count */
#define BFZ_AIR_CHIP 0xffffffffu    /* chip word of a BFU1 proof made from a program */
typedef struct {
  int32_t width, num_nodes, num_constraints, degree, log_quotient_degree;
  int32_t instructions, live_values, _pad;   /* of the compiled list */
} bfz_air_shape;
int bfz_air_export(int chip, uint8_t** prog, size_t* len);
int bfz_air_info(const uint8_t* prog, size_t len, bfz_air_shape* out);
int bfz_air_eval(const uint8_t* prog, size_t len, const uint32_t* local, const uint32_t* next,
                 const uint32_t is_first[4], const uint32_t is_last[4],
                 const uint32_t is_transition[4], uint32_t* out);
int bfz_air_check(const uint8_t* prog, size_t len, const uint32_t* trace, size_t height,
                  size_t width, int on_device, bfz_uni_check_result* out,
                  int32_t* first_fail_per_row);
int bfz_air_prove(const uint8_t* prog, size_t len, const uint32_t* trace, size_t height,
                  size_t width, bfz_challenger* ch, uint8_t** proof, size_t* proof_len,
                  bfz_timings* timings);
int bfz_air_verify(const uint8_t* prog, size_t len, bfz_challenger* ch, const uint8_t* proof,
                   size_t proof_len, bfz_verify_outcome* out);

/* FRI_QUERIES (kb31_poseidon2.rs:59-62): 1..4096, or 0 = environment FRI_QUERIES / 84. */
int bfz_set_num_queries(int num_queries);

/* PCS transcript variant, decision D1 of DESIGN.md §2 ([p3-recalled] TwoAdicFriPcs::open at
 * zkMIPS/Plonky3 93967fce): 1 = every opened value is observed before the FRI batching
 * challenge alpha is sampled (default), 0 = alpha is sampled first; -1 = environment
 * BFZ_OBSERVE_OPENINGS.  Applies to bfz_prove*, bfz_verify*, identically in the oracle. */
int bfz_set_pcs_variant(int observe_openings);

/* Test-only fault injection, no reference counterpart: bit 0 perturbs the device challenger's
 * uploaded sponge state, so the host's replay of the device-sampled challenges must fail the
 * proof with "device transcript diverged" (tests/test_gpu.py).  Bit 1 makes bfz_verify_batch and
 * bfz_uni_verify_batch with on_device = 1 run their host side only (stages, packing, the queries
 * the packing keeps on the host) with a stand-in for the kernels that reports no failure and needs
 * no device, so that side is testable without a GPU (tests/test_verify_batch.py,
 * tests/test_uni_device.py); its verdicts are then not a verification.  Bit 2 cuts the key hash of the device path of bfz_*_debug_interactions to its low
 * 12 bits before anything uses it (home slot and tag alike), so distinct keys share tags and the
 * multi-round path runs; verdicts and records must not change.  0 (default) = off. */
int bfz_set_fault_injection(int mask);

/* Proof wire format.  bfz_prove* return the BFZ1 normal form; bfz_proof_to_bincode turns it
 * into the reference's bytes: bincode::serialize(&MachineProof<KoalaBearPoseidon2>)
 * (crates/core/machine/src/utils/prove.rs:46), i.e. ShardProof (crates/stark/src/types.rs:66-73)
 * with bincode 1.x default options, chip_ordering entries in proof order.  field_repr selects
 * how a KoalaBear word is serialized: 0 = Montgomery word (p3 MontyField31 serde, default,
 * [p3-recalled]), 1 = canonical value.  bfz_proof_from_bincode is the inverse;
 * bfz_verify_bincode verifies the bincode bytes directly.  *out is malloc'd (bfz_free). */
int bfz_proof_to_bincode(const uint8_t* proof, size_t len, int field_repr, uint8_t** out,
                         size_t* out_len);
int bfz_proof_from_bincode(const uint8_t* bytes, size_t len, int field_repr, uint8_t** out,
                           size_t* out_len);
int bfz_verify_bincode(const char* elf, const uint32_t vk_commit[8], const uint8_t* bytes,
                       size_t len, int field_repr);

int bfz_coset_lde(const uint32_t* evals, size_t n, size_t w, uint32_t shift, uint32_t* lde_out);
/* Test hooks of the NTT / LDE kernels (tests/test_ntt_paths_gpu.py).  Host layouts as
 * bfz_coset_lde: row-major natural-order input in Montgomery words, row-major output in device
 * (bit-reversed) row order.  Each call allocates its device buffers itself; every output buffer
 * has 64 words of 0xFFFFFFFF before and after it, checked after the run (an overwritten one is an
 * error naming the buffer), and starts as all 0xFFFFFFFF, so a word the call leaves unwritten
 * comes back as that.
 *
 * bfz_coset_lde_ex: the prover's coset_lde_ex.  The source columns lie src_stride >= n words apart
 * and src_skew (0..3) words past a 16-byte boundary; only_half 0 / 1 writes LDE rows [0, n) /
 * [n, 2n) only, -1 both.  mode bit 0 (in place, needs only_half 0 or 1, src_stride 2n, no skew):
 * the source is half 1 - only_half of the output buffer itself, as the quotient chunks call it.
 * mode bit 1: heights up to 2^8 take the general three-launch path instead of the one-block kernel.
 *
 * bfz_lde_shard: the sharded LDE of rank `rank` of 2^log_world, through the dispatch of a sharded
 * proof: shard_out (m x w, m = 2n / 2^log_world) = LDE rows [rank m, (rank + 1) m); next_out
 * (m x n_next) = the rows of next_rank's block for the columns next_cols; coef_out (n x w) = n times
 * the interpolant's coefficients, everywhere from the unfused path; the fused path stores them for
 * [j0, j0 + len) only and leaves the inverse DFT's first-pass values in every other word (coef_out and next_out may be NULL: not fetched).  flags: bit 0 unfused, bit 1 no half-LDE kernel at two ranks, bit 2 no fused DIF
 * stages (this call only; the BFZ_FUSED_RESIDUE, BFZ_MID_HALF, BFZ_FUSED_DIF switches are not read).
 * *dft_low_out: the stage the fused kernel left the forward DFT at (-1: all of it), -2 = unfused.
 *
 * bfz_ntt_last_paths: the kernel families the calling thread's last call of either hook launched
 * (csrc/ntt.h NTT_* bits). */
int bfz_coset_lde_ex(const uint32_t* evals, size_t n, size_t w, size_t src_stride, int src_skew,
                     uint32_t shift, int only_half, int mode, uint32_t* lde_out);
int bfz_lde_shard(const uint32_t* evals, size_t n, size_t w, uint32_t shift, int log_world, int rank,
                  int next_rank, const int* next_cols, size_t n_next, size_t j0, size_t len,
                  int flags, uint32_t* coef_out, uint32_t* shard_out, uint32_t* next_out,
                  int* dft_low_out);
int bfz_ntt_last_paths(uint32_t* mask_out);
int bfz_commit(const uint32_t* const* mats, const size_t* heights, const size_t* widths,
               size_t nmats, uint32_t root[8]);
int bfz_poseidon2_permute(uint32_t* states, size_t n);
/* The latency-optimised form used for small Merkle layers (16 lanes per state, DPP). */
int bfz_poseidon2_permute_small(uint32_t* states, size_t n);

#ifdef __cplusplus
}
#endif
#endif
