"""Python mirror of the reference SDK (crates/sdk/src/lib.rs, action.rs, proof.rs) over the
bfz C ABI.  Same names, argument meaning and error behaviour:

    client = ProverClient()                      # ProverClient::new        lib.rs:31-33
    out = client.execute(elf, stdin).run()       # ProverClient::execute    lib.rs:57-59
    pk, vk = client.setup(elf)                   # ProverClient::setup      lib.rs:133-135
    proof = client.prove(pk, stdin).run()        # ProverClient::prove      lib.rs:92-94
    client.verify(proof, vk)                     # ProverClient::verify     lib.rs:110-116

and of the core MachineProver boundary (crates/stark/src/prover.rs:27-150):

    traces = generate_traces(elf, stdin)         # generate_traces          prover.rs:58-81
    prover = CoreProver()
    data = prover.commit(pk, traces)             # MachineProver::commit    prover.rs:209-236
    ch = prover.new_challenger()
    prover.observe_into(pk, ch)                  # pk.observe_into          prover.rs:595-601
    proof = prover.open(pk, data, ch)            # MachineProver::open      prover.rs:242-553
    proof = prover.prove(pk, traces)             # MachineProver::prove     prover.rs:560-582

and of the reference's debug mode (crates/stark/src/machine.rs:288-387, debug.rs:24-105):

    report = client.debug_constraints(pk, stdin) # StarkMachine::debug_constraints on the device
    report = prover.debug_constraints(pk, traces)
    print(report)                                # chip, row and constraint of the first failure
    lookups = client.debug_interactions(pk, stdin)   # debug_interactions_with_all_chips
    lookups = prover.debug_interactions(pk, traces)  # (lookup/debug.rs:125-196): per-key
    print(lookups)                                   # send-receive discrepancies

and of the per-chip uni-STARK helpers (crates/core/machine/src/utils/prove.rs:97-159):

    res = uni_stark_check(chip, trace)           # the debug-build row check of uni_stark_prove
    proof = uni_stark_prove(chip, trace, check=True)
    proofs = client.uni_stark_prove_record(pk, stdin)    # from the traces the device generates
    outcomes = uni_stark_verify_batch(chips, proofs)     # query phase on the device

Errors raise (the reference returns Err / panics in the same places).  Proving runs on the GPU
through libbfz; verification runs the host verifier compiled into the same library.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Dict, List, Optional

from . import _lib
from ._lib import BfzError, Challenger, check, init, lib, take_bytes, u8buf


@dataclass
class BfVerifyingKey:
    """StarkVerifyingKey: preprocessed commitment (Montgomery u32 x 8) + the program that
    determines chip_information (crates/prover/src/types.rs:17-20)."""
    commit: List[int]
    elf: str


@dataclass
class BfProvingKey:
    """BfProvingKey (crates/prover/src/types.rs:8-15): device-resident pk + elf + vk."""
    handle: int
    elf: str
    vk: BfVerifyingKey

    def __del__(self):
        try:
            if self.handle:
                lib().bfz_pk_free(ctypes.c_void_p(self.handle))
                self.handle = 0
        except Exception:
            pass


# KoalaBear word representation inside bincode (bfz_proof_to_bincode): the p3 MontyField31
# serde writes the Montgomery word [p3-recalled]; CANONICAL is the alternative.
FIELD_MONTGOMERY, FIELD_CANONICAL = 0, 1


def proof_to_bincode(proof: bytes, field_repr: int = FIELD_MONTGOMERY) -> bytes:
    """BFZ1 normal form -> bincode::serialize(&ShardProof<KoalaBearPoseidon2>) bytes
    (crates/stark/src/types.rs:66-73, crates/core/machine/src/utils/prove.rs:46)."""
    buf, n = u8buf(proof)
    ptr = ctypes.POINTER(ctypes.c_uint8)()
    olen = ctypes.c_size_t()
    check(lib().bfz_proof_to_bincode(buf, n, int(field_repr), ctypes.byref(ptr), ctypes.byref(olen)))
    return take_bytes(ptr, olen.value)


def proof_from_bincode(data: bytes, field_repr: int = FIELD_MONTGOMERY) -> bytes:
    """bincode ShardProof bytes -> BFZ1 normal form (chip_ordering applied)."""
    buf, n = u8buf(data)
    ptr = ctypes.POINTER(ctypes.c_uint8)()
    olen = ctypes.c_size_t()
    check(lib().bfz_proof_from_bincode(buf, n, int(field_repr), ctypes.byref(ptr),
                                       ctypes.byref(olen)))
    return take_bytes(ptr, olen.value)


@dataclass
class BfProofWithPublicValues:
    """crates/sdk/src/proof.rs:10-13 — the proof (BFZ1 normal-form bytes) and stdin.

    `to_bincode()` gives the reference's serialized form of this struct, bincode of
    { proof: ShardProof<CoreSC>, stdin: Vec<u8> }; `from_bincode()` reads it back."""
    proof: bytes
    stdin: bytes
    public_values: bytes = b""
    cycles: int = 0

    def to_bincode(self, field_repr: int = FIELD_MONTGOMERY) -> bytes:
        import struct
        return (proof_to_bincode(self.proof, field_repr) + struct.pack("<Q", len(self.stdin))
                + bytes(self.stdin))

    @staticmethod
    def from_bincode(data: bytes, field_repr: int = FIELD_MONTGOMERY) -> "BfProofWithPublicValues":
        import struct
        # the ShardProof is everything before the trailing Vec<u8> stdin; its length is found by
        # trying the stdin lengths the tail can hold (the u64 prefix sits right before stdin)
        for k in range(0, len(data) - 7):
            cut = len(data) - k - 8
            if cut < 0:
                break
            if struct.unpack_from("<Q", data, cut)[0] == k:
                try:
                    pf = proof_from_bincode(data[:cut], field_repr)
                except BfzError:
                    continue
                return BfProofWithPublicValues(proof=pf, stdin=bytes(data[cut + 8:]))
        raise BfzError("not a bincode BfProofWithPublicValues")


@dataclass
class VerifyOutcome:
    """bfz_verify_outcome: ok, the query whose check failed first (-1 if the rejection is not a
    query's) and the host verifier's reason ("" when ok)."""
    ok: bool
    query: int
    why: str


class Execute:
    """action::Execute (crates/sdk/src/action.rs:10-33)."""

    def __init__(self, elf: str, stdin: bytes):
        self.elf, self.stdin = elf, bytes(stdin)

    def run(self) -> bytes:
        buf, n = u8buf(self.stdin)
        cap = 1 << 20
        out = (ctypes.c_uint8 * cap)()
        olen = ctypes.c_size_t()
        cyc = ctypes.c_uint64()
        check(lib().bfz_execute(self.elf.encode(), buf, n, out, cap, ctypes.byref(olen),
                                ctypes.byref(cyc)))
        return bytes(out[: min(olen.value, cap)])


class Prove:
    """action::Prove (crates/sdk/src/action.rs:35-61)."""

    def __init__(self, pk: BfProvingKey, stdin: bytes):
        self.pk, self.stdin = pk, bytes(stdin)

    def run(self) -> BfProofWithPublicValues:
        init()
        buf, n = u8buf(self.stdin)
        ptr = ctypes.POINTER(ctypes.c_uint8)()
        plen = ctypes.c_size_t()
        check(lib().bfz_prove(ctypes.c_void_p(self.pk.handle), buf, n, ctypes.byref(ptr),
                              ctypes.byref(plen)))
        return BfProofWithPublicValues(proof=take_bytes(ptr, plen.value), stdin=self.stdin,
                                       public_values=Execute(self.pk.elf, self.stdin).run())


class ProverClient:
    """crates/sdk/src/lib.rs:20-136, backed by the MI355X prover."""

    def __init__(self, device: int = 0):
        self.device = device

    @staticmethod
    def new() -> "ProverClient":
        return ProverClient()

    def execute(self, elf: str, stdin) -> Execute:
        return Execute(elf, bytes(stdin))

    def setup(self, elf: str):
        init(self.device)
        h = ctypes.c_void_p()
        commit = (ctypes.c_uint32 * 8)()
        check(lib().bfz_setup(elf.encode(), ctypes.byref(h), commit))
        vk = BfVerifyingKey(commit=list(commit), elf=elf)
        return BfProvingKey(handle=h.value, elf=elf, vk=vk), vk

    def prove(self, pk: BfProvingKey, stdin) -> Prove:
        return Prove(pk, bytes(stdin))

    def prove_batch(self, pk: BfProvingKey, stdins, exec_threads: int = 0,
                    public_values: bool = True, stats: Optional[dict] = None):
        """Proofs of pk's program over many inputs, pipelined (bfz_prove_batch): executions run
        on host threads and uploads on a copy stream while the GPU proves the previous job.
        Each proof equals prove(pk, stdin).run()'s; stats (a dict) receives the batch timings."""
        init(self.device)
        ins = [bytes(x) for x in stdins]
        k = len(ins)
        bufs = [u8buf(x) for x in ins]
        arr = (ctypes.POINTER(ctypes.c_uint8) * max(k, 1))(
            *[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b, _ in bufs])
        lens = (ctypes.c_size_t * max(k, 1))(*[n for _, n in bufs])
        outs = (ctypes.POINTER(ctypes.c_uint8) * max(k, 1))()
        olens = (ctypes.c_size_t * max(k, 1))()
        st = _lib.BatchStats()
        check(lib().bfz_prove_batch(ctypes.c_void_p(pk.handle), arr, lens, k, int(exec_threads),
                                    outs, olens, ctypes.byref(st)))
        proofs = [take_bytes(outs[i], olens[i]) for i in range(k)]
        if stats is not None:
            stats.update({name: getattr(st, name) for name, _ in st._fields_})
        return [BfProofWithPublicValues(
            proof=pf, stdin=x,
            public_values=Execute(pk.elf, x).run() if public_values else b"")
            for pf, x in zip(proofs, ins)]

    def verify(self, proof: BfProofWithPublicValues, vk: BfVerifyingKey,
               on_device: bool = False) -> None:
        """ProverClient::verify (lib.rs:110-116).  on_device=True runs the query phase on the GPU
        (bfz_verify_batch); the verdict and the reason of a rejection are the host verifier's."""
        if on_device:
            o = self.verify_batch([proof], vk, on_device=True)[0]
            if not o.ok:
                raise BfzError(f"verification failed: {o.why}")
            return
        buf, n = u8buf(proof.proof)
        commit = (ctypes.c_uint32 * 8)(*vk.commit)
        check(lib().bfz_verify(vk.elf.encode(), commit, buf, n))

    def verify_batch(self, proofs, vk: BfVerifyingKey, on_device: bool = True) -> List[VerifyOutcome]:
        """StarkMachine::verify (crates/stark/src/machine.rs:258-284) of many proofs of vk's
        program (bfz_verify_batch): BfProofWithPublicValues or BFZ1 bytes.  A rejected proof does
        not raise; its outcome says which query failed first (if one did) and why.
        on_device=True checks every proof's query phase in one batched GPU pass; False runs the
        host verifier proof by proof.  Both give the same outcomes."""
        if on_device:
            init(self.device)
        raw = [bytes(p.proof if isinstance(p, BfProofWithPublicValues) else p) for p in proofs]
        k = len(raw)
        bufs = [u8buf(x) for x in raw]
        arr = (ctypes.POINTER(ctypes.c_uint8) * max(k, 1))(
            *[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b, _ in bufs])
        lens = (ctypes.c_size_t * max(k, 1))(*[n for _, n in bufs])
        out = (_lib.VerifyOutcomeC * max(k, 1))()
        commit = (ctypes.c_uint32 * 8)(*vk.commit)
        check(lib().bfz_verify_batch(vk.elf.encode(), commit, arr, lens, k, int(bool(on_device)), out))
        return [VerifyOutcome(ok=bool(out[i].ok), query=out[i].query, why=out[i].why.decode())
                for i in range(k)]

    def verify_bincode(self, shard_proof: bytes, vk: BfVerifyingKey,
                       field_repr: int = FIELD_MONTGOMERY) -> None:
        """StarkMachine::verify on the reference's bincode ShardProof bytes."""
        buf, n = u8buf(shard_proof)
        commit = (ctypes.c_uint32 * 8)(*vk.commit)
        check(lib().bfz_verify_bincode(vk.elf.encode(), commit, buf, n, int(field_repr)))


# BfAir::chips() order (crates/core/machine/src/brainfuck/mod.rs:53-81) = chip index in the ABI
CHIPS = ("Cpu", "Program", "AddSub", "Jump", "Memory", "Byte", "MemoryInstrs", "IO")


def generate_traces(elf: str, stdin) -> list:
    """Execute + generate_dependencies + generate_traces: [(chip index, name, trace)] for the
    chips the record includes, each trace a (height, width) uint32 array in Montgomery form
    (the byte layout of the reference's RowMajorMatrix<KoalaBear>)."""
    import numpy as np
    buf, n = u8buf(bytes(stdin))
    out = []
    for c, name in enumerate(CHIPS):
        p = ctypes.POINTER(ctypes.c_uint32)()
        h, w = ctypes.c_size_t(), ctypes.c_size_t()
        rc = lib().bfz_trace(elf.encode(), buf, n, c, 0, ctypes.byref(p), ctypes.byref(h),
                             ctypes.byref(w))
        if rc == 1:
            continue
        check(rc)
        arr = np.ctypeslib.as_array(p, shape=(h.value * w.value,)).copy()
        lib().bfz_free(p)
        out.append((c, name, arr.reshape(h.value, w.value)))
    return out


def _trace_args(traces):
    import numpy as np
    mats = [np.ascontiguousarray(t, dtype=np.uint32) for _, _, t in traces]
    k = len(mats)
    chips = (ctypes.c_int * k)(*[c for c, _, _ in traces])
    ptrs = (ctypes.POINTER(ctypes.c_uint32) * k)(
        *[m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) for m in mats])
    hs = (ctypes.c_size_t * k)(*[m.shape[0] for m in mats])
    ws = (ctypes.c_size_t * k)(*[m.shape[1] for m in mats])
    return mats, chips, ptrs, hs, ws, k


class ShardMainData:
    """ShardMainData (crates/stark/src/types.rs:13-18) held in HBM by libbfz: the main traces'
    evaluations, LDEs and Merkle tree; main_commit is its root (8 Montgomery words)."""

    def __init__(self, handle: int, main_commit):
        self.handle = handle
        self.main_commit = list(main_commit)

    def __del__(self):
        if getattr(self, "handle", None):
            lib().bfz_main_data_free(ctypes.c_void_p(self.handle))
            self.handle = None


class CoreProver:
    """HIP implementation of the MachineProver trait (crates/stark/src/prover.rs:27-150) from
    host traces: `commit` (:209-236), `observe_into` (MachineProvingKey, :595-601), `open`
    (:242-553) and the default `prove` (:560-582) = commit + open on a clone of the
    challenger.  Every step runs on the device; the challenger is plain data (Challenger)."""

    def commit(self, pk: BfProvingKey, traces) -> ShardMainData:
        init()
        mats, chips, ptrs, hs, ws, k = _trace_args(traces)
        out = ctypes.c_void_p()
        root = (ctypes.c_uint32 * 8)()
        check(lib().bfz_main_commit(ctypes.c_void_p(pk.handle), chips, ptrs, hs, ws, k,
                                    ctypes.byref(out), root))
        return ShardMainData(out.value, root)

    def commit_record(self, pk: BfProvingKey, record_handle: int) -> ShardMainData:
        """commit from a device-resident record (bfz_record_new): traces generated on device."""
        init()
        out = ctypes.c_void_p()
        root = (ctypes.c_uint32 * 8)()
        check(lib().bfz_record_main_commit(ctypes.c_void_p(pk.handle),
                                           ctypes.c_void_p(record_handle), ctypes.byref(out), root))
        return ShardMainData(out.value, root)

    @staticmethod
    def new_challenger() -> Challenger:
        return Challenger()  # DuplexChallenger::new: all zero, empty buffers

    def observe_into(self, pk: BfProvingKey, ch: Challenger) -> None:
        check(lib().bfz_challenger_observe_pk(ctypes.c_void_p(pk.handle), ctypes.byref(ch)))

    def open(self, pk: BfProvingKey, data: ShardMainData, ch: Challenger) -> bytes:
        ptr = ctypes.POINTER(ctypes.c_uint8)()
        plen = ctypes.c_size_t()
        check(lib().bfz_open(ctypes.c_void_p(pk.handle), ctypes.c_void_p(data.handle),
                             ctypes.byref(ch), ctypes.byref(ptr), ctypes.byref(plen)))
        return take_bytes(ptr, plen.value)

    def prove(self, pk: BfProvingKey, traces) -> bytes:
        """One call (bfz_prove_traces): same bytes as commit + observe_into + open."""
        init()
        mats, chips, ptrs, hs, ws, k = _trace_args(traces)
        ptr = ctypes.POINTER(ctypes.c_uint8)()
        plen = ctypes.c_size_t()
        check(lib().bfz_prove_traces(ctypes.c_void_p(pk.handle), chips, ptrs, hs, ws, k,
                                     ctypes.byref(ptr), ctypes.byref(plen)))
        return take_bytes(ptr, plen.value)


@dataclass
class StarkProvingKey:
    """StarkProvingKey on the host (crates/stark/src/machine.rs:49-60) as pk_to_host returns it:
    the preprocessed commit and traces in the key's order (sorted (Reverse(height), name),
    machine.rs:182-183), chip_ordering and local_only.  traces: [(chip id, name, array)] with
    each array the row-major Montgomery matrix (RowMajorMatrix<KoalaBear>::values)."""
    commit: List[int]
    traces: list
    chip_ordering: dict
    local_only: list


class DeviceProvingKey:
    """MachineProver::DeviceProvingKey made by pk_to_device (a bfz_pk handle, freed on drop)."""

    def __init__(self, handle: int, commit):
        self.handle = handle
        self.commit = list(commit)

    def __del__(self):
        if getattr(self, "handle", None):
            lib().bfz_pk_free(ctypes.c_void_p(self.handle))
            self.handle = None


# local_only per chip (Chip::local_only; the preprocessed chips Program and Byte are not)
_LOCAL_ONLY = {"Cpu": False, "Program": False, "AddSub": True, "Jump": True, "Memory": False,
               "Byte": False, "MemoryInstrs": False, "IO": True}


def _pk_to_host(pk) -> StarkProvingKey:
    import numpy as np
    commit = (ctypes.c_uint32 * 8)()
    check(lib().bfz_pk_commit(ctypes.c_void_p(pk.handle), commit))
    named = []
    for c, name in enumerate(CHIPS):
        p = ctypes.POINTER(ctypes.c_uint32)()
        h, w = ctypes.c_size_t(), ctypes.c_size_t()
        buf, n = u8buf(b"")
        rc = lib().bfz_trace(pk.elf.encode(), buf, n, c, 1, ctypes.byref(p), ctypes.byref(h),
                             ctypes.byref(w))
        if rc == 1:
            continue
        check(rc)
        arr = np.ctypeslib.as_array(p, shape=(h.value * w.value,)).copy().reshape(h.value, w.value)
        lib().bfz_free(p)
        named.append((c, name, arr))
    named.sort(key=lambda t: (-t[2].shape[0], t[1]))  # machine.rs:182-183
    return StarkProvingKey(commit=list(commit), traces=named,
                           chip_ordering={name: i for i, (_, name, _) in enumerate(named)},
                           local_only=[_LOCAL_ONLY[name] for _, name, _ in named])


def _pk_to_device(hpk: StarkProvingKey) -> DeviceProvingKey:
    mats, chips, ptrs, hs, ws, k = _trace_args(hpk.traces)
    commit = (ctypes.c_uint32 * 8)(*hpk.commit)
    out = ctypes.c_void_p()
    check(lib().bfz_pk_from_host(chips, ptrs, hs, ws, k, commit, ctypes.byref(out)))
    return DeviceProvingKey(out.value, hpk.commit)


CoreProver.pk_to_host = staticmethod(_pk_to_host)
CoreProver.pk_to_host.__doc__ = "MachineProver::pk_to_host (prover.rs:55,205-207)."
CoreProver.pk_to_device = staticmethod(_pk_to_device)
CoreProver.pk_to_device.__doc__ = ("MachineProver::pk_to_device (prover.rs:52,201-203) -> "
                                   "bfz_pk_from_host: refuses traces or a commit that do not match.")


@dataclass
class HostBfProvingKey:
    """BfProvingKey (crates/prover/src/types.rs:8-15) exactly as BfProver::setup builds it:
    the HOST key pk_to_host(pk), the elf and the vk (crates/prover/src/lib.rs:46-56)."""
    pk: StarkProvingKey
    elf: str
    vk: BfVerifyingKey


class BfProver:
    """BfProver<HipProverComponents> (crates/prover/src/lib.rs:28-90) -- the reference's own
    flow around the HIP core prover:
      setup: MachineProver::setup, keep pk_to_host(pk)                       (lib.rs:46-56)
      prove: pk_to_device(pk.pk) every time, Executor::run, then the HipProver::prove override:
             observe_into, bfz_record_from_events (the record's events to HBM, traces and
             byte-lookup multiplicities generated there), commit, open on a clone (lib.rs:70-90,
             utils/prove.rs:23-66, prover.rs:560-582)."""

    def __init__(self):
        self.core = CoreProver()

    def setup(self, elf: str):
        init()
        h = ctypes.c_void_p()
        commit = (ctypes.c_uint32 * 8)()
        check(lib().bfz_setup(elf.encode(), ctypes.byref(h), commit))
        vk = BfVerifyingKey(commit=list(commit), elf=elf)
        dpk = BfProvingKey(handle=h.value, elf=elf, vk=vk)
        pk = HostBfProvingKey(pk=self.core.pk_to_host(dpk), elf=elf, vk=vk)
        del dpk  # the device key is dropped, as the reference keeps only the host key
        return pk, vk

    def prove(self, pk: HostBfProvingKey, stdin) -> BfProofWithPublicValues:
        from .events import ExecutionRecordArrays, record_from_events
        dpk = self.core.pk_to_device(pk.pk)                         # lib.rs:76
        rec = ExecutionRecordArrays.from_executor(pk.elf, stdin)    # Executor::run
        ch = self.core.new_challenger()                             # config().challenger()
        self.core.observe_into(dpk, ch)                             # prover.rs:572
        drec = record_from_events(dpk, rec)
        data = self.core.commit_record(dpk, drec.handle)
        opened = Challenger.from_buffer_copy(bytes(ch))             # challenger.clone()
        proof = self.core.open(dpk, data, opened)                   # prover.rs:578
        return BfProofWithPublicValues(proof=proof, stdin=bytes(stdin), public_values=rec.output,
                                       cycles=rec.global_clk)

    def verify(self, proof: BfProofWithPublicValues, vk: BfVerifyingKey) -> None:
        ProverClient().verify(proof, vk)


# LookupKind argument index (crates/stark/src/lookup/lookup.rs:17-42) -> name
KINDS = (None, "Memory", "Program", "Alu", "Jump", "MemInstr", "IO", "Byte")


def constraint_name(index: int, num_constraints: int, num_batches: int) -> str:
    """What constraint `index` of a chip with K = num_constraints is, in Chip::eval's emission
    order (crates/stark/src/chip.rs:222-228): AIR constraints, one LogUp constraint per batch,
    then the running sum's first-row, transition and last-row constraints
    (permutation.rs:157-272)."""
    k_air = num_constraints - num_batches - 3
    if index < 0 or index >= num_constraints:
        return "none"
    if index < k_air:
        return f"AIR constraint {index}"
    if index < k_air + num_batches:
        return f"LogUp batch {index - k_air}"
    return ("LogUp first-row", "LogUp transition", "LogUp last-row")[index - k_air - num_batches]


@dataclass
class ChipCheckResult:
    """bfz_chip_check: the row check of one chip."""
    chip: int
    height: int
    num_constraints: int
    num_batches: int
    failing_rows: int
    first_row: int
    first_constraint: int
    cumulative_sum: List[int]
    first_fail_per_row: Optional[object] = None  # numpy int32[height] when asked for

    @property
    def name(self) -> str:
        return CHIPS[self.chip]

    def __str__(self) -> str:
        head = f"{self.name:<12} {self.height:>8} rows, K = {self.num_constraints:<3}"
        if not self.failing_rows:
            return head + " ok"
        return (f"{head} FAILED: {self.failing_rows} failing row(s); first: chip {self.name}, "
                f"row {self.first_row}, constraint {self.first_constraint} of "
                f"{self.num_constraints} ("
                f"{constraint_name(self.first_constraint, self.num_constraints, self.num_batches)})")


def _chip_result(c, per_row=None) -> ChipCheckResult:
    return ChipCheckResult(chip=c.chip, height=c.height, num_constraints=c.num_constraints,
                           num_batches=c.num_batches, failing_rows=c.failing_rows,
                           first_row=c.first_row, first_constraint=c.first_constraint,
                           cumulative_sum=list(c.cumulative_sum), first_fail_per_row=per_row)


@dataclass
class DebugReport:
    """bfz_debug_report: what StarkMachine::debug_constraints (machine.rs:288-387) found.  Where
    the reference exits or panics (debug.rs:98-103, machine.rs:348), ok is False and str(report)
    names the chip, row and constraint.  kind_sum / kind_net / kind_count are indexed
    [kind][chip index] (KINDS, CHIPS) and valid when balance_valid."""
    ok: bool
    chips: List[ChipCheckResult]
    alpha: List[int]
    beta: List[int]
    cumulative_sum: List[int]
    balance_valid: bool
    kind_sum: list = field(default_factory=list)
    kind_net: list = field(default_factory=list)
    kind_count: list = field(default_factory=list)

    def failing(self) -> List[ChipCheckResult]:
        return [c for c in self.chips if c.failing_rows]

    def __str__(self) -> str:
        lines = ["constraints " + ("verified" if self.ok else "FAILED")]
        lines += ["  " + str(c) for c in self.chips]
        balanced = not any(self.cumulative_sum)
        lines.append("  cumulative sum " + ("zero" if balanced else "NOT zero: the lookups do not balance"))
        if self.balance_valid and not balanced:
            inc = [c.chip for c in self.chips]
            lines.append("  send - receive per lookup kind (count of sends minus receives; "
                         "* = the kind's LogUp sum over the chips is not zero)")
            lines.append("  " + f"{'kind':<10}" + "".join(f"{CHIPS[c]:>13}" for c in inc) + f"{'total':>13}")
            for k in range(1, len(KINDS)):
                bad = any(sum(self.kind_sum[k][c][e] for c in inc) % _P for e in range(4))
                row = "".join(f"{self.kind_net[k][c]:>13}" if self.kind_count[k][c] else f"{'.':>13}"
                              for c in inc)
                lines.append("  " + f"{KINDS[k]:<10}" + row +
                             f"{sum(self.kind_net[k][c] for c in inc):>13}" + (" *" if bad else ""))
        return "\n".join(lines)


_P = 0x7F000001


def _report(r) -> DebugReport:
    return DebugReport(
        ok=bool(r.ok), chips=[_chip_result(r.chips[i]) for i in range(r.n_chips)],
        alpha=list(r.alpha), beta=list(r.beta), cumulative_sum=list(r.cumulative_sum),
        balance_valid=bool(r.balance_valid),
        kind_sum=[[list(r.kind_sum[k][c]) for c in range(_lib.NUM_CHIPS)] for k in range(_lib.NUM_KINDS)],
        kind_net=[list(r.kind_net[k]) for k in range(_lib.NUM_KINDS)],
        kind_count=[list(r.kind_count[k]) for k in range(_lib.NUM_KINDS)])


def check_chip(chip: int, main, prep, perm, alpha, beta, cumsum, on_device: bool = False,
               per_row: bool = False) -> ChipCheckResult:
    """debug_constraints (crates/stark/src/debug.rs:24-105) of one chip (bfz_check_chip): main,
    prep (None without a preprocessed trace) and perm are (height, width) uint32 arrays in
    Montgomery form, perm flattened to base as bfz_perm_trace returns it; alpha, beta and cumsum
    are 4 Montgomery words.  on_device=False runs the host path (no GPU needed)."""
    import numpy as np
    P32 = ctypes.POINTER(ctypes.c_uint32)
    m = np.ascontiguousarray(main, dtype=np.uint32)
    pm = np.ascontiguousarray(perm, dtype=np.uint32)
    pr = None if prep is None else np.ascontiguousarray(prep, dtype=np.uint32)
    if m.ndim != 2 or pm.ndim != 2 or pm.shape[0] != m.shape[0] or (pr is not None and pr.shape[0] != m.shape[0]):
        raise BfzError("check_chip: main, prep and perm must have the same number of rows")
    if m.shape[1] != _MAIN_W[chip] or pm.shape[1] != _PERM_W[chip] or (
            pr is not None and pr.shape[1] != _PREP_W[chip]):
        raise BfzError(f"check_chip: wrong trace width for {CHIPS[chip]}")
    if on_device:
        init()
    out = _lib.ChipCheck()
    rows = np.zeros(m.shape[0], dtype=np.int32) if per_row else None
    check(lib().bfz_check_chip(
        int(chip), m.ctypes.data_as(P32), pr.ctypes.data_as(P32) if pr is not None else None,
        pm.ctypes.data_as(P32), m.shape[0], (ctypes.c_uint32 * 4)(*alpha),
        (ctypes.c_uint32 * 4)(*beta), (ctypes.c_uint32 * 4)(*cumsum), int(bool(on_device)),
        ctypes.byref(out),
        rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if per_row else None))
    return _chip_result(out, rows)


# main / preprocessed / flattened permutation widths per chip (CHIPS order)
_MAIN_W = (31, 1, 7, 45, 12, 2, 41, 5)
_PREP_W = (0, 6, 0, 0, 0, 2, 0, 0)
_PERM_W = (36, 8, 16, 8, 12, 8, 8, 8)

DEBUG_BALANCE = 1  # flags bit 0: compute the balance table even when the total sum is zero


def _debug_constraints_traces(self, pk: BfProvingKey, traces, ch: Optional[Challenger] = None,
                              flags: int = 0) -> DebugReport:
    """StarkMachine::debug_constraints (machine.rs:288-387) from host main traces
    (bfz_debug_constraints_traces): ch (default: a fresh challenger, which is what
    utils/prove.rs:60 passes) is advanced by the two challenge samples."""
    init()
    mats, chips, ptrs, hs, ws, k = _trace_args(traces)
    if ch is None:
        ch = Challenger()
    out = _lib.DebugReportC()
    check(lib().bfz_debug_constraints_traces(ctypes.c_void_p(pk.handle), chips, ptrs, hs, ws, k,
                                             ctypes.byref(ch), int(flags), ctypes.byref(out)))
    return _report(out)


def _debug_constraints_record(self, pk: BfProvingKey, stdin, ch: Optional[Challenger] = None,
                              flags: int = 0) -> DebugReport:
    """StarkMachine::debug_constraints (machine.rs:288-387) of (pk's program, stdin) on the
    device: bfz_record_new, then bfz_record_debug_constraints checks the traces the GPU proves
    from.  ch defaults to a fresh challenger (utils/prove.rs:60)."""
    init(self.device)
    buf, n = u8buf(bytes(stdin))
    rec = ctypes.c_void_p()
    cyc = ctypes.c_uint64()
    check(lib().bfz_record_new(ctypes.c_void_p(pk.handle), buf, n, ctypes.byref(rec),
                               ctypes.byref(cyc)))
    try:
        if ch is None:
            ch = Challenger()
        out = _lib.DebugReportC()
        check(lib().bfz_record_debug_constraints(ctypes.c_void_p(pk.handle), rec, ctypes.byref(ch),
                                                 int(flags), ctypes.byref(out)))
    finally:
        lib().bfz_record_free(rec)
    return _report(out)


CoreProver.debug_constraints = _debug_constraints_traces
ProverClient.debug_constraints = _debug_constraints_record


# ---- per-key lookup discrepancies (crates/stark/src/lookup/debug.rs:59-196)
_RINV = pow(1 << 32, -1, _P)  # Montgomery word -> canonical integer


@dataclass
class LookupDiscrepancy:
    """bfz_lookup_discrepancy: a lookup key whose sends and receives differ.  values are
    canonical integers; net, chip_net are field_to_int values (lookup/debug.rs:46-54);
    first_* is the smallest (chip, row, interaction) that carries the key."""
    kind: int
    values: List[int]
    net: int
    chip_net: List[int]
    chip_count: List[int]
    first_chip: int
    first_row: int
    first_interaction: int

    @property
    def key(self) -> str:
        """The reference's key string (lookup/debug.rs:100)."""
        return f"{KINDS[self.kind]} ({', '.join(str(v) for v in self.values)})"

    def lines(self) -> List[str]:
        out = [f"Lookup key: {self.key} Send-Receive Discrepancy: {self.net}"]
        for c in sorted((c for c in range(len(CHIPS)) if self.chip_count[c]), key=lambda c: CHIPS[c]):
            out.append(f" {CHIPS[c]} chip's send-receive discrepancy for this key is {self.chip_net[c]}")
        out.append(f" first seen at {CHIPS[self.first_chip]} row {self.first_row} "
                   f"interaction {self.first_interaction}")
        return out


@dataclass
class LookupReport:
    """bfz_lookup_report and its records: what debug_interactions_with_all_chips
    (lookup/debug.rs:125-196) prints and returns.  discrepancies holds the first `limit` unbalanced
    keys in (kind, values) order; unbalanced_keys counts all of them.  str(report) gives the
    reference's lines (keys in our order, not its string order) plus a witness line per key."""
    balanced: bool
    total_net: int
    interactions: int
    distinct_keys: int
    unbalanced_keys: int
    chip_distinct: List[int]
    discrepancies: List[LookupDiscrepancy]
    rounds: int = 0
    tag_collisions: int = 0
    table_bytes: int = 0
    chips: Optional[List[int]] = None  # included chips, when the caller knows them

    def __str__(self) -> str:
        inc = self.chips if self.chips is not None else [
            c for c in range(len(CHIPS)) if self.chip_distinct[c]]
        lines = [f"{CHIPS[c]} chip has {self.chip_distinct[c]} distinct events" for c in inc]
        lines += ["Final counts below.", "=================="]
        for d in self.discrepancies:
            lines += d.lines()
        if self.unbalanced_keys > len(self.discrepancies):
            lines.append(f"... {self.unbalanced_keys - len(self.discrepancies)} more unbalanced keys")
        lines.append("==================")
        if self.balanced:
            lines.append("All chips have the same number of sends and receives.")
        else:
            lines += ["Positive values mean sent more than received.",
                      "Negative values mean received more than sent."]
            if self.total_net != 0:
                lines.append(f"Total send-receive discrepancy: {self.total_net}")
                lines.append("you're sending more than you are receiving" if self.total_net > 0
                             else "you're receiving more than you are sending")
            else:
                lines += ["the total number of sends and receives match, but the keys don't match",
                          "check the arguments"]
        return "\n".join(lines)


def kinds_mask(kinds=None) -> int:
    """bit k per selected LookupKind: None = all, else kind indices or names of KINDS."""
    if kinds is None:
        return 0xFE
    m = 0
    for k in kinds:
        m |= 1 << (KINDS.index(k) if isinstance(k, str) else int(k))
    return m


def _lookup_report(rep, recs, chips=None) -> LookupReport:
    ds = []
    for i in range(rep.n_written):
        r = recs[i]
        ds.append(LookupDiscrepancy(
            kind=r.kind, values=[r.values[v] * _RINV % _P for v in range(r.nvals)], net=r.net,
            chip_net=list(r.chip_net), chip_count=list(r.chip_count), first_chip=r.first_chip,
            first_row=r.first_row, first_interaction=r.first_interaction))
    return LookupReport(
        balanced=bool(rep.balanced), total_net=rep.total_net, interactions=rep.interactions,
        distinct_keys=rep.distinct_keys, unbalanced_keys=rep.unbalanced_keys,
        chip_distinct=list(rep.chip_distinct), discrepancies=ds, rounds=rep.rounds,
        tag_collisions=rep.tag_collisions, table_bytes=rep.table_bytes, chips=chips)


def host_key(elf: str) -> BfProvingKey:
    """bfz_setup_host: a key that holds the program only, for the host paths
    (debug_interactions(..., on_device=False)) on a machine without a GPU."""
    h = ctypes.c_void_p()
    check(lib().bfz_setup_host(elf.encode(), ctypes.byref(h)))
    return BfProvingKey(handle=h.value, elf=elf, vk=BfVerifyingKey(commit=[], elf=elf))


def _debug_interactions_traces(self, pk: BfProvingKey, traces, kinds=None, limit: int = 256,
                               on_device: bool = True) -> LookupReport:
    """debug_interactions_with_all_chips (lookup/debug.rs:125-196) from host main traces
    (bfz_debug_interactions_traces).  on_device=False runs the host path (no GPU needed; pk may
    be a host_key)."""
    if on_device:
        init()
    mats, chips, ptrs, hs, ws, k = _trace_args(traces)
    rep = _lib.LookupReportC()
    recs = (_lib.LookupDiscrepancyC * max(1, int(limit)))()
    check(lib().bfz_debug_interactions_traces(
        ctypes.c_void_p(pk.handle), chips, ptrs, hs, ws, k, kinds_mask(kinds), int(bool(on_device)),
        ctypes.byref(rep), recs, int(limit)))
    return _lookup_report(rep, recs, sorted(c for c, _, _ in traces))


def _debug_interactions_record(self, pk: BfProvingKey, stdin, kinds=None,
                               limit: int = 256) -> LookupReport:
    """debug_interactions_with_all_chips (lookup/debug.rs:125-196) of (pk's program, stdin) on the
    device: bfz_record_new, then bfz_record_debug_interactions aggregates the traces the GPU
    proves from."""
    init(self.device)
    buf, n = u8buf(bytes(stdin))
    rec = ctypes.c_void_p()
    cyc = ctypes.c_uint64()
    check(lib().bfz_record_new(ctypes.c_void_p(pk.handle), buf, n, ctypes.byref(rec),
                               ctypes.byref(cyc)))
    try:
        rep = _lib.LookupReportC()
        recs = (_lib.LookupDiscrepancyC * max(1, int(limit)))()
        check(lib().bfz_record_debug_interactions(ctypes.c_void_p(pk.handle), rec, kinds_mask(kinds),
                                                  ctypes.byref(rep), recs, int(limit)))
    finally:
        lib().bfz_record_free(rec)
    return _lookup_report(rep, recs)


CoreProver.debug_interactions = _debug_interactions_traces
ProverClient.debug_interactions = _debug_interactions_record


# ---- per-chip uni-STARK proofs: utils::{uni_stark_prove, uni_stark_verify}
# (crates/core/machine/src/utils/prove.rs:97-159)
UNI_STARK_CHIPS = (0, 2, 3, 6, 7)  # Cpu, AddSub, Jump, MemoryInstrs, IO


@dataclass
class UniStarkInfo:
    """What the chip's AIR alone determines: constraints, their maximal degree and
    log_quotient_degree = log2_ceil(degree - 1) (the proof has 2^log_quotient_degree chunks)."""
    chip: int
    num_constraints: int
    degree: int
    log_quotient_degree: int


def uni_stark_info(chip: int) -> UniStarkInfo:
    """bfz_uni_info (host only).  Raises for Program, Memory and Byte."""
    k, d, l = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(lib().bfz_uni_info(int(chip), ctypes.byref(k), ctypes.byref(d), ctypes.byref(l)))
    return UniStarkInfo(int(chip), k.value, d.value, l.value)


@dataclass
class UniCheckResult:
    """bfz_uni_check_result: the AIR-only row check of one chip.  Constraint indices count the
    chip's own AIR constraints alone (0 .. num_constraints - 1, the K of uni_stark_info)."""
    chip: int
    height: int
    num_constraints: int
    failing_rows: int
    first_row: int
    first_constraint: int
    first_fail_per_row: Optional[object] = None  # numpy int32[height], natural order, when asked for

    @property
    def ok(self) -> bool:
        return self.failing_rows == 0

    def __str__(self) -> str:
        name = CHIPS[self.chip] if self.chip >= 0 else "custom"  # -1: a constraint program
        if not self.failing_rows:
            return f"{name}: {self.height} row(s) ok"
        return (f"{name}: {self.failing_rows} failing row(s); first: row {self.first_row}, "
                f"AIR constraint {self.first_constraint} of {self.num_constraints}")


def _uni_check_result(c, per_row=None) -> UniCheckResult:
    return UniCheckResult(chip=c.chip, height=c.height, num_constraints=c.num_constraints,
                          failing_rows=c.failing_rows, first_row=c.first_row,
                          first_constraint=c.first_constraint, first_fail_per_row=per_row)


def uni_stark_check(chip: int, trace, on_device: bool = True, per_row: bool = False) -> UniCheckResult:
    """The row check p3_uni_stark::prove runs in a debug build (utils/prove.rs:97-112) over one
    trace (as uni_stark_prove takes it): every row against the chip's AIR constraints alone
    (bfz_uni_check).  A failing trace does not raise; the result names the first failing row and
    constraint.  on_device=False runs the same row function on the host (no GPU needed)."""
    import numpy as np
    if on_device:
        init()
    m = np.ascontiguousarray(trace, dtype=np.uint32)
    if m.ndim != 2:
        raise ValueError("uni_stark_check: the trace must be a (height, width) matrix")
    out = _lib.UniCheckC()
    rows = np.zeros(m.shape[0], dtype=np.int32) if per_row else None
    check(lib().bfz_uni_check(int(chip), m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                              m.shape[0], m.shape[1], int(bool(on_device)), ctypes.byref(out),
                              rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if per_row else None))
    return _uni_check_result(out, rows)


def _raise_if_failing(res: UniCheckResult) -> None:
    if res.failing_rows:
        raise BfzError(f"uni_stark_prove: the trace violates the AIR: {res}")


def uni_stark_prove(chip: int, trace, ch: Optional[Challenger] = None,
                    timings: Optional[_lib.Timings] = None, check: bool = False) -> bytes:
    """uni_stark_prove of one chip's AIR over one trace (a (height, width) uint32 array in
    Montgomery form, as generate_traces returns) on the device; the BFU1 proof bytes.  ch (a fresh
    DuplexChallenger when None) is advanced, as the reference's &mut challenger is.  check=True
    runs uni_stark_check first and raises BfzError naming the chip, row and constraint when a row
    fails (the reference's debug-build behaviour); by default an invalid trace still proves."""
    import numpy as np
    init()
    m = np.ascontiguousarray(trace, dtype=np.uint32)
    if m.ndim != 2:
        raise ValueError("uni_stark_prove: the trace must be a (height, width) matrix")
    if check:
        _raise_if_failing(uni_stark_check(chip, m, on_device=True))
    if ch is None:
        ch = Challenger()
    ptr = ctypes.POINTER(ctypes.c_uint8)()
    plen = ctypes.c_size_t()
    # (the parameter `check` hides the module's function here)
    _lib.check(lib().bfz_uni_prove(
        int(chip), m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), m.shape[0], m.shape[1],
        ctypes.byref(ch), ctypes.byref(ptr), ctypes.byref(plen),
        ctypes.byref(timings) if timings is not None else None))
    return take_bytes(ptr, plen.value)


def uni_stark_verify(chip: int, proof: bytes, ch: Optional[Challenger] = None) -> None:
    """uni_stark_verify on the host; raises BfzError with the verifier's reason on rejection (the
    reference returns Err).  ch (fresh when None) is advanced."""
    if ch is None:
        ch = Challenger()
    buf, n = u8buf(proof)
    out = _lib.VerifyOutcomeC()
    check(lib().bfz_uni_verify(int(chip), ctypes.byref(ch), buf, n, ctypes.byref(out)))
    if not out.ok:
        raise BfzError("uni-STARK verification failed: " + out.why.decode())


def uni_stark_verify_batch(chips, proofs, on_device: bool = True, chs=None) -> List[VerifyOutcome]:
    """uni_stark_verify of many proofs (bfz_uni_verify_batch): proofs[i] is a BFU1 proof of chip
    chips[i], checked against chs[i] (fresh challengers when None; each is advanced).  A rejected
    proof does not raise.  on_device=True runs all the proofs' query phases in one batched GPU
    pass; False is uni_stark_verify's host verifier proof by proof.  Both give the same outcomes."""
    raw = [bytes(p) for p in proofs]
    k = len(raw)
    if len(chips) != k or (chs is not None and len(chs) != k):
        raise ValueError("uni_stark_verify_batch: one chip (and one challenger) per proof")
    if on_device:
        init()
    bufs = [u8buf(x) for x in raw]
    arr = (ctypes.POINTER(ctypes.c_uint8) * max(k, 1))(
        *[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b, _ in bufs])
    lens = (ctypes.c_size_t * max(k, 1))(*[n for _, n in bufs])
    cids = (ctypes.c_int * max(k, 1))(*[int(c) for c in chips])
    carr = (Challenger * max(k, 1))()
    if chs is not None:
        for i, c in enumerate(chs):
            ctypes.memmove(ctypes.byref(carr[i]), ctypes.byref(c), ctypes.sizeof(Challenger))
    out = (_lib.VerifyOutcomeC * max(k, 1))()
    check(lib().bfz_uni_verify_batch(cids, carr, arr, lens, k, int(bool(on_device)), out))
    if chs is not None:
        for i, c in enumerate(chs):
            ctypes.memmove(ctypes.byref(c), ctypes.byref(carr[i]), ctypes.sizeof(Challenger))
    return [VerifyOutcome(ok=bool(out[i].ok), query=out[i].query, why=out[i].why.decode())
            for i in range(k)]


def _uni_stark_prove_record(self, pk: BfProvingKey, stdin, chips=UNI_STARK_CHIPS,
                            check: bool = False) -> Dict[int, bytes]:
    """uni_stark_prove of the chips of (pk's program, stdin) from the traces the device generates:
    one bfz_record_new, then bfz_record_uni_prove per chip, each from a fresh challenger.  Chips
    the record does not include are left out of the result.  check=True runs
    bfz_record_uni_check before each proof and raises as uni_stark_prove(check=True) does."""
    init(self.device)
    buf, n = u8buf(bytes(stdin))
    rec = ctypes.c_void_p()
    cyc = ctypes.c_uint64()
    _lib.check(lib().bfz_record_new(ctypes.c_void_p(pk.handle), buf, n, ctypes.byref(rec),
                                    ctypes.byref(cyc)))
    out = {}
    try:
        for chip in chips:
            if check:
                res = _lib.UniCheckC()
                rc = lib().bfz_record_uni_check(rec, int(chip), ctypes.byref(res))
                if rc == 1:
                    continue
                _lib.check(rc)
                _raise_if_failing(_uni_check_result(res))
            ch = Challenger()
            ptr = ctypes.POINTER(ctypes.c_uint8)()
            plen = ctypes.c_size_t()
            rc = lib().bfz_record_uni_prove(rec, int(chip), ctypes.byref(ch), ctypes.byref(ptr),
                                            ctypes.byref(plen), None)
            if rc == 1:
                continue
            _lib.check(rc)
            out[int(chip)] = take_bytes(ptr, plen.value)
    finally:
        lib().bfz_record_free(rec)
    return out


ProverClient.uni_stark_prove_record = _uni_stark_prove_record


# ---- caller-defined AIRs as constraint programs (bfz_air_*): uni_stark_prove / uni_stark_verify
# are generic over A: Air (crates/core/machine/src/utils/prove.rs:97-159)
AIR_CHIP = 0xFFFFFFFF  # BFZ_AIR_CHIP: the chip word of a proof made from a program
_AIR_MAGIC = 0x31414642  # "BFA1"
_KB_P = 0x7F000001
(_OP_CONST, _OP_LOCAL, _OP_NEXT, _OP_FIRST, _OP_LAST, _OP_TRANS, _OP_ADD, _OP_SUB, _OP_MUL,
 _OP_NEG) = range(10)


class AirExpr:
    """A node of an AirBuilder's program.  + - * and unary - append nodes; Python ints become
    constants."""
    __slots__ = ("builder", "node")

    def __init__(self, builder, node):
        self.builder, self.node = builder, node

    def _bin(self, op, other, swap=False):
        o = self.builder._lift(other)
        a, b = (o, self) if swap else (self, o)
        return self.builder._push(op, a.node, b.node)

    def __add__(self, o):
        return self._bin(_OP_ADD, o)

    def __radd__(self, o):
        return self._bin(_OP_ADD, o, swap=True)

    def __sub__(self, o):
        return self._bin(_OP_SUB, o)

    def __rsub__(self, o):
        return self._bin(_OP_SUB, o, swap=True)

    def __mul__(self, o):
        return self._bin(_OP_MUL, o)

    def __rmul__(self, o):
        return self._bin(_OP_MUL, o, swap=True)

    def __neg__(self):
        return self.builder._push(_OP_NEG, self.node, 0)


class AirBuilder:
    """Builds a BFA1 constraint program (include/bfz.h) the way an Air::eval is written:
    local(c) / next(c) are the row's columns, is_first_row / is_last_row / is_transition the
    selectors, const(v) a canonical field constant; assert_zero / assert_eq emit constraints in
    order; build() returns the bytes bfz_air_* take."""

    def __init__(self, width: int):
        self.width = int(width)
        self._nodes: List[tuple] = []
        self._constraints: List[int] = []
        self._leaves: Dict[tuple, AirExpr] = {}

    def _push(self, op, a, b) -> AirExpr:
        self._nodes.append((op, a, b))
        return AirExpr(self, len(self._nodes) - 1)

    def _leaf(self, op, a=0) -> AirExpr:
        if (op, a) not in self._leaves:
            self._leaves[(op, a)] = self._push(op, a, 0)
        return self._leaves[(op, a)]

    def _lift(self, v) -> AirExpr:
        if isinstance(v, AirExpr):
            if v.builder is not self:
                raise ValueError("AirBuilder: an expression of another builder")
            return v
        return self.const(v)

    def _col(self, c) -> int:
        c = int(c)
        if not 0 <= c < self.width:
            raise ValueError(f"AirBuilder: column {c} outside the width {self.width}")
        return c

    def local(self, c: int) -> AirExpr:
        return self._leaf(_OP_LOCAL, self._col(c))

    def next(self, c: int) -> AirExpr:
        return self._leaf(_OP_NEXT, self._col(c))

    @property
    def is_first_row(self) -> AirExpr:
        return self._leaf(_OP_FIRST)

    @property
    def is_last_row(self) -> AirExpr:
        return self._leaf(_OP_LAST)

    @property
    def is_transition(self) -> AirExpr:
        return self._leaf(_OP_TRANS)

    def const(self, v: int) -> AirExpr:
        return self._leaf(_OP_CONST, ((int(v) % _KB_P) << 32) % _KB_P)  # the Montgomery word

    def assert_zero(self, e) -> None:
        self._constraints.append(self._lift(e).node)

    def assert_eq(self, a, b) -> None:
        self.assert_zero(self._lift(a) - b)

    def build(self) -> bytes:
        import struct
        words = [_AIR_MAGIC, self.width, len(self._nodes), len(self._constraints)]
        for n in self._nodes:
            words.extend(n)
        words.extend(self._constraints)
        return struct.pack(f"<{len(words)}I", *words)


@dataclass
class AirInfo:
    """bfz_air_shape: a program's shape and the size of its compiled instruction list."""
    width: int
    num_nodes: int
    num_constraints: int
    degree: int
    log_quotient_degree: int
    instructions: int
    live_values: int


def air_export(chip: int) -> bytes:
    """bfz_air_export (host only): the BFA1 program of a built-in chip's AIR.  Raises for Program,
    Memory and Byte as uni_stark_info does."""
    ptr = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    check(lib().bfz_air_export(int(chip), ctypes.byref(ptr), ctypes.byref(n)))
    return take_bytes(ptr, n.value)


def air_info(prog: bytes) -> AirInfo:
    """bfz_air_info (host only): validates the program; raises BfzError naming the word offset."""
    buf, n = u8buf(prog)
    out = _lib.AirShapeC()
    check(lib().bfz_air_info(buf, n, ctypes.byref(out)))
    return AirInfo(out.width, out.num_nodes, out.num_constraints, out.degree,
                   out.log_quotient_degree, out.instructions, out.live_values)


def air_eval(prog: bytes, local, next, is_first, is_last, is_transition):
    """bfz_air_eval (host only): the K constraint values over extension-field rows.  local / next:
    (width, 4) Montgomery words, the selectors 4 words each; returns a (K, 4) uint32 array."""
    import numpy as np
    info = air_info(prog)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    rows = [np.ascontiguousarray(m, dtype=np.uint32) for m in (local, next)]
    sels = [np.ascontiguousarray(v, dtype=np.uint32) for v in (is_first, is_last, is_transition)]
    if any(m.shape != (info.width, 4) for m in rows) or any(v.shape != (4,) for v in sels):
        raise ValueError("air_eval: rows are (width, 4) and selectors (4,) Montgomery words")
    out = np.zeros((info.num_constraints, 4), dtype=np.uint32)
    buf, n = u8buf(prog)
    check(lib().bfz_air_eval(buf, n, *[a.ctypes.data_as(u32p) for a in rows + sels],
                             out.ctypes.data_as(u32p)))
    return out


def air_check(prog: bytes, trace, on_device: bool = True, per_row: bool = False) -> UniCheckResult:
    """uni_stark_check for a constraint program (bfz_air_check): chip = -1 in the result."""
    import numpy as np
    if on_device:
        init()
    m = np.ascontiguousarray(trace, dtype=np.uint32)
    if m.ndim != 2:
        raise ValueError("air_check: the trace must be a (height, width) matrix")
    out = _lib.UniCheckC()
    rows = np.zeros(m.shape[0], dtype=np.int32) if per_row else None
    buf, n = u8buf(prog)
    check(lib().bfz_air_check(buf, n, m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                              m.shape[0], m.shape[1], int(bool(on_device)), ctypes.byref(out),
                              rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if per_row else None))
    return _uni_check_result(out, rows)


def air_prove(prog: bytes, trace, ch: Optional[Challenger] = None, check: bool = False) -> bytes:
    """uni_stark_prove for a constraint program (bfz_air_prove): the BFU1 proof bytes, chip word
    AIR_CHIP.  ch (fresh when None) is advanced.  check=True runs air_check first and raises
    BfzError naming the row and constraint when a row fails; by default an invalid trace still
    proves.  The AIR is not bound into the transcript (as in p3_uni_stark): the verifier must be
    given the same program."""
    import numpy as np
    init()
    m = np.ascontiguousarray(trace, dtype=np.uint32)
    if m.ndim != 2:
        raise ValueError("air_prove: the trace must be a (height, width) matrix")
    if check:
        _raise_if_failing(air_check(prog, m, on_device=True))
    if ch is None:
        ch = Challenger()
    ptr = ctypes.POINTER(ctypes.c_uint8)()
    plen = ctypes.c_size_t()
    buf, n = u8buf(prog)
    # (the parameter `check` hides the module's function here)
    _lib.check(lib().bfz_air_prove(
        buf, n, m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), m.shape[0], m.shape[1],
        ctypes.byref(ch), ctypes.byref(ptr), ctypes.byref(plen), None))
    return take_bytes(ptr, plen.value)


def air_verify(prog: bytes, proof: bytes, ch: Optional[Challenger] = None) -> None:
    """uni_stark_verify for a constraint program (bfz_air_verify, host only); raises BfzError with
    the verifier's reason on rejection.  ch (fresh when None) is advanced."""
    if ch is None:
        ch = Challenger()
    pbuf, pn = u8buf(prog)
    buf, n = u8buf(proof)
    out = _lib.VerifyOutcomeC()
    check(lib().bfz_air_verify(pbuf, pn, ctypes.byref(ch), buf, n, ctypes.byref(out)))
    if not out.ok:
        raise BfzError("uni-STARK verification failed: " + out.why.decode())


def set_num_queries(q: int) -> None:
    """FRI_QUERIES override (crates/stark/src/kb31_poseidon2.rs:59-62); 0 = environment/84."""
    check(lib().bfz_set_num_queries(int(q)))


def set_pcs_variant(observe_openings: int) -> None:
    """Decision D1: 1 = opened values observed before FRI alpha (default),
    0 = alpha sampled first, -1 = environment BFZ_OBSERVE_OPENINGS."""
    check(lib().bfz_set_pcs_variant(int(observe_openings)))
