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


def _constraint_tables(k: int):
    """(counts uint64[K], first_rows int64[K], their ctypes pointers)"""
    import numpy as np
    counts, first = np.zeros(k, dtype=np.uint64), np.full(k, -1, dtype=np.int64)
    return (counts, first, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            first.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))


def uni_stark_check_constraints(chip: int, trace, on_device: bool = True):
    """uni_stark_check without stopping at a row's first failing constraint
    (bfz_uni_check_constraints): (summary, counts, first_rows).  The summary is uni_stark_check's;
    counts[k] is the number of rows that violate constraint k and first_rows[k] the smallest of
    them (-1: none), numpy uint64[K] / int64[K] with the K of uni_stark_info."""
    import numpy as np
    if on_device:
        init()
    m = np.ascontiguousarray(trace, dtype=np.uint32)
    if m.ndim != 2:
        raise ValueError("uni_stark_check_constraints: the trace must be a (height, width) matrix")
    out = _lib.UniCheckC()
    counts, first, pc, pf = _constraint_tables(uni_stark_info(chip).num_constraints)
    check(lib().bfz_uni_check_constraints(
        int(chip), m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), m.shape[0], m.shape[1],
        int(bool(on_device)), ctypes.byref(out), pc, pf))
    return _uni_check_result(out), counts, first


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


def _uni_stark_check_constraints_record(self, pk: BfProvingKey, stdin, chip: int):
    """uni_stark_check_constraints of one chip of (pk's program, stdin) on the trace the device
    generates (bfz_record_uni_check_constraints): (summary, counts, first_rows), or None when the
    record does not include the chip."""
    init(self.device)
    buf, n = u8buf(bytes(stdin))
    rec = ctypes.c_void_p()
    cyc = ctypes.c_uint64()
    counts, first, pc, pf = _constraint_tables(uni_stark_info(chip).num_constraints)
    _lib.check(lib().bfz_record_new(ctypes.c_void_p(pk.handle), buf, n, ctypes.byref(rec),
                                    ctypes.byref(cyc)))
    try:
        res = _lib.UniCheckC()
        rc = lib().bfz_record_uni_check_constraints(rec, int(chip), ctypes.byref(res), pc, pf)
        if rc == 1:
            return None
        _lib.check(rc)
        return _uni_check_result(res), counts, first
    finally:
        lib().bfz_record_free(rec)


ProverClient.uni_stark_check_constraints_record = _uni_stark_check_constraints_record


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


def air_check_constraints(prog: bytes, trace, on_device: bool = True):
    """uni_stark_check_constraints for a constraint program (bfz_air_check_constraints):
    (summary, counts, first_rows) with the program's K; chip = -1 in the summary."""
    import numpy as np
    if on_device:
        init()
    m = np.ascontiguousarray(trace, dtype=np.uint32)
    if m.ndim != 2:
        raise ValueError("air_check_constraints: the trace must be a (height, width) matrix")
    out = _lib.UniCheckC()
    counts, first, pc, pf = _constraint_tables(air_info(prog).num_constraints)
    buf, n = u8buf(prog)
    check(lib().bfz_air_check_constraints(
        buf, n, m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), m.shape[0], m.shape[1],
        int(bool(on_device)), ctypes.byref(out), pc, pf))
    return _uni_check_result(out), counts, first


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


# ---- LogUp of caller-defined chips as interaction programs (bfz_lookups_*): Chip::new derives the
# interactions of any AIR (crates/stark/src/chip.rs:65-90) and generate_permutation_trace runs
# over whatever it is handed (crates/stark/src/permutation.rs:75-148)
_LOOKUPS_MAGIC = 0x314C4642  # "BFL1"
LOOKUPS_MAX, LOOKUPS_MAX_VALUES, LOOKUPS_MAX_TERMS = 32, 7, 8


def _mont(v: int) -> int:
    return ((int(v) % _KB_P) << 32) % _KB_P


class LookupExpr:
    """An affine expression over a row, constant + sum weight * column (a VirtualPairCol):
    + and - with expressions and ints, * with ints.  Canonical integers throughout."""
    __slots__ = ("const", "terms")

    def __init__(self, const=0, terms=None):
        self.const, self.terms = int(const) % _KB_P, dict(terms or {})  # {(source, column): weight}

    @staticmethod
    def _lift(v) -> "LookupExpr":
        return v if isinstance(v, LookupExpr) else LookupExpr(v)

    def __add__(self, o):
        o = self._lift(o)
        terms = dict(self.terms)
        for k, w in o.terms.items():
            terms[k] = (terms.get(k, 0) + w) % _KB_P
        return LookupExpr(self.const + o.const, terms)

    __radd__ = __add__

    def __mul__(self, k):
        k = int(k)  # (an expression times an expression is not affine)
        return LookupExpr(self.const * k, {c: w * k % _KB_P for c, w in self.terms.items()})

    __rmul__ = __mul__

    def __neg__(self):
        return self * -1

    def __sub__(self, o):
        return self + -self._lift(o)

    def __rsub__(self, o):
        return self._lift(o) + -self

    def _words(self) -> list:
        terms = [(k, w) for k, w in self.terms.items() if w]
        if len(terms) > LOOKUPS_MAX_TERMS:
            raise ValueError(f"LookupBuilder: more than {LOOKUPS_MAX_TERMS} terms in one expression")
        out = [_mont(self.const), len(terms)]
        for (src, col), w in terms:
            out += [src, col, _mont(w)]
        return out


class LookupBuilder:
    """Builds a BFL1 interaction program (include/bfz.h) the way an Air::eval calls the lookup
    builder: main(c) / prep(c) are the row's columns, send / receive take the canonical argument
    index, the values and the multiplicity as affine expressions (or ints).  program() returns the
    bytes bfz_lookups_* take: the sends in emission order, then the receives."""

    def __init__(self, main_width: int, prep_width: int = 0):
        self.main_width, self.prep_width = int(main_width), int(prep_width)
        self._sends: List[list] = []
        self._receives: List[list] = []

    def _col(self, src: int, c: int, width: int) -> LookupExpr:
        c = int(c)
        if not 0 <= c < width:
            raise ValueError(f"LookupBuilder: column {c} outside the width {width}")
        return LookupExpr(0, {(src, c): 1})

    def main(self, c: int) -> LookupExpr:
        return self._col(0, c, self.main_width)

    def prep(self, c: int) -> LookupExpr:
        return self._col(1, c, self.prep_width)

    def _interaction(self, send: int, kind: int, values, mult) -> list:
        values = list(values)
        if len(values) > LOOKUPS_MAX_VALUES:
            raise ValueError(f"LookupBuilder: more than {LOOKUPS_MAX_VALUES} values")
        words = [int(kind), send, len(values)]
        for e in [mult] + values:
            words += LookupExpr._lift(e)._words()
        return words

    def send(self, kind: int, values, mult) -> None:
        self._sends.append(self._interaction(1, kind, values, mult))

    def receive(self, kind: int, values, mult) -> None:
        self._receives.append(self._interaction(0, kind, values, mult))

    def program(self) -> bytes:
        import struct
        chain = self._sends + self._receives
        words = [_LOOKUPS_MAGIC, self.main_width, self.prep_width, len(chain)]
        for it in chain:
            words += it
        return struct.pack(f"<{len(words)}I", *words)


@dataclass
class LookupsInfo:
    """bfz_lookups_shape: perm_width in EF columns, list_words of the compiled list."""
    main_width: int
    prep_width: int
    n_interactions: int
    sends: int
    receives: int
    perm_width: int
    list_words: int


@dataclass
class LookupsBalance:
    """bfz_lookups_balance: balanced iff total (the sum of the chips' cumulative sums) is zero."""
    balanced: bool
    total: List[int]
    cumsums: List[List[int]]


def lookups_export(chip: int) -> bytes:
    """bfz_lookups_export (host only): the BFL1 program of a built-in chip's interactions."""
    ptr = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    check(lib().bfz_lookups_export(int(chip), ctypes.byref(ptr), ctypes.byref(n)))
    return take_bytes(ptr, n.value)


def lookups_info(prog: bytes) -> LookupsInfo:
    """bfz_lookups_info (host only): validates the program; raises BfzError naming the word
    offset."""
    buf, n = u8buf(prog)
    out = _lib.LookupsShapeC()
    check(lib().bfz_lookups_info(buf, n, ctypes.byref(out)))
    return LookupsInfo(out.main_width, out.prep_width, out.n_interactions, out.sends, out.receives,
                       out.perm_width, out.list_words)


def _lookups_trace(m, what):
    import numpy as np
    if m is None:
        return None
    m = np.ascontiguousarray(m, dtype=np.uint32)
    if m.ndim != 2:
        raise ValueError(f"{what}: a trace must be a (height, width) matrix")
    return m


def _lookups_chip_args(info: LookupsInfo, main, prep, what):
    main, prep = _lookups_trace(main, what), _lookups_trace(prep, what)
    if main is None or main.shape[1] != info.main_width:
        raise ValueError(f"{what}: the main trace must have {info.main_width} columns")
    if info.prep_width and (prep is None or prep.shape != (main.shape[0], info.prep_width)):
        raise ValueError(f"{what}: the prep trace must be ({main.shape[0]}, {info.prep_width})")
    return main, prep if info.prep_width else None


def lookups_perm_trace(prog: bytes, main, prep, alpha, beta, on_device: bool = True):
    """bfz_lookups_perm_trace: generate_permutation_trace for an interaction program.  main / prep
    (None without preprocessed columns): (height, width) Montgomery words; alpha, beta: 4
    Montgomery words each.  Returns (perm, cumsum): the (height, 4 * perm_width) flattened
    permutation trace in natural row order and the 4 words of the cumulative sum.  A zero
    denominator is not detected."""
    import numpy as np
    if on_device:
        init()
    main, prep = _lookups_chip_args(lookups_info(prog), main, prep, "lookups_perm_trace")
    u32p = ctypes.POINTER(ctypes.c_uint32)
    out, w, cs = u32p(), ctypes.c_size_t(), (ctypes.c_uint32 * 4)()
    buf, n = u8buf(prog)
    check(lib().bfz_lookups_perm_trace(
        buf, n, main.ctypes.data_as(u32p), prep.ctypes.data_as(u32p) if prep is not None else None,
        main.shape[0], (ctypes.c_uint32 * 4)(*alpha), (ctypes.c_uint32 * 4)(*beta),
        int(bool(on_device)), ctypes.byref(out), ctypes.byref(w), cs))
    perm = np.ctypeslib.as_array(out, shape=(main.shape[0], w.value)).copy()
    lib().bfz_free(out)
    return perm, list(cs)


def lookups_balance(progs, mains, preps, alpha, beta, on_device: bool = True) -> LookupsBalance:
    """bfz_lookups_balance: the verifier's sum of cumulative sums == 0
    (crates/stark/src/verifier.rs:210-213) for caller-defined chips under the caller's challenges.
    progs, mains, preps: one entry per chip (a prep entry is None without preprocessed columns)."""
    if on_device:
        init()
    k = len(progs)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    chips = [_lookups_chip_args(lookups_info(p), m, pr, "lookups_balance")
             for p, m, pr in zip(progs, mains, preps)]
    bufs = [u8buf(p) for p in progs]
    u8p = ctypes.POINTER(ctypes.c_uint8)
    cprogs = (u8p * k)(*[ctypes.cast(b, u8p) for b, _ in bufs])
    clens = (ctypes.c_size_t * k)(*[n for _, n in bufs])
    cmains = (u32p * k)(*[m.ctypes.data_as(u32p) for m, _ in chips])
    cpreps = (u32p * k)(*[pr.ctypes.data_as(u32p) if pr is not None else u32p() for _, pr in chips])
    cheights = (ctypes.c_size_t * k)(*[m.shape[0] for m, _ in chips])
    cums, total, ok = (ctypes.c_uint32 * (4 * k))(), (ctypes.c_uint32 * 4)(), ctypes.c_int()
    check(lib().bfz_lookups_balance(cprogs, clens, cmains, cpreps, cheights, k,
                                    (ctypes.c_uint32 * 4)(*alpha), (ctypes.c_uint32 * 4)(*beta),
                                    int(bool(on_device)), cums, total, ctypes.byref(ok)))
    return LookupsBalance(bool(ok.value), list(total), [list(cums[4 * i:4 * i + 4]) for i in range(k)])


def _lookups_chips_c(progs, mains, preps, what):
    """The C arrays of a set of caller-defined chips (kept alive by the returned tuple)."""
    k = len(progs)
    u32p, u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
    chips = [_lookups_chip_args(lookups_info(p), m, pr, what) for p, m, pr in zip(progs, mains, preps)]
    bufs = [u8buf(p) for p in progs]
    return ((u8p * k)(*[ctypes.cast(b, u8p) for b, _ in bufs]),
            (ctypes.c_size_t * k)(*[n for _, n in bufs]),
            (u32p * k)(*[m.ctypes.data_as(u32p) for m, _ in chips]),
            (u32p * k)(*[pr.ctypes.data_as(u32p) if pr is not None else u32p() for _, pr in chips]),
            (ctypes.c_size_t * k)(*[m.shape[0] for m, _ in chips]), k, chips, bufs)


def _lookups_record(r, chip_net=(), chip_count=()) -> LookupDiscrepancy:
    return LookupDiscrepancy(
        kind=r.kind, values=[r.values[v] * _RINV % _P for v in range(r.nvals)], net=r.net,
        chip_net=list(chip_net), chip_count=list(chip_count), first_chip=r.first_chip,
        first_row=r.first_row, first_interaction=r.first_interaction)


def lookups_debug(progs, mains, preps, kinds=None, limit: int = 256,
                  on_device: bool = True) -> LookupReport:
    """bfz_lookups_debug: debug_interactions_with_all_chips (lookup/debug.rs:59-196) for
    caller-defined chips.  progs, mains, preps as lookups_balance takes them; kinds: canonical kind
    values (None = all).  A chip's index (first_chip, chip_net, chip_count, chip_distinct) is its
    position in progs; first_interaction is the index in the program's chain order."""
    if on_device:
        init()
    cprogs, clens, cmains, cpreps, cheights, k, *_keep = _lookups_chips_c(progs, mains, preps, "lookups_debug")
    kinds = [int(x) for x in kinds] if kinds is not None else []
    ckinds = (ctypes.c_uint32 * max(1, len(kinds)))(*kinds)
    cap = int(limit)
    distinct = (ctypes.c_uint64 * k)()
    rep = _lib.LookupsReportC(chip_distinct=distinct)
    recs = (_lib.LookupsDiscrepancyC * max(1, cap))()
    nets, counts = (ctypes.c_int32 * max(1, cap * k))(), (ctypes.c_uint32 * max(1, cap * k))()
    check(lib().bfz_lookups_debug(cprogs, clens, cmains, cpreps, cheights, k, ckinds, len(kinds),
                                  int(bool(on_device)), ctypes.byref(rep), recs, nets, counts, cap))
    ds = [_lookups_record(recs[i], nets[i * k:(i + 1) * k], counts[i * k:(i + 1) * k])
          for i in range(rep.n_written)]
    return LookupReport(
        balanced=bool(rep.balanced), total_net=rep.total_net, interactions=rep.interactions,
        distinct_keys=rep.distinct_keys, unbalanced_keys=rep.unbalanced_keys,
        chip_distinct=list(distinct), discrepancies=ds, rounds=rep.rounds,
        tag_collisions=rep.tag_collisions, table_bytes=rep.table_bytes)


@dataclass
class LookupsMultiplicities:
    """bfz_lookups_multiplicities: mult holds one Montgomery word per table row; unmatched counts
    the sent keys that no table row holds and first_unmatched is the smallest of them, with the
    senders' witness (None when every key is in the table)."""
    mult: "object"
    interactions: int
    distinct_keys: int
    unmatched: int
    first_unmatched: Optional[LookupDiscrepancy]


def lookups_multiplicities(table_prog, table_main, table_prep, interaction: int, progs, mains, preps,
                           on_device: bool = True) -> LookupsMultiplicities:
    """bfz_lookups_multiplicities: the multiplicity column of a table chip from the chips that send
    to it.  interaction: the table program's interaction whose key a row holds (normally its
    receive); its own multiplicity expression is not read.  Rows that hold the same key: the first
    gets everything."""
    import numpy as np
    if on_device:
        init()
    u32p = ctypes.POINTER(ctypes.c_uint32)
    tmain, tprep = _lookups_chip_args(lookups_info(table_prog), table_main, table_prep,
                                      "lookups_multiplicities")
    cprogs, clens, cmains, cpreps, cheights, k, *_keep = _lookups_chips_c(
        progs, mains, preps, "lookups_multiplicities")
    tbuf, tn = u8buf(table_prog)
    mult = np.zeros(tmain.shape[0], dtype=np.uint32)
    rep = _lib.LookupsMultReportC()
    check(lib().bfz_lookups_multiplicities(
        tbuf, tn, tmain.ctypes.data_as(u32p), tprep.ctypes.data_as(u32p) if tprep is not None else None,
        tmain.shape[0], int(interaction), cprogs, clens, cmains, cpreps, cheights, k,
        int(bool(on_device)), mult.ctypes.data_as(u32p), ctypes.byref(rep)))
    return LookupsMultiplicities(mult, rep.interactions, rep.distinct_keys, rep.unmatched,
                                 _lookups_record(rep.first) if rep.unmatched else None)


# ---- caller-defined chips of a machine: an AIR program paired with an interaction program
@dataclass
class ChipInfo:
    """bfz_chip_shape: perm_width in EF columns; num_constraints = air_constraints + batches + 3."""
    main_width: int
    prep_width: int
    perm_width: int
    n_interactions: int
    air_constraints: int
    num_constraints: int
    degree: int
    log_quotient_degree: int


def _chip_progs(air, lookups):
    a, an = u8buf(air) if air else (None, 0)
    lk, ln = u8buf(lookups) if lookups else (None, 0)
    return a, an, lk, ln


def chip_info(air: Optional[bytes], lookups: bytes) -> ChipInfo:
    """bfz_chip_info (host only): validates the pair (air = None: a lookup-only chip) and returns
    its shape; raises BfzError naming what is wrong."""
    a, an, lk, ln = _chip_progs(air, lookups)
    out = _lib.ChipShapeC()
    check(lib().bfz_chip_info(a, an, lk, ln, ctypes.byref(out)))
    return ChipInfo(out.main_width, out.prep_width, out.perm_width, out.n_interactions,
                    out.air_constraints, out.num_constraints, out.degree, out.log_quotient_degree)


def _chip_traces(info: ChipInfo, main, prep, perm, what):
    main, prep = _lookups_chip_args(info, main, prep, what)
    perm = _lookups_trace(perm, what)
    if perm is not None and perm.shape != (main.shape[0], 4 * info.perm_width):
        raise ValueError(f"{what}: the permutation trace must be "
                         f"({main.shape[0]}, {4 * info.perm_width})")
    return main, prep, perm


def chip_check(air: Optional[bytes], lookups: bytes, main, prep, perm, alpha, beta, cumsum,
               on_device: bool = True, per_row: bool = False) -> ChipCheckResult:
    """bfz_chip_check_rows: debug_constraints (crates/stark/src/debug.rs:24-105) of one
    caller-defined chip -- the AIR's constraints, one per LogUp batch, then the running sum's
    first-row, transition and last-row constraints.  Arguments as check_chip, perm as
    lookups_perm_trace returns it; the result's chip is -1."""
    import numpy as np
    if on_device:
        init()
    main, prep, perm = _chip_traces(chip_info(air, lookups), main, prep, perm, "chip_check")
    if perm is None:
        raise ValueError("chip_check: needs the permutation trace")
    u32p = ctypes.POINTER(ctypes.c_uint32)
    a, an, lk, ln = _chip_progs(air, lookups)
    out = _lib.ChipCheck()
    rows = np.zeros(main.shape[0], dtype=np.int32) if per_row else None
    check(lib().bfz_chip_check_rows(
        a, an, lk, ln, main.ctypes.data_as(u32p),
        prep.ctypes.data_as(u32p) if prep is not None else None, perm.ctypes.data_as(u32p),
        main.shape[0], (ctypes.c_uint32 * 4)(*alpha), (ctypes.c_uint32 * 4)(*beta),
        (ctypes.c_uint32 * 4)(*cumsum), int(bool(on_device)), ctypes.byref(out),
        rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if per_row else None))
    return _chip_result(out, rows)


def chip_quotient(air: Optional[bytes], lookups: Optional[bytes], main, prep, alpha, beta,
                  quot_alpha, perm=None, cumsum=None, chip: int = -1):
    """bfz_chip_quotient (device): the chip's machine quotient (quotient_values,
    crates/stark/src/quotient.rs:18-165) on 3 H_2n.  chip = -1 runs the two programs; chip >= 0
    (air = lookups = None) runs that built-in chip's compiled kernel.  perm = None: the
    permutation trace and cumulative sum are computed on the device; otherwise both are the
    caller's.  Returns (q, cumsum): q is (2 * height, 4) Montgomery words, row i = Q(3 w_2n^i).
    A pair of AIR degree above 3 (set_chip_max_degree) has D = 2^log_quotient_degree = 4 or 8
    chunks: q is then (D * height, 4), row i = Q(3 w_(D height)^i)."""
    import numpy as np
    init()
    if chip >= 0:
        info = ChipInfo(_MAIN_W[chip], _PREP_W[chip], _PERM_W[chip] // 4, 0, 0, 0, 3, 1)
    else:
        info = chip_info(air, lookups)
    main, prep, perm = _chip_traces(info, main, prep, perm, "chip_quotient")
    if perm is not None and cumsum is None:
        raise ValueError("chip_quotient: a caller's permutation trace needs its cumulative sum")
    u32p = ctypes.POINTER(ctypes.c_uint32)
    a, an, lk, ln = _chip_progs(air, lookups)
    cs = (ctypes.c_uint32 * 4)(*(cumsum if perm is not None else [0, 0, 0, 0]))
    out = u32p()
    check(lib().bfz_chip_quotient(
        int(chip), a, an, lk, ln, main.ctypes.data_as(u32p),
        prep.ctypes.data_as(u32p) if prep is not None else None,
        perm.ctypes.data_as(u32p) if perm is not None else None, main.shape[0],
        (ctypes.c_uint32 * 4)(*alpha), (ctypes.c_uint32 * 4)(*beta), cs,
        (ctypes.c_uint32 * 4)(*quot_alpha), ctypes.byref(out)))
    q = np.ctypeslib.as_array(out, shape=(main.shape[0] << info.log_quotient_degree, 4)).copy()
    lib().bfz_free(out)
    return q, list(cs)


def chip_quotient_time(chip: int, air: Optional[bytes], lookups: bytes, main, prep, alpha, beta,
                       quot_alpha, runs: int = 20):
    """bfz_chip_quotient_time (diagnostic): per-launch HIP-event milliseconds of
    k_quotient_chip_prog on the programs and of k_quotient<chip>, alternating, `runs` each."""
    init()
    main, prep, _ = _chip_traces(chip_info(air, lookups), main, prep, None, "chip_quotient_time")
    u32p = ctypes.POINTER(ctypes.c_uint32)
    a, an, lk, ln = _chip_progs(air, lookups)
    pm, cm = (ctypes.c_float * runs)(), (ctypes.c_float * runs)()
    check(lib().bfz_chip_quotient_time(
        int(chip), a, an, lk, ln, main.ctypes.data_as(u32p),
        prep.ctypes.data_as(u32p) if prep is not None else None, main.shape[0],
        (ctypes.c_uint32 * 4)(*alpha), (ctypes.c_uint32 * 4)(*beta),
        (ctypes.c_uint32 * 4)(*quot_alpha), int(runs), pm, cm))
    return list(pm), list(cm)


# ---- machines of caller-defined chips: StarkMachine::verify (crates/stark/src/machine.rs:258-284)
# and MachineProver::commit / open (crates/stark/src/prover.rs:209-236, 242-553) over chip programs
MACHINE_MAX_CHIPS = 32
_CHECK_ALPHA, _CHECK_BETA = [_mont(5), _mont(7), _mont(11), _mont(13)], [_mont(2), _mont(3), 0, _mont(1)]


@dataclass
class MachineCheckReport:
    """bfz_machine_check: what Machine.check found.  chips[j] / names[j] / counts[j] / first_rows[j]
    belong to the j-th trace given; a chip's `chip` is its index in the machine's creation order."""
    ok: bool
    alpha: List[int]
    beta: List[int]
    cumulative_sum: List[int]  # the sum of the chips' cumulative sums; ok needs it to be zero
    chips: List[ChipCheckResult]
    names: List[str]
    counts: Optional[list] = None      # per chip: numpy uint64[num_constraints] (profile=True)
    first_rows: Optional[list] = None  # per chip: numpy int64[num_constraints], -1 = never fails

    def __str__(self) -> str:
        lines = [f"machine check: {'ok' if self.ok else 'FAILED'}; cumulative sum "
                 f"{'zero' if not any(self.cumulative_sum) else 'NOT zero'}"]
        for n, c in zip(self.names, self.chips):
            lines.append(f"  {n:<12} {c.height:>8} rows, K = {c.num_constraints:<3} " + (
                "ok" if not c.failing_rows else
                f"FAILED: {c.failing_rows} failing row(s); first: row {c.first_row}, constraint "
                f"{c.first_constraint}"))
        return "\n".join(lines)


class Machine:
    """A machine whose chips are data (bfz_machine_*).  chips: [(name, air or None, lookups,
    prep or None)], name str or bytes, prep the chip's preprocessed trace ((height, prep_width)
    Montgomery words).  With every preprocessed trace given (or none needed) the traces are
    committed on the device and the machine proves and verifies; with prep_root (8 Montgomery
    words) and prep_heights ({name: height}) instead, it only verifies and touches no device.
    Up to 32 chips; a proof takes at most 8 chips of one height (the machine prover's own limit:
    the Merkle commit takes any number of matrices at any heights) and prove refuses more."""

    def __init__(self, chips, prep_root=None, prep_heights=None):
        import numpy as np
        self.names = [n.encode() if isinstance(n, str) else bytes(n) for n, *_ in chips]
        self.programs = [(air, lk) for _, air, lk, _ in chips]
        verifier_only = prep_root is not None or prep_heights is not None
        heights = {(k.encode() if isinstance(k, str) else bytes(k)): int(v)
                   for k, v in (prep_heights or {}).items()}
        k = len(chips)
        u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
        keep = []

        def bufs(items):
            ptrs, lens = (u8p * k)(), (ctypes.c_size_t * k)()
            for i, b in enumerate(items):
                if b:
                    buf, n = u8buf(b)
                    keep.append(buf)
                    ptrs[i], lens[i] = ctypes.cast(buf, u8p), n
            return ptrs, lens

        names, name_lens = bufs(self.names)
        airs, air_lens = bufs([a for a, _ in self.programs])
        lks, lk_lens = bufs([lk for _, lk in self.programs])
        preps, hs = (u32p * k)(), (ctypes.c_size_t * k)()
        self._check_preps = {}
        for i, (_, _, _, prep) in enumerate(chips):
            if prep is not None and not verifier_only:
                t = np.ascontiguousarray(prep, dtype=np.uint32)
                if t.ndim != 2:
                    raise ValueError("Machine: a preprocessed trace must be a (height, width) matrix")
                self._check_preps[i] = t
                preps[i], hs[i] = t.ctypes.data_as(u32p), t.shape[0]
            else:
                hs[i] = heights.get(self.names[i], 0)
        if not verifier_only:
            init()
        root = (ctypes.c_uint32 * 8)(*prep_root) if prep_root is not None else None
        self._h = ctypes.c_void_p()
        check(lib().bfz_machine_create(names, name_lens, airs, air_lens, lks, lk_lens, preps, hs, k,
                                       0 if verifier_only else 1, root, ctypes.byref(self._h)))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib().bfz_machine_free(h)

    @property
    def prep_root(self) -> List[int]:
        """The preprocessed commitment as 8 Montgomery words (zeros without preprocessed columns)."""
        out = (ctypes.c_uint32 * 8)()
        check(lib().bfz_machine_prep_root(self._h, out))
        return list(out)

    def observe(self, ch: Optional[Challenger] = None) -> Challenger:
        """StarkVerifyingKey::observe_into on ch (fresh when None); returns it."""
        if ch is None:
            ch = Challenger()
        check(lib().bfz_machine_observe(self._h, ctypes.byref(ch)))
        return ch

    def _traces_c(self, traces):
        import numpy as np
        u32p = ctypes.POINTER(ctypes.c_uint32)
        items = [(self.names.index(n.encode() if isinstance(n, str) else bytes(n)),
                  np.ascontiguousarray(t, dtype=np.uint32)) for n, t in traces.items()]
        if any(t.ndim != 2 or t.shape[1] != chip_info(*self.programs[i]).main_width for i, t in items):
            raise ValueError("Machine: a trace must be a (height, main_width) matrix of its chip")
        k = len(items)
        idx, ptrs, hs = (ctypes.c_int * k)(), (u32p * k)(), (ctypes.c_size_t * k)()
        for j, (i, t) in enumerate(items):
            idx[j], ptrs[j], hs[j] = i, t.ctypes.data_as(u32p), t.shape[0]
        return idx, ptrs, hs, k, items

    def prove(self, traces, ch: Challenger, check: bool = False) -> bytes:
        """bfz_machine_prove: traces = {name: (height, main_width) Montgomery words} of the included
        chips; ch (the state after observe) is advanced.  check=True runs chip_check on every chip
        first, under fixed LogUp challenges, and raises BfzError naming the chip, row and constraint
        of the first failing row; by default an invalid trace still proves."""
        idx, ptrs, hs, k, items = self._traces_c(traces)
        if check:
            preps = self._check_preps
            for i, t in items:
                air, lk = self.programs[i]
                prep = preps.get(i)
                perm, cs = lookups_perm_trace(lk, t, prep, _CHECK_ALPHA, _CHECK_BETA)
                res = chip_check(air, lk, t, prep, perm, _CHECK_ALPHA, _CHECK_BETA, cs)
                if res.failing_rows:
                    raise BfzError(f"Machine.prove: chip {self.names[i].decode(errors='replace')} "
                                   f"violates its constraints: row {res.first_row}, constraint "
                                   f"{res.first_constraint} ({res.failing_rows} failing rows)")
        ptr, plen = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
        _lib.check(lib().bfz_machine_prove(self._h, idx, ptrs, hs, k, ctypes.byref(ch),
                                           ctypes.byref(ptr), ctypes.byref(plen)))
        return take_bytes(ptr, plen.value)

    def check(self, traces, ch: Optional[Challenger] = None, on_device: bool = True,
              profile: bool = False) -> "MachineCheckReport":
        """bfz_machine_check: StarkMachine::debug_constraints (crates/stark/src/machine.rs:288-387)
        for this machine, the call to run before any proof.  traces as prove takes them; ch (None:
        observe()) gives alpha then beta and is advanced.  Every constraint of every row of every
        chip is evaluated and the chips' cumulative sums are added up: ok needs both every row to
        hold and a zero total.  on_device=True checks all chips in one launch per class of chips;
        False is a single-threaded host loop.  profile=True adds, per chip, counts[k] (the rows on
        which constraint k is not zero) and first_rows[k] (the smallest of them, or -1).  When the
        total is not zero, lookups_debug over the same chips names the keys that do not balance."""
        import numpy as np
        idx, ptrs, hs, k, items = self._traces_c(traces)
        if ch is None:
            ch = self.observe()
        ks = [chip_info(*self.programs[i]).num_constraints for i, _ in items]
        counts = np.zeros(sum(ks), dtype=np.uint64) if profile else None
        firsts = np.zeros(sum(ks), dtype=np.int64) if profile else None
        rep, per = _lib.MachineCheckReport(), (_lib.ChipCheck * max(k, 1))()
        _lib.check(lib().bfz_machine_check(
            self._h, idx, ptrs, hs, k, ctypes.byref(ch), int(bool(on_device)), ctypes.byref(rep), per,
            counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if profile else None,
            firsts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if profile else None))
        at = np.cumsum([0] + ks)
        return MachineCheckReport(
            ok=bool(rep.ok), alpha=list(rep.alpha), beta=list(rep.beta),
            cumulative_sum=list(rep.cumulative_sum), chips=[_chip_result(per[j]) for j in range(k)],
            names=[self.names[i].decode(errors="replace") for i, _ in items],
            counts=[counts[at[j]:at[j + 1]] for j in range(k)] if profile else None,
            first_rows=[firsts[at[j]:at[j + 1]] for j in range(k)] if profile else None)

    def verify(self, proof: bytes, ch: Challenger) -> VerifyOutcome:
        """bfz_machine_verify (host only): the outcome, with the verifier's reason; ch advanced."""
        buf, n = u8buf(proof)
        out = _lib.VerifyOutcomeC()
        check(lib().bfz_machine_verify(self._h, ctypes.byref(ch), buf, n, ctypes.byref(out)))
        return VerifyOutcome(ok=bool(out.ok), query=out.query, why=out.why.decode())

    def verify_batch(self, proofs, chs=None, on_device: bool = True) -> List[VerifyOutcome]:
        """bfz_machine_verify_batch: verify of many proofs of this machine, proofs[i] against chs[i]
        (the states after observe, each advanced; fresh ones through observe() when None).  A
        rejected proof does not raise.  on_device=True runs all the proofs' query phases in one
        batched GPU pass and needs a bound device (a verifier-only machine binds none itself:
        bfz.init first); False is verify proof by proof.  Both give the same outcomes."""
        raw = [bytes(p) for p in proofs]
        k = len(raw)
        if chs is not None and len(chs) != k:
            raise ValueError("Machine.verify_batch: one challenger per proof")
        given = chs if chs is not None else [self.observe() for _ in range(k)]
        bufs = [u8buf(x) for x in raw]
        arr = (ctypes.POINTER(ctypes.c_uint8) * max(k, 1))(
            *[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b, _ in bufs])
        lens = (ctypes.c_size_t * max(k, 1))(*[n for _, n in bufs])
        carr = (Challenger * max(k, 1))()
        for i, c in enumerate(given):
            ctypes.memmove(ctypes.byref(carr[i]), ctypes.byref(c), ctypes.sizeof(Challenger))
        out = (_lib.VerifyOutcomeC * max(k, 1))()
        check(lib().bfz_machine_verify_batch(self._h, carr, arr, lens, k, int(bool(on_device)), out))
        for i, c in enumerate(given):
            ctypes.memmove(ctypes.byref(c), ctypes.byref(carr[i]), ctypes.sizeof(Challenger))
        return [VerifyOutcome(ok=bool(out[i].ok), query=out[i].query, why=out[i].why.decode())
                for i in range(k)]

    def verify_time(self, proofs, runs: int = 20):
        """bfz_machine_verify_time (diagnostic): HIP-event milliseconds of the device pass's
        launches over the accepted proofs, {"clear_ro" | "reduce" | "fold" | "paths" | "inputs":
        [runs values]}."""
        raw = [bytes(p) for p in proofs]
        k = len(raw)
        bufs = [u8buf(x) for x in raw]
        arr = (ctypes.POINTER(ctypes.c_uint8) * k)(
            *[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b, _ in bufs])
        lens = (ctypes.c_size_t * k)(*[n for _, n in bufs])
        carr = (Challenger * k)()
        for i in range(k):
            ctypes.memmove(ctypes.byref(carr[i]), ctypes.byref(self.observe()), ctypes.sizeof(Challenger))
        ms = (ctypes.c_float * (5 * runs))()
        check(lib().bfz_machine_verify_time(self._h, carr, arr, lens, k, int(runs), ms))
        return {nm: [ms[5 * r + j] for r in range(runs)]
                for j, nm in enumerate(("clear_ro", "reduce", "fold", "paths", "inputs"))}

    def time(self, traces, runs: int = 20):
        """bfz_machine_time (diagnostic): per-launch HIP-event milliseconds, as
        {"perm": (segmented, loop), "quotient": (segmented, loop)}, `runs` each."""
        idx, ptrs, hs, k, _ = self._traces_c(traces)
        pm, qm = (ctypes.c_float * (2 * runs))(), (ctypes.c_float * (2 * runs))()
        check(lib().bfz_machine_time(self._h, idx, ptrs, hs, k, int(runs), pm, qm))
        return {"perm": (list(pm[:runs]), list(pm[runs:])),
                "quotient": (list(qm[:runs]), list(qm[runs:]))}


def set_num_queries(q: int) -> None:
    """FRI_QUERIES override (crates/stark/src/kb31_poseidon2.rs:59-62); 0 = environment/84."""
    check(lib().bfz_set_num_queries(int(q)))


def set_air_max_degree(degree: int) -> None:
    """The largest constraint degree air_info / air_check / air_prove / air_verify accept: 3..9,
    0 = the default (3).  Degrees 4 and 5 prove with 4 quotient chunks, 6 to 9 with 8.  Chip
    programs and machines keep a cap of their own (set_chip_max_degree)."""
    check(lib().bfz_set_air_max_degree(int(degree)))


def set_chip_max_degree(degree: int) -> None:
    """The largest AIR degree a chip program (chip_info, chip_quotient, Machine) may have: 3..9,
    0 = the default (3); independent of set_air_max_degree.  A chip of AIR degree 4 or 5 has log
    quotient degree 2 (4 quotient chunks), 6 to 9 has 3 (8 chunks), and takes heights up to
    2^(24 - log quotient degree).  A machine made under a raised cap proves and verifies only while
    the cap still admits its chips."""
    check(lib().bfz_set_chip_max_degree(int(degree)))


def set_pcs_variant(observe_openings: int) -> None:
    """Decision D1: 1 = opened values observed before FRI alpha (default),
    0 = alpha sampled first, -1 = environment BFZ_OBSERVE_OPENINGS."""
    check(lib().bfz_set_pcs_variant(int(observe_openings)))
