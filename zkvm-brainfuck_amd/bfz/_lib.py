"""ctypes binding of the C ABI declared in include/bfz.h (the drop-in boundary).

The shared library is built in-tree (zkvm-brainfuck_amd/libbfz.so) by
`make -C zkvm-brainfuck_amd` or __graft_entry__.build().  There is no fallback: if the
library is missing, importing anything that proves raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import (POINTER, byref, c_char_p, c_double, c_int, c_int32, c_int64, c_size_t, c_uint, c_uint8,
                    c_uint32, c_uint64, c_void_p)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(HERE), "libbfz.so")


class BfzError(RuntimeError):
    """A negative status returned by the C ABI (message from bfz_last_error)."""


class Timings(ctypes.Structure):
    _fields_ = [
        ("trace_ms", c_double), ("main_commit_ms", c_double), ("perm_ms", c_double),
        ("quotient_ms", c_double), ("open_ms", c_double), ("fri_ms", c_double),
        ("total_ms", c_double), ("lde_ms", c_double), ("lde_bytes", c_double),
        ("lde_calls", c_int), ("ntt_kernel_ms", c_double), ("ntt_kernel_bytes", c_double),
        ("ntt_kernel_launches", c_int), ("p2_kernel_ms", c_double), ("p2_perms", c_double),
        ("p2_launches", c_int), ("lde_elem_stages", c_double),
        ("open_kernel_ms", c_double), ("open_kernel_bytes", c_double), ("open_kernel_launches", c_int),
        ("reduce_kernel_ms", c_double), ("reduce_kernel_bytes", c_double),
        ("reduce_kernel_launches", c_int),
        ("perm_rows_ms", c_double), ("perm_idft_ms", c_double), ("perm_dft_ms", c_double),
        ("perm_hash_ms", c_double),
        ("main_idft_ms", c_double), ("main_dft_ms", c_double), ("main_hash_ms", c_double),
        ("main_cells", c_double), ("perm_cells", c_double),
    ]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class BatchStats(ctypes.Structure):
    _fields_ = [("wall_ms", c_double), ("exec_ms", c_double), ("upload_ms", c_double),
                ("prove_ms", c_double), ("exec_threads", c_int)]


class Challenger(ctypes.Structure):
    """bfz_challenger: p3 DuplexChallenger state, Montgomery words."""
    _fields_ = [("sponge_state", c_uint32 * 16), ("input_buffer", c_uint32 * 8),
                ("n_input", c_uint32), ("output_buffer", c_uint32 * 8), ("n_output", c_uint32)]


NUM_CHIPS, NUM_KINDS = 8, 8  # BFZ_NUM_CHIPS, BFZ_NUM_KINDS


class ChipCheck(ctypes.Structure):
    """bfz_chip_check: the row check of one chip (first failing row and constraint index)."""
    _fields_ = [("chip", c_int32), ("num_constraints", c_int32), ("height", c_uint64),
                ("failing_rows", c_uint64), ("first_row", c_int64), ("first_constraint", c_int32),
                ("num_batches", c_int32), ("cumulative_sum", c_uint32 * 4)]


class DebugReportC(ctypes.Structure):
    """bfz_debug_report: StarkMachine::debug_constraints' outcome as plain data."""
    _fields_ = [("ok", c_int32), ("n_chips", c_int32), ("balance_valid", c_int32), ("_pad", c_int32),
                ("alpha", c_uint32 * 4), ("beta", c_uint32 * 4), ("cumulative_sum", c_uint32 * 4),
                ("chips", ChipCheck * NUM_CHIPS),
                ("kind_sum", ((c_uint32 * 4) * NUM_CHIPS) * NUM_KINDS),
                ("kind_net", (c_int32 * NUM_CHIPS) * NUM_KINDS),
                ("kind_count", (c_uint32 * NUM_CHIPS) * NUM_KINDS)]


LOOKUP_MAX_VALUES = 7  # BFZ_LOOKUP_MAX_VALUES


class LookupDiscrepancyC(ctypes.Structure):
    """bfz_lookup_discrepancy: one lookup key whose sends and receives differ."""
    _fields_ = [("kind", c_int32), ("nvals", c_int32), ("values", c_uint32 * LOOKUP_MAX_VALUES),
                ("net", c_int32), ("chip_net", c_int32 * NUM_CHIPS),
                ("chip_count", c_uint32 * NUM_CHIPS), ("first_chip", c_int32),
                ("first_interaction", c_int32), ("first_row", c_int64)]


class LookupReportC(ctypes.Structure):
    """bfz_lookup_report: debug_interactions_with_all_chips' outcome as plain data."""
    _fields_ = [("balanced", c_int32), ("total_net", c_int32), ("interactions", c_uint64),
                ("distinct_keys", c_uint64), ("unbalanced_keys", c_uint64),
                ("chip_distinct", c_uint64 * NUM_CHIPS), ("n_written", c_uint32),
                ("rounds", c_uint32), ("tag_collisions", c_uint32), ("table_bytes", c_uint64)]


class UniCheckC(ctypes.Structure):
    """bfz_uni_check_result: the AIR-only row check of one chip."""
    _fields_ = [("chip", c_int32), ("num_constraints", c_int32), ("height", c_uint64),
                ("failing_rows", c_uint64), ("first_row", c_int64), ("first_constraint", c_int32),
                ("_pad", c_int32)]


class AirShapeC(ctypes.Structure):
    """bfz_air_shape: the shape of a constraint program and the size of its compiled list."""
    _fields_ = [("width", c_int32), ("num_nodes", c_int32), ("num_constraints", c_int32),
                ("degree", c_int32), ("log_quotient_degree", c_int32), ("instructions", c_int32),
                ("live_values", c_int32), ("_pad", c_int32)]


class VerifyOutcomeC(ctypes.Structure):
    """bfz_verify_outcome: one proof's verdict from bfz_verify_batch."""
    _fields_ = [("ok", c_int32), ("query", c_int32), ("why", ctypes.c_char * 120)]


class Events(ctypes.Structure):
    """bfz_events: the reference ExecutionRecord's event arrays (pointers to bfz_*_event arrays,
    see bfz/events.py for their numpy layouts)."""
    _fields_ = [("cpu", c_void_p), ("n_cpu", c_size_t), ("add", c_void_p), ("n_add", c_size_t),
                ("sub", c_void_p), ("n_sub", c_size_t), ("jump", c_void_p), ("n_jump", c_size_t),
                ("io", c_void_p), ("n_io", c_size_t), ("memory_instr", c_void_p),
                ("n_memory_instr", c_size_t), ("memory", c_void_p), ("n_memory", c_size_t)]


# collective callbacks of bfz_record_prove_sharded (bfz_allgather_fn / bfz_allreduce_u32_fn)
ALLGATHER_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_size_t, c_void_p)
ALLREDUCE_FN = ctypes.CFUNCTYPE(c_int, c_void_p, POINTER(c_uint32), c_size_t)
# bfz_alltoall_fn of bfz_commit_fri_sharded (the caller owns the device exchange buffers)
ALLTOALL_FN = ctypes.CFUNCTYPE(c_int, c_void_p)

# (name, restype, argtypes) for every symbol declared in include/bfz.h
SIGNATURES = [
    ("bfz_init", c_int, [c_int]),
    ("bfz_last_error", c_char_p, []),
    ("bfz_build_id", c_char_p, []),
    ("bfz_device_name", c_int, [c_char_p, c_size_t]),
    ("bfz_free", None, [c_void_p]),
    ("bfz_host_alloc", c_int, [c_size_t, ctypes.POINTER(c_void_p)]),
    ("bfz_host_free", None, [c_void_p]),
    ("bfz_synchronize", c_int, []),
    ("bfz_selftest", c_int, [c_char_p]),
    ("bfz_execute", c_int, [c_char_p, POINTER(c_uint8), c_size_t, POINTER(c_uint8), c_size_t,
                            POINTER(c_size_t), POINTER(c_uint64)]),
    ("bfz_trace", c_int, [c_char_p, POINTER(c_uint8), c_size_t, c_int, c_int,
                          POINTER(POINTER(c_uint32)), POINTER(c_size_t), POINTER(c_size_t)]),
    ("bfz_execute_events", c_int, [c_char_p, POINTER(c_uint8), c_size_t, c_int,
                                   POINTER(POINTER(c_uint8)), POINTER(c_size_t)]),
    ("bfz_perm_trace", c_int, [c_int, POINTER(c_uint32), POINTER(c_uint32), c_size_t,
                               POINTER(c_uint32), POINTER(c_uint32), POINTER(POINTER(c_uint32)),
                               POINTER(c_size_t), POINTER(c_uint32)]),
    ("bfz_check_chip", c_int, [c_int, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32),
                               c_size_t, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32),
                               c_int, POINTER(ChipCheck), POINTER(c_int32)]),
    ("bfz_record_debug_constraints", c_int, [c_void_p, c_void_p, POINTER(Challenger), c_uint,
                                             POINTER(DebugReportC)]),
    ("bfz_debug_constraints_traces", c_int, [c_void_p, POINTER(c_int), POINTER(POINTER(c_uint32)),
                                             POINTER(c_size_t), POINTER(c_size_t), c_size_t,
                                             POINTER(Challenger), c_uint, POINTER(DebugReportC)]),
    ("bfz_record_debug_interactions", c_int, [c_void_p, c_void_p, c_uint, POINTER(LookupReportC),
                                              POINTER(LookupDiscrepancyC), c_size_t]),
    ("bfz_debug_interactions_traces", c_int, [c_void_p, POINTER(c_int), POINTER(POINTER(c_uint32)),
                                              POINTER(c_size_t), POINTER(c_size_t), c_size_t,
                                              c_uint, c_int, POINTER(LookupReportC),
                                              POINTER(LookupDiscrepancyC), c_size_t]),
    ("bfz_setup_host", c_int, [c_char_p, POINTER(c_void_p)]),
    ("bfz_trace_device", c_int, [c_char_p, POINTER(c_uint8), c_size_t, c_int,
                                 POINTER(POINTER(c_uint32)), POINTER(c_size_t), POINTER(c_size_t)]),
    ("bfz_setup", c_int, [c_char_p, POINTER(c_void_p), POINTER(c_uint32)]),
    ("bfz_pk_free", None, [c_void_p]),
    ("bfz_pk_from_host", c_int, [POINTER(c_int), POINTER(POINTER(c_uint32)), POINTER(c_size_t),
                                 POINTER(c_size_t), c_size_t, POINTER(c_uint32), POINTER(c_void_p)]),
    ("bfz_pk_commit", c_int, [c_void_p, POINTER(c_uint32)]),
    ("bfz_main_commit", c_int, [c_void_p, POINTER(c_int), POINTER(POINTER(c_uint32)),
                                POINTER(c_size_t), POINTER(c_size_t), c_size_t,
                                POINTER(c_void_p), POINTER(c_uint32)]),
    ("bfz_record_main_commit", c_int, [c_void_p, c_void_p, POINTER(c_void_p), POINTER(c_uint32)]),
    ("bfz_challenger_observe_pk", c_int, [c_void_p, POINTER(Challenger)]),
    ("bfz_open", c_int, [c_void_p, c_void_p, POINTER(Challenger), POINTER(POINTER(c_uint8)),
                         POINTER(c_size_t)]),
    ("bfz_main_data_free", None, [c_void_p]),
    ("bfz_prove", c_int, [c_void_p, POINTER(c_uint8), c_size_t, POINTER(POINTER(c_uint8)),
                          POINTER(c_size_t)]),
    ("bfz_prove_traces", c_int, [c_void_p, POINTER(c_int), POINTER(POINTER(c_uint32)),
                                 POINTER(c_size_t), POINTER(c_size_t), c_size_t,
                                 POINTER(POINTER(c_uint8)), POINTER(c_size_t)]),
    ("bfz_prove_batch", c_int, [c_void_p, POINTER(POINTER(c_uint8)), POINTER(c_size_t), c_size_t,
                                c_int, POINTER(POINTER(c_uint8)), POINTER(c_size_t),
                                POINTER(BatchStats)]),
    ("bfz_verify", c_int, [c_char_p, POINTER(c_uint32), POINTER(c_uint8), c_size_t]),
    ("bfz_verify_batch", c_int, [c_char_p, POINTER(c_uint32), POINTER(POINTER(c_uint8)),
                                 POINTER(c_size_t), c_size_t, c_int, POINTER(VerifyOutcomeC)]),
    ("bfz_record_new", c_int, [c_void_p, POINTER(c_uint8), c_size_t, POINTER(c_void_p),
                               POINTER(c_uint64)]),
    ("bfz_record_prove", c_int, [c_void_p, c_void_p, POINTER(POINTER(c_uint8)), POINTER(c_size_t),
                                 POINTER(Timings)]),
    ("bfz_record_free", None, [c_void_p]),
    ("bfz_record_from_events", c_int, [c_void_p, POINTER(Events), POINTER(c_void_p)]),
    ("bfz_record_from_cycles", c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t,
                                       POINTER(c_void_p)]),
    ("bfz_cycles_begin", c_int, [c_void_p, c_size_t, POINTER(c_void_p)]),
    ("bfz_cycles_push", c_int, [c_void_p, c_size_t, c_void_p, c_size_t]),
    ("bfz_cycles_finish", c_int, [c_void_p, c_void_p, c_size_t, POINTER(c_void_p)]),
    ("bfz_cycles_abort", None, [c_void_p]),
    ("bfz_record_prove_repeat", c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(POINTER(c_uint8)),
                                        POINTER(c_size_t), POINTER(ctypes.c_double)]),
    ("bfz_shard_solo_exchanges", c_int, [POINTER(c_int), POINTER(ctypes.c_uint64), c_size_t,
                                         POINTER(c_size_t)]),
    ("bfz_shard_solo_overlaps", c_int, [POINTER(ctypes.c_double), c_size_t, POINTER(c_size_t)]),
    ("bfz_device_pool_bytes", c_int, [c_int, POINTER(ctypes.c_uint64)]),
    ("bfz_record_prove_sharded", c_int, [c_void_p, c_void_p, c_int, c_int, ALLGATHER_FN,
                                         ALLREDUCE_FN, c_void_p, POINTER(POINTER(c_uint8)),
                                         POINTER(c_size_t), POINTER(Timings)]),
    ("bfz_record_prove_shard_solo", c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(Timings)]),
    ("bfz_commit_fri_sharded", c_int, [c_void_p, c_int, c_size_t, c_int, c_int, c_void_p, c_void_p,
                                       ALLTOALL_FN, ALLGATHER_FN, c_void_p, POINTER(c_uint32),
                                       c_size_t, POINTER(c_size_t)]),
    ("bfz_uni_info", c_int, [c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    ("bfz_uni_prove", c_int, [c_int, POINTER(c_uint32), c_size_t, c_size_t, POINTER(Challenger),
                              POINTER(POINTER(c_uint8)), POINTER(c_size_t), POINTER(Timings)]),
    ("bfz_uni_verify", c_int, [c_int, POINTER(Challenger), POINTER(c_uint8), c_size_t,
                               POINTER(VerifyOutcomeC)]),
    ("bfz_uni_check", c_int, [c_int, POINTER(c_uint32), c_size_t, c_size_t, c_int,
                              POINTER(UniCheckC), POINTER(c_int32)]),
    ("bfz_record_uni_check", c_int, [c_void_p, c_int, POINTER(UniCheckC)]),
    ("bfz_record_uni_prove", c_int, [c_void_p, c_int, POINTER(Challenger), POINTER(POINTER(c_uint8)),
                                     POINTER(c_size_t), POINTER(Timings)]),
    ("bfz_uni_verify_batch", c_int, [POINTER(c_int), POINTER(Challenger), POINTER(POINTER(c_uint8)),
                                     POINTER(c_size_t), c_size_t, c_int, POINTER(VerifyOutcomeC)]),
    ("bfz_air_export", c_int, [c_int, POINTER(POINTER(c_uint8)), POINTER(c_size_t)]),
    ("bfz_air_info", c_int, [POINTER(c_uint8), c_size_t, POINTER(AirShapeC)]),
    ("bfz_air_eval", c_int, [POINTER(c_uint8), c_size_t, POINTER(c_uint32), POINTER(c_uint32),
                             POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32),
                             POINTER(c_uint32)]),
    ("bfz_air_check", c_int, [POINTER(c_uint8), c_size_t, POINTER(c_uint32), c_size_t, c_size_t,
                              c_int, POINTER(UniCheckC), POINTER(c_int32)]),
    ("bfz_air_prove", c_int, [POINTER(c_uint8), c_size_t, POINTER(c_uint32), c_size_t, c_size_t,
                              POINTER(Challenger), POINTER(POINTER(c_uint8)), POINTER(c_size_t),
                              POINTER(Timings)]),
    ("bfz_air_verify", c_int, [POINTER(c_uint8), c_size_t, POINTER(Challenger), POINTER(c_uint8),
                               c_size_t, POINTER(VerifyOutcomeC)]),
    ("bfz_set_num_queries", c_int, [c_int]),
    ("bfz_set_pcs_variant", c_int, [c_int]),
    ("bfz_set_fault_injection", c_int, [c_int]),
    ("bfz_proof_to_bincode", c_int, [POINTER(c_uint8), c_size_t, c_int, POINTER(POINTER(c_uint8)),
                                     POINTER(c_size_t)]),
    ("bfz_proof_from_bincode", c_int, [POINTER(c_uint8), c_size_t, c_int,
                                       POINTER(POINTER(c_uint8)), POINTER(c_size_t)]),
    ("bfz_verify_bincode", c_int, [c_char_p, POINTER(c_uint32), POINTER(c_uint8), c_size_t, c_int]),
    ("bfz_coset_lde", c_int, [POINTER(c_uint32), c_size_t, c_size_t, c_uint32, POINTER(c_uint32)]),
    ("bfz_coset_lde_ex", c_int, [POINTER(c_uint32), c_size_t, c_size_t, c_size_t, c_int, c_uint32,
                                 c_int, c_int, POINTER(c_uint32)]),
    ("bfz_lde_shard", c_int, [POINTER(c_uint32), c_size_t, c_size_t, c_uint32, c_int, c_int, c_int,
                              POINTER(c_int), c_size_t, c_size_t, c_size_t, c_int,
                              POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32),
                              POINTER(c_int)]),
    ("bfz_ntt_last_paths", c_int, [POINTER(c_uint32)]),
    ("bfz_commit", c_int, [POINTER(POINTER(c_uint32)), POINTER(c_size_t), POINTER(c_size_t),
                           c_size_t, POINTER(c_uint32)]),
    ("bfz_poseidon2_permute", c_int, [POINTER(c_uint32), c_size_t]),
    ("bfz_poseidon2_permute_small", c_int, [POINTER(c_uint32), c_size_t]),
]

_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BfzError(f"{LIB_PATH} not built: run `make -C zkvm-brainfuck_amd` "
                           "(or __graft_entry__.build())")
        # One HIP runtime per process: PyTorch ships its own libamdhip64, and a process that
        # loads ROCm's copy first (through libbfz) cannot initialise torch.cuda afterwards.
        # Importing torch first makes libbfz bind to the runtime torch already loaded.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, res, args in SIGNATURES:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        built = L.bfz_build_id().decode()
        from . import srchash
        want = srchash.source_hash()
        # BFZ_AB_VARIANT=1: scripts/ab_bench.sh times builds of other source revisions in place
        if built != want and os.environ.get("BFZ_AB_VARIANT") != "1":
            raise BfzError(f"{LIB_PATH} was built from other sources (build id {built}, sources "
                           f"{want}): rebuild with `make -C zkvm-brainfuck_amd`")
        _lib = L
    return _lib


def check(status: int) -> None:
    if status != 0:
        msg = lib().bfz_last_error()
        raise BfzError(f"bfz status {status}: {msg.decode() if msg else ''}")


def u8buf(data: bytes):
    data = bytes(data)
    return (c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0"), len(data)


_initialized = None


def init(device: int = 0) -> None:
    global _initialized
    if _initialized != device:
        check(lib().bfz_init(device))
        _initialized = device


def take_bytes(ptr, n: int) -> bytes:
    try:
        return ctypes.string_at(ptr, n)
    finally:
        lib().bfz_free(ptr)


__all__ = ["lib", "check", "init", "u8buf", "take_bytes", "BfzError", "Timings", "Events", "LIB_PATH",
           "ChipCheck", "DebugReportC", "VerifyOutcomeC", "UniCheckC", "LookupDiscrepancyC", "LookupReportC",
           "SIGNATURES", "byref"]
