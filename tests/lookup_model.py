"""An independent model of the reference's per-key lookup debugger
(crates/stark/src/lookup/debug.rs:59-196) for tests/test_debug_interactions*.py.

The 31 interactions of the 8 chips are written here from the reference's AIR files, by COLUMN
NAME over the column structs (the indices follow from the #[repr(C)] field order), in the chain
order debug.rs:80 numbers them in: a chip's sends in emission order, then its receives.
debug_interactions() aggregates canonical numpy traces in a Python dict and returns the whole
report; nothing here comes from the library under test."""
import numpy as np

P = 0x7F000001
MEMORY, PROGRAM, ALU, JUMP, MEMINSTR, IO, BYTE = 1, 2, 3, 4, 5, 6, 7  # lookup/lookup.rs:17-42
KIND_NAMES = (None, "Memory", "Program", "Alu", "Jump", "MemInstr", "IO", "Byte")
CHIP_NAMES = ("Cpu", "Program", "AddSub", "Jump", "Memory", "Byte", "MemoryInstrs", "IO")
U8_RANGE, U16_RANGE = 0, 1                      # ByteOpcode (executor/src/opcode.rs:39-41)
LOOP_START, LOOP_END, ADD, SUB, FORWARD, BACKWARD, INPUT, OUTPUT = range(8)  # opcode.rs:14-28

_ACCESS = ["prev_value", "value", "prev_clk", "diff_16bit_limb", "diff_8bit_limb"]
_RANGE_CHECKER = 14  # KoalaBearWordRangeChecker: 8 bits of the top byte + 6 running products


def _word(name):
    return [f"{name}[{i}]" for i in range(4)]


# column structs, flattened in field order
COLS = {
    # CpuCols (cpu/cols.rs:29-71), MemoryReadWriteCols / MemoryWriteCols / MemoryAccessCols
    # (memory/consistency/cols.rs:13-45), InstructionCols (cpu/cols.rs:18-24)
    0: ["clk_16bit_limb", "clk_8bit_limb", "pc", "next_pc", "mp", "next_mp", "mv", "next_mv",
        "opcode"] + _word("op_a") + [f"mv_access.{f}" for f in _ACCESS]
       + [f"next_mv_access.{f}" for f in _ACCESS]
       + ["mv_accessed", "next_mv_accessed", "is_mv_immutable", "is_alu", "is_jump", "is_io",
          "is_memory_instr", "is_real"],
    1: ["multiplicity"],                                           # program/mod.rs:39-41
    # AddSubCols (alu/mod.rs:28-47) with AddOperation (operations/add.rs:12-18)
    2: ["pc", "add_operation.value", "add_operation.carry", "operand_1", "operand_2", "is_add",
        "is_sub"],
    # JumpCols (jump/cols.rs:12-31); IsZeroOperation is (inverse, result)
    3: _word("pc") + [f"pc_rc[{i}]" for i in range(_RANGE_CHECKER)] + _word("next_pc")
       + [f"next_pc_rc[{i}]" for i in range(_RANGE_CHECKER)] + _word("dst")
       + ["mv", "is_mv_zero.inverse", "is_mv_zero.result", "is_loop_start", "is_loop_end"],
    # MemCols: two SingleMemoryLocal per row (memory/memory.rs:24-48)
    4: [f"e{k}.{f}" for k in range(2)
        for f in ("addr", "initial_clk", "final_clk", "initial_value", "final_value", "is_real")],
    5: ["mult_u8", "mult_u16"],                                    # bytes/cols.rs:27-30
    # MemoryInstructionsCols (memory/instructions/cols.rs:13-35)
    6: ["pc", "clk"] + _word("mp") + [f"mp_rc[{i}]" for i in range(_RANGE_CHECKER)]
       + _word("next_mp") + [f"next_mp_rc[{i}]" for i in range(_RANGE_CHECKER)]
       + ["is_step_forward", "is_step_backward", "is_real"],
    7: ["pc", "mp", "mv", "is_input", "is_output"],                # io/mod.rs:23-35
}
PREP_COLS = {
    1: ["pc", "opcode"] + _word("op_a"),                           # program/mod.rs:31-34
    5: ["value_u8", "value_u16"],                                  # bytes/cols.rs:15-21
}
WIDTHS = {c: len(v) for c, v in COLS.items()}
assert [WIDTHS[c] for c in range(8)] == [31, 1, 7, 45, 12, 2, 41, 5]


class Row:
    """Named columns of a trace (main `m`, preprocessed `p`) as uint64 vectors."""

    def __init__(self, chip, main, prep):
        self.n = main.shape[0]
        self.m = {name: main[:, i].astype(np.uint64) for i, name in enumerate(COLS[chip])}
        self.p = {} if prep is None else {
            name: prep[:, i].astype(np.uint64) for i, name in enumerate(PREP_COLS[chip])}

    def const(self, v):
        return np.full(self.n, v % P, dtype=np.uint64)

    def word(self, name):  # Word::reduce (crates/stark/src/word.rs:66-70)
        return sum(self.m[f"{name}[{i}]"] * np.uint64(1 << (8 * i)) for i in range(4)) % np.uint64(P)


def cpu(r):
    """cpu/air.rs:28-62 in emission order: send_program (:38), eval_instruction (:66-92),
    eval_registers (:159-185; each eval_memory_access is air/memory.rs:17-50: the two range-check
    sends of :112-124 first, then the send at :46 and the receive at :49), range_check_u8
    (air/u8_air.rs:8-15), eval_clk's 24-bit range check (cpu/air.rs:117-122)."""
    m, c = r.m, r.const
    clk = (m["clk_8bit_limb"] * np.uint64(1 << 16) + m["clk_16bit_limb"]) % np.uint64(P)
    sends = [
        # air/program.rs:21-26: pc, opcode, then the whole instruction (opcode again, op_a)
        (PROGRAM, [m["pc"], m["opcode"], m["opcode"]] + [m[x] for x in _word("op_a")], m["is_real"]),
        (ALU, [m["pc"], m["opcode"], m["next_mv"], m["mv"]], m["is_alu"]),
        (JUMP, [m["pc"], m["next_pc"], m["opcode"], m["mv"]], m["is_jump"]),
        (MEMINSTR, [clk, m["pc"], m["opcode"], m["mp"], m["next_mp"]], m["is_memory_instr"]),
        (IO, [m["pc"], m["opcode"], m["mp"], m["mv"]], m["is_io"]),
    ]
    recvs = []
    for acc, used, dt in (("mv_access", "mv_accessed", 1), ("next_mv_access", "next_mv_accessed", 2)):
        sends += [
            (BYTE, [c(U16_RANGE), c(0), m[f"{acc}.diff_16bit_limb"]], m[used]),
            (BYTE, [c(U8_RANGE), m[f"{acc}.diff_8bit_limb"], c(0)], m[used]),
            (MEMORY, [m[f"{acc}.prev_clk"], m["mp"], m[f"{acc}.prev_value"]], m[used]),
        ]
        recvs.append((MEMORY, [(clk + np.uint64(dt)) % np.uint64(P), m["mp"], m[f"{acc}.value"]], m[used]))
    sends += [
        (BYTE, [c(U8_RANGE), m["mv"], c(0)], m["is_real"]),
        (BYTE, [c(U16_RANGE), c(0), m["clk_16bit_limb"]], m["is_real"]),
        (BYTE, [c(U8_RANGE), m["clk_8bit_limb"], c(0)], m["is_real"]),
    ]
    return sends, recvs


def program(r):
    """program/mod.rs:152-163 with air/program.rs:36-41."""
    p = r.p
    return [], [(PROGRAM, [p["pc"], p["opcode"], p["opcode"]] + [p[x] for x in _word("op_a")],
                 r.m["multiplicity"])]


def addsub(r):
    """alu/mod.rs:155-193; the three byte sends are AddOperation::eval's (operations/add.rs:44-76:
    a, b, value) under is_add + is_sub."""
    m, c = r.m, r.const
    real = (m["is_add"] + m["is_sub"]) % np.uint64(P)
    sends = [(BYTE, [c(U8_RANGE), m[x], c(0)], real)
             for x in ("operand_1", "operand_2", "add_operation.value")]
    recvs = [
        (ALU, [m["pc"], c(ADD), m["add_operation.value"], m["operand_1"]], m["is_add"]),
        (ALU, [m["pc"], c(SUB), m["operand_1"], m["add_operation.value"]], m["is_sub"]),
    ]
    return sends, recvs


def jump(r):
    """jump/air.rs:72-81."""
    m = r.m
    real = (m["is_loop_start"] + m["is_loop_end"]) % np.uint64(P)
    opcode = (m["is_loop_start"] * np.uint64(LOOP_START) + m["is_loop_end"] * np.uint64(LOOP_END)) % np.uint64(P)
    return [], [(JUMP, [r.word("pc"), r.word("next_pc"), opcode, m["mv"]], real)]


def memory(r):
    """memory/memory.rs:132-145: per entry a receive of the initial and a send of the final
    access."""
    m = r.m
    sends = [(MEMORY, [m[f"e{k}.final_clk"], m[f"e{k}.addr"], m[f"e{k}.final_value"]], m[f"e{k}.is_real"])
             for k in range(2)]
    recvs = [(MEMORY, [m[f"e{k}.initial_clk"], m[f"e{k}.addr"], m[f"e{k}.initial_value"]], m[f"e{k}.is_real"])
             for k in range(2)]
    return sends, recvs


def byte(r):
    """bytes/air.rs:21-44."""
    c = r.const
    return [], [(BYTE, [c(U8_RANGE), r.p["value_u8"], c(0)], r.m["mult_u8"]),
                (BYTE, [c(U16_RANGE), c(0), r.p["value_u16"]], r.m["mult_u16"])]


def meminstrs(r):
    """memory/instructions/air.rs:65-75."""
    m = r.m
    real = (m["is_step_forward"] + m["is_step_backward"]) % np.uint64(P)
    opcode = (m["is_step_forward"] * np.uint64(FORWARD) + m["is_step_backward"] * np.uint64(BACKWARD)) % np.uint64(P)
    return [], [(MEMINSTR, [m["clk"], m["pc"], opcode, r.word("mp"), r.word("next_mp")], real)]


def io(r):
    """io/mod.rs:127-141."""
    m = r.m
    real = (m["is_input"] + m["is_output"]) % np.uint64(P)
    opcode = (m["is_input"] * np.uint64(INPUT) + m["is_output"] * np.uint64(OUTPUT)) % np.uint64(P)
    return [], [(IO, [m["pc"], opcode, m["mp"], m["mv"]], real)]


CHIPS = (cpu, program, addsub, jump, memory, byte, meminstrs, io)


def interactions(chip, main, prep):
    """[(kind, is_send, values (n, nvals) uint64, multiplicity (n,) uint64)] in chain order."""
    sends, recvs = CHIPS[chip](Row(chip, np.asarray(main), None if prep is None else np.asarray(prep)))
    out = []
    for is_send, group in ((True, sends), (False, recvs)):
        for kind, values, mult in group:
            out.append((kind, is_send, np.stack([v % np.uint64(P) for v in values], axis=1),
                        mult % np.uint64(P)))
    return out


assert sum(len(interactions(c, np.zeros((1, WIDTHS[c]), dtype=np.uint32),
                            np.zeros((1, len(PREP_COLS[c])), dtype=np.uint32) if c in PREP_COLS else None))
           for c in range(8)) == 31


def field_to_int(x):  # lookup/debug.rs:46-54
    x %= P
    return x - P if x > P // 2 else x


def debug_interactions(traces, kinds=None):
    """traces: {chip: (main, prep or None)} canonical.  kinds: kind indices (None = all).
    Returns the report of debug_interactions_with_all_chips (lookup/debug.rs:125-196) as a dict;
    records: every unbalanced key in (kind, values) order."""
    want = set(range(1, 8)) if kinds is None else set(kinds)
    table = {}  # (kind, *values) -> [net mod p, chip_net[8], chip_count[8], first]
    n_inter = 0
    for chip in sorted(traces):
        main, prep = traces[chip]
        for j, (kind, is_send, values, mult) in enumerate(interactions(chip, main, prep)):
            if kind not in want:
                continue
            rows = np.nonzero(mult)[0]  # lookup/debug.rs:94
            vals = values[rows].tolist()
            ms = mult[rows].tolist()
            for row, v, mu in zip(rows.tolist(), vals, ms):
                e = table.setdefault((kind, *v), [0, [0] * 8, [0] * 8, (chip, row, j)])
                sm = mu if is_send else P - mu
                e[0] = (e[0] + sm) % P
                e[1][chip] = (e[1][chip] + sm) % P
                e[2][chip] += 1
                e[3] = min(e[3], (chip, row, j))
                n_inter += 1
    records = []
    for key in sorted(k for k, e in table.items() if e[0]):
        e = table[key]
        records.append(dict(kind=key[0], values=list(key[1:]), net=field_to_int(e[0]),
                            chip_net=[field_to_int(x) for x in e[1]], chip_count=list(e[2]),
                            first=e[3]))
    return dict(
        balanced=not records, total_net=field_to_int(sum(e[0] for e in table.values())),
        interactions=n_inter, distinct_keys=len(table), unbalanced_keys=len(records),
        chip_distinct=[sum(1 for e in table.values() if e[2][c]) for c in range(8)],
        records=records)


def key_string(rec):  # lookup/debug.rs:100 with vec_to_string (:30-40)
    return f"{KIND_NAMES[rec['kind']]} ({', '.join(str(v) for v in rec['values'])})"
