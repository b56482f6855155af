"""Every NTT / LDE kernel path of csrc/ntt.hip against the oracle's coset_lde, bit for bit: each
height (one template instantiation each), the lazy-reduction edge values, strided, unaligned and
in-place sources, and every sharded path (fused, half-LDE, unfused) at every world size the API
takes.  Through the test hooks bfz_coset_lde_ex / bfz_lde_shard, which call the production
dispatch and report the kernel families launched (bfz_ntt_last_paths), so a case also asserts
that it ran the path it names.

References: oracle_lib.coset_lde (rows bit-reversed: shard k of G is its rows [k m, (k+1) m),
m = 2n / G) and, for the coefficients a shard stores, the numpy model of ntt_cases.py, which
test_ntt_reference.py pins to the oracle.
"""
import ctypes

import numpy as np
import pytest

import ntt_cases as N
import oracle_lib as O
from bfz import _lib

pytestmark = pytest.mark.gpu
P = N.P
P32 = ctypes.POINTER(ctypes.c_uint32)
SENT = N.SENTINEL

# csrc/ntt.h NTT_* bits
PASS_DIT, PASS_DIF, R16_DIT, R16_DIF = 1 << 0, 1 << 1, 1 << 2, 1 << 3
TILE_DIT_DIN, TILE_DIT, TILE_DIF = 1 << 4, 1 << 5, 1 << 6
LDE_TINY, SCALE_SPLIT, MID_FULL, MID_HALF, MID_SHARD = 1 << 7, 1 << 8, 1 << 9, 1 << 10, 1 << 11
FOLD_R0, FOLD_R2, FOLD_R3, FOLD_RESIDUE = 1 << 12, 1 << 13, 1 << 14, 1 << 15
FOLDS = FOLD_R0 | FOLD_R2 | FOLD_R3 | FOLD_RESIDUE | MID_SHARD


def TILE_B(b):
    return 1 << (16 + b - 8)


UNFUSED, NO_MID_HALF, NO_FUSED_DIF = 1, 2, 4  # bfz_lde_shard flags
IN_PLACE, NO_TINY = 1, 2                      # bfz_coset_lde_ex mode


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.init(0)
    yield


# ------------------------------------------------------------------ inputs and references
_WORDS, _ORACLE, _COEF = {}, {}, {}


def words_of(logn, kind):
    """Device (Montgomery) words, n x w, natural rows.  kind: "edge" (the 14 edge columns),
    "big" (random, all p-1), "shard" (all p-1, random, random), "r64" (64 random columns)."""
    key = (logn, kind)
    if key not in _WORDS:
        n = 1 << logn
        rng = np.random.default_rng(1000 * logn + sum(map(ord, kind)))
        rnd = lambda w: rng.integers(0, P, size=(n, w), dtype=np.uint64).astype(np.uint32)
        if kind == "edge":
            m = N.edge_columns(logn, seed=logn)
        elif kind == "big":
            m = np.concatenate([rnd(1), np.full((n, 1), P - 1, dtype=np.uint32)], axis=1)
        elif kind == "shard":
            m = np.concatenate([np.full((n, 1), P - 1, dtype=np.uint32), rnd(2)], axis=1)
        else:
            m = rnd(64)
        m.setflags(write=False)
        _WORDS[key] = m
    return _WORDS[key]


def shard_words(logn):
    """(d): three columns (all p-1 and two random) up to 2^20, the random column of "big" above."""
    return ("shard", 3) if logn <= 20 else ("big", 1)


def oracle_lde(logn, kind, shift):
    """O.coset_lde of words_of(logn, kind) (all its columns), canonical, computed once."""
    key = (logn, kind, shift)
    if key not in _ORACLE:
        e = O.coset_lde(N.unmont(words_of(logn, kind)), shift)
        e.setflags(write=False)
        _ORACLE[key] = e
    return _ORACLE[key]


def model_coef(logn, kind, w):
    key = (logn, kind, w)
    if key not in _COEF:
        c = N.n_coefficients(N.unmont(words_of(logn, kind)[:, :w]))
        c.setflags(write=False)
        _COEF[key] = c
    return _COEF[key]


def w2n_inv(logn):
    return pow(N.two_adic_gen(logn + 1), P - 2, P)


def shifts_of(logn):
    return (1, w2n_inv(logn), int(np.random.default_rng(77 + logn).integers(2, P)))


def dshift(shift):
    return int(N.mont([shift])[0])


def last_paths():
    m = ctypes.c_uint32()
    _lib.check(_lib.lib().bfz_ntt_last_paths(ctypes.byref(m)))
    return m.value


def dev_lde(words, shift, stride=None, skew=0, only_half=-1, mode=0):
    """bfz_coset_lde_ex -> (raw output words 2n x w, path mask)."""
    src = np.ascontiguousarray(words)
    n, w = src.shape
    out = np.zeros((2 * n, w), dtype=np.uint32)
    _lib.check(_lib.lib().bfz_coset_lde_ex(src.ctypes.data_as(P32), n, w,
                                           n if stride is None else stride, skew, dshift(shift),
                                           only_half, mode, out.ctypes.data_as(P32)))
    return out, last_paths()


def dev_shard(words, shift, lg, rank, next_rank=0, next_cols=(), j0=0, ln=0, flags=0,
              want_coef=True):
    """bfz_lde_shard -> (coef n x w, shard m x w, next m x len(next_cols), dft_low, paths), raw."""
    src = np.ascontiguousarray(words)
    n, w = src.shape
    m = (2 * n) >> lg
    coef = np.zeros((n, w) if want_coef else (0, w), dtype=np.uint32)
    shard = np.zeros((m, w), dtype=np.uint32)
    nxt = np.zeros((m, max(len(next_cols), 1)), dtype=np.uint32)
    nc = (ctypes.c_int * max(len(next_cols), 1))(*next_cols)
    low = ctypes.c_int(99)
    _lib.check(_lib.lib().bfz_lde_shard(src.ctypes.data_as(P32), n, w, dshift(shift), lg, rank,
                                        next_rank, nc, len(next_cols), j0, ln, flags,
                                        coef.ctypes.data_as(P32) if want_coef else None,
                                        shard.ctypes.data_as(P32),
                                        nxt.ctypes.data_as(P32), ctypes.byref(low)))
    return coef, shard, nxt[:, :len(next_cols)], low.value, last_paths()


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def next_rank_of(rank, lg):
    """The owner of rows i + 2 (make_plan: r = bitrev(k), r2 = (r + 2) mod G, k2 = bitrev(r2))."""
    return bitrev((bitrev(rank, lg) + 2) % (1 << lg), lg)


def same(raw, exp):
    """Raw device words are the canonical values exp (and no word is the sentinel)."""
    return bool((raw < P).all()) and np.array_equal(N.unmont(raw), exp)


def full_paths(logn, no_tiny=False):
    """The families a full coset LDE of height 2^logn launches (csrc/ntt.hip coset_lde_ex)."""
    if logn > 14:
        return MID_FULL | TILE_DIF | TILE_B(min(14, logn - 4))
    if 1 <= logn <= 8 and not no_tiny:
        return LDE_TINY
    if logn == 0:
        return SCALE_SPLIT
    if logn < 4:
        return SCALE_SPLIT | PASS_DIT | PASS_DIF
    if logn < 8:
        return SCALE_SPLIT | R16_DIT | R16_DIF
    return SCALE_SPLIT | TILE_DIF | TILE_B(logn)


DIT_KINDS = TILE_DIT_DIN | TILE_DIT


# ------------------------------------------------------------------ (a) full LDE, every height
@pytest.mark.parametrize("logn", range(0, 24))
def test_full_lde_every_height(logn):
    """Shift 3, the 14 edge columns up to 2^20, a random and an all-(p-1) column above."""
    kind = "edge" if logn <= 20 else "big"
    got, paths = dev_lde(words_of(logn, kind), 3)
    assert same(got, oracle_lde(logn, kind, 3))
    assert paths & ~DIT_KINDS == full_paths(logn), hex(paths)
    if logn >= 9:
        assert paths & DIT_KINDS == TILE_DIT_DIN  # aligned contiguous source


@pytest.mark.parametrize("logn", [3, 8, 9, 14, 15, 18])
def test_full_lde_shifts(logn):
    for shift in shifts_of(logn):
        got, _ = dev_lde(words_of(logn, "edge"), shift)
        assert same(got, oracle_lde(logn, "edge", shift)), shift


@pytest.mark.parametrize("logn", [1, 2, 3, 5, 8])
def test_general_path_below_the_tile_sizes(logn):
    """The three-launch path at the heights the one-block kernel normally serves: k_ntt_pass
    (below 2^4), k_ntt_r16 (2^4 .. 2^7), the 2^8 tile."""
    got, paths = dev_lde(words_of(logn, "edge"), 3, mode=NO_TINY)
    assert same(got, oracle_lde(logn, "edge", 3))
    assert paths & ~DIT_KINDS == full_paths(logn, no_tiny=True), hex(paths)


# ------------------------------------------------------------------ (b) column counts
def mid_c2(logn):
    """MidPlan<L>::c2 (csrc/ntt.hip): the coalesced run of a second-pass tile."""
    b1 = min(logn - 4, 14)
    b2 = logn - b1
    return min(b1, 14 - b2, 5)


@pytest.mark.parametrize("logn", [9, 14, 15, 16, 19])
def test_full_lde_column_counts(logn):
    """Widths around 2^c2 (5 at every two-pass height; the same widths below), 1 and 64: the first
    w of 64 random columns, so one oracle LDE serves all of them."""
    c2 = mid_c2(max(logn, 15))
    assert c2 == 5
    exp = oracle_lde(logn, "r64", 3)
    for w in (1, (1 << c2) - 1, 1 << c2, (1 << c2) + 1, 64):
        got, _ = dev_lde(words_of(logn, "r64")[:, :w], 3)
        assert same(got, exp[:, :w]), w


# ------------------------------------------------------------------ (c) coset_lde_ex contract
EX_HEIGHTS = [1, 5, 8, 9, 12, 14, 15, 17, 18]


def ex_words(logn):
    return words_of(logn, "edge")[:, [2, 6, 11, 13]]  # p-1, alt(a, p-a), w_n^i, random


def ex_oracle(logn, shift):
    return oracle_lde(logn, "edge", shift)[:, [2, 6, 11, 13]]


@pytest.mark.parametrize("logn", EX_HEIGHTS)
@pytest.mark.parametrize("half", [0, 1])
def test_lde_ex_only_half(logn, half):
    n = 1 << logn
    got, paths = dev_lde(ex_words(logn), 3, only_half=half)
    exp = ex_oracle(logn, 3)
    assert same(got[half * n:(half + 1) * n], exp[half * n:(half + 1) * n])
    assert (got[(1 - half) * n:(2 - half) * n] == SENT).all()  # the other half: untouched
    if logn > 14:
        assert paths & MID_HALF and not paths & MID_FULL


@pytest.mark.parametrize("logn", EX_HEIGHTS)
@pytest.mark.parametrize("half", [1, 0])
def test_lde_ex_in_place(logn, half):
    """As the quotient chunks call it: the source is the other half of the output buffer, at
    stride 2n, with shift 1 (computing half 1) or w_2n^-1 (half 0).  The whole buffer is then the
    oracle's LDE, so the source half is unchanged."""
    shift = 1 if half == 1 else w2n_inv(logn)
    got, _ = dev_lde(ex_words(logn), shift, stride=2 << logn, only_half=half, mode=IN_PLACE)
    assert same(got, ex_oracle(logn, shift))


@pytest.mark.parametrize("logn", EX_HEIGHTS)
def test_lde_ex_strides_and_skews(logn):
    """Strides n + 1, n + 4, 2n and sources 1, 2, 3 words past a 16-byte boundary.  A source that
    is not 16-byte aligned, or whose stride is no multiple of 4 words, takes the tile kernel
    without the direct first window (every height above 2^8 starts with a DIT tile pass)."""
    n = 1 << logn
    exp = ex_oracle(logn, 3)
    for stride, skew in ((n + 1, 0), (n + 4, 0), (2 * n, 0), (n, 1), (n, 2), (n, 3), (n + 1, 3)):
        got, paths = dev_lde(ex_words(logn), 3, stride=stride, skew=skew)
        assert same(got, exp), (stride, skew)
        if logn >= 9:
            unaligned = skew != 0 or stride % 4 != 0
            assert paths & DIT_KINDS == (TILE_DIT if unaligned else TILE_DIT_DIN), (stride, skew)


def test_lde_ex_refuses_nonsense():
    L, z = _lib.lib(), np.zeros((16, 1), dtype=np.uint32)
    out = np.zeros((32, 1), dtype=np.uint32)
    for stride, skew, half, mode in ((32, 0, -1, IN_PLACE), (8, 0, -1, 0), (16, 4, -1, 0),
                                     (16, 0, 2, 0), (16, 0, 1, IN_PLACE)):
        assert L.bfz_coset_lde_ex(z.ctypes.data_as(P32), 16, 1, stride, skew, dshift(3), half, mode,
                                  out.ctypes.data_as(P32)) != 0


# ------------------------------------------------------------------ (d) shards
def shard_paths(logn, lg, flags, has_next):
    """(fold family, dft_low) of one rank's sharded LDE (csrc/ntt.hip coef_fold_residues)."""
    if logn <= 14 or logn > 23 or lg > 5 or flags & UNFUSED:
        return FOLD_RESIDUE, -2
    b1 = min(logn - 4, 14)
    if lg == 1 and not has_next and not flags & NO_MID_HALF:
        return MID_SHARD, b1
    if lg in (2, 3) and not flags & NO_FUSED_DIF:
        return (FOLD_R3 if lg == 2 else FOLD_R2), b1
    return FOLD_R0, -1


def coef_buffer(logn, kind, w, j0, ln, fused):
    """Every word of the coefficient buffer after a rank's sharded LDE.  The unfused path stores
    all n coefficients.  The fused path runs the inverse DFT's first pass into the buffer and its
    second pass stores coefficients for [j0, j0 + len) only, so every other word still holds the
    first pass's value (nothing reads those; a stray coefficient store shows as a mismatch)."""
    coef = model_coef(logn, kind, w)
    if not fused:
        return coef
    key = (logn, kind, w, "pass1")
    if key not in _COEF:
        p1 = N.first_pass(N.unmont(words_of(logn, kind)[:, :w]), min(logn - 4, 14))
        p1.setflags(write=False)
        _COEF[key] = p1
    e = _COEF[key].copy()
    e[j0:j0 + ln] = coef[j0:j0 + ln]
    return e


def check_shards(logn, lg, flags, ranks, whole):
    kind, w = shard_words(logn)
    words = words_of(logn, kind)[:, :w]
    exp = oracle_lde(logn, kind, 3)[:, :w]
    coef = model_coef(logn, kind, w)
    n, G = 1 << logn, 1 << lg
    m, ln = 2 * n // G, n // G
    fam, low = shard_paths(logn, lg, flags, False)
    parts = []
    for k in ranks:
        j0 = k * ln
        c, s, _, dft_low, paths = dev_shard(words, 3, lg, k, j0=j0, ln=ln, flags=flags)
        assert paths & FOLDS == fam and dft_low == low, (k, hex(paths), dft_low)
        assert same(s, exp[k * m:(k + 1) * m]), k
        assert same(c[j0:j0 + ln], coef[j0:j0 + ln]), k
        assert same(c, coef_buffer(logn, kind, w, j0, ln, fam != FOLD_RESIDUE)), k
        parts.append(s)
    if whole:
        assert same(np.concatenate(parts), exp)


def shard_ranks(logn, lg):
    G = 1 << lg
    return list(range(G)) if logn <= 20 else sorted({0, 1, G // 2, G - 1})


@pytest.mark.parametrize("lg", range(1, 6))
@pytest.mark.parametrize("logn", range(15, 24))
def test_shards_fused(logn, lg):
    """Every k_coef_fold<L, R> / shard-half k_lde_mid<L> instantiation: 2 ranks the half LDE, 4
    and 8 the folds with fused DIF stages (R = 3, 2), 16 and 32 the plain folds (R = 0)."""
    check_shards(logn, lg, 0, shard_ranks(logn, lg), whole=logn <= 20)


@pytest.mark.parametrize("flags", [NO_MID_HALF, NO_FUSED_DIF, UNFUSED])
@pytest.mark.parametrize("lg", range(1, 4))
@pytest.mark.parametrize("logn", [15, 16, 18, 20])
def test_shards_ab_switches(logn, lg, flags):
    """k_coef_fold<L, 0> at 2 / 4 / 8 ranks (no half LDE, no fused DIF) and the unfused
    k_fold_residue + ntt_passes at heights the fused path normally serves."""
    check_shards(logn, lg, flags, shard_ranks(logn, lg), whole=True)


# ------------------------------------------------------------------ (e) next-row residue
@pytest.mark.parametrize("logn,lg", [(15, 2), (15, 3), (15, 5), (17, 2), (17, 3), (17, 5),
                                     (20, 2), (20, 3), (20, 5), (12, 2)])
@pytest.mark.parametrize("w,next_cols", [(5, (0, 3, 4)), (64, (63,)), (64, tuple(range(64)))],
                         ids=["w5", "w64-last", "w64-all"])
def test_shards_next_row(logn, lg, w, next_cols):
    """The second residue of a fold (the rows of the rank that owns rows i + 2) for a subset of
    the columns, through the column map."""
    words = words_of(logn, "r64")[:, :w]
    exp = oracle_lde(logn, "r64", 3)[:, :w]
    G = 1 << lg
    m = (2 << logn) // G
    fam, low = shard_paths(logn, lg, 0, True)
    for k in sorted({0, 1, G // 2, G - 1}):
        k2 = next_rank_of(k, lg)
        _, s, nx, dft_low, paths = dev_shard(words, 3, lg, k, next_rank=k2, next_cols=next_cols,
                                             want_coef=False)
        assert paths & FOLDS == fam and dft_low == low, (k, hex(paths), dft_low)
        assert same(s, exp[k * m:(k + 1) * m]), k
        assert same(nx, exp[k2 * m:(k2 + 1) * m][:, list(next_cols)]), k


# ------------------------------------------------------------------ (f) coefficient ranges
@pytest.mark.parametrize("lg", [1, 2])
@pytest.mark.parametrize("logn", [15, 16])
def test_shards_coefficient_range_edges(logn, lg):
    """[j0, j0 + len) = everything, nothing, the last coefficient alone, an unaligned few; at
    two ranks both through the fold kernel (with next-row columns) and through k_lde_mid's side
    output (without)."""
    n = 1 << logn
    words = words_of(logn, "shard")
    exp = oracle_lde(logn, "shard", 3)
    coef = model_coef(logn, "shard", 3)
    m = 2 * n >> lg
    k = 1
    for next_cols in ((1,), ()) if lg == 1 else ((1,),):
        fam, _ = shard_paths(logn, lg, 0, bool(next_cols))
        for j0, ln in ((0, n), (0, 0), (n - 1, 1), (5, 7)):
            c, s, _, _, paths = dev_shard(words, 3, lg, k, next_rank=next_rank_of(k, lg),
                                          next_cols=next_cols, j0=j0, ln=ln)
            assert paths & FOLDS == fam, hex(paths)
            assert same(s, exp[k * m:(k + 1) * m])
            assert same(c[j0:j0 + ln], coef[j0:j0 + ln]), (j0, ln)
            assert same(c, coef_buffer(logn, "shard", 3, j0, ln, True)), (j0, ln)


# ------------------------------------------------------------------ (g) small shards, unfused
@pytest.mark.parametrize("logn", range(10, 15))
def test_small_shards(logn):
    """Below 2^15 the prover's shards are unfused; every world size with blocks of 2^10 rows or
    more, all ranks."""
    for lg in range(1, logn + 1 - 10 + 1):
        assert (2 << logn) >> lg >= 1024
        check_shards_small(logn, lg, 0)


@pytest.mark.parametrize("logn,logm", [(10, 4), (10, 6), (10, 8), (11, 6), (11, 8)])
def test_small_shards_tiny_blocks(logn, logm):
    """Blocks of 16, 64 and 256 rows: the residue's DIF runs k_ntt_r16 (log m = 4, 6) and the 2^8
    tile (at most 64 coefficients fold into one output, so 2^11 stops at 64 rows)."""
    paths = check_shards_small(logn, logn + 1 - logm, UNFUSED)
    if logm < 8:
        assert paths & R16_DIF and not paths & (TILE_DIF | PASS_DIF), hex(paths)
    else:
        assert paths & TILE_DIF and paths & TILE_B(8) and not paths & (R16_DIF | PASS_DIF), hex(paths)


def test_small_shards_fold_limit():
    """2^11 rows in blocks of 16 would fold 128 coefficients into one output: k_fold_residue takes
    64 at the most, and the call says so instead of launching."""
    words = np.ascontiguousarray(words_of(11, "edge"))
    out = np.zeros((1 << 11, 14), dtype=np.uint32)
    low, nc = ctypes.c_int(), (ctypes.c_int * 1)()
    rc = _lib.lib().bfz_lde_shard(words.ctypes.data_as(P32), 1 << 11, 14, dshift(3), 8, 0, 0, nc, 0,
                                  0, 0, UNFUSED, out.ctypes.data_as(P32), out.ctypes.data_as(P32),
                                  out.ctypes.data_as(P32), ctypes.byref(low))
    assert rc != 0 and b"64 folds" in _lib.lib().bfz_last_error()


def check_shards_small(logn, lg, flags):
    words = words_of(logn, "edge")
    exp = oracle_lde(logn, "edge", 3)
    coef = model_coef(logn, "edge", 14)
    G = 1 << lg
    m = (2 << logn) // G
    parts, paths = [], 0
    for k in range(G):
        c, s, _, dft_low, paths = dev_shard(words, 3, lg, k, j0=0, ln=0, flags=flags)
        assert paths & FOLDS == FOLD_RESIDUE and dft_low == -2
        assert same(s, exp[k * m:(k + 1) * m]), k
        parts.append(s)
        if k == 0:
            assert same(c, coef)
    assert same(np.concatenate(parts), exp)
    return paths
