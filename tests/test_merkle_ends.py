"""Merkle commitment shapes that pick every end of the loop kernels' permutation and every turn
of the column walk (csrc/merkle.hip: sponge_cols, merkle_node, merkle_node_lane), through
bfz_commit against the oracle's root, bit for bit.

Heights are trace heights n; the committed LDE has 2n rows.  A tallest matrix of 2^15 rows gives
2^16 leaves (k_hash_leaves) and a first layer of 2^15 nodes, the smallest one k_compress runs in
thread mode (> 2^14 nodes); a matrix of 2^14 rows is injected there, shorter ones into the
lane-mode layers above.
"""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
from bfz import _lib

pytestmark = pytest.mark.gpu
P = O.P
P32 = ctypes.POINTER(ctypes.c_uint32)
T = 1 << 15  # tallest trace height


def mont(a):
    return ((np.asarray(a, dtype=np.uint64) << np.uint64(32)) % np.uint64(P)).astype(np.uint32)


def unmont(a):
    inv = pow(2, -32, P)
    return ((np.asarray(a, dtype=np.uint64) * np.uint64(inv)) % np.uint64(P)).astype(np.uint32)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.init(0)
    yield


def commit_case(shapes, seed):
    rng = np.random.default_rng(seed)
    mats = [rng.integers(0, P, size=s, dtype=np.uint64).astype(np.uint32) for s in shapes]
    exp = O.merkle_root([O.coset_lde(m, 3) for m in mats])
    dev = [mont(m).copy() for m in mats]
    ptrs = (P32 * len(dev))(*[d.ctypes.data_as(P32) for d in dev])
    hs = (ctypes.c_size_t * len(dev))(*[s[0] for s in shapes])
    ws = (ctypes.c_size_t * len(dev))(*[s[1] for s in shapes])
    root = (ctypes.c_uint32 * 8)()
    _lib.check(_lib.lib().bfz_commit(ptrs, hs, ws, len(dev), root))
    assert unmont(list(root)).tolist() == exp


# A short first chunk (1, 7), exactly full chunks (8, 16), full chunks then a partial one
# (9, 17), the headline's widths (31, 36).  Width 8 alone is also the tree whose every
# k_compress layer has nothing injected (a single step).
@pytest.mark.parametrize("w", [1, 7, 8, 9, 16, 17, 31, 36])
def test_leaf_widths(w):
    commit_case([(T, w)], 100 + w)


# Matrices of one height: a segment's end inside a chunk, on a chunk's end, and twice.
@pytest.mark.parametrize("ws", [(5, 12), (8, 8), (3, 5, 9)])
def test_leaf_segments(ws):
    commit_case([(T, w) for w in ws], 200 + sum(ws))


# Injection into the thread-mode layer (2^15 nodes).
@pytest.mark.parametrize("ws", [(1,), (8,), (9,), (41,), (7, 45)])
def test_inject_thread_layer(ws):
    commit_case([(T, 8)] + [(T >> 1, w) for w in ws], 300 + sum(ws))


# Injection into lane-mode layers: a medium layer (k_compress_lanes) and subtree launches
# (k_compress_top), two matrices of one height among them.
@pytest.mark.parametrize("small", [[(1 << 12, 9), (1 << 9, 45)], [(16, 5), (16, 12)]])
def test_inject_lane_layers(small):
    commit_case([(T, 8)] + small, 400 + len(small) + small[0][1])
