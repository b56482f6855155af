"""Chips of AIR degree 4 and 9 on the device: the chip quotient on 3 H_(D n) against Python integers
(slab 0 and k_quotient_machine_coset on the further slabs), and machine proofs whose chips have 8,
4 and 2 quotient chunks against the host verifier's out-of-domain check."""
import re

import numpy as np
import pytest

import chip_cases as C
import chip_high_degree_cases as H
from bfz import sdk

pytestmark = pytest.mark.gpu
MIXED = (("pow9", 512), ("pow4", 4), ("mulgate", 16))  # slab 1: two segments; slabs 2, 3: one
EQUAL = (("pow4", 4), ("pow9", 4))                     # two one-block segments side by side


@pytest.fixture(autouse=True)
def raised_cap():
    sdk.set_num_queries(6)
    sdk.set_chip_max_degree(9)
    yield
    sdk.set_chip_max_degree(0)
    sdk.set_num_queries(0)


@pytest.mark.parametrize("n", [1, 4], ids=["n1-next-wraps", "n4-partial-block"])
@pytest.mark.parametrize("k", [4, 9])
def test_chip_quotient_against_integers(k, n):
    air, lk, mirror = H.pow_chip(k)
    D = 1 << sdk.chip_info(air, lk).log_quotient_degree
    main = H.pow_trace(k, n)
    alpha, beta, qalpha = C.challenges(100 * k + n)
    q, cs = sdk.chip_quotient(air, lk, main, None, alpha, beta, qalpha)
    assert q.shape == (D * n, 4)
    perm, cs2 = sdk.lookups_perm_trace(lk, main, None, alpha, beta)
    assert cs == cs2
    canon = lambda t: [[int(x) for x in row] for row in C.unmont(np.array(t, dtype=np.uint32))]
    want = H.ref_quotient(mirror, lk, canon(main), canon(perm), *(canon([c])[0] for c in (alpha, beta, cs, qalpha)), D)
    assert canon(q) == want


@pytest.mark.parametrize("heights,counts", [(MIXED, {"pow9": 8, "pow4": 4, "mulgate": 2, "table": 2}),
                                            (EQUAL, {"pow9": 8, "pow4": 4, "table": 2})],
                         ids=["mixed-heights", "equal-heights"])
def test_machine_proves_and_verifies(heights, counts):
    m, traces = H.machine(heights)
    ch = m.observe()
    proof = m.prove(traces, ch, check=True)
    chv = m.observe()
    out = m.verify(proof, chv)
    assert out.ok, out.why
    assert bytes(chv) == bytes(ch)
    assert m.prove(traces, m.observe()) == proof
    order = sorted(traces, key=lambda nm: (-len(traces[nm]), nm))  # commit order
    assert H.chunk_counts(proof) == [counts[nm] for nm in order]
    chd, chh = [m.observe()], [m.observe()]
    dev, host = m.verify_batch([proof], chd, on_device=True), m.verify_batch([proof], chh, on_device=False)
    assert dev == host and dev[0].ok, (dev, host)
    assert bytes(chd[0]) == bytes(chh[0]) == bytes(ch)


def test_rejections():
    m, traces = H.machine(EQUAL)
    bad = dict(traces, pow9=C.flip(traces["pow9"], 3, 1))  # a row that sends nothing: the sums still balance
    out = m.verify(m.prove(bad, m.observe()), m.observe())
    assert not out.ok and out.why == "OOD evaluation mismatch on chip pow9", out
    proof = m.prove(traces, m.observe())
    # the same names over pow4's programs: the proof's 8 chunks are not that chip's 4
    other = sdk.Machine([(nm, *(H.pow_chip(4)[:2] if nm == b"pow9" else m.programs[i]), None)
                         for i, nm in enumerate(m.names)], prep_root=m.prep_root,
                        prep_heights={"table": len(traces["table"])})
    out = other.verify(proof, other.observe())
    assert not out.ok and out.why == "opened-value shape mismatch", out
    sdk.set_chip_max_degree(0)
    out = m.verify(proof, m.observe())
    assert not out.ok and re.search(r"chip program: AIR degree [49] is above 3 \(log quotient degree 1\)", out.why), out
