"""Machines of caller-defined chips on the device: Machine.prove against the built-in prover byte
for byte (every stage and both segmented kernels on mixed heights), and a custom machine against
a plain Python-integer reference."""
import numpy as np
import pytest

import air_program_cases as A
import bincode_ref as BR
import chip_cases as C
import lookups_cases as L
import machine_cases as M
import uni_stark_model as U
from bfz import _lib, guests, sdk

pytestmark = pytest.mark.gpu
QUERIES = 6


@pytest.fixture(autouse=True)
def few_queries():
    sdk.set_num_queries(QUERIES)
    yield
    sdk.set_num_queries(0)


@pytest.mark.parametrize("prog,stdin,nchips", [(guests.HELLO, (), 8), (guests.LOOP, (), 7)],
                         ids=["hello-all-eight", "loop-without-MemoryInstrs"])
def test_builtin_parity(prog, stdin, nchips):
    """hello includes all eight chips, I/O among them (it prints); loop leaves MemoryInstrs out, so
    a chip of the machine's list is missing from the proof."""
    traces = M.guest_traces(prog, stdin)
    assert len(traces) == nchips
    client, core = sdk.ProverClient(), sdk.CoreProver()
    pk, vk = client.setup(prog)
    m = M.builtin_machine(prog, stdin)
    assert m.prep_root == list(vk.commit)
    tr = [(c, name, main) for c, name, main, _ in traces]
    want = core.prove(pk, tr)
    ch_ref = core.new_challenger()
    core.observe_into(pk, ch_ref)
    assert core.open(pk, core.commit(pk, tr), ch_ref) == want
    ch = m.observe()
    got = m.prove({name: main for _, name, main, _ in traces}, ch)
    assert got == want
    assert bytes(ch) == bytes(ch_ref)
    client.verify(sdk.BfProofWithPublicValues(proof=got, stdin=bytes(stdin)), vk)
    chv = m.observe()
    out = m.verify(got, chv)
    assert out.ok, out.why
    assert bytes(chv) == bytes(ch)


def _canon(t):
    return [[int(x) for x in row] for row in C.unmont(t)]


@pytest.mark.parametrize("heights", [(4,), (1, 512)], ids=["n4", "n1+n512"])
def test_custom_machine(heights, monkeypatch):
    m, traces = M.custom_machine(heights)
    proof = m.prove(traces, m.observe(), check=True)
    out = m.verify(proof, m.observe())
    assert out.ok, out.why
    if heights != (4,):
        return
    # the transcript in Python integers: commit order is table (16 rows), then m4
    n = 4
    monkeypatch.setattr(BR, "CHIPS", ("m4", "table"))  # a chip word indexes the machine's list
    pf = BR.parse_bfz1(proof)
    op = pf["opened"]
    assert pf["chips"] == [1, 0] and [o["log_degree"] for o in op] == [4, 2]
    ch = U.Challenger()
    ch.observe_all([int(x) for x in C.unmont(np.array(m.prep_root, dtype=np.uint32))] + [0] * 7)
    ch.observe_all(pf["roots"][0])
    alpha, beta = list(ch.sample_ef().c), list(ch.sample_ef().c)
    ch.observe_all(pf["roots"][1])
    for o in op:
        ch.observe_all(o["cumsum"])
    qalpha = list(ch.sample_ef().c)
    ch.observe_all(pf["roots"][2])
    zeta = list(ch.sample_ef().c)
    main = _canon(traces["m4"])
    sender = op[1]
    # main_local = the trace's interpolant at zeta (component-wise: the coefficients are in Fp)
    zp = [[1, 0, 0, 0]]
    for _ in range(2 * n):
        zp.append(L.ef_mul(zp[-1], zeta))

    def at_zeta(coef):
        acc = [0] * 4
        for j, c in enumerate(coef):
            acc = L.ef_add(acc, C.ef_scale(zp[j], c))
        return acc

    for c in range(4):
        assert sender["main_local"][c] == at_zeta(C.interpolate([r[c] for r in main], n))
    # the quotient chunks at zeta = the evaluation of ref_quotient's output
    perm, cs = sdk.lookups_perm_trace(M.sender_program(), traces["m4"], None,
                                      C.mont(np.array(alpha)).tolist(), C.mont(np.array(beta)).tolist())
    assert [int(x) for x in C.unmont(np.array(cs, dtype=np.uint32))] == sender["cumsum"]
    q = C.ref_quotient(A.mulgate_mirror, M.sender_program(), main, None, _canon(perm), alpha, beta,
                       sender["cumsum"], qalpha)
    w2n = C.two_adic_gen(3)
    for cc in range(2):  # chunk cc lives on 3 w_2n^cc H_n: rows cc, cc + 2, ... of q
        sh_inv = pow(3 * pow(w2n, cc, C.P) % C.P, C.P - 2, C.P)
        for e in range(4):
            coef = C.interpolate([q[cc + 2 * k][e] for k in range(n)], n)
            val = [0] * 4
            for j, cj in enumerate(coef):
                val = L.ef_add(val, C.ef_scale(zp[j], cj * pow(sh_inv, j, C.P) % C.P))
            assert sender["quotient"][cc][e] == val


@pytest.mark.parametrize("bad,why", [("cell", "OOD evaluation mismatch on chip m4"),
                                     ("mult", "cumulative sums do not sum to zero")])
def test_custom_machine_rejections(bad, why):
    m, traces = M.custom_machine((4,))
    t = dict(traces)
    if bad == "cell":
        t["m4"] = C.flip(traces["m4"], 1, 2)
    else:
        t["table"] = C.flip(traces["table"], 0, 0)
    proof = m.prove(t, m.observe())
    out = m.verify(proof, m.observe())
    assert not out.ok and out.why == why, out
    if bad == "cell":
        with pytest.raises(_lib.BfzError, match=r"chip m4 violates its constraints: row 1, constraint 1"):
            m.prove(t, m.observe(), check=True)


def test_nine_chips_of_one_height_refused():
    """The Merkle commit takes 16 matrices of one height, the quotient round two per chip."""
    names = [f"c{i}" for i in range(9)]
    m = sdk.Machine([(nm, A.mulgate_program(), C.mulgate_lookups(), None) for nm in names])
    with pytest.raises(_lib.BfzError, match="9 chips of height 4, a proof takes at most 8 of one height"):
        m.prove({nm: A.mulgate_case(4)[2] for nm in names}, m.observe())
