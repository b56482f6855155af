"""Machines of caller-defined chips, host paths: a verifier-only Machine of the exported programs
against the oracle's hello proof (which pins chip_perm_eval_ef and the AIR fold), and
bfz_machine_create's refusals."""
import hashlib

import pytest

import air_program_cases as A
import bincode_ref as BR
import chip_cases as C
import machine_cases as M
import oracle_lib as O
import uni_stark_model as U
from bfz import _lib, guests, sdk


# sha256 of repr(U.challenger_words(ch)) of the challenger in which the built-in prover's bfz_open
# ends on the hello guest at the default query count; its proof is the oracle's, byte for byte
# (tests/test_gpu.py), and bfz_verify hands no challenger back.
HELLO_END = "389d438f69a71aeb50ba1a0ddb749a1102ab389ada2d88e90ad24da387510cb1"


def _verify(proof):
    m = M.builtin_machine(guests.HELLO, verifier_only=True)
    ch = m.observe()
    return m.verify(proof, ch), ch


def _tampered(field):
    model = BR.parse_bfz1(O.prove(guests.HELLO, []))
    v = model["opened"][0][field]
    word = v if field == "cumsum" else v[0]
    word[0] = (word[0] + 1) % O.P
    return BR.encode_bfz1(model)


def test_oracle_hello_proof_accepted():
    out, ch = _verify(O.prove(guests.HELLO, []))
    assert out.ok, out.why
    assert hashlib.sha256(repr(U.challenger_words(ch)).encode()).hexdigest() == HELLO_END


@pytest.mark.parametrize("field,why", [("main_local", "OOD evaluation mismatch on chip"),
                                       ("cumsum", "cumulative sums do not sum to zero")])
def test_tampered_oracle_proof_rejected(field, why):
    """One opened main value changed: rejected at the out-of-domain check.  One cumulative sum
    changed: rejected at the sum check."""
    out, _ = _verify(_tampered(field))
    assert not out.ok and out.why.startswith(why)


def _chip(name="c", air=True, width=4):
    lk = C.mulgate_lookups() if width == 4 else C.prep_lookups()
    return (name, A.mulgate_program() if air else None, lk, None)


@pytest.mark.parametrize("chips,kw,match", [
    ([_chip("a"), _chip("a")], {}, "duplicate chip name a"),
    ([_chip(f"c{i}") for i in range(33)], {}, "33 chips, at most 32"),
    ([_chip("w", width=2)], {}, "the AIR's width 4 is not the interactions' main width 2"),
    ([_chip("p", air=False, width=2)], {"prep_root": [0] * 8, "prep_heights": {"p": 12}},
     "preprocessed height not a power of two"),
], ids=["duplicate", "33-chips", "width", "prep-height"])
def test_create_refusals(chips, kw, match):
    with pytest.raises(_lib.BfzError, match=match):
        sdk.Machine(chips, **({"prep_root": [0] * 8, "prep_heights": {}} | kw))


def test_verifier_only_machine_refuses_to_prove():
    m = sdk.Machine([_chip("g")], prep_root=[0] * 8, prep_heights={})
    with pytest.raises(_lib.BfzError, match="verifier-only machine cannot prove"):
        m.prove({"g": A.mulgate_case(4)[2]}, m.observe())
