"""The reference's word on what a verdict must be: a full single-field tamper sweep
(tests/tamper.py) through the restated verifier, on the CPU.

The seven circuits are those of tests/test_verifier_gpu.py's CIRCUITS — boolean (boolean1),
public_sum, ranged (range_full_254), logic (and_30), fixed_base (test_circuit_20_5),
variable_base (add_point) and chain_40_public — proved by the C oracle
(oracle/plk_prover_oracle.c) as in test_prover_oracle.test_oracle_proof_verifies. For each:

* the honest proof is accepted by verifier.verify and by verifier_pair.accepts;
* every item of tamper.variants (each of the 16 evaluations +-1, each of the 11 commitments
  +G / negated / identity, each public input +1, the first two swapped) and of
  tamper.key_variants (each of the 15 key commitments +G, label, m + 1, 2n, the first public
  input index + 1) is rejected by verifier_pair.accepts, with no exception raised. The number of
  variants skipped because they would equal the original is 0 for all seven circuits, and the
  test asserts it;
* the first evaluation, commitment, key commitment and public input variants are also
  rejected by verifier.verify;
* plk_verifier_challenges (host code, no GPU) returns for EVERY tamper.variants item exactly
  verifier_pair.pair's challenges — no field is missing from the product's transcript. The
  pair computed for the verdict is the one compared, so nothing is sampled.

Each circuit's sweep is split into three cases (evaluations, commitments, inputs and key) to
keep a case near ten seconds.

tests/test_verifier_soundness_gpu.py relies on this file for the expected verdicts and does
not call the restated verifier per variant.
"""
import numpy as np
import pytest

import pyref as P
import tamper
import verifier
import verifier_pair as VP
from test_prover_oracle import OracleProof, build, oracle_prove, tau_for, vd_for
from test_verifier_gpu import CIRCUITS

SEEDS = {name: 71 + i for i, name in enumerate(CIRCUITS)}


def accepts(pair, tau):
    """verifier_pair.accepts on an already computed pair."""
    _, c, w = pair
    return c == VP.gmul(w, tau)


_CASES = {}


def case(oracle, name):
    """The oracle's proof of one circuit, made once: (vd, proof, public inputs, tau)."""
    if name not in _CASES:
        from dusk_plonk_amd.prover import Proof, fr_int
        seed = SEEDS[name]
        tau_limbs, tau = tau_for(seed + 100)
        cs = build(CIRCUITS[name])
        res = oracle_prove(oracle, cs, b"oracle", seed, tau_limbs)
        proof = Proof.from_words(res["comms"], res["evals"])
        _CASES[name] = (vd_for(res, cs, b"oracle"), proof, [fr_int(p) for p in res["pis"]], tau)
    return _CASES[name]


# One case per circuit and part, so that no case runs much longer than ten seconds: a restated
# pair costs 0.1 - 0.2 s and a circuit's sweep holds 84 to 125 of them. The parts partition the
# sweep; nothing is sampled.
PARTS = {"evaluations": ("eval",), "commitments": ("comm+G", "comm neg", "comm identity"),
         "inputs and key": ("pi",)}


@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("name", list(CIRCUITS))
def test_every_single_field_change_is_rejected(plk, oracle, name, part):
    vd, proof, pis, tau = case(oracle, name)
    ver = vd.verifier()
    verifier.verify(vd, proof, pis, tau)
    honest = VP.pair(vd, proof, pis)
    assert accepts(honest, tau) and VP.accepts(vd, proof, pis, tau)
    assert ver.challenges(proof, pis) == honest[0]

    skipped = []
    items = list(tamper.variants(proof, pis, skipped))
    assert skipped == []
    npi = len(pis)
    names = [what for what, _, _ in items]
    assert len(names) == len(set(names)) == 32 + 33 + npi + (1 if npi >= 2 else 0)
    assert {tamper.kind(what) for what in names} == set(tamper.KINDS[: 5 if npi else 4])
    mine = [it for it in items if tamper.kind(it[0]) in PARTS[part]]
    assert len(mine) == {"evaluations": 32, "commitments": 33}.get(part, len(items) - 65)
    for what, p, pi in mine:
        pair = VP.pair(vd, p, pi)
        assert not accepts(pair, tau), what
        assert ver.challenges(p, pi) == pair[0], what
        assert pair[0] != honest[0], what  # every field reaches the transcript
    # the same verdict from verifier.verify on the first of the part
    for what, p, pi in mine[:1]:
        with pytest.raises(verifier.VerificationError):
            verifier.verify(vd, p, pi, tau)

    if part == "inputs and key":
        keys = list(tamper.key_variants(vd))
        assert len(keys) == 15 + 3 + (1 if npi else 0)
        for what, vd2 in keys:
            assert not VP.accepts(vd2, proof, pis, tau), what
        with pytest.raises(verifier.VerificationError):
            verifier.verify(keys[0][1], proof, pis, tau)


def test_helper_works_on_oracle_proofs(plk, oracle):
    """tamper.variants on an OracleProof gives the variants it gives on a Proof, and leaves
    the original untouched."""
    from dusk_plonk_amd.prover import Proof, fr_int
    tau_limbs, _ = tau_for(171)
    cs = build(CIRCUITS["public_sum"])
    res = oracle_prove(oracle, cs, b"oracle", 71, tau_limbs)
    a, b = OracleProof(res), Proof.from_words(res["comms"], res["evals"])
    pis = [fr_int(p) for p in res["pis"]]
    va, vb = list(tamper.variants(a, pis)), list(tamper.variants(b, pis))
    assert [v[0] for v in va] == [v[0] for v in vb] and len(va) == 66
    for (what, pa, pia), (_, pb, pib) in zip(va, vb):
        assert pia == pib
        differs = 0
        for c in VP.COMM_NAMES:
            assert np.array_equal(getattr(pa, c), getattr(pb, c)), what
            differs += not np.array_equal(getattr(pa, c), getattr(b, c))
        for e in tamper.EVAL_NAMES:
            assert getattr(pa, e) == getattr(pb, e), what
            differs += getattr(pa, e) != getattr(b, e)
        differs += pia != pis
        assert differs == 1, what  # exactly one thing changed
    assert a.a_eval == b.a_eval and np.array_equal(a.a_comm, b.a_comm)
    assert pis == [fr_int(p) for p in res["pis"]]
    assert P.g1_add(tamper.point(b.a_comm), P.G1_GEN) == tamper.point(va[32][1].a_comm)
