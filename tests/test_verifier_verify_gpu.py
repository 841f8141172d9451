"""Verifier::verify to its end on the GPU: every proof's own KZG pair (plk_verifier_pairs,
csrc/verifier.hip k_proof_pairs) against the restated pair and the single folds, bit for bit,
in both replay modes; the batch verdict (plk_verifier_verify) and the per-proof verdicts
(plk_verifier_verify_each) on the circuits of tests/test_verifier_gpu.py, with bad proofs at
the half-wave and wave boundaries of the pairs kernel.
"""
import numpy as np
import pytest

import pyref as P
import verifier_pair as VP
from verifier_pair import copy_proof
from test_prover_oracle import build
from test_verifier_gpu import CIRCUITS, Setup, public_sum_j

pytestmark = pytest.mark.gpu

R = P.R_MOD
COUNT = 67  # two proofs per wave of the pairs kernel, an odd count, more than one wave anywhere
BAD = [0, 31, 32, 33, 64, 66]


class Setup67(Setup):
    def __init__(self, plk):
        super().__init__(plk)
        self.opening = plk.OpeningKey.setup(self.tau)
        prover, _, ver, _, _ = self.key["public_sum"]
        self.proofs, self.pis = [], []
        for j in range(COUNT):
            p, pi = prover.prove_composer(build(public_sum_j(j)), 2000 + j)
            self.proofs.append(p)
            self.pis.append(pi)
        self.singles = np.stack([np.stack(ver.fold([p], [pi], [1])) for p, pi in zip(self.proofs, self.pis)])

    def spoiled(self, at):
        proofs = list(self.proofs)
        for k in at:
            proofs[k] = copy_proof(proofs[k], d_eval=(proofs[k].d_eval + 1 + k) % R)
        return proofs


@pytest.fixture(scope="module")
def S(plk, gpu_ctx):
    return Setup67(plk)


@pytest.mark.parametrize("replay", ["host", "device"])
@pytest.mark.parametrize("name", list(CIRCUITS))
def test_pairs_equal_the_restated_pair_and_the_fold(S, name, replay):
    _, vd, ver, proof, pis = S.key[name]
    _, c, w = VP.pair(vd, proof, pis)
    ver.set_replay(replay)
    try:
        got = ver.pairs([proof], [pis])
    finally:
        ver.set_replay("host")
    assert got.shape == (1, 2, 13)
    assert np.array_equal(got[0, 0], VP.to_words(c)) and np.array_equal(got[0, 1], VP.to_words(w))
    fc, fw = ver.fold([proof], [pis], [1])
    assert np.array_equal(got[0, 0], fc) and np.array_equal(got[0, 1], fw)


@pytest.mark.parametrize("replay", ["host", "device"])
def test_pairs_of_a_batch_equal_the_single_folds(S, replay):
    ver = S.key["public_sum"][2]
    ver.set_replay(replay)
    try:
        got = ver.pairs(S.proofs, S.pis)
    finally:
        ver.set_replay("host")
    assert np.array_equal(got, S.singles)


def test_pairs_with_identity_commitments(S):
    """Identity key commitments (unused widgets) and an identity w_z_chall_w_comm."""
    _, vd, ver, proof, pis = S.key["boolean"]
    assert any(int(c[12]) for c in vd.comms)
    p = copy_proof(proof, w_z_chall_w_comm=np.array([0] * 12 + [1], dtype=np.uint64))
    _, c, w = VP.pair(vd, p, pis)
    got = ver.pairs([p], [pis])
    assert np.array_equal(got[0, 0], VP.to_words(c)) and np.array_equal(got[0, 1], VP.to_words(w))


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_verify_accepts(S, name):
    _, _, ver, proof, pis = S.key[name]
    assert ver.verify(proof, pis, S.opening) is None


def test_verify_rejects(S, plk):
    from dusk_plonk_amd.prover import PlonkKey, VerificationError
    _, vd, ver, proof, pis = S.key["fixed_base"]
    bad = {
        "evaluation": (copy_proof(proof, c_eval=(proof.c_eval + 1) % R), pis),
        "public input": (proof, [pis[0], (pis[1] + 1) % R] + pis[2:]),
        "swapped commitments": (copy_proof(proof, a_comm=proof.b_comm, b_comm=proof.a_comm), pis),
    }
    cs = build(CIRCUITS["fixed_base"])
    other, _ = PlonkKey.compile_composer(S.pp, b"another key", cs)
    bad["another key"] = (other.prove_composer(cs, 5)[0], pis)
    for what, (p, pi) in bad.items():
        with pytest.raises(VerificationError, match="PairingCheckFailure"):
            ver.verify(p, pi, S.opening)
        assert list(ver.verify_each([p], [pi], S.opening)) == [False], what


def noncanonical(proof):
    from dusk_plonk_amd.prover import Proof
    raw = np.frombuffer(proof.raw_bytes(), dtype=np.uint64)
    comms, evals = raw[: 11 * 13].reshape(11, 13).copy(), raw[11 * 13:].reshape(16, 4).copy()
    evals[6] = np.array(P.int_to_limbs(R, 4), dtype=np.uint64)  # d_next_eval = r
    return Proof.from_words(comms, evals)


def off_curve(proof):
    from dusk_plonk_amd.prover import Proof
    raw = np.frombuffer(proof.raw_bytes(), dtype=np.uint64)
    comms, evals = raw[: 11 * 13].reshape(11, 13).copy(), raw[11 * 13:].reshape(16, 4).copy()
    comms[4, 6] ^= np.uint64(1)  # z_comm leaves the curve
    return Proof.from_words(comms, evals)


def test_malformed_input_is_an_error_not_a_verdict(S, plk):
    _, _, ver, proof, pis = S.key["ranged"]
    for spoil in (noncanonical, off_curve):
        p = spoil(proof)
        for call in (lambda: ver.verify(p, pis, S.opening),
                     lambda: ver.verify_batch([proof, p], [pis, pis], S.opening),
                     lambda: ver.verify_each([proof, p], [pis, pis], S.opening),
                     lambda: ver.pairs([p, proof], [pis, pis])):
            with pytest.raises(plk.PlonkError) as err:
                call()
            assert err.value.status == plk.PLK_E_ARG


def test_verify_batch(S):
    ver = S.key["public_sum"][2]
    assert ver.verify_batch(S.proofs, S.pis, S.opening) is True
    assert ver.verify_batch(S.spoiled([40]), S.pis, S.opening) is False


@pytest.mark.parametrize("replay", ["host", "device"])
def test_verify_each(S, replay):
    ver = S.key["public_sum"][2]
    ver.set_replay(replay)
    try:
        good = ver.verify_each(S.proofs, S.pis, S.opening)
        got = ver.verify_each(S.spoiled(BAD), S.pis, S.opening)
    finally:
        ver.set_replay("host")
    assert good.dtype == bool and good.all() and good.shape == (COUNT,)
    assert [j for j in range(COUNT) if not got[j]] == BAD


def test_verify_each_of_one_agrees_with_verify(S):
    from dusk_plonk_amd.prover import VerificationError
    ver = S.key["public_sum"][2]
    for proofs in (S.proofs, S.spoiled([0])):
        each = bool(ver.verify_each(proofs[:1], S.pis[:1], S.opening)[0])
        try:
            ver.verify(proofs[0], S.pis[0], S.opening)
            whole = True
        except VerificationError:
            whole = False
        assert each == whole
    assert bool(ver.verify_each(S.proofs[:1], S.pis[:1], S.opening)[0])
