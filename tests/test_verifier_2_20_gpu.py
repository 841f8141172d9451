"""The verifier on the GPU at n = 2^20, on a proof it did not make: the C oracle's proof of the
bench circuit (tests/golden/proof_2_20.npz: key commitments, proof, one public input at index
n - 9), built exactly as tests/test_verifier_cpu.py's fixture. No SRS and no prover: the
domain enters the verifier through log_n (the z^n squarings on host and device) and through
pi_winv = omega^-index only. Every other GPU verifier test has n <= 512 and proofs of the GPU
prover's own.

The restated pair costs the same at 2^20 as at n = 8 (the domain enters through pow); it is
called four times in all.
"""
import numpy as np
import pytest

import pyref as P
import tamper
import verifier_pair as VP
from test_verifier_cpu import fixture  # noqa: F401  (the module fixture, reused)
from test_verifier_gpu import holds

pytestmark = pytest.mark.gpu

R = P.R_MOD


@pytest.fixture(scope="module")
def G(plk, gpu_ctx, fixture):  # noqa: F811
    vd, proof, pis, tau, _ = fixture
    assert vd.n == 1 << 20 and list(vd.pi_indexes) == [vd.n - 9] and len(pis) == 1 and pis[0]
    ch, c, w = VP.pair(vd, proof, pis)
    bad = {
        0: (VP.copy_proof(proof, d_next_eval=(proof.d_next_eval + 1) % R), pis),
        63: (proof, [(pis[0] + 1) % R]),
        64: (VP.copy_proof(proof, t_4_comm=tamper.plus_g(proof.t_4_comm)), pis),
    }
    for j, (p, pi) in bad.items():  # the reference's word: each of the three is rejected
        assert not VP.accepts(vd, p, pi, tau), j
    return vd, vd.verifier(), proof, pis, tau, (ch, c, w), bad, plk.OpeningKey.setup(tau)


@pytest.mark.parametrize("replay", ["host", "device"])
def test_golden_proof_folds_and_verifies(G, replay):
    vd, ver, proof, pis, tau, (ch, c, w), _, opening = G
    ver.set_replay(replay)
    try:
        assert ver.challenges_batch([proof], [pis]) == [ver.challenges(proof, pis)] == [ch]
        got_c, got_w = ver.fold([proof], [pis], [1])
        assert ver.verify(proof, pis, opening) is None
    finally:
        ver.set_replay("host")
    assert np.array_equal(got_c, VP.to_words(c)) and np.array_equal(got_w, VP.to_words(w))
    assert holds(got_c, got_w, tau)


@pytest.mark.parametrize("replay", ["host", "device"])
def test_batch_of_65_with_three_bad_proofs(G, replay):
    vd, ver, proof, pis, tau, _, bad, opening = G
    proofs, pil = [proof] * 65, [list(pis) for _ in range(65)]
    for j, (p, pi) in bad.items():
        proofs[j], pil[j] = p, pi
    good = [j for j in range(65) if j not in bad]
    assert len(good) == 62
    ver.set_replay(replay)
    try:
        each = ver.verify_each(proofs, pil, opening)
        whole = ver.verify_batch(proofs, pil, opening)
        rest = ver.verify_batch([proofs[j] for j in good], [pil[j] for j in good], opening)
    finally:
        ver.set_replay("host")
    assert [j for j in range(65) if not each[j]] == sorted(bad)
    assert whole is False and rest is True
