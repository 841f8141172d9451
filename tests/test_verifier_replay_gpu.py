"""The verifier's transcript replay on the GPU (csrc/verifier_replay.hip, PLK_REPLAY_DEVICE)
against the host replay, which stays the contract: the challenges of every proof exactly, the
folded pair byte for byte with explicit weights, the per-proof random weights, the argument
checks. Shapes, circuits and proofs are tests/test_verifier_gpu.py's.

The z = 1 and z_h(z) = 0 refusals cannot be reached through the API (z is a hash output); the
device check stands next to the host's wording in replay_mid and only reading covers it.
"""
import numpy as np
import pytest

import pyref as P
import verifier_pair as VP
from verifier_pair import copy_proof
from test_prover_oracle import build
from test_verifier_gpu import CIRCUITS, Setup, holds, public_sum_j, weighted
from test_verifier_replay import fold_weights

pytestmark = pytest.mark.gpu

R = P.R_MOD


@pytest.fixture(scope="module")
def S(plk, gpu_ctx):
    return Setup(plk)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 1. the challenges ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CIRCUITS))
def test_challenges_batch_every_circuit(S, name):
    """None, 1, 4 and 40 public inputs (one zero), identity key commitments, n = 8 .. 512."""
    _, vd, ver, proof, pis = S.key[name]
    assert ver.challenges_batch([proof], [pis]) == [ver.challenges(proof, pis)]
    identity = np.array([0] * 12 + [1], dtype=np.uint64)
    p = copy_proof(proof, w_z_chall_w_comm=identity, t_4_comm=identity)
    assert ver.challenges_batch([proof, p], [pis, pis]) == [ver.challenges(proof, pis),
                                                            ver.challenges(p, pis)]


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_challenges_batch_wave_edges(S, count):
    proofs, pis, _, _ = S.batch()
    ver = S.key["public_sum"][2]
    want = [ver.challenges(p, pi) for p, pi in zip(proofs[:count], pis[:count])]
    assert ver.challenges_batch(proofs[:count], pis[:count]) == want


# ---- 2. sponge alignment --------------------------------------------------------------------
def _variants(vd):
    from dusk_plonk_amd.prover import VerifierData
    for k in (1, 5, 160, 165, 166, 167, 400):
        yield f"label of {k}", VerifierData(bytes(97 + i % 26 for i in range(k)), vd.n, vd.m,
                                            vd.comms, vd.pi_indexes)
    for m in (vd.m + 1, (1 << 40) + 12345):
        yield f"m = {m}", VerifierData(vd.label, vd.n, m, vd.comms, vd.pi_indexes)


@pytest.mark.parametrize("name", ["chain_40_public", "public_sum"])
def test_sponge_alignment(S, name):
    """Another label length or m moves the base position across the 166-byte rate and with it
    every slot of the schedule. The proofs need not verify under such a verifier."""
    _, vd, _, proof, pis = S.key[name]
    proofs, pis_l = [proof], [pis]
    if name == "public_sum":
        bp, bpi, _, _ = S.batch()
        proofs, pis_l = proofs + bp[:2], pis_l + bpi[:2]
    seen = set()
    for what, vd2 in _variants(vd):
        ver = vd2.verifier()
        want = [ver.challenges(p, pi) for p, pi in zip(proofs, pis_l)]
        assert ver.challenges_batch(proofs, pis_l) == want, what
        seen.add(tuple(want[0]))
    assert len(seen) == 9


# ---- 3. the fold, explicit weights ----------------------------------------------------------
@pytest.mark.parametrize("name", list(CIRCUITS))
def test_single_fold_device_equals_host_and_the_restated_pair(S, name):
    _, vd, ver, proof, pis = S.key[name]
    _, c, w = VP.pair(vd, proof, pis)
    dev = ver.fold([proof], [pis], [1], replay="device")
    assert ver.replay == "host"
    assert same(dev, ver.fold([proof], [pis], [1]))
    assert np.array_equal(dev[0], VP.to_words(c)) and np.array_equal(dev[1], VP.to_words(w))
    assert holds(*dev, S.tau)


def test_five_proofs_explicit_weights_device(S):
    prover, vd, ver, _, _ = S.key["public_sum"]
    proofs, pis = [], []
    for j in range(5):
        p, pi = prover.prove_composer(build(public_sum_j(j)), 70 + j)
        proofs.append(p)
        pis.append(pi)
    weights = [1, R - 1, (R - 1) // 2, 0x1234567890ABCDEF, 3 ** 150 % R]
    dev = ver.fold(proofs, pis, weights, replay="device")
    assert same(dev, ver.fold(proofs, pis, weights))
    want = weighted([VP.pair(vd, p, pi)[1:] for p, pi in zip(proofs, pis)], weights)
    assert np.array_equal(dev[0], VP.to_words(want[0])) and np.array_equal(dev[1], VP.to_words(want[1]))
    assert holds(*dev, S.tau)


@pytest.mark.parametrize("count", [64, 257])
def test_batch_device_equals_host(S, count):
    proofs, pis, _, weights = S.batch()
    ver = S.key["public_sum"][2]
    dev = ver.fold(proofs[:count], pis[:count], weights[:count], replay="device")
    assert same(dev, ver.fold(proofs[:count], pis[:count], weights[:count]))
    assert holds(*dev, S.tau)


# ---- 4. one bad proof -----------------------------------------------------------------------
@pytest.mark.parametrize("count", [64, 257])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_bad_proof_fails_the_device_fold(S, count, where):
    proofs, pis, _, weights = S.batch()
    proofs, pis, weights = list(proofs[:count]), pis[:count], weights[:count]
    at = {"first": 0, "middle": count // 2, "last": count - 1}[where]
    proofs[at] = copy_proof(proofs[at], d_eval=(proofs[at].d_eval + 1) % R)
    ver = S.key["public_sum"][2]
    assert not holds(*ver.fold(proofs, pis, weights, replay="device"), S.tau)
    assert not holds(*ver.fold(proofs, pis, replay="device"), S.tau)  # a zero or dropped rho_j


# ---- 5. random weights ----------------------------------------------------------------------
def test_random_weights_device(S):
    proofs, pis, _, _ = S.batch()
    proofs, pis = list(proofs[:16]), pis[:16]
    ver = S.key["public_sum"][2]
    a = ver.fold(proofs, pis, replay="device")
    b = ver.fold(proofs, pis, replay="device")
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
    assert holds(*a, S.tau) and holds(*b, S.tau)
    proofs[9] = copy_proof(proofs[9], a_eval=(proofs[9].a_eval + 1) % R)
    assert not holds(*ver.fold(proofs, pis, replay="device"), S.tau)


# ---- 6. the weights kernel ------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 64, 65, 257])
def test_fold_weights_device_equals_host_mirror(plk, gpu_ctx, count):
    entropy = bytes((11 * i + count) % 256 for i in range(32))
    u = [pow(7, 500 + 13 * j + count, R) for j in range(count)]
    assert fold_weights(plk, gpu_ctx.handle, entropy, u) == fold_weights(plk, None, entropy, u)


# ---- 7. argument checks ---------------------------------------------------------------------
def test_argument_checks_device(S, plk):
    from dusk_plonk_amd.prover import Proof
    _, vd, ver, proof, pis = S.key["ranged"]
    _, _, ver4, proof4, pis4 = S.key["fixed_base"]
    raw = np.frombuffer(proof.raw_bytes(), dtype=np.uint64)
    comms, evals = raw[: 11 * 13].reshape(11, 13).copy(), raw[11 * 13:].reshape(16, 4).copy()
    r_limbs = np.array(P.int_to_limbs(R, 4), dtype=np.uint64)
    e = evals.copy()
    e[6] = r_limbs  # d_next_eval = r: not canonical
    c = comms.copy()
    c[4, 6] ^= np.uint64(1)  # z_comm leaves the curve
    bad_pi = [pis4[0], r_limbs] + list(pis4[2:])
    for what, call in {
        "evaluation": lambda: ver.fold([Proof.from_words(comms, e)], [pis], [1], replay="device"),
        "evaluation, batch": lambda: ver.challenges_batch([Proof.from_words(comms, e)], [pis]),
        "public input": lambda: ver4.fold([proof4], [bad_pi], [1], replay="device"),
        "public input, batch": lambda: ver4.challenges_batch([proof4], [bad_pi]),
        "off-curve z_comm": lambda: ver.fold([Proof.from_words(c, evals)], [pis], [1], replay="device"),
        "weight": lambda: ver.fold([proof], [pis], [r_limbs], replay="device"),
        "count = 0": lambda: ver.fold([], [], replay="device"),
        "count = 0, batch": lambda: ver.challenges_batch([], []),
        "mode": lambda: ver.fold([proof], [pis], [1], replay=2),
    }.items():
        with pytest.raises(plk.PlonkError) as err:
            call()
        assert err.value.status == plk.PLK_E_ARG, what
    assert ver.replay == "host"
    assert holds(*ver.fold([proof], [pis], [1], replay="device"), S.tau)  # and works afterwards


# ---- 8. the kernel time ---------------------------------------------------------------------
def test_last_replay_ms(S):
    _, _, ver, proof, pis = S.key["logic"]
    ver.fold([proof], [pis], [1], replay="device")
    assert ver.last_replay_ms() > 0
    ver.fold([proof], [pis], [1])
    assert ver.last_replay_ms() == 0
    ver.challenges_batch([proof], [pis])
    assert ver.last_replay_ms() > 0
