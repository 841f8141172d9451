"""The verifier on the GPU (plk_verifier_fold, csrc/verifier.hip + csrc/msm_var.hip) against the
restated verifier's KZG pair (tests/verifier_pair.py), bit-exact, on proofs the GPU prover makes:
every widget's linearisation (arithmetic, range, logic, fixed-base, variable-base), circuits
with none, one, four and forty public inputs (one of them zero), identity key commitments.

The pairing is not part of the product; the tests know the SRS trapdoor tau and check the final
equation e(C, H) == e(W, [tau]H) as C == tau W in G1 (tests/verifier.py's device).
"""
import numpy as np
import pytest

import g1_ingest_ref as ref
import pyref as P
import verifier_pair as VP
from verifier_pair import copy_proof
from test_prover_oracle import CASES, build, tau_for

pytestmark = pytest.mark.gpu

R = P.R_MOD


def case(name):
    return next(c[1] for c in CASES if c[0] == name)


def chain_40_public(cs):
    """A chain circuit with 40 public inputs, one of them zero."""
    for i in range(40):
        cs.append_public(0 if i == 7 else 1000 + i)
    cs.synthetic_chain(50, 3)


def public_sum_j(j):
    from test_prover_oracle import public_sum
    return public_sum(10 + j, 20 + 3 * j, 30 + 4 * j)


CIRCUITS = {
    "boolean": case("boolean1"),               # n = 8, no public input
    "public_sum": case("public_sum"),          # one public input
    "ranged": case("range_full_254"),          # n = 64, the range widget
    "logic": case("and_30"),                   # the logic widget
    "fixed_base": case("test_circuit_20_5"),   # fixed-base scalar mul, range, 4 public inputs
    "variable_base": case("add_point"),        # variable-base addition
    "chain_40_public": chain_40_public,
}


class Setup:
    """One SRS for every circuit; per circuit the key, the verifier and one proof."""

    def __init__(self, plk):
        from dusk_plonk_amd.prover import PlonkKey
        self.tau_limbs, self.tau = tau_for(0xF01D)
        self.pp = plk.PlonkParams.setup(9, self.tau_limbs)
        self.key = {}
        for name, fn in CIRCUITS.items():
            cs = build(fn)
            prover, vd = PlonkKey.compile_composer(self.pp, b"fold", cs)
            proof, pis = prover.prove_composer(cs, 40 + len(self.key))
            self.key[name] = (prover, vd, vd.verifier(), proof, pis)
        self._batch = None

    def batch(self):
        """257 proofs of the public_sum circuit with their own witnesses and public inputs,
        each one's single fold (count = 1, weight 1) and 128-bit weights."""
        if self._batch is None:
            prover, vd, ver, _, _ = self.key["public_sum"]
            proofs, pis = [], []
            for j in range(257):
                p, pi = prover.prove_composer(build(public_sum_j(j)), 1000 + j)
                proofs.append(p)
                pis.append(pi)
            singles = [ver.fold([p], [pi], [1]) for p, pi in zip(proofs, pis)]
            rng = np.random.Generator(np.random.PCG64(9))
            weights = [int.from_bytes(rng.bytes(16), "little") for _ in range(257)]
            self._batch = (proofs, pis, singles, weights)
        return self._batch


@pytest.fixture(scope="module")
def S(plk, gpu_ctx):
    return Setup(plk)


def pts(words):
    return P.g1_vec_from_np(np.asarray(words, dtype=np.uint64).reshape(1, 13))[0]


def holds(c_words, w_words, tau):
    """The final KZG equation with the trapdoor: C == tau W."""
    return pts(c_words) == P.g1_mul(pts(w_words), tau)


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_single_fold_equals_the_restated_pair(S, name):
    """count = 1, weight 1: (C, W) is exactly batch_check's pair, and it satisfies the
    equation. This pins what the caller feeds to the pairing."""
    _, vd, ver, proof, pis = S.key[name]
    ch, c, w = VP.pair(vd, proof, pis)
    assert ver.challenges(proof, pis) == ch
    got_c, got_w = ver.fold([proof], [pis], [1])
    assert np.array_equal(got_c, VP.to_words(c))
    assert np.array_equal(got_w, VP.to_words(w))
    assert holds(got_c, got_w, S.tau)


def test_rejects(S, plk):
    from dusk_plonk_amd.prover import PlonkKey
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
        c, w = ver.fold([p], [pi], [1])
        _, want_c, want_w = VP.pair(vd, p, pi)
        assert np.array_equal(c, VP.to_words(want_c)) and np.array_equal(w, VP.to_words(want_w)), what
        assert not holds(c, w, S.tau), what


def weighted(pairs, weights):
    """sum_j rho_j (C_j, W_j) in Python from pyref points."""
    c = w = None
    for (pc, pw), rho in zip(pairs, weights):
        c = P.g1_add(c, P.g1_mul(pc, rho % R))
        w = P.g1_add(w, P.g1_mul(pw, rho % R))
    return c, w


def test_five_proofs_explicit_weights(S):
    """Five proofs of one circuit (own witnesses, own public inputs): sum_j rho_j (pair_j)."""
    prover, vd, ver, _, _ = S.key["public_sum"]
    proofs, pis = [], []
    for j in range(5):
        p, pi = prover.prove_composer(build(public_sum_j(j)), 70 + j)
        proofs.append(p)
        pis.append(pi)
    weights = [1, R - 1, (R - 1) // 2, 0x1234567890ABCDEF, 3 ** 150 % R]
    want = weighted([VP.pair(vd, p, pi)[1:] for p, pi in zip(proofs, pis)], weights)
    c, w = ver.fold(proofs, pis, weights)
    assert np.array_equal(c, VP.to_words(want[0])) and np.array_equal(w, VP.to_words(want[1]))
    assert holds(c, w, S.tau)


@pytest.mark.parametrize("count", [64, 257])
def test_batch_equals_weighted_single_folds(S, plk, count):
    proofs, pis, singles, weights = S.batch()
    proofs, pis, singles, weights = proofs[:count], pis[:count], singles[:count], weights[:count]
    c, w = S.key["public_sum"][2].fold(proofs, pis, weights)
    for got, k in ((c, 0), (w, 1)):
        terms = [P.g1_mul(pts(s[k]), rho) for s, rho in zip(singles, weights)]
        assert np.array_equal(got, plk.g1_sum(P.g1_vec_to_np(terms)).words)
    assert holds(c, w, S.tau)


@pytest.mark.parametrize("count", [64, 257])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_bad_proof_fails_the_batch(S, count, where):
    proofs, pis, _, weights = S.batch()
    proofs, pis, weights = list(proofs[:count]), pis[:count], weights[:count]
    at = {"first": 0, "middle": count // 2, "last": count - 1}[where]
    proofs[at] = copy_proof(proofs[at], d_eval=(proofs[at].d_eval + 1) % R)
    c, w = S.key["public_sum"][2].fold(proofs, pis, weights)
    assert not holds(c, w, S.tau)


def test_random_weights(S):
    proofs, pis, _, _ = S.batch()
    proofs, pis = list(proofs[:16]), pis[:16]
    ver = S.key["public_sum"][2]
    a = ver.fold(proofs, pis)
    b = ver.fold(proofs, pis)
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
    assert holds(*a, S.tau) and holds(*b, S.tau)
    proofs[9] = copy_proof(proofs[9], a_eval=(proofs[9].a_eval + 1) % R)
    assert not holds(*ver.fold(proofs, pis), S.tau)


def test_argument_checks(S, plk):
    from dusk_plonk_amd.prover import Proof
    _, vd, ver, proof, pis = S.key["ranged"]
    raw = np.frombuffer(proof.raw_bytes(), dtype=np.uint64)
    comms, evals = raw[: 11 * 13].reshape(11, 13).copy(), raw[11 * 13:].reshape(16, 4).copy()
    r_limbs = np.array(P.int_to_limbs(R, 4), dtype=np.uint64)
    e = evals.copy()
    e[6] = r_limbs  # d_next_eval = r: not canonical
    with pytest.raises(plk.PlonkError) as err:
        ver.fold([Proof.from_words(comms, e)], [pis], [1])
    assert err.value.status == plk.PLK_E_ARG
    with pytest.raises(plk.PlonkError) as err:
        ver.challenges(Proof.from_words(comms, e), pis)
    assert err.value.status == plk.PLK_E_ARG
    c = comms.copy()
    c[4, 6] ^= np.uint64(1)  # z_comm leaves the curve
    with pytest.raises(plk.PlonkError) as err:
        ver.fold([Proof.from_words(c, evals)], [pis], [1])
    assert err.value.status == plk.PLK_E_ARG
    with pytest.raises(plk.PlonkError) as err:
        ver.fold([proof], [pis], [r_limbs])  # weight r as raw limbs
    assert err.value.status == plk.PLK_E_ARG
    with pytest.raises(plk.PlonkError) as err:
        ver.fold([], [])
    assert err.value.status == plk.PLK_E_ARG


def test_identity_commitments_are_legal(S):
    """An identity w_z_chall_w_comm is an argument like any other (the pair is the helper's);
    the boolean circuit's key holds identity selector commitments (unused widgets)."""
    _, vd, ver, proof, pis = S.key["boolean"]
    assert any(int(c[12]) for c in vd.comms)
    identity = np.array([0] * 12 + [1], dtype=np.uint64)
    p = copy_proof(proof, w_z_chall_w_comm=identity)
    _, c, w = VP.pair(vd, p, pis)
    got_c, got_w = ver.fold([p], [pis], [1])
    assert np.array_equal(got_c, VP.to_words(c)) and np.array_equal(got_w, VP.to_words(w))


# ---- the plk_g1 input rules of plk_verifier_pairs, through one tampered commitment -------------
@pytest.mark.parametrize("lane", ref.ABI_LANES)
@pytest.mark.parametrize("what", ref.ABI_REFUSED)
def test_pairs_refuse_a_malformed_commitment(S, plk, what, lane):
    proofs, pis, _, _ = S.batch()
    proofs, pis = list(proofs[:65]), pis[:65]
    proofs[lane] = copy_proof(proofs[lane], z_comm=ref.abi_spoil(proofs[lane].z_comm, what))
    with pytest.raises(plk.PlonkError) as err:
        S.key["public_sum"][2].pairs(proofs, pis)
    assert err.value.status == plk.PLK_E_ARG


@pytest.mark.parametrize("replay", ["host", "device"])
@pytest.mark.parametrize("lane", ref.ABI_LANES)
def test_pairs_identity_word_hides_the_coordinates(S, lane, replay):
    """An identity commitment over arbitrary coordinate words gives the pair of the identity."""
    proofs, pis, _, _ = S.batch()
    proofs, pis = list(proofs[:65]), pis[:65]
    _, vd, ver, _, _ = S.key["public_sum"]
    garbage = ref.abi_spoil(proofs[lane].w_z_chall_w_comm, ref.ABI_IDENTITY)
    clean = copy_proof(proofs[lane], w_z_chall_w_comm=np.array([0] * 12 + [1], dtype=np.uint64))
    proofs[lane] = copy_proof(proofs[lane], w_z_chall_w_comm=garbage)
    _, c, w = VP.pair(vd, clean, pis[lane])
    ver.set_replay(replay)
    try:
        got = ver.pairs(proofs, pis)
    finally:
        ver.set_replay("host")
    assert np.array_equal(got[lane, 0], VP.to_words(c)) and np.array_equal(got[lane, 1], VP.to_words(w))
