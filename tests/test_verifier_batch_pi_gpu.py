"""Batches whose proofs each carry several public inputs of their own: the per-proof stride of
the public inputs (replay_host_batch's `public_inputs + j * npi`, k_replay_prep's and
replay_mid's `npi * j + i`, the item / proof split of k_replay_prep's thread index, the Python
packing of the list of lists) and the skip of zero inputs across lanes (the host's den[k++]
compaction, the device's per-lane test), in both replay modes.

Two keys, proofs from the GPU prover:
* five inputs then a chain of 20 gates (label b"pi", n = 32), 130 proofs; proof j takes pattern
  j % 7 of PATTERNS (all non-zero, all zero, first zero, last zero, two adjacent zeros, only the
  middle one non-zero, all r - 1) with values that depend on j;
* chain_40_public's shape (40 inputs, n = 128), 66 proofs with per-proof values and per-proof
  zero positions.
Every proof's single fold (count = 1, weight 1) is the reference here; it is pinned against the
restated pair on one proof of each pattern.

Cross-talk cases: one proof's inputs are changed and exactly that proof must fail. Proof 64
takes proof 65's inputs; in proof 33 a non-zero input moves one position down onto a zero and
leaves a zero behind (only the positions of a zero and a non-zero change); in the first proof
that has one (proof 0 of the 40-input key, proof 1 of the five-input key, whose proof 0 is the
all-non-zero pattern) a zero input becomes 1.
"""
import numpy as np
import pytest

import pyref as P
import verifier_pair as VP
from test_prover_oracle import build, tau_for
from test_verifier_gpu import holds, pts

pytestmark = pytest.mark.gpu

R = P.R_MOD
PATTERNS = ("all non-zero", "all zero", "first zero", "last zero", "two adjacent zeros",
            "only the middle non-zero", "all r - 1")


def inputs_5(j):
    v = [1000 * j + 10 * i + 1 for i in range(5)]
    zero = {0: [], 1: [0, 1, 2, 3, 4], 2: [0], 3: [4], 4: [2, 3], 5: [0, 1, 3, 4]}
    if j % 7 == 6:
        return [R - 1] * 5
    return [0 if i in zero[j % 7] else x for i, x in enumerate(v)]


def inputs_40(j):
    """Values and zero positions of their own: one zero at 7j mod 40, for odd j two more at
    3j + 1 and 3j + 2 mod 40 (adjacent), for j = 5 mod 8 the last one as well."""
    v = [100000 * (j + 1) + 37 * i + 1 for i in range(40)]
    zero = {7 * j % 40}
    if j % 2:
        zero |= {(3 * j + 1) % 40, (3 * j + 2) % 40}
    if j % 8 == 5:
        zero.add(39)
    return [0 if i in zero else x for i, x in enumerate(v)]


def circuit(values, chain_gates, seed):
    def f(cs):
        for v in values:
            cs.append_public(-v % R)  # the public input of append_public(x) is -x
        cs.synthetic_chain(chain_gates, seed)
    return f


KEYS = {"five": (inputs_5, 20, 130, 32), "forty": (inputs_40, 50, 66, 128)}


class Batch:
    def __init__(self, plk, pp, tau, which):
        from dusk_plonk_amd.prover import PlonkKey
        inputs, gates, count, n = KEYS[which]
        first = [1 + i for i in range(len(inputs(0)))]  # compiled from an all-non-zero vector
        self.prover, self.vd = PlonkKey.compile_composer(pp, b"pi", build(circuit(first, gates, 3)))
        assert self.vd.n == n and len(self.vd.pi_indexes) == len(first)
        self.ver, self.tau, self.count = self.vd.verifier(), tau, count
        self.proofs, self.pis = [], []
        for j in range(count):
            p, pi = self.prover.prove_composer(build(circuit(inputs(j), gates, 100 + j)), 500 + j)
            assert pi == [x % R for x in inputs(j)]
            self.proofs.append(p)
            self.pis.append(pi)
        self.singles = np.stack([np.stack(self.ver.fold([p], [pi], [1]))
                                 for p, pi in zip(self.proofs, self.pis)])
        self.challenges = [self.ver.challenges(p, pi) for p, pi in zip(self.proofs, self.pis)]
        rng = np.random.Generator(np.random.PCG64(31))
        self.weights = [int.from_bytes(rng.bytes(16), "little") for _ in range(count)]

    def cross_talk(self):
        """name -> (index, that proof's changed inputs)."""
        out = {"inputs of the next proof": (64, list(self.pis[65]))}
        pi = list(self.pis[33])
        i = next(i for i in range(1, len(pi)) if pi[i] and not pi[i - 1])
        pi[i - 1], pi[i] = pi[i], 0
        out["a zero and a non-zero trade places"] = (33, pi)
        j = next(j for j in range(self.count) if 0 in self.pis[j])
        pi = list(self.pis[j])
        pi[pi.index(0)] = 1
        out["a zero becomes 1"] = (j, pi)
        return out


@pytest.fixture(scope="module")
def B(plk, gpu_ctx):
    tau_limbs, tau = tau_for(0xB17C)
    pp = plk.PlonkParams.setup(7, tau_limbs)
    opening = plk.OpeningKey.setup(tau)
    return {which: Batch(plk, pp, tau, which) for which in KEYS}, opening


def test_input_vectors_are_what_the_cases_need(B):
    five, forty = B[0]["five"], B[0]["forty"]
    assert [five.pis[j].count(0) for j in range(7)] == [0, 5, 1, 1, 2, 4, 0]
    assert five.pis[6] == [R - 1] * 5 and five.pis[4][2:4] == [0, 0] and five.pis[5][2] != 0
    distinct = {tuple(pi) for pi in five.pis}
    # all-zero and all r - 1 cannot differ between proofs; every other vector is its proof's own
    same = [sum(1 for j in range(130) if j % 7 == k) for k in (1, 6)]
    assert len(distinct) == 130 - (same[0] - 1) - (same[1] - 1)
    assert len({tuple(pi) for pi in forty.pis}) == 66
    # 7j mod 40 takes all 40 positions over j < 40; proofs 40 .. 65 repeat positions, not values
    assert len({tuple(i for i, x in enumerate(pi) if x == 0) for pi in forty.pis}) == 40
    assert forty.pis[0][0] == 0 and five.pis[0].count(0) == 0 and 0 in five.pis[1]
    for b in (five, forty):
        assert b.pis[64] != b.pis[65]
        assert sorted(j for j, _ in b.cross_talk().values()) == [0 if b is forty else 1, 33, 64]


@pytest.mark.parametrize("which", list(KEYS))
def test_single_folds_equal_the_restated_pair(B, which):
    """One proof of each of the seven patterns (proofs 0 .. 6 of either key)."""
    b = B[0][which]
    for j in range(7):
        ch, c, w = VP.pair(b.vd, b.proofs[j], b.pis[j])
        assert b.challenges[j] == ch, j
        assert np.array_equal(b.singles[j, 0], VP.to_words(c)), j
        assert np.array_equal(b.singles[j, 1], VP.to_words(w)), j
        assert holds(b.singles[j, 0], b.singles[j, 1], b.tau), j


@pytest.mark.parametrize("which", list(KEYS))
def test_challenges_batch_equals_the_single_challenges(B, which):
    b = B[0][which]
    for count in (1, 63, 64, 65, b.count):
        assert b.ver.challenges_batch(b.proofs[:count], b.pis[:count]) == b.challenges[:count], count


@pytest.mark.parametrize("which", list(KEYS))
def test_fold_equals_the_weighted_single_folds(B, plk, which):
    b = B[0][which]
    host = b.ver.fold(b.proofs, b.pis, b.weights, replay="host")
    dev = b.ver.fold(b.proofs, b.pis, b.weights, replay="device")
    for k in (0, 1):
        terms = [P.g1_mul(pts(s[k]), rho) for s, rho in zip(b.singles, b.weights)]
        assert np.array_equal(host[k], plk.g1_sum(P.g1_vec_to_np(terms)).words)
        assert np.array_equal(dev[k], host[k])
    assert holds(*host, b.tau)


@pytest.mark.parametrize("replay", ["host", "device"])
@pytest.mark.parametrize("which", list(KEYS))
def test_pairs_and_verdicts(B, which, replay):
    b, opening = B[0][which], B[1]
    b.ver.set_replay(replay)
    try:
        pairs = b.ver.pairs(b.proofs, b.pis)
        each = b.ver.verify_each(b.proofs, b.pis, opening)
        whole = b.ver.verify_batch(b.proofs, b.pis, opening)
    finally:
        b.ver.set_replay("host")
    for j in range(b.count):
        assert np.array_equal(pairs[j], b.singles[j]), j
    assert each.all() and each.shape == (b.count,)
    assert whole is True


@pytest.mark.parametrize("replay", ["host", "device"])
@pytest.mark.parametrize("which", list(KEYS))
def test_cross_talk(B, which, replay):
    b, opening = B[0][which], B[1]
    for what, (at, pi) in b.cross_talk().items():
        assert pi != b.pis[at]
        pis = list(b.pis)
        pis[at] = pi
        b.ver.set_replay(replay)
        try:
            each = b.ver.verify_each(b.proofs, pis, opening)
            fold = b.ver.fold(b.proofs, pis, b.weights)
        finally:
            b.ver.set_replay("host")
        assert [j for j in range(b.count) if not each[j]] == [at], what
        assert not holds(*fold, b.tau), what
