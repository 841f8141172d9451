"""The verifier on the GPU under the full single-field tamper sweep of tests/tamper.py, in both
replay modes, on the seven circuits of tests/test_verifier_gpu.py.

What a verdict must be is the restated verifier's word, tests/test_verifier_soundness.py (CPU):
every variant is rejected. Here one batch per circuit holds the honest proof at indices 0, 32 and
last with every variant between them (68 proofs and more: past the 64-pair block of k_pairing
and many 4-proof blocks of k_proof_pairs); the per-proof verdicts must be True exactly at the
honest indices, the batch verdict False, and every row of pairs() the proof's own single fold.
No call may raise: an identity commitment is an argument, not an error. The restated pair is
called directly on one row of each variant kind only; the single folds are pinned against it by
tests/test_verifier_gpu.py.

Key variants (tamper.key_variants): a verifier made from a key with one thing changed refuses
the honest proof; across the seven circuits every one of the 15 key commitments has its +G
pair compared with the restated pair under the same changed key.
"""
import numpy as np
import pytest

import tamper
import verifier_pair as VP
from test_verifier_gpu import CIRCUITS, Setup

pytestmark = pytest.mark.gpu

NAMES = list(CIRCUITS)


class SweepSetup(Setup):
    def __init__(self, plk):
        super().__init__(plk)
        self.opening = plk.OpeningKey.setup(self.tau)
        self._sweep = {}

    def sweep(self, name):
        """(names, proofs, pis, honest indices, single folds uint64[count, 2, 13]) of one
        circuit's batch; names[j] is None at the honest indices."""
        if name not in self._sweep:
            _, _, ver, proof, pis = self.key[name]
            skipped = []
            items = list(tamper.variants(proof, pis, skipped))
            assert skipped == []
            npi = len(pis)
            assert len(items) == 32 + 33 + npi + (1 if npi >= 2 else 0)
            honest = (None, proof, list(pis))
            batch = [honest] + items[:31] + [honest] + items[31:] + [honest]
            names = [b[0] for b in batch]
            proofs, pil = [b[1] for b in batch], [b[2] for b in batch]
            at = [0, 32, len(batch) - 1]
            assert [j for j, n in enumerate(names) if n is None] == at and len(batch) >= 68
            singles = np.stack([np.stack(ver.fold([p], [pi], [1])) for p, pi in zip(proofs, pil)])
            self._sweep[name] = (names, proofs, pil, at, singles)
        return self._sweep[name]


@pytest.fixture(scope="module")
def S(plk, gpu_ctx):
    return SweepSetup(plk)


@pytest.mark.parametrize("replay", ["host", "device"])
@pytest.mark.parametrize("name", NAMES)
def test_sweep_in_one_batch(S, name, replay):
    _, _, ver, _, _ = S.key[name]
    names, proofs, pis, at, singles = S.sweep(name)
    ver.set_replay(replay)
    try:
        each = ver.verify_each(proofs, pis, S.opening)
        whole = ver.verify_batch(proofs, pis, S.opening)
        good = ver.verify_batch([proofs[j] for j in at], [pis[j] for j in at], S.opening)
        pairs = ver.pairs(proofs, pis)
        mine = np.stack([np.stack(ver.fold([p], [pi], [1])) for p, pi in zip(proofs, pis)])
    finally:
        ver.set_replay("host")
    accepted = [j for j in range(len(proofs)) if each[j]]
    assert accepted == at, [names[j] for j in set(accepted) ^ set(at)]
    assert whole is False and good is True
    for j in range(len(proofs)):
        assert np.array_equal(pairs[j], mine[j]), names[j]  # the single folds of this mode
        assert np.array_equal(mine[j], singles[j]), names[j]  # and of the host's


@pytest.mark.parametrize("name", NAMES)
def test_one_row_of_each_kind_equals_the_restated_pair(S, name):
    _, vd, _, _, _ = S.key[name]
    names, proofs, pis, _, singles = S.sweep(name)
    seen = set()
    for j, what in enumerate(names):
        k = tamper.kind(what) if what else None
        if k is None or k in seen:
            continue
        seen.add(k)
        _, c, w = VP.pair(vd, proofs[j], pis[j])
        assert np.array_equal(singles[j, 0], VP.to_words(c)), what
        assert np.array_equal(singles[j, 1], VP.to_words(w)), what
    npi = len(pis[0])
    assert seen == set(tamper.KINDS[: 5 if npi else 4])


@pytest.mark.parametrize("name", NAMES)
def test_changed_key_refuses_the_honest_proof(S, plk, name):
    from dusk_plonk_amd.prover import VerificationError
    _, vd, _, proof, pis = S.key[name]
    keys = list(tamper.key_variants(vd))
    assert len(keys) == 18 + (1 if pis else 0)
    for what, vd2 in keys:
        idx = list(vd2.pi_indexes)
        if any(b <= a for a, b in zip(idx, idx[1:])) or any(i >= vd2.n for i in idx):
            # Verifier::new takes strictly increasing indexes inside the domain only
            # (include/plk.h): an index moved onto its neighbour (chain_40_public) or past the
            # last row (public_sum) makes a key that is refused before any proof is seen
            assert what == "pi_index[0]+1"
            with pytest.raises(plk.PlonkError) as e:
                vd2.verifier()
            assert e.value.status == plk.PLK_E_ARG, what
            continue
        with pytest.raises(VerificationError, match="PairingCheckFailure"):
            vd2.verifier().verify(proof, pis, S.opening)
    # this circuit's share of the 15 key commitments: the +G pair is the restated pair's
    at = NAMES.index(name)
    mine = list(range(at, 15, len(NAMES)))
    assert sorted(sum((list(range(i, 15, len(NAMES))) for i in range(len(NAMES))), [])) == list(range(15))
    for i in mine:
        what, vd2 = keys[i]
        assert what.endswith("+G")
        _, c, w = VP.pair(vd2, proof, pis)
        got_c, got_w = vd2.verifier().fold([proof], [pis], [1])
        assert np.array_equal(got_c, VP.to_words(c)) and np.array_equal(got_w, VP.to_words(w)), what
