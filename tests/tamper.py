"""Single-field tamperings of a proof, its public inputs and a verifier key — TEST
INFRASTRUCTURE (no test in it).

`variants(proof, pis)` changes exactly one thing of a (proof, public inputs) pair at a time and
`key_variants(vd)` one thing of a VerifierData; a sound verifier rejects every one of them. The
sweeps of tests/test_verifier_soundness.py (the restated verifier, CPU) and
tests/test_verifier_soundness_gpu.py (the verifier on the GPU) walk them. A variant that would
equal the original (the negation or the identity replacement of an identity commitment, a swap
of two equal inputs) is not yielded: its name goes to the caller's `skipped` list, and the tests
assert that list is empty for the circuits they use, so a sweep cannot thin out unnoticed.

The proof may be a dusk_plonk_amd.prover.Proof or a test_prover_oracle.OracleProof: commitments
are uint64[13] ABI words and evaluations canonical ints on both.
"""
from __future__ import annotations

import copy

import numpy as np

import pyref as P
from verifier_pair import COMM_NAMES

R = P.R_MOD
EVAL_NAMES = ("a_eval", "b_eval", "c_eval", "d_eval", "a_next_eval", "b_next_eval", "d_next_eval",
              "q_arith_eval", "q_c_eval", "q_l_eval", "q_r_eval", "s_sigma_1_eval",
              "s_sigma_2_eval", "s_sigma_3_eval", "r_poly_eval", "perm_eval")
KINDS = ("eval", "comm+G", "comm neg", "comm identity", "pi")


def identity_words():
    return np.array([0] * 12 + [1], dtype=np.uint64)


def point(words):
    """uint64[13] ABI words -> pyref affine point (None: the identity)."""
    return P.g1_vec_from_np(np.asarray(words, dtype=np.uint64).reshape(1, 13))[0]


def words(p):
    return P.g1_vec_to_np([p])[0]


def plus_g(w):
    """P + G as ABI words; the identity becomes G."""
    return words(P.g1_add(point(w), P.G1_GEN))


def changed(proof, **changes):
    """A copy of `proof` with the named evaluations (ints) or commitments (words) replaced."""
    if hasattr(proof, "raw"):
        from verifier_pair import copy_proof
        return copy_proof(proof, **changes)
    q = copy.copy(proof)
    for k, v in changes.items():
        setattr(q, k, v)
    return q


def kind(name: str) -> str:
    """The variant kind (one of KINDS) of a name that `variants` yields."""
    if name.startswith("pi"):
        return "pi"
    if name.endswith("_eval+1") or name.endswith("_eval-1"):
        return "eval"
    return "comm" + name[name.index("_comm") + 5:]


def variants(proof, pis, skipped=None):
    """Yields (name, proof', pis'), each differing from (proof, pis) in exactly one thing: every
    evaluation +1 and -1 mod r; every commitment P + G, -P and the identity; every public input
    +1 mod r; the first two public inputs swapped. Names of variants that would equal the
    original are appended to `skipped` instead."""
    skipped = [] if skipped is None else skipped
    pis = list(pis)
    for e in EVAL_NAMES:
        v = getattr(proof, e)
        yield f"{e}+1", changed(proof, **{e: (v + 1) % R}), pis
        yield f"{e}-1", changed(proof, **{e: (v - 1) % R}), pis
    for c in COMM_NAMES:
        w = np.asarray(getattr(proof, c), dtype=np.uint64)
        p = point(w)
        yield f"{c}+G", changed(proof, **{c: plus_g(w)}), pis
        if p is None:  # -O = O: nothing would change
            skipped += [f"{c} neg", f"{c} identity"]
            continue
        yield f"{c} neg", changed(proof, **{c: words(P.g1_neg(p))}), pis
        yield f"{c} identity", changed(proof, **{c: identity_words()}), pis
    for i, v in enumerate(pis):
        yield f"pi[{i}]+1", proof, pis[:i] + [(v + 1) % R] + pis[i + 1:]
    if len(pis) >= 2:
        if pis[0] % R == pis[1] % R:
            skipped.append("pi swap")
        else:
            yield "pi swap", proof, [pis[1], pis[0]] + pis[2:]


def key_variants(vd):
    """Yields (name, VerifierData') with one thing of the key changed: each of the 15 commitments
    +G (an identity becomes G), the last label byte, m + 1, 2n, the first public input index
    + 1."""
    from dusk_plonk_amd.prover import VerifierData
    from verifier import SEED_LABELS
    comms = np.asarray(vd.comms, dtype=np.uint64).reshape(15, 13)
    for i, lab in enumerate(SEED_LABELS):
        c = comms.copy()
        c[i] = plus_g(c[i])
        yield f"{lab.decode()}+G", VerifierData(vd.label, vd.n, vd.m, c, list(vd.pi_indexes))
    label = vd.label[:-1] + bytes([vd.label[-1] ^ 1])
    yield "label", VerifierData(label, vd.n, vd.m, comms, list(vd.pi_indexes))
    yield "m+1", VerifierData(vd.label, vd.n, vd.m + 1, comms, list(vd.pi_indexes))
    yield "2n", VerifierData(vd.label, 2 * vd.n, vd.m, comms, list(vd.pi_indexes))
    if len(vd.pi_indexes):
        idx = [int(vd.pi_indexes[0]) + 1] + [int(i) for i in vd.pi_indexes[1:]]
        yield "pi_index[0]+1", VerifierData(vd.label, vd.n, vd.m, comms, idx)
