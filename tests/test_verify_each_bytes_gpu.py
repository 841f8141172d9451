"""plk_verifier_verify_each_bytes: compact bytes in, one verdict per proof out (1 valid, 0
well-formed but wrong, 0x10 | status when ingest rejected it), on the 67 public_sum proofs of
tests/test_verifier_verify_gpu.py in both replay modes.
"""
import numpy as np
import pytest

import g1_ingest_ref as ref
import pyref as P
from test_verifier_verify_gpu import COUNT, Setup67

pytestmark = pytest.mark.gpu

REJECT = {0: ref.ENCODING, 32: ref.RANGE, 33: ref.OFF_CURVE, 64: ref.SUBGROUP, 66: ref.RANGE}
WRONG = [1, 31, 63, 65]  # well-formed, d_eval + 1: the pairing check fails


@pytest.fixture(scope="module")
def S(plk, gpu_ctx):
    return Setup67(plk)


@pytest.fixture(scope="module")
def low():
    rng = np.random.Generator(np.random.PCG64(0xB17E5))
    return {q: ref.low_order_point(q, rng) for q in (3, 11)}


def with_point(data, field, b48):
    return data[:48 * field] + b48 + data[48 * field + 48:]


def add_to_a_comm(proof, t) -> bytes:
    """The compact proof with the low-order point t added to a_comm: its only defect."""
    a = P.g1_vec_from_np(proof.a_comm.reshape(1, 13))[0]
    return with_point(proof.to_compact(), 0, ref.compress(P.g1_add(a, t)))


def batch(S, low):
    blobs = [p.to_compact() for p in S.spoiled(WRONG)]
    x_none = next(x for x in range(ref.p - 1, 0, -1) if not ref.has_point(x))
    for k, code in REJECT.items():
        if code == ref.ENCODING:
            blobs[k] = with_point(blobs[k], 4, bytes([0xE0]) + bytes(47))
        elif code == ref.RANGE and k == 66:
            blobs[k] = blobs[k][:-32] + ref.r.to_bytes(32, "little")  # perm_eval = r
        elif code == ref.RANGE:
            blobs[k] = with_point(blobs[k], 10, ref.raw48(ref.p, 0xA0))
        elif code == ref.OFF_CURVE:
            blobs[k] = with_point(blobs[k], 7, ref.raw48(x_none, 0x80))
        else:
            blobs[k] = add_to_a_comm(S.proofs[k], low[11])
        assert ref.proof_status(blobs[k]) == code
    return blobs


@pytest.mark.parametrize("replay", ["host", "device"])
def test_verify_each_bytes(plk, S, low, replay):
    from dusk_plonk_amd.prover import Proof
    ver = S.key["public_sum"][2]
    blobs = batch(S, low)
    want = np.ones(COUNT, dtype=np.uint8)
    want[WRONG] = 0
    for k, code in REJECT.items():
        want[k] = 0x10 | code
    keep = [j for j in range(COUNT) if j not in REJECT]
    ver.set_replay(replay)
    try:
        got = ver.verify_each_bytes(b"".join(blobs), S.pis, S.opening)
        each = ver.verify_each([Proof.from_compact(blobs[j]) for j in keep], [S.pis[j] for j in keep],
                               S.opening)
        clean = ver.verify_each_bytes(b"".join(p.to_compact() for p in S.proofs), S.pis, S.opening)
    finally:
        ver.set_replay("host")
    assert got.dtype == np.uint8 and list(got) == list(want)
    assert list(got[keep]) == list(each.astype(np.uint8))
    assert list(clean) == [1] * COUNT


def test_all_rejected_batch_is_ok_with_no_valid_verdict(plk, S):
    ver = S.key["public_sum"][2]
    blobs = [bytes([b[0] & 0x7F]) + b[1:] for b in (p.to_compact() for p in S.proofs[:5])]
    got = ver.verify_each_bytes(b"".join(blobs), S.pis[:5], S.opening)
    assert list(got) == [0x10 | ref.ENCODING] * 5
    one = ver.verify_each_bytes(blobs[0], S.pis[:1], S.opening)
    assert list(one) == [0x10 | ref.ENCODING]


@pytest.mark.parametrize("q", [3, 11])
def test_a_non_member_commitment_is_the_only_defect(plk, S, low, q):
    ver = S.key["public_sum"][2]
    blobs = [p.to_compact() for p in S.proofs[:9]]
    blobs[4] = add_to_a_comm(S.proofs[4], low[q])
    assert ref.proof_status(blobs[4], True) == ref.SUBGROUP and ref.proof_status(blobs[4], False) == ref.OK
    got = ver.verify_each_bytes(b"".join(blobs), S.pis[:9], S.opening, subgroup=True)
    assert list(got) == [1, 1, 1, 1, 0x10 | ref.SUBGROUP, 1, 1, 1, 1]
    # unchecked, it is an ordinary verdict, whatever the pairing says; the others are unchanged
    got0 = ver.verify_each_bytes(b"".join(blobs), S.pis[:9], S.opening, subgroup=False)
    assert got0[4] in (0, 1)
    assert list(np.delete(got0, 4)) == [1] * 8
