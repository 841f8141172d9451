"""The compact proof format on the host (plk_proof_encode_compact / plk_proof_decode_compact,
csrc/ingest.hip): 11 zkcrypto-compressed commitments and 16 canonical little-endian scalars,
1 040 bytes, ASSUMED (parity unpinned) like the SCALE codec. CPU only: the host decode is the
single-proof path and runs the same square root and endomorphism subgroup test as the kernels;
here it is held against the pure-Python reference tests/g1_ingest_ref.py, whose membership
truth is [r]P == O.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import g1_ingest_ref as ref
import pyref as P

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "proof_scale.npz"
GEN_COMPRESSED = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac58"
                               "6c55e83ff97a1aeffb3af00adb22c6bb")
A_COMM, Z_COMM = 0, 4
EVAL0 = 11 * 48


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(GOLD, allow_pickle=False))


@pytest.fixture(scope="module")
def golden_proof(plk, fixture):
    from dusk_plonk_amd.prover import Proof
    return Proof.from_words(fixture["comms"], fixture["evals"])


def proof_of(points, evals):
    from dusk_plonk_amd.prover import Proof
    return Proof.from_words(P.g1_vec_to_np(points), P.fr_vec_to_np(evals))


def points_of(proof):
    from dusk_plonk_amd.prover import _COMMS
    return P.g1_vec_from_np(np.stack([getattr(proof, c) for c in _COMMS]))


def evals_of(proof):
    from dusk_plonk_amd.prover import _EVALS
    return [getattr(proof, e) for e in _EVALS]


def with_point(data: bytes, field: int, b48: bytes) -> bytes:
    return data[:48 * field] + b48 + data[48 * field + 48:]


def rejected(plk, data, subgroup=True):
    from dusk_plonk_amd.prover import Proof
    with pytest.raises(plk.PlonkError) as err:
        Proof.from_compact(data, subgroup=subgroup)
    return err.value.status == plk.PLK_E_ARG


def test_abi_constants(plk):
    from dusk_plonk_amd import plonk, prover
    hdr = (ROOT / "include" / "plk.h").read_text()
    defs = dict(re.findall(r"^#define (PLK_INGEST_\w+) (\d+)", hdr, re.M))
    assert {k: int(v) for k, v in defs.items()} == {
        "PLK_INGEST_OK": 0, "PLK_INGEST_ENCODING": 1, "PLK_INGEST_RANGE": 2,
        "PLK_INGEST_OFF_CURVE": 3, "PLK_INGEST_SUBGROUP": 4}
    assert (plonk.INGEST_OK, plonk.INGEST_ENCODING, plonk.INGEST_RANGE, plonk.INGEST_OFF_CURVE,
            plonk.INGEST_SUBGROUP) == (0, 1, 2, 3, 4)
    assert (ref.OK, ref.ENCODING, ref.RANGE, ref.OFF_CURVE, ref.SUBGROUP) == (0, 1, 2, 3, 4)
    assert "#define PLK_PROOF_COMPACT_BYTES (11 * 48 + 16 * 32)" in hdr
    assert prover.PROOF_COMPACT_BYTES == ref.COMPACT_BYTES == 1040
    n = plk.plonk.C.c_size_t()
    lib = prover._bind()
    raw = prover.PlkProof()
    assert lib.plk_proof_encode_compact(plk.plonk.C.byref(raw), None, 0, plk.plonk.C.byref(n)) == plk.PLK_OK
    assert n.value == 1040
    assert lib.plk_proof_encode_compact(None, None, 0, None) == plk.PLK_E_ARG
    assert lib.plk_proof_decode_compact(None, 0, None, 1) == plk.PLK_E_ARG


def test_generator_known_vector(plk):
    from dusk_plonk_amd.prover import Proof
    assert GEN_COMPRESSED == ref.compress(P.G1_GEN)
    pts = [P.G1_GEN] + [None] * 10
    data = proof_of(pts, range(16)).to_compact()
    assert data[:48] == GEN_COMPRESSED
    back = Proof.from_compact(data)
    assert points_of(back) == pts
    assert ref.decompress(GEN_COMPRESSED) == (ref.OK, P.G1_GEN, False)
    # the other root: the sort bit alone selects it
    neg = bytes([GEN_COMPRESSED[0] ^ 0x20]) + GEN_COMPRESSED[1:]
    assert points_of(Proof.from_compact(with_point(data, 0, neg)))[0] == P.g1_neg(P.G1_GEN)


def test_round_trip_golden_proof(plk, golden_proof):
    from dusk_plonk_amd.prover import Proof
    data = golden_proof.to_compact()
    assert len(data) == 1040
    assert data == ref.proof_to_compact(points_of(golden_proof), evals_of(golden_proof))
    back = Proof.from_compact(data)
    assert back == golden_proof and back.to_compact() == data
    assert Proof.from_compact(data, subgroup=False) == golden_proof
    assert ref.proof_status(data) == ref.OK


def test_round_trip_identity_commitments(plk, golden_proof):
    from dusk_plonk_amd.prover import Proof
    pts = points_of(golden_proof)
    pts[Z_COMM] = None
    pts[10] = None
    p = proof_of(pts, evals_of(golden_proof))
    data = p.to_compact()
    for f in (Z_COMM, 10):
        assert data[48 * f: 48 * f + 48] == bytes([0xC0]) + bytes(47)
    assert Proof.from_compact(data) == p


def test_compression_matches_the_transcript(plk, golden_proof):
    """The bytes of every commitment are the ones the transcript hashes: tests/verifier.py's
    compress is the restated transcript's (pinned against the library's transcript by the
    challenge tests), and both roots of an x and the identity go through both."""
    import verifier as V
    pts = points_of(golden_proof)
    pts[1] = P.g1_neg(pts[0])
    pts[2] = None
    data = proof_of(pts, evals_of(golden_proof)).to_compact()
    for f, pt in enumerate(pts):
        assert data[48 * f: 48 * f + 48] == V.compress(pt) == ref.compress(pt), f
    assert data[0] & 0x20 != data[48] & 0x20
    for i, e in enumerate(evals_of(golden_proof)):
        assert data[EVAL0 + 32 * i: EVAL0 + 32 * i + 32] == (e % ref.r).to_bytes(32, "little")


def no_root_below_p():
    x = ref.p - 1
    while ref.has_point(x):
        x -= 1
    return x


def test_rejections(plk, golden_proof):
    """Each malformation on its own in an otherwise valid proof; the reference names the reason
    and the same position with a well-formed value decodes."""
    from dusk_plonk_amd.prover import Proof
    good = golden_proof.to_compact()
    gx = P.G1_GEN[0]
    x_none = no_root_below_p()
    assert not ref.has_point(x_none) and all(ref.has_point(x) for x in range(x_none + 1, ref.p))
    inf = bytes([0xC0]) + bytes(47)
    cases = {
        "bit 7 clear": (ref.raw48(gx, 0x00), ref.ENCODING),
        "bit 7 clear, sort set": (ref.raw48(gx, 0x20), ref.ENCODING),
        "infinity with the sort bit": (bytes([0xE0]) + bytes(47), ref.ENCODING),
        "infinity with a tail byte": (inf[:47] + b"\x01", ref.ENCODING),
        "infinity with a low bit of byte 0": (bytes([0xC1]) + bytes(47), ref.ENCODING),
        "infinity bit without compression": (bytes([0x40]) + bytes(47), ref.ENCODING),
        "x = p": (ref.raw48(ref.p, 0x80), ref.RANGE),
        "x = 2^381 - 1": (ref.raw48((1 << 381) - 1, 0xA0), ref.RANGE),
        "x with no root": (ref.raw48(x_none, 0x80), ref.OFF_CURVE),
    }
    for field in (A_COMM, Z_COMM, 10):
        assert Proof.from_compact(with_point(good, field, inf)).to_compact()[48 * field:][:48] == inf
        for what, (b48, code) in cases.items():
            bad = with_point(good, field, b48)
            assert ref.proof_status(bad) == code, what
            assert rejected(plk, bad) and rejected(plk, bad, subgroup=False), (what, field)
    # x = p - 1 itself is well-formed when it has a root
    if ref.has_point(ref.p - 1):
        q = Proof.from_compact(with_point(good, 0, ref.raw48(ref.p - 1, 0x80)), subgroup=False)
        assert points_of(q)[0] == ref.decompress(ref.raw48(ref.p - 1, 0x80), subgroup=False)[1]
    # scalars: r is out of range, r - 1 is not
    for i in (0, 6, 15):
        at = EVAL0 + 32 * i
        bad = good[:at] + ref.r.to_bytes(32, "little") + good[at + 32:]
        assert ref.proof_status(bad) == ref.RANGE and rejected(plk, bad)
        top = good[:at] + b"\xff" * 32 + good[at + 32:]
        assert rejected(plk, top)
        ok = good[:at] + (ref.r - 1).to_bytes(32, "little") + good[at + 32:]
        assert evals_of(Proof.from_compact(ok))[i] == ref.r - 1
    for n in (0, 1039, 1041, 1579):
        assert rejected(plk, (good + good)[:n])


@pytest.fixture(scope="module")
def low_order():
    rng = np.random.Generator(np.random.PCG64(0x10C))
    return {q: ref.low_order_point(q, rng) for q in ref.H_PRIMES}


@pytest.mark.parametrize("q", ref.H_PRIMES)
def test_non_members_are_rejected_only_by_the_subgroup_check(plk, golden_proof, low_order, q):
    from dusk_plonk_amd.prover import Proof
    good = golden_proof.to_compact()
    t = low_order[q]
    x = P.g1_add(ref.member(7 + q), t)
    assert P.g1_is_on_curve(x) and not ref.in_subgroup(x) and not ref.in_subgroup(t)
    for field, pt in ((A_COMM, x), (10, x), (Z_COMM, t), (Z_COMM, P.g1_neg(t))):
        bad = with_point(good, field, ref.compress(pt))
        assert ref.proof_status(bad) == ref.SUBGROUP and ref.proof_status(bad, False) == ref.OK
        assert rejected(plk, bad, subgroup=True)
        assert points_of(Proof.from_compact(bad, subgroup=False))[field] == pt


def test_members_pass_the_subgroup_check(plk, golden_proof):
    """[h]Q of random curve points, small multiples of G and the points of a real proof."""
    from dusk_plonk_amd.prover import Proof
    rng = np.random.Generator(np.random.PCG64(0x10D))
    good = golden_proof.to_compact()
    members = [ref.mul(ref.random_curve_point(rng), ref.H) for _ in range(3)]
    members += [ref.member(k) for k in (1, 2, 3, ref.r - 1)]
    for pt in members:
        assert ref.in_subgroup(pt)
        data = with_point(good, 3, ref.compress(pt))
        assert points_of(Proof.from_compact(data, subgroup=True))[3] == pt
    # a random curve point is a non-member (the cofactor is 2^125.8)
    q = ref.random_curve_point(rng)
    assert not ref.in_subgroup(q)
    assert rejected(plk, with_point(good, 3, ref.compress(q)))
