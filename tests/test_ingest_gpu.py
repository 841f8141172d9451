"""The ingest kernels (csrc/ingest.hip k_g1_decompress, k_g1_subgroup, k_fr_decode) against the
pure-Python reference tests/g1_ingest_ref.py, limb for limb: plk_g1_decompress_batch and
plk_g1_subgroup_check_batch on 193 points (three waves and one lane) with every status class at
lanes 0, 63, 64 and 192, and plk_proofs_ingest on 67 compact proofs against the host decode.
"""
import numpy as np
import pytest

import g1_ingest_ref as ref
import pyref as P

pytestmark = pytest.mark.gpu

N = 193
EDGE = (0, 63, 64, 192)
INF = bytes([0xC0]) + bytes(47)


class Points:
    """The 193 encodings, one specimen per status class, and the reference's answers (cached by
    encoding: the same bytes always decode the same)."""

    def __init__(self):
        rng = np.random.Generator(np.random.PCG64(0x1A6E57))
        self.non_members = [ref.non_member(q, rng, k=3 + q) for q in ref.H_PRIMES]
        self.low = [ref.low_order_point(q, rng) for q in ref.H_PRIMES]
        members, acc = [], ref.member(int.from_bytes(rng.bytes(31), "little"))
        step = ref.member(int.from_bytes(rng.bytes(31), "little"))
        for _ in range(24):
            members.append(acc)
            acc = P.g1_add(acc, step)
        members += [ref.mul(ref.random_curve_point(rng), ref.H) for _ in range(2)]
        self.members = members
        x_none = [x for x in range(ref.p - 1, ref.p - 40, -1) if not ref.has_point(x)][:4]
        x_none += [x for x in range(5, 60) if not ref.has_point(x)][:3]
        g = P.G1_GEN
        items = [ref.compress(m) for m in members]
        items += [ref.compress(g), ref.compress(P.g1_neg(g))]            # both roots of one x
        items += [ref.raw48(x, 0x80 | (0x20 * (i & 1))) for i, x in enumerate(x_none)]
        items += [ref.raw48(ref.p - 1, 0x80), ref.raw48(ref.p - 1, 0xA0)]
        items += [ref.raw48(ref.p, 0x80), ref.raw48(ref.p + 1, 0xA0), ref.raw48((1 << 381) - 1, 0x80)]
        items += [ref.raw48(0, 0x80), ref.raw48(0, 0xA0)]                   # x = 0: (0, +-2)
        items += [INF]
        items += [ref.raw48(g[0], 0x00), ref.raw48(g[0], 0x20), bytes([0xE0]) + bytes(47),
                  INF[:47] + b"\x01", bytes([0x40]) + bytes(47), bytes(48), b"\xff" * 48]
        items += [ref.compress(x) for x in self.non_members]
        items += [ref.compress(t) for t in self.low] + [ref.compress(P.g1_neg(t)) for t in self.low]
        items += [ref.compress(ref.random_curve_point(rng)) for _ in range(3)]
        self.base = [items[i % len(items)] for i in range(N)]
        assert len(items) <= N
        self.specimen = {ref.OK: ref.compress(members[0]), ref.ENCODING: ref.raw48(g[0], 0x20),
                         ref.RANGE: ref.raw48(ref.p, 0x80), ref.OFF_CURVE: ref.raw48(x_none[0], 0x80),
                         ref.SUBGROUP: ref.compress(self.non_members[2])}
        self._cache = {}

    def batch(self, code):
        items = list(self.base)
        for lane in EDGE:
            items[lane] = self.specimen[code]
        return items

    def expect(self, items, subgroup):
        st, words = [], []
        for b in items:
            if (b, subgroup) not in self._cache:
                self._cache[(b, subgroup)] = ref.decompress_words(b, subgroup)
            s, w = self._cache[(b, subgroup)]
            st.append(s)
            words.append(w)
        return np.array(st, dtype=np.uint8), np.stack(words)


@pytest.fixture(scope="module")
def pts():
    return Points()


@pytest.mark.parametrize("code", [ref.OK, ref.ENCODING, ref.RANGE, ref.OFF_CURVE, ref.SUBGROUP])
def test_decompress_batch_equals_the_reference(plk, gpu_ctx, pts, code):
    items = pts.batch(code)
    want_st, want = pts.expect(items, True)
    assert all(want_st[lane] == code for lane in EDGE)
    assert set(want_st) == {0, 1, 2, 3, 4}
    got, st = plk.g1_decompress(b"".join(items), subgroup=True, ctx=gpu_ctx)
    assert got.shape == (N, 13) and st.shape == (N,)
    assert np.array_equal(st, want_st)
    assert np.array_equal(got, want)
    assert not got[st != 0].any()
    dec_ms, sub_ms = plk.ingest_last_ms(gpu_ctx)
    assert dec_ms > 0 and sub_ms > 0


def test_decompress_without_the_subgroup_check_returns_the_non_members(plk, gpu_ctx, pts):
    items = pts.batch(ref.SUBGROUP)
    want_st, want = pts.expect(items, False)
    assert ref.SUBGROUP not in set(want_st)
    got, st = plk.g1_decompress(b"".join(items), subgroup=False, ctx=gpu_ctx)
    assert np.array_equal(st, want_st) and np.array_equal(got, want)
    x = P.g1_vec_to_np([pts.non_members[2]])[0]
    for lane in EDGE:
        assert np.array_equal(got[lane], x)
    assert plk.ingest_last_ms(gpu_ctx)[1] == 0


def test_decompress_one_point_and_bad_arguments(plk, gpu_ctx, pts):
    got, st = plk.g1_decompress(pts.specimen[ref.OK], ctx=gpu_ctx)
    assert list(st) == [0] and np.array_equal(got[0], P.g1_vec_to_np([pts.members[0]])[0])
    lib = plk.plonk._lib()
    out, s = np.zeros((1, 13), dtype=np.uint64), np.zeros(1, dtype=np.uint8)
    buf = np.frombuffer(INF, dtype=np.uint8)
    ptr = plk.plonk._ptr
    assert lib.plk_g1_decompress_batch(gpu_ctx.handle, ptr(buf), 0, 1, ptr(out), ptr(s)) == plk.PLK_E_ARG
    assert lib.plk_g1_decompress_batch(gpu_ctx.handle, None, 1, 1, ptr(out), ptr(s)) == plk.PLK_E_ARG
    assert lib.plk_g1_decompress_batch(gpu_ctx.handle, ptr(buf), 1, 1, ptr(out), None) == plk.PLK_E_ARG


def test_subgroup_check_batch_equals_r_times_p(plk, gpu_ctx, pts):
    """The finite curve points of the set, plus identities, as ABI points: [r]P == O."""
    items = pts.batch(ref.SUBGROUP)
    _, words = pts.expect(items, False)
    finite = [w for w in words if w.any()]
    ident = P.g1_vec_to_np([None])[0]
    points = [ident] + finite + [ident]
    points = (points * (N // len(points) + 1))[:N]
    for lane in EDGE[:2]:
        points[lane] = ident
    arr = np.stack(points)
    want = np.array([ref.in_subgroup(pt) for pt in P.g1_vec_from_np(arr)])
    assert want.any() and not want.all()
    got = plk.g1_subgroup_check(arr, ctx=gpu_ctx)
    assert got.dtype == bool and np.array_equal(got, want)
    # an off-curve point, a non-canonical one, a bad infinity word: PLK_E_ARG
    mid = next(i for i in range(65, N) if not arr[i, 12])
    last = next(i for i in range(N - 1, 0, -1) if not arr[i, 12])
    for spoil in ((mid, 6, 1), (last, 5, 1 << 63), (0, 12, 2)):
        bad = arr.copy()
        bad[spoil[0], spoil[1]] ^= np.uint64(spoil[2])
        with pytest.raises(plk.PlonkError) as err:
            plk.g1_subgroup_check(bad, ctx=gpu_ctx)
        assert err.value.status == plk.PLK_E_ARG


# ---- plk_proofs_ingest -------------------------------------------------------------------
COUNT = 67
BAD = [0, 31, 32, 33, 64, 66]


@pytest.fixture(scope="module")
def S(plk, gpu_ctx):
    from test_verifier_verify_gpu import Setup67
    return Setup67(plk)


def spoil(data: bytes, code: int, pts, k: int) -> bytes:
    """One failure of class `code` in one field of a compact proof."""
    field = k % 11
    put = lambda b: data[:48 * field] + b + data[48 * field + 48:]
    if code == ref.ENCODING:
        return put(bytes([data[48 * field] & 0x7F]) + data[48 * field + 1: 48 * field + 48])
    if code == ref.RANGE and k % 2:
        at = 528 + 32 * (k % 16)
        return data[:at] + ref.r.to_bytes(32, "little") + data[at + 32:]
    return put(pts.specimen[code])


def test_proofs_ingest(plk, gpu_ctx, S, pts):
    from dusk_plonk_amd.prover import Proof, ingest_proofs
    blobs = [p.to_compact() for p in S.proofs]
    codes = {0: ref.ENCODING, 31: ref.RANGE, 32: ref.RANGE, 33: ref.OFF_CURVE, 64: ref.SUBGROUP,
             66: ref.ENCODING}
    assert sorted(codes) == BAD
    for k, c in codes.items():
        blobs[k] = spoil(blobs[k], c, pts, k)
        assert ref.proof_status(blobs[k]) == c
    proofs, status = ingest_proofs(b"".join(blobs), subgroup=True, ctx=gpu_ctx)
    assert len(proofs) == COUNT and list(status) == [codes.get(j, 0) for j in range(COUNT)]
    for j in range(COUNT):
        if j in codes:
            assert proofs[j] is None
            with pytest.raises(plk.PlonkError):
                Proof.from_compact(blobs[j])
        else:  # byte for byte the host decode, which gives back the prover's proof
            assert proofs[j].raw_bytes() == Proof.from_compact(blobs[j]).raw_bytes()
            assert proofs[j] == S.proofs[j]
    # the raw output of a rejected proof is all zero bytes
    from dusk_plonk_amd.prover import PlkProof, _bind
    raw = (PlkProof * COUNT)()
    st = np.zeros(COUNT, dtype=np.uint8)
    assert _bind().plk_proofs_ingest(gpu_ctx.handle, b"".join(blobs), COUNT, 1, raw,
                                     plk.plonk._ptr(st)) == plk.PLK_OK
    for j in BAD:
        assert bytes(raw[j]) == bytes(len(bytes(raw[j])))
    # without the subgroup check the non-member proof decodes
    proofs0, status0 = ingest_proofs(b"".join(blobs), subgroup=False, ctx=gpu_ctx)
    assert list(status0) == [0 if j == 64 else codes.get(j, 0) for j in range(COUNT)]
    # count = 1, good and bad
    one, st1 = ingest_proofs(blobs[1], ctx=gpu_ctx)
    assert list(st1) == [0] and one[0] == S.proofs[1]
    one, st1 = ingest_proofs(blobs[33], ctx=gpu_ctx)
    assert list(st1) == [ref.OFF_CURVE] and one[0] is None


# ---- the plk_g1 input rules of plk_g1_subgroup_check_batch ------------------------------------
@pytest.fixture(scope="module")
def abi_batch(pts):
    """65 finite curve points, members and non-members, and [r]P == O of each in Python."""
    points = (pts.members + pts.non_members + pts.low)
    points = (points * (65 // len(points) + 1))[:65]
    member = {pt: ref.in_subgroup(pt) for pt in set(points)}
    return points, np.array([member[pt] for pt in points])


@pytest.mark.parametrize("lane", ref.ABI_LANES)
@pytest.mark.parametrize("what", ref.ABI_REFUSED)
def test_subgroup_check_refuses_a_malformed_point(plk, gpu_ctx, abi_batch, what, lane):
    arr = P.g1_vec_to_np(abi_batch[0])
    arr[lane] = ref.abi_spoil(arr[lane], what)
    with pytest.raises(plk.PlonkError) as err:
        plk.g1_subgroup_check(arr, ctx=gpu_ctx)
    assert err.value.status == plk.PLK_E_ARG


@pytest.mark.parametrize("lane", ref.ABI_LANES)
def test_subgroup_check_identity_word_hides_the_coordinates(plk, gpu_ctx, abi_batch, lane):
    arr = P.g1_vec_to_np(abi_batch[0])
    arr[lane] = ref.abi_spoil(arr[lane], ref.ABI_IDENTITY)
    want = abi_batch[1].copy()
    want[lane] = True  # the identity has order r
    assert want.any() and not want.all()
    assert np.array_equal(plk.g1_subgroup_check(arr, ctx=gpu_ctx), want)
