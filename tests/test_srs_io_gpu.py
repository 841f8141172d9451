"""An SRS from bytes and its verification on the GPU (csrc/srs_io.hip) against Python integers:
plk_srs_load_bytes / plk_srs_export_bytes in both byte forms, the uncompressed decoder's status
classes at the wave boundaries, the fold against [sum rho_i tau^(i+1)]G and [sum rho_i tau^i]G, and
plk_srs_verify's verdict on honest and tampered SRSs.

Sizes: 193 points (three waves and a lane, as the ingest tests) and 2^10 + 8 (a trimmed 2^10 SRS).
The tampered cases load and commit without complaint through plk_srs_load; only verify tells.
"""
import numpy as np
import pytest

import g1_ingest_ref as ref
import pyref as P

pytestmark = pytest.mark.gpu

p, r = P.P_MOD, P.R_MOD
SIZES = (193, (1 << 10) + 8)
FORMATS = ("compressed", "uncompressed")
EDGE = (0, 63, 64, 192)
TAU = 0x3A7D1F6B5C2E49081726354453627180F9EAD7C6B5A49382716F5E4D3C2B1A09 % r
SEED = bytes(range(100, 132))
INF_RAW = bytes([0x40]) + bytes(95)


def tau_limbs(tau=TAU):
    return P.fr_vec_to_np([tau])[0]


def words(pt):
    return P.g1_vec_to_np([pt])[0]


def encode_raw(pt) -> bytes:
    """The uncompressed form: x then y big-endian, 0x40 and zeros for the identity."""
    if pt is None:
        return INF_RAW
    return pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")


def raw96(x: int, y: int, flags: int = 0) -> bytes:
    b = bytearray(x.to_bytes(48, "big") + y.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


def decode_raw(b: bytes, subgroup: bool = True):
    """(status, point, identity): the strict decoding of include/plk.h."""
    assert len(b) == 96
    if b[0] & 0xA0:
        return ref.ENCODING, None, False
    if b[0] & 0x40:
        return (ref.OK, None, True) if b == INF_RAW else (ref.ENCODING, None, False)
    x, y = int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big")
    if x >= p or y >= p:
        return ref.RANGE, None, False
    if (y * y - x ** 3 - 4) % p:
        return ref.OFF_CURVE, None, False
    if subgroup and not ref.in_subgroup((x, y)):
        return ref.SUBGROUP, None, False
    return ref.OK, (x, y), False


def encode(pt, fmt):
    return ref.compress(pt) if fmt == "compressed" else encode_raw(pt)


class Srs:
    """One honest SRS per size, its points as Python integers, and the matching opening key."""

    def __init__(self, plk, ctx):
        self.plk, self.ctx = plk, ctx
        self.pp = {n: plk.PlonkParams.setup(0, tau_limbs(), ctx, n_points=n) for n in SIZES}
        self.words = {n: self.pp[n].points() for n in SIZES}
        self.pts = {n: P.g1_vec_from_np(self.words[n]) for n in SIZES}
        self.key = plk.OpeningKey.setup(TAU)
        rng = np.random.Generator(np.random.PCG64(0x5125))
        self.non_member = ref.non_member(10177, rng)

    def tampered(self, n, edits):
        """plk_srs_load of the honest points with rows replaced: {index: point or None}."""
        w = self.words[n].copy()
        for k, pt in edits.items():
            w[k] = words(pt)
        return self.plk.PlonkParams.load(w, self.ctx)


@pytest.fixture(scope="module")
def S(plk, gpu_ctx):
    s = Srs(plk, gpu_ctx)
    # the SRS the rest is measured against: g1[i] = [tau^i] G at a few indices, in Python
    for n in SIZES:
        for i in (0, 1, 2, n - 1):
            assert s.pts[n][i] == P.g1_mul(P.G1_GEN, pow(TAU, i, r))
    return s


def rejected(plk, ctx, blob, fmt, subgroup=True):
    with pytest.raises(plk.PlonkError) as e:
        plk.PlonkParams.from_bytes(blob, fmt, subgroup, ctx)
    assert e.value.status == plk.PLK_E_ARG
    return e.value.bad_index, e.value.bad_status


# ---- round trip --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_round_trip(plk, gpu_ctx, S, fmt, n):
    pp = S.pp[n]
    blob = pp.to_bytes(fmt)
    assert blob == b"".join(encode(pt, fmt) for pt in S.pts[n])
    back = plk.PlonkParams.from_bytes(blob, fmt, True, gpu_ctx)
    assert back.n == n and np.array_equal(back.points(), S.words[n])
    dec_ms, sub_ms = plk.plonk.srs_last_load_ms(gpu_ctx)
    assert dec_ms > 0 and sub_ms > 0
    assert back.to_bytes(fmt) == blob
    # a slice of the export
    size = len(blob) // n
    assert pp.to_bytes(fmt, 63, 3) == blob[63 * size:66 * size]
    rng = np.random.Generator(np.random.PCG64(n))
    poly = P.fr_vec_to_np([int.from_bytes(rng.bytes(40), "little") % r for _ in range(n)])
    a, b = pp.commit(plk.Coefficients(poly)), back.commit(plk.Coefficients(poly))
    assert a.words.tobytes() == b.words.tobytes() and not a.is_identity
    # the imported SRS verifies, with the point and subgroup passes already behind it
    v = back.verify(S.key, SEED)
    assert v.ok and v.verdict == plk.plonk.SRS_OK and v.bad_index is None


def test_end_to_end_proof_on_an_imported_srs(plk, gpu_ctx, S):
    from dusk_plonk_amd.prover import Plonk, PlonkKey
    n = SIZES[1]
    pp = plk.PlonkParams.from_bytes(S.pp[n].to_bytes("compressed"), "compressed", True, gpu_ctx)
    key = plk.OpeningKey.from_bytes(*S.key.to_bytes("compressed"), "compressed")
    cs = Plonk()
    cs.append_public(12345)
    cs.synthetic_chain(900, 3)
    prover, vd = PlonkKey.compile_composer(pp, b"imported srs", cs)
    proof, pis = prover.prove_composer(cs, 77)
    assert vd.verifier().verify(proof, pis, key) is None
    key_u = plk.OpeningKey.from_bytes(*S.key.to_bytes("uncompressed"), "uncompressed")
    assert vd.verifier().verify(proof, pis, key_u) is None


# ---- the uncompressed decoder ------------------------------------------------------------------
@pytest.fixture(scope="module")
def specimens(S):
    g = P.G1_GEN
    x_none = next(x for x in range(5, 60) if not ref.has_point(x))
    spec = {
        ref.ENCODING: [raw96(g[0], g[1], 0x80), raw96(g[0], g[1], 0x20), raw96(g[0], g[1], 0x40),
                       INF_RAW[:95] + b"\x01"],
        ref.RANGE: [raw96(p, g[1]), raw96(g[0], p), raw96(g[0], p + g[1]), raw96((1 << 381) - 1, 1)],
        ref.OFF_CURVE: [raw96(g[0], (g[1] + 1) % p), raw96(x_none, 2), raw96(g[0], g[1] - 1), raw96(0, 0)],
        ref.SUBGROUP: [encode_raw(S.non_member)] * 4,
    }
    for code, items in spec.items():
        for b in items:
            assert decode_raw(b)[0] == code
    return spec


@pytest.mark.parametrize("code", [ref.ENCODING, ref.RANGE, ref.OFF_CURVE, ref.SUBGROUP])
def test_uncompressed_rejects_at_the_wave_boundaries(plk, gpu_ctx, S, specimens, code):
    n = SIZES[0]
    base = [encode_raw(pt) for pt in S.pts[n]]
    for lane, spec in zip(EDGE, specimens[code]):
        items = list(base)
        items[lane] = spec
        assert rejected(plk, gpu_ctx, b"".join(items), "uncompressed") == (lane, code)


def test_uncompressed_accepts_members_identities_and_the_other_root(plk, gpu_ctx, S):
    n = SIZES[0]
    pts = list(S.pts[n])
    for lane in EDGE:
        pts[lane] = None                      # infinity encodings are accepted
    pts[1], pts[65] = P.g1_neg(pts[1]), P.g1_neg(pts[65])   # y = the other root of a valid x
    items = [encode_raw(pt) for pt in pts]
    for b in items:
        assert decode_raw(b)[0] == ref.OK
    got = plk.PlonkParams.from_bytes(b"".join(items), "uncompressed", True, gpu_ctx)
    assert np.array_equal(got.points(), P.g1_vec_to_np(pts))
    assert got.to_bytes("uncompressed") == b"".join(items)
    assert got.to_bytes("compressed") == b"".join(ref.compress(pt) for pt in pts)
    # y off by one is off the curve
    x, y = S.pts[n][65]
    items[65] = raw96(x, (y + 1) % p)
    assert rejected(plk, gpu_ctx, b"".join(items), "uncompressed") == (65, ref.OFF_CURVE)


def test_the_smallest_rejected_index_is_reported(plk, gpu_ctx, S, specimens):
    n = SIZES[0]
    for fmt in FORMATS:
        items = [encode(pt, fmt) for pt in S.pts[n]]
        if fmt == "uncompressed":
            items[192] = specimens[ref.ENCODING][0]
            items[64] = specimens[ref.RANGE][0]
            items[63] = specimens[ref.OFF_CURVE][0]
            want = (63, ref.OFF_CURVE)
        else:
            items[192] = ref.raw48(P.G1_GEN[0], 0x20)          # encoding
            items[100] = ref.raw48(p, 0x80)                    # range
            items[64] = ref.compress(S.non_member)             # found by the later kernel
            want = (64, ref.SUBGROUP)
        assert rejected(plk, gpu_ctx, b"".join(items), fmt) == want


def test_bad_arguments(plk, gpu_ctx, S):
    lib, ptr = plk.plonk._lib(), plk.plonk._ptr
    import ctypes as C
    buf = np.frombuffer(ref.compress(P.G1_GEN), dtype=np.uint8)
    h = C.c_void_p()
    assert lib.plk_srs_load_bytes(gpu_ctx.handle, ptr(buf), 0, 0, 1, C.byref(h), None, None) == plk.PLK_E_ARG
    assert lib.plk_srs_load_bytes(gpu_ctx.handle, None, 1, 0, 1, C.byref(h), None, None) == plk.PLK_E_ARG
    assert lib.plk_srs_load_bytes(gpu_ctx.handle, ptr(buf), 1, 2, 1, C.byref(h), None, None) == plk.PLK_E_ARG
    assert lib.plk_srs_load_bytes(gpu_ctx.handle, ptr(buf), 1, 0, 1, None, None, None) == plk.PLK_E_ARG
    pp = S.pp[SIZES[0]]
    out = np.zeros(96, dtype=np.uint8)
    assert lib.plk_srs_export_bytes(pp._h, 193, 1, 0, ptr(out)) == plk.PLK_E_ARG
    assert lib.plk_srs_export_bytes(pp._h, 0, 1, 7, ptr(out)) == plk.PLK_E_ARG
    v, idx = C.c_int(0), C.c_uint64(0)
    assert lib.plk_srs_verify(gpu_ctx.handle, pp._h, None, None, C.byref(v), C.byref(idx)) == plk.PLK_E_ARG
    assert lib.plk_srs_verify(None, pp._h, S.key._h, None, C.byref(v), C.byref(idx)) == plk.PLK_E_ARG


# ---- load rejects ------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [0, 64, SIZES[0] - 1])
def test_a_non_member_is_refused_or_found_by_verify(plk, gpu_ctx, S, at):
    n = SIZES[0]
    items = [ref.compress(pt) for pt in S.pts[n]]
    items[at] = ref.compress(S.non_member)
    blob = b"".join(items)
    assert rejected(plk, gpu_ctx, blob, "compressed") == (at, ref.SUBGROUP)
    loose = plk.PlonkParams.from_bytes(blob, "compressed", False, gpu_ctx)
    assert np.array_equal(loose.points(at, 1)[0], words(S.non_member))
    assert plk.plonk.srs_last_load_ms(gpu_ctx)[1] == 0
    v = loose.verify(S.key, SEED)
    assert (v.ok, v.verdict, v.bad_index) == (False, plk.plonk.SRS_SUBGROUP, at)


# ---- the fold ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_fold_equals_the_python_expectation(plk, gpu_ctx, S, n):
    rho = P.fr_vec_from_np(plk.plonk.debug_srs_weights(SEED, n, gpu_ctx))
    assert rho == P.fr_vec_from_np(plk.plonk.debug_srs_weights(SEED, n))   # the host mirror
    assert len(rho) == n - 1 and rho[0] == 1 and all(0 < v < 1 << 128 for v in rho)
    assert len(set(rho)) == n - 1
    sw, t = 0, 1
    for v in rho:
        sw = (sw + v * t) % r
        t = t * TAU % r
    sc = sw * TAU % r
    got = S.pp[n].fold_chain(SEED)
    assert np.array_equal(got[0], words(P.g1_mul(P.G1_GEN, sc)))
    assert np.array_equal(got[1], words(P.g1_mul(P.G1_GEN, sw)))
    assert S.key.check(got)
    other = S.pp[n].fold_chain(bytes(32))
    assert not np.array_equal(other, got) and S.key.check(other)
    assert not np.array_equal(S.pp[n].fold_chain(None), S.pp[n].fold_chain(None))


def test_fold_of_one_point_is_the_identity_pair(plk, gpu_ctx, S):
    one = plk.PlonkParams.from_bytes(ref.compress(P.G1_GEN), "compressed", True, gpu_ctx)
    got = one.fold_chain(SEED)
    assert np.array_equal(got, np.stack([words(None), words(None)]))
    assert one.verify(S.key, SEED).ok


# ---- verify ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_verify_accepts_the_honest_srs(plk, S, n):
    for seed in (None, SEED):
        v = S.pp[n].verify(S.key, seed)
        assert v.ok and v.verdict == plk.plonk.SRS_OK and v.bad_index is None
    fold_ms, pairing_ms = S.pp[n].last_verify_ms()
    assert fold_ms > 0 and pairing_ms > 0


def verdict(pp, key, seed=SEED):
    v = pp.verify(key, seed)   # a bad SRS is a verdict: no exception may come out of here
    assert not v.ok
    return v.verdict, v.bad_index


@pytest.mark.parametrize("k", [1, 63, 64, SIZES[0] - 1])
def test_verify_rejects_one_wrong_power(plk, S, k):
    n = SIZES[0]
    bad = S.tampered(n, {k: P.g1_add(S.pts[n][k], P.G1_GEN)})      # [tau^k + 1] G
    poly = P.fr_vec_to_np(list(range(1, n + 1)))
    assert not bad.commit(plk.Coefficients(poly)).is_identity       # it loads and commits
    assert verdict(bad, S.key) == (plk.plonk.SRS_CHAIN, None)
    assert verdict(bad, S.key, None) == (plk.plonk.SRS_CHAIN, None)


def test_verify_rejects_swapped_neighbours_and_another_tau(plk, S):
    n = SIZES[1]
    bad = S.tampered(n, {500: S.pts[n][501], 501: S.pts[n][500]})
    assert verdict(bad, S.key) == (plk.plonk.SRS_CHAIN, None)
    other = plk.OpeningKey.setup(TAU + 1)
    for m in SIZES:
        assert verdict(S.pp[m], other) == (plk.plonk.SRS_CHAIN, None)


def test_verify_rejects_a_scaled_srs(plk, S):
    """Every point times 5: the chain holds for the same tau, only the generator test tells."""
    n = SIZES[0]
    scaled = S.tampered(n, {i: P.g1_mul(pt, 5) for i, pt in enumerate(S.pts[n])})
    assert S.key.check(scaled.fold_chain(SEED))
    assert verdict(scaled, S.key) == (plk.plonk.SRS_GENERATOR, None)


def test_verify_rejects_an_identity_and_a_point_off_the_curve(plk, S):
    n = SIZES[0]
    assert verdict(S.tampered(n, {7: None, 100: None}), S.key) == (plk.plonk.SRS_INFINITY, 7)
    w = S.words[n].copy()
    w[64, 6] ^= np.uint64(1)                                  # y off the curve
    w[100, 0:6] = P.int_to_limbs(p, 6)                        # a limb pattern >= p
    bad = plk.PlonkParams.load(w, S.ctx)
    assert verdict(bad, S.key) == (plk.plonk.SRS_POINT, 64)
    w = S.words[n].copy()
    w[192, 0:6] = P.int_to_limbs(p + 1, 6)
    assert verdict(plk.PlonkParams.load(w, S.ctx), S.key) == (plk.plonk.SRS_POINT, 192)
