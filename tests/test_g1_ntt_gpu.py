"""The transform over G1 (csrc/g1_ntt.hip) alone, through plk_debug_g1_ntt: both directions
against [sum_j k_j omega^(+-ij)]G, computed from the inputs' discrete logs by the Python-integer
scalar transform and one reference multiplication per output. Bit for bit, in both forms of the
twiddle multiplication (PLK_G1_NTT_FORM: "xyzz" inside the butterfly, the hook's default, and
"glv", affine between the levels, the form plk_kzg_open_domain runs).

Sizes: 2 and 4 (one and two levels), 64 and 128 (half a wave and one wave of butterflies), 256
(one block of the butterfly kernels, 128 lanes) and 512 (two blocks)."""
import numpy as np
import pytest

import kzg_ref as K
import pyref as P

pytestmark = pytest.mark.gpu

R = P.R_MOD
KS = [1, 2, 6, 7, 8, 9]


def input_logs(kind: str, k: int):
    n = 1 << k
    rng = P.SplitMix64(1000 + k)
    if kind == "random":
        return [rng.fr() for _ in range(n)]
    if kind == "all equal":  # every first-level butterfly: a doubling and an identity difference
        return [rng.fr()] * n
    if kind == "alternating":  # P, -P, P, ..
        p = rng.fr()
        return [p if i % 2 == 0 else R - p for i in range(n)]
    if kind == "identities":
        return [0] * n
    if kind.startswith("single"):
        at = {"single 0": 0, "single 1": 1, "single last": n - 1}[kind]
        return [rng.fr() if i == at else 0 for i in range(n)]
    if kind == "root powers":  # [tau^i]G for tau the primitive n-th root: the transform is a delta
        return [pow(P.omega(k), i, R) for i in range(n)]
    raise ValueError(kind)


KINDS = ["random", "all equal", "alternating", "identities", "single 0", "single 1", "single last",
         "root powers"]


@pytest.fixture(params=["xyzz", "glv"])
def form(request, monkeypatch):
    monkeypatch.setenv("PLK_G1_NTT_FORM", request.param)  # read by the library at every call
    return request.param


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", KS)
def test_transform_matches_the_integers(plk, gpu_ctx, form, k, kind, direction):
    logs = input_logs(kind, k)
    want_logs = P.dft(logs, k) if direction == 1 else P.idft(logs, k)
    if kind == "root powers" and direction == -1:  # n^-1 sum_j w^(j - ij): the delta at i = 1
        assert want_logs == [1 if i == 1 else 0 for i in range(1 << k)]
    got = plk.debug_g1_ntt(K.gen_mul_np(logs), k, direction, gpu_ctx)
    assert np.array_equal(got, K.gen_mul_np(want_logs))


@pytest.mark.parametrize("kind", ["random", "all equal", "single 1"])
@pytest.mark.parametrize("k", KS)
def test_forward_then_inverse_returns_the_input_bytes(plk, gpu_ctx, form, k, kind):
    pts = K.gen_mul_np(input_logs(kind, k))
    fwd = plk.debug_g1_ntt(pts, k, 1, gpu_ctx)
    assert np.array_equal(plk.debug_g1_ntt(fwd, k, -1, gpu_ctx), pts)


def test_points_outside_g1_transform_exactly_in_the_xyzz_form(plk, gpu_ctx, monkeypatch):
    # the windowed multiplication uses no endomorphism: any curve point is legal input
    import g1_ingest_ref as G
    monkeypatch.setenv("PLK_G1_NTT_FORM", "xyzz")
    rng = np.random.default_rng(5)
    t = G.low_order_point(11, rng)
    w = P.omega(2)
    p0, p1, p2, p3 = pts = [G.member(3), P.g1_add(G.member(9), t), None, G.member(4)]
    assert not G.in_subgroup(p1)
    got = plk.debug_g1_ntt(P.g1_vec_to_np(pts), 2, 1, gpu_ctx)
    # off G1 "omega^3 P" is not "-(omega P)": the transform is its butterfly network with the
    # canonical twiddle as an integer (g1_ingest_ref.mul does not reduce mod r)
    sub = lambda a, b: P.g1_add(a, P.g1_neg(b))
    e, o = P.g1_add(p0, p2), P.g1_add(p1, p3)
    d, wd = sub(p0, p2), G.mul(sub(p1, p3), w)
    want = [P.g1_add(e, o), P.g1_add(d, wd), sub(e, o), sub(d, wd)]
    assert np.array_equal(got, P.g1_vec_to_np(want))


def test_arguments(plk, gpu_ctx):
    lib = plk.plonk._lib()
    pts = K.gen_mul_np([1, 2])
    out = np.zeros_like(pts)
    ptr = plk.plonk._ptr
    assert lib.plk_debug_g1_ntt(gpu_ctx.handle, ptr(pts), 1, 0, ptr(out)) == plk.PLK_E_ARG
    assert lib.plk_debug_g1_ntt(gpu_ctx.handle, ptr(pts), 21, 1, ptr(out)) == plk.PLK_E_ARG
    assert lib.plk_debug_g1_ntt(gpu_ctx.handle, None, 1, 1, ptr(out)) == plk.PLK_E_ARG
    bad = pts.copy()
    bad[1, 0] ^= np.uint64(1)  # off the curve
    assert lib.plk_debug_g1_ntt(gpu_ctx.handle, ptr(bad), 1, 1, ptr(out)) == plk.PLK_E_ARG
