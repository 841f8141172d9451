"""The batched scalar multiplication of csrc/g1_mul.hip (plk_g1_mul_batch) against the plain
double-and-add of tests/g1_ingest_ref.py, and its device split against the host mirror.

Points: G, a few [k]G and the identity. Scalars: the edge list of tests/srs_update_ref.py (where a
quotient digit of the division by z could be off by one; 0 and 2z end the chain on the identity
and on a doubling) and seeded random values. Batch sizes cross kBatchAff = 32, a wave and a block.
The reference products are computed once (about 260 of them) and shared.
"""
import numpy as np
import pytest

import g1_ingest_ref as ref
import pyref as P
import srs_update_ref as U

pytestmark = pytest.mark.gpu

p, r, Z = P.P_MOD, P.R_MOD, U.Z
SIZES = (1, 33, 63, 64, 65, 129, 257)
IDENTITY_ROW = np.array([0] * 12 + [1], dtype=np.uint64)


def words(pt):
    return P.g1_vec_to_np([pt])[0]


@pytest.fixture(scope="module")
def cases():
    """257 (point, scalar, product): every point with every edge scalar, then random pairs."""
    points = [P.G1_GEN, ref.member(2), ref.member(0xDEADBEEFCAFEF00D), ref.member(r - 5), None]
    edge = U.edge_scalars()
    assert 0 in edge and r - 1 in edge and 2 * Z in edge
    pairs = [(pt, k) for k in edge for pt in points]
    rnd = U.random_scalars(2 * (max(SIZES) - len(pairs)), 0x6D756C)
    pairs += [(ref.member(rnd[2 * i] | 1), rnd[2 * i + 1]) for i in range(max(SIZES) - len(pairs))]
    assert len(pairs) == max(SIZES)
    return [(pt, k, ref.mul(pt, k) if pt is not None else None) for pt, k in pairs]


def run(plk, ctx, sel, assume):
    pts = P.g1_vec_to_np([c[0] for c in sel])
    ks = P.fr_vec_to_np([c[1] for c in sel])
    return plk.plonk.g1_mul(pts, ks, assume, ctx)


@pytest.mark.parametrize("n", SIZES)
def test_against_the_python_reference(plk, gpu_ctx, cases, n):
    off = (37 * n) % len(cases)  # another stretch of the case list per size
    sel = [cases[(off + i) % len(cases)] for i in range(n)]
    got = run(plk, gpu_ctx, sel, False)
    want = P.g1_vec_to_np([c[2] for c in sel])
    assert got.shape == (n, 13)
    for i in range(n):
        assert np.array_equal(got[i], want[i]), (n, i, hex(sel[i][1]))
    # the caller's word for membership changes nothing
    assert got.tobytes() == run(plk, gpu_ctx, sel, True).tobytes()
    assert plk.plonk.g1_mul_last_ms(gpu_ctx) > 0


def test_every_edge_scalar_on_every_point(plk, gpu_ctx, cases):
    """The 170 edge cases in one batch, and what the identity looks like."""
    sel = cases[:5 * len(U.edge_scalars())]
    assert len(sel) == 170
    got = run(plk, gpu_ctx, sel, False)
    for row, (pt, k, want) in zip(got, sel):
        assert np.array_equal(row, words(want)), hex(k)
        if pt is None or k == 0:
            assert want is None and np.array_equal(row, IDENTITY_ROW)
    assert sum(1 for c in sel if c[2] is None) >= 34 + 4


def test_empty_batch(plk, gpu_ctx):
    out = plk.plonk.g1_mul(np.zeros((0, 13), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64), False, gpu_ctx)
    assert out.shape == (0, 13)


def refused(plk, ctx, pts, ks, assume):
    with pytest.raises(plk.PlonkError) as e:
        plk.plonk.g1_mul(pts, ks, assume, ctx)
    return e.value.status == plk.PLK_E_ARG


def test_refusals(plk, gpu_ctx):
    rng = np.random.Generator(np.random.PCG64(0x6E6D))
    good = [ref.member(3), P.G1_GEN, None, ref.member(11)]
    pts = P.g1_vec_to_np(good)
    ks = P.fr_vec_to_np([5, 6, 7, 8])
    assert np.array_equal(plk.plonk.g1_mul(pts, ks, False, gpu_ctx),
                          P.g1_vec_to_np([ref.mul(a, k) for a, k in zip(good, (5, 6, 7, 8))]))
    # a curve point outside G1: refused unless the caller vouches for it
    bad = pts.copy()
    bad[1] = words(ref.non_member(10177, rng))
    assert refused(plk, gpu_ctx, bad, ks, False)
    plk.plonk.g1_mul(bad, ks, True, gpu_ctx)  # no membership test: the call goes through
    for assume in (False, True):
        off = pts.copy()  # off the curve
        off[3, 6] ^= np.uint64(1)
        assert refused(plk, gpu_ctx, off, ks, assume)
        big = pts.copy()  # x = p in "Montgomery" limbs: not canonical
        big[0, :6] = np.array(P.int_to_limbs(p, 6), dtype=np.uint64)
        assert refused(plk, gpu_ctx, big, ks, assume)
        inf2 = pts.copy()
        inf2[2, 12] = 2
        assert refused(plk, gpu_ctx, inf2, ks, assume)
        ks_bad = ks.copy()  # a scalar >= r
        ks_bad[1] = np.array(P.int_to_limbs(r, 4), dtype=np.uint64)
        assert refused(plk, gpu_ctx, pts, ks_bad, assume)


def test_device_split_equals_the_host_mirror(plk, gpu_ctx):
    scalars = U.edge_scalars() + U.random_scalars(2000, 0x5717)
    vals = P.fr_vec_to_np(scalars)
    dev = plk.plonk.debug_glv_split(vals, gpu_ctx)
    assert np.array_equal(dev, plk.plonk.debug_glv_split(vals))
    assert np.array_equal(dev, U.split_rows(scalars))


# ---- the plk_g1 input rules, at the first lane, a wave's last lane and the next wave's first ----
@pytest.fixture(scope="module")
def abi_batch(cases):
    """65 of the random (finite point, scalar, product) cases."""
    sel = cases[5 * len(U.edge_scalars()):][:65]
    assert len(sel) == 65 and all(c[0] is not None for c in sel)
    return sel


@pytest.mark.parametrize("assume", [False, True])
@pytest.mark.parametrize("lane", ref.ABI_LANES)
@pytest.mark.parametrize("what", ref.ABI_REFUSED)
def test_malformed_point_is_refused(plk, gpu_ctx, abi_batch, what, lane, assume):
    pts = P.g1_vec_to_np([c[0] for c in abi_batch])
    pts[lane] = ref.abi_spoil(pts[lane], what)
    assert refused(plk, gpu_ctx, pts, P.fr_vec_to_np([c[1] for c in abi_batch]), assume)


@pytest.mark.parametrize("assume", [False, True])
@pytest.mark.parametrize("lane", ref.ABI_LANES)
def test_identity_word_hides_the_coordinates(plk, gpu_ctx, abi_batch, lane, assume):
    pts = P.g1_vec_to_np([c[0] for c in abi_batch])
    pts[lane] = ref.abi_spoil(pts[lane], ref.ABI_IDENTITY)
    want = P.g1_vec_to_np([c[2] for c in abi_batch])
    want[lane] = IDENTITY_ROW
    got = plk.plonk.g1_mul(pts, P.fr_vec_to_np([c[1] for c in abi_batch]), assume, gpu_ctx)
    assert np.array_equal(got, want)
