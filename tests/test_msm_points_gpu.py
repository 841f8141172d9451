"""GPU parity of the variable-base MSM (plk_msm_points, csrc/msm_var.hip): canonical affine
outputs bit-exact against the C oracle's Jacobian Pippenger (tests/oracle_lib.py) over the
sizes at which the kernels change shape (one task / several tasks per bucket, one / several
workgroups of the sort, every window size the cost model picks up to 2^16 + 1 points), the
scalars at the edges of the signed-digit recoding, and the exceptional cases of the group law
(repeated points, P and -P, identity inputs, an identity result); the curve check; and the
batched form over disjoint ranges of one point array.
"""
import numpy as np
import pytest

import g1_ingest_ref as ref
import pyref as P
from oracle_lib import random_fr

pytestmark = pytest.mark.gpu

R = P.R_MOD
N_MAX = (1 << 16) + 1
IDENTITY = np.array([0] * 12 + [1], dtype=np.uint64)


@pytest.fixture(scope="module")
def points(plk, gpu_ctx):
    """2^16 + 1 distinct points in no particular order (SRS powers, shuffled)."""
    tau = random_fr(1, seed=0xA11)[0]
    pp = plk.PlonkParams.setup(16, tau, gpu_ctx, n_points=N_MAX)
    pts = pp.points()
    return pts[np.random.Generator(np.random.PCG64(5)).permutation(N_MAX)]


def mont(vals):
    return P.fr_vec_to_np([v % R for v in vals])


EDGE = [0, 1, R - 1, (R - 1) // 2, (R + 1) // 2]


def scalars_for(n, seed):
    """Random scalars with the recoding's edge values 0, 1, r - 1, (r - 1) / 2, (r + 1) / 2 in
    front (as many as fit)."""
    sc = random_fr(max(n, 1), seed=seed)[:n].copy()
    k = min(n, len(EDGE))
    if k:
        sc[:k] = mont(EDGE[:k])
    return sc


def neg(words):
    x, y = P.g1_vec_from_np(words.reshape(1, 13))[0]
    return P.g1_vec_to_np([(x, (P.P_MOD - y) % P.P_MOD)])[0]


@pytest.mark.parametrize("n", [0, 1, 2, 27, 63, 64, 65, 4099, N_MAX])
def test_msm_points_vs_oracle(plk, gpu_ctx, oracle, points, n):
    sc = scalars_for(n, seed=n + 1)
    got = plk.msm_points(points[:n], sc, gpu_ctx).words
    want = oracle.msm(points[:n], sc) if n else IDENTITY
    assert np.array_equal(got, want)


@pytest.mark.parametrize("value", EDGE)
def test_single_edge_scalar(plk, gpu_ctx, oracle, points, value):
    sc = mont([value] * 5)
    got = plk.msm_points(points[:5], sc, gpu_ctx).words
    assert np.array_equal(got, oracle.msm(points[:5], sc))


def test_all_equal_scalars_overflow_one_task(plk, gpu_ctx, oracle, points):
    """300 points under one scalar: every window's entries share a bucket, more than a task
    holds."""
    sc = np.repeat(random_fr(1, seed=77), 300, axis=0)
    got = plk.msm_points(points[:300], sc, gpu_ctx).words
    assert np.array_equal(got, oracle.msm(points[:300], sc))


def test_repeated_points_take_the_doubling_path(plk, gpu_ctx, oracle, points):
    """The same point many times under the same scalar: the accumulation adds P to P."""
    pts = np.repeat(points[3:4], 70, axis=0)
    sc = np.repeat(random_fr(1, seed=78), 70, axis=0)
    got = plk.msm_points(pts, sc, gpu_ctx).words
    assert np.array_equal(got, oracle.msm(pts, sc))
    # and under different scalars, mixed with other points
    pts = np.concatenate([pts[:20], points[100:130], pts[:20]])
    sc = scalars_for(70, seed=79)
    got = plk.msm_points(pts, sc, gpu_ctx).words
    assert np.array_equal(got, oracle.msm(pts, sc))


def test_opposite_points_cancel(plk, gpu_ctx, oracle, points):
    s = random_fr(1, seed=80)
    pair = np.stack([points[7], neg(points[7])])
    got = plk.msm_points(pair, np.repeat(s, 2, axis=0), gpu_ctx)
    assert got.is_identity and np.array_equal(got.words, IDENTITY)
    # the pair inside a larger sum contributes nothing
    pts = np.concatenate([pair, points[200:240]])
    sc = np.concatenate([np.repeat(s, 2, axis=0), random_fr(40, seed=81)])
    got = plk.msm_points(pts, sc, gpu_ctx).words
    assert np.array_equal(got, oracle.msm(points[200:240], sc[2:]))


def test_identity_inputs_and_identity_result(plk, gpu_ctx, oracle, points):
    pts = points[:50].copy()
    sc = random_fr(50, seed=82)
    holes = [0, 17, 49]
    pts[holes] = IDENTITY
    keep = [i for i in range(50) if i not in holes]
    got = plk.msm_points(pts, sc, gpu_ctx).words
    assert np.array_equal(got, oracle.msm(points[keep], sc[keep]))
    # nothing but identity inputs, and nothing but zero scalars
    assert plk.msm_points(np.tile(IDENTITY, (9, 1)), sc[:9], gpu_ctx).is_identity
    assert plk.msm_points(points[:9], np.zeros((9, 4), dtype=np.uint64), gpu_ctx).is_identity


def test_off_curve_point_is_rejected(plk, gpu_ctx, points):
    pts = points[:40].copy()
    pts[23, 6] ^= np.uint64(1)  # y limb 0
    with pytest.raises(plk.PlonkError) as e:
        plk.msm_points(pts, random_fr(40, seed=83), gpu_ctx)
    assert e.value.status == plk.PLK_E_ARG
    pts = points[:40].copy()
    pts[5, 12] = 2  # an infinity word that is neither 0 nor 1
    with pytest.raises(plk.PlonkError) as e:
        plk.msm_points(pts, random_fr(40, seed=83), gpu_ctx)
    assert e.value.status == plk.PLK_E_ARG


def test_two_ranges_in_one_batch_equal_two_calls(plk, gpu_ctx, oracle, points):
    """The form the verifier's fold uses: two sums of very different lengths over disjoint
    ranges of one point array."""
    n = 16 + 11 * 37 + 2 * 37
    split = 16 + 11 * 37
    sc = scalars_for(n, seed=84)
    both = plk.msm_points_ranges(points[:n], sc, [(0, split), (split, n - split)], gpu_ctx)
    assert np.array_equal(both[0].words, plk.msm_points(points[:split], sc[:split], gpu_ctx).words)
    assert np.array_equal(both[1].words, plk.msm_points(points[split:n], sc[split:], gpu_ctx).words)
    assert np.array_equal(both[0].words, oracle.msm(points[:split], sc[:split]))
    assert np.array_equal(both[1].words, oracle.msm(points[split:n], sc[split:]))
    # an empty range beside a full one
    one = plk.msm_points_ranges(points[:n], sc, [(0, 0), (5, 60)], gpu_ctx)
    assert one[0].is_identity
    assert np.array_equal(one[1].words, oracle.msm(points[5:65], sc[5:65]))


# ---- the plk_g1 input rules, at the first lane, a wave's last lane and the next wave's first ----
@pytest.fixture(scope="module")
def abi_batch():
    """65 points of G1 and 65 scalars as Python integers, with each term's product."""
    rng = P.SplitMix64(0xAB1)
    step, acc, pts = ref.member(0x9E3779B97F4A7C15), ref.member(3), []
    for _ in range(65):
        pts.append(acc)
        acc = P.g1_add(acc, step)
    ks = [rng.fr() for _ in range(65)]
    return pts, ks, [P.g1_mul(pt, k) for pt, k in zip(pts, ks)]


@pytest.mark.parametrize("lane", ref.ABI_LANES)
@pytest.mark.parametrize("what", ref.ABI_REFUSED)
def test_malformed_point_is_refused(plk, gpu_ctx, abi_batch, what, lane):
    pts = P.g1_vec_to_np(abi_batch[0])
    pts[lane] = ref.abi_spoil(pts[lane], what)
    with pytest.raises(plk.PlonkError) as e:
        plk.msm_points(pts, P.fr_vec_to_np(abi_batch[1]), gpu_ctx)
    assert e.value.status == plk.PLK_E_ARG


@pytest.mark.parametrize("lane", ref.ABI_LANES)
def test_identity_word_hides_the_coordinates(plk, gpu_ctx, abi_batch, lane):
    points, ks, terms = abi_batch
    pts = P.g1_vec_to_np(points)
    pts[lane] = ref.abi_spoil(pts[lane], ref.ABI_IDENTITY)
    want = None
    for i, t in enumerate(terms):
        if i != lane:
            want = P.g1_add(want, t)
    got = plk.msm_points(pts, P.fr_vec_to_np(ks), gpu_ctx).words
    assert np.array_equal(got, P.g1_vec_to_np([want])[0])
