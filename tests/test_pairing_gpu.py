"""The batched pairing kernel (csrc/pairing.hip k_pairing) against the fixture, the host code and
the G1 equation C == tau W: the values bit for bit at one lane, a full wave, one lane over and
more than two waves with points at infinity among them; the verdicts of plk_pairing_check_batch
at counts around the wave size with wrong pairs at the first, wave-boundary and last positions.
"""
import numpy as np
import pytest

import g1_ingest_ref as ref
import pairing_tower_ops as T
import pyref as P
from make_pairing_vectors import OUT

pytestmark = pytest.mark.gpu

TAU = 0x6C1F2E3D4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978


@pytest.fixture(scope="module")
def vec():
    return dict(np.load(OUT, allow_pickle=False))


@pytest.fixture(scope="module")
def points(vec):
    """130 G1 points: the fixture's three P whose Q is H first, then k G."""
    pts = [P.g1_mul(P.G1_GEN, k) for k in range(2, 129)]
    return np.concatenate([vec["p"][[0, 1, 6]], P.g1_vec_to_np(pts)])


@pytest.mark.parametrize("i", range(8))
def test_one_lane_equals_the_fixture(plk, gpu_ctx, vec, i):
    got = plk.debug_pairing(vec["p"][i:i + 1], vec["q"][i], gpu_ctx)
    assert np.array_equal(got[0], vec["value"][i])


@pytest.mark.parametrize("n", [64, 65, 130])
def test_kernel_equals_host_and_fixture(plk, gpu_ctx, vec, points, n):
    pts = points[:n].copy()
    infinite = [0, 63, 64, 129] if n == 130 else []
    for k in infinite:
        pts[k] = 0
        pts[k, 12] = 1
    h = vec["q"][0]
    got = plk.debug_pairing(pts, h, gpu_ctx)
    assert np.array_equal(got, plk.debug_pairing(pts, h))
    for row, k in ((0, 0), (1, 1), (2, 6)):
        if row not in infinite:
            assert np.array_equal(got[row], vec["value"][k])
    one = np.zeros(72, dtype=np.uint64)
    one[:6] = P.int_to_limbs(P.fp_to_mont(1), 6)
    for k in infinite:
        assert np.array_equal(got[k], one)


@pytest.fixture(scope="module")
def honest():
    """65 honest pairs (tau s_j G, s_j G) as affine points."""
    rng = P.SplitMix64(0xBA7C4)
    out = []
    for _ in range(65):
        w = P.g1_mul(P.G1_GEN, rng.fr())
        out.append((P.g1_mul(w, TAU), w))
    return out


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_check_batch(plk, gpu_ctx, honest, count):
    pairs = list(honest[:count])
    wrong = sorted({k for k in (0, 63, 64, count - 1) if k < count})
    if count == 1:
        wrong = [0]
    for k in wrong:
        pairs[k] = (P.g1_add(pairs[k][0], P.G1_GEN), pairs[k][1])
    if count > 8:
        pairs[3] = (None, None)          # accepted
        pairs[5] = (pairs[5][0], None)   # (finite, infinity): rejected
        pairs[7] = (None, pairs[7][1])   # (infinity, finite): rejected
    words = np.stack([P.g1_vec_to_np([c, w]) for c, w in pairs])
    key = plk.OpeningKey.setup(TAU)
    got = key.check_batch(words, gpu_ctx)
    assert got.dtype == bool and got.shape == (count,)
    assert list(got) == [c == P.g1_mul(w, TAU) for c, w in pairs]
    assert list(got) == [key.check(words[j]) for j in range(count)]
    for k in wrong:
        assert not got[k]
    if count == 1:  # and the honest pair alone
        assert list(key.check_batch(np.stack([P.g1_vec_to_np(list(honest[0]))]), gpu_ctx)) == [True]


@pytest.mark.parametrize("first", [0, 3])
def test_check_batch_with_points_outside_the_subgroup(plk, gpu_ctx, honest, first):
    """The pairs of test_pairing_cpu's test_check_with_points_outside_the_subgroup (the order-3
    point (0, 2) in C, in W, in both) at lanes 0, 63 and 64 of 65 pairs: the kernel's verdicts
    are the host check's, pair by pair, and a wrong pair moved by T stays wrong."""
    odd = T.off_subgroup_pairs(TAU, honest[0][1])
    pairs = list(honest)
    for i, lane in enumerate(ref.ABI_LANES):
        pairs[lane] = odd[(first + i) % len(odd)][1]
    c, w = honest[9]
    pairs[9] = (P.g1_add(P.g1_add(c, P.G1_GEN), T.T3), w)
    words = np.stack([P.g1_vec_to_np([c, w]) for c, w in pairs])
    key = plk.OpeningKey.setup(TAU)
    got = key.check_batch(words, gpu_ctx)
    assert list(got) == [key.check(words[j]) for j in range(65)]
    assert not got[9] and all(got[lane] for lane in ref.ABI_LANES)


def test_check_batch_refuses_malformed_points(plk, gpu_ctx, honest):
    words = np.stack([P.g1_vec_to_np(list(pr)) for pr in honest[:3]])
    words[1, 1, 6] ^= np.uint64(1)  # W of pair 1 leaves the curve
    key = plk.OpeningKey.setup(TAU)
    with pytest.raises(plk.PlonkError) as err:
        key.check_batch(words, gpu_ctx)
    assert err.value.status == plk.PLK_E_ARG


# ---- the plk_g1 input rules of plk_pairing_check_batch, on C and on W --------------------------
@pytest.mark.parametrize("lane", ref.ABI_LANES)
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("what", ref.ABI_REFUSED)
def test_check_batch_refuses_a_malformed_point(plk, gpu_ctx, honest, what, which, lane):
    words = np.stack([P.g1_vec_to_np(list(pr)) for pr in honest])
    words[lane, which] = ref.abi_spoil(words[lane, which], what)
    with pytest.raises(plk.PlonkError) as err:
        plk.OpeningKey.setup(TAU).check_batch(words, gpu_ctx)
    assert err.value.status == plk.PLK_E_ARG


@pytest.mark.parametrize("lane", ref.ABI_LANES)
def test_check_batch_identity_word_hides_the_coordinates(plk, gpu_ctx, honest, lane):
    """(O, O) holds and (O, W) does not, whatever the identity's coordinate words are."""
    words = np.stack([P.g1_vec_to_np(list(pr)) for pr in honest])
    key = plk.OpeningKey.setup(TAU)
    words[lane, 0] = ref.abi_spoil(words[lane, 0], ref.ABI_IDENTITY)
    assert list(key.check_batch(words, gpu_ctx)) == [j != lane for j in range(65)]
    words[lane, 1] = ref.abi_spoil(words[lane, 1], ref.ABI_IDENTITY)
    assert list(key.check_batch(words, gpu_ctx)) == [True] * 65
