"""Updating an SRS on the GPU (plk_srs_update / plk_srs_verify_update) against plk_srs_setup:
setup(tau).update(s) must equal setup(tau s) bit for bit. k_srs_powers (a 255-step ladder on the
packed field with the fixed generator) shares no multiplication code with k_g1_mul (the split, the
endomorphism table, the redundant-limb lazy law), so the one checks the other.

Sizes: 2 (the smallest legal), 3, 33 (over kBatchAff), 257 (over a wave and a block of the batch
inversion), 1 027, and 2^16 + 3 once (more blocks than CUs, a ragged tail).
"""
import numpy as np
import pytest

import g1_ingest_ref as ref
import pairing_ref as R
import pyref as P
import srs_update_ref as U

pytestmark = pytest.mark.gpu

p, r, Z = P.P_MOD, P.R_MOD, U.Z
TAU = 0x3A7D1F6B5C2E49081726354453627180F9EAD7C6B5A49382716F5E4D3C2B1A09 % r
S_RANDOM = U.random_scalars(2, 0x757064)
SCALARS = (1, 2, Z, r - 1, *S_RANDOM)
SIZES = (2, 3, 33, 257, 1027)
SEED = bytes(range(60, 92))
N = 257  # the size of the verdict tests
S1, S2 = S_RANDOM


def limbs(v):
    return P.fr_vec_to_np([v])[0]


def words(pt):
    return P.g1_vec_to_np([pt])[0]


def setup(plk, ctx, tau, n):
    return plk.PlonkParams.setup(0, limbs(tau), ctx, n_points=n)


def g2_row(q):
    (x0, x1), (y0, y1) = q
    f = lambda v: P.int_to_limbs(P.fp_to_mont(v), 6)  # noqa: E731
    return np.array(f(x0) + f(x1) + f(y0) + f(y1) + [0], dtype=np.uint64)


class World:
    """One honest SRS per size with its key, and one honest update of the N-point SRS."""

    def __init__(self, plk, ctx):
        self.plk, self.ctx = plk, ctx
        self.key = plk.OpeningKey.setup(TAU)
        self.pp = {n: setup(plk, ctx, TAU, n) for n in SIZES}
        self.new, self.new_key, self.witness = self.pp[N].update(self.key, S1)
        self.prev_tau = self.pp[N].points(1, 1)[0]
        self.new_words = self.new.points()


@pytest.fixture(scope="module")
def W(plk, gpu_ctx):
    return World(plk, gpu_ctx)


# ---- update equals setup ----------------------------------------------------------------------
@pytest.mark.parametrize("s", SCALARS)
@pytest.mark.parametrize("n", SIZES)
def test_update_equals_setup(plk, gpu_ctx, W, n, s):
    before = W.pp[n].points()
    new, new_key, witness = W.pp[n].update(W.key, s)
    fresh = setup(plk, gpu_ctx, TAU * s % r, n)
    assert new.n == n and np.array_equal(new.points(), fresh.points())
    assert np.array_equal(new.points(0, 1)[0], words(P.G1_GEN))
    assert np.array_equal(W.pp[n].points(), before)  # the input SRS is untouched
    want_key = plk.OpeningKey.setup(TAU * s % r)
    for got, exp in zip(new_key.points(), want_key.points()):
        assert np.array_equal(got, exp)
    assert np.array_equal(witness, plk.OpeningKey.setup(s).points()[1])
    v = new.verify(new_key, SEED)
    assert v.ok and v.verdict == plk.plonk.SRS_OK
    rng = np.random.Generator(np.random.PCG64(n))
    poly = plk.Coefficients(P.fr_vec_to_np([int.from_bytes(rng.bytes(40), "little") % r for _ in range(n)]))
    a, b = new.commit(poly), fresh.commit(poly)  # the new SRS is MSM-ready
    assert a.words.tobytes() == b.words.tobytes() and not a.is_identity
    assert plk.plonk.g1_mul_last_ms(gpu_ctx) > 0


def test_update_equals_setup_over_more_blocks_than_cus(plk, gpu_ctx, W):
    n = (1 << 16) + 3
    new, new_key, _ = setup(plk, gpu_ctx, TAU, n).update(W.key, S2)
    fresh = setup(plk, gpu_ctx, TAU * S2 % r, n)
    assert np.array_equal(new.points(), fresh.points())
    assert new.verify(new_key, SEED).ok


# ---- verdicts ---------------------------------------------------------------------------------
def test_an_honest_update_and_a_chain_of_two_verify(plk, gpu_ctx, W):
    v = W.new.verify_update(W.prev_tau, W.new_key, W.witness, SEED)
    assert v.ok and v.verdict == plk.plonk.SRS_OK and v.bad_index is None
    assert W.new.verify_update(W.prev_tau, W.new_key, W.witness).ok  # OS entropy for the fold
    second, key2, wit2 = W.new.update(W.new_key, S2)
    v = second.verify_update(W.new.points(1, 1)[0], key2, wit2, SEED)
    assert v.ok
    fresh = setup(plk, gpu_ctx, TAU * S1 * S2 % r, N)
    assert np.array_equal(second.points(), fresh.points())
    assert np.array_equal(key2.points()[1], plk.OpeningKey.setup(TAU * S1 * S2 % r).points()[1])
    # the first update's witness does not vouch for the second step
    assert second.verify_update(W.new.points(1, 1)[0], key2, W.witness, SEED).verdict == plk.plonk.SRS_LINK


def test_link_verdicts(plk, W):
    link = plk.plonk.SRS_LINK
    other = W.key.update(S2)[1]  # the witness of another s
    assert W.new.verify_update(W.prev_tau, W.new_key, other, SEED).verdict == link
    wrong_prev = words(ref.member(99))
    assert W.new.verify_update(wrong_prev, W.new_key, W.witness, SEED).verdict == link
    assert W.new.verify_update(words(None), W.new_key, W.witness, SEED).verdict == link
    v = W.new.verify_update(W.prev_tau, W.new_key, other, SEED)
    assert not v.ok and not v and v.bad_index is None


def twist_point_outside_g2():
    rng = np.random.Generator(np.random.PCG64(0x63))
    while True:
        x = (int.from_bytes(rng.bytes(48), "big") % p, int.from_bytes(rng.bytes(48), "big") % p)
        y = R.f2sqrt(R.f2add(R.f2mul(R.f2mul(x, x), x), (4, 4)))
        if y is not None:
            q = (x, y)
            assert R.g2_is_on_curve(q) and R.g2_mul(q, r) is not None
            return q


def test_witness_verdicts_and_the_order_of_classes(plk, gpu_ctx, W):
    wit = plk.plonk.SRS_WITNESS
    identity = np.zeros(25, dtype=np.uint64)
    identity[24] = 1
    assert W.new.verify_update(W.prev_tau, W.new_key, identity, SEED).verdict == wit
    outside = g2_row(twist_point_outside_g2())
    assert W.new.verify_update(W.prev_tau, W.new_key, outside, SEED).verdict == wit
    off_twist = W.witness.copy()
    off_twist[12] ^= np.uint64(1)
    assert W.new.verify_update(W.prev_tau, W.new_key, off_twist, SEED).verdict == wit
    # one point of the new SRS replaced before loading: the chain breaks
    tampered = W.new_words.copy()
    tampered[5] = words(ref.member(12345))
    bad = plk.PlonkParams.load(tampered, gpu_ctx)
    assert bad.verify_update(W.prev_tau, W.new_key, W.witness, SEED).verdict == plk.plonk.SRS_CHAIN
    # a bad witness AND a broken chain: the witness is looked at first
    assert bad.verify_update(W.prev_tau, W.new_key, identity, SEED).verdict == wit
    assert bad.verify_update(W.prev_tau, W.new_key, outside, SEED).verdict == wit


# ---- OS entropy -------------------------------------------------------------------------------
def test_two_updates_from_os_entropy_differ_and_verify(plk, W):
    pp = W.pp[33]
    prev = pp.points(1, 1)[0]
    a, ka, wa = pp.update(W.key)
    b, kb, wb = pp.update(W.key)
    pa, pb, p0 = a.points(), b.points(), pp.points()
    assert not np.array_equal(pa[1:], pb[1:]) and not np.array_equal(wa, wb)
    assert not np.array_equal(pa[1:], p0[1:]) and not np.array_equal(pb[1:], p0[1:])
    assert np.array_equal(pa[0], p0[0]) and np.array_equal(pb[0], p0[0])
    assert a.verify_update(prev, ka, wa).ok and b.verify_update(prev, kb, wb).ok
    assert a.verify_update(prev, ka, wb).verdict == plk.plonk.SRS_LINK
    assert a.verify_update(prev, kb, wa).verdict == plk.plonk.SRS_CHAIN


# ---- untrusted input --------------------------------------------------------------------------
def test_an_srs_with_a_non_member_refuses_the_update(plk, gpu_ctx, W):
    rng = np.random.Generator(np.random.PCG64(0x756E))
    w = W.pp[33].points().copy()
    w[5] = words(ref.non_member(10177, rng))
    w[9] = words(ref.non_member(859267, rng))
    loaded = plk.PlonkParams.load(w, gpu_ctx)
    with pytest.raises(plk.PlonkError) as e:
        loaded.update(W.key, S1)
    assert e.value.status == plk.PLK_E_ARG and e.value.bad_index == 5
    off = W.pp[33].points().copy()  # off the curve: the point pass names it
    off[7, 6] ^= np.uint64(1)
    with pytest.raises(plk.PlonkError) as e:
        plk.PlonkParams.load(off, gpu_ctx).update(W.key, S1)
    assert e.value.status == plk.PLK_E_ARG and e.value.bad_index == 7
    # the same points without the bad one update as usual
    good = plk.PlonkParams.load(W.pp[33].points(), gpu_ctx)
    new, _, _ = good.update(W.key, S1)
    assert np.array_equal(new.points(), setup(plk, gpu_ctx, TAU * S1 % r, 33).points())


@pytest.mark.parametrize("s", (0, r))
def test_zero_and_r_are_refused(plk, W, s):
    with pytest.raises(plk.PlonkError) as e:
        W.pp[33].update(W.key, s)
    assert e.value.status == plk.PLK_E_ARG and e.value.bad_index is None


def test_a_single_point_is_refused(plk, gpu_ctx, W):
    one = setup(plk, gpu_ctx, TAU, 1)
    with pytest.raises(plk.PlonkError) as e:
        one.update(W.key, S1)
    assert e.value.status == plk.PLK_E_ARG


# ---- bytes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ("compressed", "uncompressed"))
def test_the_path_of_a_ceremony_participant(plk, gpu_ctx, W, fmt):
    """Export, import somewhere else, verify the update there."""
    blob = W.new.to_bytes(fmt)
    h, bh = W.new_key.to_bytes(fmt)
    wit = plk.plonk.g2_to_bytes(W.witness, fmt)
    prev = W.pp[N].to_bytes(fmt, 1, 1)
    back = plk.PlonkParams.from_bytes(blob, fmt, True, gpu_ctx)
    key = plk.OpeningKey.from_bytes(h, bh, fmt)
    prev_pt = plk.PlonkParams.from_bytes(prev, fmt, True, gpu_ctx).points()[0]
    v = back.verify_update(prev_pt, key, plk.plonk.g2_from_bytes(wit, fmt), SEED)
    assert v.ok and v.verdict == plk.plonk.SRS_OK
    assert np.array_equal(back.points(), W.new_words)
