"""The MSM stage model (tests/msm_stage_ref.py) against the definition, without a GPU: for every
window size the library takes, the model's recoding rebuilds each scalar, and its stage chain
(sort layout -> partials -> bucket or run sums -> bit sums -> host tail) over a layout of its own
ends at pyref.msm_naive. The model's checks of a device layout must also refuse wrong layouts."""
import random

import numpy as np
import pytest

import msm_stage_ref as M
import pyref as P

N = 32
TAU = 0x1234567890ABCDEF1234567890ABCDEF % P.R_MOD
CS = [c for c in range(8, 23) if c != 21]


@pytest.fixture(scope="module")
def srs():
    pts = P.srs_setup(TAU, N)
    return pts, [pow(TAU, i, P.R_MOD) for i in range(N)]


def scalars_for(c):
    lay = P.msm_window_layout(c)
    edges = M.edge_scalars(lay)
    rng = random.Random(100 + c)
    return lay, (edges + [rng.randrange(P.R_MOD) for _ in range(N)])[:N]


def test_edge_scalars_hit_their_digits():
    """The patterns do what their names say, on a layout with narrow windows (c = 13) and one
    without (c = 15)."""
    for c in (13, 15):
        lay = P.msm_window_layout(c)
        e = M.edge_halves(lay)
        d, _ = M.recode(e["last_bucket"], lay)
        assert all(abs(x) == 1 << (c - 1) for _, x in d[:-2])  # bucket B - 1, no carry
        d, _ = M.recode(e["carry_each"], lay)
        assert all(x < 0 for _, x in d[:-2])
        d, _ = M.recode(e["all_ones"], lay)
        assert d[0][1] == -1 and sum(1 for _, x in d if x == 0) >= len(lay) - 3
        d, _ = M.recode(e["under_carry_even"], lay)
        assert all(x == (1 << (c - 1)) for _, x in d[1:-2:2])
        assert len(M.edge_scalars(lay)) <= N


@pytest.mark.parametrize("c", CS)
def test_recoding_rebuilds_every_scalar(c):
    lay, sc = scalars_for(c)
    B = 1 << (P.msm_effective_c(c) - 1)
    for s in sc:
        digits, neg = M.recode(s, lay)
        assert M.rebuild(digits, neg, lay) == s % P.R_MOD
        assert all(abs(d) <= B for _, d in digits)
        assert M.scalar_half(s)[0] <= M.HALF


@pytest.mark.parametrize("c", CS)
def test_stage_chain_ends_at_msm_naive(srs, c):
    pts, dlog = srs
    lay, sc = scalars_for(c)
    want = P.msm_naive(pts, sc)
    wide = (1 << (P.msm_effective_c(c) - 1)) > 32768
    for chunk, rb in ((8, 4), (3, 1)) if wide else ((8, 4), (1, 4), (5, 4)):
        h = M.header(c=c, n_srs=N, chunk=chunk, rb=rb)
        off, srt, toff, tasks = M.build_device_layout(sc, h)
        M.check_sorted(M.entries_of(sc, h), off, srt, h["B"])
        M.check_tasks(h, off, toff, tasks)
        out = M.model_chain(h, dlog, off, srt, toff, tasks)
        assert out["final"] == M.direct_dlog(h, dlog, sc)
        assert M.affine_dlog(out["final"]) == want, (c, chunk, rb)


@pytest.mark.parametrize("c,parts", [(17, 2), (17, 4), (20, 8), (20, 32)])
def test_parts_sum_to_the_whole(srs, c, parts):
    pts, dlog = srs
    lay, sc = scalars_for(c)
    total = 0
    for part in range(parts):
        h = M.header(c=c, n_srs=N, chunk=64, rb=4, part=part, parts=parts)
        off, srt, toff, tasks = M.build_device_layout(sc, h)
        out = M.model_chain(h, dlog, off, srt, toff, tasks)
        assert out["final"] == M.direct_dlog(h, dlog, sc), part
        total += out["final"]
    assert total % P.R_MOD == sum(s * q for s, q in zip(sc, dlog)) % P.R_MOD
    if parts == 2:  # pyref's own statement of a share, on points
        h = M.header(c=c, n_srs=N, part=1, parts=parts)
        assert M.affine_dlog(M.direct_dlog(h, dlog, sc)) == P.msm_bucket_part(pts, sc, c, 1, parts)


def test_tally_names_the_exceptional_additions():
    """tau = 1 and equal scalars: every table point of a window is the same multiple of G."""
    h = M.header(c=10, n_srs=4, chunk=8)
    s = 5
    for dlog, want in (([1, 1, 1, 1], "equal"), ([1, P.R_MOD - 1, 1, 0], "opposite")):
        off, srt, toff, tasks = M.build_device_layout([s] * 4, h)
        t = M.model_chain(h, dlog, off, srt, toff, tasks)["tally"].n["accumulate"]
        assert t[want] >= 1, dict(t)
    assert t["operand_inf"] >= 1 and t["acc_inf"] >= 1 and t["result_inf"] >= 1


def test_checks_refuse_wrong_layouts():
    c = 10
    lay, sc = scalars_for(c)
    sc = sc + [sc[-1]] * 20  # a bucket with more than one task
    h = M.header(c=c, n_srs=len(sc), chunk=8)
    off, srt, toff, tasks = M.build_device_layout(sc, h)
    buckets = M.entries_of(sc, h)
    M.check_sorted(buckets, off, srt, h["B"])
    first, length, _ = M.check_tasks(h, off, toff, tasks)
    assert length.max() == 8 and length.min() < 8
    bad = tasks.copy()  # the length field holding length instead of length - 1, on one tail
    i = int(np.argmin(length))
    bad[i, 1] += 1 << M.TASK_SHIFT
    with pytest.raises(AssertionError):
        M.check_tasks(h, off, toff, bad)
    bad = tasks.copy()  # two records swapped across the full / tail boundary
    j = int(np.argmax(length))
    bad[[i, j]] = bad[[j, i]]
    with pytest.raises(AssertionError):
        M.check_tasks(h, off, toff, bad)
    bad = srt.copy()  # an entry with its sign flipped
    bad[0] ^= M.SIGN
    with pytest.raises(AssertionError):
        M.check_sorted(buckets, off, bad, h["B"])
    bad = srt.copy()  # two entries of different buckets exchanged: counts unchanged
    a, b = int(off[np.nonzero(np.diff(off))[0][0]]), int(off[h["B"]]) - 1
    bad[[a, b]] = bad[[b, a]]
    with pytest.raises(AssertionError):
        M.check_sorted(buckets, off, bad, h["B"])
