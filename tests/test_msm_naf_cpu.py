"""The row-table recoding's model (tests/msm_naf_ref.py) against the conditions the MSM relies on:
exact reconstruction, at most ceil(255 / (c + 1)) digits (never more than the window layout's W,
so the sort's buffers keep their size, and never more than the greedy walk), every digit odd with
|d| < 2^c at a position <= 254, and buckets balanced well enough for the Lagrange commit's guard.
The kernel's form of the walk (position and borrow over the unchanged half) equals the paper form.
"""
import random

import numpy as np
import pytest

import msm_naf_ref as N
import msm_stage_ref as M
import pyref as P

R = N.R
CS = (17, 20)


def check_digits(h, c, digits):
    assert sum(d << p for p, d in digits) == h, hex(h)
    assert len(digits) <= N.max_digits(c) <= len(P.msm_window_layout(c)), hex(h)
    assert len(digits) == N.greedy_count(h, c), hex(h)
    pos = [p for p, _ in digits]
    assert pos == sorted(set(pos)) and all(0 <= p <= 254 for p in pos), hex(h)
    assert all(d & 1 and abs(d) < 1 << c for _, d in digits), hex(h)


@pytest.mark.parametrize("c", CS)
def test_edge_scalars(c):
    for s in N.edge_scalars(c) + M.edge_scalars(P.msm_window_layout(c)):
        digits, neg = N.recode(s, c)
        h = R - s if neg else s
        assert 0 <= h <= N.HALF
        check_digits(h, c, digits)
        assert N.walk_bits(h, c) == digits, hex(s)
        assert (-1 if neg else 1) * sum(d << p for p, d in digits) % R == s % R


@pytest.mark.parametrize("c", CS)
def test_equal_runs_share_buckets(c):
    """A run of equal scalars is one recoding: every copy lands in the same buckets, and the
    entry codes differ in the scalar's index alone."""
    s = 0x0123456789ABCDEF0FEDCBA9876543210123456789ABCDEF0FEDCBA987654321 % R
    h = M.header(c=c, n_srs=64)
    ent = N.entries_of([s] * 9, h)
    per = len(ent) // 9
    assert per == len(N.recode(s, c)[0]) and len(ent) == 9 * per
    for i in range(9):
        for (b0, c0), (b, code) in zip(ent[:per], ent[i * per:(i + 1) * per]):
            assert b == b0 and code == c0 + i


@pytest.fixture(scope="module")
def halves():
    rng = random.Random(0x4E4146)
    return [rng.randrange(N.HALF + 1) for _ in range(1 << 17)]


@pytest.mark.parametrize("c", CS)
def test_uniform_scalars(halves, c):
    """2^17 seeded uniform halves: the conditions, the mean digit count, the fullest bucket.
    Bucket counts scale with the number of scalars, so the guard's 256 entries per bucket at 2^20
    scalars and c = 20 (commit.hip lagrange_bucket_max) is 32 here; at c = 17 (an SRS below 2^20
    points) 2^17 scalars are a dense column as it stands, under the same guard of 256."""
    counts = np.zeros(1 << (c - 1), dtype=np.int64)
    total = 0
    for i, h in enumerate(halves):
        digits = N.walk(h, c)
        check_digits(h, c, digits)
        if i < 2048:
            assert N.walk_bits(h, c) == digits
        total += len(digits)
        for _, d in digits:
            counts[(abs(d) - 1) // 2] += 1
    mean_digits = total / len(halves)
    fullest, mean = int(counts.max()), total / len(counts)
    print(f"\n[msm-naf] c {c}: digits per scalar {mean_digits:.3f}, fullest bucket {fullest}, "
          f"mean {mean:.2f}, 512-bucket bins max/avg "
          f"{counts.reshape(-1, 512).sum(axis=1).max() / (512 * mean):.2f}")
    # the sliding window saves digits over the fixed grid: 255 / (c + 2) + 1 expected at most
    assert mean_digits < 255 / (c + 2) + 1 < len(P.msm_window_layout(c))
    assert fullest < (256 // 8 if c == 20 else 256)


def test_layout_policy_and_table_cap(plk, monkeypatch):
    """Which table an SRS is set up with (plk_msm_table_policy, no GPU): PLK_MSM_NAF = 1 asks for
    the row table and wide bucket sets alone get it, an SRS of 2^20 points and up takes it by
    default, 0 and PLK_MSM_C on its own keep the window table, and a row table above the injected cap falls back to the window table, as after a
    refused allocation, instead of failing the setup."""
    import ctypes as C

    def policy(n, c, c_from_env=0):
        naf, nbytes = C.c_uint32(), C.c_uint64()
        assert plk.plonk._lib().plk_msm_table_policy(n, c, c_from_env, C.byref(naf), C.byref(nbytes)) == plk.PLK_OK
        return bool(naf.value), nbytes.value

    n = (1 << 20) + 8
    monkeypatch.delenv("PLK_MSM_TABLE_CAP", raising=False)
    monkeypatch.setenv("PLK_MSM_NAF", "0")
    assert policy(n, 20) == (False, 13 * n * 97)
    monkeypatch.delenv("PLK_MSM_NAF")
    assert policy(n, 20, 1) == (False, 13 * n * 97)  # PLK_MSM_C alone: today's layout
    assert policy(n, 20) == (True, 255 * n * 97)  # the default from 2^20 points
    assert policy(1 << 20, 20)[0] and not policy((1 << 20) - 1, 17)[0] and not policy(1 << 16, 17)[0]
    monkeypatch.setenv("PLK_MSM_NAF", "1")
    assert policy(n, 20, 1) == (True, 255 * n * 97)
    assert policy(1 << 16, 17) == (True, 255 * (1 << 16) * 97)
    assert policy(1 << 14, 13) == (False, 20 * (1 << 14) * 97)  # a narrow set has no sum of the Y_r
    assert policy(1 << 24, 20)[0] is False  # 255 n would not fit the entry code's 31 bits
    monkeypatch.setenv("PLK_MSM_TABLE_CAP", str(255 * n * 96 - 1))
    assert policy(n, 20) == (False, 13 * n * 97)
    monkeypatch.setenv("PLK_MSM_TABLE_CAP", str(255 * n * 96))
    assert policy(n, 20) == (True, 255 * n * 97)
    assert plk.plonk._lib().plk_msm_table_policy(0, 20, 0, None, None) == plk.PLK_E_ARG
