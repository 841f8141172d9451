"""The batched transform over G1 (csrc/g1_ntt.hip g1_ntt_run_batch) through
plk_debug_g1_ntt_batch: `batch` transforms laid out one after the other, one launch per level over
all of them, against plk_debug_g1_ntt run block by block (itself held to the integers by
test_g1_ntt_gpu.py). Bit for bit, both directions, both forms of the twiddle multiplication.

Sizes 2, 8 and 64 points; batches of 1 (the single transform's own path), 3 (odd, and with 2 points
less than one wave of butterflies in all) and 64 (with 64 points: 2048 butterflies, 16 blocks of
the butterfly kernels, so a kernel block holds lanes of several transforms). The blocks differ from
one another and hold identities, repeated points and P, -P pairs."""
import functools

import numpy as np
import pytest

import kzg_ref as K
import pyref as P

pytestmark = pytest.mark.gpu

R = P.R_MOD


@functools.lru_cache(maxsize=None)
def pool():
    """200 points P_i, their negatives and the identity, as ABI rows."""
    rng = P.SplitMix64(2024)
    logs = [rng.fr() for _ in range(200)]
    return K.gen_mul_np(logs + [R - x for x in logs] + [0])


def blocks(k: int, batch: int) -> np.ndarray:
    rng = np.random.default_rng(100 * k + batch)
    pts = pool()
    idx = rng.integers(0, pts.shape[0], size=batch << k)
    n = 1 << k
    if batch > 1:
        idx[n:2 * n] = idx[n]  # one block of one repeated point: doublings and identity differences
        idx[2 * n:3 * n] = 400  # one block of identities
    return pts[idx]


@pytest.fixture(params=["xyzz", "glv"])
def form(request, monkeypatch):
    monkeypatch.setenv("PLK_G1_NTT_FORM", request.param)  # read by the library at every call
    return request.param


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("batch", [1, 3, 64])
@pytest.mark.parametrize("k", [1, 3, 6])
def test_batch_equals_the_single_transform_block_by_block(plk, gpu_ctx, form, k, batch, direction):
    n = 1 << k
    pts = blocks(k, batch)
    got = plk.debug_g1_ntt_batch(pts, k, batch, direction, gpu_ctx)
    if batch == 1:
        assert np.array_equal(got, plk.debug_g1_ntt(pts, k, direction, gpu_ctx))
        return
    for b in range(batch):
        want = plk.debug_g1_ntt(pts[b * n:(b + 1) * n], k, direction, gpu_ctx)
        assert np.array_equal(got[b * n:(b + 1) * n], want), b


def test_batch_of_one_point_transforms_and_round_trip(plk, gpu_ctx, form):
    pts = blocks(0, 5)
    assert np.array_equal(plk.debug_g1_ntt_batch(pts, 0, 5, 1, gpu_ctx), pts)
    pts = blocks(3, 3)
    fwd = plk.debug_g1_ntt_batch(pts, 3, 3, 1, gpu_ctx)
    assert np.array_equal(plk.debug_g1_ntt_batch(fwd, 3, 3, -1, gpu_ctx), pts)


def test_batch_arguments(plk, gpu_ctx):
    lib, ptr = plk.plonk._lib(), plk.plonk._ptr
    pts = blocks(1, 3)
    out = np.zeros_like(pts)
    assert lib.plk_debug_g1_ntt_batch(gpu_ctx.handle, ptr(pts), 1, 0, 1, ptr(out)) == plk.PLK_E_ARG
    assert lib.plk_debug_g1_ntt_batch(gpu_ctx.handle, ptr(pts), 1, 3, 0, ptr(out)) == plk.PLK_E_ARG
    assert lib.plk_debug_g1_ntt_batch(gpu_ctx.handle, ptr(pts), 20, 2, 1, ptr(out)) == plk.PLK_E_ARG
    assert lib.plk_debug_g1_ntt_batch(gpu_ctx.handle, None, 1, 3, 1, ptr(out)) == plk.PLK_E_ARG
    bad = pts.copy()
    bad[:] = pool()[7]
    bad[5, 6] ^= np.uint64(1)  # y of a finite point: off the curve
    assert lib.plk_debug_g1_ntt_batch(gpu_ctx.handle, ptr(bad), 1, 3, 1, ptr(out)) == plk.PLK_E_ARG
