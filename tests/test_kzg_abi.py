"""Argument checks of the KZG entries that come before any device use: they answer without a GPU.
(The same refusals on a live SRS, where a well-formed call succeeds, are in test_kzg_open_gpu.py.)"""
import ctypes as C

import numpy as np

import pyref as P

R = P.R_MOD


def fr_rows(vals, mont=True):
    return P.fr_vec_to_np(vals, mont=mont)


def test_null_arguments_are_refused(plk):
    lib, ptr = plk.plonk._lib(), plk.plonk._ptr
    f, z = fr_rows([1, 2, 3]), fr_rows([5])
    vals, wit = np.zeros((4, 4), dtype=np.uint64), np.zeros((4, 13), dtype=np.uint64)
    idx = C.c_uint64(7)
    assert lib.plk_kzg_open(None, ptr(f), 3, ptr(z), 1, ptr(vals), ptr(wit)) == plk.PLK_E_ARG
    assert lib.plk_kzg_open_domain(None, 2, ptr(f), 3, ptr(vals), ptr(wit), C.byref(idx)) == plk.PLK_E_ARG
    assert idx.value == 0xFFFFFFFFFFFFFFFF  # no SRS point was looked at
    assert lib.plk_kzg_open_domain(None, 2, ptr(f), 3, ptr(vals), ptr(wit), None) == plk.PLK_E_ARG
    assert lib.plk_kzg_last_open_ms(None, None, None, None) == plk.PLK_E_ARG
    g = P.g1_vec_to_np([P.G1_GEN])
    pair = np.zeros((2, 13), dtype=np.uint64)
    assert lib.plk_kzg_fold(None, ptr(g), ptr(g), ptr(z), ptr(z), ptr(g), 1, None, ptr(pair)) == plk.PLK_E_ARG
    assert lib.plk_debug_g1_ntt(None, ptr(g), 0, 1, ptr(g)) == plk.PLK_E_ARG


def test_shapes_and_scalars_are_refused_before_the_srs_is_touched(plk):
    """log_n 0 and 21, len > n and a scalar >= r: PLK_E_ARG whatever the SRS (here: none)."""
    lib, ptr = plk.plonk._lib(), plk.plonk._ptr
    f = fr_rows([1, 2, 3, 4, 5])
    vals, wit = np.zeros((8, 4), dtype=np.uint64), np.zeros((8, 13), dtype=np.uint64)
    for log_n, length in ((0, 1), (21, 5), (2, 5)):
        assert lib.plk_kzg_open_domain(None, log_n, ptr(f), length, ptr(vals), ptr(wit), None) == plk.PLK_E_ARG
    big = fr_rows([R, 1], mont=False)  # the plain words of r: not a canonical limb pattern
    assert lib.plk_kzg_open_domain(None, 1, ptr(big), 2, ptr(vals), ptr(wit), None) == plk.PLK_E_ARG
    z = fr_rows([5])
    assert lib.plk_kzg_open(None, ptr(big), 2, ptr(z), 1, ptr(vals), ptr(wit)) == plk.PLK_E_ARG
    assert lib.plk_kzg_open(None, ptr(f), 5, ptr(big), 1, ptr(vals), ptr(wit)) == plk.PLK_E_ARG


def test_python_surface(plk):
    for name in ("open", "open_domain", "open_multiple"):
        assert callable(getattr(plk.PlonkParams, name))
    for name in ("fold_openings", "check_openings"):
        assert callable(getattr(plk.OpeningKey, name))
    assert callable(plk.kzg_last_open_ms) and callable(plk.debug_g1_ntt)
    for sym in ("plk_kzg_open", "plk_kzg_open_domain", "plk_kzg_last_open_ms", "plk_kzg_fold",
                "plk_debug_g1_ntt"):
        assert sym in plk.ABI_SYMBOLS
