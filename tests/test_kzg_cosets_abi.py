"""The coset-opening entries without a GPU: the argument checks that come before any device use,
the Python surface, and the coset view of a domain's values (pure index arithmetic)."""
import ctypes as C

import numpy as np
import pytest

import pyref as P

R = P.R_MOD


def test_null_arguments_are_refused(plk):
    lib, ptr = plk.plonk._lib(), plk.plonk._ptr
    f, z = P.fr_vec_to_np([1, 2, 3]), P.fr_vec_to_np([5])
    vals, wit = np.zeros((4, 4), dtype=np.uint64), np.zeros((4, 13), dtype=np.uint64)
    idx = C.c_uint64(7)
    assert lib.plk_kzg_open_cosets(None, 2, 1, ptr(f), 3, ptr(vals), ptr(wit), C.byref(idx)) == plk.PLK_E_ARG
    assert idx.value == 0xFFFFFFFFFFFFFFFF  # no SRS point was looked at
    assert lib.plk_kzg_open_cosets(None, 2, 1, ptr(f), 3, ptr(vals), ptr(wit), None) == plk.PLK_E_ARG
    g = P.g1_vec_to_np([P.G1_GEN])
    pair = np.zeros((2, 13), dtype=np.uint64)
    assert lib.plk_kzg_fold_cosets(None, 0, ptr(g), ptr(z), ptr(z), ptr(g), 1, None, ptr(pair)) == plk.PLK_E_ARG
    assert lib.plk_debug_g1_colsum(None, ptr(g), 1, 1, ptr(g)) == plk.PLK_E_ARG
    assert lib.plk_debug_g1_ntt_batch(None, ptr(g), 0, 1, 1, ptr(g)) == plk.PLK_E_ARG


def test_python_surface(plk):
    for name in ("open_cosets", "power_key_matches"):
        assert callable(getattr(plk.PlonkParams, name))
    for name in ("fold_cosets", "check_cosets"):
        assert callable(getattr(plk.OpeningKey, name))
    assert callable(plk.debug_g1_colsum) and callable(plk.debug_g1_ntt_batch)
    for sym in ("plk_kzg_open_cosets", "plk_kzg_fold_cosets", "plk_debug_g1_colsum", "plk_debug_g1_ntt_batch"):
        assert sym in plk.ABI_SYMBOLS
    assert plk.plonk._lib().plk_abi_version() == 2


@pytest.mark.parametrize("k,log_l", [(1, 0), (1, 1), (3, 1), (4, 2), (4, 4), (5, 0)])
def test_coset_view_of_the_values(plk, k, log_l):
    n, l, r = 1 << k, 1 << log_l, 1 << (k - log_l)
    vals = plk.PointsValue(P.fr_vec_to_np(list(range(100, 100 + n))))
    rows = vals.cosets(log_l)
    assert rows.shape == (r, l, 4)
    for j in range(r):
        assert P.fr_vec_from_np(np.ascontiguousarray(rows[j])) == [100 + j + r * i for i in range(l)]
    with pytest.raises(ValueError):
        vals.cosets(k + 1)
