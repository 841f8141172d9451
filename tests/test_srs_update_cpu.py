"""The host side of the SRS update (include/plk.h "Updating an SRS"): the scalar split's host
mirror against Python integers, the opening key's update against a fresh setup, the G2 byte pair
and the binding. Needs no GPU.
"""
import numpy as np
import pytest

import g1_ingest_ref as ref
import pyref as P
import srs_update_ref as U

r, Z = U.r, U.Z
TAU = 0x3A7D1F6B5C2E49081726354453627180F9EAD7C6B5A49382716F5E4D3C2B1A09 % r
NEW_SYMBOLS = ("plk_g1_mul_batch", "plk_g1_mul_last_ms", "plk_opening_key_update", "plk_srs_update",
               "plk_srs_verify_update", "plk_g2_to_bytes", "plk_g2_from_bytes", "plk_debug_glv_split")


def test_symbols_are_declared(plk):
    lib = plk.plonk._lib()
    for s in NEW_SYMBOLS:
        assert s in plk.ABI_SYMBOLS and hasattr(lib, s), s
    assert lib.plk_abi_version() == 2
    assert (plk.plonk.SRS_WITNESS, plk.plonk.SRS_LINK) == (6, 7)
    for name in ("g1_mul", "g1_mul_last_ms", "debug_glv_split", "g2_to_bytes", "g2_from_bytes"):
        assert callable(getattr(plk.plonk, name))
    assert callable(plk.PlonkParams.update) and callable(plk.PlonkParams.verify_update)
    assert callable(plk.OpeningKey.update)


def test_the_reference_chain_is_a_scalar_multiplication():
    """The model the kernel follows (split, table, 128 steps) against the plain double-and-add."""
    pt = ref.member(7)
    assert U.psi(P.G1_GEN) == ref.mul(P.G1_GEN, r - Z)  # (beta x, y) = [-z] P
    for k in (0, 1, 2, Z - 1, Z, Z + 1, 2 * Z, Z * (Z - 1) - 1, r - 2, r - 1, 1 << 128, 1 << 254,
              *U.random_scalars(4, 0x71)):
        assert U.chain_mul(pt, k) == ref.mul(pt, k), hex(k)


def test_host_split_against_python_integers(plk):
    scalars = U.edge_scalars() + U.random_scalars(2000, 0x5717)
    assert all(0 <= k < r for k in scalars)
    got = plk.plonk.debug_glv_split(P.fr_vec_to_np(scalars))
    assert got.shape == (len(scalars), 4)
    for k, row in zip(scalars, got):
        a = int(row[0]) | (int(row[1]) << 64)
        b = int(row[2]) | (int(row[3]) << 64)
        assert a == Z - k % Z and b == k // Z + 1, hex(k)
        assert 1 <= a <= Z and 1 <= b <= Z
        assert (a - b * Z) % r == -k % r
    assert np.array_equal(got, U.split_rows(scalars))


def test_split_refuses_a_non_canonical_scalar(plk):
    raw = np.array([[(r >> (64 * i)) & P.MASK64 for i in range(4)]], dtype=np.uint64)
    with pytest.raises(plk.PlonkError) as e:
        plk.plonk.debug_glv_split(raw)
    assert e.value.status == plk.PLK_E_ARG
    assert plk.plonk.debug_glv_split(np.zeros((0, 4), dtype=np.uint64)).shape == (0, 4)


@pytest.mark.parametrize("s", (1, 2, Z, r - 1, 0x1F2E3D4C5B6A79880796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F % r))
def test_opening_key_update_equals_a_fresh_setup(plk, s):
    key = plk.OpeningKey.setup(TAU)
    new, witness = key.update(s)
    want = plk.OpeningKey.setup(TAU * s % r)
    for got, exp in zip(new.points(), want.points()):
        assert np.array_equal(got, exp)
    assert np.array_equal(witness, plk.OpeningKey.setup(s).points()[1])
    # Montgomery limbs are taken as well as integers, and the input key is untouched
    again, w2 = key.update(P.fr_vec_to_np([s])[0])
    assert np.array_equal(again.points()[1], want.points()[1]) and np.array_equal(w2, witness)
    assert np.array_equal(key.points()[1], plk.OpeningKey.setup(TAU).points()[1])


@pytest.mark.parametrize("s", (0, r))
def test_opening_key_update_refuses_zero_and_r(plk, s):
    key = plk.OpeningKey.setup(TAU)
    with pytest.raises(plk.PlonkError) as e:
        key.update(s)
    assert e.value.status == plk.PLK_E_ARG


@pytest.mark.parametrize("fmt", ("compressed", "uncompressed"))
def test_witness_bytes_round_trip(plk, fmt):
    key = plk.OpeningKey.setup(TAU)
    _, witness = key.update(0x1234567)
    blob = plk.plonk.g2_to_bytes(witness, fmt)
    assert len(blob) == (96 if fmt == "compressed" else 192)
    # the form of the opening key's own bytes
    assert blob == plk.OpeningKey.setup(0x1234567).to_bytes(fmt)[1]
    assert np.array_equal(plk.plonk.g2_from_bytes(blob, fmt), witness)
    bad = bytearray(blob)
    bad[0] ^= 0x80
    with pytest.raises(plk.PlonkError) as e:
        plk.plonk.g2_from_bytes(bytes(bad), fmt)
    assert e.value.status == plk.PLK_E_ARG


def test_null_arguments_are_rejected_without_gpu(plk):
    lib = plk.plonk._lib()
    assert lib.plk_g1_mul_batch(None, None, None, 1, 0, None) == plk.PLK_E_ARG
    assert lib.plk_g1_mul_last_ms(None, None) == plk.PLK_E_ARG
    assert lib.plk_opening_key_update(None, None, None, None) == plk.PLK_E_ARG
    assert lib.plk_srs_update(None, None, None, None, None, None, None) == plk.PLK_E_ARG
    assert lib.plk_srs_verify_update(None, None, None, None, None, None, None, None) == plk.PLK_E_ARG
    assert lib.plk_debug_glv_split(None, None, 1, None) == plk.PLK_E_ARG
