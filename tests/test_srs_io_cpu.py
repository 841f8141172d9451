"""The opening key in zkcrypto's G2 byte forms (plk_opening_key_load_bytes / _to_bytes, host only)
and the host Fp2 square root behind the compressed form (csrc/pairing_host.hpp f2_sqrt), against
Python integers built on tests/pairing_ref.py. Needs no GPU.

The encodings are ASSUMED to be zkcrypto's (parity unpinned, include/plk.h): what is pinned here
is the layout the header states and the strictness of the decoder.
"""
import numpy as np
import pytest

import pairing_ref as R
import pyref as P

p = P.P_MOD
HALF = (p - 1) // 2
FORMATS = ("compressed", "uncompressed")
XI4 = (4, 4)  # 4 (1 + u)


def fp_limbs(v):
    return P.int_to_limbs(P.fp_to_mont(v), 6)


def g2_row(q):
    """plk_g2: x.c0, x.c1, y.c0, y.c1 as Montgomery limbs, then the infinity word."""
    (x0, x1), (y0, y1) = q
    return np.array(fp_limbs(x0) + fp_limbs(x1) + fp_limbs(y0) + fp_limbs(y1) + [0], dtype=np.uint64)


def g2_from_row(row):
    v = [P.fp_from_mont(P.limbs_to_int(row[6 * i:6 * i + 6])) for i in range(4)]
    return ((v[0], v[1]), (v[2], v[3]))


def y_is_larger(y):
    return y[0] > HALF if y[1] == 0 else y[1] > HALF


def encode(q, fmt):
    """The header's layout: x.c1 then x.c0 big-endian (then y.c1, y.c0), flags in byte 0."""
    (x0, x1), (y0, y1) = q
    if fmt == "compressed":
        b = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
        b[0] |= 0x80 | (0x20 if y_is_larger((y0, y1)) else 0)
        return bytes(b)
    return b"".join(v.to_bytes(48, "big") for v in (x1, x0, y1, y0))


def twist_rhs(x):
    return R.f2add(R.f2mul(R.f2mul(x, x), x), XI4)


def rand_f2(rng):
    return (int.from_bytes(rng.bytes(48), "big") % p, int.from_bytes(rng.bytes(48), "big") % p)


@pytest.fixture(scope="module")
def key_points():
    tau = 0x1234567890ABCDEF1234567890ABCDEF
    return tau, R.G2_GEN, R.g2_mul(R.G2_GEN, tau)


@pytest.mark.parametrize("fmt", FORMATS)
def test_round_trip_and_bytes_equal_the_python_encoder(plk, key_points, fmt):
    tau, h, bh = key_points
    key = plk.OpeningKey.setup(tau)
    a, b = key.to_bytes(fmt)
    assert len(a) == len(b) == (96 if fmt == "compressed" else 192)
    assert a == encode(h, fmt) and b == encode(bh, fmt)
    back = plk.OpeningKey.from_bytes(a, b, fmt)
    for got, want in zip(back.points(), key.points()):
        assert np.array_equal(got, want)
    assert np.array_equal(back.points()[1], g2_row(bh))
    assert back.to_bytes(fmt) == (a, b)
    # the loaded key decides as the original
    w = P.g1_mul(P.G1_GEN, 11)
    pair = np.stack([P.g1_vec_to_np([P.g1_mul(w, tau)])[0], P.g1_vec_to_np([w])[0]])
    assert back.check(pair)
    pair[0] = P.g1_vec_to_np([P.g1_mul(w, tau + 1)])[0]
    assert not back.check(pair)


def rejected(plk, a, b, fmt):
    with pytest.raises(plk.PlonkError) as e:
        plk.OpeningKey.from_bytes(a, b, fmt)
    return e.value.status == plk.PLK_E_ARG


def test_flag_bits_are_strict(plk, key_points):
    _, h, bh = key_points
    good = {f: (encode(h, f), encode(bh, f)) for f in FORMATS}

    def with_byte0(data, v):
        return bytes([v]) + data[1:]

    c, u = good["compressed"][1], good["uncompressed"][1]
    hc, hu = good["compressed"][0], good["uncompressed"][0]
    assert rejected(plk, hc, with_byte0(c, c[0] & 0x7F), "compressed")      # bit 7 clear
    assert rejected(plk, hc, with_byte0(c, c[0] | 0x40), "compressed")      # infinity bit on a point
    assert rejected(plk, hu, with_byte0(u, u[0] | 0x80), "uncompressed")    # bit 7 set
    assert rejected(plk, hu, with_byte0(u, u[0] | 0x20), "uncompressed")    # sort bit set
    assert rejected(plk, hu, with_byte0(u, u[0] | 0x40), "uncompressed")    # infinity bit on a point
    assert rejected(plk, with_byte0(hc, hc[0] & 0x7F), c, "compressed")     # the same for H
    # a byte under the infinity bit
    assert rejected(plk, hc, bytes([0xC0]) + bytes(94) + b"\x01", "compressed")
    assert rejected(plk, hc, bytes([0xE0]) + bytes(95), "compressed")
    assert rejected(plk, hu, bytes([0x40]) + bytes(190) + b"\x01", "uncompressed")
    # wrong lengths never reach the library
    assert rejected(plk, hc[:95], c, "compressed")


def test_infinity_is_refused(plk, key_points):
    _, h, _ = key_points
    assert rejected(plk, encode(h, "compressed"), bytes([0xC0]) + bytes(95), "compressed")
    assert rejected(plk, bytes([0xC0]) + bytes(95), encode(h, "compressed"), "compressed")
    assert rejected(plk, encode(h, "uncompressed"), bytes([0x40]) + bytes(191), "uncompressed")


def test_coefficients_at_or_above_p_are_refused(plk, key_points):
    _, h, bh = key_points
    (x0, x1), (y0, y1) = bh
    hc, hu = encode(h, "compressed"), encode(h, "uncompressed")

    def comp(c1, c0):
        b = bytearray(c1.to_bytes(48, "big") + c0.to_bytes(48, "big"))
        b[0] |= 0x80
        return bytes(b)

    assert rejected(plk, hc, comp(p, x0), "compressed")
    assert rejected(plk, hc, comp(x1, p), "compressed")
    assert rejected(plk, hc, comp(x1, p + 5), "compressed")
    assert rejected(plk, hc, comp((1 << 381) - 1, x0), "compressed")
    for k in range(4):
        v = [x1, x0, y1, y0]
        v[k] = v[k] + p
        assert rejected(plk, hu, b"".join(t.to_bytes(48, "big") for t in v), "uncompressed"), k


def test_x_without_a_root_and_y_off_the_twist_are_refused(plk, key_points):
    _, h, bh = key_points
    hc, hu = encode(h, "compressed"), encode(h, "uncompressed")
    rng = np.random.Generator(np.random.PCG64(0x62))
    found = 0
    while found < 3:
        x = rand_f2(rng)
        if R.f2_is_square(twist_rhs(x)):
            continue
        found += 1
        assert rejected(plk, hc, encode((x, (0, 0)), "compressed"), "compressed")
    (x, (y0, y1)) = bh
    assert rejected(plk, hu, encode((x, ((y0 + 1) % p, y1)), "uncompressed"), "uncompressed")
    assert rejected(plk, hu, encode((x, (y0, (y1 + 1) % p)), "uncompressed"), "uncompressed")


def test_the_wrong_sort_bit_decodes_to_the_negative(plk, key_points):
    """-Q is a valid key point, so nothing fails: the points are compared."""
    _, h, bh = key_points
    c = bytearray(encode(bh, "compressed"))
    c[0] ^= 0x20
    key = plk.OpeningKey.from_bytes(encode(h, "compressed"), bytes(c), "compressed")
    assert g2_from_row(key.points()[1]) == R.g2_neg(bh)
    assert g2_from_row(key.points()[0]) == h


def test_a_twist_point_outside_g2_is_refused(plk, key_points):
    _, h, _ = key_points
    rng = np.random.Generator(np.random.PCG64(0x63))
    while True:
        x = rand_f2(rng)
        y = R.f2sqrt(twist_rhs(x))
        if y is not None:
            break
    q = (x, y)
    assert R.g2_is_on_curve(q) and R.g2_mul(q, P.R_MOD) is not None  # on the twist, not of order r
    for fmt in FORMATS:
        assert rejected(plk, encode(h, fmt), encode(q, fmt), fmt)
        assert rejected(plk, encode(q, fmt), encode(h, fmt), fmt)


def f2_words(a):
    return np.array(fp_limbs(a[0]) + fp_limbs(a[1]), dtype=np.uint64)


def f2_of_words(w):
    return (P.fp_from_mont(P.limbs_to_int(w[:6])), P.fp_from_mont(P.limbs_to_int(w[6:])))


def test_host_fp2_square_root(plk):
    rng = np.random.Generator(np.random.PCG64(0x64))
    roots = [rand_f2(rng) for _ in range(64)]
    # edge values: purely real and purely imaginary roots and squares, 0, 1, -1, u
    roots += [(3, 0), (0, 3), (p - 1, 0), (0, p - 1), (0, 0), (1, 0), (0, 1), (5, 5)]
    squares = [R.f2mul(s, s) for s in roots]
    squares += [(p - 1, 0), (4, 0), (0, 4), (p - 4, 0), (2, 0), (0, 2)]  # c1 = 0 / c0 = 0
    for a in squares:
        want = R.f2sqrt(a)
        got, ok = plk.plonk.debug_f2_sqrt(f2_words(a))
        assert ok == (want is not None) == R.f2_is_square(a), a
        if want is not None:
            g = f2_of_words(got)
            assert g in (want, R.f2neg(want)), a
            assert R.f2mul(g, g) == a
        else:
            assert not got.any()
    n = 0
    while n < 8:  # non-squares
        a = rand_f2(rng)
        if R.f2_is_square(a):
            continue
        n += 1
        got, ok = plk.plonk.debug_f2_sqrt(f2_words(a))
        assert not ok and R.f2sqrt(a) is None


def test_symbols_are_declared(plk):
    lib = plk.plonk._lib()
    for s in ("plk_srs_load_bytes", "plk_srs_export_bytes", "plk_srs_fold", "plk_srs_verify",
              "plk_opening_key_load_bytes", "plk_opening_key_to_bytes", "plk_debug_srs_weights"):
        assert s in plk.ABI_SYMBOLS and hasattr(lib, s)
    assert lib.plk_abi_version() == 2


def test_host_weights_need_no_gpu(plk):
    """rho_0 = 1, the others 128-bit; another seed or another n gives other weights."""
    a = plk.plonk.debug_srs_weights(bytes(range(32)), 9)
    b = plk.plonk.debug_srs_weights(bytes(range(1, 33)), 9)
    c = plk.plonk.debug_srs_weights(bytes(range(32)), 10)
    va, vb, vc = (P.fr_vec_from_np(x) for x in (a, b, c))
    assert len(va) == 8 and len(vc) == 9
    assert va[0] == vb[0] == vc[0] == 1
    assert all(0 < v < 1 << 128 for v in va + vb + vc)
    assert len(set(va[1:] + vb[1:] + vc[1:])) == 7 + 7 + 8
