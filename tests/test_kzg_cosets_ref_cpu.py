"""The index arithmetic of plk_kzg_open_cosets and plk_kzg_fold_cosets, pinned without any kernel
(tests/kzg_cosets_ref.py): the pipeline against the definition by long division, the interpolant
from the values against the division's remainder, the fold identity log C = tau^l log W, log_l = 0
against the per-point witnesses, and the generator identities the coset order rests on. All in the
exponent (every point replaced by its discrete log), once on real points."""
import pytest

import kzg_cosets_ref as KC
import kzg_ref as K
import pyref as P
from test_kzg_open_gpu import polys

R = P.R_MOD
SHAPES = [(k, log_l) for k in range(1, 6) for log_l in range(k + 1)]


def taus(k: int):
    rng = P.SplitMix64(4711 + k)
    return {"random": rng.fr(), "one": 1, "minus one": R - 1, "omega^3": pow(P.omega(k), 3, R),
            "2n-th root": P.omega(k + 1)}


@pytest.mark.parametrize("k,log_l", SHAPES)
def test_generator_identities(k, log_l):
    l, r = 1 << log_l, 1 << (k - log_l)
    w = P.omega(k)
    assert pow(w, l, R) == (P.omega(k - log_l) if k > log_l else 1)
    assert pow(w, r, R) == (P.omega(log_l) if log_l else 1)


@pytest.mark.parametrize("k,log_l", SHAPES)
def test_pipeline_is_the_definition_in_the_exponent(k, log_l):
    n = 1 << k
    for tname, tau in taus(k).items():
        srs = [pow(tau, m, R) for m in range(n)]
        for pname, f in polys(n, 100 + k).items():
            want = KC.coset_witness_logs(f, tau, k, log_l)
            got = KC.fk_open_cosets(K.ExpGroup, srs, f, k, log_l, KC.group_fft)
            assert got == want, (tname, pname)


@pytest.mark.parametrize("k,log_l", [(2, 1), (3, 1), (3, 2)])
def test_pipeline_by_the_plain_transform_and_on_points(k, log_l):
    n = 1 << k
    tau = taus(k)["omega^3"]
    f = polys(n, 150 + k)["random"]
    want = KC.coset_witness_logs(f, tau, k, log_l)
    assert KC.fk_open_cosets(K.ExpGroup, [pow(tau, m, R) for m in range(n)], f, k, log_l) == want
    got = KC.fk_open_cosets(K.PointGroup, P.srs_setup(tau, n), f, k, log_l, KC.group_fft)
    assert got == K.gen_mul_many(want)


@pytest.mark.parametrize("k,log_l", SHAPES)
def test_interpolant_from_the_values_is_the_remainder(k, log_l):
    n, l, r = 1 << k, 1 << log_l, 1 << (k - log_l)
    w = P.omega(k)
    rng = P.SplitMix64(77 + k)
    for pname, f in polys(n, 200 + k).items():
        values = [P.poly_eval(f, pow(w, i, R)) for i in range(n)]
        shifts = [(pow(w, j, R), values[j::r]) for j in range(r)]  # coset j: entries j + r i
        z = rng.fr()  # and a shift outside the domain
        shifts.append((z, KC.coset_values(f, z, log_l)))
        for z, row in shifts:
            assert row == KC.coset_values(f, z, log_l), pname
            _, rem = KC.divide_by_coset(f, l, pow(z, l, R))
            assert KC.coset_interpolant(row, z, log_l) == rem, pname


@pytest.mark.parametrize("k,log_l", SHAPES)
def test_fold_identity_in_the_exponent(k, log_l):
    # log C == tau^l * log W  <=>  e(C, H) == e(W, [tau^l]H)
    n, l, r = 1 << k, 1 << log_l, 1 << (k - log_l)
    rng = P.SplitMix64(300 + 8 * k + log_l)
    tau, w = rng.fr(), P.omega(k)
    f = [rng.fr() for _ in range(n)]
    zs = [pow(w, j, R) for j in range(r)] + [rng.fr()]
    rows = [KC.coset_values(f, z, log_l) for z in zs]
    wits = [P.poly_eval(KC.divide_by_coset(f, l, pow(z, l, R))[0], tau) for z in zs]
    assert wits[:r] == KC.coset_witness_logs(f, tau, k, log_l)
    coms = [P.poly_eval(f, tau)] * len(zs)
    rhos = [1] + [rng.fr() >> 127 for _ in zs[1:]]
    c, wl = KC.fold_cosets_pair_logs(coms, zs, rows, wits, rhos, tau, log_l)
    assert c == pow(tau, l, R) * wl % R
    for at in (0, l - 1):  # one altered value, first and last of a row
        bad = [row[:] for row in rows]
        bad[-1][at] = (bad[-1][at] + 1) % R
        c, wl = KC.fold_cosets_pair_logs(coms, zs, bad, wits, rhos, tau, log_l)
        assert c != pow(tau, l, R) * wl % R


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_cosets_of_one_point_are_the_per_point_witnesses(k):
    n = 1 << k
    for tname, tau in taus(k).items():
        for pname, f in polys(n, 400 + k).items():
            assert KC.coset_witness_logs(f, tau, k, 0) == K.witness_logs(f, tau, k), (tname, pname)
    # and the fold at l = 1 is the fold of single openings
    rng = P.SplitMix64(5)
    tau, f = rng.fr(), [rng.fr() for _ in range(n)]
    zs = [rng.fr() for _ in range(3)]
    ys = [P.poly_eval(f, z) for z in zs]
    ws = [P.poly_eval(P.ruffini(f, z), tau) for z in zs]
    rhos = [1, rng.fr(), rng.fr()]
    coms = [P.poly_eval(f, tau)] * 3
    assert (KC.fold_cosets_pair_logs(coms, zs, [[y] for y in ys], ws, rhos, tau, 0)
            == K.fold_pair_logs(coms, zs, ys, ws, rhos))
