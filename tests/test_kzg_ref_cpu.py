"""The index arithmetic of plk_kzg_open_domain, pinned without any kernel: the Feist-Khovratovich
pipeline of tests/kzg_ref.py (reversed and padded SRS, embedded coefficients, the slice [n, 2n),
the final transform) against the definition pi_i = [q_i(tau)]G from a plain Ruffini loop — in the
exponent (every point replaced by its discrete log, arithmetic mod r) and on real points."""
import pytest

import kzg_ref as K
import pyref as P

R = P.R_MOD


def taus(k: int):
    """random, 1, r - 1, omega (an opening point), omega^3 and the primitive 2n-th root (both put
    identities into A and u = +-v into butterflies)."""
    rng = P.SplitMix64(8349 + k)
    return {"random": rng.fr(), "one": 1, "minus one": R - 1, "omega": P.omega(k),
            "omega^3": pow(P.omega(k), 3, R), "2n-th root": P.omega(k + 1)}


def polys(n: int, seed: int):
    rng = P.SplitMix64(seed)
    out = {"random n": [rng.fr() for _ in range(n)], "constant": [rng.fr()], "zero": [],
           "X^(n-1)": [0] * (n - 1) + [1], "edges": [R - 1] + [0] * (n - 2) + [R - 1]}
    if n > 1:
        out["random n-1"] = [rng.fr() for _ in range(n - 1)]
    return out


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_pipeline_in_the_exponent(k):
    n = 1 << k
    for tname, tau in taus(k).items():
        srs = [pow(tau, m, R) for m in range(n)]
        for pname, f in polys(n, 100 + k).items():
            want = K.witness_logs(f, tau, k)
            got = K.fk_open_domain(K.ExpGroup, srs, f, k)
            assert got == want, (tname, pname)
            w = P.omega(k)
            for i in range(n):  # the closed form, where the opening point is not tau
                z = pow(w, i, R)
                if (tau - z) % R:
                    assert want[i] == K.witness_log_closed(f, tau, z), (tname, pname, i)


@pytest.mark.parametrize("k", [1, 2])
def test_pipeline_on_points(k):
    n = 1 << k
    for tname, tau in taus(k).items():
        srs = P.srs_setup(tau, n)
        for pname, f in polys(n, 200 + k).items():
            want = K.gen_mul_many(K.witness_logs(f, tau, k))
            assert K.fk_open_domain(K.PointGroup, srs, f, k, K.group_fft) == want, (tname, pname)


@pytest.mark.parametrize("k", [1, 3, 4])
def test_recursive_transform_is_the_definition(k):
    rng = P.SplitMix64(300 + k)
    xs = [rng.fr() for _ in range(1 << k)]
    for inverse in (False, True):
        assert K.group_fft(K.ExpGroup, xs, k, inverse) == K.group_dft(K.ExpGroup, xs, k, inverse)
    assert K.group_fft(K.ExpGroup, K.group_fft(K.ExpGroup, xs, k), k, True) == xs


def test_fixed_base_table_is_the_plain_multiplication():
    rng = P.SplitMix64(7)
    ks = [0, 1, 2, 255, 256, R - 1, R, R + 5] + [rng.fr() for _ in range(8)]
    assert K.gen_mul_many(ks) == [P.g1_mul(P.G1_GEN, s) for s in ks]


def test_fold_of_true_openings_satisfies_the_pairing_relation_in_the_exponent():
    # log C == tau * log W  <=>  e(C, H) == e(W, [tau]H)
    rng = P.SplitMix64(11)
    tau = rng.fr()
    fs = [[rng.fr() for _ in range(5)] for _ in range(4)]
    zs = [rng.fr() for _ in fs]
    ys = [P.poly_eval(f, z) for f, z in zip(fs, zs)]
    cs = [P.poly_eval(f, tau) for f in fs]
    ws = [P.poly_eval(P.ruffini(f, z), tau) for f, z in zip(fs, zs)]
    rhos = [1] + [rng.fr() >> 127 for _ in fs[1:]]
    c, w = K.fold_pair_logs(cs, zs, ys, ws, rhos)
    assert c == tau * w % R
    ys[2] = (ys[2] + 1) % R
    c, w = K.fold_pair_logs(cs, zs, ys, ws, rhos)
    assert c != tau * w % R
