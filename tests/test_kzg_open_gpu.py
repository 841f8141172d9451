"""KZG openings on the GPU (csrc/kzg.hip): plk_kzg_open_domain against the route through the
existing primitives (compute_aggregate_witness, then commit) and against Python integers,
plk_kzg_open at arbitrary points, open_multiple, the refusal of an SRS outside G1, and the fold
of openings into one pairing check. Every comparison is bit for bit."""
import functools

import numpy as np
import pytest

import g1_ingest_ref as G
import kzg_ref as K
import pyref as P

pytestmark = pytest.mark.gpu

R = P.R_MOD
TAU_KINDS = ["random", "one", "minus one", "omega^3", "2n-th root"]


def tau_of(kind: str, k: int) -> int:
    return {"random": P.SplitMix64(77 + k).fr(), "one": 1, "minus one": R - 1,
            "omega^3": pow(P.omega(k), 3, R),  # an opening point coincides with tau; A holds identities
            "2n-th root": P.omega(k + 1)}[kind]


def fr_np(vals):
    return P.fr_vec_to_np(vals)


@functools.lru_cache(maxsize=None)
def _params(plk, k: int, kind: str):
    return plk.PlonkParams.setup(k, fr_np([tau_of(kind, k)])[0])


def polys(n: int, seed: int):
    rng = P.SplitMix64(seed)
    out = {"random": [rng.fr() for _ in range(n)],
           "n-1": [rng.fr() for _ in range(n - 1)] if n > 1 else [rng.fr()],
           "zero": [0] * n, "constant": [rng.fr()], "length 1 of n": [rng.fr()] + [0] * (n - 1),
           "X^(n-1)": [0] * (n - 1) + [1],
           "ends 0": [0] + [rng.fr() for _ in range(n - 2)] + [0] if n > 2 else [0, 0],
           "ends 1": [1] + [rng.fr() for _ in range(n - 2)] + [1] if n > 2 else [1, 1],
           "ends r-1": [R - 1] + [rng.fr() for _ in range(n - 2)] + [R - 1] if n > 2 else [R - 1, R - 1]}
    return out


IDENTITY_ROW = P.g1_vec_to_np([None])[0]


# ------------------------------------------------------------------ open_domain
@pytest.mark.parametrize("kind", TAU_KINDS)
@pytest.mark.parametrize("k", [1, 2, 4, 6, 8])
def test_open_domain_equals_the_route_through_existing_primitives(plk, gpu_ctx, k, kind):
    n = 1 << k
    pp = _params(plk, k, kind)
    fft = plk.Fft(k, gpu_ctx)
    one = fr_np([1])[0]
    cases = polys(n, 500 + k)
    if k == 8:  # 256 divisions and commits per polynomial: the two dense ones
        cases = {name: cases[name] for name in ("random", "n-1")}
    for name, f in cases.items():
        fc = plk.Coefficients(fr_np(f))
        values, wit = pp.open_domain(k, fc)
        assert np.array_equal(values.values, fft.dft(fc).values), (name, "values")
        for i in range(n):
            q = pp.compute_aggregate_witness([fc], fft.elements[i], one)
            want = pp.commit(q).words if len(q) else IDENTITY_ROW
            assert np.array_equal(wit[i], want), (name, i)
        if name in ("constant", "zero"):
            assert all(np.array_equal(row, IDENTITY_ROW) for row in wit), name


@pytest.mark.parametrize("kind", TAU_KINDS)
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_open_domain_equals_the_integers(plk, gpu_ctx, k, kind):
    n, tau, w = 1 << k, tau_of(kind, k), P.omega(k)
    pp = _params(plk, k, kind)
    for name, f in polys(n, 600 + k).items():
        values, wit = pp.open_domain(k, fr_np(f))
        logs = K.witness_logs(f, tau, k)
        for i in range(n):  # the closed form, where the opening point is not tau itself
            if (tau - pow(w, i, R)) % R:
                assert logs[i] == K.witness_log_closed(f, tau, pow(w, i, R))
        assert np.array_equal(wit, K.gen_mul_np(logs)), name
        assert P.fr_vec_from_np(values.values) == [P.poly_eval(f, pow(w, i, R)) for i in range(n)], name


def test_cached_table_and_another_size_give_the_bytes_of_fresh_objects(plk, gpu_ctx):
    tau = fr_np([tau_of("random", 4)])[0]
    rng = P.SplitMix64(9)
    f4, f3 = fr_np([rng.fr() for _ in range(16)]), fr_np([rng.fr() for _ in range(7)])
    fresh4 = plk.PlonkParams.setup(4, tau).open_domain(4, f4)
    fresh3 = plk.PlonkParams.setup(4, tau).open_domain(3, f3)
    pp = plk.PlonkParams.setup(4, tau)
    first = pp.open_domain(4, f4)
    assert plk.kzg_last_open_ms(gpu_ctx)[2] > 0  # the table was built
    second = pp.open_domain(4, f4)
    t = plk.kzg_last_open_ms(gpu_ctx)
    assert t[2] == 0 and t[0] > 0 and t[1] > 0  # the table was cached
    other = pp.open_domain(3, f3)
    again = pp.open_domain(4, f4)
    for got, want in ((first, fresh4), (second, fresh4), (again, fresh4), (other, fresh3)):
        assert np.array_equal(got[0].values, want[0].values) and np.array_equal(got[1], want[1])


def test_both_forms_of_the_transform_give_the_same_bytes(plk, gpu_ctx, monkeypatch):
    k = 5
    tau = fr_np([tau_of("omega^3", k)])[0]
    rng = P.SplitMix64(13)
    f = fr_np([rng.fr() for _ in range(1 << k)])
    default = plk.PlonkParams.setup(k, tau).open_domain(k, f)
    for form in ("xyzz", "glv"):
        monkeypatch.setenv("PLK_G1_NTT_FORM", form)  # read by the library at every call
        got = plk.PlonkParams.setup(k, tau).open_domain(k, f)
        assert np.array_equal(got[0].values, default[0].values) and np.array_equal(got[1], default[1]), form


def test_open_domain_arguments_on_a_live_srs(plk, gpu_ctx):
    pp = _params(plk, 2, "random")  # 12 points
    f = fr_np([1, 2, 3])
    pp.open_domain(2, f)
    for k, poly in ((0, f[:1]), (21, f), (2, fr_np([1, 2, 3, 4, 5])),
                    (2, P.fr_vec_to_np([R], mont=False))):
        with pytest.raises(plk.PlonkError) as e:
            pp.open_domain(k, poly)
        assert e.value.status == plk.PLK_E_ARG and e.value.bad_index is None
    with pytest.raises(plk.PlonkError) as e:
        pp.open_domain(4, f)  # 16 > 12 points
    assert e.value.status == plk.PLK_E_DEGREE


# ------------------------------------------------------------------ open at arbitrary points
@pytest.mark.parametrize("count", [1, 5, 70])
def test_open_at_arbitrary_points(plk, gpu_ctx, count):
    k = 6
    tau = tau_of("random", k)
    pp = _params(plk, k, "random")  # 72 points
    rng = P.SplitMix64(40 + count)
    f = [rng.fr() for _ in range(40)]
    zs = ([0, 1, P.omega(k), R - 1] + [rng.fr() for _ in range(count)])[:count]
    if count == 1:
        zs = [0]
    values, wit = pp.open(plk.Coefficients(fr_np(f)), fr_np(zs))
    assert P.fr_vec_from_np(values) == [P.poly_eval(f, z) for z in zs]
    assert np.array_equal(wit, K.gen_mul_np([P.poly_eval(P.ruffini(f, z), tau) for z in zs]))


def test_open_short_polynomials_and_degree(plk, gpu_ctx):
    pp = _params(plk, 2, "random")  # 12 points
    zs = fr_np([3, 0])
    for f, want in (([], 0), ([5], 5), ([5, 0, 0], 5)):
        values, wit = pp.open(fr_np(f) if f else np.zeros((0, 4), dtype=np.uint64), zs)
        assert P.fr_vec_from_np(values) == [want, want]
        assert all(np.array_equal(row, IDENTITY_ROW) for row in wit)
    with pytest.raises(plk.PlonkError) as e:
        pp.open(fr_np([1] * 13), zs)
    assert e.value.status == plk.PLK_E_DEGREE
    pp.open(fr_np([1] * 12 + [0]), zs)  # trailing zeros do not count, as in commit
    with pytest.raises(plk.PlonkError) as e:
        pp.open(fr_np([1, 2]), P.fr_vec_to_np([R], mont=False))
    assert e.value.status == plk.PLK_E_ARG


def test_open_multiple_in_the_shape_of_the_reference_test(plk, gpu_ctx):
    k = 6
    tau = tau_of("random", k)
    pp = _params(plk, k, "random")
    rng = P.SplitMix64(2627)
    fs = [[rng.fr() for _ in range(m)] for m in (26, 27, 28)]
    z, v = rng.fr(), rng.fr()
    values, w = pp.open_multiple([plk.Coefficients(fr_np(f)) for f in fs], fr_np([z])[0], fr_np([v])[0])
    assert P.fr_vec_from_np(values) == [P.poly_eval(f, z) for f in fs]
    assert np.array_equal(w.words, K.gen_mul_np([P.poly_eval(P.aggregate_witness(fs, z, v), tau)])[0])


# ------------------------------------------------------------------ an SRS outside G1
def test_loaded_srs_with_a_point_outside_g1_is_refused_with_its_index(plk, gpu_ctx):
    k, bad = 3, 5
    pts = _params(plk, k, "random").points().copy()
    outsider = G.non_member(11, np.random.default_rng(3))
    assert P.g1_is_on_curve(outsider) and not G.in_subgroup(outsider)
    pts[bad] = P.g1_vec_to_np([outsider])[0]
    pp = plk.PlonkParams.load(pts)
    f = [3, 1, 4, 1, 5, 9, 2, 6]
    with pytest.raises(plk.PlonkError) as e:
        pp.open_domain(k, fr_np(f))
    assert e.value.status == plk.PLK_E_ARG and e.value.bad_index == bad
    with pytest.raises(plk.PlonkError) as e:  # nothing was cached by the refusal
        pp.open_domain(k, fr_np(f))
    assert e.value.bad_index == bad
    pp.open_domain(2, fr_np(f[:4]))  # the first four points are in G1
    z = 7
    values, wit = pp.open(fr_np(f), fr_np([z]))  # plain curve arithmetic: no membership needed
    assert P.fr_vec_from_np(values) == [P.poly_eval(f, z)]
    want = P.msm_naive(P.g1_vec_from_np(pts[:7]), P.ruffini(f, z))
    assert np.array_equal(wit, P.g1_vec_to_np([want]))
    # an SRS that load() took on faith and that is in G1 passes the same test and opens
    good = plk.PlonkParams.load(_params(plk, k, "random").points())
    assert np.array_equal(good.open_domain(k, fr_np(f))[1], _params(plk, k, "random").open_domain(k, fr_np(f))[1])


# ------------------------------------------------------------------ folding
@pytest.fixture(scope="module")
def opened(plk, gpu_ctx):
    """64 openings of one polynomial over the 2^6 domain, and what the checks need."""
    k = 6
    tau = tau_of("random", k)
    pp = _params(plk, k, "random")
    rng = P.SplitMix64(66)
    f = [rng.fr() for _ in range(1 << k)]
    values, wit = pp.open_domain(k, fr_np(f))
    com = pp.commit(plk.Coefficients(fr_np(f))).words
    return dict(tau=tau, f=f, g=pp.points(0, 1)[0], key=plk.OpeningKey.setup(tau),
                coms=np.tile(com, (1 << k, 1)), zs=plk.Fft(k, gpu_ctx).elements.copy(),
                ys=values.values.copy(), wits=wit.copy(), pp=pp)


def altered(o, what: str, at: int):
    coms, zs, ys, wits = (o[n].copy() for n in ("coms", "zs", "ys", "wits"))
    if what == "value":
        ys[at] = fr_np([(P.fr_vec_from_np(ys[at])[0] + 1) % R])[0]
    elif what == "point":
        zs[at] = fr_np([12345])[0]
    elif what == "witness":
        wits[at] = K.gen_mul_np([424242])[0]
    else:
        coms[at] = K.gen_mul_np([171717])[0]
    return coms, zs, ys, wits


def test_check_openings_accepts_true_openings(plk, gpu_ctx, opened):
    o = opened
    assert o["key"].check_openings(o["g"], o["coms"], o["zs"], o["ys"], o["wits"], ctx=gpu_ctx)
    rng = P.SplitMix64(5)
    zs = fr_np([0, 1, R - 1] + [rng.fr() for _ in range(4)])
    ys, wits = o["pp"].open(fr_np(o["f"]), zs)
    assert o["key"].check_openings(o["g"], o["coms"][:7], zs, ys, wits, ctx=gpu_ctx)


@pytest.mark.parametrize("at", [0, 63])
@pytest.mark.parametrize("what", ["value", "point", "witness", "commitment"])
def test_check_openings_rejects_one_altered_opening(plk, gpu_ctx, opened, what, at):
    o = opened
    coms, zs, ys, wits = altered(o, what, at)
    assert not o["key"].check_openings(o["g"], coms, zs, ys, wits, ctx=gpu_ctx)


def test_explicit_weights_reproduce_the_pair_of_the_integers(plk, gpu_ctx, opened):
    o, n, tau = opened, 9, opened["tau"]
    rng = P.SplitMix64(31)
    rhos = [1, 0, R - 1] + [rng.fr() for _ in range(n - 3)]
    zs, ys = P.fr_vec_from_np(o["zs"][:n]), P.fr_vec_from_np(o["ys"][:n])
    wlogs = K.witness_logs(o["f"], tau, 6)[:n]
    clog = P.poly_eval(o["f"], tau)
    pair = o["key"].fold_openings(o["g"], o["coms"][:n], o["zs"][:n], o["ys"][:n], o["wits"][:n],
                                  weights=fr_np(rhos), ctx=gpu_ctx)
    assert np.array_equal(pair, K.gen_mul_np(K.fold_pair_logs([clog] * n, zs, ys, wlogs, rhos)))
    assert o["key"].check(pair)


def test_one_opening_with_weight_one_is_its_own_pair(plk, gpu_ctx, opened):
    o, i = opened, 17
    pair = o["key"].fold_openings(o["g"], o["coms"][i], o["zs"][i], o["ys"][i], o["wits"][i],
                                  weights=fr_np([1]), ctx=gpu_ctx)
    c, w = P.g1_vec_from_np(o["coms"][i])[0], P.g1_vec_from_np(o["wits"][i])[0]
    z, y = P.fr_vec_from_np(o["zs"][i])[0], P.fr_vec_from_np(o["ys"][i])[0]
    want_c = P.g1_add(P.g1_add(c, P.g1_mul(P.G1_GEN, R - y)), P.g1_mul(w, z))
    assert np.array_equal(pair, P.g1_vec_to_np([want_c, w]))
    # the weights drawn inside the library start at rho_0 = 1: the same pair
    assert np.array_equal(pair, o["key"].fold_openings(o["g"], o["coms"][i], o["zs"][i], o["ys"][i],
                                                       o["wits"][i], ctx=gpu_ctx))


def test_per_opening_route_marks_exactly_the_altered_opening(plk, gpu_ctx, opened):
    o, n, at = opened, 8, 5
    coms, zs, ys, wits = (a[:n] for a in altered(o, "value", at))
    one = fr_np([1])
    pairs = np.stack([o["key"].fold_openings(o["g"], coms[i], zs[i], ys[i], wits[i], weights=one, ctx=gpu_ctx)
                      for i in range(n)])
    assert o["key"].check_batch(pairs, gpu_ctx).tolist() == [i != at for i in range(n)]


def test_fold_refusals(plk, gpu_ctx, opened):
    o, n = opened, 3
    args = [o["coms"][:n], o["zs"][:n], o["ys"][:n], o["wits"][:n]]
    big = P.fr_vec_to_np([R], mont=False)[0]
    off = o["wits"][:n].copy()
    off[1, 6] ^= np.uint64(1)  # y: off the curve
    for which, repl in ((1, big), (2, big)):
        a = [x.copy() for x in args]
        a[which][2] = repl
        with pytest.raises(plk.PlonkError) as e:
            o["key"].fold_openings(o["g"], *a, ctx=gpu_ctx)
        assert e.value.status == plk.PLK_E_ARG
    with pytest.raises(plk.PlonkError) as e:
        o["key"].fold_openings(o["g"], args[0], args[1], args[2], off, ctx=gpu_ctx)
    assert e.value.status == plk.PLK_E_ARG
    with pytest.raises(plk.PlonkError) as e:
        o["key"].fold_openings(o["g"], *args, weights=np.stack([big] * n), ctx=gpu_ctx)
    assert e.value.status == plk.PLK_E_ARG
    with pytest.raises(plk.PlonkError) as e:
        o["key"].fold_openings(o["g"], np.zeros((0, 13), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64),
                               np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 13), dtype=np.uint64), ctx=gpu_ctx)
    assert e.value.status == plk.PLK_E_ARG
