"""KZG coset openings on the GPU (csrc/kzg.hip plk_kzg_open_cosets / plk_kzg_fold_cosets): the
witnesses against Python integers (the definition by long division, tests/kzg_cosets_ref.py) and
against the route through the existing primitives (divide on the host, then commit), the table
cache, both forms of the transform, the refusals, and the fold of coset openings into one pairing
check against the key of tau^l. Every comparison is bit for bit."""
import numpy as np
import pytest

import g1_ingest_ref as G
import kzg_cosets_ref as KC
import kzg_ref as K
import pyref as P
from test_kzg_open_gpu import IDENTITY_ROW, TAU_KINDS, _params, fr_np, polys, tau_of

pytestmark = pytest.mark.gpu

R = P.R_MOD
SHAPES = [(k, log_l) for k in (1, 2, 3, 4, 6) for log_l in sorted({0, 1, k - 1, k})]


def shifts_of(k: int, log_l: int):
    """The shift of coset j < r: omega^j."""
    w = P.omega(k)
    return [pow(w, j, R) for j in range(1 << (k - log_l))]


# ------------------------------------------------------------------ open_cosets
@pytest.mark.parametrize("kind", TAU_KINDS)
@pytest.mark.parametrize("k,log_l", SHAPES)
def test_open_cosets_equals_the_integers(plk, gpu_ctx, k, log_l, kind):
    n, r, tau, w = 1 << k, 1 << (k - log_l), tau_of(kind, k), P.omega(k)
    pp = _params(plk, k, kind)
    cases = polys(n, 700 + k)
    if k == 6:  # the two dense ones
        cases = {name: cases[name] for name in ("random", "n-1")}
    for name, f in cases.items():
        values, wit = pp.open_cosets(k, log_l, fr_np(f))
        assert wit.shape == (r, 13)
        assert np.array_equal(wit, K.gen_mul_np(KC.coset_witness_logs(f, tau, k, log_l))), name
        assert P.fr_vec_from_np(values.values) == [P.poly_eval(f, pow(w, i, R)) for i in range(n)], name
        rows = values.cosets(log_l)
        assert rows.shape == (r, 1 << log_l, 4)
        for j in (0, r - 1):
            assert P.fr_vec_from_np(rows[j]) == KC.coset_values(f, pow(w, j, R), log_l), (name, j)
        if log_l == k or name in ("constant", "zero"):
            assert all(np.array_equal(row, IDENTITY_ROW) for row in wit), name


@pytest.mark.parametrize("log_l", [2, 3])
def test_witnesses_are_the_commitments_to_the_quotients(plk, gpu_ctx, log_l):
    k = 6
    n, l, r = 1 << k, 1 << log_l, 1 << (k - log_l)
    pp = _params(plk, k, "random")
    psi = pow(P.omega(k), l, R)
    for name, f in polys(n, 800 + log_l).items():
        _, wit = pp.open_cosets(k, log_l, plk.Coefficients(fr_np(f)))
        for j in range(r):
            q, _ = KC.divide_by_coset(f, l, pow(psi, j, R))
            while q and q[-1] == 0:
                q.pop()
            want = pp.commit(plk.Coefficients(fr_np(q))).words if q else IDENTITY_ROW
            assert np.array_equal(wit[j], want), (name, j)


@pytest.mark.parametrize("kind", TAU_KINDS)
@pytest.mark.parametrize("k", [1, 4, 6])
def test_cosets_of_one_point_are_open_domain_byte_for_byte(plk, gpu_ctx, k, kind):
    tau = fr_np([tau_of(kind, k)])[0]
    cases = polys(1 << k, 900 + k)
    f = fr_np(cases["random"])  # each call on an SRS object of its own: each builds its table
    a = plk.PlonkParams.setup(k, tau).open_cosets(k, 0, f)
    b = plk.PlonkParams.setup(k, tau).open_domain(k, f)
    assert np.array_equal(a[0].values, b[0].values) and np.array_equal(a[1], b[1])
    pp = _params(plk, k, kind)  # and with the table shared, whichever call built it
    for name, f in cases.items():
        b = pp.open_domain(k, fr_np(f))
        a = pp.open_cosets(k, 0, fr_np(f))
        assert np.array_equal(a[0].values, b[0].values) and np.array_equal(a[1], b[1]), name


def test_cached_table_and_another_log_l_give_the_bytes_of_fresh_objects(plk, gpu_ctx):
    k = 4
    tau = fr_np([tau_of("random", k)])[0]
    rng = P.SplitMix64(19)
    f = fr_np([rng.fr() for _ in range(1 << k)])
    fresh = {log_l: plk.PlonkParams.setup(k, tau).open_cosets(k, log_l, f) for log_l in (0, 1, 2, 4)}
    pp = plk.PlonkParams.setup(k, tau)
    first = pp.open_cosets(k, 2, f)
    assert plk.kzg_last_open_ms(gpu_ctx)[2] > 0  # the table was built
    second = pp.open_cosets(k, 2, f)
    t = plk.kzg_last_open_ms(gpu_ctx)
    assert t[2] == 0 and t[0] > 0 and t[1] > 0  # the table was cached
    others = {log_l: pp.open_cosets(k, log_l, f) for log_l in (1, 0, 4)}
    dom = pp.open_domain(k, f)
    again = pp.open_cosets(k, 2, f)
    for got, want in ((first, fresh[2]), (second, fresh[2]), (again, fresh[2]), (dom, fresh[0]),
                      *((others[x], fresh[x]) for x in others)):
        assert np.array_equal(got[0].values, want[0].values) and np.array_equal(got[1], want[1])


def test_both_forms_of_the_transform_give_the_same_bytes(plk, gpu_ctx, monkeypatch):
    k = 5
    tau = fr_np([tau_of("omega^3", k)])[0]
    rng = P.SplitMix64(23)
    f = fr_np([rng.fr() for _ in range(1 << k)])
    for log_l in (1, 3):
        default = plk.PlonkParams.setup(k, tau).open_cosets(k, log_l, f)
        for form in ("xyzz", "glv"):
            monkeypatch.setenv("PLK_G1_NTT_FORM", form)  # read by the library at every call
            got = plk.PlonkParams.setup(k, tau).open_cosets(k, log_l, f)
            assert np.array_equal(got[0].values, default[0].values) and np.array_equal(got[1], default[1]), form
        monkeypatch.delenv("PLK_G1_NTT_FORM")


def test_open_cosets_arguments_on_a_live_srs(plk, gpu_ctx):
    pp = _params(plk, 2, "random")  # 12 points
    f = fr_np([1, 2, 3])
    pp.open_cosets(2, 1, f)
    for k, log_l, poly in ((0, 0, f[:1]), (21, 1, f), (2, 3, f), (2, 1, fr_np([1, 2, 3, 4, 5])),
                           (2, 1, P.fr_vec_to_np([R], mont=False))):
        with pytest.raises(plk.PlonkError) as e:
            pp.open_cosets(k, log_l, poly)
        assert e.value.status == plk.PLK_E_ARG and e.value.bad_index is None
    for log_l in (1, 4):
        with pytest.raises(plk.PlonkError) as e:
            pp.open_cosets(4, log_l, f)  # 16 > 12 points
        assert e.value.status == plk.PLK_E_DEGREE


def test_loaded_srs_with_a_point_outside_g1_is_refused_with_its_index(plk, gpu_ctx):
    k, bad = 3, 5
    pts = _params(plk, k, "random").points().copy()
    outsider = G.non_member(11, np.random.default_rng(3))
    pts[bad] = P.g1_vec_to_np([outsider])[0]
    pp = plk.PlonkParams.load(pts)
    f = fr_np([3, 1, 4, 1, 5, 9, 2, 6])
    for log_l in (1, 1, 2, 3):  # nothing is cached by a refusal
        with pytest.raises(plk.PlonkError) as e:
            pp.open_cosets(k, log_l, f)
        assert e.value.status == plk.PLK_E_ARG and e.value.bad_index == bad
    pp.open_cosets(2, 1, f[:4])  # the first four points are in G1
    good = plk.PlonkParams.load(_params(plk, k, "random").points())
    assert np.array_equal(good.open_cosets(k, 1, f)[1], _params(plk, k, "random").open_cosets(k, 1, f)[1])


# ------------------------------------------------------------------ folding
K6, LOG_L = 6, 2


@pytest.fixture(scope="module")
def opened(plk, gpu_ctx):
    """The 16 coset openings of one polynomial over the 2^6 domain at l = 4, and what the checks need."""
    tau = tau_of("random", K6)
    pp = _params(plk, K6, "random")
    rng = P.SplitMix64(606)
    f = [rng.fr() for _ in range(1 << K6)]
    values, wit = pp.open_cosets(K6, LOG_L, fr_np(f))
    com = pp.commit(plk.Coefficients(fr_np(f))).words
    zs = shifts_of(K6, LOG_L)
    return dict(tau=tau, f=f, pp=pp, key=plk.OpeningKey.setup(pow(tau, 1 << LOG_L, R)),
                key_tau=plk.OpeningKey.setup(tau), com=com, coms=np.tile(com, (len(zs), 1)),
                zs_int=zs, zs=fr_np(zs), ys=np.ascontiguousarray(values.cosets(LOG_L)), wits=wit.copy())


def altered(o, what: str, at: int):
    coms, zs, ys, wits = (o[n].copy() for n in ("coms", "zs", "ys", "wits"))
    if what in ("first value", "last value"):
        i = 0 if what == "first value" else ys.shape[1] - 1
        ys[at, i] = fr_np([(P.fr_vec_from_np(ys[at, i:i + 1])[0] + 1) % R])[0]
    elif what == "shift":
        zs[at] = fr_np([12345])[0]
    elif what == "witness":
        wits[at] = K.gen_mul_np([424242])[0]
    else:
        coms[at] = K.gen_mul_np([171717])[0]
    return coms, zs, ys, wits


def test_check_cosets_accepts_true_openings(plk, gpu_ctx, opened):
    o = opened
    assert o["key"].check_cosets(o["pp"], LOG_L, o["coms"], o["zs"], o["ys"], o["wits"])
    assert o["key"].check_cosets(o["pp"], LOG_L, o["com"], o["zs"], o["ys"], o["wits"])  # one commitment for all
    assert o["key"].check_cosets(o["pp"], LOG_L, o["com"], o["zs"][3:8], o["ys"][3:8], o["wits"][3:8])


@pytest.mark.parametrize("at", [0, 15])
@pytest.mark.parametrize("what", ["first value", "last value", "shift", "witness", "commitment"])
def test_check_cosets_rejects_one_altered_opening(plk, gpu_ctx, opened, what, at):
    o = opened
    coms, zs, ys, wits = altered(o, what, at)
    assert not o["key"].check_cosets(o["pp"], LOG_L, coms, zs, ys, wits)


def test_check_cosets_against_the_key_of_tau_rejects(plk, gpu_ctx, opened):
    o = opened
    assert not o["key_tau"].check_cosets(o["pp"], LOG_L, o["coms"], o["zs"], o["ys"], o["wits"])


def test_explicit_weights_reproduce_the_pair_of_the_integers(plk, gpu_ctx, opened):
    o, n, tau = opened, 9, opened["tau"]
    rng = P.SplitMix64(37)
    rhos = [1, 0, R - 1] + [rng.fr() for _ in range(n - 3)]
    zs = o["zs_int"][:n]
    rows = [P.fr_vec_from_np(row) for row in o["ys"][:n]]
    wlogs = KC.coset_witness_logs(o["f"], tau, K6, LOG_L)[:n]
    clog = P.poly_eval(o["f"], tau)
    pair = o["key"].fold_cosets(o["pp"], LOG_L, o["coms"][:n], o["zs"][:n], o["ys"][:n], o["wits"][:n],
                                weights=fr_np(rhos))
    want = KC.fold_cosets_pair_logs([clog] * n, zs, rows, wlogs, rhos, tau, LOG_L)
    assert np.array_equal(pair, K.gen_mul_np(want))
    assert o["key"].check(pair)


def test_one_opening_with_weight_one_is_its_own_pair(plk, gpu_ctx, opened):
    o, j, tau, l = opened, 11, opened["tau"], 1 << LOG_L
    pair = o["key"].fold_cosets(o["pp"], LOG_L, o["com"], o["zs"][j], o["ys"][j], o["wits"][j], weights=fr_np([1]))
    z = o["zs_int"][j]
    interp = KC.coset_interpolant(P.fr_vec_from_np(o["ys"][j]), z, LOG_L)
    wlog = KC.coset_witness_logs(o["f"], tau, K6, LOG_L)[j]
    clog = (P.poly_eval(o["f"], tau) - P.poly_eval(interp, tau) + pow(z, l, R) * wlog) % R
    assert np.array_equal(pair, K.gen_mul_np([clog, wlog]))
    assert np.array_equal(pair[1], o["wits"][j])
    # the weights drawn inside the library start at rho_0 = 1: the same pair
    assert np.array_equal(pair, o["key"].fold_cosets(o["pp"], LOG_L, o["com"], o["zs"][j], o["ys"][j], o["wits"][j]))


def test_shifts_outside_the_domain(plk, gpu_ctx, opened):
    o, tau, l = opened, opened["tau"], 1 << LOG_L
    rng = P.SplitMix64(41)
    zs = [rng.fr() for _ in range(3)] + [1, R - 1]
    rows = [KC.coset_values(o["f"], z, LOG_L) for z in zs]
    wits = K.gen_mul_np([P.poly_eval(KC.divide_by_coset(o["f"], l, pow(z, l, R))[0], tau) for z in zs])
    ys = np.stack([fr_np(row) for row in rows])
    assert o["key"].check_cosets(o["pp"], LOG_L, o["com"], fr_np(zs), ys, wits)
    ys[1, 2] = fr_np([(rows[1][2] + 1) % R])[0]
    assert not o["key"].check_cosets(o["pp"], LOG_L, o["com"], fr_np(zs), ys, wits)


def test_fold_at_one_point_per_coset_is_fold_openings_byte_for_byte(plk, gpu_ctx, opened):
    o, n = opened, 9
    pp = o["pp"]
    values, wit = pp.open_cosets(K6, 0, fr_np(o["f"]))
    zs = fr_np(shifts_of(K6, 0)[:n])
    rng = P.SplitMix64(43)
    rhos = fr_np([1, 0, R - 1] + [rng.fr() for _ in range(n - 3)])
    a = o["key_tau"].fold_cosets(pp, 0, o["com"], zs, values.values[:n], wit[:n], weights=rhos)
    b = o["key_tau"].fold_openings(pp.points(0, 1)[0], np.tile(o["com"], (n, 1)), zs, values.values[:n], wit[:n],
                                   weights=rhos, ctx=gpu_ctx)
    assert np.array_equal(a, b)
    assert o["key_tau"].check(a)
    assert o["key_tau"].check_cosets(pp, 0, o["com"], zs, values.values[:n], wit[:n])


def test_power_key_matches(plk, gpu_ctx, opened):
    o = opened
    assert o["pp"].power_key_matches(o["key"], LOG_L)
    assert not o["pp"].power_key_matches(o["key_tau"], LOG_L)
    assert o["pp"].power_key_matches(o["key_tau"], 0)
    assert not o["pp"].power_key_matches(o["key"], 0)
    assert not o["pp"].power_key_matches(o["key"], 1)


def test_fold_refusals(plk, gpu_ctx, opened):
    o, n = opened, 3
    args = [o["coms"][:n], o["zs"][:n], o["ys"][:n], o["wits"][:n]]
    big = P.fr_vec_to_np([R], mont=False)[0]
    zero = fr_np([0])[0]

    def refused(*a, pp=o["pp"], log_l=LOG_L, **kw):
        with pytest.raises(plk.PlonkError) as e:
            o["key"].fold_cosets(pp, log_l, *a, **kw)
        assert e.value.status == plk.PLK_E_ARG

    for which, at, repl in ((1, 2, big), (1, 1, zero), (2, (2, 3), big), (2, (0, 0), big)):
        a = [x.copy() for x in args]
        a[which][at] = repl
        refused(*a)
    for which in (0, 3):
        a = [x.copy() for x in args]
        a[which][1, 6] ^= np.uint64(1)  # y: off the curve
        refused(*a)
    refused(*args, weights=np.stack([big] * n))
    refused(np.zeros((0, 13), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64),
            np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 13), dtype=np.uint64))
    small = _params(plk, 2, "random")  # 12 points: shorter than 16
    refused(args[0][:1], args[1][:1], np.tile(args[2][0, 0], (16, 1)), args[3][:1], pp=small, log_l=4)
    refused(args[0][:1], args[1][:1], args[2][0, :1], args[3][:1], log_l=21)
