"""The fixed-base MSM stage by stage on the GPU (plk_debug_msm_snapshot) against the integer model
of tests/msm_stage_ref.py: digits, sort, task records, accumulation partials, bucket or run sums,
bit sums, host tail. Integers are compared bit for bit, device XYZZ rows as curve points; nothing
has a tolerance. Every case also checks that the hook's final point is the one the public entry
point (plk_commit_batch_dev[_part]) returns for the same input.

Model cost, measured (host Python, one CPU core, the model on a layout of its own, no
GPU): recoding, the integer checks and the stage chain 0.16 s at 1 025 scalars and c = 13
(20 500 entries), 0.04 s at 256 scalars and c = 17; a device row met as a curve point costs one
fixed-base multiplication, 0.35-0.4 ms, so the point stages of the largest point shapes take
1.9 s (1 025 scalars at c = 13: 4 843 distinct points) and 1.4 s (256 scalars at c = 17: 4 063);
the integer stages at 32 768 scalars take about a second. With the GPU the slowest case of this
file ran 1.1 s and the whole file 26 s.
"""
import collections
import random

import numpy as np
import pytest

import msm_stage_ref as M
import pyref as P

pytestmark = pytest.mark.gpu

R = P.R_MOD
TAU = 0x2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F80912 % R
Q = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % R  # Q = Q G
EQUAL_RUNS = (8, 9, 16, 17, 32, 64, 65, 128)  # chunk, chunk + 1, 2 chunk for chunk = 8, 16, 64

_SRS = {}
STATS = {"path": collections.Counter(), "accumulate": collections.Counter(), "tally": M.Tally()}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    _SRS.clear()
    print("\n[msm-stage] cases per sort path:", dict(STATS["path"]))
    print("[msm-stage] cases per k_accumulate<HAS_INF, LONE>:", dict(STATS["accumulate"]))
    print("[msm-stage] events:", STATS["tally"].as_dict())


def tau_srs(plk, ctx, c, n, tau=TAU):
    """An n-point SRS of tau with window size c forced, and its points' multiples of G."""
    key = (c, n, tau)
    if key not in _SRS:
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PLK_MSM_C", str(c))
            pp = plk.PlonkParams.setup(max(1, (n - 1).bit_length()), P.fr_vec_to_np([tau])[0], ctx,
                                       n_points=n)
        dlog, t = [], 1
        for _ in range(n):
            dlog.append(t)
            t = t * tau % R
        _SRS[key] = (pp, dlog)
    return _SRS[key]


def loaded_srs(plk, ctx, c, dlog):
    """An SRS loaded from chosen points dlog[i] G (0: the identity)."""
    key = (c, tuple(dlog))
    if key not in _SRS:
        pts = P.g1_vec_to_np([M.affine_dlog(k) for k in dlog])
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PLK_MSM_C", str(c))
            pp = plk.PlonkParams.load(pts, ctx)
        _SRS[key] = (pp, list(dlog))
    return _SRS[key]


def scalar_set(c, n, seed, equal_runs=EQUAL_RUNS):
    """n scalars: the layout's edge scalars in both signs (rotated by the seed when n is short),
    runs of equal scalars, random ones."""
    rng = random.Random(seed)
    edges = M.edge_scalars(P.msm_window_layout(c))
    rot = seed % len(edges)
    out = edges[rot:] + edges[:rot]
    for run in equal_runs:
        if len(out) + run <= n:
            out += [rng.randrange(R)] * run
    out += [rng.randrange(R) for _ in range(max(0, n - len(out)))]
    return out[:n]


def sort_path(h):
    if h["wide"]:
        return f"wide_fb{h['fb']}"
    if h["sort_one"]:
        return "sort_one_hold" if h["hold"] else "sort_one_big"
    return "hist_sort_small" if h["B"] <= 4096 else "hist_scan"


def public_points(plk, pp, arrs, part, parts):
    import torch
    devs = [torch.from_numpy(a.view(np.int64).copy()).cuda() for a in arrs]
    torch.cuda.synchronize()
    return pp.commit_batch_dev([(d.data_ptr() if a.shape[0] else 0, a.shape[0]) for d, a in zip(devs, arrs)],
                               raise_on_error=False, part=part, parts=parts)


def run_case(plk, pp, dlog, slots, oracle=None, points=True, shared_chip=False, tail_quad=1,
             part=0, parts=1, guard_limit=0):
    """One snapshot of a batch, every stage of every slot against the model. Returns (header,
    slots' snapshots, tally of this case)."""
    arrs = [P.fr_vec_to_np(s) if len(s) else np.zeros((0, 4), np.uint64) for s in slots]
    h, snap = plk.plonk.debug_msm_snapshot(pp, arrs, shared_chip=shared_chip, tail_quad=tail_quad,
                                           part=part, parts=parts, guard_limit=guard_limit,
                                           points=points)
    B, n_srs = h["B"], h["n_srs"]
    assert len(dlog) == n_srs
    STATS["path"][sort_path(h)] += 1
    STATS["accumulate"][f"<{bool(h['has_inf'])}, {not shared_chip}>".lower()] += 1
    tally = M.Tally()
    public = public_points(plk, pp, arrs, part, parts)
    for k, (sc, d) in enumerate(zip(slots, snap)):
        where = f"slot {k} of {len(slots)}, len {len(sc)}, c {h['c']}"
        use = sc[:n_srs]
        tail_nonzero = any(s % R for s in sc[n_srs:])
        # ---- integer stages
        entries = M.entries_of(use, h)
        n = M.check_sorted(entries, d["offsets"], d["sorted"], B)
        assert d["entries"] == n == int(d["offsets"][B]), where
        counts = np.diff(d["offsets"].astype(np.int64))
        hot = bool(guard_limit) and int(counts.max(initial=0)) > guard_limit
        if guard_limit:
            assert d["max_count"] == int(counts.max(initial=0)), where
        assert (d["flag"] == h["gen"]) == tail_nonzero, where
        assert d["status"] == (plk.PLK_E_DEGREE if tail_nonzero else plk.PLK_OK), where
        if hot:  # k_guard cleared the slot's tasks: nothing accumulated, a void output, status OK
            assert not d["task_off"].any() and len(d["tasks"]) == 0, where
            assert not d["point"].any(), where
            continue
        first, length, pidx = M.check_tasks(h, d["offsets"], d["task_off"], d["tasks"])
        # ---- point stages
        want = M.direct_dlog(h, dlog, use)
        if points:
            t = M.Tally()
            out = M.model_chain(h, dlog, d["offsets"], d["sorted"], d["task_off"], d["tasks"], t)
            tally.merge(t)
            for p, kp in enumerate(out["partials"]):
                M.check_row(d["partials"][p], kp, M.BOUND_2P, f"{where}: partials[{p}]")
            if h["wide"]:
                M.check_rows_sparse(d["rsum"], out["rsum"], M.BOUND_LAZY, f"{where}: rsum")
                M.check_rows_sparse(d["ys"], out["ys"], M.BOUND_2P, f"{where}: ys")
                M.check_rows_sparse(d["zs"], out["zs"], M.BOUND_2P, f"{where}: zs")
            else:
                M.check_rows_sparse(d["bsum"], out["bsum"], M.BOUND_LAZY, f"{where}: bsum")
            for j, kj in enumerate(out["bits"]):
                M.check_row(d["bits"][j], kj, M.BOUND_2P, f"{where}: T_{j}")
            assert out["final"] == want, where
        # ---- the final point: the definition, the oracle, the public entry point
        if tail_nonzero:
            assert not d["point"].any(), where
            assert isinstance(public[k], plk.PlonkError) and public[k].status == plk.PLK_E_DEGREE
            continue
        assert P.g1_vec_from_np(d["point"])[0] == M.affine_dlog(want), where
        if oracle is not None and parts == 1 and len(use):
            assert np.array_equal(d["point"], oracle.msm(pp.points(0, len(use)), arrs[k][:len(use)])), where
        assert np.array_equal(public[k].words, d["point"]), where
    STATS["tally"].merge(tally)
    return h, snap, tally


# ------------------------------------------------------------------------------- sort paths
@pytest.mark.parametrize("n", [1, 63, 1024, 1025, 8192])
@pytest.mark.parametrize("c", [8, 10, 12, 13])
def test_sort_one_hold(plk, gpu_ctx, oracle, c, n):
    """k_sort_one<C, HOLD> (B <= 4096, <= 8192 scalars, chunk floor 8): compile-time layouts 10,
    12, 13 and the run-time digit_at at c = 8. Point stages up to 1025 scalars."""
    pp, dlog = tau_srs(plk, gpu_ctx, c, 8192)
    h, _, _ = run_case(plk, pp, dlog, [scalar_set(c, n, 1000 * c + n)], oracle, points=n <= 1025)
    assert sort_path(h) == "sort_one_hold" and h["chunk"] == 8 and h["c"] == c


@pytest.mark.parametrize("c,n", [(10, 8193), (10, 32768), (13, 8193), (13, 32768)])
def test_sort_one_big(plk, gpu_ctx, oracle, c, n):
    """k_sort_one<C, !HOLD> (8192 < scalars <= 32768, chunk floor 16); integer stages and the
    final point."""
    pp, dlog = tau_srs(plk, gpu_ctx, c, 32769)
    h, _, _ = run_case(plk, pp, dlog, [scalar_set(c, n, 7 * c + n)], oracle, points=False)
    assert sort_path(h) == "sort_one_big" and h["chunk"] == 16


def test_hist_sort_small(plk, gpu_ctx, oracle):
    """k_hist + k_sort_small + k_scatter (B <= 4096, more than 32768 scalars)."""
    pp, dlog = tau_srs(plk, gpu_ctx, 10, 32769)
    h, _, _ = run_case(plk, pp, dlog, [scalar_set(10, 32769, 5)], oracle, points=False)
    assert sort_path(h) == "hist_sort_small"


@pytest.mark.parametrize("n", [1, 257, 513, 4096])
@pytest.mark.parametrize("c", [14, 15, 16])
def test_hist_scan(plk, gpu_ctx, oracle, c, n):
    """k_hist + k_block_scan + k_scan_buckets + k_scatter + k_make_tasks (4096 < B <= 32768):
    the compile-time layout 15 and digit_at at 14 and 16. Nearly every entry has a bucket of its
    own here (~9 000 distinct points at 513 scalars), so the point stages stop at 513."""
    pp, dlog = tau_srs(plk, gpu_ctx, c, 4096)
    h, _, _ = run_case(plk, pp, dlog, [scalar_set(c, n, 31 * c + n)], oracle, points=n <= 513)
    assert sort_path(h) == "hist_scan" and h["chunk"] == 16


WIDE = [  # (c forced, effective c, parts, fb)
    (17, 17, 1, 10), (17, 17, 2, 9), (17, 17, 4, 8), (18, 17, 1, 10), (20, 20, 1, 10),
    (20, 20, 2, 9), (20, 20, 8, 8)]


@pytest.mark.parametrize("n", [1, 64, 256, 1024])
@pytest.mark.parametrize("c,c_eff,parts,fb", WIDE, ids=[f"c{r[0]}p{r[2]}" for r in WIDE])
def test_wide_lone(plk, gpu_ctx, oracle, c, c_eff, parts, fb, n):
    """Wide sets, a lone MSM: k_chist, k_cscatter, k_fine<FB>, k_make_tasks_wide<FB>, every part at
    64 scalars and the first and last otherwise. Point stages up to 256 scalars (~3 800 partials
    and as many run sums there), integer stages at 1024."""
    pp, dlog = tau_srs(plk, gpu_ctx, c, 1024)
    sc = scalar_set(c_eff, n, 13 * c + n)
    every = n == 64 or parts == 1
    total = 0
    for part in range(parts) if every else (0, parts - 1):
        pts = n <= 256
        h, snap, _ = run_case(plk, pp, dlog, [sc], oracle, points=pts, part=part, parts=parts)
        assert sort_path(h) == f"wide_fb{fb}" and h["c"] == c_eff and h["b_lo"] == part * h["B"]
        total += M.direct_dlog(h, dlog, sc)
    if every:  # the parts' shares sum to the whole
        assert total % R == sum(s * q for s, q in zip(sc, dlog)) % R


@pytest.mark.parametrize("c,parts", [(17, 1), (17, 4), (20, 1), (20, 8)])
def test_wide_batch(plk, gpu_ctx, oracle, c, parts):
    """Wide sets in a batch (chunk = 64, the batch's run width): unequal lengths, 64, 65 and 128
    equal scalars (the task length field at its maximum, 63), an empty and an all-zero slot."""
    pp, dlog = tau_srs(plk, gpu_ctx, c, 1024)
    skew = scalar_set(c, 300, 3, equal_runs=(64, 65, 128))
    slots = [skew, [], [0] * 17, scalar_set(c, 64, 4), scalar_set(c, 1, 5)]
    pts = c == 17 or parts > 1  # c = 20 whole: 2^19 run-sum rows per slot, two slots below
    for part in (0, parts - 1) if parts > 1 else (0,):
        h, snap, _ = run_case(plk, pp, dlog, slots, oracle, points=pts, part=part, parts=parts)
        assert h["wide"] and h["chunk"] == 64
        if parts == 1:
            _, length, _ = M.unpack_tasks(snap[0]["tasks"])
            assert length.max() == 64 and 1 in length
    if parts == 1:  # integer stages at 1024 scalars, two slots; point stages on two short ones
        run_case(plk, pp, dlog, [scalar_set(c, 1024, 6), scalar_set(c, 1000, 7)], oracle, points=False)
        run_case(plk, pp, dlog, [skew[:256], scalar_set(c, 64, 4)], oracle, points=True)


@pytest.mark.parametrize("c", [10, 15, 17])
def test_batch_of_16(plk, gpu_ctx, oracle, c):
    """16 slots of unequal lengths, an empty slot and an all-zero slot, on a sort_one, a k_hist
    and a wide SRS, and 2 slots of it, point stages on every slot."""
    n_srs = 200
    pp, dlog = tau_srs(plk, gpu_ctx, c, n_srs)
    lens = [200, 0, 17, 1, 63, 64, 65, 128, 2, 3, 133, 16, 8, 9, 100, 33]
    slots = [scalar_set(c, n, 50 + i) for i, n in enumerate(lens)]
    slots[2] = [0] * 17
    slots[10] = [slots[10][0]] * 133  # all scalars equal: W buckets of 133 entries
    h, _, _ = run_case(plk, pp, dlog, slots, oracle, points=True)
    assert h["chunk"] == (64 if c == 17 else 8 if c == 10 else 16)
    run_case(plk, pp, dlog, [slots[4], slots[5]], oracle, points=True)


# ---------------------------------------------------------------- guard and degree check
@pytest.mark.parametrize("c", [10, 15, 17])
def test_guard_and_degree_check(plk, gpu_ctx, oracle, c):
    """guard_limit: max_count is the largest bucket count and a slot over the limit is void with
    status OK. A check_len tail: zero passes, a non-zero coefficient gives PLK_E_DEGREE and a
    stamped flag (run_case holds both to the model)."""
    n_srs = 400
    pp, dlog = tau_srs(plk, gpu_ctx, c, n_srs)
    quiet = scalar_set(c, 100, 1, equal_runs=(8,))
    # the limit is the quiet slot's own largest bucket (at the limit is not over it); limit + 1
    # equal scalars then put limit + 1 entries into one bucket per window at least
    hm = M.header(c=c, n_srs=n_srs)
    limit = int(np.bincount([b for b, _ in M.entries_of(quiet, hm)]).max())
    assert limit < n_srs
    hot = [TAU] * (limit + 1)
    h, snap, _ = run_case(plk, pp, dlog, [quiet, hot, []], oracle, points=False, guard_limit=limit)
    assert snap[0]["max_count"] == limit < snap[1]["max_count"] and snap[2]["max_count"] == 0
    assert snap[1]["status"] == plk.PLK_OK and len(snap[1]["tasks"]) == 0 and len(snap[0]["tasks"])
    assert not snap[1]["point"].any() and snap[0]["point"].any()
    full = scalar_set(c, n_srs, 2)
    zero_tail = full + [0] * 9
    bad_tail = full + [0] * 8 + [5]
    h, snap, _ = run_case(plk, pp, dlog, [zero_tail, bad_tail, full[:50]], oracle, points=False)
    assert [d["status"] for d in snap] == [plk.PLK_OK, plk.PLK_E_DEGREE, plk.PLK_OK]
    assert snap[1]["flag"] == h["gen"] != snap[0]["flag"]
    h, snap, _ = run_case(plk, pp, dlog, [bad_tail], oracle, points=False)  # lone
    assert snap[0]["status"] == plk.PLK_E_DEGREE


# -------------------------------------------------- exceptional additions inside the loops
FORMS = [(sc, tq) for sc in (False, True) for tq in (0, 1, 2)]
FORM_IDS = [f"shared{int(sc)}-quad{tq}" for sc, tq in FORMS]
S_EQ = 0x0123456789ABCDEF0FEDCBA9876543210123456789ABCDEF0FEDCBA987654321 % R


def accumulate_events(t):
    return t.n["accumulate"]


@pytest.mark.parametrize("shared_chip,tail_quad", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("c", [10, 17])
def test_accumulate_exceptional(plk, gpu_ctx, c, shared_chip, tail_quad):
    """Equal scalars put an SRS prefix into one task per window, so k_accumulate's prefetch loop
    meets, whatever order the sort left: {Q, Q} a doubling at the second entry; {Q, -Q} a partial
    at infinity; {O, O} a first entry and a partial at infinity; {Q, -Q, Q} a doubling, or a
    cancellation and an addition onto infinity. tau = 1 and tau = -1 run <HAS_INF = false>, the
    loaded SRSs (identity points among Q and -Q) <HAS_INF = true>; shared_chip picks LONE. Lone
    and in a batch (another chunk on the narrow set, another run width on the wide one)."""
    kw = dict(shared_chip=shared_chip, tail_quad=tail_quad)
    eq = lambda n: [S_EQ] * n
    # tau = 1: {G, G}, and longer runs of G through the loop (tasks of chunk and a tail)
    pp, dlog = tau_srs(plk, gpu_ctx, c, 160, tau=1)
    for slots in ([eq(2)], [eq(2), eq(3), eq(150), eq(64)]):
        h, _, t = run_case(plk, pp, dlog, slots, **kw)
        a = accumulate_events(t)
        assert not h["has_inf"] and a["equal"] >= 1, dict(a)
    # tau = -1: {G, -G} and {G, -G, G}
    pp, dlog = tau_srs(plk, gpu_ctx, c, 160, tau=R - 1)
    for slots in ([eq(2)], [eq(3)], [eq(2), eq(3), eq(150)]):
        h, _, t = run_case(plk, pp, dlog, slots, **kw)
        a = accumulate_events(t)
        if len(slots[0]) == 2:
            assert a["opposite"] >= 1 and a["partial_inf"] >= 1, dict(a)
        else:
            assert a["equal"] >= 1 or (a["opposite"] >= 1 and a["acc_inf"] >= 1), dict(a)
    # chosen points: {Q, -Q} then Q; {O, O} then Q, Q, -Q, O ...
    srs_a = [Q, R - Q, Q, Q, 0, R - Q, R - Q, Q, 0, 0, Q, Q] + [Q, R - Q] * 30
    srs_b = [0, 0, Q, Q, R - Q, 0, Q, R - Q, 0, Q] + [Q] * 20 + [0, R - Q] * 20
    pp, dlog = loaded_srs(plk, gpu_ctx, c, srs_a)
    for slots in ([eq(2)], [eq(3)], [eq(3), eq(2), eq(12), eq(72)]):
        h, _, t = run_case(plk, pp, dlog, slots, **kw)
        a = accumulate_events(t)
        assert h["has_inf"]
        if len(slots[0]) == 2:
            assert a["opposite"] >= 1 and a["partial_inf"] >= 1, dict(a)
        else:
            assert a["equal"] >= 1 or (a["opposite"] >= 1 and a["acc_inf"] >= 1), dict(a)
    pp, dlog = loaded_srs(plk, gpu_ctx, c, srs_b)
    for slots in ([eq(2)], [eq(4)], [eq(2), eq(10), eq(70)]):
        h, _, t = run_case(plk, pp, dlog, slots, **kw)
        a = accumulate_events(t)
        assert h["has_inf"] and a["operand_inf"] >= 2, dict(a)
        if len(slots[0]) == 2:
            assert a["partial_inf"] >= 1 and (len(slots) > 1 or a["adds"] == 0), dict(a)
        if len(slots[0]) == 4:  # {O, O, Q, Q}: an addition onto infinity or a doubling
            assert a["acc_inf"] >= 1 or a["equal"] >= 1, dict(a)


@pytest.mark.parametrize("shared_chip,tail_quad", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("c", [17, 20])
def test_runsum_exceptional(plk, gpu_ctx, c, shared_chip, tail_quad):
    """tau = 1 and scalars below 2^(c-1): scalar d is one entry, G (or -G for r - d), of bucket
    d - 1. k_runsum1 and k_runsum2 add in a fixed order, so the model's tally is exact: adjacent
    buckets of a run holding G and G (R + S a doubling), G and -G (a cancellation), a run whose top
    buckets are empty, R_(r,0) = R_(r,1) (k_runsum2's doubling) and R_(r,0) = -R_(r,1) (its
    cancellation). Lone and in a batch (rb differs)."""
    pp, dlog = tau_srs(plk, gpu_ctx, c, 64, tau=1)
    d = 0x1000  # bucket d - 1 = 0xfff odd; d + 1 -> bucket 0x1000 starts a run
    sc = [
        d + 1, d + 2,                  # buckets 0x1000, 0x1001: G, G -> R + S doubles
        d + 33, R - (d + 34),          # 0x1020: G, 0x1021: -G -> R + S cancels
        d + 66,                        # 0x1041 alone: R_(r,0) = R_(r,1), k_runsum2 doubles
        d + 98, R - (d + 97), R - (d + 97),  # 0x1061: G, 0x1060: -2G -> R_(r,0) = -R_(r,1)
        d + 130, d + 130,              # 0x1081: {G, G} in one task
        d + 161,                       # 0x10a0 alone, the run's lowest: R_(r,1) is the identity
    ]
    for slots in ([sc], [sc, sc[:2], sc[2:4]]):
        h, _, t = run_case(plk, pp, dlog, slots, shared_chip=shared_chip, tail_quad=tail_quad)
        assert h["wide"] and h["rb"] >= 1
        r1, r2 = t.n["runsum1"], t.n["runsum2"]
        assert r1["equal"] >= 1 and r1["opposite"] >= 1 and r1["result_inf"] >= 1, dict(r1)
        assert r1["top_bucket_empty"] >= 1 and r1["acc_inf"] >= 1, dict(r1)
        assert r2["equal"] >= 1 and r2["opposite"] >= 1 and r2["operand_inf"] >= 1, dict(r2)
        assert t.n["accumulate"]["equal"] >= 1
