"""The row-table layout of the fixed-base MSM (PLK_MSM_NAF = 1: a table row per bit position, the
scalars recoded as a signed sliding window) on the GPU: the device's digits and sort against the
integer model of tests/msm_naf_ref.py through plk_debug_msm_snapshot, integer for integer; the
commits against the oracle's MSM; a bucket-range split against the whole; a proof against the same
proof on the window table, byte for byte. Nothing has a tolerance.

The snapshot's `sorted` holds every digit the device emitted as its entry code (position n_srs +
index, sign) under its bucket, so the digit stage is compared through the sort stage.
"""
import numpy as np
import pytest

import msm_naf_ref as N
import msm_stage_ref as M
import pyref as P

pytestmark = pytest.mark.gpu

R = P.R_MOD
TAU = 0x2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F80912 % R
Q = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % R
C = 17
N_SRS = 1025
_SRS = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_srs():
    yield
    _SRS.clear()


def setup_srs(plk, ctx, naf, n=N_SRS, cap=None):
    """An n-point SRS of TAU at c = 17 with the layout forced, and its points' multiples of G."""
    key = ("tau", naf, n, cap)
    if key not in _SRS:
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PLK_MSM_C", str(C))
            mp.setenv("PLK_MSM_NAF", "1" if naf else "0")
            if cap is not None:
                mp.setenv("PLK_MSM_TABLE_CAP", str(cap))
            pp = plk.PlonkParams.setup(max(1, (n - 1).bit_length()), P.fr_vec_to_np([TAU])[0], ctx,
                                       n_points=n)
        dlog, t = [], 1
        for _ in range(n):
            dlog.append(t)
            t = t * TAU % R
        _SRS[key] = (pp, dlog)
    return _SRS[key]


def loaded_srs(plk, ctx, dlog):
    key = ("loaded", tuple(dlog))
    if key not in _SRS:
        pts = P.g1_vec_to_np([M.affine_dlog(k) for k in dlog])
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PLK_MSM_C", str(C))
            mp.setenv("PLK_MSM_NAF", "1")
            pp = plk.PlonkParams.load(pts, ctx)
        _SRS[key] = (pp, list(dlog))
    return _SRS[key]


def scalar_set(n, seed):
    """n scalars: the recoding's edge scalars in both signs (rotated by the seed when n is short),
    runs of equal scalars, random ones."""
    import random
    rng = random.Random(seed)
    edges = N.edge_scalars(C)
    rot = seed % len(edges)
    out = edges[rot:] + edges[:rot]
    for run in (8, 65):
        if len(out) + run <= n:
            out += [rng.randrange(R)] * run
    out += [rng.randrange(R) for _ in range(max(0, n - len(out)))]
    return out[:n]


def public_points(pp, arrs, part=0, parts=1):
    import torch
    devs = [torch.from_numpy(a.view(np.int64).copy()).cuda() for a in arrs]
    torch.cuda.synchronize()
    return pp.commit_batch_dev([(d.data_ptr() if a.shape[0] else 0, a.shape[0]) for d, a in zip(devs, arrs)],
                               raise_on_error=False, part=part, parts=parts)


def run_case(plk, pp, dlog, slots, oracle=None, part=0, parts=1):
    """One snapshot of a batch: every slot's sort and task records against the model, its point
    against the definition, the oracle and the public entry point. Returns the points."""
    assert pp.table_layout() == {"naf": True, "rows": 255,
                                 "table_bytes": 255 * len(dlog) * 97}
    arrs = [P.fr_vec_to_np(s) if len(s) else np.zeros((0, 4), np.uint64) for s in slots]
    h, snap = plk.plonk.debug_msm_snapshot(pp, arrs, part=part, parts=parts, points=False)
    assert h["c"] == C and h["wide"] and h["W"] == 15 == N.max_digits(C) and h["n_srs"] == len(dlog)
    public = public_points(pp, arrs, part, parts)
    out = []
    for k, (sc, d) in enumerate(zip(slots, snap)):
        where = f"slot {k} of {len(slots)}, len {len(sc)}, part {part}/{parts}"
        entries = N.entries_of(sc, h)
        n = M.check_sorted(entries, d["offsets"], d["sorted"], h["B"])
        assert d["entries"] == n == int(d["offsets"][h["B"]]), where
        M.check_tasks(h, d["offsets"], d["task_off"], d["tasks"])
        assert d["status"] == plk.PLK_OK, where
        want = N.direct_dlog(h, dlog, sc)
        assert P.g1_vec_from_np(d["point"])[0] == M.affine_dlog(want), where
        if oracle is not None and parts == 1 and len(sc):
            assert np.array_equal(d["point"], oracle.msm(pp.points(0, len(sc)), arrs[k])), where
        assert np.array_equal(public[k].words, d["point"]), where
        out.append(want)
    return out


@pytest.mark.parametrize("n", [1, 63, 256, 1025])
def test_recoding_and_commit(plk, gpu_ctx, oracle, n):
    """The device's digits and sort equal the model's, the commit the oracle's MSM."""
    pp, dlog = setup_srs(plk, gpu_ctx, True)
    run_case(plk, pp, dlog, [scalar_set(n, 100 + n)], oracle)


def test_batch_of_unequal_slots(plk, gpu_ctx, oracle):
    pp, dlog = setup_srs(plk, gpu_ctx, True)
    slots = [scalar_set(300, 1), scalar_set(63, 2), [], scalar_set(1025, 3)]
    run_case(plk, pp, dlog, slots, oracle)


def test_srs_with_infinity_points(plk, gpu_ctx, oracle):
    srs = [0, Q, R - Q, 0, 0, Q] + [Q, 0, R - Q, 3 * Q % R] * 16
    pp, dlog = loaded_srs(plk, gpu_ctx, srs)
    sc = scalar_set(len(srs), 9)
    run_case(plk, pp, dlog, [sc, sc[:5], [sc[1]] * len(srs)], oracle)


def test_bucket_range_split(plk, gpu_ctx, oracle):
    """parts = 2: each half of the bucket range against the model's share, their sum the whole."""
    pp, dlog = setup_srs(plk, gpu_ctx, True)
    sc = scalar_set(256, 21)
    whole = run_case(plk, pp, dlog, [sc], oracle)[0]
    shares = [run_case(plk, pp, dlog, [sc], part=part, parts=2)[0] for part in (0, 1)]
    assert sum(shares) % R == whole == sum(s * q for s, q in zip(sc, dlog)) % R


def test_table_cap_falls_back_to_windows(plk, gpu_ctx, oracle):
    """A row table above PLK_MSM_TABLE_CAP is treated as one that could not be allocated: the SRS
    gets the window table and commits as ever."""
    pp, dlog = setup_srs(plk, gpu_ctx, True, n=200, cap=200 * 96 * 100)
    lay = pp.table_layout()
    assert lay == {"naf": False, "rows": 15, "table_bytes": 15 * 200 * 97}
    sc = P.fr_vec_to_np(scalar_set(200, 5))
    assert np.array_equal(public_points(pp, [sc])[0].words, oracle.msm(pp.points(0, 200), sc))


def test_proof_equals_the_window_layout(plk):
    """One 2^13-gate proof with the row table forced at c = 17, byte for byte the window table's."""
    from dusk_plonk_amd.prover import PlonkKey
    from oracle_lib import random_fr

    class Chain:
        def __init__(self, gates, seed):
            self.gates, self.seed = gates, seed

        def synthesize(self, cs):
            cs.synthetic_chain(self.gates, self.seed)

    tau = random_fr(1, seed=13)[0]
    gates = (1 << 13) - 8 - 6
    proofs = []
    for naf in ("0", "1"):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PLK_MSM_C", str(C))
            mp.setenv("PLK_MSM_NAF", naf)
            pp = plk.PlonkParams.setup(13, tau)
            assert pp.table_layout()["naf"] == (naf == "1")
            prover, vd = PlonkKey.compile_with_circuit(pp, b"chain", Chain(gates, 1))
        proof, pi = prover.create_proof(7, Chain(gates, 2))
        proofs.append(proof.raw_bytes())
        del prover, pp
    assert proofs[0] == proofs[1]
