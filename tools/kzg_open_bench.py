#!/usr/bin/env python3
"""kzg_open_bench.py — time the KZG openings (csrc/kzg.hip, csrc/g1_ntt.hip).

For n = 2^8, 2^12 and 2^16 (--log-sizes) it measures, in one run on one box:

  * PlonkParams.open_domain of a dense polynomial of n coefficients, once per form of the G1
    transform (PLK_G1_NTT_FORM = xyzz / glv, a fresh SRS object each): the first call's wall clock
    and table build (plk_kzg_last_open_ms), then warm calls: wall clock and the HIP-event split
    into transforms and pointwise multiplication. From the table build, one forward transform of
    2n points, the time per twiddle multiplication of that form: table_ms over
    n log2(2n) - (2n - 1) multiplications (batch inversions and additions included).
  * the route a caller had before these entries, per point one compute_aggregate_witness and one
    commit, over --loop-points points (256) and extrapolated linearly to n points;
  * PlonkParams.open (one upload, 16 quotients per commit batch) over the same points.

And for 1, 64, 4 096 and 65 536 openings (--fold-counts) of a 2^16 open_domain:
OpeningKey.fold_openings plus one host check, against that many host checks (one check timed in
the same run, times the count).

Medians over --rounds rounds after --warmup untimed ones. One JSON line per size and per fold
count is appended to profiles/kzg_open.jsonl (or --out). Fails without a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FORMS = ("xyzz", "glv")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--log-sizes", type=int, nargs="+", default=[8, 12, 16])
    ap.add_argument("--fold-counts", type=int, nargs="+", default=[1, 64, 4096, 65536])
    ap.add_argument("--loop-points", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kzg_open.jsonl"))
    ns = ap.parse_args(argv)

    import numpy as np
    import dusk_plonk_amd as plk

    info = plk.check_build()
    if plk.device_count() == 0:
        raise SystemExit("kzg_open_bench.py: no GPU visible")
    ctx = plk.Context.default(0)
    tau = np.array([3, 1, 4, 1], dtype=np.uint64)
    one = plk.plonk._fr_limbs(1)
    rng = np.random.default_rng(8349)
    build = {k: info[k] for k in ("src", "flags", "variant", "tree_src")}

    def wall(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def med(vals):
        return round(statistics.median(vals), 4)

    def poly(n):
        f = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
        f[:, 3] >>= np.uint64(2)  # below 2^253 < r: canonical limbs
        return f

    lines = []
    last = None
    for log_n in ns.log_sizes:
        n = 1 << log_n
        f = poly(n)
        fc = plk.Coefficients(f)
        rec = {"tool": "kzg_open_bench", "log_n": log_n, "points": n, "rounds": ns.rounds, "warmup": ns.warmup}
        mults = n * (log_n + 1) - (2 * n - 1)  # a forward transform of 2n points
        ref = None
        for form in FORMS:
            os.environ["PLK_G1_NTT_FORM"] = form
            pp = plk.PlonkParams.setup(log_n, tau, ctx)
            (values, wit), ms = wall(lambda: pp.open_domain(log_n, fc))
            rec[f"{form}_first_ms"] = round(ms, 4)
            table_ms = plk.kzg_last_open_ms(ctx)[2]
            rec[f"{form}_table_ms"] = round(table_ms, 4)
            rec[f"{form}_table_ns_per_mul"] = round(table_ms * 1e6 / mults, 2)
            if ref is None:
                ref = wit
            elif not np.array_equal(ref, wit):
                raise SystemExit("kzg_open_bench.py: the two forms disagree")
            ws, ts, ms_ = [], [], []
            for rnd in range(ns.warmup + ns.rounds):
                _, ms = wall(lambda: pp.open_domain(log_n, fc))
                if rnd >= ns.warmup:
                    t = plk.kzg_last_open_ms(ctx)
                    ws.append(ms)
                    ts.append(t[0])
                    ms_.append(t[1])
            rec[f"{form}_warm_ms"], rec[f"{form}_transform_ms"], rec[f"{form}_mul_ms"] = med(ws), med(ts), med(ms_)
            last = (pp, f, values, wit, log_n)
        os.environ.pop("PLK_G1_NTT_FORM", None)
        pp = last[0]
        m = min(n, ns.loop_points)
        zs = plk.Fft(log_n, ctx).elements[:m].copy()

        def loop():
            for i in range(m):
                pp.commit(pp.compute_aggregate_witness([fc], zs[i], one))

        loops, opens = [], []
        for rnd in range(ns.warmup + ns.rounds):
            _, ms = wall(loop)
            (_, w2), ms2 = wall(lambda: pp.open(fc, zs))
            if rnd >= ns.warmup:
                loops.append(ms)
                opens.append(ms2)
        if not np.array_equal(w2, ref[:m]):
            raise SystemExit("kzg_open_bench.py: open and open_domain disagree")
        rec["loop_points"] = m
        rec["loop_ms_per_point"] = round(statistics.median(loops) / m, 5)
        rec["loop_ms_extrapolated"] = round(statistics.median(loops) / m * n, 3)
        rec["open_ms_per_point"] = round(statistics.median(opens) / m, 5)
        for form in FORMS:
            rec[f"loop_over_{form}_warm"] = round(rec["loop_ms_extrapolated"] / rec[f"{form}_warm_ms"], 2)
        rec["build_id"] = build
        lines.append(rec)

    if ns.fold_counts:
        pp, f, values, wit, log_n = last
        n = 1 << log_n
        key = plk.OpeningKey.setup(tau)
        g = pp.points(0, 1)[0]
        com = pp.commit(plk.Coefficients(f)).words
        zs = plk.Fft(log_n, ctx).elements
        key.check(key.fold_openings(g, com, zs[0], values.values[0], wit[0], ctx=ctx))  # untimed first use
        checks = []
        for _ in range(5):
            pair = key.fold_openings(g, com, zs[1], values.values[1], wit[1], ctx=ctx)
            t0 = time.perf_counter()
            ok = key.check(pair)
            checks.append((time.perf_counter() - t0) * 1e3)
            if not ok:
                raise SystemExit("kzg_open_bench.py: a true opening was rejected")
        one_check = statistics.median(checks)
        for count in ns.fold_counts:
            c = min(count, n)
            coms = np.tile(com, (c, 1))
            folds, totals = [], []
            for rnd in range(ns.warmup + ns.rounds):
                pair, ms = wall(lambda: key.fold_openings(g, coms, zs[:c], values.values[:c], wit[:c], ctx=ctx))
                t0 = time.perf_counter()
                ok = key.check(pair)
                ms2 = (time.perf_counter() - t0) * 1e3
                if not ok:
                    raise SystemExit("kzg_open_bench.py: the fold of true openings was rejected")
                if rnd >= ns.warmup:
                    folds.append(ms)
                    totals.append(ms + ms2)
            lines.append({"tool": "kzg_open_bench", "fold_openings": c, "fold_ms": med(folds),
                          "fold_and_check_ms": med(totals), "host_check_ms": round(one_check, 4),
                          "host_checks_ms": round(one_check * c, 3),
                          "host_checks_over_fold_and_check": round(one_check * c / statistics.median(totals), 2),
                          "rounds": ns.rounds, "warmup": ns.warmup, "build_id": build})

    with open(ns.out, "a") as fh:
        for rec in lines:
            line = json.dumps(rec)
            fh.write(line + "\n")
            print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
