#!/usr/bin/env python3
"""srs_update_bench.py — time the SRS update and its verification (csrc/g1_mul.hip, srs_io.hip).

For an SRS of 2^16 and of 2^20 points (--log-sizes) it measures, in one run on one box:

  * PlonkParams.update with an explicit secret on an SRS imported from bytes (known to be in G1,
    so the point and subgroup passes are skipped): wall clock (the powers, the multiplication
    kernel, the batch inversion, the MSM table build of the new SRS, the opening key on the host),
    and the multiplication kernel alone from plk_g1_mul_last_ms (HIP events around it);
  * the same update on an SRS fresh from plk_srs_setup, which runs both passes first;
  * PlonkParams.verify_update on the result (wall clock);
  * the yardstick, in the same run: the same number of points through plk_srs_setup (wall clock),
    whose k_srs_powers performs one 255-step double-and-add per point on the packed field, and
    plk_srs_load of the same points (wall clock: upload and the MSM table build, which setup and
    update pay as well). `setup_less_load_ms` = setup - load is k_srs_powers plus one batch
    inversion up to the upload's time; `update_less_load_ms` the same for the update.

The sizes are interleaved round by round; medians over --rounds rounds after --warmup untimed
ones. One JSON line per size is appended to profiles/srs_update.jsonl (or --out). Fails without a
GPU.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--log-sizes", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "srs_update.jsonl"))
    ns = ap.parse_args(argv)

    import numpy as np
    import dusk_plonk_amd as plk

    info = plk.check_build()
    if plk.device_count() == 0:
        raise SystemExit("srs_update_bench.py: no GPU visible")
    ctx = plk.Context.default(0)
    tau = np.array([3, 1, 4, 1], dtype=np.uint64)
    secret = np.array([2, 7, 1, 8], dtype=np.uint64)
    key = plk.OpeningKey.setup(tau)

    def wall(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    sizes = {}
    for log_n in ns.log_sizes:
        n = 1 << log_n
        pp = plk.PlonkParams.setup(log_n, tau, ctx, n_points=n)
        sizes[log_n] = {"n": n, "points": pp.points(), "comp": pp.to_bytes("compressed"), "t": {}}
        del pp

    def add(t, name, v):
        t.setdefault(name, []).append(v)

    for rnd in range(ns.warmup + ns.rounds):
        for log_n in ns.log_sizes:
            s = sizes[log_n]
            n = s["n"]
            t = {} if rnd < ns.warmup else s["t"]
            imported = plk.PlonkParams.from_bytes(s["comp"], "compressed", True, ctx)
            (new, new_key, wit), ms = wall(lambda: imported.update(key, secret))
            add(t, "update_ms", ms)
            add(t, "mul_kernel_ms", plk.plonk.g1_mul_last_ms(ctx))
            v, ms = wall(lambda: new.verify_update(s["points"][1], new_key, wit))
            if not v.ok:
                raise SystemExit(f"srs_update_bench.py: verify_update said {v!r}")
            add(t, "verify_update_ms", ms)
            del new, new_key, imported
            fresh, ms = wall(lambda: plk.PlonkParams.setup(log_n, tau, ctx, n_points=n))
            add(t, "setup_ms", ms)
            (new, new_key, wit), ms = wall(lambda: fresh.update(key, secret))
            add(t, "update_after_setup_ms", ms)
            del new, new_key, fresh
            loaded, ms = wall(lambda: plk.PlonkParams.load(s["points"], ctx))
            add(t, "srs_load_ms", ms)
            del loaded

    with open(ns.out, "a") as fh:
        for log_n in ns.log_sizes:
            s = sizes[log_n]
            rec = {"tool": "srs_update_bench", "log_n": log_n, "points": s["n"], "rounds": ns.rounds,
                   "warmup": ns.warmup}
            for name, vals in s["t"].items():
                rec[name] = round(statistics.median(vals), 4)
                rec[name + "_min"] = round(min(vals), 4)
                rec[name + "_max"] = round(max(vals), 4)
            rec["mul_kernel_ns_per_point"] = round(rec["mul_kernel_ms"] * 1e6 / s["n"], 2)
            rec["setup_less_load_ms"] = round(rec["setup_ms"] - rec["srs_load_ms"], 4)
            rec["update_less_load_ms"] = round(rec["update_ms"] - rec["srs_load_ms"], 4)
            rec["mul_kernel_over_setup_less_load"] = round(rec["mul_kernel_ms"] / rec["setup_less_load_ms"], 3)
            rec["update_over_setup"] = round(rec["update_ms"] / rec["setup_ms"], 3)
            rec["build_id"] = {k: info[k] for k in ("src", "flags", "variant", "tree_src")}
            line = json.dumps(rec)
            fh.write(line + "\n")
            print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
