#!/usr/bin/env python3
"""srs_bench.py — time the SRS import and its verification (csrc/srs_io.hip) on the GPU.

For an SRS of 2^16 and of 2^20 points (--log-sizes) it measures, in one run on one box:

  * PlonkParams.from_bytes per format (wall clock: upload, decode, subgroup test, the table build
    of srs_finish), with the decode and subgroup kernel times from plk_srs_last_load_ms (HIP
    events around each). `rest_ms` is the wall time less the two kernels: upload, the infinity
    scan and the MSM table build, which plk_srs_load pays as well;
  * the host route of the same build: the host decoder (plk_proof_decode_compact with the
    subgroup test, 11 points a call) over --host-points points, EXTRAPOLATED linearly to the
    SRS's size (`host_decode_extrapolated`: true), plus PlonkParams.load of the decoded points
    (wall clock: the limb conversion, upload and table build);
  * PlonkParams.verify on the imported SRS (point and subgroup passes already behind it), split
    into the fold and the host pairing check (plk_srs_last_verify_ms), and on an SRS fresh from
    plk_srs_load (every step);
  * PlonkParams.to_bytes (compressed).

The sizes are interleaved round by round; medians over --rounds rounds after --warmup untimed
ones. One JSON line per size is appended to profiles/srs_ingest.jsonl (or --out). Fails without a
GPU.
"""
from __future__ import annotations

import argparse
import ctypes as C
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
    ap.add_argument("--host-points", type=int, default=256, help="points the host decoder is timed on")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "srs_ingest.jsonl"))
    ns = ap.parse_args(argv)

    import numpy as np
    import dusk_plonk_amd as plk

    info = plk.check_build()
    if plk.device_count() == 0:
        raise SystemExit("srs_bench.py: no GPU visible")
    ctx = plk.Context.default(0)
    lib, ptr = plk.plonk._lib(), plk.plonk._ptr
    tau = np.array([3, 1, 4, 1], dtype=np.uint64)
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
        sizes[log_n] = {"n": n, "points": pp.points(), "comp": pp.to_bytes("compressed"),
                        "raw": pp.to_bytes("uncompressed"), "t": {}}
        del pp

    # the host decoder: compact proofs made of 11 SRS points and 16 zero scalars each
    calls = (ns.host_points + 10) // 11
    blob = sizes[ns.log_sizes[0]]["comp"]
    proofs = [np.frombuffer(blob[528 * j:528 * (j + 1)] + bytes(512), dtype=np.uint8) for j in range(calls)]
    out = np.zeros(11 * 104 + 16 * 32, dtype=np.uint8)
    dec = lib.plk_proof_decode_compact
    dec.restype, dec.argtypes = C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
    host_us = []
    for _ in range(ns.warmup + ns.rounds):
        t0 = time.perf_counter()
        for b in proofs:
            if dec(ptr(b), b.size, ptr(out), 1) != plk.PLK_OK:
                raise SystemExit("srs_bench.py: the host decoder refused an SRS point")
        host_us.append((time.perf_counter() - t0) * 1e6 / (11 * calls))
    host_us = statistics.median(host_us[ns.warmup:])

    def add(t, name, v):
        t.setdefault(name, []).append(v)

    for rnd in range(ns.warmup + ns.rounds):
        for log_n in ns.log_sizes:
            s = sizes[log_n]
            t = {} if rnd < ns.warmup else s["t"]
            for fmt, blob in (("compressed", s["comp"]), ("uncompressed", s["raw"])):
                got, ms = wall(lambda: plk.PlonkParams.from_bytes(blob, fmt, True, ctx))
                d, g = plk.plonk.srs_last_load_ms(ctx)
                add(t, f"load_bytes_{fmt}_ms", ms)
                add(t, f"decode_{fmt}_kernel_ms", d)
                add(t, f"subgroup_{fmt}_kernel_ms", g)
                add(t, f"rest_{fmt}_ms", ms - d - g)
                if fmt == "compressed":
                    imported = got
                del got
            loaded, ms = wall(lambda: plk.PlonkParams.load(s["points"], ctx))
            add(t, "srs_load_ms", ms)
            v, ms = wall(lambda: loaded.verify(key))
            f, q = loaded.last_verify_ms()
            if not v.ok:
                raise SystemExit(f"srs_bench.py: verify said {v!r}")
            add(t, "verify_after_load_ms", ms)
            add(t, "verify_after_load_checks_ms", ms - f - q)
            v, ms = wall(lambda: imported.verify(key))
            f, q = imported.last_verify_ms()
            if not v.ok:
                raise SystemExit(f"srs_bench.py: verify said {v!r}")
            add(t, "verify_ms", ms)
            add(t, "verify_fold_ms", f)
            add(t, "verify_pairing_ms", q)
            _, ms = wall(lambda: imported.to_bytes("compressed"))
            add(t, "export_compressed_ms", ms)
            del imported, loaded

    with open(ns.out, "a") as fh:
        for log_n in ns.log_sizes:
            s = sizes[log_n]
            rec = {"tool": "srs_bench", "log_n": log_n, "points": s["n"], "rounds": ns.rounds,
                   "warmup": ns.warmup}
            for name, vals in s["t"].items():
                rec[name] = round(statistics.median(vals), 4)
                rec[name + "_min"] = round(min(vals), 4)
                rec[name + "_max"] = round(max(vals), 4)
            rec["host_decode_us_per_point"] = round(host_us, 3)
            rec["host_decode_measured_points"] = 11 * calls
            rec["host_decode_extrapolated"] = True
            rec["host_decode_ms"] = round(host_us * s["n"] / 1e3, 1)
            rec["host_route_ms"] = round(rec["host_decode_ms"] + rec["srs_load_ms"], 1)
            rec["host_route_over_load_bytes_compressed"] = round(
                rec["host_route_ms"] / rec["load_bytes_compressed_ms"], 2)
            rec["build_id"] = {k: info[k] for k in ("src", "flags", "variant", "tree_src")}
            line = json.dumps(rec)
            fh.write(line + "\n")
            print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
