#!/usr/bin/env python3
"""verify_each_bench.py — time the per-proof verdicts (plk_verifier_verify_each) on the GPU.

For count = 1, 64, 1 024 and 16 384 proofs of the bench circuit at n = 2^12 (the proofs and their
cycling through --distinct distinct ones as in tools/verify_bench.py) it measures, in one run:

  * plk_verifier_verify_each as a whole (HIP events on the context's stream around the call) and
    its two GPU phases from plk_verifier_last_each_stats: the pairs kernel (k_proof_pairs) and the
    pairing kernel (k_pairing);
  * plk_verifier_fold of the same batch (random weights), and plk_verifier_verify of it;
  * `count` single folds (count = 1, weight 1), the only route to per-proof G1 pairs before
    plk_verifier_pairs existed — measured in full up to --single-cap (256) folds and
    EXTRAPOLATED linearly from those above (`single_folds_extrapolated`: true);
  * the host plk_pairing_check of one pair (wall clock).

The calls are interleaved round by round (every round visits every count), medians over --rounds
rounds after --warmup untimed ones. One JSON line per count to profiles/verify_each.jsonl (or
--out). Fails without a GPU.
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
    ap.add_argument("--log-n", type=int, default=12)
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 64, 1024, 16384])
    ap.add_argument("--distinct", type=int, default=256, help="distinct proofs made up front")
    ap.add_argument("--single-cap", type=int, default=256, help="single folds measured in full")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "verify_each.jsonl"))
    ns = ap.parse_args(argv)

    import ctypes as C

    import numpy as np
    import torch
    import dusk_plonk_amd as plk
    from dusk_plonk_amd.prover import PlkFr, PlkProof, Plonk, PlonkKey, _bind, _fr
    from bench import bench_circuit

    info = plk.check_build()
    if plk.device_count() == 0:
        raise SystemExit("verify_each_bench.py: no GPU visible")
    ctx = plk.Context.default(0)
    k, n = ns.log_n, 1 << ns.log_n
    tau = np.array([3, 1, 4, 1], dtype=np.uint64)
    pp = plk.PlonkParams.setup(k, tau, ctx)
    opening = plk.OpeningKey.setup(tau)
    chain = n - 15
    prover, vd = PlonkKey.compile_composer(pp, b"verify-each-bench", bench_circuit(Plonk, chain, 1))
    ver = vd.verifier(ctx)
    distinct = min(ns.distinct, max(ns.counts))
    made = [prover.prove_composer(bench_circuit(Plonk, chain, 100 + j), 7 + j) for j in range(distinct)]
    stream = torch.cuda.ExternalStream(ctx.stream())
    lib = _bind()
    packed = {}
    for b in ns.counts:
        raw = (PlkProof * b)(*[made[j % distinct][0].raw for j in range(b)])
        packed[b] = (raw, ver._pis([made[j % distinct][1] for j in range(b)], b))
    one = (PlkFr * 1)(_fr(1))
    pair = np.zeros((2, 13), dtype=np.uint64)
    ok_int = C.c_int(0)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        st = call()
        e1.record(stream)
        e1.synchronize()
        if st != plk.PLK_OK:
            raise plk.PlonkError(st, "verify_each_bench")
        return e0.elapsed_time(e1)

    def run(b):
        raw, pis = packed[b]
        ok = np.zeros(b, dtype=np.uint8)
        each = timed(lambda: lib.plk_verifier_verify_each(ctx.handle, ver._h, opening._h, raw, pis, b,
                                                          ok.ctypes.data_as(C.c_void_p)))
        if not ok.all():
            raise SystemExit("verify_each_bench.py: an honest proof was rejected")
        pairs_ms, pairing_ms = ver.last_each_stats()
        fold = timed(lambda: lib.plk_verifier_fold(ctx.handle, ver._h, raw, pis, b, None,
                                                   pair.ctypes.data_as(C.c_void_p)))
        verify = timed(lambda: lib.plk_verifier_verify(ctx.handle, ver._h, opening._h, raw, pis, b, None,
                                                       C.byref(ok_int)))
        if not ok_int.value:
            raise SystemExit("verify_each_bench.py: an honest batch was rejected")
        m = min(b, ns.single_cap)
        npi = len(vd.pi_indexes)
        t0 = time.perf_counter()
        for j in range(m):
            st = lib.plk_verifier_fold(ctx.handle, ver._h, C.byref(raw, j * C.sizeof(PlkProof)),
                                       C.byref(pis, j * npi * C.sizeof(PlkFr)), 1, one,
                                       pair.ctypes.data_as(C.c_void_p))
            if st != plk.PLK_OK:
                raise plk.PlonkError(st, "plk_verifier_fold")
        singles = (time.perf_counter() - t0) * 1e3 * (b / m)
        t0 = time.perf_counter()
        st = lib.plk_pairing_check(opening._h, pair.ctypes.data_as(C.c_void_p), C.byref(ok_int))
        host_check = (time.perf_counter() - t0) * 1e3
        if st != plk.PLK_OK or not ok_int.value:
            raise SystemExit("verify_each_bench.py: the host check rejected an honest pair")
        return each, pairs_ms, pairing_ms, fold, verify, singles, host_check

    times = {b: [] for b in ns.counts}
    for rnd in range(ns.warmup + ns.rounds):
        for b in ns.counts:
            t = run(b)
            if rnd >= ns.warmup:
                times[b].append(t)
    build = {key: info.get(key) for key in ("src", "flags", "variant", "tree_src")}
    names = ("verify_each_ms", "pairs_kernel_ms", "pairing_kernel_ms", "fold_ms", "verify_ms",
             "single_folds_ms", "host_pairing_check_ms")
    lines = []
    for b in ns.counts:
        line = {"tool": "verify_each_bench", "log_n": k, "count": b, "distinct_proofs": distinct,
                "rounds": ns.rounds, "warmup": ns.warmup, "replay": ver.replay}
        for i, name in enumerate(names):
            col = [t[i] for t in times[b]]
            line[name] = round(statistics.median(col), 4)
            line[name + "_min"] = round(min(col), 4)
            line[name + "_max"] = round(max(col), 4)
        line["single_folds_extrapolated"] = b > ns.single_cap
        line["single_folds_measured"] = min(b, ns.single_cap)
        line["verify_each_us_per_proof"] = round(line["verify_each_ms"] / b * 1e3, 3)
        line["single_folds_over_verify_each"] = round(line["single_folds_ms"] / line["verify_each_ms"], 2)
        line["build_id"] = build
        lines.append(line)
        print(json.dumps(line), flush=True)
    outp = Path(ns.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text("".join(json.dumps(ln) + "\n" for ln in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
