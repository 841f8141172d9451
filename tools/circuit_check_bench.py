#!/usr/bin/env python3
"""circuit_check_bench.py — time the circuit check (csrc/circuit_check.hip) on the GPU.

On the bench chain at n = 2^16 and 2^20 (--log-n), satisfied and with one bad gate, it measures in
one process, shapes warmed up:

  * plk_composer_check on the device: wall clock (upload, kernel, readback) and the kernel alone
    (plk_check_last_ms, HIP events around k_gate_check);
  * the host mirror (plk_composer_check with a NULL context);
  * create_proof: the good proof, and the failing one (PLK_E_DEGREE), the only route to the verdict
    without the check;
  * diagnose() after each of them: wall clock and kernel;
  * the key: plk_key_compile's wall clock and the device memory it takes (hipMemGetInfo before and
    after). --key-only measures just these two, and so also runs on a library from before the check
    (PLK_LIB=... PLK_LIB_ANY_SRC=1) for the comparison of the gate table's cost.

Medians over --rounds rounds after --warmup untimed ones, calls interleaved round by round. One
JSON line per size and witness is appended to profiles/circuit_check.jsonl (or --out). Fails
without a GPU.
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
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--key-rounds", type=int, default=3, help="key compiles timed per size")
    ap.add_argument("--key-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "circuit_check.jsonl"))
    ns = ap.parse_args(argv)

    import ctypes as C

    import numpy as np
    import torch
    import dusk_plonk_amd as plk
    from dusk_plonk_amd.prover import Plonk, PlonkKey, _bind
    from bench import bench_circuit

    info = plk.check_build()
    if plk.device_count() == 0:
        raise SystemExit("circuit_check_bench.py: no GPU visible")
    ctx = plk.Context.default(0)
    build = {key: info.get(key) for key in ("src", "flags", "variant", "tree_src")}
    tau = np.array([3, 1, 4, 1], dtype=np.uint64)

    def wall(call):
        t0 = time.perf_counter()
        out = call()
        return (time.perf_counter() - t0) * 1e3, out

    def med(col):
        return {"": round(statistics.median(col), 4), "_min": round(min(col), 4), "_max": round(max(col), 4)}

    lines = []
    for k in ns.log_n:
        n, chain = 1 << k, (1 << k) - 15
        pp = plk.PlonkParams.setup(k, tau, ctx)
        good = bench_circuit(Plonk, chain, 1)
        m = good.m()
        # the key: compile time and device memory, a fresh key each time (the last one is kept)
        compile_ms, key_bytes, prover = [], [], None
        for _ in range(1 + ns.key_rounds):
            prover = None
            ctx.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            ms, (prover, _) = wall(lambda: PlonkKey.compile_composer(pp, b"check-bench", good))
            ctx.synchronize()
            compile_ms.append(ms)
            key_bytes.append(free0 - torch.cuda.mem_get_info()[0])
        key = {"tool": "circuit_check_bench", "what": "key", "log_n": k, "gates": m,
               "key_compile_ms": round(statistics.median(compile_ms[1:]), 3),
               "key_compile_ms_all": [round(x, 3) for x in compile_ms],
               "key_device_bytes": int(statistics.median(key_bytes)),
               "key_device_bytes_all": [int(x) for x in key_bytes], "build_id": build}
        lines.append(key)
        print(json.dumps(key), flush=True)
        if ns.key_only:
            continue
        # one bad gate: the last chain gate's output feeds no other gate
        bad = bench_circuit(Plonk, chain, 1)
        size = C.c_size_t()
        _bind().plk_composer_size(bad._h, None, C.byref(size))
        nw = size.value
        bad.set_witness(nw - 2, bad[nw - 2] + 1)
        for label, cs in (("satisfied", good), ("one_bad_gate", bad)):
            want_fail = 0 if cs is good else 1
            t = {name: [] for name in ("device_check_ms", "device_check_kernel_ms", "host_check_ms",
                                       "create_proof_ms", "diagnose_ms", "diagnose_kernel_ms")}
            for rnd in range(ns.warmup + ns.rounds):
                dev_ms, rep = wall(lambda: cs.check(ctx))
                dev_k = plk.check_last_ms(ctx)
                host_ms, hrep = wall(lambda: cs.check(host=True))
                if rep.failing != want_fail or not rep == hrep:
                    raise SystemExit(f"circuit_check_bench.py: {label}: device {rep.failing} host "
                                     f"{hrep.failing} failing gates, expected {want_fail}")

                def prove():
                    try:
                        prover.prove_composer(cs, 7)
                        return True
                    except plk.PlonkError as e:
                        if e.status != plk.PLK_E_DEGREE:
                            raise
                        return False
                prove_ms, proved = wall(prove)
                diag_ms, drep = wall(prover.diagnose)
                diag_k = plk.check_last_ms(ctx)
                if proved != (want_fail == 0) or not drep == rep:
                    raise SystemExit(f"circuit_check_bench.py: {label}: proof {proved}, diagnosis "
                                     f"{drep.failing} failing gates")
                if rnd >= ns.warmup:
                    for name, v in zip(t, (dev_ms, dev_k, host_ms, prove_ms, diag_ms, diag_k)):
                        t[name].append(v)
            line = {"tool": "circuit_check_bench", "what": "check", "log_n": k, "gates": m,
                    "witnesses": nw, "witness": label, "failing": want_fail,
                    "proof_succeeds": want_fail == 0, "rounds": ns.rounds, "warmup": ns.warmup,
                    "upload_bytes": 32 * nw + 24 * m}
            for name, col in t.items():
                for suffix, v in med(col).items():
                    line[name + suffix] = v
            line["host_over_device"] = round(line["host_check_ms"] / line["device_check_ms"], 2)
            line["create_proof_over_diagnose"] = round(line["create_proof_ms"] / line["diagnose_ms"], 1)
            line["build_id"] = build
            lines.append(line)
            print(json.dumps(line), flush=True)
        prover = None
    outp = Path(ns.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    with outp.open("a") as f:
        f.write("".join(json.dumps(ln) + "\n" for ln in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
