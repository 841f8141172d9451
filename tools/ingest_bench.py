#!/usr/bin/env python3
"""ingest_bench.py — time the ingest stage (plk_proofs_ingest, csrc/ingest.hip) on the GPU.

For count = 1, 64, 1 024 and 16 384 compact proofs of the bench circuit at n = 2^12 (--distinct
distinct proofs, cycled, as in tools/verify_each_bench.py) it measures, in one run:

  * the two kernels of plk_proofs_ingest from plk_ingest_last_ms (HIP events around each):
    k_g1_decompress and k_g1_subgroup over 11 count points;
  * plk_proofs_ingest as a whole (wall clock: upload, kernels, download, the host status pass);
  * plk_verifier_verify_each_bytes beside plk_verifier_verify_each on the same, already decoded
    proofs (wall clock);
  * the host loop of plk_proof_decode_compact (subgroup check on), measured in full up to
    --host-cap (256) proofs and EXTRAPOLATED linearly above (`host_decode_extrapolated`: true).

The calls are interleaved round by round, medians over --rounds rounds after --warmup untimed
ones. One JSON line per count is appended to profiles/ingest.jsonl (or --out). Fails without a
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
    ap.add_argument("--log-n", type=int, default=12)
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 64, 1024, 16384])
    ap.add_argument("--distinct", type=int, default=256, help="distinct proofs made up front")
    ap.add_argument("--host-cap", type=int, default=256, help="host decodes measured in full")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ingest.jsonl"))
    ns = ap.parse_args(argv)

    import ctypes as C

    import numpy as np
    import dusk_plonk_amd as plk
    from dusk_plonk_amd.prover import PROOF_COMPACT_BYTES, PlkProof, Plonk, PlonkKey, _bind
    from bench import bench_circuit

    info = plk.check_build()
    if plk.device_count() == 0:
        raise SystemExit("ingest_bench.py: no GPU visible")
    ctx = plk.Context.default(0)
    k, n = ns.log_n, 1 << ns.log_n
    tau = np.array([3, 1, 4, 1], dtype=np.uint64)
    pp = plk.PlonkParams.setup(k, tau, ctx)
    opening = plk.OpeningKey.setup(tau)
    chain = n - 15
    prover, vd = PlonkKey.compile_composer(pp, b"ingest-bench", bench_circuit(Plonk, chain, 1))
    ver = vd.verifier(ctx)
    distinct = min(ns.distinct, max(ns.counts))
    made = [prover.prove_composer(bench_circuit(Plonk, chain, 100 + j), 7 + j) for j in range(distinct)]
    compact = [p.to_compact() for p, _ in made]
    lib = _bind()
    packed = {}
    for b in ns.counts:
        blob = b"".join(compact[j % distinct] for j in range(b))
        raw = (PlkProof * b)(*[made[j % distinct][0].raw for j in range(b)])
        packed[b] = (blob, raw, ver._pis([made[j % distinct][1] for j in range(b)], b))

    def wall(call, what):
        t0 = time.perf_counter()
        st = call()
        ms = (time.perf_counter() - t0) * 1e3
        if st != plk.PLK_OK:
            raise plk.PlonkError(st, what)
        return ms

    def run(b):
        blob, raw, pis = packed[b]
        out = (PlkProof * b)()
        status = np.zeros(b, dtype=np.uint8)
        verdict = np.zeros(b, dtype=np.uint8)
        ingest = wall(lambda: lib.plk_proofs_ingest(ctx.handle, blob, b, 1, out,
                                                    status.ctypes.data_as(C.c_void_p)), "plk_proofs_ingest")
        dec_ms, sub_ms = plk.ingest_last_ms(ctx)
        if status.any() or bytes(out) != bytes(raw):
            raise SystemExit("ingest_bench.py: an honest proof was rejected or decoded differently")
        each_bytes = wall(lambda: lib.plk_verifier_verify_each_bytes(
            ctx.handle, ver._h, opening._h, blob, pis, b, 1, verdict.ctypes.data_as(C.c_void_p)),
            "plk_verifier_verify_each_bytes")
        if not (verdict == 1).all():
            raise SystemExit("ingest_bench.py: an honest proof got no valid verdict")
        each = wall(lambda: lib.plk_verifier_verify_each(ctx.handle, ver._h, opening._h, raw, pis, b,
                                                         verdict.ctypes.data_as(C.c_void_p)),
                    "plk_verifier_verify_each")
        m = min(b, ns.host_cap)
        one = PlkProof()
        t0 = time.perf_counter()
        for j in range(m):
            st = lib.plk_proof_decode_compact(blob[j * PROOF_COMPACT_BYTES: (j + 1) * PROOF_COMPACT_BYTES],
                                              PROOF_COMPACT_BYTES, C.byref(one), 1)
            if st != plk.PLK_OK:
                raise plk.PlonkError(st, "plk_proof_decode_compact")
        host = (time.perf_counter() - t0) * 1e3 * (b / m)
        return dec_ms, sub_ms, ingest, each_bytes, each, host

    times = {b: [] for b in ns.counts}
    for rnd in range(ns.warmup + ns.rounds):
        for b in ns.counts:
            t = run(b)
            if rnd >= ns.warmup:
                times[b].append(t)
    build = {key: info.get(key) for key in ("src", "flags", "variant", "tree_src")}
    names = ("decompress_kernel_ms", "subgroup_kernel_ms", "ingest_ms", "verify_each_bytes_ms",
             "verify_each_ms", "host_decode_ms")
    lines = []
    for b in ns.counts:
        line = {"tool": "ingest_bench", "log_n": k, "count": b, "points": 11 * b,
                "distinct_proofs": distinct, "rounds": ns.rounds, "warmup": ns.warmup,
                "replay": ver.replay}
        for i, name in enumerate(names):
            col = [t[i] for t in times[b]]
            line[name] = round(statistics.median(col), 4)
            line[name + "_min"] = round(min(col), 4)
            line[name + "_max"] = round(max(col), 4)
        line["host_decode_extrapolated"] = b > ns.host_cap
        line["host_decode_measured"] = min(b, ns.host_cap)
        line["ingest_us_per_proof"] = round(line["ingest_ms"] / b * 1e3, 3)
        line["host_decode_over_ingest"] = round(line["host_decode_ms"] / line["ingest_ms"], 2)
        line["build_id"] = build
        lines.append(line)
        print(json.dumps(line), flush=True)
    outp = Path(ns.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    with outp.open("a") as f:
        f.write("".join(json.dumps(ln) + "\n" for ln in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
