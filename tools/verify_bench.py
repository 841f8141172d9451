#!/usr/bin/env python3
"""verify_bench.py — time the batched verifier (plk_verifier_fold) on the GPU.

Folds B = 1, 64, 1 024 and 16 384 proofs of the bench circuit at n = 2^12 (bench.py's
bench_circuit: a chain of gates and one public input) into the final KZG pair. The proofs are
made once, outside the timed region: --distinct of them (default 256, each with its own
witness, public input and blinding) and a batch of B cycles through them, so a large batch
costs no minutes of proving; every position still replays its transcript and contributes its
own points and weighted scalars.

Timing: HIP events on the context's stream around each fold (the call returns when the pair is
on the host), the batch sizes interleaved round by round (B = 1, 64, ..., then again) so that
drift of the box hits every size alike; medians over --rounds rounds after --warmup untimed
ones. The library's own split is reported beside it: host milliseconds of the transcript
replays, and milliseconds of the GPU phase (upload, scalar kernels, the variable-base MSM and
its host tail). Comparison points printed with every line: the reference's published 7.643 ms
per single verification (its README, an Apple M1 figure — not this host) and the prover's own
proofs/s at this size from README.md (9.6 M constraints/s at 2^12).

--replay host device (the default: both) folds every batch with the transcripts replayed on
the host threads and on the GPU (plk_verifier_set_replay), the two modes one after the other
for each batch size within every round: the host mode of the same run is the yardstick of the
device mode.

Writes one JSON line per batch size and mode to profiles/verify_fold_replay.jsonl (or --out),
each with `replay`, `replay_ms` (host milliseconds before / between the GPU work), `gpu_ms`,
`replay_kernel_ms` (the device replay's kernels, HIP events) and the build id.
profiles/verify_fold.jsonl is the record of the host replay from before the device mode
existed. Fails without a GPU.
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

REFERENCE_VERIFY_MS = 7.643          # /root/reference README "Verification" (Apple M1)
PROVER_CONSTRAINTS_PER_S_2_12 = 9.6e6  # README.md, final size sweep at 2^12


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--log-n", type=int, default=12)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024, 16384])
    ap.add_argument("--distinct", type=int, default=256, help="distinct proofs made up front")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--replay", nargs="+", choices=["host", "device"], default=["host", "device"])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "verify_fold_replay.jsonl"))
    ns = ap.parse_args(argv)

    import torch
    import dusk_plonk_amd as plk
    from dusk_plonk_amd.prover import Plonk, PlonkKey
    from bench import bench_circuit

    info = plk.check_build()
    if plk.device_count() == 0:
        raise SystemExit("verify_bench.py: no GPU visible")
    ctx = plk.Context.default(0)
    k, n = ns.log_n, 1 << ns.log_n
    import numpy as np
    tau = np.array([3, 1, 4, 1], dtype=np.uint64)
    pp = plk.PlonkParams.setup(k, tau, ctx)
    chain = n - 15
    prover, vd = PlonkKey.compile_composer(pp, b"verify-bench", bench_circuit(Plonk, chain, 1))
    ver = vd.verifier(ctx)
    t0 = time.perf_counter()
    distinct = min(ns.distinct, max(ns.batches))
    made = [prover.prove_composer(bench_circuit(Plonk, chain, 100 + j), 7 + j) for j in range(distinct)]
    prove_s = time.perf_counter() - t0
    stream = torch.cuda.ExternalStream(ctx.stream())

    def fold(b):
        proofs = [made[j % distinct][0] for j in range(b)]
        pis = [made[j % distinct][1] for j in range(b)]
        return proofs, pis

    batches = {b: fold(b) for b in ns.batches}
    # marshalling the Python lists into C arrays is not the verifier's time: do it once
    import ctypes as C
    from dusk_plonk_amd.prover import PlkProof, _bind
    lib = _bind()
    packed = {}
    for b, (proofs, pis) in batches.items():
        raw = (PlkProof * b)(*[p.raw for p in proofs])
        packed[b] = (raw, ver._pis(pis, b))
    out = np.zeros((2, 13), dtype=np.uint64)

    def run(b, mode):
        raw, pis = packed[b]
        ver.set_replay(mode)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        st = lib.plk_verifier_fold(ctx.handle, ver._h, raw, pis, b, None, out.ctypes.data_as(C.c_void_p))
        e1.record(stream)
        e1.synchronize()
        if st != plk.PLK_OK:
            raise plk.PlonkError(st, "plk_verifier_fold")
        return (e0.elapsed_time(e1),) + ver.last_fold_stats() + (ver.last_replay_ms(),)

    cases = [(b, mode) for b in ns.batches for mode in ns.replay]
    times = {c: [] for c in cases}
    for rnd in range(ns.warmup + ns.rounds):
        for c in cases:  # interleaved: every round visits every batch size in every mode
            t = run(*c)
            if rnd >= ns.warmup:
                times[c].append(t)
    build = {key: info.get(key) for key in ("src", "flags", "variant", "tree_src")}
    lines = []
    for b, mode in cases:
        tot = [t[0] for t in times[b, mode]]
        med = statistics.median(tot)
        col = lambda i: round(statistics.median(t[i] for t in times[b, mode]), 4)
        line = {
            "tool": "verify_bench", "log_n": k, "batch": b, "replay": mode, "distinct_proofs": distinct,
            "rounds": ns.rounds, "warmup": ns.warmup, "weights": "random (NULL)",
            "fold_ms_median": round(med, 4), "fold_ms_min": round(min(tot), 4),
            "fold_ms_max": round(max(tot), 4),
            "replay_ms": col(1), "gpu_ms": col(2), "replay_kernel_ms": col(3),
            "replay_kernel_us_per_proof": round(col(3) / b * 1e3, 4),
            "ms_per_proof": round(med / b, 6), "proofs_per_s": round(b / med * 1e3, 1),
            "reference_verify_ms_published_m1": REFERENCE_VERIFY_MS,
            "prover_proofs_per_s_readme": round(PROVER_CONSTRAINTS_PER_S_2_12 / n, 1),
            "proving_the_distinct_proofs_s": round(prove_s, 2),
            "build_id": build,
        }
        lines.append(line)
        print(json.dumps(line), flush=True)
    outp = Path(ns.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text("".join(json.dumps(ln) + "\n" for ln in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
