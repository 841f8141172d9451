#!/usr/bin/env python3
"""msm_naf_record.py — what the MSM's row table (PLK_MSM_NAF = 1) costs and saves beside the
window table, recorded for profiles/ (DESIGN §7).

  python tools/msm_naf_record.py isa  [--out profiles/msm_naf_walk_isa.json]
      no GPU: the compiled k_chist_naf, k_cscatter_naf and k_chist<20> / k_cscatter<20> (the
      window layout's pair) as instruction counts per straight-line block, from libplk.so's
      gfx950 code object (tools/isa_count.py), with the kernels' register and LDS use from the
      build's resource report.

  python tools/msm_naf_record.py gpu [--log-n 20] [--out profiles/msm_naf_setup.jsonl]
      one child process per layout (PLK_MSM_NAF = 0, 1), alternated --reps times on one GPU:
      SRS setup wall time and table bytes, key compile wall time (first and second in the
      process) and the device memory the key takes (free memory before minus after), and one
      commit of 2^log_n random scalars: entries (point additions) and k_accumulate's time.
      One JSON line per child with the build id. Stops at the first child that fails.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def isa(ns) -> int:
    import tempfile

    import isa_count

    lib = ROOT / "dusk-plonk_amd" / "libplk.so"
    pats = {"k_chist_naf": "k_chist_naf", "k_cscatter_naf": "k_cscatter_naf",
            "k_chist<20>": "k_chistILj20E", "k_cscatter<20>": "k_cscatterILj20E"}
    out = {"kernels": {}}
    with tempfile.TemporaryDirectory() as d:
        lines = [ln for co in isa_count._code_objects(lib, Path(d)) for ln in isa_count._disasm(co)]
    for name, pat in pats.items():
        blocks = isa_count.kernel_blocks(lines, pat)
        out["kernels"][name] = {
            "instructions": sum(sum(c.values()) for _, c in blocks),
            "valu": sum(v for _, c in blocks for k, v in c.items() if k.startswith("v_")),
            "blocks": [{"offset": off, "instructions": sum(c.values()),
                        "valu_issue_cycles": round(isa_count.valu_cycles(c), 1)}
                       for off, c in blocks if sum(c.values()) >= 8]}
    res = (ROOT / "dusk-plonk_amd" / "build" / "msm_sort.res.txt")
    if res.exists():
        cur = None
        for line in res.read_text().splitlines():
            m = re.search(r"remark: +([^:]+): (.*?) \[-Rpass", line)
            if not m:
                continue
            k, v = m.group(1).strip(), m.group(2).strip()
            if k == "Function Name":
                cur = next((n for n, p in pats.items() if p in v), None)
            elif cur and k in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
                               "LDS Size [bytes/block]"):
                out["kernels"][cur][k] = int(v)
    Path(ns.out).write_text(json.dumps(out, indent=1) + "\n")
    for name, d in out["kernels"].items():
        print(name, d["instructions"], "instructions,", d["valu"], "VALU")
    return 0


def child(ns) -> int:
    import numpy as np
    import torch

    import dusk_plonk_amd as plk
    from dusk_plonk_amd.prover import PlonkKey

    class Chain:
        def __init__(self, gates, seed):
            self.gates, self.seed = gates, seed

        def synthesize(self, cs):
            cs.synthetic_chain(self.gates, self.seed)

    info = plk.check_build()
    ctx = plk.Context.default(0)
    k, n = ns.log_n, 1 << ns.log_n
    tau = np.array([3, 1, 4, 1], dtype=np.uint64)
    rec = {"tag": ns.tag, "log_n": k, "naf_env": os.environ.get("PLK_MSM_NAF"), "build": info}

    def wall(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        return out, time.perf_counter() - t0

    pp, rec["srs_setup_s"] = wall(lambda: plk.PlonkParams.setup(k, tau, ctx))
    rec.update(pp.table_layout())
    gates = n - 8 - 6
    keep = []
    for i in range(2):
        free0 = torch.cuda.mem_get_info()[0]
        pv, rec[f"compile_s_{i}"] = wall(lambda: PlonkKey.compile_with_circuit(pp, b"chain", Chain(gates, 1)))
        rec[f"key_bytes_{i}"] = free0 - torch.cuda.mem_get_info()[0]
        keep.append(pv)
    rng = np.random.default_rng(7)
    sc = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)  # below r: top limb < 2^62
    dev = torch.from_numpy(sc.view(np.int64)).cuda()
    torch.cuda.synchronize()
    for _ in range(3):
        pp.commit_batch_dev([(dev.data_ptr(), n)])
    ms, adds, c = pp.last_msm_stats()
    rec.update(commit_entries=adds, entries_per_scalar=adds / n, accumulate_ms=ms, window_bits=c)
    print(json.dumps(rec), flush=True)
    return 0


def gpu(ns) -> int:
    out = Path(ns.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for rep in range(ns.reps):
        for tag, naf in (("windows", "0"), ("rows", "1")):
            cmd = [sys.executable, __file__, "child", "--log-n", str(ns.log_n), "--tag", tag]
            r = subprocess.run(["timeout", "-k", "10", str(ns.timeout), *cmd], cwd=ROOT,
                               env={**os.environ, "PLK_MSM_NAF": naf}, capture_output=True, text=True)
            if r.returncode != 0:
                print(f"[msm-naf] {tag}: rc {r.returncode}\n{r.stderr[-3000:]}", flush=True)
                return 1
            line = r.stdout.strip().splitlines()[-1]
            json.loads(line)
            print(line, flush=True)
            with open(out, "a") as f:
                f.write(line + "\n")
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("what", choices=["isa", "gpu", "child"])
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    ns = ap.parse_args(argv)
    if not ns.out:
        ns.out = str(ROOT / "profiles" / ("msm_naf_walk_isa.json" if ns.what == "isa" else "msm_naf_setup.jsonl"))
    return {"isa": isa, "gpu": gpu, "child": child}[ns.what](ns)


if __name__ == "__main__":
    sys.exit(main())
