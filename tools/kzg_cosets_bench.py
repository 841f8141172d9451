#!/usr/bin/env python3
"""kzg_cosets_bench.py — time the KZG coset openings (csrc/kzg.hip, csrc/g1_colsum.hip).

For n = 2^12 and 2^16 (--log-sizes) and cosets of l = 1, 16 and 64 points (--log-ls 0 4 6) it
measures, in one run on one box:

  * PlonkParams.open_cosets of a dense polynomial of n coefficients on a fresh SRS object: the
    first call's wall clock and table build (plk_kzg_last_open_ms), then warm calls: wall clock and
    the HIP-event split into transforms (with the column sum) and pointwise multiplication;
  * PlonkParams.open_domain at the same n in the same run (first and warm), what open_cosets is
    held against: the same 2n multiplications, transforms of 2n and n points instead of 2r and r;
  * the per-coset route a caller had before: the quotient f div (X^l - y) by long division on the
    host (Python integers), then one commit, over at most --loop-cosets cosets (16; at most 64) and
    extrapolated linearly to all r = n / l cosets. The division and the commit are timed apart,
    since a host library would divide much faster than Python does; both figures are labelled
    extrapolated.

And for 64 and 4 096 openings (--fold-counts) at l = 64 of the largest size (the r cosets of the
domain, repeated when the count exceeds r): OpeningKey.fold_cosets plus one host pairing check on
the key of tau^l, against that many single-opening checks (one fold of one opening plus its host
check timed in the same run, times the count).

Medians over --rounds rounds after --warmup untimed ones. One JSON line per (size, l) and per fold
count is appended to profiles/kzg_cosets.jsonl (or --out). Fails without a GPU.
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

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--log-sizes", type=int, nargs="+", default=[12, 16])
    ap.add_argument("--log-ls", type=int, nargs="+", default=[0, 4, 6])
    ap.add_argument("--fold-counts", type=int, nargs="+", default=[64, 4096])
    ap.add_argument("--fold-log-l", type=int, default=6)
    ap.add_argument("--loop-cosets", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kzg_cosets.jsonl"))
    ns = ap.parse_args(argv)
    if not 1 <= ns.loop_cosets <= 64:
        raise SystemExit("kzg_cosets_bench.py: --loop-cosets in 1 .. 64")

    import numpy as np
    import dusk_plonk_amd as plk

    info = plk.check_build()
    if plk.device_count() == 0:
        raise SystemExit("kzg_cosets_bench.py: no GPU visible")
    ctx = plk.Context.default(0)
    tau_int = 0x1D4F3A7C55E1B2096A8F4C3D2E1B0A99887766554433221100FFEEDDCCBBAA99 % R
    tau = plk.plonk._fr_limbs(tau_int)
    build = {k: info[k] for k in ("src", "flags", "variant", "tree_src")}

    def wall(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def med(vals):
        return round(statistics.median(vals), 4)

    def fr_rows(ints):
        return np.stack([plk.plonk._fr_limbs(v) for v in ints]) if ints else np.zeros((0, 4), dtype=np.uint64)

    def timed_opens(fn):
        """first wall ms, table ms, then the medians of warm wall / transform / multiplication ms"""
        out, first = wall(fn)
        table = plk.kzg_last_open_ms(ctx)[2]
        ws, ts, ms_ = [], [], []
        for rnd in range(ns.warmup + ns.rounds):
            _, ms = wall(fn)
            if rnd >= ns.warmup:
                t = plk.kzg_last_open_ms(ctx)
                ws.append(ms)
                ts.append(t[0])
                ms_.append(t[1])
        return out, round(first, 4), round(table, 4), med(ws), med(ts), med(ms_)

    import random
    prng = random.Random(8349)
    lines = []
    last = None
    for log_n in ns.log_sizes:
        n = 1 << log_n
        f_int = [prng.randrange(R) for _ in range(n)]
        fc = plk.Coefficients(fr_rows(f_int))
        omega = int.from_bytes(plk.Fft(log_n, ctx).elements[1].tobytes(), "little") * pow(1 << 256, -1, R) % R
        pp = plk.PlonkParams.setup(log_n, tau, ctx)
        (dvalues, dwit), d_first, d_table, d_warm, d_tr, d_mul = timed_opens(lambda: pp.open_domain(log_n, fc))
        for log_l in ns.log_ls:
            if log_l > log_n:
                continue
            l, r = 1 << log_l, n >> log_l
            pp = plk.PlonkParams.setup(log_n, tau, ctx)  # a fresh SRS object: the table is built
            (values, wit), first, table, warm, tr, mul = timed_opens(lambda: pp.open_cosets(log_n, log_l, fc))
            if not np.array_equal(values.values, dvalues.values) or (log_l == 0 and not np.array_equal(wit, dwit)):
                raise SystemExit("kzg_cosets_bench.py: open_cosets and open_domain disagree")
            rec = {"tool": "kzg_cosets_bench", "log_n": log_n, "log_l": log_l, "cosets": r,
                   "rounds": ns.rounds, "warmup": ns.warmup,
                   "cosets_first_ms": first, "cosets_table_ms": table, "cosets_warm_ms": warm,
                   "cosets_transform_ms": tr, "cosets_mul_ms": mul,
                   "domain_first_ms": d_first, "domain_table_ms": d_table, "domain_warm_ms": d_warm,
                   "domain_transform_ms": d_tr, "domain_mul_ms": d_mul,
                   "domain_warm_over_cosets_warm": round(d_warm / warm, 3)}
            # the per-coset route: long division on the host, then one commit
            m = min(r, ns.loop_cosets)
            psi = pow(omega, l, R)
            div_ms, com_ms = [], []
            for j in range(m):
                y = pow(psi, j, R)
                t0 = time.perf_counter()
                rem = f_int[:]
                for i in range(n - 1, l - 1, -1):
                    rem[i - l] = (rem[i - l] + rem[i] * y) % R
                q = fr_rows(rem[l:])
                div_ms.append((time.perf_counter() - t0) * 1e3)
                if len(q) == 0:
                    com_ms.append(0.0)
                    continue
                com, ms = wall(lambda: pp.commit(plk.Coefficients(q)))
                com_ms.append(ms)
                if not np.array_equal(com.words, wit[j]):
                    raise SystemExit("kzg_cosets_bench.py: open_cosets and divide-then-commit disagree")
            rec["loop_cosets"] = m
            rec["loop_divide_ms_per_coset"] = round(statistics.median(div_ms), 4)
            rec["loop_commit_ms_per_coset"] = round(statistics.median(com_ms), 4)
            rec["loop_commit_ms_extrapolated"] = round(statistics.median(com_ms) * r, 3)
            rec["loop_ms_extrapolated"] = round((statistics.median(div_ms) + statistics.median(com_ms)) * r, 3)
            rec["loop_commit_extrapolated_over_cosets_warm"] = round(rec["loop_commit_ms_extrapolated"] / warm, 2)
            rec["build_id"] = build
            lines.append(rec)
            if log_l == ns.fold_log_l:
                last = (pp, fc, values, wit, log_n, omega)

    if ns.fold_counts and last is not None:
        pp, fc, values, wit, log_n, omega = last
        log_l = ns.fold_log_l
        l, r = 1 << log_l, (1 << log_n) >> log_l
        key = plk.OpeningKey.setup(pow(tau_int, l, R))
        if not pp.power_key_matches(key, log_l):
            raise SystemExit("kzg_cosets_bench.py: the key of tau^l does not match the SRS")
        com = pp.commit(fc).words
        rows = np.ascontiguousarray(values.cosets(log_l))
        zs = fr_rows([pow(omega, j, R) for j in range(r)])
        one = fr_rows([1])
        singles = []
        for rnd in range(1 + 5):  # the first use untimed
            t0 = time.perf_counter()
            ok = key.check(key.fold_cosets(pp, log_l, com, zs[1], rows[1], wit[1], weights=one))
            if rnd:
                singles.append((time.perf_counter() - t0) * 1e3)
            if not ok:
                raise SystemExit("kzg_cosets_bench.py: a true opening was rejected")
        one_check = statistics.median(singles)
        for count in ns.fold_counts:
            idx = np.arange(count) % r
            cz, cy, cw = zs[idx], np.ascontiguousarray(rows[idx]), wit[idx]
            folds, totals = [], []
            for rnd in range(ns.warmup + ns.rounds):
                pair, ms = wall(lambda: key.fold_cosets(pp, log_l, com, cz, cy, cw))
                t0 = time.perf_counter()
                ok = key.check(pair)
                ms2 = (time.perf_counter() - t0) * 1e3
                if not ok:
                    raise SystemExit("kzg_cosets_bench.py: the fold of true openings was rejected")
                if rnd >= ns.warmup:
                    folds.append(ms)
                    totals.append(ms + ms2)
            lines.append({"tool": "kzg_cosets_bench", "fold_cosets": count, "log_l": log_l, "log_n": log_n,
                          "distinct_cosets": min(count, r), "fold_ms": med(folds),
                          "fold_and_check_ms": med(totals), "single_fold_and_check_ms": round(one_check, 4),
                          "single_checks_ms": round(one_check * count, 3),
                          "single_checks_over_fold_and_check": round(one_check * count / statistics.median(totals), 2),
                          "rounds": ns.rounds, "warmup": ns.warmup, "build_id": build})

    Path(ns.out).parent.mkdir(parents=True, exist_ok=True)
    with open(ns.out, "a") as fh:
        for rec in lines:
            line = json.dumps(rec)
            fh.write(line + "\n")
            print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
