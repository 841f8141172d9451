"""Records tests/golden/prover_digests.json: SHA-256 digests of what key compilation and the
prover hand out, for the smallest circuits that reach each branch of csrc/key.hip, csrc/commit.hip
and csrc/prover.hip. tests/test_prover_digests_gpu.py recomputes them and asserts equality.

    python tools/record_prover_digests.py --commit <id of the commit being recorded>

Run on a GPU at the commit whose behaviour is the reference (the parent of a refactor): the file
is never re-recorded to make a test pass. Per case three digests: the proof bytes
(Proof.to_bytes()), the key's 15 commitments (plk_key_info) and plk_debug_block_eval of a fixed
11-coefficient input; some cases carry more (CASES). `--case NAME` prints one case's record as a
JSON line (how the PLK_LAGRANGE_COMMIT=0 case runs: the variable is read at key compile, so that
case is computed in a fresh child process with it set).
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "oracle", ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

GOLDEN = ROOT / "tests" / "golden" / "prover_digests.json"
SEED = 0x5EED


def _chain_with_publics(n, publics, fn=None):
    """`fn`'s gates (or none), `publics` public-input gates, then chain gates up to m = n - 2
    (n - 1 at n = 8, where the composer's own six gates leave room for no less)."""
    def build():
        from dusk_plonk_amd.prover import Plonk
        cs = Plonk()
        if fn:
            fn(cs)
        for i in range(publics):
            cs.append_public(0x1234567 + 97 * i)
        m = max(n - 2, 7)
        assert cs.m() < m, (cs.m(), m)
        cs.synthetic_chain(m - cs.m(), 31 * n + publics)
        assert n // 2 < cs.m() <= n
        return cs
    return build


def _gadgets(cs):
    import test_prover_oracle as T
    T.ranged(0xA7, 8)(cs)
    T.logic(T.A_RND, T.B_RND, 8, False)(cs)
    T.add_point(T.JJ_A, T.JJ_B)(cs)


def _fixed(cs):
    import test_prover_oracle as T
    T.mul_generator(T.JJ_A)(cs)


def _hot_wire():
    """4000 addition gates whose b wire is one witness of value 5: n = 4096, and that wire's 4000
    equal small values crowd one MSM bucket past lagrange_bucket_max."""
    from test_lagrange_commit_gpu import constant_b_circuit
    from test_prover_oracle import build
    return build(constant_b_circuit(4000, 4000, 5))


# name -> (n, composer builder, kind). Kinds: "proof" (the three digests), "hot" (also
# commit_info()), "lagrange_off" (the same in a child process under PLK_LAGRANGE_COMMIT=0),
# "unsatisfied" (the last witness off by one: the status and what diagnose() reports).
CASES = {
    "n8_pi0": (8, _chain_with_publics(8, 0), "proof"),            # six blocks, no closed-form top
    "n16_pi0": (16, _chain_with_publics(16, 0), "proof"),         # four blocks; no PI term
    "n16_pi1": (16, _chain_with_publics(16, 1), "proof"),         # sparse PI
    "n16_pi4": (16, _chain_with_publics(16, 4), "proof"),         # sparse PI, kPiSparse of them
    "n16_pi5": (16, _chain_with_publics(16, 5), "proof"),         # direct PI
    "n32_pi16": (32, _chain_with_publics(32, 16), "proof"),       # direct PI, kPiDirect of them
    "n32_pi17": (32, _chain_with_publics(32, 17), "proof"),       # PI uploaded and transformed
    "n64_range_logic_var": (64, _chain_with_publics(64, 1, _gadgets), "proof"),
    "n1024_fixed": (1024, _chain_with_publics(1024, 1, _fixed), "proof"),
    "n4096_hot_wire": (4096, _hot_wire, "hot"),
    "n16_lagrange_off": (16, _chain_with_publics(16, 1), "lagrange_off"),
    "n16_unsatisfied": (16, _chain_with_publics(16, 1), "unsatisfied"),
}
NOTE = ("Recorded by tools/record_prover_digests.py. A composer starts with six gates, so n = 16 "
        "holds at most ten public-input gates: the kPiDirect boundary (16 and 17 public inputs) "
        "is taken at n = 32, the nearest size that reaches it.")


def sha(data) -> str:
    return hashlib.sha256(bytes(data)).hexdigest()


def block_eval(plk, prover) -> np.ndarray:
    from oracle_lib import random_fr
    coef = random_fr(11, seed=0xB10C)
    lib = plk.plonk._lib()
    blocks = C.c_int()
    out = np.zeros((6 * prover.n, 4), dtype=np.uint64)
    st = lib.plk_debug_block_eval(prover._key, coef.ctypes.data_as(C.c_void_p), coef.shape[0],
                                  out.ctypes.data_as(C.c_void_p), out.shape[0], C.byref(blocks))
    assert st == plk.PLK_OK, st
    return out[: blocks.value * prover.n]


def record_case(plk, name: str) -> dict:
    """One case's record, computed in this process."""
    from dusk_plonk_amd.prover import PlonkKey
    from oracle_lib import random_fr
    import test_prover_oracle as T
    n, build, kind = CASES[name]
    cs = build()
    k = max(0, (T.n_trim(cs.m()) - 8 - 1).bit_length())
    pp = plk.PlonkParams.setup(k, random_fr(1, seed=700 + k)[0])
    prover, vd = PlonkKey.compile_composer(pp, b"digest", cs)
    assert vd.n == n, (name, vd.n)
    rec = {"key": sha(np.ascontiguousarray(vd.comms).tobytes()),
           "block_eval": sha(block_eval(plk, prover).tobytes())}
    lane = prover.lane()
    try:
        if kind == "unsatisfied":
            nw = cs.export()[1].shape[0]
            cs.set_witness(nw - 1, cs[nw - 1] + 1)
            try:
                lane.prove_composer(cs, SEED)
                rec["status"] = plk.PLK_OK
            except plk.PlonkError as e:
                rec["status"] = e.status
            rep = lane.diagnose()
            rec["failing"] = rep.failing
            rec["failures"] = [[f.gate, f.mask, f"{f.residual:#x}"] for f in rep.failures]
            return rec
        proof, pis = lane.prove_composer(cs, SEED)
        rec["proof"] = sha(proof.to_bytes())
        basis, entries = lane.commit_info()
        if kind == "hot":
            rec["commit_basis"], rec["commit_entries"] = basis, entries
        if kind == "lagrange_off":
            rec["commit_basis"] = basis
    finally:
        lane.close()
    return rec


def case_record(plk, name: str) -> dict:
    """record_case, in a child process with PLK_LAGRANGE_COMMIT=0 where the case asks for it."""
    if CASES[name][2] != "lagrange_off":
        return record_case(plk, name)
    env = dict(os.environ, PLK_LAGRANGE_COMMIT="0")
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--case", name], env=env,
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"{name}: child failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", help="id of the commit being recorded (noted in the file)")
    ap.add_argument("--case", help="print this case's record and exit")
    ap.add_argument("--out", default=str(GOLDEN))
    a = ap.parse_args()
    import dusk_plonk_amd as plk
    if plk.device_count() == 0:
        raise SystemExit("no GPU visible")
    if a.case:
        print(json.dumps(record_case(plk, a.case)))
        return 0
    if not a.commit:
        ap.error("--commit is required when recording")
    cases = {name: case_record(plk, name) for name in CASES}
    # every case must have reached the branch it is named for, on the commit being recorded
    hot = cases["n4096_hot_wire"]
    assert hot["commit_basis"] == ["lagrange", "coefficient", "lagrange", "lagrange"], hot
    assert cases["n16_lagrange_off"]["commit_basis"] == ["coefficient"] * 4
    assert cases["n16_unsatisfied"]["status"] == plk.PLK_E_DEGREE
    assert cases["n16_unsatisfied"]["failing"] >= 1
    assert cases["n16_lagrange_off"]["proof"] == cases["n16_pi1"]["proof"]
    doc = {"recorded_at_commit": a.commit, "note": NOTE, "seed": SEED, "cases": cases}
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {a.out}: {len(cases)} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
