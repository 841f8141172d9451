"""Structured inputs through the NTT family on the GPU, bit-exact on canonical Montgomery words
against the C oracle and, for the tones, against the closed form.

Uniformly random data (every other transform test) keeps the lazy butterflies of csrc/ntt.hip in
the middle of their ranges: no residue is ever 0, no difference ever exactly k r. These patterns
put exact zeros where the kernel carries them as 0, r or 2r: constants and deltas (one nonzero
output / input), tones x_i = w^(s i) (one nonzero output, n - 1 exact zeros), periodic inputs
(first-stage differences exactly 0), antiperiodic inputs (first-stage sums exactly 0 mod r, the
value r or 2r inside the lazy range; whole sub-transforms zero after the first stage) and ramps.

Sizes: k = 1..9 single-pass plans at every radix (the in-register first stage at 7 and 9),
k = 10..18 two-pass plans 5 + 5 .. 9 + 9 (both LDS strides, the quad-transpose path), k = 19 the
smallest three-pass plan 7 + 6 + 6 (a middle pass with inter-pass twiddles and no post scale);
the pruned first pass at k = 12 and 16 and the folded first pass (plk_debug_block_eval) at
k = 4 and 10. Every output is also asserted canonical (< r) on its own, so that a stray r where 0
belongs is reported as such."""
import ctypes as C
import functools

import numpy as np
import pytest

import pyref as P
from oracle_lib import random_fr

R_LIMBS = np.array(P.int_to_limbs(P.R_MOD, 4), dtype=np.uint64)
TRANSFORMS = ((1, False, "dft"), (-1, False, "idft"), (1, True, "coset_dft"), (-1, True, "coset_idft"))
FAMILIES = ("const", "delta", "tone", "periodic", "antiperiodic", "ramp")
LARGE = ("const", "tone", "antiperiodic")  # k >= 17: tone(1), antiperiodic(1), const(r - 1) only


def enc(vals) -> np.ndarray:
    return P.fr_vec_to_np([v % P.R_MOD for v in vals])


def below_r(a: np.ndarray) -> np.ndarray:
    """Row-wise a < r on 4 x 64-bit words."""
    lt = np.zeros(a.shape[0], dtype=bool)
    eq = np.ones(a.shape[0], dtype=bool)
    for i in (3, 2, 1, 0):
        lt |= eq & (a[:, i] < R_LIMBS[i])
        eq &= a[:, i] == R_LIMBS[i]
    return lt


def neg(a: np.ndarray) -> np.ndarray:
    """Row-wise -a mod r of canonical words (the Montgomery form of -x is r - mont(x))."""
    out = np.zeros_like(a)
    borrow = np.zeros(a.shape[0], dtype=bool)
    for i in range(4):
        out[:, i] = R_LIMBS[i] - a[:, i] - borrow.astype(np.uint64)
        borrow = (a[:, i] > R_LIMBS[i]) | ((a[:, i] == R_LIMBS[i]) & borrow)
    out[~a.any(axis=1)] = 0
    return out


def assert_canonical(a: np.ndarray, what):
    bad = np.flatnonzero(~below_r(a))
    assert bad.size == 0, (f"{what}: {bad.size} outputs are not canonical (>= r); first at index "
                           f"{bad[0]}: {[hex(int(w)) for w in a[bad[0]]]}")


@functools.lru_cache(maxsize=None)
def elements(oracle, k: int) -> np.ndarray:
    """w^i, i < n, with w = pyref.omega(k) (the oracle's table, tied to pyref at i = 1 and n - 1)."""
    el = oracle.elements(k)
    w = P.omega(k)
    assert np.array_equal(el[[0, 1, -1]], enc([1, w, pow(w, (1 << k) - 1, P.R_MOD)]))
    el.setflags(write=False)
    return el


def patterns(oracle, family: str, k: int) -> list:
    """(name, input, (dft closed form, idft closed form) or None) of one family at n = 2^k."""
    n = 1 << k
    one = enc([1])[0]
    out = []
    if family == "const":
        for name, c in (("1", 1), ("r-1", P.R_MOD - 1)):
            if k < 17 or name == "r-1":
                out.append((f"const({name})", np.tile(enc([c]), (n, 1)), None))
    elif family == "delta":
        for j in sorted({0, 1, n // 2, n - 1}):
            x = np.zeros((n, 4), dtype=np.uint64)
            x[j] = one
            out.append((f"delta({j})", x, None))
    elif family == "tone":
        el = elements(oracle, k)
        for s in sorted({1, n // 2, n - 1} if k < 17 else {1}):
            x = el[(s * np.arange(n, dtype=np.int64)) % n]
            dft = np.zeros((n, 4), dtype=np.uint64)
            dft[(n - s) % n] = enc([n])[0]  # sum_i w^(i (s + j)) = n at s + j = 0 mod n
            idft = np.zeros((n, 4), dtype=np.uint64)
            idft[s % n] = one
            out.append((f"tone({s})", x, (dft, idft)))
    elif family in ("periodic", "antiperiodic"):
        for t in (1, 2, 3):
            if k < t or (k >= 17 and t > 1):
                continue
            p = n >> t
            b = random_fr(p, seed=4000 + 10 * k + t)
            blocks = [b if family == "periodic" or m % 2 == 0 else neg(b) for m in range(1 << t)]
            out.append((f"{family}({t})", np.concatenate(blocks), None))
    else:
        out.append(("ramp(i)", enc(range(n)), None))
        out.append(("ramp(r-1-i)", enc(P.R_MOD - 1 - i for i in range(n)), None))
    return out


CASES = [(k, fam) for k in range(1, 17) for fam in FAMILIES] + [(k, fam) for k in (17, 18, 19) for fam in LARGE]


@pytest.mark.gpu
@pytest.mark.parametrize("k,family", CASES)
def test_structured_inputs_vs_oracle(plk, gpu_ctx, oracle, k, family):
    """Every pattern of the family through dft, idft, coset_dft and coset_idft: canonical
    outputs, equal to the oracle's word for word; the tones also equal their closed form."""
    f = plk.Fft(k, gpu_ctx)
    pats = patterns(oracle, family, k)
    assert pats
    for name, x, closed in pats:
        for direction, coset, fn in TRANSFORMS:
            arg = plk.Coefficients(x) if direction > 0 else plk.PointsValue(x)
            got = getattr(f, fn)(arg).values
            assert_canonical(got, (k, name, fn))
            want = oracle.ntt(x, k, direction, coset)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (k, name, fn, f"{bad.size} of {1 << k} outputs differ, first at {bad[0]}")
            if closed is not None and not coset:
                assert np.array_equal(got, closed[0] if direction > 0 else closed[1]), (k, name, fn, "closed form")


def test_neg_and_below_r_helpers():
    """The test's own word arithmetic against Python integers (no GPU)."""
    vals = [0, 1, 2, P.R_MOD - 1, P.R_MOD - 2, 1 << 64, (1 << 128) - 1, (1 << 192), P.R_MOD >> 1]
    a = P.fr_vec_to_np(vals, mont=False)
    assert P.fr_vec_from_np(neg(a), mont=False) == [(-v) % P.R_MOD for v in vals]
    edge = P.fr_vec_to_np([P.R_MOD - 1, P.R_MOD, P.R_MOD + 1, 0, (1 << 256) - 1], mont=False)
    assert below_r(edge).tolist() == [True, False, False, True, False]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["const(1)", "const(r-1)", "tone(1)", "ramp(i)", "ramp(r-1-i)"])
@pytest.mark.parametrize("k", [12, 16])
def test_structured_pruned_first_pass(plk, gpu_ctx, oracle, k, name):
    """Zero-padded inputs of at most n/8 + n/R coefficients take the closed-form first stages
    (ntt.hip PRUNE; R = 2^6 at k = 12, 2^8 at k = 16): lengths 1, n/8, n/8 + 1 and n/8 + n/R."""
    n = 1 << k
    fam = name.split("(")[0]
    x = next(x for nm, x, _ in patterns(oracle, fam, k) if nm == name)
    f = plk.Fft(k, gpu_ctx)
    lr = (k + 1) // 2  # the first of two passes (plan_domain)
    for m in (1, n // 8, n // 8 + 1, n // 8 + (n >> lr)):
        xm = x[:m]
        for coset, fn in ((False, "dft"), (True, "coset_dft")):
            got = getattr(f, fn)(plk.Coefficients(xm)).values
            assert_canonical(got, (k, name, m, fn))
            assert np.array_equal(got, oracle.ntt(xm, k, 1, coset)), (k, name, m, fn)


@pytest.fixture(scope="module")
def chain_keys(plk):
    """One compiled key per size for the block evaluations (tests/test_quotient_domain_gpu.py)."""
    from dusk_plonk_amd.prover import PlonkKey
    from test_quotient_domain_gpu import bench_like, params_for, tau_for
    keys = {}
    for k in (4, 10):
        tau_limbs, _ = tau_for(0xE0 + k)
        cs = bench_like(k, 5)
        pp, _ = params_for(plk, cs.m(), tau_limbs)
        keys[k] = PlonkKey.compile_composer(pp, b"blocks", cs)[0]
    return keys


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [1, 8])
@pytest.mark.parametrize("name", ["const(r-1)", "tone(1)"])
@pytest.mark.parametrize("k", [4, 10])
def test_structured_folded_first_pass(plk, oracle, chain_keys, k, name, extra):
    """Coefficient vectors of length n + 1 and n + 8 through plk_debug_block_eval: the first pass
    folds the coefficients past n onto the first rows (ntt.hip PRE = 2). Block m, row u is point
    8u + m of the oracle's coset_dft over g H_8n."""
    n = 1 << k
    if name == "tone(1)":
        coef = elements(oracle, k)[np.arange(n + extra) % n]
    else:
        coef = np.tile(enc([P.R_MOD - 1]), (n + extra, 1))
    coef = np.ascontiguousarray(coef)
    lib = plk.plonk._lib()
    blocks = C.c_int()
    out = np.zeros((5 * n, 4), dtype=np.uint64)
    st = lib.plk_debug_block_eval(chain_keys[k]._key, coef.ctypes.data_as(C.c_void_p),
                                  coef.shape[0], out.ctypes.data_as(C.c_void_p), out.shape[0],
                                  C.byref(blocks))
    assert st == plk.PLK_OK and blocks.value == 5
    assert_canonical(out, (k, name, extra))
    ref = oracle.coset_dft(coef, k + 3)
    for m in range(5):
        assert np.array_equal(out[m * n:(m + 1) * n], ref[m::8]), f"block {m}"
