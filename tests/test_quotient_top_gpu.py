"""Round 3 on four cosets with the top seven coefficients of t in closed form (csrc/prover.hpp,
csrc/quotient_top.hpp), on the GPU:

* t itself. A lane proves a satisfied circuit built by the composer and plk_debug_prover_round3
  hands back the polynomials of that round (selectors, sigmas, blinded wires, z, the challenges)
  and the t the prover committed. The reference (tests/quotient_top_ref.py) forms the whole
  numerator N from them in Python integers and divides by Z_H: EVERY one of the 4n + 8
  coefficients is compared (t[4n + 7] = 0 included; the Kronecker product keeps n = 1024 at about
  a second, so nothing is sampled). Sizes n = 16 (smallest on this path), 64, 1024 (four
  workgroups of the combine). Widget kinds per size: arithmetic + public inputs, range, logic and
  variable-base at 16 and 64; fixed-base needs the 269 gates of component_mul_generator and the
  composer has no raw fixed-base gate, so it runs at n = 1024 only, alone and with every other
  widget in one circuit.
* stage "coset_combine_top" alone: four residues t mod (X^n - c_m) of a random t of degree 4n + 6
  and its top seven coefficients give back t, at n = 8 + (ragged) sizes around the workgroup.
* refusal. A witness that breaks one arithmetic gate, the public input only, or the last row
  (n = 16, 64), one range term and one logic term (n = 64): PLK_E_DEGREE from the self-check at
  zeta, and the next proof on the same lane succeeds. (A witness that breaks a copy constraint
  while every gate holds cannot be written through the composer: all wires are gathered from one
  witness vector by the key's indices, so copies agree by construction.)"""
from __future__ import annotations

import random

import numpy as np
import pytest

import circuit_check_ref as M
import prover_stage_ref as S
import quotient_top_ref as Q
import test_prover_oracle as T
from oracle_lib import random_fr

pytestmark = pytest.mark.gpu
r = S.r
NAMES = ("alpha", "beta", "gamma", "range_sep", "logic_sep", "fixed_sep", "var_sep")
_PP = {}


def params(plk, m):
    k = max(0, (T.n_trim(m) - 8 - 1).bit_length())
    if k not in _PP:
        _PP[k] = plk.PlonkParams.setup(k, random_fr(1, seed=700 + k)[0])
    return _PP[k]


def padded(fn, n, seed, public=True, fill=None):
    """The circuit `fn` (or none), one public input, then chain gates up to m = fill (default
    n - 2) gates: n / 2 < m <= n."""
    from dusk_plonk_amd.prover import Plonk
    cs = Plonk()
    if fn:
        fn(cs)
    if public:
        cs.append_public(0x1234567 + seed)
    m = n - 2 if fill is None else fill
    assert cs.m() < m, (cs.m(), m)
    cs.synthetic_chain(m - cs.m(), seed)
    assert cs.m() == m and n // 2 < m <= n
    return cs


def everything(cs):
    T.readme_circuit(20, 5, 25, 100, 2)(cs)
    T.logic(T.A_RND, T.B_RND, 64, True)(cs)
    T.add_point(T.JJ_A, T.JJ_B)(cs)


KINDS = {
    "arith": (None, 0), "range8": (T.ranged(0xA7, 8), 1), "range76": (T.ranged(2**64 - 1, 76), 1),
    "logic8": (T.logic(T.A_RND, T.B_RND, 8, False), 2), "logic64": (T.logic(T.A_RND, T.B_RND, 64, True), 2),
    "var": (T.add_point(T.JJ_A, T.JJ_B), 8), "fixed": (T.mul_generator(T.JJ_A), 4),
    "all": (everything, 15),
}
T_CASES = [(16, "arith"), (16, "range8"), (16, "logic8"), (16, "var"),
           (64, "arith"), (64, "range76"), (64, "logic64"), (64, "var"),
           (1024, "arith"), (1024, "fixed"), (1024, "all")]


def ints(words):
    return [S.unword(w) for w in S.from_np(np.ascontiguousarray(words))]


@pytest.mark.parametrize("n,kind", T_CASES, ids=[f"{n}-{k}" for n, k in T_CASES])
def test_t_equals_numerator_over_zh(plk, gpu_ctx, n, kind):
    from dusk_plonk_amd.prover import PlonkKey
    fn, want_flags = KINDS[kind]
    cs = padded(fn, n, 31 * n + len(kind))
    prover, vd = PlonkKey.compile_composer(params(plk, cs.m()), b"top", cs)
    assert vd.n == n
    lane = prover.lane()
    try:
        lane.prove_composer(cs, 5)
        d = lane.round3()
    finally:
        lane.close()
    sel = [ints(row) for row in d["sel"]]
    flags = sum(bit for bit, q in ((1, S.QRANGE), (2, S.QLOGIC), (4, S.QFIXED), (8, S.QVAR)) if any(sel[q]))
    assert flags == want_flags
    omega = S.unword(S.from_np(plk.Fft(n.bit_length() - 1, gpu_ctx).elements[1:2])[0])
    vals, idx = cs.public_inputs()
    num = Q.numerator(n, omega, [ints(w) for w in d["wires"]], ints(d["z"]), sel,
                      [ints(s) for s in d["sigma"]], list(zip(idx, vals)), dict(zip(NAMES, ints(d["ch"]))),
                      flags, mul=Q.mul_kronecker)
    want, exact = Q.divide_by_zh(num, n)
    assert exact, "the reference's own numerator is not a multiple of Z_H"
    got = ints(d["t"])
    assert len(got) == 4 * n + 8 and len(want) == 4 * n + 7
    assert any(want[4 * n:]), "blinded wires: the closed-form coefficients are not all zero"
    bad = [k for k in range(4 * n + 7) if got[k] != want[k]]
    assert not bad, (len(bad), bad[:8])
    assert got[4 * n + 7] == 0


def inverse_vandermonde(cm):
    """Row l, column m: the coefficient of Y^l in prod_{j != m} (Y - c_j) / (c_m - c_j)."""
    B = len(cm)
    mat = [[0] * B for _ in range(B)]
    for m in range(B):
        poly, den = [1], 1
        for j in range(B):
            if j != m:
                poly = Q.mul_schoolbook(poly, [(-cm[j]) % r, 1])
                den = den * (cm[m] - cm[j]) % r
        for l in range(B):
            mat[l][m] = poly[l] * pow(den, -1, r) % r
    return mat


@pytest.mark.parametrize("n", (8, 16, 255, 257, 1024))
def test_coset_combine_top_gives_back_t(gpu_ctx, n):
    rng = random.Random(n)
    for trial in range(2):
        t = S.draw(rng, 4 * n + 7, edge_share=1.0 if trial else 0.5)
        if trial:
            t[4 * n:] = [r - 1] * 7
        cm = [rng.randrange(2, r) for _ in range(4)]
        blocks = []
        for c in cm:  # t mod (X^n - c): chunk l folds in with c^l
            blocks += [sum(pow(c, l, r) * t[l * n + k] for l in range(5) if l * n + k < len(t)) % r
                       for k in range(n)]
        p = [1]
        for c in cm:
            p = Q.mul_schoolbook(p, [(-c) % r, 1])
        mat = inverse_vandermonde(cm)
        sc = np.concatenate([S.words_np([x for row in mat for x in row], -1), S.words_np(t[4 * n:] + p)])
        got = gpu_ctx.prover_stage("coset_combine_top", [S.words_np(blocks)], sc, [], 4 * n + 8)
        assert np.array_equal(got, S.words_np(t + [0])), (n, trial)


def test_coset_combine_top_refuses_bad_shapes(plk, gpu_ctx):
    for n, n_sc, cap in ((7, 28, 36), (16, 27, 72), (16, 28, 71)):
        with pytest.raises(plk.PlonkError) as e:
            gpu_ctx.prover_stage("coset_combine_top", [S.words_np([1] * (4 * n))], S.words_np([1] * n_sc),
                                 [], cap)
        assert e.value.status == plk.PLK_E_ARG


# ---- refusal ------------------------------------------------------------------------------
def pure_class_witness(cs, cls):
    """The first witness whose increment makes gates fail in class `cls` (index into
    M.CLASS_MASK) and in no other class, by the Python model of the circuit check."""
    nw = cs.export()[1].shape[0]
    for w in range(2, nw):
        with M.tampered(cs, w):
            failing, by_class, _ = M.summarize(M.check(cs))
        if failing and by_class[cls] and sum(by_class) == by_class[cls]:
            return w
    raise AssertionError("no witness breaks only that class")


def refusal_cases(n):
    """(name, composer, witness to tamper, what the model must report for the tampered circuit)."""
    out = []
    cs = padded(None, n, 3 * n)  # the public input is gate 6, chain gates follow
    nw = cs.export()[1].shape[0]
    out.append(("arith_gate", cs, nw - 1, lambda f: len(f) == 1 and f[0][1] == 1))
    vals, idx = cs.public_inputs()
    w_pub = T_wire(cs, idx[0], 0)
    out.append(("public_input", padded(None, n, 3 * n), w_pub, lambda f, g=idx[0]: [x[0] for x in f] == [g]))
    full = padded(None, n, 5 * n, fill=n)  # m = n: the last gate is row n - 1
    out.append(("last_row", full, full.export()[1].shape[0] - 1, lambda f: [x[0] for x in f] == [n - 1]))
    if n == 64:
        rg = padded(T.ranged(2**64 - 1, 76), n, 7 * n)
        out.append(("range_term", rg, pure_class_witness(rg, 1), lambda f: all(x[1] & 0xF0 for x in f)))
        lg = padded(T.logic(T.A_RND, T.B_RND, 64, True), n, 9 * n)
        out.append(("logic_term", lg, pure_class_witness(lg, 2), lambda f: all(x[1] & 0x1F00 for x in f)))
    return out


def T_wire(cs, gate, col):
    g = cs.export()[0][gate]
    return (int(g[44 + col // 2]) >> (32 * (col % 2))) & 0xFFFFFFFF


@pytest.mark.parametrize("n", (16, 64))
def test_unsatisfied_circuit_is_refused_and_the_lane_recovers(plk, n):
    from dusk_plonk_amd.prover import PlonkKey
    for name, cs, w, expect in refusal_cases(n):
        prover, vd = PlonkKey.compile_composer(params(plk, cs.m()), b"refuse", cs)
        assert vd.n == n, name
        lane = prover.lane()
        try:
            good, _ = lane.prove_composer(cs, 11)
            with M.tampered(cs, w):
                fails = M.summarize(M.check(cs))[2]
                assert fails and expect(fails), (name, fails)
                with pytest.raises(plk.PlonkError) as e:
                    lane.prove_composer(cs, 11)
                assert e.value.status == plk.PLK_E_DEGREE, name
                assert not lane.diagnose().ok, name  # the refused witness is still there to diagnose
            again, _ = lane.prove_composer(cs, 11)
            assert again.raw_bytes() == good.raw_bytes(), name
        finally:
            lane.close()
