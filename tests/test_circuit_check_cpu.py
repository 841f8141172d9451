"""The circuit check's host mirror (plk_composer_check with a NULL context: the kernel's per-gate
function of csrc/circuit_check.hpp in a host loop) against the Python-integer model
tests/circuit_check_ref.py, and the model against the pinned quotient model. No GPU."""
import ctypes as C
import random

import pytest

import circuit_check_ref as M
import prover_stage_ref as S
import test_prover_oracle as T

r = S.r


def host(cs, cap=None):
    """The host mirror's verdict with every failing gate listed (cap >= m)."""
    return M.report_tuple(cs.check(host=True, max_failures=cs.m() if cap is None else cap))


def model(cs):
    return M.summarize(M.check(cs))


# ---- the model against the pinned model ---------------------------------------------------
def _weighted(terms, k):
    return sum(t * pow(k, j, r) for j, t in enumerate(terms)) % r


def test_model_terms_sum_to_the_pinned_widgets():
    rng = random.Random(0xC1C)
    for _ in range(20):
        a, a_n, b, b_n, c, d, d_n, q_l, q_r, q_c, k = (rng.randrange(r) for _ in range(11))
        assert _weighted(M.logic_terms(a, a_n, b, b_n, c, d, d_n, q_c), k) == \
            S.logic_widget(a, a_n, b, b_n, c, d, d_n, q_c, k)
        assert _weighted(M.fixed_terms(a, a_n, b, b_n, c, d, d_n, q_l, q_r, q_c), k) == \
            S.fixed_base_widget(a, a_n, b, b_n, c, d, d_n, q_l, q_r, q_c, k)
        assert _weighted(M.var_terms(a, a_n, b, b_n, c, d, d_n), k) == \
            S.var_base_widget(a, a_n, b, b_n, c, d, d_n, k)


def test_model_arithmetic_and_range_are_the_quotient_rows():
    """prover_stage_ref.quotient on two points with alpha = 0 (no permutation or L1 term),
    1 / v_h = 1 and one widget on: row 0 is the arithmetic term plus PI, or range_sep times the
    range terms weighted by powers of range_sep^2."""
    rng = random.Random(0xC2C)
    for _ in range(10):
        a, b, c, d = ([rng.randrange(r), rng.randrange(r)] for _ in range(4))
        q = [rng.randrange(r) for _ in range(11)]
        pi, sep = rng.randrange(r), rng.randrange(1, r)
        ch = dict(alpha=0, beta=rng.randrange(r), gamma=rng.randrange(r), range_sep=sep,
                  logic_sep=0, fixed_sep=0, var_sep=0)
        sel = [[v, 0] for v in q]
        rnd = [[rng.randrange(r), rng.randrange(r)] for _ in range(4)]
        args = dict(z=[1, 1], l1=[0, 0], sigma=rnd, elements=[1, r - 1], s_m=[7], vh_inv=[1])
        off = dict(range=False, logic=False, fixed=False, var=False)
        t = S.quotient(2, 1, a, b, c, d, args["z"], [pi, 0], args["l1"], sel, args["sigma"],
                       args["elements"], ch, args["s_m"], args["vh_inv"], off)
        assert t[0] == M.gate_check(q[:7] + [0] * 4, a[0], b[0], c[0], d[0], a[1], b[1], d[1], pi)[1]
        only_range = [[0, 0] for _ in range(11)]
        only_range[S.QRANGE] = [1, 0]
        t = S.quotient(2, 1, a, b, c, d, args["z"], None, args["l1"], only_range, args["sigma"],
                       args["elements"], ch, args["s_m"], args["vh_inv"], dict(off, range=True))
        assert t[0] == sep * _weighted(M.range_terms(a[0], b[0], c[0], d[0], d[1]), sep * sep % r) % r


# ---- the host mirror against the model ------------------------------------------------------
@pytest.mark.parametrize("name,fn,seed", T.CASES, ids=[c[0] for c in T.CASES])
def test_satisfied_circuits_pass(plk, name, fn, seed):
    cs = T.build(fn)
    rep = cs.check(host=True)
    assert rep.ok and bool(rep) and rep.failing == 0 and rep.failures == []
    assert rep.gates == cs.m()
    assert model(cs)[0] == 0


BAD = M.bad_cases()


@pytest.mark.parametrize("name,bad,good,m,gates", BAD, ids=[c[0] for c in BAD])
def test_unsatisfied_circuits(plk, name, bad, good, m, gates):
    cs = T.build(bad)
    assert cs.m() == m
    want = model(cs)
    assert [(g, mk) for g, mk, _ in want[2]] == [(g, 0x1) for g in gates]
    assert host(cs, cap=m) == want
    rep = cs.check(host=True)
    assert not rep.ok and not rep and rep.gates == m
    assert T.build(good).check(host=True).ok


def test_tamper_sweep(plk):
    seen, last_gate_failed = 0, False
    for name, cs, idx in M.sweep_cases():
        assert model(cs)[0] == 0, name
        for w in idx:
            with M.tampered(cs, w):
                want = model(cs)
                assert host(cs) == want, (name, w)
                for g, mk, _ in want[2]:
                    seen |= mk
                    last_gate_failed |= g == cs.m() - 1
    missing = [b for b in M.ALL_TERM_BITS if not seen >> b & 1]
    assert not missing, f"term bits the sweep never set: {missing}"
    assert seen == sum(1 << b for b in M.ALL_TERM_BITS)
    assert last_gate_failed


def test_pooled_public_input_gate(plk):
    cs = T.build(T.public_sum(10, 20, 31))
    rep = cs.check(host=True)
    _, idx = cs.public_inputs()
    assert [(f.gate, f.mask, f.residual) for f in rep.failures] == [(idx[0], 0x1, r - 1)]
    assert host(cs) == model(cs)
    assert str(rep.failures[0]) == f"gate {idx[0]}: arithmetic, residual = {r - 1:#x}"
    assert T.build(T.public_sum(10, 20, 30)).check(host=True).ok


def test_report_strings(plk):
    _, cs, idx = M.sweep_cases()[-1]
    with M.tampered(cs, idx[0]):
        rep = cs.check(host=True)
    f = rep.failures[0]
    assert f.gate == cs.m() - 1 and f.classes == ["range"] and f.terms == [("range", 3)]
    assert str(f) == f"gate {f.gate}: range term 3"
    assert str(rep).splitlines()[0] == f"1 of {rep.gates} gates fail"


def test_cap_semantics(plk):
    from dusk_plonk_amd.prover import PlkCheckSummary, PlkGateFailure, Plonk, _bind
    cs = Plonk()
    cs.synthetic_chain(40, 5)
    nw = cs.export()[1].shape[0]
    for w in range(8, nw, 3):
        cs.set_witness(w, cs[w] + 1)
    failing, by_class, fails = model(cs)
    assert failing > 8
    lib = _bind()
    s, cnt = PlkCheckSummary(), C.c_size_t(99)
    assert lib.plk_composer_check(None, cs._h, C.byref(s), None, 0, C.byref(cnt)) == plk.PLK_OK
    assert (s.gates, s.failing, cnt.value) == (cs.m(), failing, 0)
    assert list(s.by_class) == by_class
    assert lib.plk_composer_check(None, cs._h, C.byref(s), None, 0, None) == plk.PLK_OK
    out = (PlkGateFailure * 5)()
    assert lib.plk_composer_check(None, cs._h, C.byref(s), out, 5, C.byref(cnt)) == plk.PLK_OK
    assert cnt.value == 5 and s.failing == failing
    assert [(o.gate, o.mask) for o in out] == [(g, mk) for g, mk, _ in fails[:5]]
    rep = cs.check(host=True, max_failures=failing + 7)
    assert len(rep.failures) == failing
    assert cs.check(host=True, max_failures=0).failures == []


def test_null_arguments(plk):
    from dusk_plonk_amd.prover import PlkCheckSummary, Plonk, _bind
    lib, s, cs = _bind(), PlkCheckSummary(), Plonk()
    assert lib.plk_composer_check(None, None, C.byref(s), None, 0, None) == plk.PLK_E_ARG
    assert lib.plk_composer_check(None, cs._h, None, None, 0, None) == plk.PLK_E_ARG
    assert lib.plk_prover_diagnose(None, C.byref(s), None, 0, None) == plk.PLK_E_ARG
    assert lib.plk_key_diagnose(None, C.byref(s), None, 0, None) == plk.PLK_E_ARG
    assert lib.plk_check_last_ms(None, None) == plk.PLK_E_ARG


def test_symbols_declared_and_exported(plk):
    lib = plk.plonk._lib()
    for name in ("plk_composer_check", "plk_prover_diagnose", "plk_key_diagnose", "plk_check_last_ms"):
        assert name in plk.ABI_SYMBOLS
        assert hasattr(lib, name)
    assert lib.plk_abi_version() == 2
    assert plk.CircuitReport is not None and plk.GateFailure is not None
