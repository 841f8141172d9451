"""The circuit check on the GPU (k_gate_check, csrc/circuit_check.hip): plk_composer_check on the
device against the host mirror and the Python-integer model (tests/circuit_check_ref.py), mask
for mask, at the shapes where a gate-per-lane kernel with wave and block reductions can go
wrong, and plk_prover_diagnose / plk_key_diagnose on the witness a prover holds."""
import pytest

import circuit_check_ref as M
import test_prover_oracle as T
from oracle_lib import random_fr

pytestmark = pytest.mark.gpu

r = T.R_MOD


def model(cs, pi_override=None):
    return M.summarize(M.check(cs, pi_override))


def agree(cs, ctx, want=None):
    """Device == host mirror == model on `cs`, every failing gate listed; returns the model's."""
    want = want or model(cs)
    assert M.report_tuple(cs.check(ctx, max_failures=cs.m())) == want
    assert M.report_tuple(cs.check(host=True, max_failures=cs.m())) == want
    return want


_PP = {}


def params(plk, m):
    """PlonkParams for a circuit of m gates (one per size, shared by the tests)."""
    k = max(0, (T.n_trim(m) - 8 - 1).bit_length())
    if k not in _PP:
        _PP[k] = plk.PlonkParams.setup(k, random_fr(1, seed=900 + k)[0])
    return _PP[k]


def compile_key(plk, cs, label=b"check"):
    from dusk_plonk_amd.prover import PlonkKey
    return PlonkKey.compile_composer(params(plk, cs.m()), label, cs)[0]


def fails_degree(plk, fn):
    with pytest.raises(plk.PlonkError) as e:
        fn()
    assert e.value.status == plk.PLK_E_DEGREE
    return e.value


# ---- device == host mirror == model --------------------------------------------------------
@pytest.mark.parametrize("name,fn,seed", T.CASES, ids=[c[0] for c in T.CASES])
def test_satisfied_circuits(plk, gpu_ctx, name, fn, seed):
    cs = T.build(fn)
    want = agree(cs, gpu_ctx)
    assert want[0] == 0
    rep = cs.check(gpu_ctx)
    assert rep.ok and rep.gates == cs.m() and rep.failures == []
    assert plk.check_last_ms(gpu_ctx) > 0


BAD = M.bad_cases()


@pytest.mark.parametrize("name,bad,good,m,gates", BAD, ids=[c[0] for c in BAD])
def test_unsatisfied_circuits(plk, gpu_ctx, name, bad, good, m, gates):
    cs = T.build(bad)
    want = agree(cs, gpu_ctx)
    assert [(g, mk) for g, mk, _ in want[2]] == [(g, 0x1) for g in gates]


def test_tamper_sweep(plk, gpu_ctx):
    seen = 0
    for name, cs, idx in M.sweep_cases():
        for w in idx:
            with M.tampered(cs, w):
                for _, mk, _ in agree(cs, gpu_ctx)[2]:
                    seen |= mk
    assert seen == sum(1 << b for b in M.ALL_TERM_BITS)


# ---- shapes: wave (64) and block (256) boundaries --------------------------------------------
def wire(cs, gate, col):
    """The witness index of column col (0 a, 1 b, 2 o, 3 d) of a gate."""
    g = cs.export()[0][gate]
    return (int(g[44 + col // 2]) >> (32 * (col % 2))) & 0xFFFFFFFF


@pytest.mark.parametrize("m", [63, 64, 65, 255, 256, 257, 1025])
def test_chain_boundaries(plk, gpu_ctx, m):
    from dusk_plonk_amd.prover import Plonk
    cs = Plonk()
    cs.synthetic_chain(m - 6, 40 + m)
    assert cs.m() == m
    assert agree(cs, gpu_ctx)[0] == 0
    edges = {0, m - 1} | {e + s for e in range(64, m + 1, 64) for s in (-1, 0)}
    edges |= {e + s for e in (256, 512, 768, 1024) for s in (-1, 0)}
    for g in sorted(e for e in edges if 0 <= e < m):
        # gate 0 pins Plonk::ZERO, which every chain gate carries on its d wire: tamper its a wire
        with M.tampered(cs, wire(cs, g, 0 if g == 0 else 2)):
            want = agree(cs, gpu_ctx)
            assert g in [f[0] for f in want[2]], (m, g)
            rep = cs.check(gpu_ctx, max_failures=1)
            assert [f.gate for f in rep.failures] == [want[2][0][0]]


@pytest.mark.parametrize("widget,col,bit", [("range", 3, M.RANGE0 + 3), ("logic", 0, M.LOGIC0)])
def test_widget_row_straddles_the_block_boundary(plk, gpu_ctx, widget, col, bit):
    """A widget row at gate 255 whose next row is gate 256, the first lane of the next block:
    the accumulator on the far side is tampered, and gate 255 fails the term that reads it."""
    from dusk_plonk_amd.prover import Plonk
    cs = Plonk()
    cs.synthetic_chain(249, 3)  # the widget's first row is gate 6 + 249
    if widget == "range":
        cs.component_range(cs.append_witness(2**64 - 1), 76)
    else:
        cs.append_logic_and(cs.append_witness(T.A_RND & (2**30 - 1)),
                            cs.append_witness(T.B_RND & (2**30 - 1)), 30)
    sel = cs.export()[0][:, 28:32] if widget == "range" else cs.export()[0][:, 32:36]
    assert sel[255].any() and sel[256].any() and not sel[254].any()
    assert agree(cs, gpu_ctx)[0] == 0
    with M.tampered(cs, wire(cs, 256, col), add=4):  # a quad moved by 4 leaves 0..3
        want = agree(cs, gpu_ctx)
        at255 = [mk for g, mk, _ in want[2] if g == 255]
        assert at255 and at255[0] >> bit & 1


def test_many_failures(plk, gpu_ctx):
    from dusk_plonk_amd.prover import GATE_CLASSES, Plonk
    cs = Plonk()
    cs.synthetic_chain(1019, 9)
    assert cs.m() == 1025
    for w in range(2, cs.export()[1].shape[0], 3):
        cs.set_witness(w, cs[w] + 1)
    failing, by_class, fails = agree(cs, gpu_ctx)
    assert failing > 256
    rep = cs.check(gpu_ctx, max_failures=16)
    assert rep.failing == failing and [rep.by_class[c] for c in GATE_CLASSES] == by_class
    assert [(f.gate, f.mask, f.residual) for f in rep.failures] == fails[:16]
    assert [f.gate for f in rep.failures] == sorted(f.gate for f in rep.failures)
    assert cs.check(gpu_ctx, max_failures=0).failing == failing


# ---- diagnosis -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,bad,good,m,gates", BAD, ids=[c[0] for c in BAD])
def test_diagnose_unsatisfied(plk, gpu_ctx, name, bad, good, m, gates):
    good_cs, bad_cs = T.build(good), T.build(bad)
    prover = compile_key(plk, good_cs)
    prover.prove_composer(good_cs, 5)
    assert prover.diagnose().ok
    fails_degree(plk, lambda: prover.prove_composer(bad_cs, 5))
    rep = prover.diagnose(max_failures=m)
    assert not rep.ok
    assert rep == bad_cs.check(gpu_ctx, max_failures=m)
    assert M.report_tuple(rep) == model(bad_cs)
    err = fails_degree(plk, lambda: prover.prove_composer(bad_cs, 5, explain=True))
    assert err.report == prover.diagnose() and not err.report.ok
    assert fails_degree(plk, lambda: prover.prove_composer(bad_cs, 5)).report is None


@pytest.mark.parametrize("name,fn,seed", T.CASES, ids=[c[0] for c in T.CASES])
def test_diagnose_satisfied(plk, gpu_ctx, name, fn, seed):
    cs = T.build(fn)
    prover = compile_key(plk, cs)
    prover.prove_composer(cs, seed, explain=True)  # succeeds: the report says so
    rep = prover.diagnose()
    assert rep.ok and rep.gates == cs.m()


def test_public_inputs_are_per_proof(plk, gpu_ctx):
    """One PublicSum key, three proofs with different public inputs: the diagnosis reads this
    proof's values, not the compile-time ones and not the previous proof's."""
    prover = compile_key(plk, T.build(T.public_sum(10, 20, 30)))
    prover.prove_composer(T.build(T.public_sum(10, 20, 30)), 1)
    assert prover.diagnose().ok
    bad = T.build(T.public_sum(10, 20, 31))
    fails_degree(plk, lambda: prover.prove_composer(bad, 1))
    rep = prover.diagnose()
    _, idx = bad.public_inputs()
    assert [(f.gate, f.mask, f.residual) for f in rep.failures] == [(idx[0], 0x1, r - 1)]
    assert rep == bad.check(gpu_ctx)
    prover.prove_composer(T.build(T.public_sum(1, 2, 3)), 1)
    assert prover.diagnose().ok


def test_diagnosis_leaves_the_prover_undisturbed(plk, gpu_ctx):
    good, bad = T.build(T.ranged(7, 76)), T.build(T.ranged(2**76, 76))
    prover = compile_key(plk, good)
    lane = prover.lane()
    for p in (prover, lane):
        with pytest.raises(plk.PlonkError) as e:  # no proof yet: no witness to check
            p.diagnose()
        assert e.value.status == plk.PLK_E_ARG
    want = compile_key(plk, good).prove_composer(good, 77)[0].raw_bytes()
    for p in (prover, lane):
        fails_degree(plk, lambda: p.prove_composer(bad, 77))
        assert p.diagnose().failing == 1
        assert p.prove_composer(good, 77)[0].raw_bytes() == want
        assert p.diagnose().ok
    # a proof refused for its structure leaves no witness to check
    with pytest.raises(plk.PlonkError) as e:
        lane.prove_composer(T.build(T.boolean(1)), 77)
    assert e.value.status == plk.PLK_E_ARG
    with pytest.raises(plk.PlonkError) as e:
        lane.diagnose()
    assert e.value.status == plk.PLK_E_ARG
    lane.close()
