"""The quotient round on five n-point cosets (csrc/prover.hpp): GPU proofs byte for byte
against the restated CPU prover (oracle/plk_prover_oracle.c, which works over g H_8n like the
reference), the block transform of polynomials longer than n against the oracle's 8n coset
transform, the three public-input paths (rotated L1 rows up to kPiSparse = 4, pk_pi_coef up to
kPiDirect = 16, the idft beyond) and the degree failure of an unsatisfied circuit.

Sizes: k = 4 is the smallest domain that takes five blocks (eight coefficients left for the
zero check of t_4); 5 / 9 and 10 / 12 sit either side of the n-point transform's single-pass
limit (ntt.hip plan_domain: one pass up to 2^9). Three-pass plans are covered by the 2^20
fixture test of tests/test_prover_oracle.py.
"""
import ctypes as C

import numpy as np
import pytest

from oracle_lib import random_fr

pytestmark = pytest.mark.gpu

R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def tau_for(seed):
    from dusk_plonk_amd.prover import fr_int
    t = random_fr(1, seed=seed)[0]
    return t, fr_int(t)


def n_trim(m):
    """Points of the trimmed SRS: next_pow2(m + 6) + 8 (key.rs:81-82)."""
    return (1 << max(0, (m + 6 - 1).bit_length())) + 8


def assert_proof_equals(proof, pis, ref):
    from dusk_plonk_amd.prover import fr_int
    raw = np.frombuffer(proof.raw_bytes(), dtype=np.uint64)
    assert np.array_equal(raw[: 11 * 13].reshape(11, 13), ref["comms"]), "commitments differ"
    assert np.array_equal(raw[11 * 13:].reshape(16, 4), ref["evals"]), "evaluations differ"
    assert pis == [fr_int(p) for p in ref["pis"]]


def params_for(plk, m, tau_limbs):
    """PlonkParams covering the circuit's trimmed SRS, and that SRS's points for the oracle."""
    k = max(0, (n_trim(m) - 8 - 1).bit_length())
    pp = plk.PlonkParams.setup(k, tau_limbs)
    return pp, pp.points(0, n_trim(m))


def bench_like(k, seed):
    """bench.py's circuit (Plonk::initialize, the chain, one public input) at n = 2^k: m = n - 8
    gates as in the benchmark, except at k = 4 where n - 8 = 8 gates would pad to n = 8: there
    m = n - 6 = 10, the most the trimmed SRS of 2^4 + 8 points takes."""
    from dusk_plonk_amd.prover import Plonk
    m = (1 << k) - (6 if k == 4 else 8)
    cs = Plonk()
    cs.synthetic_chain(m - 7, seed)
    cs.append_public((seed * 0x9E3779B97F4A7C15 + 12345) % (1 << 250))
    assert cs.m() == m
    return cs


@pytest.mark.parametrize("k", [4, 5, 9, 10, 12])
def test_bench_circuit_proof_equals_oracle(plk, oracle, k):
    from dusk_plonk_amd.prover import PlonkKey
    tau_limbs, _ = tau_for(0xD0 + k)
    cs = bench_like(k, 90 + k)
    gates, wit = cs.export()
    pp, srs = params_for(plk, gates.shape[0], tau_limbs)
    ref = oracle.prove(gates, wit, srs, b"blocks", 3 + k)
    prover, vd = PlonkKey.compile_composer(pp, b"blocks", cs)
    assert vd.n == 1 << k
    assert np.array_equal(vd.comms, ref["vk"])
    proof, pis = prover.prove_composer(cs, 3 + k)
    assert_proof_equals(proof, pis, ref)


@pytest.fixture(scope="module")
def chain_keys(plk):
    """One compiled key per size, shared by the block-evaluation cases."""
    from dusk_plonk_amd.prover import PlonkKey
    keys = {}
    for k in (4, 10):
        tau_limbs, _ = tau_for(0xE0 + k)
        cs = bench_like(k, 5)
        pp, _ = params_for(plk, cs.m(), tau_limbs)
        keys[k] = PlonkKey.compile_composer(pp, b"blocks", cs)[0]
    return keys


@pytest.mark.parametrize("extra", [0, 1, 3, 8])
@pytest.mark.parametrize("k", [4, 10])
def test_block_eval_equals_oracle_coset_8n(plk, oracle, chain_keys, k, extra):
    """plk_debug_block_eval (the prover's forward block transform, folding the coefficients
    past n onto the block): block m, row u is point 8u + m of the oracle's coset_dft over
    g H_8n — exact equality of the canonical Montgomery words."""
    n = 1 << k
    coef = random_fr(n + extra, seed=1000 * k + extra)
    lib = plk.plonk._lib()
    blocks = C.c_int()
    out = np.zeros((5 * n, 4), dtype=np.uint64)
    st = lib.plk_debug_block_eval(chain_keys[k]._key, coef.ctypes.data_as(C.c_void_p),
                                  coef.shape[0], out.ctypes.data_as(C.c_void_p), out.shape[0],
                                  C.byref(blocks))
    assert st == plk.PLK_OK and blocks.value == 5
    ref = oracle.coset_dft(coef, k + 3)
    for m in range(5):
        assert np.array_equal(out[m * n:(m + 1) * n], ref[m::8]), f"block {m}"


def public_inputs_circuit(k, where):
    """m = n = 2^k gates: the six of Plonk::initialize, then chain gates with a public-input
    gate (append_public) at every gate index in `where`."""
    from dusk_plonk_amd.prover import Plonk
    n = 1 << k
    cs = Plonk()
    at = 6
    for j, i in enumerate(sorted(where) + [n]):
        if i > at:
            cs.synthetic_chain(i - at, 17 + j)
        if i < n:
            cs.append_public(0x1234567 * (j + 1) + (j << 200))
        at = i + 1
    assert cs.m() == n
    return cs


def pi_layouts(n):
    """count -> gate indices. The first gate a circuit can carry a public input on is gate 6
    (after Plonk::initialize) and the last is row n - 1, whose rotation (u - (n - 1)) mod n
    wraps for every u but the last; n - 2 / n - 1 and 6 / 7 are the adjacent pairs."""
    spread = [8 + (j * (n - 11)) // 12 for j in range(12)]  # 12 distinct rows in [8, n - 3)
    return {
        "1_first": [6], "1_last": [n - 1],
        "4": [6, 7, n - 2, n - 1],
        "5": [6, 7, n // 2, n - 2, n - 1],
        "17": sorted(set([6, 7, n - 3, n - 2, n - 1] + spread)),
    }


@pytest.mark.parametrize("layout", ["1_first", "1_last", "4", "5", "17"])
@pytest.mark.parametrize("k", [5, 10])
def test_public_inputs_proof_equals_oracle(plk, oracle, k, layout):
    from dusk_plonk_amd.prover import PlonkKey
    where = pi_layouts(1 << k)[layout]
    assert len(where) == int(layout.split("_")[0])
    tau_limbs, _ = tau_for(0xF0 + k)
    cs = public_inputs_circuit(k, where)
    gates, wit = cs.export()
    pp, srs = params_for(plk, gates.shape[0], tau_limbs)
    ref = oracle.prove(gates, wit, srs, b"pi", 21)
    prover, vd = PlonkKey.compile_composer(pp, b"pi", cs)
    assert vd.n == 1 << k and list(vd.pi_indexes) == where
    assert np.array_equal(vd.comms, ref["vk"])
    proof, pis = prover.prove_composer(cs, 21)
    assert len(pis) == len(where)
    assert_proof_equals(proof, pis, ref)


@pytest.mark.parametrize("k", [4, 10])
def test_one_wrong_witness_fails_with_degree_error(plk, k):
    """The chain's last output off by one: the interpolant over the five blocks does not
    vanish in t[4n + 8, 5n) and the t_4 commit's zero check fails (csrc/prover.hpp)."""
    from dusk_plonk_amd.prover import PlonkKey
    tau_limbs, _ = tau_for(0xC0 + k)
    cs = bench_like(k, 9)
    pp, _ = params_for(plk, cs.m(), tau_limbs)
    prover, _ = PlonkKey.compile_composer(pp, b"bad", cs)
    prover.prove_composer(cs, 1)  # the satisfied circuit proves
    _, wit = cs.export()
    w = wit.shape[0] - 2  # the last chain gate's output (the public input's witness follows)
    cs.set_witness(w, (cs[w] + 1) % R_MOD)
    with pytest.raises(plk.PlonkError) as e:
        prover.prove_composer(cs, 1)
    assert e.value.status == plk.PLK_E_DEGREE
