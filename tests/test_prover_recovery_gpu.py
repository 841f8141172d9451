"""A failed create_proof must leave its prover or lane as good as new. PLK_E_DEGREE returns from
the middle of round 3, after the lane's buffers, the MSM workspace's generation stamps and the
transcript have been used; the structure check returns PLK_E_ARG before round 1. Everywhere else
in the suite a failure is the last thing its prover or lane does. Here the proofs made AFTER a
failure are compared byte for byte with the same proof made before it, with a freshly compiled
prover's, and (lanes) with the same proof made alone afterwards; each good proof of the
single-prover sequences is also accepted by the restated verifier (tests/verifier.py).
"""
import concurrent.futures as cf

import pytest

from test_prover_gpu import Boolean, Ranged, tau_and_params
from test_prover_lanes import fresh, setup_key
from test_quotient_domain_gpu import bench_like
from verifier import verify

pytestmark = pytest.mark.gpu

R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def composer(circuit):
    from dusk_plonk_amd.prover import Plonk
    cs = Plonk()
    circuit.synthesize(cs)
    return cs


def unsatisfied_chain(cs):
    """The chain's last output off by one (the public input's witness follows it), as in
    tests/test_quotient_domain_gpu.py."""
    _, wit = cs.export()
    w = wit.shape[0] - 2
    cs.set_witness(w, (cs[w] + 1) % R_MOD)
    return cs


def sequence(plk, pp, tau, label, key_cs, a, bad, b):
    """prove a -> fail on bad -> prove a again -> prove b, on one prover; a, bad, b are
    functions that build a composer."""
    from dusk_plonk_amd.prover import PlonkKey
    prover, vd = PlonkKey.compile_composer(pp, label, key_cs())
    first, pis_a = prover.prove_composer(a(), 21)
    verify(vd, first, pis_a, tau)
    with pytest.raises(plk.PlonkError) as e:
        prover.prove_composer(bad(), 22)
    assert e.value.status == plk.PLK_E_DEGREE
    again, pis_again = prover.prove_composer(a(), 21)
    assert again.raw_bytes() == first.raw_bytes() and pis_again == pis_a
    other, pis_b = prover.prove_composer(b(), 23)
    verify(vd, other, pis_b, tau)
    new, vd_new = PlonkKey.compile_composer(pp, label, key_cs())
    want, want_pis = new.prove_composer(b(), 23)
    assert other.raw_bytes() == want.raw_bytes() and pis_b == want_pis
    assert other.raw_bytes() != first.raw_bytes()
    return prover


def test_chain_2_6_after_a_degree_failure(plk):
    """n = 2^6, one public input: the wires are committed from their Lagrange values."""
    tau, pp = tau_and_params(plk, 6, 0x2EC)
    prover = sequence(plk, pp, tau, b"recover", lambda: bench_like(6, 5), lambda: bench_like(6, 5),
                      lambda: unsatisfied_chain(bench_like(6, 5)), lambda: bench_like(6, 9))
    assert prover.n == 64
    ln = prover.lane()
    try:
        ln.prove_composer(bench_like(6, 5), 21)
        assert ln.commit_info()[0] == ["lagrange"] * 4
    finally:
        ln.close()


def test_range_after_a_degree_failure(plk):
    tau, pp = tau_and_params(plk, 6, 8349)
    sequence(plk, pp, tau, b"demo", lambda: composer(Ranged(7, 76)), lambda: composer(Ranged(7, 76)),
             lambda: composer(Ranged((R_MOD - 2**77) % R_MOD, 76)),
             lambda: composer(Ranged(2**64 - 1, 76)))


def test_boolean_after_a_degree_failure(plk):
    tau, pp = tau_and_params(plk, 4, 8349)
    sequence(plk, pp, tau, b"plonk", lambda: composer(Boolean(1)), lambda: composer(Boolean(1)),
             lambda: composer(Boolean(2)), lambda: composer(Boolean(0)))


@pytest.fixture(scope="module")
def key10(plk):
    return setup_key(plk, 10)


def test_three_lanes_one_failing_every_other_proof(plk, key10):
    """Three lanes of one n = 2^10 key in three threads: lane 1 alternates unsatisfied and good
    circuits (four of each), lanes 0 and 2 prove four good circuits each."""
    _, _, prover, _, gates = key10
    lanes = [prover.lane() for _ in range(3)]
    jobs = {i: [(100 * i + j, 300 + 10 * i + j, False) for j in range(4)] for i in (0, 2)}
    jobs[1] = [(100 + j // 2, 310 + j // 2, j % 2 == 0) for j in range(8)]  # bad, good, bad, ...

    def run(i):
        out = []
        for cseed, bseed, bad in jobs[i]:
            cs = fresh(gates, cseed)
            if not bad:
                out.append((cseed, bseed, lanes[i].prove_composer(cs, bseed)))
                continue
            try:
                lanes[i].prove_composer(unsatisfied_chain(cs), bseed)
                out.append((cseed, bseed, None))
            except plk.PlonkError as e:
                out.append((cseed, bseed, e.status))
        return out

    try:
        with cf.ThreadPoolExecutor(3) as ex:
            got = list(ex.map(run, range(3)))
        assert [len(g) for g in got] == [4, 8, 4]
        assert [r[2] for r in got[1][0::2]] == [plk.PLK_E_DEGREE] * 4
        alone = lanes[0]
        good = [r for g in got for r in g if not isinstance(r[2], int)]
        assert len(good) == 12 and all(r[2] is not None for r in good)
        for cseed, bseed, (proof, pis) in good:
            want, want_pis = alone.prove_composer(fresh(gates, cseed), bseed)
            assert proof.raw_bytes() == want.raw_bytes() and pis == want_pis, (cseed, bseed)
        # and lane 1 once more, after the threads have joined
        proof, pis = lanes[1].prove_composer(fresh(gates, 555), 556)
        want, want_pis = alone.prove_composer(fresh(gates, 555), 556)
        assert proof.raw_bytes() == want.raw_bytes() and pis == want_pis
    finally:
        for ln in lanes:
            ln.close()


def test_proof_after_a_structure_mismatch_equals_a_fresh_provers(plk, key10):
    """The refusals of tests/test_prover_lanes.py::test_structure_mismatch_is_refused, then the
    bytes of the next proof."""
    from dusk_plonk_amd.prover import Constraint, Plonk, PlonkKey
    _, pp, prover, _, gates = key10
    other = Plonk()  # same gate count, different wiring (no copy chain)
    for i in range(gates):
        w = other.append_witness(i + 3)
        other.append_gate(Constraint().left(1).a(w).constant(-(i + 3)))
    other.append_public(5)
    moved = Plonk()  # the public input at another gate
    moved.append_public((1 * 0x9E3779B97F4A7C15 + 12345) % (1 << 250))
    moved.synthetic_chain(gates, 1)
    for cs in (other, moved):
        assert cs.m() == prover.m
        with pytest.raises(plk.PlonkError) as e:
            prover.prove_composer(cs, 1)
        assert e.value.status == plk.PLK_E_ARG
    p, pi = prover.prove_composer(fresh(gates, 77), 1)
    new, _ = PlonkKey.compile_composer(pp, b"lanes", fresh(gates, 1))
    want, want_pi = new.prove_composer(fresh(gates, 77), 1)
    assert p.raw_bytes() == want.raw_bytes() and pi == want_pi and len(pi) == 1
