"""Round 1's wire commits from Lagrange values (lagrange.hip, commit.hip).

Basis: the Lagrange-basis SRS of a 2^k domain (n + 3 points: [L_i(tau)]G1, then the three
blinder points [tau^(n+t)]G1 - [tau^t]G1) commits [values | blinders] to the same point, bit for
bit, as the SRS itself commits idft(values) + b(X)(X^n - 1); built from the points alone (an SRS
reloaded through plk_srs_load gives the same table).
Proofs: the bench circuit proved with the Lagrange commit on and off gives the same bytes.
Guard: a wire whose values crowd one MSM bucket is committed from its coefficients.
"""
import numpy as np
import pytest

from oracle_lib import random_fr
from test_prover_oracle import bench_chain, build, n_trim, tau_for

R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
KS = [3, 5, 10, 12]


def to_int(limbs):
    return sum(int(limbs[i]) << (64 * i) for i in range(4))


def to_limbs(v):
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def blinded_coefficients(oracle, values, blinders, k):
    """idft(values) + b(X)(X^n - 1) as Montgomery limbs (sums of Montgomery forms are
    Montgomery forms): n + len(blinders) coefficients."""
    n = 1 << k
    coef = oracle.idft(values, k)
    out = np.zeros((n + len(blinders), 4), dtype=np.uint64)
    out[:n] = coef
    for i, b in enumerate(blinders):
        out[i] = to_limbs((to_int(out[i]) - to_int(b)) % R_MOD)
        out[n + i] = b
    return out


def value_cases(k):
    """(name, values, blinders): dense random; three nonzero values; all zeros with nonzero
    blinders; all zeros with zero blinders (the identity)."""
    n = 1 << k
    zero = np.zeros((n, 4), dtype=np.uint64)
    sparse = zero.copy()
    for j, i in enumerate([0, n // 2 + 1, n - 1]):
        sparse[i] = random_fr(1, seed=900 + 10 * k + j)[0]
    return [
        ("dense", random_fr(n, seed=40 + k), random_fr(2, seed=50 + k)),
        ("three", sparse, random_fr(2, seed=60 + k)),
        ("zeros_blinded", zero, random_fr(2, seed=70 + k)),
        ("identity", zero, np.zeros((2, 4), dtype=np.uint64)),
    ]


@pytest.fixture(scope="module")
def bases(plk, gpu_ctx):
    """Per k: the SRS from setup, the same points reloaded, and both Lagrange-basis SRSs."""
    out = {}
    for k in KS:
        tau, _ = tau_for(0x1A6 + k)
        pp = plk.PlonkParams.setup(k, tau, gpu_ctx)
        re = plk.PlonkParams.load(pp.points(), gpu_ctx)
        out[k] = (pp, pp.lagrange(k), re.lagrange(k))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_lagrange_srs_from_points_alone(bases, k):
    """A reloaded SRS (no tau) gives the same n + 3 points as the one made by setup."""
    _, lag, lag_re = bases[k]
    assert lag.n == (1 << k) + 3
    assert np.array_equal(lag.points(), lag_re.points())


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_lagrange_commit_equals_coefficient_commit(plk, oracle, bases, k):
    pp, lag, lag_re = bases[k]
    for name, values, blinders in value_cases(k):
        want = pp.commit(plk.Coefficients(blinded_coefficients(oracle, values, blinders, k))).words
        scalars = np.concatenate([values, blinders])
        assert np.array_equal(lag.commit(plk.Coefficients(scalars)).words, want), name
        assert np.array_equal(lag_re.commit(plk.Coefficients(scalars)).words, want), name
        if name == "identity":
            assert int(want[12]) == 1
        if name == "dense":  # and against the C oracle's MSM over the Lagrange points
            assert np.array_equal(oracle.msm(lag.points(), scalars), want)


@pytest.mark.gpu
def test_lagrange_srs_tau_root_of_unity(plk, oracle, gpu_ctx):
    """tau = the domain generator at k = 4: [L_i(tau)] is the generator for i = 1 and infinity
    elsewhere, and Z_0 = [tau^n] - [1] is infinity. Commits agree with the coefficient path."""
    k, n = 4, 16
    omega = oracle.elements(k)[1]
    pp = plk.PlonkParams.setup(k, omega, gpu_ctx)
    lag = pp.lagrange(k)
    pts = lag.points()
    inf = pts[:, 12] != 0
    assert list(np.nonzero(~inf[:n])[0]) == [1]
    assert np.array_equal(pts[1], pp.points(0, 1)[0])
    assert inf[n] and inf[n + 1] and inf[n + 2]  # tau^(n+t) = tau^t
    for name, values, blinders in value_cases(k):
        want = pp.commit(plk.Coefficients(blinded_coefficients(oracle, values, blinders, k))).words
        got = lag.commit(plk.Coefficients(np.concatenate([values, blinders]))).words
        assert np.array_equal(got, want), name


def prove_lane(prover, cs, seed):
    ln = prover.lane()
    try:
        proof, pis = ln.prove_composer(cs, seed)
        return proof.raw_bytes(), pis, ln.commit_info()
    finally:
        ln.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 12])
def test_bench_proof_same_bytes_with_switch_off(plk, gpu_ctx, monkeypatch, k):
    """The bench circuit, proved on a key with the Lagrange-basis SRS and on one compiled under
    PLK_LAGRANGE_COMMIT=0: identical bytes; all four wires on the Lagrange basis, the fourth
    (zero but for the dummy gates) with fewer than 100 MSM entries."""
    from dusk_plonk_amd.prover import PlonkKey
    tau, _ = tau_for(0xB0B + k)
    cs = build(bench_chain((1 << k) - 15, 79))
    pp = plk.PlonkParams.setup(k, tau, gpu_ctx)
    prover, _ = PlonkKey.compile_composer(pp, b"bench", cs)
    on_bytes, on_pis, (basis, entries) = prove_lane(prover, cs, 13)
    assert basis == ["lagrange"] * 4
    assert entries[3] < 100, entries
    assert min(entries[:3]) > 1000, entries  # the dense wires' commits were counted
    monkeypatch.setenv("PLK_LAGRANGE_COMMIT", "0")
    prover_off, _ = PlonkKey.compile_composer(pp, b"bench", cs)
    off_bytes, off_pis, (basis_off, _) = prove_lane(prover_off, cs, 13)
    assert basis_off == ["coefficient"] * 4
    assert on_bytes == off_bytes and on_pis == off_pis


def constant_b_circuit(gates, const_gates, seed):
    """`gates` addition gates a + b = o with random a; b is the witness 5 on the first
    `const_gates` of them and random on the rest."""
    def f(cs):
        from dusk_plonk_amd.prover import Constraint, fr_int
        five = cs.append_witness(5)
        vals = random_fr(2 * gates, seed=seed)
        for i in range(gates):
            wa = cs.append_witness(fr_int(vals[2 * i]))
            wb = five if i < const_gates else cs.append_witness(fr_int(vals[2 * i + 1]))
            cs.gate_add(Constraint().left(1).right(1).a(wa).b(wb))
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("const_gates,b_basis", [(1000, "coefficient"), (170, "lagrange")],
                         ids=["hot", "under_bound"])
def test_guard_sends_crowded_wire_to_coefficients(plk, oracle, gpu_ctx, const_gates, b_basis):
    """k = 10 (c = 10: 512 buckets, a dense wire ~52 entries each, bound 4 x 64 = 256). b = 5 on
    all 1000 gates puts 1000 entries into bucket 4: that wire is committed from its coefficients,
    the others from their values. b = 5 on 170 gates (~222 entries in the bucket) stays under the
    bound. Either way the proof is the CPU prover oracle's, byte for byte."""
    from dusk_plonk_amd.prover import PlonkKey
    tau, _ = tau_for(0x60A2D)
    cs = build(constant_b_circuit(1000, const_gates, 5))
    gates, wit = cs.export()
    assert 512 < gates.shape[0] <= 1024
    pp = plk.PlonkParams.setup(10, tau, gpu_ctx)
    ref = oracle.prove(gates, wit, pp.points(0, n_trim(gates.shape[0])), b"guard", 3)
    prover, vd = PlonkKey.compile_composer(pp, b"guard", cs)
    assert np.array_equal(vd.comms, ref["vk"])
    raw, _, (basis, entries) = prove_lane(prover, cs, 3)
    assert basis == ["lagrange", b_basis, "lagrange", "lagrange"], (basis, entries)
    words = np.frombuffer(raw, dtype=np.uint64)
    assert np.array_equal(words[: 11 * 13].reshape(11, 13), ref["comms"])
    assert np.array_equal(words[11 * 13:].reshape(16, 4), ref["evals"])
