"""CPU tests of the verifier's host side (csrc/verifier.hip): the symbols, Verifier::new's
argument checks, the transcript replay (plk_verifier_challenges) against the Python replay on
the committed 2^20 proof, and the test helper tests/verifier_pair.py against tests/verifier.py.
None of them needs a GPU.
"""
from pathlib import Path

import ctypes as C
import numpy as np
import pytest

import verifier
import verifier_pair as VP
from test_prover_oracle import tau_for

GOLD = Path(__file__).resolve().parent / "golden" / "proof_2_20.npz"
NEW_SYMBOLS = ("plk_msm_points", "plk_msm_points_ranges", "plk_verifier_create",
               "plk_verifier_destroy", "plk_verifier_challenges", "plk_verifier_fold",
               "plk_verifier_last_fold_stats")


@pytest.fixture(scope="module")
def fixture(plk):
    """The bench circuit's proof at n = 2^20 (tests/golden/make_proof_2_20.py): m = n - 8 gates,
    the one public input on the last gate, label b"bench", tau from seed 0x5EED."""
    from dusk_plonk_amd.prover import Proof, VerifierData, fr_int
    g = dict(np.load(GOLD, allow_pickle=False))
    n = 1 << int(g["meta"][0])
    vd = VerifierData(b"bench", n, n - 8, g["vk"], [n - 9])
    proof = Proof.from_words(g["comms"], g["evals"])
    pis = [fr_int(p) for p in g["pis"]]
    return vd, proof, pis, tau_for(int(g["meta"][3]))[1], g


def test_symbols_exported_and_bound(plk):
    from dusk_plonk_amd.prover import _bind
    lib = _bind()
    for s in NEW_SYMBOLS:
        assert s in plk.ABI_SYMBOLS and hasattr(lib, s)
        assert getattr(lib, s).argtypes is not None, s
    assert lib.plk_abi_version() == 2
    assert callable(plk.msm_points) and callable(plk.PlonkParams.msm_points)


def test_create_rejects_bad_arguments(plk, fixture):
    from dusk_plonk_amd.prover import _bind
    lib = _bind()
    vk = np.ascontiguousarray(fixture[4]["vk"])
    vkp = vk.ctypes.data_as(C.c_void_p)
    idx = (C.c_uint64 * 1)(3)
    h = C.c_void_p()
    assert lib.plk_verifier_create(None, 8, 7, vkp, idx, 1, C.byref(h)) == plk.PLK_E_ARG
    assert lib.plk_verifier_create(b"x", 8, 7, None, idx, 1, C.byref(h)) == plk.PLK_E_ARG
    assert lib.plk_verifier_create(b"x", 8, 7, vkp, None, 1, C.byref(h)) == plk.PLK_E_ARG
    assert lib.plk_verifier_create(b"x", 8, 7, vkp, idx, 1, None) == plk.PLK_E_ARG
    for n in (0, 1, 6, 12, (1 << 20) + 1):  # not a power of two >= 2
        assert lib.plk_verifier_create(b"x", n, 7, vkp, idx, 0, C.byref(h)) == plk.PLK_E_ARG, n
    idx[0] = 8  # a public input index outside the domain
    assert lib.plk_verifier_create(b"x", 8, 7, vkp, idx, 1, C.byref(h)) == plk.PLK_E_ARG
    assert not h.value
    assert lib.plk_verifier_create(b"x", 8, 7, vkp, None, 0, C.byref(h)) == plk.PLK_OK and h.value
    assert lib.plk_verifier_destroy(h) == plk.PLK_OK
    assert lib.plk_verifier_destroy(None) == plk.PLK_E_ARG
    assert lib.plk_verifier_challenges(None, None, None, None) == plk.PLK_E_ARG
    assert lib.plk_verifier_fold(None, None, None, None, 0, None, None) == plk.PLK_E_ARG
    assert lib.plk_msm_points(None, None, None, 0, None) == plk.PLK_E_ARG


def test_helper_agrees_with_the_restated_verifier(fixture):
    """tests/verifier_pair.py's accept / reject is tests/verifier.py's."""
    from verifier_pair import copy_proof
    vd, proof, pis, tau, _ = fixture
    verifier.verify(vd, proof, pis, tau)
    assert VP.accepts(vd, proof, pis, tau)
    bad = copy_proof(proof, b_eval=(proof.b_eval + 1) % verifier.r)
    with pytest.raises(verifier.VerificationError):
        verifier.verify(vd, bad, pis, tau)
    assert not VP.accepts(vd, bad, pis, tau)
    with pytest.raises(verifier.VerificationError):
        verifier.verify(vd, proof, [(pis[0] + 1) % verifier.r], tau)
    assert not VP.accepts(vd, proof, [(pis[0] + 1) % verifier.r], tau)


def test_challenges_equal_the_python_replay(fixture):
    from verifier_pair import copy_proof
    vd, proof, pis, _, _ = fixture
    ver = vd.verifier()
    want = VP.pair(vd, proof, pis)[0]
    got = ver.challenges(proof, pis)
    assert got == want
    # one evaluation changed: it enters the transcript after z, so the challenges from v on move
    # and the earlier ones do not
    moved = copy_proof(proof, q_l_eval=(proof.q_l_eval + 1) % verifier.r)
    got2 = ver.challenges(moved, pis)
    assert got2 == VP.pair(vd, moved, pis)[0]
    assert got2[:8] == got[:8]
    assert all(a != b for a, b in zip(got2[8:], got[8:]))


def test_wrong_public_input_count_raises_before_the_gpu(plk, fixture):
    """InconsistentPublicInputsLen (verifier.rs:51-56): PLK_E_ARG from the Python mirror, with
    no context made (this test runs without a GPU)."""
    vd, proof, pis, _, _ = fixture
    ver = vd.verifier()
    for bad in ([[]], [pis + pis], [pis, pis], []):
        with pytest.raises(plk.PlonkError) as e:
            ver.fold([proof], bad)
        assert e.value.status == plk.PLK_E_ARG
    with pytest.raises(plk.PlonkError) as e:
        ver.challenges(proof, [])
    assert e.value.status == plk.PLK_E_ARG
