"""The device-replay additions of the verifier that need no GPU: the fold weights' host mirror
(plk_debug_fold_weights with ctx = NULL, which runs the compiled-schedule transcript of
csrc/transcript_dev.hpp on the host) against a restatement with the Python merlin transcript,
the replay mode switch and the NULL-argument checks of the new entry points."""
import ctypes as C

import pytest

import pyref as P
from transcript import Transcript

R = P.R_MOD


def restated_weights(entropy: bytes, u: list) -> list:
    """rho_0 = 1; rho_j = 128 bits of challenge_bytes("rho", 16) from a clone of the root
    (count, every u, the entropy) after append_u64("index", j)."""
    root = Transcript(b"plk-verifier-fold")
    root.append_u64(b"count", len(u))
    for x in u:
        root.append_message(b"u", x.to_bytes(32, "little"))
    root.append_message(b"entropy", entropy)
    out = [1]
    for j in range(1, len(u)):
        t = root.clone()
        t.append_u64(b"index", j)
        out.append(int.from_bytes(t.challenge_bytes(b"rho", 16), "little"))
    return out


def fold_weights(plk, ctx_handle, entropy: bytes, u: list) -> list:
    from dusk_plonk_amd.prover import PlkFr, _bind, _fr, fr_int
    n = len(u)
    arr = (PlkFr * max(1, n))(*[_fr(x) for x in u])
    out = (PlkFr * max(1, n))()
    ent = (C.c_uint8 * 32)(*entropy)
    st = _bind().plk_debug_fold_weights(ctx_handle, ent, arr, n, out)
    if st != plk.PLK_OK:
        raise plk.PlonkError(st, "plk_debug_fold_weights")
    return [fr_int(out[j]) for j in range(n)]


@pytest.mark.parametrize("count", [1, 3, 70])
def test_host_mirror_of_the_fold_weights(plk, count):
    entropy = bytes((7 * i + count) % 256 for i in range(32))
    u = [pow(5, 1000 + 31 * j + count, R) for j in range(count)]
    got = fold_weights(plk, None, entropy, u)
    assert got == restated_weights(entropy, u)
    assert got[0] == 1
    assert all(r < 1 << 128 for r in got[1:])
    assert len(set(got)) == count
    if count > 1:  # bound to the entropy and to every u
        other = fold_weights(plk, None, bytes(32), u)
        assert all(a != b for a, b in zip(got[1:], other[1:]))
        u2 = u[:-1] + [(u[-1] + 1) % R]
        assert all(a != b for a, b in zip(got[1:], fold_weights(plk, None, entropy, u2)[1:]))


def test_fold_weights_argument_checks(plk):
    from dusk_plonk_amd.prover import PlkFr, _bind
    b = _bind()
    ent, one, out = (C.c_uint8 * 32)(), (PlkFr * 1)(), (PlkFr * 1)()
    assert b.plk_debug_fold_weights(None, None, one, 1, out) == plk.PLK_E_ARG
    assert b.plk_debug_fold_weights(None, ent, None, 1, out) == plk.PLK_E_ARG
    assert b.plk_debug_fold_weights(None, ent, one, 1, None) == plk.PLK_E_ARG
    assert b.plk_debug_fold_weights(None, ent, one, 0, out) == plk.PLK_E_ARG
    for i, limb in enumerate(P.int_to_limbs(R, 4)):  # u = r: not canonical
        one[0].l[i] = limb
    assert b.plk_debug_fold_weights(None, ent, one, 1, out) == plk.PLK_E_ARG


def _host_verifier(plk):
    """A verifier needs no GPU: identity key commitments, two public inputs."""
    import numpy as np
    from dusk_plonk_amd.prover import VerifierData
    comms = np.zeros((15, 13), dtype=np.uint64)
    comms[:, 12] = 1
    return VerifierData(b"replay", 8, 5, comms, [1, 3]).verifier()


def test_set_replay(plk):
    from dusk_plonk_amd.prover import _bind
    ver = _host_verifier(plk)
    b = _bind()
    assert ver.replay == "host"
    assert b.plk_verifier_set_replay(ver._h, 1) == plk.PLK_OK
    assert b.plk_verifier_set_replay(ver._h, 0) == plk.PLK_OK
    assert b.plk_verifier_set_replay(ver._h, 2) == plk.PLK_E_ARG
    assert b.plk_verifier_set_replay(ver._h, -1) == plk.PLK_E_ARG
    ver.set_replay("device")
    assert ver.replay == "device"
    with pytest.raises(plk.PlonkError) as err:
        ver.set_replay(2)
    assert err.value.status == plk.PLK_E_ARG
    with pytest.raises(plk.PlonkError) as err:
        ver.set_replay("gpu")
    assert err.value.status == plk.PLK_E_ARG
    assert ver.replay == "device"
    assert ver.last_replay_ms() == 0.0


def test_new_entry_points_reject_null_without_gpu(plk):
    from dusk_plonk_amd.prover import PlkFr, PlkProof, _bind
    b = _bind()
    ver = _host_verifier(plk)
    proofs, pis, out = (PlkProof * 1)(), (PlkFr * 2)(), (PlkFr * 11)()
    ms = C.c_float()
    assert b.plk_verifier_set_replay(None, 0) == plk.PLK_E_ARG
    assert b.plk_verifier_last_replay_ms(None, C.byref(ms)) == plk.PLK_E_ARG
    assert b.plk_verifier_last_replay_ms(ver._h, None) == plk.PLK_E_ARG
    assert b.plk_verifier_challenges_batch(None, ver._h, proofs, pis, 1, out) == plk.PLK_E_ARG
    assert b.plk_verifier_challenges_batch(None, None, None, None, 0, None) == plk.PLK_E_ARG
