"""The KZG pair of the restated verifier — TEST INFRASTRUCTURE.

tests/verifier.py's `verify` checks a proof and returns nothing; the verifier on the GPU
(plk_verifier_fold) returns the two G1 points (C, W) that go into the final pairing equation
e(C, H) == e(W, [tau]H). `pair` restates verify's computation (the same transcript replay and
algebra, /root/reference/src/prover/proof.rs:70-591 and commitment_scheme.rs:24-152, with
verifier.py's helpers) and RETURNS (challenges, total_c, total_w), so the tests can pin the
pair itself. tests/test_verifier_cpu.py keeps it honest: its accept / reject agrees with
verifier.verify.
"""
from __future__ import annotations

import numpy as np

import pyref as P
from verifier import (K1, K2, K3, SEED_LABELS, VerificationError, append_commitment,
                      append_scalar, base_transcript, challenge_scalar, gmul, gsum, pt, r)

COMM_NAMES = ("a_comm", "b_comm", "c_comm", "d_comm", "z_comm", "t_low_comm", "t_mid_comm",
              "t_high_comm", "t_4_comm", "w_z_chall_comm", "w_z_chall_w_comm")


def delta(f):
    return f * (f - 1) * (f - 2) * (f - 3) % r


def pair(vd, proof, public_inputs):
    """-> ([beta, gamma, alpha, range, logic, fixed, variable separation, z, v_a, v_b, u],
    total_c, total_w) with the points as pyref affine (x, y) tuples or None."""
    if len(public_inputs) != len(vd.pi_indexes):
        raise VerificationError("InconsistentPublicInputsLen")
    t = base_transcript(vd)
    for v in public_inputs:
        append_scalar(t, b"pi", v)
    n = vd.n
    C = {c: pt(getattr(proof, c)) for c in COMM_NAMES}
    for lab, c in ((b"a_w", "a_comm"), (b"b_w", "b_comm"), (b"c_w", "c_comm"), (b"d_w", "d_comm")):
        append_commitment(t, lab, C[c])
    beta = challenge_scalar(t, b"beta")
    append_scalar(t, b"beta", beta)
    gamma = challenge_scalar(t, b"gamma")
    append_commitment(t, b"z", C["z_comm"])
    alpha = challenge_scalar(t, b"alpha")
    range_sep = challenge_scalar(t, b"range separation challenge")
    logic_sep = challenge_scalar(t, b"logic separation challenge")
    fixed_sep = challenge_scalar(t, b"fixed base separation challenge")
    var_sep = challenge_scalar(t, b"variable base separation challenge")
    for lab, c in ((b"t_low", "t_low_comm"), (b"t_mid", "t_mid_comm"), (b"t_high", "t_high_comm"),
                   (b"t_4", "t_4_comm")):
        append_commitment(t, lab, C[c])
    z = challenge_scalar(t, b"z_challenge")

    e = proof
    omega = P.omega(n.bit_length() - 1)
    zn = pow(z, n, r)
    z_h = (zn - 1) % r
    if z_h == 0 or z == 1:
        raise VerificationError("z in the domain")
    l1 = z_h * pow(n * (z - 1) % r, -1, r) % r
    winv = pow(omega, -1, r)
    pi_eval = 0
    for idx, v in zip(vd.pi_indexes, public_inputs):
        if v % r:
            pi_eval += v * pow((pow(winv, idx, r) * z - 1) % r, -1, r)
    pi_eval = pi_eval * z_h * pow(n, -1, r) % r
    b0 = (e.a_eval + beta * e.s_sigma_1_eval + gamma) % r
    b1 = (e.b_eval + beta * e.s_sigma_2_eval + gamma) % r
    b2 = (e.c_eval + beta * e.s_sigma_3_eval + gamma) % r
    b3 = (e.d_eval + gamma) * e.perm_eval * alpha % r
    t_eval = ((e.r_poly_eval + pi_eval) - b0 * b1 * b2 * b3 - l1 * alpha * alpha) \
        * pow(z_h, -1, r) % r
    t_comm = gsum([(C["t_low_comm"], 1), (C["t_mid_comm"], zn), (C["t_high_comm"], zn * zn),
                   (C["t_4_comm"], zn * zn * zn)])
    for lab, v in ((b"a_eval", e.a_eval), (b"b_eval", e.b_eval), (b"c_eval", e.c_eval),
                   (b"d_eval", e.d_eval), (b"a_next_eval", e.a_next_eval),
                   (b"b_next_eval", e.b_next_eval), (b"d_next_eval", e.d_next_eval),
                   (b"s_sigma_1_eval", e.s_sigma_1_eval), (b"s_sigma_2_eval", e.s_sigma_2_eval),
                   (b"s_sigma_3_eval", e.s_sigma_3_eval), (b"q_arith_eval", e.q_arith_eval),
                   (b"q_c_eval", e.q_c_eval), (b"q_l_eval", e.q_l_eval),
                   (b"q_r_eval", e.q_r_eval), (b"perm_eval", e.perm_eval),
                   (b"t_eval", t_eval), (b"r_eval", e.r_poly_eval)):
        append_scalar(t, lab, v)
    vk = {lab.decode(): pt(c) for lab, c in zip(SEED_LABELS, vd.comms)}
    qar = e.q_arith_eval
    terms = [(vk["q_m"], e.a_eval * e.b_eval * qar), (vk["q_l"], e.a_eval * qar),
             (vk["q_r"], e.b_eval * qar), (vk["q_o"], e.c_eval * qar), (vk["q_4"], e.d_eval * qar),
             (vk["q_c"], qar)]
    kap = range_sep * range_sep % r
    rr = (delta(e.c_eval - 4 * e.d_eval) + delta(e.b_eval - 4 * e.c_eval) * kap
          + delta(e.a_eval - 4 * e.b_eval) * kap * kap
          + delta(e.d_next_eval - 4 * e.a_eval) * kap * kap * kap) % r
    terms.append((vk["q_range"], rr * range_sep))
    k = logic_sep * logic_sep % r
    qa = (e.a_next_eval - 4 * e.a_eval) % r
    qb = (e.b_next_eval - 4 * e.b_eval) % r
    qd = (e.d_next_eval - 4 * e.d_eval) % r
    w = e.c_eval
    f = w * (w * (4 * w - 18 * (qa + qb) + 81) + 18 * (qa * qa + qb * qb)
             - 81 * (qa + qb) + 83) % r
    xor_and = (3 * (qa + qb + qd) - 2 * f + e.q_c_eval * (9 * qd - 3 * (qa + qb))) % r
    lt = (delta(qa) + delta(qb) * k + delta(qd) * k ** 2 + (w - qa * qb) * k ** 3
          + xor_and * k ** 4) % r
    terms.append((vk["q_logic"], lt * logic_sep))
    ed = (-10240 * pow(10241, -1, r)) % r
    k = fixed_sep * fixed_sep % r
    ax, axn, ay, ayn = e.a_eval, e.a_next_eval, e.b_eval, e.b_next_eval
    xya, acc, accn = e.c_eval, e.d_eval, e.d_next_eval
    xb, yb, xyb = e.q_l_eval, e.q_r_eval, e.q_c_eval
    bit = (accn - 2 * acc) % r
    ya = (bit * bit * (yb - 1) + 1) % r
    xa = xb * bit % r
    prod = xya * ax * ay * ed % r
    w = (bit * (bit - 1) * (bit + 1) + (bit * xyb - xya) * k
         + (axn + axn * prod - (ax * ya + ay * xa)) * k ** 2
         + (ayn - ayn * prod - (ay * ya + ax * xa)) * k ** 3) % r
    terms.append((vk["q_fixed_group_add"], w * fixed_sep))
    k = var_sep * var_sep % r
    x1, x3, y1, y3 = e.a_eval, e.a_next_eval, e.b_eval, e.b_next_eval
    x2, y2, x1y2 = e.c_eval, e.d_eval, e.d_next_eval
    dp = ed * x1y2 * y1 * x2 % r
    w = ((x1 * y2 - x1y2) + (x1y2 + y1 * x2 - (x3 + x3 * dp)) * k
         + (y1 * y2 + x1 * x2 - (y3 - y3 * dp)) * k * k) % r
    terms.append((vk["q_variable_group_add"], w * var_sep))
    bz = beta * z % r
    x = ((e.a_eval + bz + gamma) * (e.b_eval + K1 * bz + gamma) * (e.c_eval + K2 * bz + gamma)
         * (e.d_eval + K3 * bz + gamma) * alpha) % r
    terms.append((C["z_comm"], x + l1 * alpha * alpha))
    terms.append((vk["s_sigma_4"], -(b0 * b1 * b2 * beta * e.perm_eval * alpha) % r))
    # an identity key commitment contributes nothing whatever its scalar (verifier.py skips them)
    r_comm = gsum([(p, s) for p, s in terms if p is not None])
    va = challenge_scalar(t, b"v_challenge")
    parts_a = [(t_eval, t_comm), (e.r_poly_eval, r_comm), (e.a_eval, C["a_comm"]),
               (e.b_eval, C["b_comm"]), (e.c_eval, C["c_comm"]), (e.d_eval, C["d_comm"]),
               (e.s_sigma_1_eval, vk["s_sigma_1"]), (e.s_sigma_2_eval, vk["s_sigma_2"]),
               (e.s_sigma_3_eval, vk["s_sigma_3"])]
    vb = challenge_scalar(t, b"v_challenge")
    parts_b = [(e.perm_eval, C["z_comm"]), (e.a_next_eval, C["a_comm"]),
               (e.b_next_eval, C["b_comm"]), (e.d_next_eval, C["d_comm"])]

    def flatten(parts, v):
        comm = gsum([(c, pow(v, i, r)) for i, (_, c) in enumerate(parts)])
        ev = sum(val * pow(v, i, r) for i, (val, _) in enumerate(parts)) % r
        return comm, ev

    fa = flatten(parts_a, va)
    fb = flatten(parts_b, vb)
    append_commitment(t, b"w_z", C["w_z_chall_comm"])
    append_commitment(t, b"w_z_w", C["w_z_chall_w_comm"])
    u = challenge_scalar(t, b"batch")
    points = [z, z * omega % r]
    total_c, total_w, g_mult = None, None, 0
    for k, ((comm, ev), w, point) in enumerate(zip((fa, fb), (C["w_z_chall_comm"],
                                                              C["w_z_chall_w_comm"]), points)):
        uk = pow(u, k, r)
        c = P.g1_add(comm, gmul(w, point))
        g_mult = (g_mult + uk * ev) % r
        total_c = P.g1_add(total_c, gmul(c, uk))
        total_w = P.g1_add(total_w, gmul(w, uk))
    total_c = P.g1_add(total_c, gmul(P.G1_GEN, -g_mult))
    ch = [beta, gamma, alpha, range_sep, logic_sep, fixed_sep, var_sep, z, va, vb, u]
    return ch, total_c, total_w


def accepts(vd, proof, public_inputs, tau: int) -> bool:
    """e(C, H) == e(W, [tau]H) checked as C == tau W with the trapdoor (tests only)."""
    _, c, w = pair(vd, proof, public_inputs)
    return c == gmul(w, tau)


def to_words(p):
    """pyref affine point (or None) -> uint64[13] ABI words."""
    return P.g1_vec_to_np([p])[0]


def copy_proof(proof, **changes):
    """A copy of `proof` with evaluations (canonical ints) or commitments (uint64[13]) replaced."""
    from dusk_plonk_amd.prover import Proof, _COMMS, _EVALS, _fr, fr_limbs
    comms = np.stack([np.asarray(changes.get(c, getattr(proof, c)), dtype=np.uint64)
                      for c in _COMMS])
    evals = np.stack([fr_limbs(_fr(changes.get(e, getattr(proof, e)))) for e in _EVALS])
    return Proof.from_words(comms, evals)
