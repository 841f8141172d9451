"""Python-integer model of the circuit check (include/plk.h, "circuit check"; csrc/circuit_check.hpp):
every summand of the numerator of prover_stage_ref.quotient evaluated on its own at a gate, from
`Plonk.export()`. The permutation and L1 terms are left out (wires are witness indices). The next
row of gate i is gate i + 1; of the last gate, the zero row.

Mask bits: 0 arithmetic (its value is the residual); 4..7 range; 8..12 logic; 16..19 fixed-base;
20..22 variable-base. A widget's bits are evaluated only where its selector is non-zero."""
from __future__ import annotations

import numpy as np

from prover_stage_ref import EDWARDS_D, delta, r

RINV = pow(1 << 256, -1, r)
ARITH, RANGE0, LOGIC0, FIXED0, VAR0 = 0, 4, 8, 16, 20
CLASS_MASK = (0x1, 0xF << 4, 0x1F << 8, 0xF << 16, 0x7 << 20)  # arith range logic fixed var
ALL_TERM_BITS = ([ARITH] + [RANGE0 + j for j in range(4)] + [LOGIC0 + j for j in range(5)]
                 + [FIXED0 + j for j in range(4)] + [VAR0 + j for j in range(3)])


def range_terms(a, b, c, d, d_n):
    return [delta((c - 4 * d) % r), delta((b - 4 * c) % r), delta((a - 4 * b) % r),
            delta((d_n - 4 * a) % r)]


def logic_terms(a, a_n, b, b_n, c, d, d_n, q_c):
    qa, qb, qd, w = (a_n - 4 * a) % r, (b_n - 4 * b) % r, (d_n - 4 * d) % r, c
    s = qa + qb
    f = w * (w * (4 * w - 18 * s + 81) + 18 * (qa * qa + qb * qb) - 81 * s + 83)
    xor_and = 3 * (s + qd) - 2 * f + q_c * (9 * qd - 3 * s)
    return [delta(qa), delta(qb), delta(qd), (w - qa * qb) % r, xor_and % r]


def fixed_terms(a, a_n, b, b_n, c, d, d_n, q_l, q_r, q_c):
    bit = (d_n - 2 * d) % r
    y_alpha = (bit * bit * (q_r - 1) + 1) % r
    x_alpha = q_l * bit % r
    prod = c * a * b * EDWARDS_D % r
    return [bit * (bit - 1) * (bit + 1) % r, (bit * q_c - c) % r,
            (a_n * (1 + prod) - (a * y_alpha + b * x_alpha)) % r,
            (b_n * (1 - prod) - (b * y_alpha + a * x_alpha)) % r]


def var_terms(a, a_n, b, b_n, c, d, d_n):
    x1, y1, x2, y2, x3, y3, x1y2 = a, b, c, d, a_n, b_n, d_n
    dp = EDWARDS_D * x1y2 * y1 * x2 % r
    return [(x1 * y2 - x1y2) % r, (x1y2 + y1 * x2 - x3 * (1 + dp)) % r,
            (y1 * y2 + x1 * x2 - y3 * (1 - dp)) % r]


def gate_check(q, a, b, c, d, a_n, b_n, d_n, pi):
    """(mask, residual) of one gate; q the 11 selectors in SEL order, plain values."""
    q_m, q_l, q_r, q_o, q_4, q_c, q_arith, q_range, q_logic, q_fixed, q_var = q
    res = (q_arith * (q_m * a * b + q_l * a + q_r * b + q_o * c + q_4 * d + q_c) + pi) % r
    mask = int(res != 0) << ARITH
    groups = []
    if q_range:
        groups.append((RANGE0, range_terms(a, b, c, d, d_n)))
    if q_logic:
        groups.append((LOGIC0, logic_terms(a, a_n, b, b_n, c, d, d_n, q_c)))
    if q_fixed:
        groups.append((FIXED0, fixed_terms(a, a_n, b, b_n, c, d, d_n, q_l, q_r, q_c)))
    if q_var:
        groups.append((VAR0, var_terms(a, a_n, b, b_n, c, d, d_n)))
    for lo, terms in groups:
        for j, t in enumerate(terms):
            mask |= int(t != 0) << (lo + j)
    return mask, res


def _ints(words) -> list:
    """(k, 4) uint64 Montgomery rows -> plain ints."""
    w = np.asarray(words, dtype=np.uint64).reshape(-1, 4)
    return [sum(int(x) << (64 * i) for i, x in enumerate(row)) * RINV % r for row in w]


def check_export(gates, wit, pi_override=None):
    """[(mask, residual)] per gate of an exported circuit (gates (m, 51), witness (nw, 4)).
    pi_override: public-input values by ordinal in place of the exported ones."""
    m = gates.shape[0]
    w = _ints(wit)
    sel = _ints(np.ascontiguousarray(gates[:, :44]).reshape(-1, 4))
    pis = _ints(np.ascontiguousarray(gates[:, 47:51]))
    wires = [(int(g[44]) & 0xFFFFFFFF, int(g[44]) >> 32, int(g[45]) & 0xFFFFFFFF, int(g[45]) >> 32)
             for g in gates]
    out, ordinal = [], 0
    for i in range(m):
        a, b, c, d = (w[j] for j in wires[i])
        a_n, b_n, _, d_n = (w[j] for j in wires[i + 1]) if i + 1 < m else (0, 0, 0, 0)
        pi = 0
        if int(gates[i][46]) & 1:
            pi = pis[i] if pi_override is None else pi_override[ordinal] % r
            ordinal += 1
        out.append(gate_check(sel[11 * i: 11 * i + 11], a, b, c, d, a_n, b_n, d_n, pi))
    return out


def check(cs, pi_override=None):
    return check_export(*cs.export(), pi_override=pi_override)


def summarize(verdicts):
    """(failing, [by class], [(gate, mask, residual) of the failing gates, ascending])."""
    fails = [(i, mk, res) for i, (mk, res) in enumerate(verdicts) if mk]
    by_class = [sum(1 for _, mk, _ in fails if mk & cm) for cm in CLASS_MASK]
    return len(fails), by_class, fails


# ---- the circuits both test files check -------------------------------------------------
def bad_cases():
    """The nine unsatisfied circuits of test_prover_oracle.test_oracle_rejects_unsatisfied with
    the matching satisfied circuit of the same structure, the gate count and the failing gates
    (all with mask 0x1): (name, bad builder, good builder, m, [gates])."""
    import test_prover_oracle as T
    return [
        ("boolean2", T.boolean(2), T.boolean(1), 7, [6]),
        ("range_neg", T.ranged((T.R_MOD - 2**77) % T.R_MOD, 76), T.ranged(7, 76), 18, [17]),
        ("range_2^76", T.ranged(2**76, 76), T.ranged(7, 76), 18, [17]),
        ("decomposition_flip", T.decomposition(0x1234567890ABCDEF * 31337, 256, flip=10),
         T.decomposition(0x1234567890ABCDEF * 31337, 256), 775, [529]),
        ("and_wrong", T.logic(T.A_RND, T.B_RND, 254, False, wrong=True),
         T.logic(T.A_RND, T.B_RND, 254, False), 135, [134]),
        ("xor_wrong", T.logic(T.A_RND, T.B_RND, 64, True, wrong=True),
         T.logic(T.A_RND, T.B_RND, 64, True), 40, [39]),
        ("mul_generator_wrong", T.mul_generator(T.JJ_A, wrong=True), T.mul_generator(T.JJ_A),
         269, [267, 268]),
        ("add_point_wrong", T.add_point(T.JJ_A, T.JJ_B, wrong=True), T.add_point(T.JJ_A, T.JJ_B),
         10, [8, 9]),
        ("test_circuit_wrong_c", T.readme_circuit(20, 5, 26, 100, 2),
         T.readme_circuit(20, 5, 25, 100, 2), 287, [6]),
    ]


def range_tail(cs):
    """A circuit whose LAST gate is a range gate (append_custom_gate, q_range = 1) on a fresh
    zero witness: its next row is the zero row. Returns that witness."""
    from dusk_plonk_amd.prover import Constraint
    cs.component_range(cs.append_witness(2**64 - 1), 76)
    z = cs.append_witness(0)
    cs.append_custom_gate(Constraint().range(1).a(z))
    return z


def sweep_cases():
    """(name, composer, witness indexes to tamper): the four circuits of the tamper sweep, each
    with w = 2, 2 + s, ... for s = max(1, nw // 60), and range_tail with its own witness."""
    import test_prover_oracle as T
    out = []
    for name, fn in (("ranged", T.ranged(2**64 - 1, 76)), ("logic", T.logic(T.A_RND, T.B_RND, 30, False)),
                     ("mul_generator", T.mul_generator(T.JJ_A)), ("add_point", T.add_point(T.JJ_A, T.JJ_B))):
        cs = T.build(fn)
        nw = cs.export()[1].shape[0]
        out.append((name, cs, list(range(2, nw, max(1, nw // 60)))))
    from dusk_plonk_amd.prover import Plonk
    cs = Plonk()
    out.append(("range_tail", cs, [range_tail(cs)]))
    return out


class tampered:
    """with tampered(cs, w): witness w is one larger inside the block."""

    def __init__(self, cs, w, add=1):
        self.cs, self.w, self.add = cs, w, add

    def __enter__(self):
        self.old = self.cs[self.w]
        self.cs.set_witness(self.w, (self.old + self.add) % r)
        return self.cs

    def __exit__(self, *exc):
        self.cs.set_witness(self.w, self.old)
        return False


def report_tuple(rep):
    """A CircuitReport in the shape of summarize(): (failing, [by class], [(gate, mask, residual)])."""
    from dusk_plonk_amd.prover import GATE_CLASSES
    return (rep.failing, [rep.by_class[c] for c in GATE_CLASSES],
            [(f.gate, f.mask, f.residual) for f in rep.failures])
