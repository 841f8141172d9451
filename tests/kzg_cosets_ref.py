"""Python-integer model of the coset openings (include/plk.h plk_kzg_open_cosets / _fold_cosets).

n = 2^k, l = 2^log_l, r = n / l, w = omega(k). Coset j < r is w^j <w^r>, its vanishing polynomial
X^l - psi^j with psi = w^l, and f = q_j (X^l - psi^j) + I_j with deg I_j < l; the witness is
[q_j(tau)]G.
  * the definition: plain long division by X^l - y (divide_by_coset, coset_witness_logs);
  * the pipeline of csrc/kzg.hip (fk_open_cosets) over any group of tests/kzg_ref.py: per residue
    a < l the table DFT_2r of the reversed, identity-padded sub-SRS s_(a + b l), the coefficients
    (2r)^-1 DFT_2r of f_(a + c l), their products summed over a, the unscaled IDFT_2r, its slice
    [r, 2r) and the final DFT_r;
  * the interpolant from the l values alone (coset_interpolant): I = sum_i c_i z^-i X^i with
    c = IDFT_l(values), for any non-zero shift z;
  * the fold of openings into one pair, in the exponent (fold_cosets_pair_logs).
"""
import kzg_ref as K
import pyref as P

R = P.R_MOD


def fr_dft(xs, k: int):
    return list(xs) if k == 0 else P.dft(xs, k)


def fr_idft(xs, k: int):
    return list(xs) if k == 0 else P.idft(xs, k)


def group_dft(G, xs, k: int, inverse: bool = False):
    return list(xs) if k == 0 else K.group_dft(G, xs, k, inverse)


def group_fft(G, xs, k: int, inverse: bool = False):
    return list(xs) if k == 0 else K.group_fft(G, xs, k, inverse)


def divide_by_coset(f, l: int, y: int):
    """(q, rem) with f = q (X^l - y) + rem, deg rem < l: schoolbook long division."""
    rem = [c % R for c in f]
    q = [0] * max(len(rem) - l, 0)
    for i in range(len(rem) - 1, l - 1, -1):
        c = rem[i]
        q[i - l] = c
        rem[i] = 0
        rem[i - l] = (rem[i - l] + c * y) % R
    rem = rem[:l] + [0] * (l - len(rem))
    return q, rem


def coset_witness_logs(f, tau: int, k: int, log_l: int):
    """The definition: log of pi_j = q_j(tau) for every coset j < r."""
    l, r = 1 << log_l, 1 << (k - log_l)
    psi = pow(P.omega(k), l, R)
    return [P.poly_eval(divide_by_coset(f, l, pow(psi, j, R))[0], tau) for j in range(r)]


def coset_values(f, z: int, log_l: int):
    """f on the coset z <w_l>, in the l-point domain's natural order."""
    w = P.omega(log_l) if log_l else 1
    return [P.poly_eval(f, z * pow(w, i, R) % R) for i in range(1 << log_l)]


def coset_interpolant(values, z: int, log_l: int):
    """The coefficients of the polynomial of degree < l that takes `values` on z <w_l>."""
    c = fr_idft(values, log_l)
    zi = pow(z, -1, R)
    return [ci * pow(zi, i, R) % R for i, ci in enumerate(c)]


def fk_open_cosets(G, srs, f, k: int, log_l: int, group_dft=group_dft):
    """The pipeline of csrc/kzg.hip over the group G; srs: at least n elements of G, s_m."""
    n, l, lr = 1 << k, 1 << log_l, k - log_l
    r = 1 << lr
    assert len(f) <= n <= len(srs)
    if r == 1:
        return [G.zero]
    f = list(f) + [0] * (n - len(f))
    inv2r = pow(2 * r, -1, R)
    U = [G.zero] * (2 * r)
    for a in range(l):
        sa, fa = srs[a::l][:r], f[a::l]
        table = group_dft(G, [sa[r - 1 - i] for i in range(r)] + [G.zero] * r, lr + 1)
        B = [x * inv2r % R for x in fr_dft(fa + [0] * r, lr + 1)]
        for t in range(2 * r):
            U[t] = G.add(U[t], G.mul(B[t], table[t]))
    c = [G.mul(2 * r, x) for x in group_dft(G, U, lr + 1, inverse=True)]  # the unscaled inverse
    h = c[r:]
    assert h[r - 1] == G.zero  # slot 2r - 1: no term reaches it
    return group_dft(G, h, lr)


def fold_cosets_pair_logs(commit_logs, zs, value_rows, wit_logs, rhos, tau: int, log_l: int):
    """(log C, log W) of the fold: C = sum rho_k (C_k + z_k^l W_k) - sum_i P_i [tau^i]G with
    P_i = sum_k rho_k z_k^-i c_(k,i), W = sum rho_k W_k."""
    l = 1 << log_l
    p = [0] * l
    for z, row, rho in zip(zs, value_rows, rhos):
        for i, c in enumerate(coset_interpolant(row, z, log_l)):
            p[i] = (p[i] + rho * c) % R
    c = sum(rho * (ck + pow(z, l, R) * wk) for ck, z, wk, rho in zip(commit_logs, zs, wit_logs, rhos))
    c = (c - P.poly_eval(p, tau)) % R
    w = sum(rho * wk for wk, rho in zip(wit_logs, rhos)) % R
    return c, w
