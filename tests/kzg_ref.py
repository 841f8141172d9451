"""Python-integer model of the KZG openings (include/plk.h "KZG openings").

Three independent statements of the witness of f at z = omega^i on an SRS s_m = [tau^m]G:
  * the definition: pi_i = [q_i(tau)]G with q_i = (f - f(z)) / (X - z) from a plain Ruffini loop
    (witness_logs);
  * the closed form [(f(tau) - f(z)) / (tau - z)]G where tau != z (witness_log_closed);
  * the Feist-Khovratovich pipeline of csrc/kzg.hip (fk_open_domain): the reversed, identity-padded
    SRS a, the zero-padded coefficients b, A = DFT_2n(a), B = DFT_2n(b), U_t = [B_t] A_t,
    c = IDFT_2n(U), h = c[n, 2n), pi = DFT_n(h) — over any group given as (zero, add, mul), so it
    runs both in the exponent (integers mod r, every point replaced by its discrete log) and on
    real points (oracle/pyref.py's jac_* arithmetic).
A fixed-base multiplication table makes [k]G cheap enough for the GPU tests' references.
"""
import pyref as P

R = P.R_MOD


# ------------------------------------------------------------------------------- groups
class ExpGroup:
    """G1 in the exponent: a point is its discrete log mod r."""
    zero = 0

    @staticmethod
    def add(a, b):
        return (a + b) % R

    @staticmethod
    def mul(s, a):
        return s * a % R


class PointGroup:
    """G1 itself: affine pairs, None for the identity."""
    zero = None

    @staticmethod
    def add(a, b):
        return P.g1_add(a, b)

    @staticmethod
    def mul(s, a):
        s %= R
        if s == 1:
            return a
        if s == R - 1:
            return P.g1_neg(a)
        return P.g1_mul(a, s)


def group_dft(G, xs, k: int, inverse: bool = False):
    """out_i = sum_j w^(+-ij) xs_j over the 2^k domain from the definition (O(n^2)), natural
    order; the inverse carries n^-1."""
    n = 1 << k
    assert len(xs) == n
    w = P.omega(k)
    if inverse:
        w = pow(w, -1, R)
    scale = pow(n, -1, R) if inverse else 1
    out = []
    for i in range(n):
        acc = G.zero
        for j in range(n):
            acc = G.add(acc, G.mul(pow(w, i * j, R) * scale % R, xs[j]))
        out.append(acc)
    return out


def group_fft(G, xs, k: int, inverse: bool = False):
    """The same transform by recursive decimation in time (n log n multiplications): what the
    pipeline on real points uses; test_kzg_ref_cpu.py holds it to group_dft in the exponent."""
    w = P.omega(k)
    if inverse:
        w = pow(w, -1, R)

    def rec(a, w):
        if len(a) == 1:
            return a[:]
        even, odd = rec(a[0::2], w * w % R), rec(a[1::2], w * w % R)
        h, t, out = len(a) // 2, 1, [G.zero] * len(a)
        for i in range(h):
            x = G.mul(t, odd[i])
            out[i] = G.add(even[i], x)
            out[i + h] = G.add(even[i], G.mul(R - 1, x))
            t = t * w % R
        return out

    out = rec(list(xs), w)
    if inverse:
        ninv = pow(1 << k, -1, R)
        out = [G.mul(ninv, x) for x in out]
    return out


# ------------------------------------------------------------------------------ witnesses
def witness_logs(f, tau: int, k: int):
    """The definition: log of pi_i = q_i(tau) mod r for every i < 2^k."""
    n, w = 1 << k, P.omega(k)
    f = list(f) + [0] * (n - len(f))
    return [P.poly_eval(P.ruffini(f, pow(w, i, R)), tau) for i in range(n)]


def witness_log_closed(f, tau: int, z: int):
    """(f(tau) - f(z)) / (tau - z) mod r; tau != z."""
    assert (tau - z) % R
    return (P.poly_eval(f, tau) - P.poly_eval(f, z)) * pow(tau - z, -1, R) % R


def fk_open_domain(G, srs, f, k: int, group_dft=group_dft):
    """The pipeline of csrc/kzg.hip over the group G; srs: at least n elements of G, s_m."""
    n = 1 << k
    assert len(f) <= n <= len(srs)
    a = [srs[n - 1 - i] for i in range(n)] + [G.zero] * n
    b = list(f) + [0] * (2 * n - len(f))
    A = group_dft(G, a, k + 1)
    B = P.dft(b, k + 1)
    U = [G.mul(B[t], A[t]) for t in range(2 * n)]
    c = group_dft(G, U, k + 1, inverse=True)
    h = c[n:]
    assert h[n - 1] == G.zero  # slot 2n - 1: no term reaches it
    return group_dft(G, h, k)


def fold_pair_logs(commit_logs, zs, ys, wit_logs, rhos):
    """(log C, log W) of the fold: C = sum rho (C_k - y_k G + z_k W_k), W = sum rho W_k."""
    c = sum(r * (ck - y + z * wk) for ck, z, y, wk, r in zip(commit_logs, zs, ys, wit_logs, rhos)) % R
    w = sum(r * wk for wk, r in zip(wit_logs, rhos)) % R
    return c, w


# ----------------------------------------------------------------- fixed-base multiplication
_WIN = 8
_TABLE = None  # _TABLE[w][d - 1] = [d 2^(8 w)]G, Jacobian


def _table():
    global _TABLE
    if _TABLE is None:
        tab, base = [], P.jac_from_affine(P.G1_GEN)
        for _ in range((P.FR_BITS + _WIN - 1) // _WIN):
            row, acc = [], (1, 1, 0)
            for _ in range((1 << _WIN) - 1):
                acc = P.jac_add(acc, base)
                row.append(acc)
            tab.append(row)
            base = P.jac_add(row[-1], base)  # 2^8 * base
        _TABLE = tab
    return _TABLE


def _batch_affine(jacs):
    """Jacobian points -> affine / None with one inversion (Montgomery's trick)."""
    p = P.P_MOD
    pref, acc = [], 1
    for (_, _, z) in jacs:
        if z % p:
            acc = acc * z % p
        pref.append(acc)
    inv = pow(acc, p - 2, p)
    out = [None] * len(jacs)
    for i in range(len(jacs) - 1, -1, -1):
        x, y, z = jacs[i]
        if z % p == 0:
            continue
        prev = pref[i - 1] if i else 1
        zi = inv * prev % p
        inv = inv * z % p
        zi2 = zi * zi % p
        out[i] = (x * zi2 % p, y * zi2 * zi % p)
    return out


def gen_mul_many(scalars):
    """[k]G for every k (reduced mod r): affine pairs, None for the identity."""
    tab = _table()
    jacs = []
    for s in scalars:
        s %= R
        acc, w = (1, 1, 0), 0
        while s:
            d = s & ((1 << _WIN) - 1)
            if d:
                acc = P.jac_add(acc, tab[w][d - 1])
            s >>= _WIN
            w += 1
        jacs.append(acc)
    return _batch_affine(jacs)


def gen_mul_np(scalars):
    """The same as ABI rows uint64[n, 13]."""
    return P.g1_vec_to_np(gen_mul_many(scalars))
