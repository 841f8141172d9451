"""The redundant-limb field of the hot loops (csrc/ffr.hpp: Fp 13 x 30, Fr 9 x 29) through
plk_debug_rx_op, against Python integers (tests/rx_ref.py), at the operands where the
hand-derived bounds are tight: rows whose lower limbs are all 2^B - 1 (the only ones that push an
unsplit 64-bit column of rx_mul_add past 2^64), the value bounds k p and k p +- 1, and the
unnormalised multiplicands the NTT feeds the Fr products. Every product form (plain, interleaved
group, inline-asm columns) is compared limb for limb with the one exact Montgomery result."""
import numpy as np
import pytest

import rx_ref as R

FIELD_NAMES = ("fp", "fr")
# op -> the products' operands as indices into the call's rows (a, b, c, d): one entry per
# output, each a list of (x, y) factors summed
PRODUCT_OPS = {
    "mul": [[(0, 1)]],
    "sqr": [[(0, 0)]],
    "mul_add": [[(0, 1), (2, 3)]],
    "mul2": [[(0, 1)], [(2, 3)]],
    "mul2_asm": [[(0, 1)], [(2, 3)]],
    "sqr2": [[(0, 0)], [(1, 1)]],
    "sqr2_asm": [[(0, 0)], [(1, 1)]],
    "mul_add_mul2": [[(0, 1), (2, 3)], [(0, 3)], [(2, 1)]],
    "mul_add_mul2_asm": [[(0, 1), (2, 3)], [(0, 3)], [(2, 1)]],
    "mul3": [[(0, 1)], [(2, 3)], [(3, 0)]],
}
ASM_OPS = {"fp": ("mul2_asm", "sqr2_asm", "mul_add_mul2_asm"), "fr": ("mul2_asm",)}
ARITY = {"mul": 2, "sqr": 1, "sqr2": 2, "sqr2_asm": 2}  # every other product op takes 4 rows
SUB_CP = {"fp": (3, 4, 5, 6, 10), "fr": (3, 5, 6)}


def product_cases():
    return [(field, op) for field in FIELD_NAMES for op in PRODUCT_OPS
            if not (op.endswith("_asm") and op not in ASM_OPS[field])]


def operand_columns(field: str, op: str, kind: str) -> list:
    """The operand rows of one product op, one list per operand: edges crossed (every edge row
    with every edge row for one or two operands, the core rows for four), or the random rows
    against shuffles of themselves."""
    n = ARITY.get(op, 4)
    if kind == "random":
        rows = R.random_rows(field)
        return [list(rows)] + [R.shuffled(rows, 100 + k) for k in range(1, n)]
    if n == 1:
        return [list(R.edge_rows(field))]
    return R.cross(R.edge_rows(field) if n == 2 else R.core_rows(field), n)


def as_np(rows) -> np.ndarray:
    return np.array(rows, dtype=np.uint32)


def check_products(F, op, cols, out):
    """Exact limbs of every output; the documented range [0, 2p) wherever the operand product
    is inside the contract (N < (R' / p) p^2). Operand limbs are inside RxPlan's bound in all
    rows, so the exact comparison holds past the value bound too."""
    vals = [[F.value(r) for r in col] for col in cols]
    got = out.tolist()
    for j, terms in enumerate(PRODUCT_OPS[op]):
        for i in range(len(cols[0])):
            n = sum(vals[x][i] * vals[y][i] for x, y in terms)
            t = F.mont(n)
            exp = list(F.limbs(t))
            assert got[i][j] == exp, (
                f"{F.name} {op} output {j} row {i}: operands {[cols[k][i] for k in range(len(cols))]}"
                f" gave {got[i][j]}, expected {exp}")
            if n < F.prod_bound:
                assert t < 2 * F.p


# ------------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_reference_agrees_with_modular_arithmetic(field):
    F = R.FIELDS[field]
    p, rinv = F.p, pow(F.Rp, -1, F.p)
    rows = R.edge_rows(field) + R.random_rows(field)
    prev = rows[-1]
    for row in rows:
        v, w = F.value(row), F.value(prev)
        assert F.limbs(v) == row and F.value(F.limbs(v)) == v
        for n in (v * w, v * v, v * w + w * w):
            t = F.mont(n)
            assert t % p == n * rinv % p and t * F.Rp - n == ((n * F.ninv) % F.Rp) * p
            assert t < n // F.Rp + p + 1
        prev = row
    for a, b, c, d in zip(*R.cross(R.core_rows(field), 4)):
        n = F.value(a) * F.value(b) + F.value(c) * F.value(d)
        assert F.mont(n) % p == n * rinv % p


def test_operands_overflow_an_unsplit_mul_add_column():
    """The set holds rows for which ONE 64-bit accumulator per column of rx_mul_add (a plan that
    splits nothing) would pass 2^64; random rows never do."""
    F = R.FP
    cols = R.cross(R.core_rows("fp"), 4)
    over = [q for q in zip(*cols) if R.unsplit_mul_add_max_column(F, *q) >= 1 << 64]
    assert len(over) >= 100
    ml = R.max_limb_rows(F)
    assert R.unsplit_mul_add_max_column(F, ml[5], ml[5], ml[5], ml[5]) >= 1 << 64
    assert (ml[5],) * 4 in set(zip(*cols))
    rnd = operand_columns("fp", "mul_add", "random")
    assert max(R.unsplit_mul_add_max_column(F, *q) for q in list(zip(*rnd))[:1500]) < 1 << 64


def test_fr_columns_stay_below_2_64_on_the_documented_operands():
    """Fr keeps one accumulator per column: the NTT's unnormalised multiplicands at their
    documented limb bounds, against a max-limb second factor, stay below 2^64."""
    F = R.FR
    big, small = R.fr_unnormalised_rows()
    zero = (0,) * F.L
    worst = max(R.unsplit_mul_add_max_column(F, a, b, zero, zero)
                for a in big + small for b in R.fr_max_limb_seconds())
    assert worst < 1 << 64


@pytest.mark.parametrize("field,op", [(f, op) for f in FIELD_NAMES for op in ASM_OPS[f]])
def test_asm_forms_see_max_limbs_in_every_position(field, op):
    """Some case of each inline-asm form holds 2^B - 1 in every lower limb of every operand, so
    every mad of every column statement multiplies two maximal operands."""
    F = R.FIELDS[field]
    cols = operand_columns(field, op, "edges")
    full = [all(all(v == F.mask for v in col[i][:-1]) for col in cols) for i in range(len(cols[0]))]
    assert any(full)
    tops = {tuple(col[i][-1] for col in cols) for i in range(len(full)) if full[i]}
    assert ((1 << R.TOP_BITS) - 1,) * len(cols) in tops


@pytest.mark.parametrize("field", FIELD_NAMES)
def test_operand_classes(field):
    F = R.FIELDS[field]
    p = F.p
    vals = {F.value(r) for r in R.edge_rows(field)}
    for k in range(1, F.kmax + 1):
        assert {k * p - 1, k * p, k * p + 1} <= vals
    assert {0, 1, p - 1, p + 1, 2 * p - 1, 2 * p} <= vals
    # Fp: inside RxPlan's limb bound; Fr (no split plan): up to the 21r + 1 of the value edges
    top = 1 << R.TOP_BITS if field == "fp" else F.top_of(21 * p + 1) + 1
    assert all(F.normalised(r) and r[-1] < top for r in R.edge_rows(field))
    rnd = [F.value(r) for r in R.random_rows(field)]
    assert len(rnd) == 6000 and max(rnd[:2000]) < 2 * p and max(rnd[2000:4000]) < 8 * p
    assert 8 * p < max(rnd[4000:]) < 12 * p
    if field == "fr":
        big, small = R.fr_unnormalised_rows()
        assert max(max(r) for r in big) == int(2 ** 31.6) - 1
        assert all(F.value(r) < 21 * p for r in big)
        assert max(max(r) for r in small) < (1 << 29) + (1 << 30)
        assert all(p < F.value(r) < 5 * p for r in small)


def test_hooks_reject_bad_arguments_without_gpu(plk):
    lib = plk.plonk._lib()
    assert lib.plk_debug_rx_op(None, 1, 0, None, None, None, None, None, 0) == plk.PLK_E_ARG
    assert lib.plk_debug_g1r_op(None, 0, None, None, None, None, 0) == plk.PLK_E_ARG
    assert lib.plk_debug_ntt_lazy_op(None, 0, None, None, 0) == plk.PLK_E_ARG


# ------------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["edges", "random"])
@pytest.mark.parametrize("field,op", product_cases())
def test_products(gpu_ctx, field, op, kind):
    F = R.FIELDS[field]
    cols = operand_columns(field, op, kind)
    out = gpu_ctx.rx_op(field, op, *[as_np(c) for c in cols])
    check_products(F, op, cols, out)


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_canon(gpu_ctx, field):
    """rx_canon = rx_mul(a, R' mod p): exact limbs, [0, 2p), the same residue."""
    F = R.FIELDS[field]
    rows = R.edge_rows(field) + R.random_rows(field)
    got = gpu_ctx.rx_op(field, "canon", as_np(rows))[:, 0].tolist()
    for row, g in zip(rows, got):
        v = F.value(row)
        t = F.mont(v * F.one)
        assert g == list(F.limbs(t)), (row, g)
        assert t % F.p == v % F.p
        if v * F.one < F.prod_bound:
            assert t < 2 * F.p


@pytest.mark.gpu
def test_fr_unnormalised_multiplicands(gpu_ctx):
    """rx_mul and the NTT's twmul2 (rx_mul2<FrCfg, true>) on unnormalised first factors at their
    documented bounds, the other factor normalised below 2r."""
    F = R.FR
    r = F.p
    big, small = R.fr_unnormalised_rows()
    firsts = list(big + small)
    seconds = [F.limbs(v) for v in (0, 1, r - 1, r, r + 1, 2 * r - 1)]
    seconds += list(R.fr_max_limb_seconds())
    seconds += list(R.random_rows("fr")[:8])
    a, b = R.cross(firsts, 1)[0] * len(seconds), [s for s in seconds for _ in firsts]
    assert all(F.value(x) * F.value(y) < F.prod_bound for x, y in zip(a, b))
    check_products(F, "mul", [a, b], gpu_ctx.rx_op("fr", "mul", as_np(a), as_np(b)))
    c, d = a[::-1], b[::-1]
    check_products(F, "mul2_asm", [a, b, c, d],
                   gpu_ctx.rx_op("fr", "mul2_asm", as_np(a), as_np(b), as_np(c), as_np(d)))
    # the permutation argument's rx_mul_add(rx_sub_u<FrCfg, 3>(..), alpha, ..): one unnormalised
    # first factor, the other three normalised below 2r
    a, b = list(small) * len(seconds), [s for s in seconds for _ in small]
    c, d = b[::-1], R.shuffled(b, 5)
    check_products(F, "mul_add", [a, b, c, d],
                   gpu_ctx.rx_op("fr", "mul_add", as_np(a), as_np(b), as_np(c), as_np(d)))


def below(F, rows, k):
    return [r for r in rows if F.value(r) < k * F.p]


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_add_sub(gpu_ctx, field):
    """rx_add, rx_sub: [0, 2p) x [0, 2p) -> [0, 2p); rx_sub_lazy: a - b + 2p, normalised."""
    F = R.FIELDS[field]
    p = F.p
    rows = below(F, R.edge_rows(field), 2)
    a, b = R.cross(rows, 2)
    rnd = R.random_rows(field)[:2000]
    a, b = a + list(rnd), b + R.shuffled(rnd, 7)
    A, Bn = as_np(a), as_np(b)
    va, vb = [F.value(x) for x in a], [F.value(x) for x in b]
    exp = {"add": [x + y - (2 * p if x + y >= 2 * p else 0) for x, y in zip(va, vb)],
           "sub": [x - y + (2 * p if x < y else 0) for x, y in zip(va, vb)],
           "sub_lazy": [x - y + 2 * p for x, y in zip(va, vb)]}
    for op, e in exp.items():
        got = gpu_ctx.rx_op(field, op, A, Bn)[:, 0].tolist()
        assert got == [list(F.limbs(v)) for v in e], op
        assert all(0 <= v < (4 if op == "sub_lazy" else 2) * p for v in e)


@pytest.mark.gpu
@pytest.mark.parametrize("field,cp", [(f, cp) for f in FIELD_NAMES for cp in SUB_CP[f]])
def test_sub_u_sub_n(gpu_ctx, field, cp):
    """a + cp p - b. rx_sub_n (and rx_sub_u of the split shape, Fp): signed carries, exact
    normalised limbs for every normalised pair with a non-negative result. rx_sub_u of Fr: limb by
    limb without carries for a < 2p and b < (cp - 1) p: the exact value, limbs below 2^(B + 2),
    value below (cp + 2) p."""
    F = R.FIELDS[field]
    p = F.p
    rows = R.edge_rows(field)
    rnd = R.random_rows(field)
    pairs = [(a, b) for a, b in zip(*R.cross(rows, 2))] + list(zip(rnd, R.shuffled(rnd, 9)))
    pairs = [(a, b) for a, b in pairs if F.value(a) + cp * p - F.value(b) >= 0]
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    exp = [F.value(x) + cp * p - F.value(y) for x, y in pairs]
    got = gpu_ctx.rx_op(field, "sub_n", as_np(a), as_np(b), cp=cp)[:, 0].tolist()
    assert got == [list(F.limbs(v)) for v in exp]
    if field == "fp":
        got = gpu_ctx.rx_op(field, "sub_u", as_np(a), as_np(b), cp=cp)[:, 0].tolist()
        assert got == [list(F.limbs(v)) for v in exp]
        return
    keep = [i for i, (x, y) in enumerate(pairs) if F.value(x) < 2 * p and F.value(y) < (cp - 1) * p]
    assert len(keep) > 1000
    a, b = [a[i] for i in keep], [b[i] for i in keep]
    got = gpu_ctx.rx_op(field, "sub_u", as_np(a), as_np(b), cp=cp)[:, 0].tolist()
    for g, i in zip(got, keep):
        assert F.value(g) == exp[i] and exp[i] < (cp + 2) * p
        assert max(g) < 1 << (F.B + 2)


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_sub2_n_and_small_mul(gpu_ctx, field):
    """rx_sub2_n<6>: a + 6p - b - 2e in one signed-carry pass (the X3 of the additions: a, b, e
    below 2p; also any normalised triple with a non-negative result); rx_small_mul_n<2>, <3>."""
    F = R.FIELDS[field]
    p = F.p
    rows = list(dict.fromkeys(R.core_rows(field) + tuple(below(F, R.edge_rows(field), 2))))[:24]
    tri = list(zip(*R.cross(rows, 3)))
    rnd = R.random_rows(field)[:2000]
    tri += list(zip(rnd, R.shuffled(rnd, 3), R.shuffled(rnd, 4)))
    tri = [t for t in tri if F.value(t[0]) + 6 * p - F.value(t[1]) - 2 * F.value(t[2]) >= 0]
    assert len(tri) > 3000
    exp = [F.value(a) + 6 * p - F.value(b) - 2 * F.value(e) for a, b, e in tri]
    got = gpu_ctx.rx_op(field, "sub2_n6", *[as_np([t[k] for t in tri]) for k in range(3)])
    assert got[:, 0].tolist() == [list(F.limbs(v)) for v in exp]
    assert all(0 < v < 8 * p for v, t in zip(exp, tri) if all(F.value(x) < 2 * p for x in t))
    rows = R.edge_rows(field) + R.random_rows(field)
    for k, op in ((2, "small_mul2"), (3, "small_mul3")):
        got = gpu_ctx.rx_op(field, op, as_np(rows))[:, 0].tolist()
        assert got == [list(F.limbs(k * F.value(r))) for r in rows], op


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_zero_tests(gpu_ctx, field):
    """rx_is_zero is true on exactly {0, p}; rx_is_zero_u on every multiple k p below 12p and on
    none of k p +- 1."""
    F = R.FIELDS[field]
    p = F.p
    rows = R.edge_rows(field) + R.random_rows(field)
    got = gpu_ctx.rx_op(field, "is_zero", as_np(rows))[:, 0]
    assert not got[:, 1:].any()
    assert got[:, 0].tolist() == [int(F.value(r) in (0, p)) for r in rows]
    assert sum(got[:, 0].tolist()) == 2
    rows = [r for r in rows if F.value(r) <= 12 * p + 1]
    got = gpu_ctx.rx_op(field, "is_zero_u", as_np(rows))[:, 0]
    assert not got[:, 1:].any()
    assert got[:, 0].tolist() == [int(F.value(r) % p == 0) for r in rows]
    vals = {F.value(r): g for r, g in zip(rows, got[:, 0].tolist())}
    for k in range(12):
        assert vals[k * p] == 1
        assert vals[k * p + 1] == 0 and (k == 0 or vals[k * p - 1] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_unpack_pack(gpu_ctx, field):
    """rx_unpack of a packed N-word value gives its normalised limbs (the top limb takes the
    rest) and rx_pack gives the words back."""
    F = R.FIELDS[field]
    bits = 32 * F.N
    vals = [F.value(r) for r in R.edge_rows(field) + R.random_rows(field)[:1000]]
    vals += [(1 << bits) - 1, 1 << (bits - 1), (1 << bits) - (1 << 31)]
    vals += [(1 << (32 * j)) - 1 for j in range(1, F.N)] + [1 << (32 * j) for j in range(1, F.N)]
    vals = [v for v in vals if v < 1 << bits]
    words = np.zeros((len(vals), F.L), dtype=np.uint32)
    for i, v in enumerate(vals):
        words[i, :F.N] = [(v >> (32 * k)) & 0xFFFFFFFF for k in range(F.N)]
    got = gpu_ctx.rx_op(field, "unpack_pack", words)
    assert got[:, 0].tolist() == [list(F.limbs(v)) for v in vals]
    assert (got[:, 1] == words).all()
