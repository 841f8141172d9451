"""Integer model of the fixed-base MSM pipeline (csrc/msm.hip, msm_sort.hip, msm_acc.hip, msm_reduce.hip), stage by stage,
for the snapshots of plk_debug_msm_snapshot (tests/test_msm_stage_gpu.py) and its own CPU test
(tests/test_msm_stage_ref_cpu.py).

What each stage leaves, as the model states it (h: the snapshot header):

  recoding   every scalar s goes to h' = min(s, r - s) (sign flipped for r - s), then to W signed
             digits over the windows of pyref.msm_window_layout(c); the final carry is 0. A digit
             d != 0 of scalar i in window w is the entry  code = w n_srs + i | sign << 31  of
             bucket |d| - 1 - b_lo (kept when it falls in [0, B): a part keeps its range only).
  offsets    offsets[b] = entries of the buckets below b; offsets[B] = the slot's entry count.
  sorted     sorted[offsets[b] .. offsets[b+1]) = bucket b's codes, in any order.
  tasks      task_off[b] = tasks of the buckets below b, ceil(count / chunk) per bucket. Bucket b's
             tasks tile its entry range in pieces of `chunk` with one shorter tail; piece t writes
             partial task_off[b] + t; record = {first entry, partial | (length - 1) << 26}. Record
             order: full tasks in bucket order, then the tails grouped by length, longest first.
  partials   partials[p] = the sum of its task's table points, added in the order of `sorted`.
             The table point of a code is +-2^(o_w - s_w) P_i (o_w the window's bit offset, s_w = 1
             for a narrow window whose digits come doubled).
  bsum       narrow sets: bsum[b] = S_b, the sum of bucket b's partials.
  rsum ys zs wide sets, runs of K = 2^rb buckets: rsum[rK + t] = R_(r,t) = sum_(t' >= t) S_(rK+t'),
             taken partial by partial from the run's top bucket down; ys[r] = Y_r = R_(r,0);
             zs[r] = T_r = sum_t R_(r,t), the infinite R_(r,t) skipped.
  bit sums   over the values v_x (x < 256 G: S_b narrow, Y_r wide): T_j = sum of v_x over x with
             bit j set, T_0 also + sum_x v_x; wide sets add T_nbits = sum_r T_r, T_(nbits+1) =
             sum_r Y_r.
  host tail  acc = part * T_(nbits+1) (wide parts), Horner over T_(nbits-1) .. T_0; wide sets then
             (acc - sum_r Y_r) 2^rb + sum_r T_r.

The derived values (B, chunk, rb, NR, ...) are the header's: the model holds no copy of the host's
sizing rules. Group elements are discrete logarithms: every SRS the tests use is made of known
multiples q_i of the generator G (a tau, or chosen points), G1 has prime order r, so the integers
mod r with 0 for the identity ARE the group, exceptional cases included (equal operands: equal
residues; opposite: residues summing to 0). A residue k meets the device's XYZZ row as the curve
point k G (FixedBase, pyref's Jacobian law), compared cross-multiplied, without an inversion.

While it adds, the model tallies per stage the exceptional additions it meets (Tally).
"""
from __future__ import annotations

import collections
import functools

import numpy as np

import pyref as P
import rx_ref

R = P.R_MOD
HALF = (R - 1) // 2
TASK_SHIFT = 26            # msm_common.hpp kTaskShift, task_record() (kChunkMax <= 64)
SIGN = 0x80000000
INV2 = pow(2, -1, R)

# header words of plk_debug_msm_snapshot (include/plk.h), in order
HDR_FIELDS = ("B", "W", "narrow", "c", "chunk", "rb", "fb", "NC", "NR", "G", "nbits", "nout",
              "wide", "sort_one", "hold", "task_stride", "sorted_stride", "max_tasks_used",
              "b_lo", "n_srs", "gen", "part", "parts", "has_inf")
EVENTS = ("equal", "opposite", "operand_inf", "acc_inf", "result_inf")


def header(**kw) -> dict:
    """A header for the CPU chain (no device): the caller chooses chunk and rb, the rest follows
    from c as msm_run_batch derives it for a whole MSM (parts = 1)."""
    c = P.msm_effective_c(kw["c"])
    lay = P.msm_window_layout(c)
    B = (1 << (c - 1)) // kw.get("parts", 1)
    wide = int((1 << (c - 1)) > 32768)
    rb = kw.get("rb", 4)
    NR = B >> rb
    vals = B if not wide else NR
    G = (vals + 255) // 256
    nbits = 8 + G.bit_length() - 1
    h = dict(B=B, W=len(lay), narrow=sum(s for _, _, s in lay), c=c, chunk=kw.get("chunk", 8),
             rb=rb, fb=10, NC=B >> 10, NR=NR, G=G, nbits=nbits, nout=nbits + (2 if wide else 0),
             wide=wide, sort_one=0, hold=0, task_stride=0, sorted_stride=0, max_tasks_used=1 << 30,
             b_lo=kw.get("part", 0) * B, n_srs=kw["n_srs"], gen=1, part=kw.get("part", 0),
             parts=kw.get("parts", 1), has_inf=0)
    assert G & (G - 1) == 0
    return h


# ---------------------------------------------------------------------------------- recoding
def scalar_half(s: int):
    s %= R
    neg = s > HALF
    return (R - s if neg else s), neg


def layout_of(h: dict):
    lay = P.msm_window_layout(h["c"])
    assert len(lay) == h["W"] and sum(s for _, _, s in lay) == h["narrow"], (lay, h)
    return lay


def recode(s: int, lay):
    """[(w, d)] of scalar s, d the bucket-scale digit (narrow windows doubled), and the sign flip."""
    hs, neg = scalar_half(s)
    out, carry = [], 0
    for w, (o, cw, sh) in enumerate(lay):
        d = ((hs >> o) & ((1 << cw) - 1)) + carry
        carry = 1 if d > (1 << (cw - 1)) else 0
        if carry:
            d -= 1 << cw
        out.append((w, d << sh))
    assert carry == 0, hex(s)
    return out, neg


def rebuild(digits, neg, lay) -> int:
    """The scalar a recoding stands for: sum_w d_w 2^(o_w - s_w), negated for a flipped one."""
    v = sum(d * (1 << o) // (1 << sh) for (w, d), (o, cw, sh) in zip(digits, lay))
    assert all(d % (1 << sh) == 0 for (w, d), (o, cw, sh) in zip(digits, lay))
    return (-v if neg else v) % R


def entries_of(scalars, h: dict):
    """[(bucket, code)] of a slot's scalars, in scalar then window order."""
    lay, n, lo, B = layout_of(h), h["n_srs"], h["b_lo"], h["B"]
    out = []
    for i, s in enumerate(scalars):
        digits, neg = recode(s, lay)
        for w, d in digits:
            b = abs(d) - 1 - lo
            if d != 0 and 0 <= b < B:
                out.append((b, (w * n + i) | (SIGN if (d < 0) != neg else 0)))
    return out


def check_sorted(entries, offsets, sorted_codes, B: int) -> int:
    """offsets are the scan of the expected bucket counts, and each bucket's range of `sorted`
    holds the bucket's multiset of codes (both sides ordered by bucket, then code). `entries`:
    entries_of's list. Returns the entry count."""
    eb = np.array([b for b, _ in entries], dtype=np.int64)
    ec = np.array([c for _, c in entries], dtype=np.int64)
    want = np.concatenate([[0], np.cumsum(np.bincount(eb, minlength=B))]).astype(np.int64)
    assert np.array_equal(np.asarray(offsets, dtype=np.int64), want), "offsets"
    n = int(want[B])
    got = np.asarray(sorted_codes, dtype=np.int64)
    assert len(got) == n, (len(got), n)
    gb = np.repeat(np.arange(B, dtype=np.int64), want[1:] - want[:-1])
    ge, gg = np.lexsort((ec, eb)), np.lexsort((got, gb))
    bad = np.nonzero(ec[ge] != got[gg])[0]
    assert len(bad) == 0, f"bucket {int(eb[ge][bad[0]])}: holds {int(got[gg][bad[0]]):#x}, wants {int(ec[ge][bad[0]]):#x}"
    return n


def unpack_tasks(tasks):
    t = np.asarray(tasks, dtype=np.uint32).reshape(-1, 2)
    first = t[:, 0].astype(np.int64)
    length = (t[:, 1] >> TASK_SHIFT).astype(np.int64) + 1
    pidx = (t[:, 1] & ((1 << TASK_SHIFT) - 1)).astype(np.int64)
    return first, length, pidx


def check_tasks(h: dict, offsets, task_off, tasks):
    """The task rules and the record order. Returns (first, length, pidx) per record."""
    B, chunk = h["B"], h["chunk"]
    off = np.asarray(offsets, dtype=np.int64)
    toff = np.asarray(task_off, dtype=np.int64)
    cnt = off[1:] - off[:-1]
    assert toff[0] == 0
    assert np.array_equal(toff[1:] - toff[:-1], (cnt + chunk - 1) // chunk), "task_off"
    n = int(toff[B])
    assert n <= h["max_tasks_used"], (n, h["max_tasks_used"])
    first, length, pidx = unpack_tasks(tasks)
    assert len(first) == n, (len(first), n)
    if n == 0:
        return first, length, pidx
    assert length.min() >= 1 and length.max() <= chunk
    # the bucket of a task: the last one whose range starts at or below its first entry and is
    # not empty (first < offsets[b + 1])
    b = np.searchsorted(off, first, side="right") - 1
    assert (b >= 0).all() and (b < B).all()
    rel = first - off[b]
    assert (rel % chunk == 0).all(), "a task starts off a chunk boundary of its bucket"
    piece = rel // chunk
    assert np.array_equal(pidx, toff[b] + piece), "partial index"
    assert (first + length <= off[b + 1]).all(), "a task runs past its bucket"
    # every entry once: the pieces of a bucket are distinct, lengths chunk but for the tail
    assert len(np.unique(pidx)) == n and pidx.min() == 0 and pidx.max() == n - 1
    last = piece == (cnt[b] - 1) // chunk
    assert (length[~last] == chunk).all(), "a piece before the tail is short"
    assert np.array_equal(length[last], (cnt[b] - piece * chunk)[last]), "tail length"
    assert int(length.sum()) == int(off[B]), "entries covered"
    # record order: full tasks in bucket order, then tails by length, longest first
    nfull = int((cnt // chunk).sum())
    assert (length[:nfull] == chunk).all() and (np.diff(first[:nfull]) > 0).all(), "full tasks"
    tails = length[nfull:]
    assert (tails < chunk).all() and (np.diff(tails) <= 0).all(), "tails: longest first"
    return first, length, pidx


def build_device_layout(scalars, h: dict):
    """A legal device layout for the CPU chain: (offsets, sorted, task_off, tasks)."""
    B, chunk = h["B"], h["chunk"]
    buckets = collections.defaultdict(list)
    for b, code in entries_of(scalars, h):
        buckets[b].append(code)
    off = np.zeros(B + 1, dtype=np.int64)
    toff = np.zeros(B + 1, dtype=np.int64)
    for b, cs in buckets.items():
        off[b + 1] = len(cs)
        toff[b + 1] = (len(cs) + chunk - 1) // chunk
    off, toff = np.cumsum(off), np.cumsum(toff)
    srt = np.zeros(int(off[B]), dtype=np.uint32)
    full, tails = [], []
    for b in sorted(buckets):
        cs = buckets[b][::-1]  # any order inside a bucket: here reversed
        srt[off[b]:off[b + 1]] = cs
        for t in range(0, len(cs), chunk):
            ln = min(chunk, len(cs) - t)
            rec = (int(off[b]) + t, int(toff[b]) + t // chunk | (ln - 1) << TASK_SHIFT)
            (full if ln == chunk else tails).append((ln, rec))
    tails.sort(key=lambda x: -x[0])
    tasks = np.array([r for _, r in full + tails], dtype=np.uint32).reshape(-1, 2)
    return off, srt, toff, tasks


# -------------------------------------------------------------------------------- the group
class Tally:
    """Exceptional additions met, per stage."""

    def __init__(self):
        self.n = collections.defaultdict(collections.Counter)

    def add(self, stage: str, acc: int, v: int) -> int:
        c = self.n[stage]
        c["adds"] += 1
        if v == 0:
            c["operand_inf"] += 1
        if acc == 0:
            c["acc_inf"] += 1
        if acc and v:
            if acc == v:
                c["equal"] += 1
            elif (acc + v) % R == 0:
                c["opposite"] += 1
        r = (acc + v) % R
        if r == 0:
            c["result_inf"] += 1
        return r

    def merge(self, other: "Tally"):
        for st, c in other.n.items():
            self.n[st].update(c)

    def as_dict(self):
        return {st: dict(sorted(c.items())) for st, c in sorted(self.n.items())}


def table_dlog(code: int, h: dict, lay, srs_dlog) -> int:
    """The table point of an entry code, as a multiple of G."""
    w, i = divmod(code & 0x7FFFFFFF, h["n_srs"])
    o, cw, sh = lay[w]
    m = pow(2, o, R) * (INV2 if sh else 1) % R
    v = srs_dlog[i] * m % R
    return (R - v) % R if code & SIGN else v


def model_partials(h, srs_dlog, sorted_codes, first, length, pidx, tally: Tally):
    """partials[p] in the device's entry order (k_accumulate: the first entry initialises the
    accumulator, an identity table point is skipped, the rest are mixed additions)."""
    lay = layout_of(h)
    out = [0] * len(first)
    c = tally.n["accumulate"]
    for f, ln, p in zip(first.tolist(), length.tolist(), pidx.tolist()):
        acc = table_dlog(int(sorted_codes[f]), h, lay, srs_dlog)
        if acc == 0:
            c["operand_inf"] += 1
        for e in range(f + 1, f + ln):
            v = table_dlog(int(sorted_codes[e]), h, lay, srs_dlog)
            if v == 0:  # HAS_INF: skipped, no addition
                c["operand_inf"] += 1
                continue
            acc = tally.add("accumulate", acc, v)
        if acc == 0:
            c["partial_inf"] += 1
        out[p] = acc
    return out


def model_bucket_sums(h, task_off, partials):
    """S_b, as values (k_bucket_sum's tree order is not modelled)."""
    toff = np.asarray(task_off, dtype=np.int64)
    S = {}
    for b in np.nonzero(toff[1:] > toff[:-1])[0].tolist():
        S[b] = sum(partials[toff[b]:toff[b + 1]]) % R
    return S


def model_run_sums(h, task_off, partials, tally: Tally):
    """(rsum {b: R}, ys {r: Y}, zs {r: T}) of the runs that hold a partial, in k_runsum1's and
    k_runsum2's order of additions; every other rsum / ys / zs entry is the identity."""
    K, NR = 1 << h["rb"], h["NR"]
    toff = np.asarray(task_off, dtype=np.int64)
    runs = np.nonzero(toff[K::K][:NR] > toff[0::K][:NR])[0].tolist()
    rsum, ys, zs = {}, {}, {}
    c2 = tally.n["runsum2"]
    for r in runs:
        acc, pe = 0, int(toff[r * K + K])
        for t in range(K - 1, -1, -1):
            b = r * K + t
            p0 = int(toff[b])
            if acc == 0 and p0 == pe and t == K - 1:
                tally.n["runsum1"]["top_bucket_empty"] += 1
            for p in range(p0, pe):
                acc = tally.add("runsum1", acc, partials[p])
            pe = p0
            rsum[b] = acc
        T = rsum[r * K]
        for t in range(1, K):
            v = rsum[r * K + t]
            if v == 0:
                c2["operand_inf"] += 1  # skipped, no addition
                continue
            T = tally.add("runsum2", T, v)
        ys[r], zs[r] = rsum[r * K], T
    return rsum, ys, zs


def model_bit_sums(h, values: dict, zs: dict | None):
    """T_j over the values {x: v_x} (the rest identity); wide sets: + sum of zs, sum of values."""
    T = [0] * h["nout"]
    for x, v in values.items():
        for j in range(h["nbits"]):
            if (x >> j) & 1:
                T[j] += v
        T[0] += v
    if h["wide"]:
        T[h["nbits"]] = sum(zs.values())
        T[h["nbits"] + 1] = sum(values.values())
    return [t % R for t in T]


def model_host_tail(h, T) -> int:
    nbits = h["nbits"]
    acc = h["part"] * T[nbits + 1] if h["wide"] and h["part"] else 0
    for j in range(nbits - 1, -1, -1):
        acc = 2 * acc + T[j]
    if h["wide"]:
        acc = (acc - T[nbits + 1]) * (1 << h["rb"]) + T[nbits]
    return acc % R


def model_chain(h, srs_dlog, offsets, sorted_codes, task_off, tasks, tally: Tally | None = None):
    """Every stage from a device (or build_device_layout) sort. Returns a dict of the stages."""
    tally = tally if tally is not None else Tally()
    first, length, pidx = unpack_tasks(tasks)
    partials = model_partials(h, srs_dlog, sorted_codes, first, length, pidx, tally)
    out = {"partials": partials, "tally": tally}
    if h["wide"]:
        out["rsum"], out["ys"], out["zs"] = model_run_sums(h, task_off, partials, tally)
        out["bits"] = model_bit_sums(h, out["ys"], out["zs"])
    else:
        out["bsum"] = model_bucket_sums(h, task_off, partials)
        out["bits"] = model_bit_sums(h, out["bsum"], None)
    out["final"] = model_host_tail(h, out["bits"])
    return out


def direct_dlog(h, srs_dlog, scalars) -> int:
    """The slot's result by definition: sum_i s_i q_i, a part's share of it for parts > 1."""
    if h["parts"] == 1:
        return sum(s * q for s, q in zip(scalars, srs_dlog)) % R
    lay = layout_of(h)
    return sum(table_dlog(code, h, lay, srs_dlog) * (b + h["b_lo"] + 1)
               for b, code in entries_of(scalars, h)) % R


# ------------------------------------------------------------------------ curve points, decoding
class FixedBase:
    """k -> k G in Jacobian coordinates (pyref's law), 8-bit windows over a table of multiples."""

    def __init__(self):
        self.rows = []
        base = P.jac_from_affine(P.G1_GEN)
        for _ in range(32):
            row, acc = [None], (1, 1, 0)
            for _ in range(255):
                acc = P.jac_add(acc, base)
                row.append(acc)
            self.rows.append(row)
            base = P.jac_add(acc, base)  # 256 base

    def mul(self, k: int):
        acc = (1, 1, 0)
        k %= R
        for w in range(32):
            d = (k >> (8 * w)) & 255
            if d:
                acc = P.jac_add(acc, self.rows[w][d])
        return acc


@functools.lru_cache(maxsize=None)
def fixed_base() -> FixedBase:
    return FixedBase()


@functools.lru_cache(maxsize=1 << 16)
def mul_g(k: int):
    """k G, Jacobian; cached: a run sum keeps its value over the empty buckets below it."""
    return fixed_base().mul(k)


FP = rx_ref.FP
PM = P.P_MOD
BOUND_2P = (2, 2, 2, 2)     # partials, ys, zs, bit sums: every coordinate in [0, 2p)
BOUND_LAZY = (8, 4, 2, 2)   # rsum (stored lazily), bsum (an operand of the lazy additions)


def row_ints(row):
    """X, Y, ZZ, ZZZ of a packed 48-word XYZZ row, as integers (R'-domain values, unreduced)."""
    b = np.ascontiguousarray(row, dtype=np.uint32).tobytes()
    return tuple(int.from_bytes(b[48 * i:48 * i + 48], "little") for i in range(4))


def check_row(row, k: int, bound=BOUND_2P, what=""):
    """The device row is the point k G (identity for k = 0), well formed and inside `bound`."""
    X, Y, ZZ, ZZZ = v = row_ints(row)
    for name, x, m in zip("X Y ZZ ZZZ".split(), v, bound):
        assert x < m * PM, f"{what}: {name} >= {m}p"
    if k % R == 0:
        assert ZZ in (0, PM), f"{what}: expected the identity, ZZ = {hex(ZZ)}"
        return
    assert ZZ not in (0, PM), f"{what}: identity, expected {k} G"
    assert pow(ZZ, 3, PM) == ZZZ * ZZZ * FP.Rp % PM, f"{what}: ZZ^3 != ZZZ^2"
    Xe, Ye, Ze = mul_g(k % R)
    z2 = Ze * Ze % PM
    assert X * z2 % PM == Xe * ZZ % PM, f"{what}: x differs from {k} G"
    assert Y * z2 * Ze % PM == Ye * ZZZ % PM, f"{what}: y differs from {k} G"


def rows_identity(rows) -> np.ndarray:
    """Per packed row: ZZ in {0, p}."""
    zz = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 48)[:, 24:36]
    pw = np.frombuffer(PM.to_bytes(48, "little"), dtype=np.uint32)
    return (zz == 0).all(axis=1) | (zz == pw).all(axis=1)


def check_rows_sparse(rows, want: dict, bound, what: str):
    """rows[x] is want[x] G for x in want and the identity everywhere else."""
    ident = rows_identity(rows)
    mask = np.ones(len(ident), dtype=bool)
    seen = set()  # equal rows standing for equal values are decoded once
    for x, k in want.items():
        key = (rows[x].tobytes(), k)
        if key not in seen:
            check_row(rows[x], k, bound, f"{what}[{x}]")
            seen.add(key)
        mask[x] = False
    assert ident[mask].all(), f"{what}: a row outside the model's support is not the identity"


def affine_dlog(k: int):
    """k G as a pyref affine point (None: identity)."""
    return P.jac_to_affine(fixed_base().mul(k)) if k % R else None


# ------------------------------------------------------------------------------ edge scalars
def _clamp(h: int) -> int:
    """h with its top bits cleared until it is a canonical half, h <= (r - 1) / 2."""
    while h > HALF:
        h &= ~(1 << (h.bit_length() - 1))
    return h


def edge_halves(lay) -> dict:
    """The recoding's edge patterns of a window layout, as halves h <= (r - 1) / 2 (a pattern whose
    top windows would pass (r - 1) / 2 loses its top bits)."""
    def pat(f):
        return _clamp(sum(f(w, cw) << o for w, (o, cw, sh) in enumerate(lay)))
    return {
        "last_bucket": pat(lambda w, cw: 1 << (cw - 1)),          # no carry, bucket B - 1
        "carry_each": pat(lambda w, cw: (1 << (cw - 1)) + 1),     # a carry out of every window
        # 2^(cw-1) - 1 above a window that carries: + 1 lands on the threshold, no carry
        "under_carry_even": pat(lambda w, cw: (1 << (cw - 1)) + (1 if w % 2 == 0 else -1)),
        "under_carry_odd": pat(lambda w, cw: (1 << (cw - 1)) + (1 if w % 2 == 1 else -1)),
        # all ones: val + carry = 2^cw, a zero digit that still carries, a chain to the top
        "all_ones": _clamp((1 << 255) - 1),
        "half": HALF, "zero": 0, "one": 1,
    }


def edge_scalars(lay) -> list:
    """Every edge half in both signs, h and r - h, then (r + 1) / 2 and r - 1 by name."""
    out = []
    for h in edge_halves(lay).values():
        out += [h % R, (R - h) % R]
    return out + [(R + 1) // 2, R - 1]
