"""Cases, packers, float64 oracle and derived bound of the bf16 attention kernels (csrc/attention.hip), shared by
tests/test_gpu_attention_contract.py (ctypes straight to the ABI) and tests/test_host_attention_cases.py (the generators are what they claim:
no GPU).  numpy only; nothing here goes through the library.

Routes: d64 = attn_fwd<1>, d64ps = attn_fwd<1, PS> (pre-scaled Q, scale <= 0), d128 = attn_fwd<2>, d192 = attn_fwd<3> (all four through
visrep_attention_fwd), cls = attn_fwd_cls (visrep_mhsa_cls_fwd, pre-scaled Q), wide = attn_fwd_wide (head width 512).

Inputs are float64 arrays whose values are exactly representable in bf16: q [B, Tq, H, D], k / v [Bk, Tk, H, D] (Bk = 1 when the keys are
shared).  The packers lay them out as include/visrep.h describes the ABI: Q / K row-major windows inside a wider NaN-filled buffer at a 16-byte
aligned column offset, K followed by NaN rows, V^T [H D, ldvt] with column perm16(global key) and every other column holding the largest
finite bf16 with alternating sign (the header promises only "finite"), the output as a window inside a buffer pre-filled with a NaN pattern.

Oracle: softmax(Q K^T scale) V in float64 per image (shared keys: image 0's; causal: keys t <= query position; pre-scaled Q: the exponent is
base 2 of the raw scores).

Bound, per output element.  P = the float64 softmax, A = P |V|, O = P V, u = 2^-8 (bf16 unit roundoff), L = the largest |logit log2 e| of
the case:

    |got - O|  <=  u (A + |O|)  +  2 * 2^-21 L A

First term: P enters the P.V MFMA rounded to bf16 (relative error u per key, hence u A) while the row sum adds the fp32 p, then the output is
rounded to bf16 once (u |O|).  Second term: the scores are fp32 (the pre-scaled kernels carry -reference in the accumulator: ulp(L) per MFMA
step) and v_exp_f32 is good to about an ulp, i.e. a few 2^-23 L of the exponent, in numerator and denominator.  fp32 accumulation of P.V and of
the row sum is below both.  Because bf16 rounding is relative, the bound does not depend on where a kernel keeps its softmax reference
(running maximum, deferred by up to 2^8, fixed at the first tile up to 2^100): rounding_model() restates those three schemes with exactly
these roundings and the host test holds it to the same bound.

Table sizes: EDGE_GRID 81 (72 = every (Tq, Tk) once with route / kv_shared / causal chosen for pairwise cover, + 9 single-query full batches),
CLS_GRID 24, WIDE_GRID 48, GROWTH 38, EXACT 12, REFUSALS 23."""
import itertools
from typing import NamedTuple

import numpy as np

U = 2.0 ** -8
LOG2E = 1.4426950408889634
NAN_BITS = 0x7FD5                         # a quiet bf16 NaN with a recognisable payload: fills every byte no kernel may read or write
PAD_POS, PAD_NEG = 0x7F7F, 0xFF7F         # +- the largest finite bf16: V^T columns that belong to no key
ROUTE_D = {"d64": 64, "d64ps": 64, "d128": 128, "d192": 192, "cls": 64, "wide": 512}
ROUTE_COUNTER = {"d64": "attn", "d64ps": "attn", "d128": "attn", "d192": "attn", "cls": "attn_cls", "wide": "attn_wide"}
ROUTE_SCALE = {"d64": 0.125, "d64ps": 0.0, "d128": 128 ** -0.5, "d192": 160 ** -0.5, "cls": 0.0, "wide": 512 ** -0.5}
PRESCALED = ("d64ps", "cls")
LAYOUTS = ("tight", "window", "narrow_a", "narrow_b")
C0, C1 = 5, 9                             # the two head channels the constructed cases steer scores through


class Case(NamedTuple):
    route: str
    B: int
    Tq: int
    Tk: int
    H: int
    shared: int = 0
    causal: int = 0
    kind: str = "rand"                    # rand | ones | qzero | wgrow | stair | onelane | shift | clsgap
    param: tuple = ()
    seed: int = 0

    @property
    def D(self):
        return ROUTE_D[self.route]

    @property
    def id(self):
        s = f"{self.route}-B{self.B}-Tq{self.Tq}-Tk{self.Tk}-H{self.H}"
        s += "-shared" * self.shared + "-causal" * self.causal
        return s + (f"-{self.kind}{'_'.join(str(p) for p in self.param)}" if self.kind != "rand" else "")


# ------------------------------------------------------------------------------------------------ bf16
def bf16_round(x):
    """float64 -> the nearest bf16 (ties to even), returned as float64.  Finite values only."""
    f = np.ascontiguousarray(x, dtype=np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(x))


def bf16_bits(x):
    """bf16-exact float64 -> uint16 storage (asserts exactness)."""
    f = np.ascontiguousarray(x, dtype=np.float32)
    assert np.array_equal(f.astype(np.float64), x), "not fp32-exact"
    u = f.view(np.uint32)
    assert not (u & 0xFFFF).any(), "not bf16-exact"
    return (u >> 16).astype(np.uint16)


def bf16_from_bits(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def finite_bits(b):
    return (np.asarray(b) & 0x7F80) != 0x7F80


def perm16(m):
    """Column of key m inside the V^T rows: within every aligned block of 16 keys the two middle groups of four change places
    (keys 4..7 <-> 8..11), include/visrep.h / the header comment of csrc/attention.hip."""
    m = np.asarray(m)
    blk, r = m // 16 * 16, m % 16
    g, e = r // 4, r % 4
    return blk + np.array([0, 2, 1, 3])[g] * 4 + e


def round_up(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ inputs
def exp_factor(case, scale):
    """exponent of 2 = q.k * this."""
    return 1.0 if case.route in PRESCALED else scale * LOG2E


def first_key(case):
    """The key the constructed cases put the first tile's maximum on: the CLS key for the image-aligned kernel (its initial reference)."""
    return 0 if case.route == "cls" else 3


def growth_rows(case):
    place = case.param[1]
    return {"all": list(range(case.Tq)), "wave2": [64 + 5], "tail": [case.Tq - 1]}[place]


def make_inputs(case, absent=False):
    """{"q", "k", "v": bf16-exact float64, "scale": what the ABI gets}.  absent: a wgrow case without its growth row(s)."""
    rs = np.random.RandomState(1000 + case.seed)
    B, Tq, Tk, H, D = case.B, case.Tq, case.Tk, case.H, case.D
    Bk = 1 if case.shared else B
    scale = ROUTE_SCALE[case.route]
    if case.kind == "wgrow":
        scale = float(np.float32(1.0 / LOG2E))                  # exponent of 2 = the raw score (to 2^-24)
    c = exp_factor(case, scale)
    qc = 0.125 * LOG2E if case.route in PRESCALED else 1.0      # what the folded projection puts into Q
    quiet = case.kind in ("wgrow", "stair", "onelane")          # background scores of a few hundredths: the constructed keys decide
    amp = 0.05 if quiet else 1.0
    q = rs.standard_normal((B, Tq, H, D)) * (amp if quiet else qc)
    k = rs.standard_normal((Bk, Tk, H, D)) * amp
    v = rs.standard_normal((Bk, Tk, H, D))
    if case.kind == "ones":
        v[:] = 1.0
    elif case.kind == "qzero":
        q[:] = 0.0
    elif case.kind != "rand":
        q[..., C0] = 0.0; q[..., C1] = 0.0; k[..., C0] = 0.0; k[..., C1] = 0.0
        k0 = first_key(case)
        if case.kind == "wgrow":
            g, place, tile = case.param
            q[..., C1] = 1.0
            k[:, k0, :, C1] = 2.0 / c                           # every row's first-tile maximum: 2 (+ background)
            k[:, 64 * tile + 17, :, C0] = (2.0 + g) / c
            if not absent:
                q[:, growth_rows(case), :, C0] = 1.0
        elif case.kind == "stair":
            q[..., C0] = 1.0
            for t in range(Tk // 64):
                k[:, 64 * t + 11 + (case.route == "cls"), :, C0] = t * case.param[0] / c
        elif case.kind == "onelane":
            q[..., C1] = 1.0
            k[:, k0, :, C1] = 2.0 / c
            q[:, 39, :, C0] = 1.0                               # wave 1, lane 7 of the first query tile
            k[:, 64 + 20, :, C0] = 14.0 / c
        elif case.kind == "shift":                              # every score of every row moves by param[0]: the softmax does not
            q[..., C1] = 24.0
            k[..., C1] = case.param[0] / 24.0 / c
        elif case.kind == "clsgap":
            q[..., C1] = 24.0
            k[:, 0, :, C1] = case.param[0] / 24.0 / c
        else:
            raise ValueError(case.kind)
    return {"q": bf16_round(q), "k": bf16_round(k), "v": bf16_round(v), "scale": scale}


def exponents(inp, case, b):
    """[H, Tq, Tk] float64: the exponent of 2 of every (query, key) of image b, -inf where the causal mask hides the key."""
    q, k = inp["q"][b], inp["k"][0 if case.shared else b]
    E = (q.transpose(1, 0, 2) @ k.transpose(1, 2, 0)) * exp_factor(case, inp["scale"])
    if case.causal:
        E[:, np.arange(case.Tk)[None, :] > np.arange(case.Tq)[:, None]] = -np.inf
    return E


# ------------------------------------------------------------------------------------------------ oracle, bound, rounding model
def oracle(inp, case):
    """(O, A, L): O = softmax V and A = softmax |V| as [B, Tq, H, D] float64, L = the largest finite |exponent of 2|."""
    O = np.empty_like(inp["q"]); A = np.empty_like(O); L = 0.0
    for b in range(case.B):
        E = exponents(inp, case, b)
        L = max(L, float(np.abs(E[np.isfinite(E)]).max()))
        P = np.exp2(E - E.max(-1, keepdims=True))
        P /= P.sum(-1, keepdims=True)
        vh = inp["v"][0 if case.shared else b].transpose(1, 0, 2)
        O[b] = (P @ vh).transpose(1, 0, 2)
        A[b] = (P @ np.abs(vh)).transpose(1, 0, 2)
    return O, A, L


def bound(O, A, L):
    return U * (A + np.abs(O)) + 2.0 * 2.0 ** -21 * L * A


def ratio(got, O, A, L):
    """max |got - O| / bound; inf where got is not finite."""
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - O) / np.maximum(bound(O, A, L), 1e-300)).max())


def _f32(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def key_tiles(case, b):
    """The key slices (local key indices) one image's keys are consumed in: global 64-key blocks for attn_fwd (the image starts at residue
    b Tk % 64 of its first block), whole tiles after the CLS key for attn_fwd_cls, whole tiles for attn_fwd_wide."""
    if case.route == "cls":
        return [slice(1 + 64 * t, 65 + 64 * t) for t in range((case.Tk - 1) // 64)]
    tok0 = 0 if case.shared else b * case.Tk
    edges = [0] + list(range(64 - tok0 % 64, case.Tk, 64)) + [case.Tk]
    return [slice(a, e) for a, e in zip(edges[:-1], edges[1:]) if e > a]


def rounding_model(inp, case):
    """The three reference schemes with the roundings the bound is derived from, and no other: fp32 scores, p = fp32 exp2(score - reference),
    row sum over the fp32 p, P.V over the bf16-rounded p, fp32 state, one bf16 rounding of O / l.  Reference: first tile's maximum, moved
    when a later tile's maximum exceeds it by more than 8 (attn_fwd plain and pre-scaled); the CLS score, moved likewise (attn_fwd_cls);
    fixed at the first tile's maximum unless some row of a 128-row block outgrows it by more than 100, then the true maximum (attn_fwd_wide)."""
    out = np.empty_like(inp["q"])
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(case.B):
            E = _f32(exponents(inp, case, b))
            vh = inp["v"][0 if case.shared else b].transpose(1, 0, 2)
            tiles = key_tiles(case, b)
            for h in range(case.H):
                Eh, V = E[h], vh[h]
                R = Eh.shape[0]
                if case.route == "cls":
                    m, l, o = Eh[:, 0].copy(), np.ones(R), np.repeat(V[:1], R, 0)
                else:
                    m, l, o = np.full(R, -np.inf), np.zeros(R), np.zeros((R, V.shape[1]))
                if case.route == "wide":
                    m = Eh[:, tiles[0]].max(1)
                    over = (Eh.max(1) - m) > 100.0
                    for r0 in range(0, R, 128):
                        if over[r0:r0 + 128].any():
                            m[r0:r0 + 128] = Eh[r0:r0 + 128].max(1)
                for ti, sl in enumerate(tiles):
                    mloc = Eh[:, sl].max(1)
                    if case.route == "wide":
                        m_new = m
                    elif ti == 0 and case.route != "cls":
                        m_new = mloc
                    else:
                        m_new = np.where(mloc - m > 8.0, mloc, m)
                    alpha = np.where(m_new == m, 1.0, _f32(np.exp2(_f32(m - m_new))))
                    p = _f32(np.exp2(_f32(Eh[:, sl] - m_new[:, None])))
                    l = _f32(l * alpha + _f32(p.sum(1)))
                    o = _f32(o * alpha[:, None] + bf16_round(p) @ V[sl])
                    m = m_new
                out[b, :, h] = bf16_round(o / l[:, None])
    return out


def exact_bound(inp, case):
    """EXACT cases: (want, bound) per element.
    ones:  V == 1 -> 1, within u + u (the numerator rounds P to bf16, the denominator does not: at most u relative, then the output
           rounding, u above 1).
    qzero: Q == 0 -> the mean of V over the valid keys; p == 1 is exact in bf16, so what is left is the output rounding u |mean| and the fp32
           sums, (n + 2) 2^-24 mean |V| for n keys (n - 1 additions, the reciprocal and the product)."""
    O, A, _ = oracle(inp, case)
    if case.kind == "ones":
        return np.ones_like(O), np.full_like(O, 2 * U)
    return O, U * np.abs(O) + (case.Tk + 2) * 2.0 ** -24 * A


# ------------------------------------------------------------------------------------------------ layouts and packers
def layout_dims(layout, case):
    """Leading dimensions (elements), window column offsets (elements) and the byte shift of the output pointer off 16-byte alignment."""
    HD = case.H * case.D
    cls = case.route == "cls"
    kcols = case.B * (case.Tk - 1) if cls else round_up(case.Tk if case.shared else case.B * case.Tk, 64)
    qw = 2 * HD if cls else HD                                  # the CLS entry point takes Q | K as one buffer
    d = {"ldq": qw, "qoff": 0, "ldk": HD, "koff": 0, "ldvt": kcols, "ldo": HD, "oshift": 0, "ldvc": HD, "vcoff": 0}
    if layout == "window":
        d.update(ldq=qw + 72, qoff=40, ldk=HD + 24, koff=16, ldvt=kcols + 192, ldo=HD + 8, ldvc=HD + 12, vcoff=4)
    elif layout == "narrow_a":
        d.update(ldo=HD + 4)                                    # rows 8-byte aligned only: two 8-byte stores per group
    elif layout == "narrow_b":
        d.update(ldo=HD + 8, oshift=8)                          # ldo % 8 == 0, but the base pointer is 8 bytes off
    else:
        assert layout == "tight", layout
    return d


def _window(x2d, ld, off, extra_rows, align=8):
    M, W = x2d.shape
    assert off % align == 0 and off + W <= ld
    buf = np.full((M + extra_rows, ld), NAN_BITS, dtype=np.uint16)
    buf[:M, off:off + W] = bf16_bits(x2d)
    return buf


def pack_vt(v2d, ldvt, hostile=True):
    """[keys, H D] -> V^T [H D, ldvt]: key m in column perm16(m); every other column +- the largest finite bf16 (zero if not hostile)."""
    M, N = v2d.shape
    assert ldvt % 64 == 0 and ldvt >= round_up(M, 64)
    buf = np.zeros((N, ldvt), dtype=np.uint16)
    if hostile:
        buf[:, 0::2], buf[:, 1::2] = PAD_POS, PAD_NEG
    buf[:, perm16(np.arange(M))] = bf16_bits(v2d).T
    return buf


OUT_LEAD = 64                             # guard elements in front of the output window (128 bytes: keeps the 16-byte alignment)


def pack(inp, case, layout, hostile=True):
    """{"bufs": {name: (uint16 array, element offset of the pointer inside it)}, "dims": layout_dims, "M", "HD"}.  hostile = False: the same
    values with K ending at its last row and V^T pad columns zero."""
    d = layout_dims(layout, case)
    B, Tq, Tk, H, D = case.B, case.Tq, case.Tk, case.H, case.D
    HD, M = H * D, B * Tq
    q2, k2, v2 = (inp[n].reshape(-1, HD) for n in ("q", "k", "v"))
    bufs = {}
    if case.route == "cls":
        bufs["q"] = (_window(np.concatenate([q2, k2], 1), d["ldq"], d["qoff"], 3 if hostile else 0), d["qoff"])
        patch = np.arange(B * Tk) % Tk != 0
        bufs["vt"] = (pack_vt(v2[patch], d["ldvt"], hostile), 0)
        bufs["vcls"] = (_window(v2[~patch], d["ldvc"], d["vcoff"], 0, align=4), d["vcoff"])
    else:
        bufs["q"] = (_window(q2, d["ldq"], d["qoff"], 0), d["qoff"])
        bufs["k"] = (_window(k2, d["ldk"], d["koff"], 70 if hostile else 0), d["koff"])
        bufs["vt"] = (pack_vt(v2, d["ldvt"], hostile), 0)
    lead = OUT_LEAD + d["oshift"] // 2
    bufs["out"] = (np.full(lead + M * d["ldo"] + 64, NAN_BITS, dtype=np.uint16), lead)
    return {"bufs": bufs, "dims": d, "M": M, "HD": HD}


def out_window(outbuf, packed):
    """The [M, H D] window of a flat output buffer; asserts that every element outside it still holds NAN_BITS."""
    d, M, HD = packed["dims"], packed["M"], packed["HD"]
    lead = packed["bufs"]["out"][1]
    flat = np.asarray(outbuf, dtype=np.uint16).reshape(-1)
    inside = np.zeros(flat.shape, dtype=bool)
    idx = lead + (np.arange(M)[:, None] * d["ldo"] + np.arange(HD)[None, :])
    inside[idx] = True
    assert (flat[~inside] == NAN_BITS).all(), f"{int((flat[~inside] != NAN_BITS).sum())} elements outside the output window were written"
    return flat[idx]


# ------------------------------------------------------------------------------------------------ case tables
TQS = (1, 31, 32, 33, 127, 128, 129, 257)
TKS = (1, 3, 63, 64, 65, 77, 127, 129, 577)
EDGE_ROUTES = ("d64", "d64ps", "d128", "d192")
B_WANT = {1: 130, 3: 50, 63: 64, 64: 3, 65: 64, 77: 60, 127: 64, 129: 64, 577: 64}
WANTED_RESIDUES = (0, 1, 13, 31, 32, 63)


def edge_batch(tq, tk, shared):
    """Images of an EDGE_GRID case: as many as the residues want while the case stays under 2,500 query tokens (shared keys: the start
    residue is 0 whatever B is)."""
    return (2 if tq > 200 else 3) if shared else min(B_WANT[tk], max(2, 2400 // tq))


def required_residues(tk):
    return sorted(set(WANTED_RESIDUES) & {b * tk % 64 for b in range(B_WANT[tk])})


def _edge_grid():
    """Pairwise cover of Tq x Tk x route x kv_shared x causal: every (Tq, Tk) once, the other three factors chosen greedily (first best in
    product order) so that every pair of values of any two factors occurs; then, per Tk, one single-query case with the full batch (the
    start residues b Tk % 64; Tk = 1 x B = 130 and Tk = 3 x B = 50 among them)."""
    factors = (TQS, TKS, EDGE_ROUTES, (0, 1), (0, 1))
    pairs = lambda row: {((i, row[i]), (j, row[j])) for i in range(5) for j in range(i + 1, 5)}
    todo = set().union(*(pairs(r) for r in itertools.product(*factors)))
    rows = []
    for tq, tk in itertools.product(TQS, TKS):
        best = max(itertools.product(*factors[2:]), key=lambda c: len(pairs((tq, tk) + c) & todo))
        rows.append((tq, tk) + best)
        todo -= pairs(rows[-1])
    while todo:
        rows.append(max(itertools.product(*factors), key=lambda r: len(pairs(r) & todo)))
        todo -= pairs(rows[-1])
    cases = [Case(r, edge_batch(tq, tk, sh), tq, tk, 2, sh, ca, seed=i) for i, (tq, tk, r, sh, ca) in enumerate(rows)]
    cases += [Case(EDGE_ROUTES[i % 4], B_WANT[tk], 1, tk, 2, 0, 0, seed=500 + i) for i, tk in enumerate(TKS)]
    return tuple(cases)


EDGE_GRID = _edge_grid()
CLS_GRID = tuple(Case("cls", B, T, T, H, seed=600 + i) for i, (T, B, H) in enumerate(itertools.product((65, 129, 257, 577), (1, 3, 70), (1, 3))))
WIDE_GRID = tuple(Case("wide", 2, Tq, Tk, H, sh, seed=700 + i)
                  for i, (Tk, Tq, H, sh) in enumerate(itertools.product((64, 128, 576), (1, 96, 130, 300), (1, 2), (0, 1))))


def grid_layouts(grid):
    """(case, layout) pairs of a grid: every case tight and under one of the other three layouts in turn - per ROUTE, so that every route
    meets every layout."""
    seen, out = {}, []
    for c in grid:
        n = seen.get(c.route, 0)
        seen[c.route] = n + 1
        out += [(c, "tight"), (c, LAYOUTS[1 + n % 3])]
    return out


WIDE_GROWTHS = (0, 60, 99, 101, 115, 126, 200)
GROWTH = tuple(
    [Case("wide", 1, 130, 192, 1, kind="wgrow", param=(g, place, 1 if (gi + pi) % 2 == 0 else 2), seed=800 + 3 * gi + pi)
     for gi, g in enumerate(WIDE_GROWTHS) for pi, place in enumerate(("all", "wave2", "tail"))]
    + [Case(r, 2, 577 if r == "cls" else 96, 577 if r == "cls" else 576, 1, kind=kind, param=param, seed=850 + 10 * ri + ki)
       for ri, r in enumerate(("d64ps", "cls", "d64"))
       for ki, (kind, param) in enumerate((("stair", (7.5,)), ("stair", (8.5,)), ("onelane", ()), ("shift", (-3000.0,)), ("shift", (3000.0,))))]
    + [Case("cls", 2, 577, 577, 1, kind="clsgap", param=(g,), seed=890 + i) for i, g in enumerate((-3000.0, 3000.0))])

EXACT = tuple(Case(r, B, Tq, Tk, H, 0, ca, kind=kind, seed=900 + i)
              for i, ((r, B, Tq, Tk, H, ca), kind) in enumerate(itertools.product(
                  (("d64", 3, 70, 77, 2, 0), ("d64ps", 3, 70, 77, 2, 0), ("d128", 2, 70, 77, 2, 0), ("d192", 2, 33, 130, 1, 0),
                   ("cls", 3, 129, 129, 2, 0), ("wide", 2, 70, 128, 1, 0)), ("ones", "qzero"))))


def growth_figures(inp, case):
    """What a GROWTH case claims, measured in float64 from its inputs (image 0, head 0): see the host test for the conditions."""
    E = exponents(inp, case, 0)[0]
    tmax = np.stack([E[:, sl].max(1) for sl in key_tiles(case, 0)], 1)       # [rows, tiles]
    if case.kind == "wgrow":
        rows = growth_rows(case)
        others = [r for r in range(case.Tq) if r not in rows]
        return {"gap": E[rows].max(1) - tmax[rows, 0], "other_gap": E[others].max(1) - tmax[others, 0] if others else np.zeros(0),
                "tile": int(np.argmax(tmax[rows[0]]))}
    if case.kind == "stair":
        return {"steps": np.diff(tmax, axis=1)}
    if case.kind == "onelane":                                               # the second tile against the reference the first one left
        gap = tmax[:, 1] - (E[:, 0] if case.route == "cls" else tmax[:, 0])
        return {"row": float(gap[39]), "others": np.delete(gap, 39)}
    if case.kind == "shift":
        return {"first": E[:, 0] if case.route == "cls" else tmax[:, 0]}
    if case.kind == "clsgap":
        return {"gap": E[:, 0] - E[:, 1:].max(1)}
    raise ValueError(case.kind)


# ------------------------------------------------------------------------------------------------ refusals
# (name, entry point, overrides of the valid base call, return code, text in visrep_last_error).  A pointer override is None (null) or a
# byte offset added to the valid pointer; anything else replaces the argument.
ATTN_BASE = dict(q=0, ldq=128, k=0, ldk=128, vt=0, ldvt=128, out=0, ldo=128, B=1, Tq=64, Tk=64, H=2, head_dim=64, kv_shared=0, causal=0, scale=0.125)
CLS_BASE = dict(qk=0, ldqk=256, vt=0, ldvt=128, vcls=0, ldvc=128, out=0, ldo=128, B=2, T=65, H=2, head_dim=64)
POINTERS = ("q", "k", "vt", "out", "qk", "vcls")
ERR_ARG, ERR_SHAPE = -1, -2
_W512 = {"head_dim": 512, "H": 1, "ldq": 512, "ldk": 512, "ldo": 512}
REFUSALS = tuple(
    [(f"attn null {p}", "attn", {p: None}, ERR_ARG, "null pointer") for p in ("q", "k", "vt", "out")]
    + [(f"attn {p} + {o} bytes", "attn", {p: o}, ERR_ARG, "16-byte aligned") for p, o in (("q", 8), ("k", 2), ("vt", 8))]
    + [("attn out + 4 bytes", "attn", {"out": 4}, ERR_ARG, "8-byte aligned"),
       ("attn ldvt short", "attn", {"Tk": 65, "ldvt": 64}, ERR_SHAPE, "ldvt must cover"),
       ("attn pre-scaled Q at head 128", "attn", {"head_dim": 128, "H": 1, "scale": 0.0}, ERR_ARG, "pre-scaled Q"),
       ("attn head 512 causal", "attn", dict(_W512, causal=1), ERR_SHAPE, "head_dim 512 needs"),
       ("attn head 512 ragged Tk", "attn", dict(_W512, Tk=65), ERR_SHAPE, "head_dim 512 needs"),
       ("attn head 512 scale 0", "attn", dict(_W512, scale=0.0), ERR_SHAPE, "head_dim 512 needs")]
    + [(f"cls null {p}", "cls", {p: None}, ERR_ARG, "null pointer") for p in ("qk", "vt", "vcls", "out")]
    + [(f"cls {p} + 8 bytes", "cls", {p: 8}, ERR_ARG, "16-byte aligned") for p in ("qk", "vt")]
    + [(f"cls {p} + 4 bytes", "cls", {p: 4}, ERR_ARG, "8-byte aligned") for p in ("vcls", "out")]
    + [("mhsa qk + 8 bytes", "mhsa", {"qk": 8}, ERR_ARG, "16-byte aligned"), ("mhsa null out", "mhsa", {"out": None}, ERR_ARG, "null pointer")])
MHSA_BASE = dict(qk=0, ldqk=256, vt=0, ldvt=128, out=0, ldo=128, B=1, T=64, H=2, head_dim=64, scale=0.125)


def refusal_args(entry, overrides, base_ptr):
    """Positional arguments (without the stream) of a refused call: every pointer base_ptr (16-byte aligned), then the overrides."""
    a = dict({"attn": ATTN_BASE, "cls": CLS_BASE, "mhsa": MHSA_BASE}[entry])
    for n in a:
        if n in POINTERS:
            a[n] = base_ptr
    for n, v in overrides.items():
        a[n] = (None if v is None else base_ptr + v) if n in POINTERS else v
    return list(a.values())
