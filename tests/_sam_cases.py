"""Cases, float64 oracles, bound and rounding model of the SAM ViT kernels (csrc/attention_relpos.hip), and the HF oracle of the composed
tower; shared by tests/test_host_sam.py (no GPU) and tests/test_gpu_sam.py.  numpy and torch only; nothing here goes through the library.

Attention inputs are float64 arrays whose values are exact in bf16: q, k, v [NB, T, H, 64] (T = S S), and fp32-exact tables rel_h, rel_w
[NB, H, T, S].  The logit of (query, key) is  scale q.k + rel_h[q, k // S] + rel_w[q, k % S],  scale = 0.125 (the kernel's scale > 0 route:
Q is the UNSCALED query).

Bound, per output element, in the terms of tests/_attention_cases.py (P = the float64 softmax, A = P |V|, O = P V, u = 2^-8):

    |got - O|  <=  u (A + |O|)  +  4 * 2^-21 L A,        L = the largest |biased logit * log2 e| of the case.

The first term and 2 * 2^-21 L A of the second are the derivation of _attention_cases.py unchanged (bf16 P in P.V, one bf16 rounding of the
output; fp32 scores and v_exp_f32 good to a few 2^-23 L in numerator and denominator).  The position term adds three fp32 roundings per logit,
read off the kernel's sequence  b = fl(rel_h + rel_w);  c = fl(b log2 e);  t = fl(s scale log2 e + c)  (one fma): at most 2^-24 |b| log2 e,
2^-24 |c| and 2^-24 |t|, i.e. together at most 3 * 2^-24 Lc with Lc = the largest of |bias log2 e| and |t| over the case.  Two opposed terms
could make Lc exceed L by any factor; every case here keeps Lc <= 2 L, which the host test asserts on every case's inputs and the GPU test on the inputs it runs (`components`), so the
three roundings stay below 6 * 2^-24 L = 0.75 * 2^-21 L in the exponent, once in the numerator and once in the denominator: 1.5 * 2^-21 L A,
rounded up to 2.  Hence the constant 4 where the plain kernels have 2.  It is derived, not fitted: the rounding model below restates the
kernel's scheme with exactly these roundings and the host test holds it to the same bound."""
from typing import NamedTuple

import numpy as np
import torch

import _attention_cases as AC

U, LOG2E, SCALE = AC.U, AC.LOG2E, 0.125
THR = 8.0                                  # attn_fwd_relpos moves its reference when a tile's maximum exceeds it by more than 2^8


class Case(NamedTuple):
    S: int
    NB: int
    H: int
    kind: str = "rand"                     # rand | bias30 | stair | shift
    param: tuple = ()
    seed: int = 0

    @property
    def T(self):
        return self.S * self.S

    @property
    def id(self):
        return f"S{self.S}-NB{self.NB}-H{self.H}" + (f"-{self.kind}{'_'.join(str(p) for p in self.param)}" if self.kind != "rand" else "")


def tiny_spec(image_size: int = 160, patch: int = 8, d: int = 128, heads: int = 2, layers: int = 4, mlp: int = 256, window: int = 14,
              global_attn_indexes=(1, 3), out_channels: int = 64):
    """The tests' small tower: g = 20 (2 x 2 padded windows) by default; out_channels 64 = the smallest width visrep_conv3x3_bf16 accepts."""
    from law_of_vision_representation_in_mllms_amd import sam_weights as SW
    return SW.SamSpec("tiny-sam", image_size, patch, d, layers, heads, mlp, window, tuple(global_attn_indexes), out_channels)


def f32_exact(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def make_inputs(case):
    rs = np.random.RandomState(4000 + case.seed + 17 * case.S + case.NB)
    NB, T, S, H = case.NB, case.T, case.S, case.H
    quiet = case.kind in ("stair", "shift")
    amp = 0.05 if quiet else 1.0
    q = rs.standard_normal((NB, T, H, 64)) * amp
    k = rs.standard_normal((NB, T, H, 64)) * amp
    v = rs.standard_normal((NB, T, H, 64))
    bamp = {"rand": 1.0, "bias30": 10.0}.get(case.kind, 0.02)
    rel_h = rs.standard_normal((NB, H, T, S)) * bamp
    rel_w = rs.standard_normal((NB, H, T, S)) * bamp
    if case.kind == "bias30":                                   # |rel_h + rel_w| up to about 30: the position term dominates 0.125 q.k (|.| ~ 1)
        rel_h, rel_w = np.clip(rel_h, -15, 15), np.clip(rel_w, -15, 15)
    elif case.kind == "stair":                                  # the row maximum of consecutive 64-key tiles climbs by param[0] exp2 units
        step = case.param[0] / LOG2E
        rel_h[:] = 0.0
        rel_w[:] = 0.0
        key = np.arange(T)
        kh = key // S
        assert 64 % S == 0, "a stair needs key rows that lie inside one 64-key tile"
        for t in range(T // 64):                                # one key row per tile
            rel_h[:, :, :, kh[64 * t + S]] = t * step
    elif case.kind == "shift":                                  # every logit of every row moves by param[0]: the softmax does not
        rel_h += case.param[0] / LOG2E
    return {"q": AC.bf16_round(q), "k": AC.bf16_round(k), "v": AC.bf16_round(v), "rel_h": f32_exact(rel_h), "rel_w": f32_exact(rel_w)}


def bias_full(inp, case, g):
    """[H, T, T]: rel_h[q, k // S] + rel_w[q, k % S] of grid g."""
    key = np.arange(case.T)
    return inp["rel_h"][g][:, :, key // case.S] + inp["rel_w"][g][:, :, key % case.S]


def exponents(inp, case, g):
    """[H, T, T] float64: the exponent of 2 of every (query, key) of grid g."""
    qk = inp["q"][g].transpose(1, 0, 2) @ inp["k"][g].transpose(1, 2, 0)
    return (qk * SCALE + bias_full(inp, case, g)) * LOG2E


def components(inp, case):
    """(L, Lc): the largest |biased logit log2 e| and the largest single component (|bias log2 e|, |scale q.k log2 e|) of the case."""
    L = Lc = 0.0
    for g in range(case.NB):
        b = bias_full(inp, case, g) * LOG2E
        E = exponents(inp, case, g)
        L = max(L, float(np.abs(E).max()))
        Lc = max(Lc, float(np.abs(b).max()), float(np.abs(E - b).max()))
    return L, max(Lc, L)


def oracle(inp, case):
    """(O, A, L) as _attention_cases.oracle: [NB, T, H, 64] float64 and the largest |exponent of 2|."""
    O = np.empty_like(inp["q"]); A = np.empty_like(O); L = 0.0
    for g in range(case.NB):
        E = exponents(inp, case, g)
        L = max(L, float(np.abs(E).max()))
        P = np.exp2(E - E.max(-1, keepdims=True))
        P /= P.sum(-1, keepdims=True)
        vh = inp["v"][g].transpose(1, 0, 2)
        O[g] = (P @ vh).transpose(1, 0, 2)
        A[g] = (P @ np.abs(vh)).transpose(1, 0, 2)
    return O, A, L


def bound(O, A, L):
    return U * (A + np.abs(O)) + 4.0 * 2.0 ** -21 * L * A


def ratio(got, O, A, L):
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - O) / np.maximum(bound(O, A, L), 1e-300)).max())


def key_tiles(case, g):
    """Local key slices of grid g: the global 64-key blocks it overlaps (it starts at residue g T % 64 of its first block)."""
    tok0 = g * case.T
    edges = [0] + list(range(64 - tok0 % 64, case.T, 64)) + [case.T]
    return [slice(a, e) for a, e in zip(edges[:-1], edges[1:]) if e > a]


def rounding_model(inp, case):
    """attn_fwd_relpos's scheme with the roundings the bound is derived from and no other: fp32 q.k, b = fl(rel_h + rel_w), c = fl(b log2 e),
    t = fl(s * fl(scale log2 e) + c), reference = the first tile's row maximum, moved when a later tile's exceeds it by more than 8,
    p = fl(exp2(fl(t - m))), fp32 row sum of p, P.V over bf16(p), fp32 state, one bf16 rounding of O / l."""
    f = AC._f32
    sc = float(np.float32(np.float32(SCALE) * np.float32(LOG2E)))
    l2 = float(np.float32(LOG2E))
    out = np.empty_like(inp["q"])
    key = np.arange(case.T)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(case.NB):
            s = f(inp["q"][g].transpose(1, 0, 2) @ inp["k"][g].transpose(1, 2, 0))
            b = f(inp["rel_h"][g][:, :, key // case.S] + inp["rel_w"][g][:, :, key % case.S])
            E = f(s * sc + f(b * l2))
            vh = inp["v"][g].transpose(1, 0, 2)
            for h in range(case.H):
                Eh, V = E[h], vh[h]
                R = Eh.shape[0]
                m, l, o = np.full(R, -np.inf), np.zeros(R), np.zeros((R, 64))
                for ti, sl in enumerate(key_tiles(case, g)):
                    mloc = Eh[:, sl].max(1)
                    m_new = mloc if ti == 0 else np.where(mloc - m > THR, mloc, m)
                    alpha = np.where(m_new == m, 1.0, f(np.exp2(f(m - m_new))))
                    p = f(np.exp2(f(Eh[:, sl] - m_new[:, None])))
                    l = f(l * alpha + f(p.sum(1)))
                    o = f(o * alpha[:, None] + AC.bf16_round(p) @ V[sl])
                    m = m_new
                out[g, :, h] = AC.bf16_round(o / l[:, None])
    return out


# ------------------------------------------------------------------------------------------------ packing (the ABI's layouts)
def pack(inp, case, window=False):
    """{"qk", "vt", "out": (uint16 array, element offset), "rel_h", "rel_w": float32 arrays, "ldqk", "ldvt", "ldo"}.  window: Q | K inside a wider
    NaN-filled buffer followed by NaN rows, V^T with +-3.4e38 in every column that belongs to no key and 192 spare columns, the output a
    window in a NaN-filled buffer."""
    NB, T, H = case.NB, case.T, case.H
    HD, M = H * 64, NB * T
    q2, k2, v2 = (inp[n].reshape(M, HD) for n in ("q", "k", "v"))
    ldqk, qoff, ldo = (2 * HD + 72, 40, HD + 8) if window else (2 * HD, 0, HD)
    ldvt = AC.round_up(M, 64) + (192 if window else 0)
    qk = AC._window(np.concatenate([q2, k2], 1), ldqk, qoff, 70 if window else 0)
    lead = AC.OUT_LEAD
    out = np.full(lead + M * ldo + 64, AC.NAN_BITS, dtype=np.uint16)
    return {"qk": (qk, qoff), "vt": (AC.pack_vt(v2, ldvt, hostile=True), 0), "out": (out, lead), "ldqk": ldqk, "ldvt": ldvt, "ldo": ldo,
            "rel_h": np.ascontiguousarray(inp["rel_h"], dtype=np.float32), "rel_w": np.ascontiguousarray(inp["rel_w"], dtype=np.float32),
            "M": M, "HD": HD}


def out_window(outbuf, packed):
    return AC.out_window(outbuf, {"dims": {"ldo": packed["ldo"]}, "M": packed["M"], "HD": packed["HD"], "bufs": {"out": packed["out"]}})


GRID = tuple(Case(S, NB, H, seed=i) for i, (S, NB, H) in enumerate(
    [(S, NB, H) for S in (2, 8, 9, 14, 20) for NB in (1, 3, 50) for H in (1, 3)]))
GLOBAL = Case(64, 1, 1, seed=90)
BIAS30 = (Case(14, 3, 2, "bias30", seed=91), Case(9, 5, 1, "bias30", seed=92))
GROWTH = tuple(Case(S, 2, 1, kind, param, seed=93 + i) for i, (S, kind, param) in enumerate(
    [(16, "stair", (7.5,)), (16, "stair", (8.5,)), (14, "shift", (-3000.0,)), (14, "shift", (3000.0,))]))


# ------------------------------------------------------------------------------------------------ index test (exact)
def index_case(S, mode, seed=0):
    """K = 0; tables of +-60 one-hot patterns: query q puts all its mass on key tgt[q] (a permutation-like map that is neither symmetric in
    h / w nor in q / k).  mode 'h': rel_w = 0 and the target's ROW is chosen, the mass spreads evenly over the S keys of that row - V is
    constant along a row then, so the output is still one V row; 'w' likewise; 'hw': both tables, one key.  Returns (inp, want [T, 64])."""
    T = S * S
    rs = np.random.RandomState(7000 + seed)
    qi = np.arange(T)
    qh, qw = qi // S, qi % S
    th, tw = (2 * qh + qw + 1) % S, (qw + 3 * qh + 2) % S
    q = AC.bf16_round(rs.standard_normal((1, T, 1, 64)))
    k = np.zeros((1, T, 1, 64))
    v = AC.bf16_round(rs.standard_normal((1, T, 1, 64)))
    rel_h = np.zeros((1, 1, T, S)); rel_w = np.zeros((1, 1, T, S))
    key = np.arange(T)
    if mode in ("h", "hw"):
        rel_h[:] = -60.0
        rel_h[0, 0, qi, th] = 60.0
    if mode in ("w", "hw"):
        rel_w[:] = -60.0
        rel_w[0, 0, qi, tw] = 60.0
    if mode == "h":
        v[0, :, 0] = v[0, (key // S) * S, 0]                    # constant along a row
        want = v[0, th * S, 0]
    elif mode == "w":
        v[0, :, 0] = v[0, key % S, 0]                           # constant along a column
        want = v[0, tw, 0]
    else:
        want = v[0, th * S + tw, 0]
    return {"q": q, "k": k, "v": v, "rel_h": rel_h, "rel_w": rel_w}, want


# ------------------------------------------------------------------------------------------------ tables
def tables_oracle(q, Rh, Rw, NB, S, H):
    """float64 tables and the gamma_64 bound 64 * 2^-24 sum |q_i r_i| per entry.  q [NB T, H 64] (bf16-exact), Rh / Rw [2 S - 1, 64]."""
    T = S * S
    qq = q.reshape(NB, T, H, 64).transpose(0, 2, 1, 3)          # [NB, H, T, 64]
    qi = np.arange(T)
    ih = (qi // S)[:, None] - np.arange(S)[None, :] + S - 1     # [T, S]
    iw = (qi % S)[:, None] - np.arange(S)[None, :] + S - 1
    rh = np.einsum("ghtc,tkc->ghtk", qq, Rh[ih]); rw = np.einsum("ghtc,tkc->ghtk", qq, Rw[iw])
    bh = np.einsum("ghtc,tkc->ghtk", np.abs(qq), np.abs(Rh[ih])); bw = np.einsum("ghtc,tkc->ghtk", np.abs(qq), np.abs(Rw[iw]))
    return rh, rw, 64 * 2.0 ** -24 * bh, 64 * 2.0 ** -24 * bw


# ------------------------------------------------------------------------------------------------ windows
def window_rows(B, g, w):
    """src [B nw nw w w]: the map token row of every window row, -1 for a pad position (window_partition of the zero-padded map)."""
    nw = -(-g // w)
    r = np.arange(B * nw * nw * w * w)
    t, wi = r % (w * w), r // (w * w)
    wx, wy, b = wi % nw, (wi // nw) % nw, wi // (nw * nw)
    y, x = wy * w + t // w, wx * w + t % w
    return np.where((y < g) & (x < g), (b * g + y) * g + x, -1)


# ------------------------------------------------------------------------------------------------ the HF oracle of the tower
def hf_from_packed(spec, w, dtype=torch.float32):
    """transformers.SamVisionModel carrying the packed weights.  load_state_dict on purpose: SamVisionConfig.initializer_range is 1e-10, a
    freshly constructed module is the identity in every block, and this transformers makes torch.nn.init.* a no-op on initialised parameters."""
    from transformers import SamVisionModel
    from law_of_vision_representation_in_mllms_amd import sam_weights as SW
    m = SamVisionModel(SW.hf_config(spec)).eval()
    res = m.load_state_dict(SW.to_hf_state_dict(spec, w), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m.to(dtype)


@torch.no_grad()
def hf_states(model, pixels):
    """The L + 2 states as token rows: embeddings + positions, every layer's output, the neck map."""
    enc = model.vision_encoder
    x = enc.patch_embed(pixels.to(enc.pos_embed.dtype)) + enc.pos_embed
    B = x.shape[0]
    states = [x.reshape(B, -1, x.shape[-1])]
    for layer in enc.layers:
        x = layer(x)
        x = x[0] if isinstance(x, tuple) else x
        states.append(x.reshape(B, -1, x.shape[-1]))
    n = enc.neck(x)                                             # takes the channels-last map, returns [B, C, g, g]
    states.append(n.permute(0, 2, 3, 1).reshape(B, -1, n.shape[1]))
    return [s.float() for s in states]


def rel_err(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


_ORACLE_CACHE = {}


def tower_reference(spec, w, pixels, key):
    """(fp32 states, e_ref per state) of the HF module with the packed weights, computed once per key."""
    if key not in _ORACLE_CACHE:
        ref = hf_states(hf_from_packed(spec, w), pixels)
        lo = hf_states(hf_from_packed(spec, w, torch.bfloat16), pixels.to(torch.bfloat16))
        _ORACLE_CACHE[key] = (ref, [rel_err(a, b) for a, b in zip(lo, ref)])
    return _ORACLE_CACHE[key]


def zero_rel(w):
    out = dict(w)
    out["layers"] = [dict(L, rel_h=torch.zeros_like(L["rel_h"]), rel_w=torch.zeros_like(L["rel_w"])) for L in w["layers"]]
    return out


def pixels_for(spec, B, seed=0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((B, 3, spec.image_size, spec.image_size)).astype(np.float32))
