"""Attention operands that hold every row and every key to account.

With Gaussian q and k a softmax row is spread over hundreds of keys: a kernel that drops, doubles or mis-pairs ONE key moves a row by about
1 / Lk and the global rel-L2 by nothing.  Here every row's softmax sits on one known key (kind "one") or, exactly halved, on two (kind "two"),
so the row's exact answer is that key's V row (or the mean of the two) and any such mistake is an O(1) error of that (row, head):

    codes[h][j]   in {-1, +1}^128, one per key and head, from a seeded generator
    k[j]          = a * codes[j]
    v[j]          Gaussian rounded to bf16, different for every key and head
    "one"         q[i] = a * codes[pi(i)]                           pi(i) = (7 i + 3) % Lk, plus overrides (below)
    "two"         q[i] = a * (codes[pi(i)] + codes[pj(i)])          pj(i) = (pi(i) + Lk // 2 + 5) % Lk: the two logits are EQUAL (the same sum of
                                                                    the same terms, whatever roundings a kernel applies to q), the answer is
                                                                    (v[pi] + v[pj]) / 2

a is 1.5, 2 or 3 (and 4 where a test needs the long kernel's optimistic pass to give up: none of the three takes a row out of its window): every operand is exact in bf16, and in e4m3 under a power-of-two block scale.
The own logit is a^2 * 128 (* 1 / sqrt(128) at the seams that scale), the others a^2 * N(0, 128): the row's mass off its key is < 1e-5
(tests/test_attn_probe_inputs.py asserts >= 0.99 for every shape in use).

Overrides: rows spread evenly over [0, Lq) (the last row among them) are sent to the first key, the last key and the keys on both sides of every
64-key tile edge and every edge in `edges` (the pieces of a split key axis); a "two" row whose partner would fall into the same tile or piece
moves the partner on by whole tiles until it does not.

key_tail = (n, m) (cross-attention): keys n-1 .. Lk-1 are made identical (code and V), the maps run over the n keys walked, and the last of them is
the tail key: a "one" row on it must return v[n-1], a "two" row pairing it with key j  (m v[n-1] + v[j]) / (m + 1).

References are fp64 softmax attention on the same operands (oracle.wan_dit_oracle.attention; attention_base2 for the seams whose q carries
softmax_scale * log2(e): p = 2^(q.k)).  flash_restatement is a flash kernel's rounding points (unnormalised P in bf16, fp32 sums, bf16 output).
"""
import math

import numpy as np
import torch

KB = 64
GAINS = (1.5, 2.0, 3.0)


def bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


def draw_codes(seed: int, Lk: int, heads: int) -> np.ndarray:
    """[heads, Lk, 128] in {-1, +1}."""
    return np.random.default_rng(seed).integers(0, 2, size=(heads, Lk, 128)).astype(np.float64) * 2 - 1


def draw_values(seed: int, Lk: int, heads: int) -> torch.Tensor:
    """[Lk, heads * 128] fp64 holding bf16 values."""
    return bf16(torch.from_numpy(np.random.default_rng(seed).standard_normal((Lk, heads * 128))))


def piece_edges(Lk: int, pieces: int):
    """First keys of pieces 1 .. of the long kernel's split key axis (whole tiles, ceil(tiles / pieces) each)."""
    tiles = (Lk + KB - 1) // KB
    per = (tiles + pieces - 1) // pieces
    return [z * per * KB for z in range(1, pieces) if z * per * KB < Lk]


def key_maps(Lq: int, Lk: int, edges=()):
    """pi, pj (int arrays [Lq]) and the override targets that found a row."""
    pi = (7 * np.arange(Lq) + 3) % Lk
    bounds = sorted(set(e for e in edges if 0 < e < Lk))
    targets = [0, Lk - 1]
    for e in bounds + [e for e in range(KB, Lk, KB) if e not in bounds]:
        targets += [e - 1, e]
    targets = list(dict.fromkeys(targets))[:Lq]
    rows = np.unique(np.linspace(0, Lq - 1, len(targets)).round().astype(int))[::-1]          # the last row first: it takes the first key
    targets = targets[:len(rows)]
    pi[rows] = targets
    cuts = [0] + bounds + [Lk]
    piece = lambda j: np.searchsorted(cuts, j, side="right")
    pj = (pi + Lk // 2 + 5) % Lk
    if Lk >= 3 * KB:
        for _ in range(Lk // KB):
            clash = (pj // KB == pi // KB) | ((piece(pj) == piece(pi)) if bounds else False)
            if not clash.any():
                break
            pj = np.where(clash, (pj + KB) % Lk, pj)
    pj = np.where(pj == pi, (pi + 1) % Lk, pj) if Lk > 1 else pj
    return pi, pj, targets


def build(kind: str, a: float, Lq: int, Lk: int, heads: int, seed: int = 0, edges=(), key_tail=None, v_seed=None):
    """q [Lq, D], k [Lk, D], v [Lk, D] (fp64 tensors of bf16 values, D = heads * 128) and the maps.  key_tail = (n, m): Lk = n - 1 + m."""
    assert kind in ("one", "two") and Lq >= 1 and Lk >= 2
    n = Lk
    if key_tail is not None:
        n, m = key_tail
        assert n - 1 + m == Lk and n >= 2
    codes = draw_codes(1000 + seed, Lk, heads)
    v = draw_values(2000 + seed if v_seed is None else v_seed, Lk, heads)
    if key_tail is not None:
        codes[:, n - 1:] = codes[:, n - 1:n]
        v[n - 1:] = v[n - 1]
    pi, pj, targets = key_maps(Lq, n, edges)
    c = torch.from_numpy(codes)                                     # [heads, Lk, 128]
    qc = c[:, pi] if kind == "one" else c[:, pi] + c[:, pj]        # [heads, Lq, 128]
    q = (a * qc).permute(1, 0, 2).reshape(Lq, heads * 128).contiguous()
    k = (a * c).permute(1, 0, 2).reshape(Lk, heads * 128).contiguous()
    assert torch.equal(bf16(q), q) and torch.equal(bf16(k), k)
    return {"q": q, "k": k, "v": v, "pi": pi, "pj": pj if kind == "two" else None, "targets": targets, "kind": kind, "a": a, "heads": heads,
            "key_tail": key_tail, "walked": n}


def softmax64(q: torch.Tensor, k: torch.Tensor, heads: int, base2: bool = False) -> torch.Tensor:
    """[heads, Lq, Lk] fp64 softmax of q.k / sqrt(128) (base2: of 2^(q.k), q carrying the scale)."""
    qh = q.double().reshape(q.shape[0], heads, 128).transpose(0, 1)
    kh = k.double().reshape(k.shape[0], heads, 128).transpose(0, 1)
    s = qh @ kh.transpose(1, 2)
    s = s * math.log(2.0) if base2 else s / math.sqrt(128.0)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    return p / p.sum(-1, keepdim=True)


def attention_base2(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int) -> torch.Tensor:
    """fp64 softmax2(q.k^T) v, [Lq, heads * 128]: the seams whose q already carries softmax_scale * log2(e)."""
    vh = v.double().reshape(v.shape[0], heads, 128).transpose(0, 1)
    return (softmax64(q, k, heads, base2=True) @ vh).transpose(0, 1).reshape(q.shape[0], heads * 128)


def reference(p: dict, base2: bool = False) -> torch.Tensor:
    """fp64 attention over ALL keys of the probe (a key_tail's copies included), [Lq, D]."""
    if base2:
        return attention_base2(p["q"], p["k"], p["v"], p["heads"])
    from oracle import wan_dit_oracle as wdo
    return wdo.attention(p["q"].double()[None], p["k"].double()[None], p["v"].double()[None], p["heads"])[0]


def intended_mass(p: dict, base2: bool = False) -> float:
    """The smallest share of a row's fp64 softmax that lies on its intended key (pair); a key_tail's copies count as the tail key."""
    P = softmax64(p["q"], p["k"], p["heads"], base2)
    n = p["walked"]
    if P.shape[-1] > n:
        P = torch.cat([P[..., :n - 1], P[..., n - 1:].sum(-1, keepdim=True)], -1)
    rows = torch.arange(P.shape[1])
    mass = P[:, rows, torch.from_numpy(p["pi"])]
    if p["pj"] is not None:
        mass = mass + P[:, rows, torch.from_numpy(p["pj"])]
    return float(mass.min())


def closed_form(p: dict) -> torch.Tensor:
    """What the rows return when all the mass is on the intended keys: v[pi], (v[pi] + v[pj]) / 2, with a tail key counted m times."""
    v, pi = p["v"], torch.from_numpy(p["pi"])
    if p["pj"] is None:
        return v[pi]
    pj = torch.from_numpy(p["pj"])
    n, m = p["key_tail"] if p["key_tail"] is not None else (-1, 1)
    wi = torch.where(pi == n - 1, float(m), 1.0).double()[:, None]
    wj = torch.where(pj == n - 1, float(m), 1.0).double()[:, None]
    return (wi * v[pi] + wj * v[pj]) / (wi + wj)


def flash_restatement(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, base2: bool = False) -> torch.Tensor:
    """A flash kernel's rounding points on exact scores: p = exp(s - max) in fp32, the row sum over the fp32 p, P rounded to bf16 for P V (fp32
    sums), the quotient rounded to bf16."""
    qh = q.double().reshape(q.shape[0], heads, 128).transpose(0, 1)
    kh = k.double().reshape(k.shape[0], heads, 128).transpose(0, 1)
    vh = v.float().reshape(v.shape[0], heads, 128).transpose(0, 1)
    s = qh @ kh.transpose(1, 2)
    s = s * math.log(2.0) if base2 else s / math.sqrt(128.0)
    p = torch.exp(s - s.amax(-1, keepdim=True)).float()
    l = p.sum(-1, keepdim=True, dtype=torch.float32)
    o = (p.to(torch.bfloat16).float() @ vh) / l
    return o.to(torch.bfloat16).double().transpose(0, 1).reshape(q.shape[0], heads * 128)


# ---- the cases of tests/test_gpu_attention_rows.py (tests/test_attn_probe_inputs.py checks every one on the CPU) ----------------------------------
SHORT_SHAPES = [(64, 64, 1), (130, 77, 2), (300, 513, 3)]
LONG_SHAPES = [(256, 2048, 1), (300, 2111, 2), (513, 4133, 1), (2304, 2304, 1)]
SPLIT_SHAPE = (300, 8192 + 77, 2)
QK8_SHAPE = (300, 2111, 2)
VT_SHAPES = [(130, 77, 2), (300, 2111, 2)]
CROSS_PLAIN = [(300, 33), (300, 96), (513, 128), (300, 130), (513, 512)]                     # (Lq, keys walked): resident 2, 3, 4 blocks; streaming
CROSS_TAILS = [(300, 33, 480), (513, 128, 1), (300, 129, 2), (300, 96, 2), (300, 130, 383)]  # (Lq, n, m): Lk = n - 1 + m
FRAMES = dict(frames=5, rows_per_frame=130, heads=2, keys_per_frame=(40, 72), ranges=((0, 650), (57, 400), (130, 130)))


def frame_probe(kind: str, a: float, keys_per_frame: int, seed: int = 0):
    """The talk variant's frame attention: the same code set in every frame, another V per frame.  q [650, D], k, v [5 kpf, D]."""
    F, rpf, heads = FRAMES["frames"], FRAMES["rows_per_frame"], FRAMES["heads"]
    per = [build(kind, a, rpf, keys_per_frame, heads, seed=seed, v_seed=3000 + 17 * seed + f) for f in range(F)]
    assert all(torch.equal(per[0]["k"], p["k"]) and not torch.equal(per[0]["v"], p["v"]) for p in per[1:])
    return per, torch.cat([p["q"] for p in per]), torch.cat([p["k"] for p in per]), torch.cat([p["v"] for p in per])


def all_probes():
    """(name, probe, base2) for every operand set the GPU tests use (the frame sets as one probe per frame)."""
    out = []
    for Lq, Lk, heads in SHORT_SHAPES:
        for kind in ("one", "two"):
            out.append((f"short-{Lq}x{Lk}x{heads}-{kind}", build(kind, 2.0, Lq, Lk, heads, seed=Lk), False))
    for s in (0, 1):
        out.append((f"short-batch{s}", build("two", 1.5, 130, 77, 2, seed=500 + s), False))
    for Lq, Lk, heads in LONG_SHAPES:
        for kind, a in (("one", 1.5), ("two", 3.0), ("one", 4.0)):
            out.append((f"long-{Lq}x{Lk}x{heads}-{kind}-{a}", build(kind, a, Lq, Lk, heads, seed=Lk), False))
    Lq, Lk, heads = SPLIT_SHAPE
    for kind in ("two", "one"):
        out.append((f"split-{kind}", build(kind, 2.0, Lq, Lk, heads, seed=7, edges=piece_edges(Lk, 2)), False))
    for kind in ("one", "two"):
        out.append((f"qk8-{kind}", build(kind, 2.0, *QK8_SHAPE, seed=9), False))
    for Lq, Lk, heads in VT_SHAPES:
        for pre in (0, 1):
            out.append((f"vt-{Lq}x{Lk}-pre{pre}", build("two" if pre else "one", 1.5, Lq, Lk, heads, seed=20 + pre), bool(pre)))
    for Lq, Lk in CROSS_PLAIN:
        for kind in ("one", "two"):
            out.append((f"cross-{Lq}x{Lk}-{kind}", build(kind, 1.5, Lq, Lk, 2, seed=30 + Lk), True))
    for Lq, n, m in CROSS_TAILS:
        for kind in ("one", "two"):
            out.append((f"cross-tail-{Lq}x{n}x{m}-{kind}", build(kind, 2.0, Lq, n - 1 + m, 2, seed=40 + n, key_tail=(n, m)), True))
    for kpf in FRAMES["keys_per_frame"]:
        for kind in ("one", "two"):
            for f, p in enumerate(frame_probe(kind, 2.0, kpf, seed=kpf)[0]):
                out.append((f"frames-{kpf}-{kind}-f{f}", p, False))
    return out
