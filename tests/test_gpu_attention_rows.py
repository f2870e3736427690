"""-m gpu: every attention seam, every ROW and HEAD on its own, on operands that pin each row's softmax to one known key or an exactly halved pair
(tests/attn_probe.py; the operand sets are checked on the CPU by tests/test_attn_probe_inputs.py).

The attention tests elsewhere feed Gaussian operands and assert one global rel-L2: a key dropped in a masked last tile, a V column mis-paired
under the key permutation, a wrong piece in the split merge, a wrong multiplicity of the key_tail or a row reading the next frame's keys moves that
figure by less than its tolerance.  Here each of those is an O(1) error of some (row, head), and the assertion is the project's attention tolerance
(test_flash_attention: "a little over one bf16 ulp", rel-L2 <= 6e-3) applied per (row, head) against fp64 attention on the same bf16 operands.

Measured on an MI355X, worst (row, head) rel-L2 (global rel-L2 of the same outputs: 0 .. 2.3e-3):
    short-key kernel, batch of two      "one" 0 (the V row comes back bit for bit), "two" 2.4e-3 (the mean of two V rows rounded once to bf16: the CPU restatement's figure)
    long kernel, optimistic pass        "one" a = 1.5: 5.4e-3, "two" a = 3: 4.4e-3; identical with SVI_FLASH_M16 = 1 and 0.  The pass's reference is the tile-0 maximum
                                        + 64, not the row maximum, so the row's P is no power of two: its bf16 rounding scales the whole V row by up to 2^-8 before the
                                        output is rounded once more — two roundings where the short kernels have one, still inside the bound
    long kernel, complete kernel        "one" a = 4: 0 (every flagged workgroup)
    split key axis                      2 pieces: "two" 3.7e-3, "one" 5.0e-3; unsplit: 4.0e-3, 5.1e-3
    fp8 QK^T                            "one" 5.0e-3, "two" 4.1e-3
    svi_attention_vt_fwd, padded        short 5.4e-9 / 2.1e-3 (q_prescaled 0 / 1), long 5.5e-3 / 2.3e-3; out's padding unchanged
    svi_cross_attention_fwd             "one" 0, "two" 2.3e-3, with and without the query normalisation (same bits); key_tail rows 0 / 1.9e-3
    svi_attention_frames_fwd            "one" 0, "two" 2.4e-3
Flagged workgroups of the optimistic pass (svi_attention_last_flagged) through svi_attention_fwd: a = 1.5 kind "one" and a = 3 kind "two": 0 of 1 / 4 / 3 / 9, a = 2 (split,
fp8): 0 (the peak of a = 3, kind "two" is 147 + 1.15 (c_pi . c_pj) log2 units against a tile-0 maximum of ~ 45: inside the 160 the pass covers, so none of the three gains leaves it); a = 4, which is as
exact in bf16 and e4m3 (peak 261): 1 of 1, 4 of 4, 2 of 3 (the third workgroup holds one row, pinned to key 0), 9 of 9; svi_attention_vt_fwd with q_prescaled = 1 at
a = 1.5 (peak 288): 4 of 4.
"""
import ctypes as C

import pytest
import torch

import attn_probe as ap
from gpu_util import dev, report, row_errs

pytestmark = pytest.mark.gpu

BOUND = 6e-3


@pytest.fixture(scope="module")
def hip():
    import svi_hip
    assert svi_hip._lib.lib().svi_device_count() >= 1
    return svi_hip


@pytest.fixture(scope="module")
def probes():
    """name -> (operands, base2, fp64 reference computed once)."""
    cache = {}
    table = {n: (p, b2) for n, p, b2 in ap.all_probes()}

    def get(name):
        if name not in cache:
            p, b2 = table[name]
            cache[name] = (p, ap.reference(p, b2))
        return cache[name]
    return get


def last_flagged():
    from svi_hip import _lib as L
    a, b = C.c_int32(), C.c_int32()
    L.check(L.lib().svi_attention_last_flagged(L.current_stream(), C.byref(a), C.byref(b)), "svi_attention_last_flagged")
    return a.value, b.value


def vt_of(v, ldvt=None, fill=0.0):
    """V^T [D, ldvt] bf16 on the device, columns past the keys filled."""
    Lk, D = v.shape
    ldvt = (Lk + 7) // 8 * 8 if ldvt is None else ldvt
    vt = torch.full((D, ldvt), fill, dtype=torch.bfloat16, device="cuda")
    vt[:, :Lk] = dev(v).t()
    return vt


def check(name, got, want, heads, **info):
    worst, at, glob = row_errs(got, want, heads)
    report("attention_rows", case=name, worst_row_rel_l2=worst, row=at[0], head=at[1], tile_of_row=at[0] // 128, global_rel_l2=glob, **info)
    print(f"attention_rows {name}: worst (row, head) {worst:.3e} at {at}, global {glob:.3e} {info}")
    assert torch.isfinite(got.float()).all() and worst <= BOUND, (name, worst, at, glob)
    return worst


class switches:
    def __init__(self, **sw):
        self.sw = sw

    def __enter__(self):
        from svi_hip import _lib as L
        for k, v in self.sw.items():
            L.set_switch(k, v)

    def __exit__(self, *a):
        from svi_hip import _lib as L
        for k in self.sw:
            L.set_switch(k, None)


def flash(hip, p):
    return hip.flash_attention(dev(p["q"])[None], dev(p["k"])[None], dev(p["v"])[None], p["heads"])[0]


# ------------------------------------------------------------------------------------------ svi_attention_fwd, short key axes
@pytest.mark.parametrize("kind", ["one", "two"])
@pytest.mark.parametrize("Lq,Lk,heads", ap.SHORT_SHAPES)
def test_short_key_kernel_rows(hip, probes, Lq, Lk, heads, kind):
    """flash_fwd_kernel<0> (Lq == Lk) and <1>: one tile, a masked last tile, rows that end inside a 128-row workgroup, three heads."""
    name = f"short-{Lq}x{Lk}x{heads}-{kind}"
    p, want = probes(name)
    check(name, flash(hip, p), want, heads)


def test_short_key_kernel_batch_of_two(hip, probes):
    """Two samples with different codes in one call: a sample served from the other's K or V is an O(1) error of every row."""
    (p0, w0), (p1, w1) = probes("short-batch0"), probes("short-batch1")
    q, k, v = (dev(torch.stack([p0[n], p1[n]])) for n in ("q", "k", "v"))
    got = hip.flash_attention(q, k, v, 2)
    check("short-batch0", got[0], w0, 2)
    check("short-batch1", got[1], w1, 2)


# ------------------------------------------------------------------------------------------ svi_attention_fwd, the long kernel
@pytest.mark.parametrize("m16", [1, 0])
@pytest.mark.parametrize("kind,a,expect_flags", [("one", 1.5, False), ("two", 3.0, False), ("one", 4.0, True)])
@pytest.mark.parametrize("Lq,Lk,heads", ap.LONG_SHAPES)
def test_long_kernel_rows_in_both_passes(hip, probes, Lq, Lk, heads, kind, a, expect_flags, m16):
    """The optimistic pass (flash_fwd3_kernel, SVI_FLASH_M16=0: flash_fwd2_kernel<.., 1>) and the complete kernel behind it, Lq == Lk and Lq != Lk.
    The optimistic pass covers rows whose peak lies up to 160 log2 units above their tile-0 maximum.  a = 1.5: peak 36.7 log2 units, no workgroup
    flagged, every row is the optimistic pass's.  a = 3, kind "two": peak 147 + 1.15 (c_pi . c_pj) against a tile-0 maximum of ~ 45: still inside
    the window, 0 flagged (measured; no parametrisation of the three gains flags a workgroup).  a = 4: peak 261, tile-0 maximum ~ 55 — the workgroups
    with a row whose key lies outside tile 0 are flagged (1 / 1, 4 / 4, 2 / 3, 9 / 9) and all their rows are the complete kernel's."""
    name = f"long-{Lq}x{Lk}x{heads}-{kind}-{a}"
    p, want = probes(name)
    with switches(SVI_FLASH_M16=m16):
        got = flash(hip, p)
        flagged, nwg = last_flagged()
    check(name, got, want, heads, m16=m16, flagged=flagged, workgroups=nwg)
    assert nwg == (Lq + 255) // 256 * heads
    assert (flagged > 0) == expect_flags, (flagged, nwg)


# ------------------------------------------------------------------------------------------ the split key axis
@pytest.mark.parametrize("kind", ["two", "one"])
@pytest.mark.parametrize("pieces", [2, 1])
def test_split_key_axis_rows(hip, probes, pieces, kind):
    """8269 keys in two pieces of 65 and 65 tiles (the last ragged) and merged, against the same operands unsplit.  Kind "two": the two keys of every
    row lie in different pieces, so every row is a merge of two equal halves; kind "one": rows on both sides of the piece edge, on the last key and on
    keys of the ragged piece — the other piece contributes ~ 0."""
    name = f"split-{kind}"
    p, want = probes(name)
    with switches(SVI_FLASH_SPLIT=pieces):
        got = flash(hip, p)
        flagged, nwg = last_flagged()
    check(name, got, want, p["heads"], pieces=pieces, flagged=flagged, workgroups=nwg)
    assert nwg == 2 * p["heads"] * pieces


# ------------------------------------------------------------------------------------------ fp8 QK^T
@pytest.mark.parametrize("kind", ["one", "two"])
def test_fp8_qk_rows(hip, probes, kind):
    """SVI_ATTN_QK8=1: +-a, +-2a and 0 are exact in e4m3 under the quantiser's power-of-two block scale, so the fp64 reference and the bound stand."""
    name = f"qk8-{kind}"
    p, want = probes(name)
    with switches(SVI_ATTN_QK8=1):
        got = flash(hip, p)
        flagged, nwg = last_flagged()
    check(name, got, want, p["heads"], flagged=flagged, workgroups=nwg)


# ------------------------------------------------------------------------------------------ svi_attention_vt_fwd, padded leading dimensions
@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("Lq,Lk,heads", ap.VT_SHAPES)
def test_vt_seam_with_padded_leading_dimensions(hip, probes, Lq, Lk, heads, pre):
    """ldq = ldk = ldo = heads * 128 + 64, ldvt = Lk rounded up to 8, + 24; the padding of q, k and V^T (all of it inside the tensors allocated here) holds
    1e4, that of out a pattern that must come back bit for bit.  q_prescaled = 1: q is taken as carrying softmax_scale * log2(e) (SVI_QK_SCALE_LOG2E), the
    reference is p = 2^(q.k) — 288 log2 units at a = 1.5, so on the long kernel these rows are the complete kernel's (flagged > 0)."""
    from svi_hip import _lib as L
    name = f"vt-{Lq}x{Lk}-pre{pre}"
    p, want = probes(name)
    D, ld, ldvt = heads * 128, heads * 128 + 64, (Lk + 7) // 8 * 8 + 24

    def padded(t):
        out = torch.full((t.shape[0], ld), 1e4, dtype=torch.bfloat16, device="cuda")
        out[:, :D] = dev(t)
        return out
    q, k, vt = padded(p["q"]), padded(p["k"]), vt_of(p["v"], ldvt, fill=1e4)
    out = ((torch.arange(Lq * ld, device="cuda") % 251).float() - 100.0).to(torch.bfloat16).reshape(Lq, ld).contiguous()
    before = out.clone()
    L.check(L.lib().svi_attention_vt_fwd(q.data_ptr(), ld, k.data_ptr(), ld, vt.data_ptr(), ldvt, out.data_ptr(), ld, Lq, Lk, heads, pre, L.current_stream()),
            "svi_attention_vt_fwd")
    flagged, nwg = last_flagged() if Lk >= 2048 else (0, 0)
    check(name, out[:, :D], want, heads, q_prescaled=pre, flagged=flagged, workgroups=nwg)
    assert torch.equal(out[:, D:].view(torch.int16), before[:, D:].view(torch.int16))
    if Lk >= 2048:
        assert (flagged > 0) == bool(pre), (flagged, nwg)


# ------------------------------------------------------------------------------------------ svi_cross_attention_fwd
def cross(hip, p, norm=False, kt=None):
    heads, Lq, Lk = p["heads"], p["q"].shape[0], p["k"].shape[0]
    q, kw = p["q"], {}
    if norm:        # rs, gain and the scale are powers of two and the stored q is the probe q divided by them: bf16(bf16(bf16(q rs) gain) scale) is the probe q exactly
        rs = 2.0 ** ((torch.arange(Lq) % 3) - 1).double()
        gain = 2.0 ** ((torch.arange(heads * 128) % 3) - 1).double()
        q = q / (rs[:, None] * gain[None, :] * 0.5)
        assert torch.equal(ap.bf16(q), q)
        kw = dict(q_rs=rs.float().cuda(), q_gain=dev(gain), q_out_scale=0.5)
    if kt is not None:
        kw["key_tail"] = torch.tensor(list(kt), dtype=torch.int32, device="cuda")
    return hip.ops.cross_attention(dev(q), dev(p["k"]), vt_of(p["v"]), heads, s_kv=Lk, **kw)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("kind", ["one", "two"])
@pytest.mark.parametrize("Lq,Lk", ap.CROSS_PLAIN)
def test_cross_attention_rows(hip, probes, Lq, Lk, kind, norm):
    """33, 96, 128 keys: flash_cross_resident_kernel with 2, 3, 4 key blocks; 130, 512: the streaming kernel; rows that end inside a 256-row chunk.  norm:
    the query normalisation applied as q is read (q_rs / q_gain / q_out_scale), with factors chosen so that the normalised q is the probe q bit for bit."""
    name = f"cross-{Lq}x{Lk}-{kind}"
    p, want = probes(name)
    check(name, cross(hip, p, norm=norm), want, 2, norm=norm)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("kind", ["one", "two"])
@pytest.mark.parametrize("Lq,n,m", ap.CROSS_TAILS)
def test_cross_attention_key_tail_multiplicity(hip, probes, Lq, n, m, kind, norm):
    """key_tail = (n, m): n keys walked, the last counted m times.  The fp64 reference runs over all n - 1 + m keys (the tail's copies written out), where a
    "one" row on the tail key returns v[n-1] and a "two" row pairing it with key j  (m v[n-1] + v[j]) / (m + 1) (asserted on the CPU): a tail counted
    once, or m - 1 or m + 1 times, is an error of 1 / (m + 1) and more of those rows for m = 1, 2, and the rows of the pinned tail key fail outright if
    the key is dropped."""
    name = f"cross-tail-{Lq}x{n}x{m}-{kind}"
    p, want = probes(name)
    got = cross(hip, p, norm=norm, kt=(n, m))
    check(name, got, want, 2, norm=norm, tail=[n, m])
    rows = torch.from_numpy(p["pi"] == n - 1)
    assert rows.any()
    check(name + "-tail-rows", got[rows.cuda()], ap.closed_form(p)[rows], 2, norm=norm, tail=[n, m])


# ------------------------------------------------------------------------------------------ svi_attention_frames_fwd
@pytest.mark.parametrize("kind", ["one", "two"])
@pytest.mark.parametrize("kpf", ap.FRAMES["keys_per_frame"])
def test_frame_attention_rows_read_their_own_frame(hip, probes, kpf, kind):
    """5 frames of 130 rows; the SAME codes in every frame and another V per frame: a row of frame f pinned to code c returns frame f's v[c], and the same
    key of any other frame is an O(1) error.  Ranges: all rows, one that starts and ends inside a frame, exactly one frame."""
    F, rpf, heads = ap.FRAMES["frames"], ap.FRAMES["rows_per_frame"], ap.FRAMES["heads"]
    per = [probes(f"frames-{kpf}-{kind}-f{f}") for f in range(F)]
    q, k, v = (torch.cat([p[n] for p, _ in per]) for n in ("q", "k", "v"))
    want = torch.cat([w for _, w in per])
    kd, vt = dev(k), vt_of(v)
    assert vt.shape[1] == F * kpf
    for row0, nrows in ap.FRAMES["ranges"]:
        got = hip.ops.frame_attention(dev(q[row0:row0 + nrows]), kd, vt, heads, rpf, kpf, row0)
        check(f"frames-{kpf}-{kind}-rows{row0}+{nrows}", got, want[row0:row0 + nrows], heads, row0=row0, rows_per_frame=rpf)
