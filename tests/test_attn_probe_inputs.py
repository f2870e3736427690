"""The operands of tests/test_gpu_attention_rows.py, checked without a GPU (tests/attn_probe.py builds them).

For every operand set the GPU tests use:
  * the fp64 softmax puts >= 0.99 of every row on its intended key (kind "one") or key pair (kind "two"), and the fp64 reference is the closed
    form (v[pi]; (v[pi] + v[pj]) / 2; (m v_tail + v_j) / (m + 1) under a key_tail) to 1e-4 per (row, head);
  * a bf16 restatement of a flash kernel's rounding points (unnormalised P in bf16, fp32 sums, bf16 output) stays within 3e-3 worst (row, head)
    rel-L2 of the fp64 result: half the GPU tests' bound of 6e-3, so the reference alone leaves that margin (measured: 1.5e-6 for "one", up to
    2.3e-3 for "two" — the rounding of the output itself);
  * a deliberately wrong reference — two V rows of one tile swapped, or the last key dropped — is an O(1) error of some (row, head) under the same
    metric, i.e. the GPU tests would fail a kernel that made that mistake.
"""
import pytest
import torch

import attn_probe as ap
from gpu_util import row_errs

PROBES = ap.all_probes()


def test_every_gpu_case_is_covered_here():
    names = [n for n, _, _ in PROBES]
    assert len(set(names)) == len(names)
    for fam in ("short-", "long-", "split-", "qk8-", "vt-", "cross-", "cross-tail-", "frames-"):
        assert any(n.startswith(fam) for n in names), fam


@pytest.mark.parametrize("name,p,base2", PROBES, ids=[n for n, _, _ in PROBES])
def test_probe_operands(name, p, base2):
    heads, n, Lk = p["heads"], p["walked"], p["k"].shape[0]
    q, k, v = p["q"], p["k"], p["v"]
    assert torch.equal(ap.bf16(v), v) and len(torch.unique(v, dim=0)) == (n if p["key_tail"] else Lk)          # another V row for every key
    assert set(p["targets"]) <= set(p["pi"].tolist()) and {0, n - 1} <= set(p["targets"])
    if n > ap.KB:
        assert {ap.KB - 1, ap.KB} <= set(p["targets"])
    if p["pj"] is not None:
        assert (p["pj"] != p["pi"]).all()
        if n >= 3 * ap.KB:
            assert (p["pj"] // ap.KB != p["pi"] // ap.KB).all()
    mass = ap.intended_mass(p, base2)
    want = ap.reference(p, base2)
    worst_cf, at_cf, _ = row_errs(want, ap.closed_form(p), heads)
    worst_rs, at_rs, _ = row_errs(ap.flash_restatement(q, k, v, heads, base2), want, heads)
    print(f"{name}: min mass {mass:.8f}, fp64 vs closed form {worst_cf:.2e} at {at_cf}, restatement {worst_rs:.2e} at {at_rs}")
    assert mass >= 0.99, mass
    assert worst_cf < 1e-4, (worst_cf, at_cf)
    assert worst_rs <= 3e-3, (worst_rs, at_rs)
    # the same metric against deliberately wrong references
    vs = v.clone()
    vs[[0, 1]] = vs[[1, 0]]                                            # keys 0 and 1 of tile 0 trade their V rows (a row is pinned to key 0)
    if p["key_tail"] and n == 2:
        vs[1:] = vs[1]
    wrong_swap = ap.attention_base2(q, k, vs, heads) if base2 else ap.reference({**p, "v": vs})
    wrong_drop = ap.attention_base2(q, k[:n - 1], v[:n - 1], heads) if base2 else ap.reference({**p, "k": k[:n - 1], "v": v[:n - 1]})
    for what, wrong in (("swap", wrong_swap), ("drop", wrong_drop)):
        w, at, glob = row_errs(want, wrong, heads)
        print(f"{name}: wrong reference ({what}): worst row {w:.3f} at {at}, global {glob:.2e}")
        assert w > 0.3, (what, w, at)


def test_split_probe_pairs_straddle_the_pieces():
    Lq, Lk, heads = ap.SPLIT_SHAPE
    edge = ap.piece_edges(Lk, 2)
    assert edge == [65 * 64]
    p = ap.build("two", 2.0, Lq, Lk, heads, seed=7, edges=edge)
    assert ((p["pi"] >= edge[0]) != (p["pj"] >= edge[0])).all()          # every row's answer is a merge of the two pieces
    one = ap.build("one", 2.0, Lq, Lk, heads, seed=7, edges=edge)
    assert {edge[0] - 1, edge[0], Lk - 1} <= set(one["pi"].tolist()) and (one["pi"] >= edge[0]).sum() >= 64          # keys of the last, ragged piece


def test_tail_rows_are_probed():
    for Lq, n, m in ap.CROSS_TAILS:
        for kind in ("one", "two"):
            p = ap.build(kind, 2.0, Lq, n - 1 + m, 2, seed=40 + n, key_tail=(n, m))
            assert (p["pi"] == n - 1).any()
            want, cf = ap.reference(p, base2=True), ap.closed_form(p)
            rows = torch.from_numpy(p["pi"] == n - 1)
            tail_v = p["v"][n - 1]
            if kind == "one":
                assert torch.allclose(want[rows], tail_v.expand_as(want[rows]), atol=1e-9)
            else:
                vj = p["v"][torch.from_numpy(p["pj"])][rows]
                assert torch.allclose(want[rows], (m * tail_v + vj) / (m + 1), atol=1e-9) and torch.allclose(cf[rows], want[rows], atol=1e-9)
