"""Without a GPU: the clip pose window's rule (include/svi_hip.h, svi_pose_window) as svi_pose_window_plan states it on the host — the same inline functions
the kernel runs — is what the reference's own statements cut (golden/dance_stream.npz, tests/gen_golden_dance_stream.py), is F.interpolate(mode='nearest')
plus the centre pad on a sweep of sizes, and is the script's loop for the frames; and both C entry points refuse bad arguments by name before anything is
launched."""
import ctypes as C

import pytest
import torch

from dance_stream_cases import CASES, CLIPS, frame_table, host_window, planned_window, pose_source, resize_pad, scaled_size
from svi_hip import _lib as L


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_reproduces_the_reference_windows(name, golden):
    g = golden("dance_stream.npz")
    N, h, w, H, W, F, m, _ = CASES[name]
    pose = pose_source(name)
    assert torch.equal(pose, torch.from_numpy(g[f"{name}.pose"]))                       # the seeded source is the one the fixture was cut from
    want = torch.from_numpy(g[f"{name}.windows"])
    assert tuple(want.shape) == (CLIPS, F, H, W, 3)
    for k in range(CLIPS):
        plan = L.pose_window_plan(N, h, w, H, W, F, m, k)
        assert torch.equal(planned_window(pose, plan), want[k]), (name, k)
        # and the tests' own host boundary (the GPU tests' reference) is the fixture too
        assert torch.equal(host_window(pose, k, F, m, H, W), want[k].permute(3, 0, 1, 2).float()), (name, k)
    assert N == 1 or not torch.equal(want[0], want[1])          # the window moves from clip to clip (a one-frame video has one window)


def test_the_cases_are_the_ones_they_claim_to_be():
    """Each case's reason for being there, checked: which axis is padded and by how much, the quirk, the short videos, the two-level carry."""
    geo = {n: scaled_size(c[1], c[2], c[3], c[4]) for n, c in CASES.items()}
    assert geo["pad_w"] == (32, 43, 0, 2) and geo["pad_h_odd"] == (27, 48, 2, 0)
    assert geo["exact_fit"] == (16, 32, 0, 0) and geo["same_size"] == (16, 16, 0, 0) and geo["downscale"] == (14, 32, 1, 0)
    assert geo["trunc_quirk"][0] == 31 and 49 * (32 / 49) < 32 and 32 / 49 < 48 / 60      # the height limits the scale and still loses a row
    assert CASES["upscale_short"][0] < CASES["upscale_short"][5] and CASES["one_frame"][0] == 1
    assert CASES["n_eq_f"][0] == CASES["n_eq_f"][5] and CASES["n_eq_f_plus_1"][0] == CASES["n_eq_f_plus_1"][5] + 1
    N, _, _, _, _, F, m, _ = CASES["upscale_short"]
    assert F - m < m                                             # clip 3's first pose was carried by clip 2, which had it carried from clip 1
    t = frame_table(N, F, m, 4)
    assert t[3][0] == t[2][F - m] == t[1][2 * (F - m)] and 2 * (F - m) >= m and t[1][m] == (F - 1) % N


def test_row_and_column_rule_is_nearest_interpolation_plus_centre_pad():
    """Live against F.interpolate on a sweep: every source size 1..40 into three clip sizes, both orientations, plus the real sizes' axes."""
    pairs = [(h, w, H, W) for H, W in ((16, 16), (32, 48), (48, 32)) for h in range(1, 41) for w in (h, (h * 7) % 41 + 1)]
    pairs += [(1080, 1920, 480, 832), (1920, 1080, 480, 832), (720, 1280, 480, 832), (49, 60, 32, 48), (173, 300, 48, 80)]
    quirks = 0
    for h, w, H, W in pairs:
        # a one-frame video whose pixel values name their own row and column (mod 251 / 241: distinct from their neighbours)
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        pose = torch.stack([yy % 251, xx % 241, (yy + xx) % 239], dim=-1).to(torch.uint8)[None] + 1
        plan = L.pose_window_plan(1, h, w, H, W, 2, 1, 0)
        assert plan["frame_src"] == [0, 0]
        assert torch.equal(planned_window(pose, plan)[0], resize_pad(pose, H, W)[0]), (h, w, H, W)
        nh, nw, top, left = scaled_size(h, w, H, W)
        assert [r >= 0 for r in plan["row_src"]] == [top <= y < top + nh for y in range(H)]
        assert [c >= 0 for c in plan["col_src"]] == [left <= x < left + nw for x in range(W)]
        quirks += (nh < H and nw < W)
    assert quirks >= 1                                           # the truncation left both axes short at least once


def test_frame_rule_is_the_scripts_loop():
    for N in (1, 2, 3, 7, 80, 81, 82, 200):
        for F in (5, 9, 81):
            for m in (1, 2, 4, 5):
                if m >= F:
                    continue
                want = frame_table(N, F, m, 6)
                for k in range(6):
                    assert L.pose_window_plan(N, 16, 16, 16, 16, F, m, k)["frame_src"] == want[k], (N, F, m, k)
    # far down a stream the cursor is still the closed form (64-bit: k (F - m) passes 2^31 / N scales)
    k, F, m, N = 2_000_000_000, 81, 5, 977
    got = L.pose_window_plan(N, 16, 16, 16, 16, F, m, k)["frame_src"]
    assert got[m:] == [((F - 1) + (k - 1) * (F - m) + (i - m)) % N for i in range(m, F)]
    assert got[:m] == [((F - 1) + (k - 2) * (F - m) + (F - m + i - m)) % N for i in range(m)]


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    lib = L.lib()
    P, Q = 4096, 1 << 20                        # never dereferenced: every call below is refused on its arguments
    ok = dict(pose=P, out=Q, N=10, h=20, w=27, H=32, W=48, F=9, m=1, k=0)
    bad = ((dict(N=0), "N = 0"), (dict(F=1), "F = 1"), (dict(m=0), "m = 0"), (dict(m=9), "m = 9"), (dict(k=-1), "k = -1"), (dict(h=0), "h = 0"),
           (dict(w=0), "w = 0"), (dict(H=15), "H = 15"), (dict(W=8), "W = 8"), (dict(h=5000, w=1), "nw = 0"))
    frame, row, col = (C.c_int32 * 16)(), (C.c_int32 * 64)(), (C.c_int32 * 64)()

    def window(**over):
        a = dict(ok, **over)
        return lib.svi_pose_window(a["pose"], a["out"], a["N"], a["h"], a["w"], a["H"], a["W"], a["F"], a["m"], a["k"], None)

    def plan(**over):
        a = dict(ok, **over)
        return lib.svi_pose_window_plan(a["N"], a["h"], a["w"], a["H"], a["W"], a["F"], a["m"], a["k"], a.get("frame", frame), a.get("row", row), a.get("col", col))
    for over, word in bad:
        for fn, who in ((window, "svi_pose_window:"), (plan, "svi_pose_window_plan:")):
            assert fn(**over) == 1, (who, over)
            assert who in L.last_error() and word in L.last_error(), (over, L.last_error())
    for over, word in ((dict(pose=None), "pose is NULL"), (dict(out=None), "out is NULL")):
        assert window(**over) == 1 and word in L.last_error(), (over, L.last_error())
    for name in ("frame", "row", "col"):
        assert plan(**{name: None}) == 1 and "NULL output" in L.last_error(), name
    assert plan() == 0 and list(frame[:9]) == list(range(9))


def test_pose_window_fails_loudly_without_gpu():
    """As test_abi's test_ops_fail_loudly_without_gpu expects of every op: a host tensor is refused by the Python seam, and the C entry point itself,
    given valid arguments on a box without a device, returns an error instead of pretending."""
    import svi_hip
    pose = torch.zeros((4, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        svi_hip.pose_window(pose, 0, 5, 1, 16, 16)
    if not torch.cuda.is_available():
        out = torch.zeros((3, 5, 16, 16))
        assert L.lib().svi_pose_window(pose.data_ptr(), out.data_ptr(), 4, 8, 8, 16, 16, 5, 1, 0, None) != 0 and L.last_error()


def test_seeds_per_clip_is_one_seed_repeated_or_one_per_clip():
    """The talk and the dance stream read their `seed` argument through one helper."""
    from svi_hip.stream import seeds_per_clip
    assert seeds_per_clip(7, 3) == [7, 7, 7] and seeds_per_clip(0, 1) == [0] and seeds_per_clip(5, 0) == []
    got = seeds_per_clip([3, 45.0, torch.tensor(87)], 3)
    assert got == [3, 45, 87] and all(type(s) is int for s in got)
    assert seeds_per_clip((1, 2), 2) == [1, 2]
    for seed, n in (([1], 2), ([1, 2, 3], 2), ([], 1)):
        with pytest.raises(ValueError, match="seeds"):
            seeds_per_clip(seed, n)
