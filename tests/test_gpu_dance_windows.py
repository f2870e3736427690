"""-m gpu: the clip pose window cut on the device (svi_pose_window; svi_hip.pose_window, PoseEmbedder.window).

The kernel is a gather of 8-bit values into floats, so everything is compared with torch.equal: against the windows the reference's own statements cut
(golden/dance_stream.npz), against the host boundary of tests/dance_stream_cases.py (held to that fixture in tests/test_dance_windows_host.py), and —
for the embedder — against PoseEmbedder.__call__ on the window built on the host."""
import pytest
import torch

import synth
from dance_stream_cases import CASES, CLIPS, host_window, planned_window, pose_source

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(CASES))
def test_windows_are_the_reference_windows(name, golden):
    import svi_hip
    N, h, w, H, W, F, m, _ = CASES[name]
    want = torch.from_numpy(golden("dance_stream.npz")[f"{name}.windows"])             # uint8 [CLIPS, F, H, W, 3]
    pose = pose_source(name).cuda()
    into = torch.full((3, F, H, W), -5.0, device="cuda")
    for k in range(CLIPS):
        got = svi_hip.pose_window(pose, k, F, m, H, W)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, F, H, W)
        assert torch.equal(got.cpu(), want[k].permute(3, 0, 1, 2).float()), (name, k)
        # into a caller's buffer: the same bits, the same tensor, every element written (clip k - 1's values and the first fill are gone)
        back = svi_hip.pose_window(pose, k, F, m, H, W, out=into)
        assert back is into and torch.equal(into, got), (name, k)


@pytest.mark.parametrize("shape", [(32, 48, 0), (32, 48, 1), (17, 18, 0), (16, 22, 3)], ids=["aligned", "off-by-4-bytes", "w18", "w22-off-by-12"])
def test_nothing_outside_out_is_written(shape):
    """The C entry point on a caller-owned buffer with sentinel floats on either side of `out`: 16-byte stores where W % 4 == 0 and out is 16-byte
    aligned, 4-byte stores otherwise (an out that is not, a width that is no multiple of 4: the last lane of a row owns fewer than four columns)."""
    from svi_hip import _lib as L
    H, W, shift = shape
    N, h, w, _, _, F, m, _ = CASES["pad_w"]
    pose = pose_source("pad_w")
    dev = pose.cuda()
    GUARD, SENTINEL = 64, -7.0
    n = 3 * F * H * W
    buf = torch.full((GUARD + shift + n + GUARD,), SENTINEL, device="cuda")
    out = buf[GUARD + shift:GUARD + shift + n]
    assert (out.data_ptr() % 16 == 0) == (shift == 0)
    for k in (0, 2):
        buf.fill_(SENTINEL)
        L.check(L.lib().svi_pose_window(dev.data_ptr(), out.data_ptr(), N, h, w, H, W, F, m, k, L.current_stream()), "svi_pose_window")
        assert torch.equal(out.cpu().reshape(3, F, H, W), host_window(pose, k, F, m, H, W)), (shape, k)
        assert bool((buf[:GUARD + shift] == SENTINEL).all()) and bool((buf[GUARD + shift + n:] == SENTINEL).all()), (shape, k)


def test_source_offsets_beyond_2_to_31_bytes():
    """9 frames of 9000 x 9000 x 3 bytes = 2.19 GB: the last frame starts at byte 1.94e9 and its rows from 7527 on lie beyond 2^31.  Zeros except a random
    pattern in the last frame; clip 2 of F = 5, m = 1 reads frames 7, 8, 0, 1, 2: frame 8 lands in window frame 1, sampled down to 16 x 16."""
    import svi_hip
    from svi_hip import _lib as L
    N, S, F, m, k = 9, 9000, 5, 1, 2
    plan = L.pose_window_plan(N, S, S, 16, 16, F, m, k)
    assert plan["frame_src"] == [7, 8, 0, 1, 2]
    rows = [r for r in plan["row_src"] if r >= 0]
    assert ((N - 1) * S + max(rows)) * S * 3 > 2 ** 31 and N * S * S * 3 < 2 ** 32
    pose = torch.zeros((N, S, S, 3), dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(11)
    pose[N - 1] = torch.randint(1, 256, (S, S, 3), generator=g, device="cuda", dtype=torch.uint8)
    got = svi_hip.pose_window(pose, k, F, m, 16, 16).cpu()
    last = pose[N - 1].cpu()[None]
    want = planned_window(last, dict(plan, frame_src=[0]))[0].permute(2, 0, 1).float()       # [3, 16, 16] of the last frame
    assert torch.equal(got[:, 1], want) and int(want.count_nonzero()) >= 3 * 15 * 15         # the pattern has no zero; a row / column may be padding
    assert not got[:, [0, 2, 3, 4]].any()
    del pose
    torch.cuda.empty_cache()


def test_embedder_window_is_the_embedder_on_the_host_built_window():
    import svi_hip
    sd = {k: torch.from_numpy(v) for k, v in synth.pose_state_dict(synth.POSE_SEED, dim=128).items()}
    emb = svi_hip.PoseEmbedder.from_state_dict(sd)
    for name in ("pad_w", "upscale_short"):
        N, h, w, H, W, F, m, _ = CASES[name]
        pose = pose_source(name)
        dev = pose.cuda()
        for k in (0, 1, 3):
            got = emb.window(dev, k, F, m, H, W)
            want = emb(host_window(pose, k, F, m, H, W).cuda())
            assert got.dtype == torch.bfloat16 and tuple(got.shape) == (1, 3 * 2 * 3, 128)
            assert torch.equal(got, want), (name, k)
        assert len(emb._windows) == 1                              # one window buffer per shape, reused by every clip and both videos
    a, b = emb.window(dev, 0, F, m, H, W), emb.window(dev, 1, F, m, H, W)
    assert not torch.equal(a, b)                                   # the window reaches the condition


def test_python_seam_refuses_what_the_kernel_cannot_take():
    import svi_hip
    pose = pose_source("pad_w").cuda()
    with pytest.raises(ValueError, match="uint8"):
        svi_hip.pose_window(pose.float(), 0, 9, 1, 32, 48)
    with pytest.raises(ValueError, match="uint8"):
        svi_hip.pose_window(pose[..., :2], 0, 9, 1, 32, 48)
    with pytest.raises(ValueError, match="contiguous"):
        svi_hip.pose_window(pose[:, ::2], 0, 9, 1, 32, 48)
    with pytest.raises(ValueError, match="out must be"):
        svi_hip.pose_window(pose, 0, 9, 1, 32, 48, out=torch.zeros((3, 9, 32, 40), device="cuda"))
    with pytest.raises(RuntimeError, match="m = 9"):
        svi_hip.pose_window(pose, 0, 9, 9, 32, 48)
    with pytest.raises(RuntimeError, match="k = -1"):
        svi_hip.pose_window(pose, -1, 9, 1, 32, 48)
    with pytest.raises(RuntimeError, match="H = 8"):
        svi_hip.pose_window(pose, 0, 9, 1, 8, 48)
