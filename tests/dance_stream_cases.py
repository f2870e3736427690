"""The dance variant's clip pose windows, restated for the tests (tests/test_dance_windows_host.py, test_gpu_dance_windows.py, test_gpu_dance_stream.py)
and for the generator of their fixture (tests/gen_golden_dance_stream.py -> tests/golden/dance_stream.npz: the windows the reference's own statements
cut, clips 0..3 of every case below).

`frame_table` is the script's loop between two clips written out plainly (the last m poses carried over, the rest read on from a cursor that wraps over
the repeat-padded video); `host_window` is the whole boundary on the host — that table, F.interpolate(mode='nearest') to the scaled size, the centre
pad, the float conversion.  tests/test_dance_windows_host.py holds both against the fixture and against svi_pose_window_plan on the CPU."""
import numpy as np
import torch

CLIPS = 4         # clip indices 0..3 of every case are in the fixture

# name: (N pose frames, source h, w, clip H, W, F frames per clip, m motion frames, seed) — the smallest shapes at which the rule can go wrong
CASES = {
    # a non-integer scale (1.6), padding on one axis only: nh = 32, nw = 43, 2 columns left and 3 right; the video is read 2.9 times over by clip 3
    "pad_w": (23, 20, 27, 32, 48, 9, 1, 9101),
    # the other axis padded, odd total: nw = 48, nh = int(17 * 1.6) = 27, 2 rows above and 3 below
    "pad_h_odd": (12, 17, 30, 32, 48, 5, 2, 9102),
    # upscaling (x 3.56) of a video shorter than a clip: repeat-padding, the wrap inside clip 1, and F - m = 4 < m = 5: by clip 3 a carried pose is one
    # that was carried before (the recursion of the frame rule runs more than one level)
    "upscale_short": (7, 9, 11, 32, 48, 9, 5, 9103),
    "one_frame": (1, 10, 13, 16, 32, 5, 2, 9104),
    "n_eq_f": (5, 12, 20, 16, 32, 5, 1, 9105),
    "n_eq_f_plus_1": (6, 12, 20, 16, 32, 5, 3, 9106),
    # an exact fit: x 2 on both axes, no padding (ATen's nearest takes its own branch for equal and for doubled sizes)
    "exact_fit": (8, 8, 16, 16, 32, 5, 4, 9107),
    "same_size": (6, 16, 16, 16, 16, 5, 1, 9108),
    # downscaling by a non-integer factor, W-limited: nw = 32, nh = int(31 * (32 / 70)) = 14
    "downscale": (11, 31, 70, 16, 32, 5, 2, 9109),
    # the truncation quirk: 49 * (32 / 49) = 31.999999999999996, so nh = 31 although the height limits the scale: one padded row at the bottom.
    # A search over h, H <= 2000 finds 210026 such pairs (int(h * (H / h)) == H - 1); with H a multiple of 16 the smallest h is 49.
    "trunc_quirk": (5, 49, 60, 32, 48, 5, 1, 9110),
}


def pose_source(name: str) -> torch.Tensor:
    """The case's seeded pose video, uint8 [N, h, w, 3] as a video reader hands it over.  Dense values: every pixel tells its neighbours apart."""
    N, h, w, _, _, _, _, seed = CASES[name]
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, size=(N, h, w, 3)).astype(np.uint8))


def frame_table(N: int, F: int, m: int, clips: int):
    """Source frame of every window frame of clips 0 .. clips - 1, as the script's statements produce it: [clips][F] ints."""
    length = N if N >= F else (F // N + 1) * N                 # a video shorter than a clip is repeated until it is longer
    padded = [j % N for j in range(length)]
    window = padded[:F]
    cursor = F - 1                                             # the script's: the last frame of clip 0 is read again
    table = [window]
    for _ in range(1, clips):
        nxt = window[F - m:]
        for _ in range(m, F):
            cursor %= length
            nxt.append(padded[cursor])
            cursor += 1
        window = nxt
        table.append(window)
    return table


def scaled_size(h: int, w: int, H: int, W: int):
    """(nh, nw, pad_top, pad_left) of resize_and_pad_to_target: the scale and the products in Python's double arithmetic."""
    s = min(H / h, W / w)
    nh, nw = int(h * s), int(w * s)
    return nh, nw, (H - nh) // 2, (W - nw) // 2


def resize_pad(pose_u8: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """uint8 [N, h, w, 3] -> uint8 [N, H, W, 3]: nearest to the scaled size, zeros around it."""
    import torch.nn.functional as F
    N, h, w, _ = pose_u8.shape
    nh, nw, top, left = scaled_size(h, w, H, W)
    small = F.interpolate(pose_u8.permute(0, 3, 1, 2), size=(nh, nw), mode="nearest")
    out = torch.zeros((N, 3, H, W), dtype=torch.uint8)
    out[:, :, top:top + nh, left:left + nw] = small
    return out.permute(0, 2, 3, 1).contiguous()


def host_window(pose_u8: torch.Tensor, k: int, F: int, m: int, H: int, W: int) -> torch.Tensor:
    """Clip k's humanpose_data fp32 [3, F, H, W] (values 0..255), built on the host."""
    frames = frame_table(pose_u8.shape[0], F, m, k + 1)[k]
    return resize_pad(pose_u8.cpu(), H, W)[frames].permute(3, 0, 1, 2).float().contiguous()


def planned_window(pose_u8: torch.Tensor, plan: dict) -> torch.Tensor:
    """The window a svi_pose_window_plan result describes: uint8 [F, H, W, 3], gathered from the source by frame_src / row_src / col_src (-1: zero)."""
    f, r, c = (torch.tensor(plan[n], dtype=torch.int64) for n in ("frame_src", "row_src", "col_src"))
    got = pose_u8[f][:, r.clamp(min=0)][:, :, c.clamp(min=0)]
    keep = (r >= 0)[None, :, None, None] & (c >= 0)[None, None, :, None]
    return got * keep
