"""Generate tests/golden/dance_stream.npz: the pose windows the REFERENCE's own statements cut for clips 0..3 of a dance stream.

Nothing of the reference is restated here: resize_and_pad_to_target is compiled out of utils/image_process.py (gen_golden._reference_toplevel: executed,
not copied; the module's own imports — cv2, matplotlib, scipy — are not needed), and the script's window statements (test_svi_dance.py:215-227 before the
clip loop, :281-288 at the end of its body) are compiled out of the script by line range, with the script's own module-level `max_frames` replaced by the
case's clip length.  They run on the seeded 8-bit pose videos of tests/dance_stream_cases.py; per case the fixture keeps the source and the four windows
as uint8 [4, F, H, W, 3] (the values are 8-bit integers also where the script holds them as floats).  torch on the CPU only.

    python tests/gen_golden_dance_stream.py
"""
from __future__ import annotations

import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from dance_stream_cases import CASES, CLIPS, pose_source  # noqa: E402
from gen_golden import OUT, REF, _reference_toplevel  # noqa: E402

SCRIPT = "test_svi_dance.py"
FIRST_WINDOW, NEXT_WINDOW = (215, 227), (281, 288)


def _statements(body, first: int, last: int):
    """The outermost statements that lie wholly inside lines first..last, in order, wherever they are nested."""
    out = []
    for node in body:
        if first <= node.lineno and node.end_lineno <= last:
            out.append(node)
        elif node.lineno <= last and node.end_lineno >= first:
            for field in ("body", "orelse", "finalbody"):
                out += _statements(getattr(node, field, []) or [], first, last)
    return out


def reference_statements(lines):
    path = os.path.join(REF, SCRIPT)
    nodes = _statements(ast.parse(open(path).read()).body, *lines)
    assert nodes, lines
    return compile(ast.Module(body=nodes, type_ignores=[]), path, "exec")


def reference_windows(pose_u8: torch.Tensor, H: int, W: int, F: int, m: int, clips: int, first, nxt, resize):
    """Run the script's statements: the names are the script's own."""
    ns = dict(torch=torch, np=np, resize_and_pad_to_target=resize, max_frames=F, misc_size=[H, W], sample_fps=1, num_motion_frames=m,
              humanpose_data_torch=pose_u8.permute(0, 3, 1, 2).contiguous(), rand_ref_frame=np.zeros((H, W, 3), np.uint8), print=lambda *a: None)
    exec(first, ns)
    out = []
    for _ in range(clips):
        win = ns["humanpose_data"]
        assert tuple(win.shape) == (3, F, H, W) and bool((win.float() == win.float().round()).all())
        out.append(win.permute(1, 2, 3, 0).to(torch.uint8).numpy().copy())
        exec(nxt, ns)
    return np.stack(out)


def main():
    resize = _reference_toplevel("utils/image_process.py", "resize_and_pad_to_target", {"F": torch.nn.functional, "torch": torch})
    first, nxt = reference_statements(FIRST_WINDOW), reference_statements(NEXT_WINDOW)
    out = {}
    for name, (N, h, w, H, W, F, m, _) in CASES.items():
        pose = pose_source(name)
        wins = reference_windows(pose, H, W, F, m, CLIPS, first, nxt, resize)
        out[f"{name}.pose"] = pose.numpy()
        out[f"{name}.windows"] = wins
        rows, cols = np.flatnonzero(wins[0, 0].any(axis=(1, 2))), np.flatnonzero(wins[0, 0].any(axis=(0, 2)))
        print(f"{name}: {N} x {h} x {w} -> {CLIPS} x {F} x {H} x {W}, m = {m}: rows {rows[0]}..{rows[-1]}, columns {cols[0]}..{cols[-1]} written")
    path = os.path.join(OUT, "dance_stream.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
