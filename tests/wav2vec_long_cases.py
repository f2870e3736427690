"""Shared by tests/gen_golden_wav2vec_long.py and tests/test_gpu_wav2vec_long.py: the audio encoder's cases past 2048 frames, which tensors the fixture keeps
of each, and which rows of a tensor it keeps.  Weights and waveforms are wav2vec_cases' (rebuilt from seeds, never stored).

(name, model, samples, waveform seed, seq_len or None = get_embedding's int(seconds * 25)):
    p   tiny   4000 samples asked for 2049 frames: the first size past the resident attention kernel; the interpolation upsamples 12 frames to 2049
    q   tiny   1 344 000 samples (84 s) by get_embedding's own rule: 4199 convolution frames -> 2100; the first layer has 268 799 rows, the statistics over
               time run over 1313 (waveform) and 263 (GroupNorm) chunks
    r   base widths, one block (12 heads of 64), 16000 samples asked for 2300 frames

What is kept is what fits a fixture of under 1 MB: block l's output is column l of the stack (the test holds stage ("layer", l) to that column), and the
stages between interpolation and the first block are kept where the case is about them (q)."""
from __future__ import annotations

import numpy as np

LONG_INPUTS = (("p", "tiny", 4000, 17, 2049), ("q", "tiny", 1344000, 18, None), ("r", "base1", 16000, 19, 2300))
STAGES = {"p": ("wave", "conv6", "interp", "stack"), "q": ("wave", "conv0", "conv6", "interp", "enc_ln", "stack"), "r": ("conv6", "stack")}
MAX_FRAMES = 4096                                # the limit the tests raise their encoders to


def kept_rows(n: int) -> np.ndarray:
    """Rows of an n-row tensor the fixture keeps: every 16th and the last one; of a tensor of more than 4608 rows (the waveform and the first convolution
    layers of 84 s of audio) every (16 k)th and the last, k the smallest that keeps at most 289 rows."""
    step = 16 * max(1, -(-n // 4608))
    return np.unique(np.concatenate([np.arange(0, n, step), [n - 1]]))
