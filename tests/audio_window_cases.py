"""The talk variant's clip audio windows, restated for the tests (tests/test_audio_windows_host.py, test_gpu_audio_windows.py, test_gpu_talk_stream.py).

`windows_torch` is the index rule of include/svi_hip.h (svi_audio_windows) in plain torch; `windows_einops` writes out what the reference does —
SVITalkVideoPipeline.get_audio_embedding followed by preprocess_audio and the cast (pipelines/svi_video_talk.py:412-446) — with einops, from its
description: a [frames, 5] table of centre +- 2 indices clamped into the embedding, a fancy-index gather, then the regrouping of the frames behind the
first into groups of four.  tests/test_audio_windows_host.py holds the two against each other on the CPU."""
import torch

# (N audio frames, T latent frames, audio_start_idx): the low clamp, the high clamp, a window wider than the audio, a single audio frame, the real clip length
GPU_CASES = [(30, 3, 0), (30, 3, 25), (7, 4, 3), (1, 2, 0), (200, 21, 77)]
GPU_WIDTHS = [8, 9216]

# per later latent frame: (video frame inside the group of four, window position) of its eight rows
LATTER_ROWS = [(0, 0), (0, 1), (0, 2), (1, 2), (2, 2), (3, 2), (3, 3), (3, 4)]


def window_rows(N: int, T: int, start: int):
    """Source row of every output row: (first [5], latter [T - 1, 8]) as int64 tensors; row(f, w) = clamp(start + f + (w - 2), 0, N - 1)."""
    row = lambda f, w: min(max(start + f + (w - 2), 0), N - 1)      # noqa: E731
    first = torch.tensor([row(0, w) for w in range(5)], dtype=torch.int64)
    latter = torch.tensor([[row(1 + 4 * t + df, w) for df, w in LATTER_ROWS] for t in range(T - 1)], dtype=torch.int64).reshape(T - 1, 8)
    return first, latter


def windows_torch(emb: torch.Tensor, start: int, T: int):
    """(first [1, 5, ...], latter [T - 1, 8, ...]) bf16 of emb [N, ...]: a gather by window_rows and one rounding."""
    first, latter = window_rows(emb.shape[0], T, start)
    return emb[first][None].to(torch.bfloat16), emb[latter].to(torch.bfloat16)


def windows_einops(emb: torch.Tensor, start: int, T: int):
    """The reference's two steps on emb [N, s, c], in its shapes: audio_embed [1, frames, 5, s, c], then ([1, 1, 5, s, c], [1, T - 1, 8, s, c]) bf16."""
    from einops import rearrange
    frames = 4 * (T - 1) + 1
    centre = torch.arange(start, start + frames).unsqueeze(1) + (torch.arange(5) - 2).unsqueeze(0)
    centre = torch.clamp(centre, min=0, max=emb.shape[0] - 1)
    audio = emb[centre][None]                                                  # [1, frames, 5, s, c]
    first, later = audio[:, :1], audio[:, 1:]
    later = rearrange(later, "b (n_t n) w s c -> b n_t n w s c", n=4)
    head = rearrange(later[:, :, :1, :3], "b n_t n w s c -> b n_t (n w) s c")
    middle = rearrange(later[:, :, 1:-1, 2:3], "b n_t n w s c -> b n_t (n w) s c")
    tail = rearrange(later[:, :, -1:, 2:], "b n_t n w s c -> b n_t (n w) s c")
    return first.to(torch.bfloat16), torch.concat([head, middle, tail], dim=2).to(torch.bfloat16)


def host_tuples(emb: torch.Tensor, start: int, T: int):
    """audio_embed_tuple and the null tuple of one clip as the reference's __call__ builds them on the host (svi_video_talk.py:548-550): the windows of
    emb [N, 12, 768], and the same shapes of zeros."""
    first, latter = windows_torch(emb.float().cpu(), start, T)
    aud = (first[None], latter[None])
    return aud, tuple(torch.zeros_like(a) for a in aud)
