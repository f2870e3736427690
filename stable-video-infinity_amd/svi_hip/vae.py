"""WanVideoVAE on libsvi_hip: same encode/decode signatures as the reference class
(diffsynth/models/wan_video_vae.py:599-789).

    WanVideoVAE.from_state_dict(sd)    <- WanVideoVAE().load_state_dict(sd)
    WanVideoVAE.from_module(ref_vae)   <- borrow the fp32 parameters of a reference WanVideoVAE on the GPU
    .encode(videos, device, tiled=False, tile_size, tile_stride) -> Tensor[N,16,T',h,w]      vae:759-774
    .decode(hidden_states, device, tiled=False, tile_size, tile_stride) -> Tensor[N,3,T,H,W] vae:777-789
    .decode(..., split=(ph, pw), group=None) / .decode_part(latent, split, part, out=None)   exact spatial split over ranks (not in the reference)
    .encode(..., split=(ph, pw), group=None) / .encode_part(video, split, part, out=None) / .encode_tail(feat)   the same for the encode

The whole clip stays resident in HBM (no temporal chunking, no feature cache: see csrc/svi_vae.hip).  `tiled=True`
is the reference's spatial tiling and linear-ramp blending (vae:621-744) in one C call (svi_vae_tiled_decode / _encode): tiles are read
in place, decoded by the same kernels and blended on the GPU with the reference's fp32 arithmetic and task order.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib as L


def vae_param_shapes() -> Dict[str, tuple]:
    """Parameter inventory of the reference architecture (dim 96, z 16, mult 1,2,4,4; vae:494-517)."""
    s: Dict[str, tuple] = {}

    def conv3(n, o, i, k=(3, 3, 3)):
        s[n + ".weight"] = (o, i, *k); s[n + ".bias"] = (o,)

    def conv2(n, o, i, k=3):
        s[n + ".weight"] = (o, i, k, k); s[n + ".bias"] = (o,)

    def res(p, i, o):
        s[p + "residual.0.gamma"] = (i, 1, 1, 1); conv3(p + "residual.2", o, i)
        s[p + "residual.3.gamma"] = (o, 1, 1, 1); conv3(p + "residual.6", o, o)
        if i != o:
            conv3(p + "shortcut", o, i, (1, 1, 1))

    def attn(p, c):
        s[p + "norm.gamma"] = (c, 1, 1); conv2(p + "to_qkv", 3 * c, c, 1); conv2(p + "proj", c, c, 1)

    base, z, mult, tdown = 96, 16, (1, 2, 4, 4), (False, True, True)
    e, d = "model.encoder.", "model.decoder."
    dims = [base * u for u in (1,) + mult]
    conv3(e + "conv1", dims[0], 3)
    idx = 0
    for i, (di, do) in enumerate(zip(dims[:-1], dims[1:])):
        for _ in range(2):
            res(f"{e}downsamples.{idx}.", di, do); idx += 1; di = do
        if i != 3:
            conv2(f"{e}downsamples.{idx}.resample.1", do, do)
            if tdown[i]:
                conv3(f"{e}downsamples.{idx}.time_conv", do, do, (3, 1, 1))
            idx += 1
    top = dims[-1]
    res(e + "middle.0.", top, top); attn(e + "middle.1.", top); res(e + "middle.2.", top, top)
    s[e + "head.0.gamma"] = (top, 1, 1, 1); conv3(e + "head.2", 2 * z, top)
    conv3("model.conv1", 2 * z, 2 * z, (1, 1, 1)); conv3("model.conv2", z, z, (1, 1, 1))
    dims = [base * u for u in (mult[-1],) + mult[::-1]]
    conv3(d + "conv1", dims[0], z)
    res(d + "middle.0.", dims[0], dims[0]); attn(d + "middle.1.", dims[0]); res(d + "middle.2.", dims[0], dims[0])
    idx, tup = 0, tdown[::-1]
    for i, (di, do) in enumerate(zip(dims[:-1], dims[1:])):
        if i >= 1:
            di //= 2
        for _ in range(3):
            res(f"{d}upsamples.{idx}.", di, do); idx += 1; di = do
        if i != 3:
            conv2(f"{d}upsamples.{idx}.resample.1", do // 2, do)
            if tup[i]:
                conv3(f"{d}upsamples.{idx}.time_conv", do * 2, do, (3, 1, 1))
            idx += 1
    s[d + "head.0.gamma"] = (dims[-1], 1, 1, 1); conv3(d + "head.2", 3, dims[-1])
    return s


def device_vae_weights(seed: int, device) -> Dict[str, torch.Tensor]:
    """Random-init fp32 weights of the VAE architecture, generated on the GPU (bench / smoke only)."""
    g = torch.Generator(device=device).manual_seed(seed)
    out = {}
    for name, shape in vae_param_shapes().items():
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "gamma":
            t = 1.0 + 0.1 * torch.randn(shape, generator=g, device=device)
        elif leaf == "weight":
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            t = (torch.rand(shape, generator=g, device=device) * 2 - 1) / math.sqrt(fan_in)
        else:
            t = (torch.rand(shape, generator=g, device=device) * 2 - 1) * 0.05
        out[name] = t.float().contiguous()
    return out


def encoder_feature_channels() -> int:
    """Channels of the feature map entering the encoder's middle block (what encode_part writes and encode_tail reads)."""
    return vae_param_shapes()["model.encoder.middle.0.residual.2.weight"][1]


def default_vae_split(world: int) -> tuple:
    """The decode grid of a latency-mode group of `world` ranks: 2 -> 1 x 2, 4 -> 2 x 2, 8 -> 2 x 4, otherwise 1 x P along the width."""
    return {2: (1, 2), 4: (2, 2), 8: (2, 4)}.get(int(world), (1, int(world)))


def _encode_split_setting(vae_encode_split, group) -> dict:
    """What the conditioning encode passes on to WanVideoVAE.encode: nothing (the default), or split (+ group)."""
    if vae_encode_split is None or vae_encode_split is False:
        return {}
    if vae_encode_split is True:
        if group is None:
            raise ValueError("vae_encode_split=True takes its grid from a process group (vae_group or a latency mode); name a grid (parts_h, parts_w) to split locally")
        import torch.distributed as dist
        vae_encode_split = default_vae_split(dist.get_world_size(group))
    split = (int(vae_encode_split[0]), int(vae_encode_split[1]))
    return dict(split=split, group=None if split == (1, 1) else group)


def latency_group(loop):
    """The process group whose ranks share every clip of a DenoiseLoop (its CFG pair, else its sequence-parallel group; the world when that is
    None) — the ranks that would otherwise wait for one of them to decode.  None for a single-rank loop."""
    import torch.distributed as dist
    if getattr(loop, "cfg_pair", None) is not None:
        return loop.cfg_pair.group if loop.cfg_pair.group is not None else dist.group.WORLD
    if getattr(loop, "sequence_parallel", False):
        return loop.sp_group if loop.sp_group is not None else dist.group.WORLD
    return None


class WanVideoVAE:
    upsampling_factor = 8

    def __init__(self):
        h = C.c_void_p()
        L.check(L.lib().svi_vae_create(C.byref(h)), "svi_vae_create")
        self._h = h
        self._params: Dict[str, torch.Tensor] = {}

    @classmethod
    def from_state_dict(cls, state_dict: Dict[str, torch.Tensor], device="cuda") -> "WanVideoVAE":
        v = cls()
        v.bind({k: t.to(device=device, dtype=torch.float32).contiguous() for k, t in state_dict.items()})
        return v

    @classmethod
    def from_module(cls, ref_vae) -> "WanVideoVAE":
        v = cls()
        v.bind({k: t.to(device="cuda", dtype=torch.float32).contiguous() for k, t in ref_vae.state_dict().items()})
        return v

    def bind(self, state_dict: Dict[str, torch.Tensor]) -> None:
        lib = L.lib()
        for name, t in state_dict.items():
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError(f"VAE parameter {name} must be a contiguous CUDA fp32 tensor")
            shape = (C.c_int64 * t.dim())(*t.shape)
            L.check(lib.svi_vae_bind_weight(self._h, name.encode(), t.data_ptr(), L.SVI_F32, shape, t.dim()), f"bind {name}")
            self._params[name] = t
        L.check(lib.svi_vae_check_bound(self._h), "svi_vae_check_bound")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                L.lib().svi_vae_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---- single (whole-frame) paths: vae:747-756 ----------------------------------------------------------------
    def single_decode(self, hidden_state: torch.Tensor, device=None) -> torch.Tensor:
        """[1,16,T,h,w] -> [1,3,1+4(T-1),8h,8w] fp32, clamped to [-1,1]."""
        z = hidden_state.to(device="cuda", dtype=torch.float32).contiguous()
        _, c, t, h, w = z.shape
        if c != 16:
            raise ValueError("latents must have 16 channels")
        out = torch.empty((1, 3, 1 + 4 * (t - 1), 8 * h, 8 * w), dtype=torch.float32, device=z.device)
        L.check(L.lib().svi_vae_decode(self._h, L.ptr(z), L.ptr(out), t, h, w, L.current_stream()), "svi_vae_decode")
        return out

    def single_encode(self, video: torch.Tensor, device=None) -> torch.Tensor:
        """[1,3,1+4k,H,W] -> [1,16,1+k,H/8,W/8] fp32."""
        v = video.to(device="cuda", dtype=torch.float32).contiguous()
        _, c, t, h, w = v.shape
        if c != 3:
            raise ValueError("video must have 3 channels")
        out = torch.empty((1, 16, 1 + (t - 1) // 4, h // 8, w // 8), dtype=torch.float32, device=v.device)
        L.check(L.lib().svi_vae_encode(self._h, L.ptr(v), L.ptr(out), t, h, w, L.current_stream()), "svi_vae_encode")
        return out

    # ---- spatial tiling: vae:621-744 (one C call each; tiles, masks and the blend run on the device) ---------------------
    def tiled_decode(self, hidden_states: torch.Tensor, device, tile_size, tile_stride) -> torch.Tensor:
        """[1,16,T,h,w] -> [1,3,4T-3,8h,8w]; tile_size / tile_stride in latent pixels (vae:643-693)."""
        z = hidden_states.to(device="cuda", dtype=torch.float32).contiguous()
        _, c, t, h, w = z.shape
        if c != 16:
            raise ValueError("latents must have 16 channels")
        out = torch.empty((1, 3, 4 * t - 3, 8 * h, 8 * w), dtype=torch.float32, device=z.device)
        L.check(L.lib().svi_vae_tiled_decode(self._h, L.ptr(z), L.ptr(out), t, h, w, int(tile_size[0]), int(tile_size[1]),
                                             int(tile_stride[0]), int(tile_stride[1]), L.current_stream()), "svi_vae_tiled_decode")
        return out

    def tiled_encode(self, video: torch.Tensor, device, tile_size, tile_stride) -> torch.Tensor:
        """[1,3,T,H,W] -> [1,16,(T+3)//4,H/8,W/8]; tile_size / tile_stride in video pixels (vae:696-744)."""
        v = video.to(device="cuda", dtype=torch.float32).contiguous()
        _, c, t, h, w = v.shape
        if c != 3:
            raise ValueError("video must have 3 channels")
        out = torch.empty((1, 16, (t + 3) // 4, h // 8, w // 8), dtype=torch.float32, device=v.device)
        L.check(L.lib().svi_vae_tiled_encode(self._h, L.ptr(v), L.ptr(out), t, h, w, int(tile_size[0]), int(tile_size[1]),
                                             int(tile_stride[0]), int(tile_stride[1]), L.current_stream()), "svi_vae_tiled_encode")
        return out

    # ---- public surface: vae:759-789 ----------------------------------------------------------------------------------
    def encode(self, videos: Sequence[torch.Tensor], device=None, tiled=False, tile_size=(34, 34), tile_stride=(18, 16), split=None, group=None):
        """split = (parts_h, parts_w): the exact spatial split (see split_encode); group: the process group whose ranks each encode one part."""
        if split is not None and tiled:
            raise ValueError("VAE encode: tiled=True blends overlapping tiles, split=(ph, pw) is the exact rank split; ask for one of them")
        if split is None and group is not None:
            raise ValueError("VAE encode: a group needs split=(parts_h, parts_w)")
        outs: List[torch.Tensor] = []
        for video in videos:
            video = video.unsqueeze(0)
            if split is not None:
                hs = self.split_encode(video, split, group)
            elif tiled:
                # as the reference (vae:765-767): the x8 is applied to the loop's own variables, so from the second video of a
                # batch on the tiles are 8x larger again (one tile per video in practice); kept, it is observable behaviour
                tile_size = (tile_size[0] * 8, tile_size[1] * 8)
                tile_stride = (tile_stride[0] * 8, tile_stride[1] * 8)
                hs = self.tiled_encode(video, device, tile_size, tile_stride)
            else:
                hs = self.single_encode(video, device)
            outs.append(hs.squeeze(0))
        return torch.stack(outs)

    # ---- exact spatial split for the multi-rank latency modes (svi_vae_split_plan / svi_vae_decode_part) --------------------------------
    def decode_part(self, hidden_state: torch.Tensor, split, part: int, out: Optional[torch.Tensor] = None, _short_halo: int = 0) -> torch.Tensor:
        """Part `part` (row-major) of a split = (parts_h, parts_w) decode of ONE latent [16,T,h,w] or [1,16,T,h,w] (always the whole latent: the
        middle block attends over the frame).  out=None: a tight [3,T',oh,ow] tensor of the owned window.  out = a [3,T',H,W] tensor with
        H >= oh, W >= ow: the full frame [3,T',8h,8w] receives the window at its place, any other size (an all-gather buffer) at its origin;
        nothing outside the window is written.  `_short_halo` is for tests only: decode with the stage 0 halo that many latent pixels short."""
        z = hidden_state.to(device="cuda", dtype=torch.float32)
        z = (z[0] if z.dim() == 5 else z).contiguous()
        c, t, h, w = z.shape
        if c != 16:
            raise ValueError("latents must have 16 channels")
        ph, pw = int(split[0]), int(split[1])
        plan = L.vae_split_plan(h, w, ph, pw, int(part))
        h0, h1, w0, w1 = plan["owned"]
        oh, ow, tv = 8 * (h1 - h0), 8 * (w1 - w0), 1 + 4 * (t - 1)
        if out is None:
            out = torch.empty((3, tv, oh, ow), dtype=torch.float32, device=z.device)
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 4 and out.shape[0] == 3 and out.shape[1] == tv
                and out.shape[2] >= oh and out.shape[3] >= ow):
            raise ValueError(f"decode_part: out must be a contiguous CUDA fp32 [3, {tv}, >= {oh}, >= {ow}] tensor, got {tuple(out.shape)}")
        ld_h, ld_w = out.shape[2], out.shape[3]
        full = (ld_h, ld_w) == (8 * h, 8 * w)
        dst = out.data_ptr() + 4 * ((8 * h0) * ld_w + 8 * w0) if full else out.data_ptr()
        if _short_halo:
            s0 = plan["padded"][0]
            own = plan["owned"]
            cut = [min(s0[0] + _short_halo, own[0]), max(s0[1] - _short_halo, own[1]), min(s0[2] + _short_halo, own[2]), max(s0[3] - _short_halo, own[3])]
            flat = list(own) + list(plan["halo"]) + cut + [v for r in plan["padded"][1:] for v in r]
            L.check(L.lib().svi_vae_decode_planned(self._h, L.ptr(z), dst, t, h, w, (C.c_int32 * 24)(*flat), ld_h, ld_w, L.current_stream()), "svi_vae_decode_planned")
        else:
            L.check(L.lib().svi_vae_decode_part(self._h, L.ptr(z), dst, t, h, w, ph, pw, int(part), ld_h, ld_w, L.current_stream()), "svi_vae_decode_part")
        return out

    def split_decode(self, hidden_state: torch.Tensor, split, group=None) -> torch.Tensor:
        """[1,16,T,h,w] -> [1,3,T',8h,8w].  group=None: every part in this process, one after another, into one frame (the local schedule: tests and
        timing).  With a process group of parts_h x parts_w ranks: this rank's part into a tight buffer, one all-gather, the frame assembled on
        every rank."""
        z = hidden_state.to(device="cuda", dtype=torch.float32).contiguous()
        _, c, t, h, w = z.shape
        ph, pw = int(split[0]), int(split[1])
        n = ph * pw
        if group is not None:                            # refuse a mismatch before any collective
            import torch.distributed as dist
            world = dist.get_world_size(group)
            if world != n:
                raise ValueError(f"VAE split {ph} x {pw} needs a group of {n} ranks, this one has {world}")
        if n == 1:
            return self.single_decode(z)
        tv = 1 + 4 * (t - 1)
        out = torch.empty((1, 3, tv, 8 * h, 8 * w), dtype=torch.float32, device=z.device)
        if group is None:
            for p in range(n):
                self.decode_part(z, (ph, pw), p, out=out[0])
            return out
        import torch.distributed as dist
        from .sequence_parallel import GroupTransport, _wait
        owned = [L.vae_split_plan(h, w, ph, pw, p)["owned"] for p in range(n)]
        mh, mw = 8 * max(o[1] - o[0] for o in owned), 8 * max(o[3] - o[2] for o in owned)
        if (mh, mw) == (8 * h, 8 * w):                   # (cannot happen for n > 1; keeps a gather buffer from being taken for the full frame)
            raise ValueError("VAE split: a part as large as the frame")
        mine = torch.zeros((3, tv, mh, mw), dtype=torch.float32, device=z.device)   # parts are unequal when the grid does not divide: one size for the gather
        self.decode_part(z, (ph, pw), dist.get_rank(group), out=mine)
        parts = torch.empty((n,) + tuple(mine.shape), dtype=torch.float32, device=z.device)
        _wait(GroupTransport(group).all_gather([parts], [mine]))
        for p, (h0, h1, w0, w1) in enumerate(owned):
            out[0, :, :, 8 * h0:8 * h1, 8 * w0:8 * w1] = parts[p, :, :, :8 * (h1 - h0), :8 * (w1 - w0)]
        return out

    def decode(self, hidden_states, device=None, tiled=False, tile_size=(34, 34), tile_stride=(18, 16), split=None, group=None):
        """split = (parts_h, parts_w): the exact spatial split (see split_decode); group: the process group whose ranks each decode one part."""
        if split is not None and tiled:
            raise ValueError("VAE decode: tiled=True blends overlapping tiles, split=(ph, pw) is the exact rank split; ask for one of them")
        if split is None and group is not None:
            raise ValueError("VAE decode: a group needs split=(parts_h, parts_w)")
        outs: List[torch.Tensor] = []
        for hs in hidden_states:
            hs = hs.unsqueeze(0)
            if split is not None:
                video = self.split_decode(hs, split, group)
            elif tiled:
                video = self.tiled_decode(hs, device, tile_size, tile_stride)
            else:
                video = self.single_decode(hs, device)
            outs.append(video.squeeze(0))
        return torch.stack(outs)

    # ---- the same for the encode (svi_vae_encode_split_plan / svi_vae_encode_part / svi_vae_encode_tail) --------------------------------
    def encode_part(self, video: torch.Tensor, split, part: int, out: Optional[torch.Tensor] = None, _short_halo: int = 0) -> torch.Tensor:
        """Part `part` (row-major) of a split = (parts_h, parts_w) encode of ONE video [3,T,H,W] or [1,3,T,H,W] (always the whole video: the part's
        window is read in place): conv1 and the down stages on the crop -> the owned window of the feature map entering the encoder's middle
        block, channels-last fp32.  out=None: a tight [T',oh,ow,C] tensor.  out = a [T',h,w,C] tensor with h >= oh, w >= ow: the full map
        [T',H/8,W/8,C] receives the window at its place, any other size (an all-gather slot) at its origin; nothing outside the window is written.
        `_short_halo` is for tests only: encode with only that many video pixels of halo (a multiple of 8; the later rectangles shrink with it)."""
        v = video.to(device="cuda", dtype=torch.float32)
        v = (v[0] if v.dim() == 5 else v).contiguous()
        c, t, H, W = v.shape
        if c != 3:
            raise ValueError("video must have 3 channels")
        if (t - 1) % 4 or H % 8 or W % 8:
            raise ValueError(f"encode_part: needs T = 1+4k frames and H, W multiples of 8 (got {t}, {H}, {W})")
        ph, pw = int(split[0]), int(split[1])
        h, w = H // 8, W // 8
        plan = L.vae_encode_split_plan(h, w, ph, pw, int(part))
        h0, h1, w0, w1 = plan["owned"]
        oh, ow, tl, ch = h1 - h0, w1 - w0, 1 + (t - 1) // 4, encoder_feature_channels()
        if out is None:
            out = torch.empty((tl, oh, ow, ch), dtype=torch.float32, device=v.device)
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 4 and out.shape[0] == tl and out.shape[3] == ch
                and out.shape[1] >= oh and out.shape[2] >= ow):
            raise ValueError(f"encode_part: out must be a contiguous CUDA fp32 [{tl}, >= {oh}, >= {ow}, {ch}] tensor, got {tuple(out.shape)}")
        ld_h, ld_w = out.shape[1], out.shape[2]
        full = (ld_h, ld_w) == (h, w)
        dst = out.data_ptr() + 4 * ch * (h0 * ld_w + w0) if full else out.data_ptr()
        if _short_halo:
            if _short_halo % 8:
                raise ValueError("encode_part: _short_halo is in video pixels, a multiple of 8")
            rects = []
            for k, (a0, a1, b0, b1) in enumerate(plan["rects"]):
                f = 8 if k == 0 else 8 >> (k - 1)
                n = _short_halo * f // 8
                rects += [max(a0, h0 * f - n), min(a1, h1 * f + n), max(b0, w0 * f - n), min(b1, w1 * f + n)]
            flat = list(plan["owned"]) + [x for r in plan["reach"] for x in r] + rects
            L.check(L.lib().svi_vae_encode_planned(self._h, L.ptr(v), dst, t, H, W, (C.c_int32 * 34)(*flat), ld_h, ld_w, L.current_stream()), "svi_vae_encode_planned")
        else:
            L.check(L.lib().svi_vae_encode_part(self._h, L.ptr(v), dst, t, H, W, ph, pw, int(part), ld_h, ld_w, L.current_stream()), "svi_vae_encode_part")
        return out

    def encode_tail(self, feat: torch.Tensor) -> torch.Tensor:
        """The assembled feature map [T',h,w,C] (channels-last fp32, what the parts of encode_part tile) -> latents [16,T',h,w]: the encoder's middle
        block, head and model.conv1 on the whole frame."""
        f = feat.to(device="cuda", dtype=torch.float32).contiguous()
        if f.dim() != 4 or f.shape[3] != encoder_feature_channels():
            raise ValueError(f"encode_tail: feat must be [T', h, w, {encoder_feature_channels()}], got {tuple(f.shape)}")
        tl, h, w, _ = f.shape
        out = torch.empty((16, tl, h, w), dtype=torch.float32, device=f.device)
        L.check(L.lib().svi_vae_encode_tail(self._h, L.ptr(f), L.ptr(out), tl, h, w, L.current_stream()), "svi_vae_encode_tail")
        return out

    def split_encode(self, video: torch.Tensor, split, group=None) -> torch.Tensor:
        """[1,3,T,H,W] -> [1,16,T',H/8,W/8].  group=None: every part in this process, one after another, into one feature map, then the tail (the
        local schedule: tests and timing).  With a process group of parts_h x parts_w ranks: this rank's part into its slot, one all-gather, the
        map assembled and the tail run on every rank."""
        v = video.to(device="cuda", dtype=torch.float32).contiguous()
        _, c, t, H, W = v.shape
        ph, pw = int(split[0]), int(split[1])
        n = ph * pw
        if group is not None:                            # refuse a mismatch before any collective
            import torch.distributed as dist
            world = dist.get_world_size(group)
            if world != n:
                raise ValueError(f"VAE split {ph} x {pw} needs a group of {n} ranks, this one has {world}")
        if n == 1:
            return self.single_encode(v)
        if c != 3:
            raise ValueError("video must have 3 channels")
        h, w, tl, ch = H // 8, W // 8, 1 + (t - 1) // 4, encoder_feature_channels()
        owned = [L.vae_encode_split_plan(h, w, ph, pw, p)["owned"] for p in range(n)]       # refuses a part without a pixel
        feat = torch.empty((tl, h, w, ch), dtype=torch.float32, device=v.device)
        if group is None:
            for p in range(n):
                self.encode_part(v, (ph, pw), p, out=feat)
            return self.encode_tail(feat)[None]
        import torch.distributed as dist
        from .sequence_parallel import GroupTransport, _wait
        mh, mw = max(o[1] - o[0] for o in owned), max(o[3] - o[2] for o in owned)
        if (mh, mw) == (h, w):                           # (cannot happen for n > 1; keeps a gather slot from being taken for the full map)
            raise ValueError("VAE split: a part as large as the frame")
        mine = torch.zeros((tl, mh, mw, ch), dtype=torch.float32, device=v.device)          # parts are unequal when the grid does not divide: one size for the gather
        self.encode_part(v, (ph, pw), dist.get_rank(group), out=mine)
        parts = torch.empty((n,) + tuple(mine.shape), dtype=torch.float32, device=v.device)
        _wait(GroupTransport(group).all_gather([parts], [mine]))
        for p, (h0, h1, w0, w1) in enumerate(owned):
            feat[:, h0:h1, w0:w1] = parts[p, :, :h1 - h0, :w1 - w0]
        return self.encode_tail(feat)[None]
