"""The reference's test_svi_dance.py (pose-driven dancing video of unbounded length, clips chained by their motion frames) on the HIP backend:
svi_hip.DanceStreamLoop — the pose video is uploaded once as 8-bit frames; per clip the pose window is cut on the device (the last --num_motion_frames
poses carried over, the rest read on from a cursor that wraps; nearest resize, centre pad) and embedded, the conditioning is encoded, the denoise replays
the first clip's step graph, the clip is decoded, turned into 8-bit frames, its last --num_motion_frames frames handed to the next clip, and every clip
but the last is appended without them.

The argument surface is the reference script's: --num_motion_frames, --num_clips, --num_steps, --cfg_scale_text (--cfg_scale_audio is accepted and, as
in the reference's sampler, not read), --remove_pose, --ref_pad_cfg, --ref_pad_num, --lora_alpha, --image_path, --pose_path.  mp4 reading and writing is
not part of this script: the pose video comes in as
    --pose_path FILE.npy         uint8 [N, h, w, 3], the frames a video reader hands over, at their own resolution
and the result goes out as <output>/<name>_<timestamp>/video_u8.npy ([frames, H, W, 3] uint8, the stitched stream).  The clip size follows the
script's rule: the reference image's size, the width capped at 640 with the aspect kept, both floored to multiples of 16.  Added:
    --synthetic                  no checkpoints, no image, no pose file: the test suite's tiny image-conditioned model and a pose embedder of its width
                                 with random-init weights, seeded prompt embeddings, a synthetic reference image and a synthetic pose video
    --height / --width / --max_frames / --pose_frames   synthetic image size, frames per clip (the reference: 81), synthetic pose frames
    --use_teacache, --seed, --tiled

    python examples/test_svi_dance_hip.py --synthetic --num_clips 3 --num_steps 3
    python examples/test_svi_dance_hip.py --dit_root weights/Wan2.1-I2V-14B-480P/ --extra_module_root weights/svi-dance.safetensors \\
        --image_path data/dancer.png --pose_path data/dancer_pose.npy --num_clips 10
"""
from __future__ import annotations

import argparse
import glob
import hashlib
import json
import os
import sys
import time
from datetime import datetime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "stable-video-infinity_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

TEA_THRESH, TEA_MODEL = 0.3, "Wan2.1-I2V-14B-720P"          # what test_svi_dance.py passes when its use_teacache is set (:256-257)
MAX_WIDTH = 640                                             # test_svi_dance.py:193


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="SVI dance stream on the HIP backend (argument surface of the reference's test_svi_dance.py).  The pose video "
                                             "comes in as --pose_path FILE.npy (uint8 [N, h, w, 3]); or use --synthetic.")
    ap.add_argument("--dit_root", default="weights/Wan2.1-I2V-14B-480P/", type=str, help="Root directory of the Wan2.1-I2V model (DiT shards, VAE, umT5, CLIP).")
    ap.add_argument("--extra_module_root", default="weights/Stable-Video-Infinity/version-1.0/svi-dance.safetensors", type=str,
                    help="safetensors file(s) with the dance LoRA and the dwpose_embedding.* weights")
    ap.add_argument("--output", default="videos/", type=str)
    ap.add_argument("--cfg_scale_audio", default=1.0, type=float, help="accepted for the reference's surface; the dance sampler reads the text scale only")
    ap.add_argument("--cfg_scale_text", default=2.0, type=float)
    ap.add_argument("--train_architecture", default="lora", type=str)
    ap.add_argument("--ref_pad_cfg", default=False, action="store_true")
    ap.add_argument("--ref_pad_num", type=int, default=-1, help="0 -> no padding, k -> padding k, -1 -> full padding")
    ap.add_argument("--num_motion_frames", type=int, default=1)
    ap.add_argument("--num_clips", type=int, default=10)
    ap.add_argument("--num_steps", type=int, default=50)
    ap.add_argument("--lora_alpha", type=float, default=1.0)
    ap.add_argument("--remove_pose", action="store_true", default=False, help="no pose condition at all")
    ap.add_argument("--image_path", type=str, default=None)
    ap.add_argument("--pose_path", type=str, default=None, help="FILE.npy: the pose video, uint8 [N, h, w, 3]")
    ap.add_argument("--prompt", default="the person is dancing", type=str)
    ap.add_argument("--negative_prompt", default="bright tones, overexposed, static, blurred details, subtitles, worst quality, low quality", type=str)
    ap.add_argument("--use_teacache", default=False, action="store_true", help=f"TeaCache, threshold {TEA_THRESH}, fresh caches per clip")
    ap.add_argument("--seed", type=int, default=0, help="one seed for every clip (the reference passes None: random)")
    ap.add_argument("--tiled", default=False, action="store_true")
    ap.add_argument("--synthetic", action="store_true", help="tiny model and pose embedder with random-init weights, synthetic image, prompts and pose video: no files needed")
    ap.add_argument("--height", type=int, default=32, help="--synthetic: the reference image's height")
    ap.add_argument("--width", type=int, default=48, help="--synthetic: the reference image's width")
    ap.add_argument("--max_frames", type=int, default=0, help="frames per clip, 4 k + 1 (default: 81, the reference's; 9 with --synthetic)")
    ap.add_argument("--pose_frames", type=int, default=0, help="--synthetic: frames of the synthetic pose video (default: two clips' worth and a few, so that the stream wraps)")
    return ap.parse_args(argv)


def clip_size(image_width: int, image_height: int):
    """(height, width) of the clips for a reference image of this size (test_svi_dance.py:191-203)."""
    if image_width <= MAX_WIDTH:
        width, height = image_width, image_height
    else:
        width, height = MAX_WIDTH, int(MAX_WIDTH * (image_height / image_width))
    return (height // 16) * 16, (width // 16) * 16


def synthetic_models(dev):
    """(dit, vae, pose embedder, clip_encoder, embed(prompt)): the test suite's tiny image-conditioned architecture, random-init."""
    import synth
    import svi_hip
    from svi_hip.vae import WanVideoVAE, device_vae_weights
    cfg = dict(synth.TINY_DIT_I2V)
    sys.path.insert(0, ROOT)
    from bench import device_weights
    dit = svi_hip.WanDiT(eps=1e-6, num_heads=synth.num_heads_of(cfg), **cfg)
    dit.bind(device_weights(cfg, 0, dev))
    vae = WanVideoVAE.from_state_dict(device_vae_weights(0, dev))
    pose = svi_hip.PoseEmbedder.from_state_dict({k: torch.from_numpy(v) for k, v in synth.pose_state_dict(synth.POSE_SEED, dim=cfg["dim"]).items()}, device=dev)

    def embed(prompt: str) -> torch.Tensor:
        seed = int.from_bytes(hashlib.sha256(prompt.encode()).digest()[:4], "little")
        e = torch.randn((1, 64, cfg["text_dim"]), generator=torch.Generator(device=dev).manual_seed(seed), device=dev)
        e[:, min(63, max(4, len(prompt.split()))):] = 0
        return e.to(torch.bfloat16)

    def clip_encoder(first: torch.Tensor) -> torch.Tensor:
        base = torch.randn((1, 257, 1280), generator=torch.Generator(device=dev).manual_seed(11), device=dev)
        return (base + first.float().mean()).to(torch.bfloat16)
    return dit, vae, pose, clip_encoder, embed


def real_models(args, dev):
    """Checkpoints -> HBM -> HIP handles; the dance LoRA merged on the device, the pose embedder from the same file(s); umT5 / CLIP on the HIP encoders."""
    import svi_hip
    from svi_hip import checkpoint, lora
    root = args.dit_root
    shards = sorted(glob.glob(os.path.join(root, "diffusion_pytorch_model-*.safetensors"))) or sorted(glob.glob(os.path.join(root, "*.safetensors")))
    if not shards:
        raise SystemExit(f"no DiT shards under {root} (or run with --synthetic)")
    dit = checkpoint.load_dit(shards, device=dev)
    files = [args.extra_module_root] if args.extra_module_root.endswith(".safetensors") else sorted(glob.glob(os.path.join(args.extra_module_root, "*.safetensors")))
    pose_sd = {}
    for f in files:
        sd = checkpoint.load_safetensors(f, device=dev)
        pose_sd.update({k: v for k, v in sd.items() if "dwpose_embedding." in k})
        n = lora.load_lora_(dit, {k: v for k, v in sd.items() if "dwpose_embedding." not in k}, alpha=args.lora_alpha)
        print(f"    {n} tensors are updated by {os.path.basename(f)}.")
    if not pose_sd:
        raise SystemExit(f"{args.extra_module_root} holds no dwpose_embedding.* weights: not a dance checkpoint")
    pose = svi_hip.PoseEmbedder.from_state_dict(pose_sd, device=dev)
    vae = checkpoint.load_vae(os.path.join(root, "Wan2.1_VAE.pth"), device=dev)
    text = checkpoint.load_text_encoder(os.path.join(root, "models_t5_umt5-xxl-enc-bf16.pth"), device=dev)
    clip = checkpoint.load_image_encoder(os.path.join(root, "models_clip_open-clip-xlm-roberta-large-vit-huge-14.pth"), device=dev)
    from transformers import AutoTokenizer
    tok = AutoTokenizer.from_pretrained(os.path.join(root, "google/umt5-xxl"))

    def embed(prompt: str) -> torch.Tensor:
        enc = tok([" ".join(prompt.split())], padding="max_length", truncation=True, max_length=512, add_special_tokens=True, return_tensors="pt")
        return text.forward(enc.input_ids, enc.attention_mask, rows="valid")
    return dit, vae, pose, clip, embed


def synthetic_pose(frames: int, height: int, width: int) -> np.ndarray:
    """A pose video at a resolution of its own (not a multiple of the clip's): a coloured stroke that turns about the centre, on black."""
    h, w = 2 * height + 10, 2 * width - 6
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((frames, h, w, 3), np.uint8)
    for i in range(frames):
        a = 2 * np.pi * i / 17
        d = np.abs((xx - w / 2) * np.sin(a) - (yy - h / 2) * np.cos(a))
        stroke = d < max(1.5, h / 24)
        out[i, stroke] = ((40 + 13 * i) % 256, (200 - 7 * i) % 256, (90 + 29 * i) % 256)
    return out


def main(argv=None) -> dict:
    args = parse_args(argv)
    import svi_hip
    assert torch.cuda.is_available(), "the HIP backend needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    t0 = time.perf_counter()
    dit, vae, pose_embedder, clip_encoder, embed = synthetic_models(dev) if args.synthetic else real_models(args, dev)
    torch.cuda.synchronize()
    print(f"models resident after {time.perf_counter() - t0:.1f} s ({'synthetic tiny model' if args.synthetic else args.dit_root})")
    frames_per_clip = args.max_frames or (9 if args.synthetic else 81)
    if args.synthetic:
        height, width = clip_size(args.width, args.height)
        yy, xx = np.mgrid[0:height, 0:width]
        img = np.stack([(xx * 255 // max(width - 1, 1)), (yy * 255 // max(height - 1, 1)), np.random.RandomState(0).randint(0, 256, (height, width))], axis=-1).astype(np.uint8)
        pose = synthetic_pose(args.pose_frames or 2 * frames_per_clip + 5, height, width)
        name = "synthetic_dance"
    else:
        if not args.image_path or not args.pose_path:
            raise SystemExit("--image_path and --pose_path FILE.npy are needed (or run with --synthetic)")
        from PIL import Image
        image = Image.open(args.image_path).convert("RGB")
        height, width = clip_size(*image.size)
        img = np.asarray(image.resize((width, height)), dtype=np.uint8)
        pose = np.load(args.pose_path)
        name = os.path.splitext(os.path.basename(args.image_path))[0]
    frame = torch.from_numpy(img)
    loop = svi_hip.DanceStreamLoop(dit, vae, pose_embedder, clip_encoder=clip_encoder, num_motion_frames=args.num_motion_frames, num_frames=frames_per_clip,
                                   num_inference_steps=args.num_steps, cfg_scale=dict(audio=args.cfg_scale_audio, text=args.cfg_scale_text),
                                   cond_wo_pose=True, remove_pose=args.remove_pose, ref_pad_cfg=args.ref_pad_cfg, ref_pad_num=args.ref_pad_num, tiled=args.tiled,
                                   **(dict(tea_cache_l1_thresh=TEA_THRESH, tea_cache_model_id=TEA_MODEL) if args.use_teacache else {}))
    print(f"\n{'#' * 80}\nSTREAM {name}: {width}x{height}, {args.num_clips} clips x {frames_per_clip} frames, {args.num_steps} steps, "
          f"{pose.shape[0]} pose frames of {pose.shape[2]}x{pose.shape[1]}")
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    video = loop.run(frame[None], frame, (embed(args.prompt), embed(args.negative_prompt)), torch.from_numpy(pose), args.num_clips, seed=args.seed)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t1
    out_dir = os.path.join(args.output, f"{name}_{datetime.now().strftime('%Y%m%d_%H%M%S')}")
    os.makedirs(out_dir, exist_ok=True)
    vid = video.cpu().numpy()
    np.save(os.path.join(out_dir, "video_u8.npy"), vid)
    rec = dict(sample=name, clips=args.num_clips, frames=int(vid.shape[0]), height=height, width=width, frames_per_clip=frames_per_clip, seconds=round(dt, 3),
               pose_frames=int(pose.shape[0]), pose_size=[int(pose.shape[1]), int(pose.shape[2])], pose_windows=[t["pose_window"] for t in loop.trace],
               step_graph_captures=loop.loop.captures, teacache=bool(args.use_teacache), out=out_dir)
    print(f"stream done in {dt:.1f} s; {vid.shape[0]} frames -> {out_dir}; step graph captured {loop.loop.captures} time(s)")
    print(json.dumps({"test_svi_dance_hip": [rec]}))
    return {"test_svi_dance_hip": [rec]}


if __name__ == "__main__":
    main()
