"""The reference's test_svi_talk.py (audio-driven talking video of unbounded length, clips chained by their motion frames) on the HIP backend:
svi_hip.TalkStreamLoop — per clip the audio windows are cut on the device out of the whole stream's audio embedding and both audio slots of the DiT
re-staged where they stand, the conditioning is encoded, the three-way guidance denoise replays the first clip's step graph, the clip is decoded,
turned into 8-bit frames, its last --num_motion_frames frames handed to the next clip, and every clip is appended whole.

The argument surface is the reference script's: --num_clips, --num_motion_frames, --cfg_scale_audio, --cfg_scale_text, --num_steps, --use_teacache
(+ --tiled, --ref_pad_cfg, --ref_pad_num, --seed).  The AUDIO ENCODER IS NOT PART OF THIS SCRIPT: wav2vec2 is neither imported nor run here.  It runs once
per audio file, outside; its output — the [N, 12, 768] embedding the reference's get_embedding returns — comes in through
    --audio_embedding FILE.npy   float32 or bfloat16-as-float32 [N, 12, 768], one row per video frame of audio
or, with --synthetic, is a seeded random one.  Added:
    --synthetic                  no checkpoints, no audio, no image files: the test suite's tiny talk model with random-init weights, seeded prompt
                                 embeddings, a synthetic reference image and a synthetic embedding (--audio_frames rows)
    --height / --width / --max_frames   synthetic image size and frames per clip (the reference: 81)
Outputs: <output>/<name>_<timestamp>/video_u8.npy ([frames, H, W, 3] uint8, the stitched stream).

    python examples/test_svi_talk_hip.py --synthetic --num_clips 3 --num_steps 3 --height 32 --width 48 --max_frames 9
    python examples/test_svi_talk_hip.py --dit_root weights/Wan2.1-I2V-14B-480P/ --talk_root weights/svi-talk.safetensors --audio_embedding speech.npy \\
        --ref_image_path data/face.png --prompt "a person is talking" --num_clips 10
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

TEA_THRESH, TEA_MODEL = 0.3, "Wan2.1-I2V-14B-720P"          # what test_svi_talk.py passes with --use_teacache (:294-295)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="SVI talk stream on the HIP backend (argument surface of the reference's test_svi_talk.py).  The wav2vec2 audio "
                                             "encoder is NOT imported or run here: pass its output with --audio_embedding FILE.npy ([N, 12, 768]), or use --synthetic.")
    ap.add_argument("--dit_root", default="weights/Wan2.1-I2V-14B-480P/", type=str, help="Root directory of the Wan2.1-I2V model (DiT shards, VAE, umT5, CLIP).")
    ap.add_argument("--talk_root", default=None, type=str, help="safetensors file(s) with the talk variant's extra DiT weights (audio_proj.*, blocks.*.audio_cross_attn.*, norm_x)")
    ap.add_argument("--audio_embedding", default=None, type=str, help="FILE.npy: the audio encoder's output for the whole stream, [N, 12, 768]")
    ap.add_argument("--ref_image_path", default=None, type=str)
    ap.add_argument("--prompt", default="a person is talking", type=str)
    ap.add_argument("--negative_prompt", default="bright tones, overexposed, static, blurred details, subtitles, worst quality, low quality", type=str)
    ap.add_argument("--output", default="videos/", type=str)
    ap.add_argument("--num_clips", type=int, default=10)
    ap.add_argument("--num_motion_frames", type=int, default=1)
    ap.add_argument("--cfg_scale_audio", type=float, default=4.0)
    ap.add_argument("--cfg_scale_text", type=float, default=5.0)
    ap.add_argument("--num_steps", type=int, default=50)
    ap.add_argument("--use_teacache", default=False, action="store_true", help=f"TeaCache, threshold {TEA_THRESH}, fresh caches per clip")
    ap.add_argument("--seed", type=int, default=0, help="one seed for every clip, as in the reference's call")
    ap.add_argument("--tiled", default=False, action="store_true")
    ap.add_argument("--ref_pad_cfg", default=False, action="store_true")
    ap.add_argument("--ref_pad_num", type=int, default=0, help="0 -> no padding, k -> padding k, -1 -> full padding")
    ap.add_argument("--synthetic", action="store_true", help="tiny talk model with random-init weights, synthetic embedding, prompts and image: no files needed")
    ap.add_argument("--audio_frames", type=int, default=0, help="--synthetic: rows of the synthetic embedding (default: enough for all clips but the last's tail)")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=832)
    ap.add_argument("--max_frames", type=int, default=81, help="frames per clip (4 k + 1; the reference: 81)")
    return ap.parse_args(argv)


def synthetic_models(dev):
    """(dit, vae, clip_encoder, embed(prompt)): the test suite's tiny talk architecture, random-init."""
    import synth
    import svi_hip
    from svi_hip.vae import WanVideoVAE, device_vae_weights
    cfg = dict(synth.TINY_DIT_TALK)
    sys.path.insert(0, ROOT)
    from bench import device_weights
    dit = svi_hip.WanDiT(eps=1e-6, num_heads=synth.num_heads_of(cfg), **cfg)
    dit.bind(device_weights(cfg, 0, dev))
    vae = WanVideoVAE.from_state_dict(device_vae_weights(0, dev))

    def embed(prompt: str) -> torch.Tensor:
        seed = int.from_bytes(hashlib.sha256(prompt.encode()).digest()[:4], "little")
        e = torch.randn((1, 64, cfg["text_dim"]), generator=torch.Generator(device=dev).manual_seed(seed), device=dev)
        e[:, min(63, max(4, len(prompt.split()))):] = 0
        return e.to(torch.bfloat16)

    def clip_encoder(first: torch.Tensor) -> torch.Tensor:
        base = torch.randn((1, 257, 1280), generator=torch.Generator(device=dev).manual_seed(11), device=dev)
        return (base + first.float().mean()).to(torch.bfloat16)
    return dit, vae, clip_encoder, embed


def real_models(args, dev):
    """Checkpoints -> HBM -> HIP handles (the I2V DiT's shards plus the talk variant's extra weights); umT5 / CLIP on the HIP encoders."""
    from svi_hip import checkpoint
    root = args.dit_root
    shards = sorted(glob.glob(os.path.join(root, "diffusion_pytorch_model-*.safetensors"))) or sorted(glob.glob(os.path.join(root, "*.safetensors")))
    if not shards or not args.talk_root:
        raise SystemExit(f"need the DiT shards under {root} and --talk_root (or run with --synthetic)")
    extra = [args.talk_root] if args.talk_root.endswith(".safetensors") else sorted(glob.glob(os.path.join(args.talk_root, "*.safetensors")))
    dit = checkpoint.load_dit(shards + extra, device=dev)
    if not dit.enable_multitalk:
        raise SystemExit(f"{args.talk_root} holds no audio_proj.* weights: not a talk checkpoint")
    vae = checkpoint.load_vae(os.path.join(root, "Wan2.1_VAE.pth"), device=dev)
    text = checkpoint.load_text_encoder(os.path.join(root, "models_t5_umt5-xxl-enc-bf16.pth"), device=dev)
    clip = checkpoint.load_image_encoder(os.path.join(root, "models_clip_open-clip-xlm-roberta-large-vit-huge-14.pth"), device=dev)
    from transformers import AutoTokenizer
    tok = AutoTokenizer.from_pretrained(os.path.join(root, "google/umt5-xxl"))

    def embed(prompt: str) -> torch.Tensor:
        enc = tok([" ".join(prompt.split())], padding="max_length", truncation=True, max_length=512, add_special_tokens=True, return_tensors="pt")
        return text.forward(enc.input_ids, enc.attention_mask, rows="valid")
    return dit, vae, clip, embed


def main(argv=None) -> dict:
    args = parse_args(argv)
    import svi_hip
    assert torch.cuda.is_available(), "the HIP backend needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    t0 = time.perf_counter()
    dit, vae, clip_encoder, embed = synthetic_models(dev) if args.synthetic else real_models(args, dev)
    torch.cuda.synchronize()
    print(f"models resident after {time.perf_counter() - t0:.1f} s ({'synthetic tiny talk model' if args.synthetic else args.dit_root})")
    height, width = (args.height // 16) * 16, (args.width // 16) * 16
    if args.synthetic or args.ref_image_path is None:
        if not args.synthetic:
            raise SystemExit("--ref_image_path is needed (or run with --synthetic)")
        yy, xx = np.mgrid[0:height, 0:width]
        img = np.stack([(xx * 255 // max(width - 1, 1)), (yy * 255 // max(height - 1, 1)), np.random.RandomState(0).randint(0, 256, (height, width))], axis=-1).astype(np.uint8)
        name = "synthetic_talk"
    else:
        from PIL import Image
        img = np.asarray(Image.open(args.ref_image_path).convert("RGB").resize((width, height)), dtype=np.uint8)
        name = os.path.splitext(os.path.basename(args.ref_image_path))[0]
    if args.audio_embedding:
        emb = torch.from_numpy(np.load(args.audio_embedding).astype(np.float32))
    elif args.synthetic:
        rows = args.audio_frames or max(1, args.num_clips * args.max_frames - args.max_frames // 2)      # the last clip runs past the audio: the clamp holds the last row
        emb = 0.5 * torch.randn((rows, 12, 768), generator=torch.Generator().manual_seed(3))
    else:
        raise SystemExit("--audio_embedding FILE.npy is needed: the audio encoder is not part of this script (or run with --synthetic)")
    frame = torch.from_numpy(img)
    loop = svi_hip.TalkStreamLoop(dit, vae, clip_encoder=clip_encoder, num_motion_frames=args.num_motion_frames, num_frames=args.max_frames,
                                  num_inference_steps=args.num_steps, cfg_scale=dict(audio=args.cfg_scale_audio, text=args.cfg_scale_text),
                                  ref_pad_cfg=args.ref_pad_cfg, ref_pad_num=args.ref_pad_num, tiled=args.tiled,
                                  **(dict(tea_cache_l1_thresh=TEA_THRESH, tea_cache_model_id=TEA_MODEL) if args.use_teacache else {}))
    print(f"\n{'#' * 80}\nSTREAM {name}: {width}x{height}, {args.num_clips} clips x {args.max_frames} frames, {args.num_steps} steps, {emb.shape[0]} audio frames")
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    video = loop.run(frame[None], frame, (embed(args.prompt), embed(args.negative_prompt)), emb, args.num_clips, seed=args.seed)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t1
    out_dir = os.path.join(args.output, f"{name}_{datetime.now().strftime('%Y%m%d_%H%M%S')}")
    os.makedirs(out_dir, exist_ok=True)
    vid = video.cpu().numpy()
    np.save(os.path.join(out_dir, "video_u8.npy"), vid)
    rec = dict(sample=name, clips=args.num_clips, frames=int(vid.shape[0]), height=height, width=width, seconds=round(dt, 3), audio_frames=int(emb.shape[0]),
               audio_starts=[t["audio_start"] for t in loop.trace], step_graph_captures=loop.loop.captures, teacache=bool(args.use_teacache), out=out_dir)
    print(f"stream done in {dt:.1f} s; {vid.shape[0]} frames -> {out_dir}; step graph captured {loop.loop.captures} time(s)")
    print(json.dumps({"test_svi_talk_hip": [rec]}))
    return {"test_svi_talk_hip": [rec]}


if __name__ == "__main__":
    main()
