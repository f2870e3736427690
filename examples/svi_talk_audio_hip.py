"""A talk stream that starts from the AUDIO SAMPLES: examples/test_svi_talk_hip.py's stream (svi_hip.TalkStreamLoop, the same models, the same argument
surface, the same outputs) with the audio encoder run on the device — svi_hip.WanAudioEncoder, wav2vec2-base in fp32, once per stream; its [N, 12, 768]
output never leaves HBM (TalkStreamLoop.run(speech=, audio_encoder=)).  Added to that script's arguments:
    --audio_samples FILE.npy     float32 [n]: the loudness-normalised 16 kHz mono samples of the whole stream.  Reading wav / mp4 files and the loudness
                                 normalisation (pyloudnorm) stay outside.
    --wav2vec_path DIR           the audio encoder: config.json + model.safetensors or pytorch_model.bin of chinese-wav2vec2-base
                                 (svi_hip.checkpoint.load_audio_encoder); no Hugging Face model class is imported or run
    --synthetic                  as there, and a random-init small encoder on a synthetic waveform (--audio_frames / 25 seconds of it) through the same path
    --audio_embedding FILE.npy   still accepted: the encoder's output made elsewhere, no encoder runs (what test_svi_talk_hip.py does)
    --max_audio_frames N         the audio encoder's per-call frame limit (25 frames per second of audio).  Unset: 2048, about 81 s; longer audio needs
                                 it raised (up to 65536, 43.7 min): the whole file is encoded in one call, as the reference does

    python examples/svi_talk_audio_hip.py --synthetic --num_clips 3 --num_steps 3 --height 32 --width 48 --max_frames 9
    python examples/svi_talk_audio_hip.py --dit_root weights/Wan2.1-I2V-14B-480P/ --talk_root weights/svi-talk.safetensors --audio_samples speech_16k.npy \\
        --wav2vec_path weights/chinese-wav2vec2-base/ --ref_image_path data/face.png --prompt "a person is talking" --num_clips 10
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from datetime import datetime

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import test_svi_talk_hip as base  # noqa: E402  (puts the package and tests/ on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--audio_samples", default=None, type=str, help="FILE.npy: float32 [n], the loudness-normalised 16 kHz mono samples (needs --wav2vec_path)")
    ap.add_argument("--wav2vec_path", default=None, type=str, help="directory of the audio encoder: config.json + model.safetensors or pytorch_model.bin")
    ap.add_argument("--max_audio_frames", default=None, type=int, help="the audio encoder's frame limit per stream (default: 2048 frames, about 81 s of audio)")
    own, rest = ap.parse_known_args(argv)
    args = base.parse_args(rest)                 # everything else is test_svi_talk_hip.py's surface (its --help lists it)
    args.audio_samples, args.wav2vec_path, args.max_audio_frames = own.audio_samples, own.wav2vec_path, own.max_audio_frames
    return args


def check_audio_length(encoder, n_samples: int) -> None:
    """Too long for the encoder's frame limit: say which flag raises it, before anything runs."""
    rows = encoder.seq_len(n_samples)
    if rows > encoder.max_frames:
        raise SystemExit(f"the audio is {rows} frames ({n_samples / 16000:.1f} s), above the audio encoder's limit of {encoder.max_frames} frames; "
                         f"pass --max_audio_frames {rows} (or more, up to {type(encoder).FRAME_CAP})")


def audio_of(args, dev) -> dict:
    """The audio keywords of TalkStreamLoop.run: the embedding, or the samples with the encoder that turns them into it on the device."""
    import svi_hip
    if args.audio_embedding:
        return dict(audio_embedding=torch.from_numpy(np.load(args.audio_embedding).astype(np.float32)))
    if args.audio_samples:
        if not args.wav2vec_path:
            raise SystemExit("--audio_samples needs --wav2vec_path DIR (the audio encoder's config.json and weights)")
        return dict(speech=np.load(args.audio_samples).astype(np.float32).reshape(-1),
                    audio_encoder=svi_hip.checkpoint.load_audio_encoder(args.wav2vec_path, device=dev, max_frames=args.max_audio_frames))
    if args.synthetic:
        import wav2vec_cases as wc
        rows = args.audio_frames or max(1, args.num_clips * args.max_frames - args.max_frames // 2)      # the last clip runs past the audio: the clamp holds the last row
        sd = {k: torch.from_numpy(v) for k, v in wc.state_dict(wc.SEEDS["talk_tiny"], wc.TALK_TINY).items()}
        return dict(speech=wc.waveform(3, max(400, rows * 640)),                                          # 640 samples = one video frame at 25 fps
                    audio_encoder=svi_hip.WanAudioEncoder.from_state_dict(sd, wc.hf_config(wc.TALK_TINY), device=dev, max_frames=args.max_audio_frames))
    raise SystemExit("audio is needed: --audio_samples FILE.npy with --wav2vec_path DIR, or --audio_embedding FILE.npy (or run with --synthetic)")


def main(argv=None) -> dict:
    args = parse_args(argv)
    import svi_hip
    assert torch.cuda.is_available(), "the HIP backend needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dit, vae, clip_encoder, embed = base.synthetic_models(dev) if args.synthetic else base.real_models(args, dev)
    audio = audio_of(args, dev)
    on_device = "speech" in audio
    if on_device:
        check_audio_length(audio["audio_encoder"], len(audio["speech"]))
    rows = audio["audio_encoder"].seq_len(len(audio["speech"])) if on_device else int(audio["audio_embedding"].shape[0])
    height, width = (args.height // 16) * 16, (args.width // 16) * 16
    if args.synthetic:
        yy, xx = np.mgrid[0:height, 0:width]
        img = np.stack([(xx * 255 // max(width - 1, 1)), (yy * 255 // max(height - 1, 1)), np.random.RandomState(0).randint(0, 256, (height, width))], axis=-1).astype(np.uint8)
        name = "synthetic_talk_audio"
    elif args.ref_image_path is None:
        raise SystemExit("--ref_image_path is needed (or run with --synthetic)")
    else:
        from PIL import Image
        img = np.asarray(Image.open(args.ref_image_path).convert("RGB").resize((width, height)), dtype=np.uint8)
        name = os.path.splitext(os.path.basename(args.ref_image_path))[0]
    frame = torch.from_numpy(img)
    loop = svi_hip.TalkStreamLoop(dit, vae, clip_encoder=clip_encoder, num_motion_frames=args.num_motion_frames, num_frames=args.max_frames,
                                  num_inference_steps=args.num_steps, cfg_scale=dict(audio=args.cfg_scale_audio, text=args.cfg_scale_text),
                                  ref_pad_cfg=args.ref_pad_cfg, ref_pad_num=args.ref_pad_num, tiled=args.tiled,
                                  **(dict(tea_cache_l1_thresh=base.TEA_THRESH, tea_cache_model_id=base.TEA_MODEL) if args.use_teacache else {}))
    print(f"STREAM {name}: {width}x{height}, {args.num_clips} clips x {args.max_frames} frames, {args.num_steps} steps, {rows} audio frames, "
          f"audio encoder {'on the device' if on_device else 'not run (embedding given)'}")
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    video = loop.run(frame[None], frame, (embed(args.prompt), embed(args.negative_prompt)), num_clips=args.num_clips, seed=args.seed, **audio)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t1
    out_dir = os.path.join(args.output, f"{name}_{datetime.now().strftime('%Y%m%d_%H%M%S')}")
    os.makedirs(out_dir, exist_ok=True)
    vid = video.cpu().numpy()
    np.save(os.path.join(out_dir, "video_u8.npy"), vid)
    rec = dict(sample=name, clips=args.num_clips, frames=int(vid.shape[0]), height=height, width=width, seconds=round(dt, 3), audio_frames=rows,
               audio_encoder_on_device=on_device, audio_starts=[t["audio_start"] for t in loop.trace], step_graph_captures=loop.loop.captures,
               teacache=bool(args.use_teacache), out=out_dir)
    print(f"stream done in {dt:.1f} s; {vid.shape[0]} frames -> {out_dir}; step graph captured {loop.loop.captures} time(s)")
    print(json.dumps({"svi_talk_audio_hip": [rec]}))
    return {"svi_talk_audio_hip": [rec]}


if __name__ == "__main__":
    main()
