"""FP8 storage with and without FP8-resident weights, alternating in one job on one box (DESIGN.md, FP8-resident weights):

    python tools/fp8_resident_ab.py [--rounds 2] [--steps 2] [--workloads c1 c5] > profiles/fp8_resident_ab.txt
    python tools/fp8_resident_ab.py --w8-256 ...                                   > profiles/fp8_resident_256_ab.txt

Per workload and mode (SVI_FP8_RESIDENT unset / 1; with --w8-256 a third arm, SVI_FP8_RESIDENT=1 SVI_GEMM_W8_256=1: the resident projections on the 256-row
tile that reads the stored bytes), one process each, modes alternating: `bench.py --workload W --fp8-storage --no-cpu-baseline` ->
ms_per_step, and torch.cuda.memory_allocated() after the model is loaded the way bench.py loads it (weights made on the device, stored as e4m3, bound).
Stops at the first child that fails."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMORY = """
import sys, torch
sys.path[:0] = [{root!r}, {root!r} + '/stable-video-infinity_amd', {root!r} + '/tests']
import bench, synth, svi_hip
cfg = dict(getattr(synth, bench.WORKLOADS[{wl!r}].get('model', 'WAN_1_3B')))
dev = torch.device('cuda:0')
torch.cuda.set_device(dev)
dit = svi_hip.WanDiT(eps=1e-6, num_heads=cfg['dim'] // 128, **cfg)
weights = {{k: v.to(torch.float8_e4m3fn) for k, v in bench.device_weights(cfg, 0, dev).items()}}
dit.bind(weights)
torch.cuda.synchronize()
print('MEM', torch.cuda.memory_allocated(), dit.weight_bytes())
"""


ARMS = ((), (("SVI_FP8_RESIDENT", "1"),), (("SVI_FP8_RESIDENT", "1"), ("SVI_GEMM_W8_256", "1")))          # bf16 copies; resident, 128^2 tile; resident, 256-row tile


def child(cmd, arm):
    env = dict(os.environ)
    env.pop("SVI_FP8_RESIDENT", None)
    env.pop("SVI_GEMM_W8_256", None)
    env.update(arm)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(f"child failed ({r.returncode}): {' '.join(cmd[:4])} ...")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--workloads", nargs="+", default=["c1", "c5"])
    ap.add_argument("--w8-256", action="store_true", help="add the third arm: resident with SVI_GEMM_W8_256=1")
    a = ap.parse_args()
    for wl in a.workloads:
        for rnd in range(a.rounds):
            for arm in ARMS[:3 if a.w8_256 else 2]:
                out = child([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", wl, "--fp8-storage", "--no-cpu-baseline", "--steps", str(a.steps), "--warmup", "1"],
                            arm)
                d = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
                line = f"{wl} round {rnd} {' '.join('='.join(kv) for kv in arm) or 'SVI_FP8_RESIDENT=unset'}  ms_per_step {d['ms_per_step']:.2f}  weights: {d['config'].get('weights')}"
                if rnd == 0:
                    mem = [l for l in child([sys.executable, "-c", MEMORY.format(root=ROOT, wl=wl)], arm).splitlines() if l.startswith("MEM")][-1]
                    line += f"  memory_allocated after load {int(mem.split()[1]) / 2 ** 30:.3f} GiB  weight_bytes {mem.split(' ', 2)[2]}"
                print(line, flush=True)


if __name__ == "__main__":
    main()
