# usage (GPU box): bash tools/c1_ab.sh <outdir> — the C1-size step (BASELINE configs[0]) with the 128^2 GEMM's loop forced to each form, alternating in one job:
# SVI_GEMM_PF = 1 (one K tile of loads in flight, rounds 1-6), 4 (four, four waves), 0 (default: four on eight waves when the launch is at most one workgroup per CU)
set -u
OUT=${1:?usage: tools/c1_ab.sh <outdir>}
mkdir -p "$OUT"
for pf in 1 4 0 1 4 0; do
  SVI_GEMM_PF=$pf timeout 300 python bench.py --full --workload c1 --steps 20 --warmup 5 --no-cpu-baseline --no-vendor --no-full-clip --no-vae 2>/dev/null | grep '"metric"' | tail -1 > "$OUT/c1_ab_pf$pf.json"
  python - "$OUT/c1_ab_pf$pf.json" $pf <<'PY'
import json, sys
j = json.load(open(sys.argv[1]))
print("SVI_GEMM_PF", sys.argv[2], "ms_per_step", j["ms_per_step"], {k: v.get("ms_per_step") for k, v in j["roofline_all"].items()})
PY
done
