"""Case table of tests/test_gpu_encoder_kernels.py (no GPU imports): one-layer encoder configurations whose widths walk
gemm_skinny_kernel<MB, NW, UN> (csrc/svi_gemm.hip) through every K loop it has, and enc_attention_kernel<T, D, BF16PTS>
(csrc/svi_encoders.hip) through every head size and the ends of its key axis.  tests/test_encoder_kernel_cases.py re-derives, without a
device, which instantiation and how many main / tail steps each case runs, and that the table as a whole covers SKINNY_CELLS.

The launcher's rule (svi_launch_gemm): MB = 1 / 2 / 4 / 8 for M <= 16 / 32 / 64 / 128; NW = 8 when K % 256 == 0, else 4; UN = 8, or 4 with
MB = 8.  A wave owns K / NW of the K axis: main steps of 32 UN, then tail steps of 32.  In a T5 block q / k / v / gate / fc1 have K = dim,
o has K = dim_attn, fc2 has K = dim_ffn.

                 K / NW   UN = 8 (MB 1, 2, 4)     UN = 4 (MB 8)
    wide   2304    288    1 main + 1 tail          2 main + 1 tail          NW = 8
           2048    256    1 main                   2 main
           2560    320    1 main + 2 tails         2 main + 2 tails
    narrow 1152    288    1 main + 1 tail          2 main + 1 tail          NW = 4
            640    160    5 tails                  1 main + 1 tail
           1408    352    1 main + 3 tails         2 main + 3 tails
    d32    1024    128    4 tails                  1 main                   NW = 8 (here for the 32-wide bf16 heads)
           2048    256    1 main                   2 main
"""
EPI_BIAS, EPI_BIAS_GATE_RES = 0, 2          # include/svi_hip.h; the CPU test holds them against svi_hip._lib's


def _t5(dim, dim_attn, dim_ffn, num_heads):
    return dict(vocab=256, dim=dim, dim_attn=dim_attn, dim_ffn=dim_ffn, num_heads=num_heads, num_layers=1, num_buckets=32, shared_pos=False)


T5_CONFIGS = {
    "wide": _t5(2304, 2048, 2560, 16),        # 16 heads of 128
    "narrow": _t5(1152, 640, 1408, 8),        # 8 heads of 80
    "d32": _t5(1024, 1024, 2048, 32),         # 32 heads of 32
    "keys": _t5(128, 128, 256, 1),            # one head of 128: the key-axis cases
}
T5_SEEDS = {"wide": 1100, "narrow": 1101, "d32": 1102, "keys": 1103}        # state-dict seeds; a case's ids use seed + 10 + its index

# ---- skinny GEMM rows: (configuration, M); forward(..., rows="valid") with n_valid = M of L = SKINNY_L positions
SKINNY_L = 160
SKINNY_M = (1, 16, 17, 32, 33, 64, 65, 100, 128)          # every MB boundary from both sides, and the last skinny size
SKINNY_CASES = [(c, m) for c in ("wide", "narrow") for m in SKINNY_M] + [("d32", m) for m in (16, 40, 128)]

# the cells the skinny cases must reach between them: (MB, NW, "main" | "main+tail")
SKINNY_CELLS = [(mb, nw, loops) for mb in (1, 2, 4, 8) for nw, loops in ((8, "main"), (8, "main+tail"), (4, "main+tail"))]


def t5_gemm_shapes(cfg, M):
    """The seven projections of one block as (name, M, N, K, epilogue), in launch order."""
    d, da, df = cfg["dim"], cfg["dim_attn"], cfg["dim_ffn"]
    return [("q", M, da, d, EPI_BIAS), ("k", M, da, d, EPI_BIAS), ("v", M, da, d, EPI_BIAS), ("o", M, d, da, EPI_BIAS_GATE_RES),
            ("gate", M, df, d, EPI_BIAS), ("fc1", M, df, d, EPI_BIAS), ("fc2", M, d, df, EPI_BIAS_GATE_RES)]


# ---- key-axis lengths of the attention kernel on the "keys" configuration: (name, L, n_valid, rows)
KEY_CASES = [("full512", 512, 512, "all"),            # the pipelines' text_len, every position valid
             ("limit2048", 2048, 2048, "all"),        # the kernel's limit and its largest LDS request
             ("odd1025", 2048, 1025, "valid")]        # 1025 = 4 * 256 + 1: a thread owns 4 or 5 keys, a lane 16 or 17
KEY_LIMIT = 2048
# the same configuration at key counts tests/test_gpu_encoders.py already runs: where the per-row bound of the key cases is measured
KEY_BASELINE_CASES = [("base160", 160, 160, "all"), ("base77", 160, 77, "all"), ("base300", 512, 300, "valid")]

# ---- fp32 head sizes through the CLIP tower: (name, configuration, image shape, seed)
_CLIP = dict(image_size=28, patch_size=14, mlp_ratio=4, num_layers=3)
_CLIP17 = dict(_CLIP, image_size=56)          # 17 tokens: every row group of the P.V stage holds a live query row, and a second block of one row
CLIP_CASES = [("d32", dict(_CLIP, dim=128, num_heads=4), (1, 3, 40, 56), 1151),
              ("d128", dict(_CLIP, dim=128, num_heads=1), (1, 3, 40, 56), 1152),
              ("d32_t17", dict(_CLIP17, dim=128, num_heads=4), (1, 3, 40, 56), 1153),
              ("d64_t17", dict(_CLIP17, dim=128, num_heads=2), (1, 3, 40, 56), 1154),        # fp32 D = 80 is tests/test_gpu_encoders.py's
              ("d128_t17", dict(_CLIP17, dim=128, num_heads=1), (1, 3, 40, 56), 1155)]
CLIP_SEED = 1150


def attention_launches():
    """Every (name, D, Lk) the GPU file puts through enc_attention_kernel."""
    out = []
    for c, m in SKINNY_CASES:
        cfg = T5_CONFIGS[c]
        out.append((f"{c}_M{m}", cfg["dim_attn"] // cfg["num_heads"], m))          # the skinny and the all-rows run share their keys
    k = T5_CONFIGS["keys"]
    out += [(n, k["dim_attn"] // k["num_heads"], valid) for n, _, valid, _ in KEY_CASES + KEY_BASELINE_CASES]
    out += [(f"clip_{n}", cfg["dim"] // cfg["num_heads"], (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1) for n, cfg, _, _ in CLIP_CASES]
    return out


def attention_lds_bytes(D, Lk):
    """launch_enc_attention's dynamic LDS request: 16 query rows and 16 score rows, fp32."""
    return (16 * D + 16 * Lk) * 4
