"""The C-ABI boundary without a GPU: the library loads, exports every symbol include/svi_hip.h declares,
the ctypes table matches the header, and host-only entry points behave (no compute calls here)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from svi_hip import _lib as L

HEADER = os.path.join(ROOT, "include", "svi_hip.h")


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(svi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = L.lib()
    names = declared_symbols()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f"{n} declared in svi_hip.h but not exported by libsvi_hip.so"


def test_ctypes_table_matches_header():
    assert sorted(n for n, _, _ in L.SYMBOLS) == declared_symbols()


def test_abi_version_is_v13_in_header_and_library():
    """v13 added the DiT's q | k projection launch (two weights side by side, the per-sample kernel choice) as an operator seam (svi_gemm_bf16_pair),
    v12 its q | k RMSNorm + RoPE launch (svi_rmsnorm_rope_qk), v11 the VAE convolution planners (svi_vae_conv_plan, svi_vae_tile_order); the header's
    define and the built library agree."""
    m = re.search(r"#define\s+SVI_HIP_ABI_VERSION\s+(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 13
    assert L.lib().svi_abi_version() == 13
    assert {"svi_vae_conv_plan", "svi_vae_tile_order", "svi_rmsnorm_rope_qk", "svi_gemm_bf16_pair"} <= set(declared_symbols())
    # the pair entry point is svi_gemm_bf16's argument list with W2, bias2, n_split, sel_m, sel_n in front of the stream
    table = {n: a for n, _, a in L.SYMBOLS}
    assert table["svi_gemm_bf16_pair"] == table["svi_gemm_bf16"][:-1] + [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]


def test_dit_handle_lifecycle_and_errors():
    lib = L.lib()
    cfg = L.DitConfig(128, 16, 256, 16, 64, 256, 1e-6, 1, 2, 2, 1, 2, 0)
    h = C.c_void_p()
    assert lib.svi_dit_create(C.byref(cfg), C.byref(h)) == 0
    # nothing bound yet -> UNBOUND with the first missing key named
    assert lib.svi_dit_check_bound(h) == 2
    assert "never bound" in L.last_error()
    # unknown key and wrong shape are rejected
    shape = (C.c_int64 * 2)(128, 128)
    assert lib.svi_dit_bind_weight(h, b"blocks.0.nope.weight", 16, L.SVI_BF16, shape, 2) == 1
    bad = (C.c_int64 * 2)(64, 128)
    assert lib.svi_dit_bind_weight(h, b"blocks.0.self_attn.q.weight", 16, L.SVI_BF16, bad, 2) == 1
    assert "shape mismatch" in L.last_error()
    assert lib.svi_dit_bind_weight(h, b"blocks.0.self_attn.q.weight", 16, L.SVI_F32, shape, 2) == 1
    assert lib.svi_dit_destroy(h) == 0
    # head_dim must be 128
    cfg2 = L.DitConfig(128, 16, 256, 16, 64, 256, 1e-6, 1, 2, 2, 2, 2, 0)
    assert lib.svi_dit_create(C.byref(cfg2), C.byref(h)) == 1
    assert "head_dim" in L.last_error()


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "stable-video-infinity_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "import oracle" not in txt and "from oracle" not in txt and "/root/reference" not in txt, f


def test_ops_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import svi_hip
    x = torch.zeros(4, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        svi_hip.layernorm_modulate(x)


def test_every_environment_switch_is_documented():
    """Each SVI_* switch the library parses (csrc/svi_api.hip) is listed in the public header and explained where its field lives
    (csrc/svi_common.h SviSwitches).  Timing ablations are not in the product source: none of their switches or macros occurs under csrc/."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "stable-video-infinity_amd", "csrc")
    src = open(os.path.join(csrc, "svi_api.hip")).read()
    parse = re.search(r"\nstatic SviSwitches parse_switches\(\) \{\n.*?\n\}\n", src, re.S).group(0)
    names = set(re.findall(r'(?:env_int|getenv)\("(SVI_[A-Z0-9_]+)"', parse))
    assert len(names) >= 14 and "SVI_FLASH_ABL" not in names
    removed = re.compile(r"SVI_ABLATIONS|SVI3_ABL|SVI_GEMM_EXPERIMENTS|SVI_W4_|SVI_FLASH_(DMA_SPLIT|SUM_DOT2|BALANCED|SHORT_NOP|ABL|ASSUME_PRESCALED)|SVI_(GEMM_EPI|VAE)_ABL")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")):
            assert not removed.search(open(os.path.join(csrc, f)).read()), f
    header = open(os.path.join(root, "include", "svi_hip.h")).read()
    common = open(os.path.join(root, "stable-video-infinity_amd", "csrc", "svi_common.h")).read()
    missing = sorted(n for n in names if n not in header or n not in common)
    assert not missing, missing
