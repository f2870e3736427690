"""CPU: what tests/golden/lora_fp8.npz (the reference's GeneralLoRAFromPeft.load on float8_e4m3fn parameters) pins, and that the fp8 merge has
no CPU path.  The device side is tests/test_gpu_lora_fp8.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import lora_fp8_util as U


@pytest.fixture(scope="module")
def cases():
    return U.load_cases()


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_fixture_is_the_fp32_merge_requantised(cases, name):
    """The reference's merge on fp8 parameters is e4m3(fp32(W) + alpha * mm(fp32(up), fp32(down))), file after file, each re-quantising: that
    expression reproduces the recorded codes exactly."""
    c = cases[name]
    w = c["before"]
    for up, down, alpha in c["files"]:
        w = U.torch_merge(w, up, down, alpha)
    assert np.array_equal(w, c["after"])
    assert (c["after"] != c["before"]).mean() > 0.5              # the merge moved most codes: the fixture can tell a merge from none


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_acceptance_band_is_tight_and_holds_the_reference(cases, name):
    """The band of the device test (lora_fp8_util.band) leaves at most 1 % of the codes undetermined on the fixture's shapes, and the reference
    itself lies inside it — per step, with the reference's own intermediate codes."""
    c = cases[name]
    w = c["before"]
    for i, (up, down, alpha) in enumerate(c["files"]):
        nxt = U.torch_merge(w, up, down, alpha)
        U.check_step(nxt, w, up, down, alpha, nxt, f"{name}[{i}] reference")
        w = nxt


def test_fixture_operands_are_what_the_issue_of_precision_needs(cases):
    up, down, _ = cases["f32_r8"]["files"][0]
    assert up.dtype == torch.float32 and not torch.equal(up, up.to(torch.bfloat16).float())      # fp32 operands that bf16 cannot hold
    assert cases["bf16_r32"]["files"][0][0].dtype == torch.bfloat16
    assert len(cases["sequence"]["files"]) == 2


def test_merge_into_a_cpu_fp8_tensor_fails_loudly():
    from svi_hip import lora
    w = torch.zeros(16, 16).to(torch.float8_e4m3fn)
    before = w.view(torch.uint8).clone()
    with pytest.raises((ValueError, RuntimeError)):
        lora.merge_lora_(w, torch.ones(16, 8), torch.ones(8, 16), 1.0)
    assert torch.equal(w.view(torch.uint8), before)


# ---------------------------------------------------------------------------------------------------------------- svi_fp8.h on the host
FP8_H = os.path.join(ROOT, "stable-video-infinity_amd", "csrc", "svi_fp8.h")
SHIM = """#include "%s"
extern "C" void cast_n(const float* in, unsigned char* out, long n) { for (long i = 0; i < n; ++i) out[i] = (unsigned char)svi_f32_to_e4m3fn(in[i]); }
extern "C" void decode_n(const unsigned char* in, float* out, long n) { for (long i = 0; i < n; ++i) out[i] = svi_e4m3fn_to_f32(in[i]); }
"""


@pytest.fixture(scope="module")
def fp8_host_lib(tmp_path_factory):
    """csrc/svi_fp8.h — the conversions the kernels use — compiled as plain host C++ by the compiler that builds the library."""
    from svi_hip.build import _hipcc
    d = tmp_path_factory.mktemp("fp8h")
    src, so = d / "shim.cpp", d / "libfp8shim.so"
    src.write_text(SHIM % FP8_H)
    subprocess.run([_hipcc(), "-x", "c++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(so)], check=True, capture_output=True)
    return ctypes.CDLL(str(so))


def test_integer_cast_is_torchs_cast_on_the_host(fp8_host_lib):
    """svi_f32_to_e4m3fn against torch's CPU `.to(torch.float8_e4m3fn)`: every fp32 bit pattern whose low 12 bits are 0, 1, 0x7ff, 0x800, 0x801 or
    0xfff (6.3 M values: every exponent, every kept-mantissa value, every tie and the patterns beside it, both signs, subnormals, inf, NaNs).
    Bit-exact; a NaN input gives the NaN code with its own sign, as torch does."""
    hi = np.arange(1 << 20, dtype=np.uint64) << 12
    low = np.array([0, 1, 0x7ff, 0x800, 0x801, 0xfff], dtype=np.uint64)
    x = (hi[:, None] | low[None, :]).reshape(-1).astype(np.uint32).view(np.float32).copy()
    got = np.empty(x.size, np.uint8)
    fp8_host_lib.cast_n(x.ctypes.data_as(ctypes.c_void_p), got.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(x.size))
    want = torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(x[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]


def test_decode_is_torchs_decode_on_the_host(fp8_host_lib):
    codes = np.arange(256, dtype=np.uint8)
    got = np.empty(256, np.float32)
    fp8_host_lib.decode_n(codes.ctypes.data_as(ctypes.c_void_p), got.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(256))
    want = torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy()
    nan = np.isnan(want)
    assert nan.sum() == 2 and np.isnan(got[nan]).all() and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- the widened dtype enum
def test_fp16_code_is_refused_where_it_has_no_meaning():
    """SVI_F16 exists for LoRA operands only: the entry points that bind weights refuse it (they name the one dtype they take) rather than read it as fp32,
    and the stand-alone cast takes fp32 or bf16 only.  Host-only calls: each check runs before anything touches a device."""
    from svi_hip import _lib as L
    lib = L.lib()
    assert L.SVI_F16 == 2
    cfg = L.DitConfig(128, 16, 256, 16, 64, 256, 1e-6, 1, 2, 2, 1, 2, 0)
    h = ctypes.c_void_p()
    assert lib.svi_dit_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    shape = (ctypes.c_int64 * 2)(128, 128)
    assert lib.svi_dit_bind_weight(h, b"blocks.0.self_attn.q.weight", 16, L.SVI_F16, shape, 2) == 1 and "must be bf16" in L.last_error()
    assert lib.svi_dit_destroy(h) == 0
    assert lib.svi_f32_to_fp8_e4m3(16, L.SVI_F16, 16, 8, None) == 1 and "fp32 or bf16" in L.last_error()
    assert lib.svi_lora_merge_e4m3(16, 8, 8, 16, 16, 3, 8, 1.0, None) == 1 and "bf16, fp16 or fp32" in L.last_error()
    assert lib.svi_lora_merge_e4m3(16, 8, 12, 16, 16, L.SVI_F16, 8, 1.0, None) == 1 and "multiples of 8" in L.last_error()

