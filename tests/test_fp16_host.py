"""CPU: the host side of the estimator's FP16 mode -- the rounding helpers of tests/fp16_ref.py against torch's half type, the
emulation against the oracle it restates, the header / binding pair of the two new symbols, the Python surfaces that must fail or
show up without a device."""
import os
import re
import subprocess
import sys

import pytest
import torch

import fp16_ref as fr
from conftest import REPO


def _values():
    g = torch.Generator().manual_seed(16)
    x = torch.randn(50000, generator=g) * torch.exp(8.0 * torch.randn(50000, generator=g))      # sixteen decades
    edge = torch.tensor([0.0, -0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -10, 2049.0, 2051.0, 65504.0, 65519.9, 65520.0, 7e4,
                         -65520.0, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12), 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.0 ** -25 * 1.0001,
                         2.5 * 2.0 ** -24, 3.5 * 2.0 ** -24, -1.5 * 2.0 ** -24, 1e-9])
    return torch.cat([x, edge])


@pytest.mark.parametrize("scale", [1.0, 2.0 ** 7, 2.0 ** -9, 2.0 ** 11])
def test_round_h_is_the_half_type(scale):
    """normal, subnormal, boundary and overflowing values: fp16(x * scale) / scale exactly, ties to even included"""
    x = _values()
    want = (x * scale).half().float() / scale
    got = fr.round_h(x, scale)
    assert got.dtype == x.dtype
    assert torch.equal(got, want), int((got != want).sum())
    assert torch.equal(fr.round_h(x.double(), scale), want.double())
    sub = (x * scale).abs() < 2.0 ** -14
    assert sub.any() and ((x * scale).abs() > 65504.0).any()      # both special ranges are exercised


def test_round_h_without_a_scale_keeps_eleven_bits():
    x = _values()[:50000]
    r = fr.round_h(x)
    m, _ = torch.frexp(r.double())
    assert torch.equal(m * 2048.0, torch.round(m * 2048.0))                       # 11 significant bits
    assert float(((r - x).abs() / x.abs()).max()) <= 2.0 ** -11                     # nearest: half a step of 2^-10 of the binade
    normal = (x.abs() >= 2.0 ** -14) & (x.abs() < 65504.0)
    assert torch.equal(r[normal], x[normal].half().float())


def test_fast_paths_equal_round_h():
    """the estimator's per-tensor and per-row fast paths are round_h under their scales"""
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(64, 256, generator=g) * torch.exp(3.0 * torch.randn(64, 256, generator=g))).double()
    am = float(x.abs().max())
    import math
    sc = 2.0 ** (14 - math.frexp(am)[1])
    assert torch.equal(fr.round_fast(x), fr.round_h(x, sc))
    W = torch.randn(48, 96, generator=g) * torch.exp(2.0 * torch.randn(48, 1, generator=g))
    assert torch.equal(fr.round_w(W), fr.round_h(W, fr.weight_scale(W)))
    top = (W.double().abs() * fr.weight_scale(W)).amax(dim=1)
    assert bool(((top >= 2.0 ** 13) & (top < 2.0 ** 14)).all())                    # registry.hip split2h_kernel's row scale


def test_emulation_with_identity_rounding_is_the_oracle(tts_sd):
    """fp16_ref.estimator restates oracle.flow.estimator: without the rounding the two agree to fp32 rounding of another operation
    order, with and without the chunk mask; with it the result moves by the 11-bit operands' error, not more"""
    from oracle import flow as oflow
    c = fr.case_inputs("i")
    args = [a[:, ..., :24] if a.dim() == 3 else a for a in fr.cfg_batch(c)]
    args[1] = (torch.arange(24)[None, None] < torch.tensor([24, 19])[:, None, None]).float()
    ident = lambda z: z
    with torch.inference_mode():
        for streaming in (False, True):
            want = oflow.estimator(tts_sd, *args, streaming=streaming, chunk=10)
            got = fr.estimator(tts_sd, *args, streaming=streaming, chunk=10, R=ident)
            assert float((got - want).abs().max()) <= 2e-5, streaming
        d = float((fr.estimator(tts_sd, *args) - oflow.estimator(tts_sd, *args)).abs().max())
    assert 1e-4 < d < 5e-2, d


def test_header_and_binding_have_the_two_symbols():
    from jyutvoice_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "jyutvoice_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+jv_flow_set_precision\s*\(\s*jv_context\s*\*\s*ctx\s*,\s*int\s+precision\s*\)\s*;", text)
    assert re.search(r"\bint\s+jv_op_set_products\s*\(\s*int\s+np\s*\)\s*;", text)
    assert re.search(r"#define\s+JV_PRECISION_FP32\s+0\b", text) and re.search(r"#define\s+JV_PRECISION_FP16\s+1\b", text)
    import ctypes as C
    assert _lib.SIGNATURES["jv_flow_set_precision"] == (C.c_int, [C.c_void_p, C.c_int])
    assert _lib.SIGNATURES["jv_op_set_products"] == (C.c_int, [C.c_int])
    assert (_lib.JV_PRECISION_FP32, _lib.JV_PRECISION_FP16) == (0, 1)
    lib = _lib.load()
    assert lib.jv_op_set_products(2) != 0 and b"jv_op_set_products" in lib.jv_last_error()      # host only: no device needed
    assert lib.jv_op_set_products(1) == 0 and lib.jv_op_set_products(3) == 0
    assert lib.jv_flow_set_precision(None, 1) != 0                                               # a null context is refused, not followed


def test_set_precision_rejects_other_names_without_a_device_call():
    from jyutvoice_amd.engine import Engine
    from jyutvoice_amd.runtime import Runtime

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"device call {name}")

    eng = Engine.__new__(Engine)      # no context: any library call through it would fail
    eng.lib, eng._h = NoDevice(), None
    for bad in ("bf16", "FP16", "", None, 1):
        with pytest.raises(ValueError, match="fp16"):
            eng.set_precision(bad)
    rt = Runtime("cuda:0")
    with pytest.raises(ValueError, match="fp32"):
        rt.set_precision("bf16")
    rt.set_precision("fp16")          # no engine yet: remembered for the context the first weights create
    assert rt.precision == "fp16" and rt.engine is None
    eng._h = None                     # (nothing for __del__ to close)


def test_infer_help_lists_the_flag():
    r = subprocess.run([sys.executable, os.path.join(REPO, "infer.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--estimator-precision" in r.stdout and "{fp32,fp16}" in r.stdout
