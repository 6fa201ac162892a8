"""CPU: the host side of the voice-cloning batch -- `pad_prompts`, and the two new C-ABI entries (jv_cfm_solve_prompted,
jv_mel_spectrogram_ragged): declared in the header, exported by the built library, listed by the ctypes binding with the
header's argument counts, and failing loudly without a device."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO

HEADER = os.path.join(REPO, "include", "jyutvoice_hip.h")
NEW = {"jv_cfm_solve_prompted": 16, "jv_mel_spectrogram_ragged": 8}      # arguments, as the issue's signatures have them


def header_prototypes():
    """name -> number of parameters, for every function include/jyutvoice_hip.h declares (comments stripped first)"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(jv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = params.strip()
        out[name] = 0 if params in ("", "void") else len(params.split(","))
    return out


@pytest.fixture(scope="module")
def lib():
    from jyutvoice_amd import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from jyutvoice_amd import _lib
    return _lib.load()


def test_new_entries_declared_exported_and_bound(lib):
    from jyutvoice_amd import _lib
    protos = header_prototypes()
    for name, nargs in NEW.items():
        assert protos.get(name) == nargs, f"{name}: the header declares {protos.get(name)} parameters"
        assert hasattr(lib, name), f"{name} not exported by the library"
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
    # and every other binding has the header's argument count too
    for name, (res, args) in _lib.SIGNATURES.items():
        assert len(args) == protos[name], name
    _, a = _lib.SIGNATURES["jv_cfm_solve_prompted"]
    assert a[7:12] == [ctypes.c_int] * 5 and a[12] is ctypes.c_float      # B, Ty, Ph, Pf, n_timesteps, temperature


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_new_entries_fail_loudly_without_a_device(lib):
    from jyutvoice_amd._lib import JvError, check
    h = ctypes.c_void_p()
    assert lib.jv_create(ctypes.byref(h), 0, 4, 256, 64) != 0 and not h.value      # no context without a device ...
    buf = (ctypes.c_float * 64)()
    ints = (ctypes.c_int32 * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    i = ctypes.cast(ints, ctypes.c_void_p)
    with pytest.raises(JvError, match="null context"):      # ... and no call without a context: the library's own error
        check(lib.jv_cfm_solve_prompted(h, p, i, p, p, i, p, 1, 1, 1, 1, 2, 1.0, None, p, None))
    with pytest.raises(JvError, match="null argument"):
        check(lib.jv_mel_spectrogram_ragged(h, p, i, 1, 1000, p, i, None))
    from jyutvoice_amd.utils.audio import extract_speech_feat_batch
    with pytest.raises(RuntimeError):
        extract_speech_feat_batch([torch.zeros(1, 24000)], device="cuda:0")


def test_pad_prompts():
    from jyutvoice_amd.utils.prompt import pad_prompts
    g = torch.Generator().manual_seed(0)
    lens = [30, 66, 0, 44]
    feats = [torch.randn(n, 80, generator=g) for n in lens]
    hs = [torch.randn(n, 80, generator=g) for n in lens]
    feat, h, p = pad_prompts(feats, hs)
    assert feat.shape == h.shape == (4, 66, 80) and feat.dtype == h.dtype == torch.float32
    assert p.dtype == torch.int64 and p.tolist() == lens
    for b, n in enumerate(lens):
        assert torch.equal(feat[b, :n], feats[b]) and torch.equal(h[b, :n], hs[b])
        assert float(feat[b, n:].abs().sum()) == 0.0 and float(h[b, n:].abs().sum()) == 0.0
    # nobody has a prompt: one row of padding, so that the tensors are never empty
    feat, h, p = pad_prompts([torch.zeros(0, 80)] * 2, [torch.zeros(0, 80)] * 2)
    assert feat.shape == h.shape == (2, 1, 80) and p.tolist() == [0, 0] and float(feat.abs().sum()) == 0.0
    # other float types are converted
    feat, h, p = pad_prompts([feats[0].double()], [hs[0].half()])
    assert feat.dtype == h.dtype == torch.float32 and torch.equal(feat[0], feats[0]) and p.tolist() == [30]


def test_pad_prompts_errors():
    from jyutvoice_amd.utils.prompt import pad_prompts
    a, b = torch.zeros(10, 80), torch.zeros(12, 80)
    with pytest.raises(ValueError, match="utterance 1"):
        pad_prompts([a, a], [a, b])
    with pytest.raises(ValueError, match="2 prompt mels but 1"):
        pad_prompts([a, a], [a])
    with pytest.raises(ValueError, match="empty"):
        pad_prompts([], [])
    with pytest.raises(ValueError, match=r"feats\[0\]"):
        pad_prompts([torch.zeros(10, 79)], [a])
    with pytest.raises(ValueError, match=r"hs\[1\]"):
        pad_prompts([a, a], [a, torch.zeros(1, 10, 80)])


def test_synthesise_validates_prompt_lengths_on_the_host():
    """the argument checks of synthesise(..., prompt_lengths=...) are host code: they need no device"""
    from jyutvoice_amd.models.jyutvoice_tts import JyutVoiceTTS
    chk = JyutVoiceTTS._check_prompt_lengths
    feat, h = torch.zeros(3, 20, 80), torch.zeros(3, 16, 80)
    assert chk(torch.tensor([16, 0, 7]), feat, h, 3) == [16, 0, 7]
    assert chk(torch.tensor([1, 2, 3], dtype=torch.int32), feat, h, 3) == [1, 2, 3]
    for bad, match in ((torch.tensor([16, 17, 0]), "utterance 1"), (torch.tensor([0, 0, -1]), "utterance 2"),
                       (torch.tensor([1, 2]), "shape"), (torch.tensor([1.0, 2.0, 3.0]), "int"), ([1, 2, 3], "tensor")):
        with pytest.raises(ValueError, match=match):
            chk(bad, feat, h, 3)
    with pytest.raises(ValueError, match="prompt_h"):
        chk(torch.tensor([1, 2, 3]), feat, None, 3)
    with pytest.raises(ValueError, match="prompt_feat must be"):
        chk(torch.tensor([1, 2, 3]), torch.zeros(3, 80, 20), h, 3)
