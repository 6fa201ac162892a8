"""GPU: vocoder parity on audio the clamp does not hide.

Four older tests -- test_hift_ragged_batch_equals_singles, test_hift_pair_matches_separate_launches (the only oracle check of
hiftpair_kernel.h), test_vocoder_compact_geometry_equals_uniform, test_hift_tiny -- feed inputs that drive the synthetic checkpoint
far past HIFT_AUDIO_LIMIT: about four reference samples in five read +-0.99 on both sides whatever the kernels computed, so a
positional fault (a seam, a masked tail, a ragged boundary inside a tile) is invisible on most of the waveform.  These are their
twins on the quiet recipe of parity_util (same shapes, same seeds), plus a larger pair case (several workgroups per utterance
in the 64- and 128-channel pair kernels) and a hostile-checkpoint pair case (the pair kernel's intermediate scale is a
load-time bound).

Every case first asserts, on the fp64 reference alone, that at most 1 % of its samples are clamped.  Bit-equality assertions
are the older tests'.  Oracle comparisons take their bound from the reference: per utterance,
    floor = rms(fp32 oracle - fp64 oracle)          (fp64: fold_weight_norm's output cast to double)
    rms(gpu - fp64) <= 8 x floor                    (4: the 22-bit fp16x3 operand planes against fp32's 24 bits; 2: summation order)
    rms(fused - separate launches) <= 2 x 8 x floor (both satisfy the line above)
with the older tests' absolute 5e-5 kept as an outer cap.  Figures go to parity_vocoder_unclipped.json in the output directory
(JV_OUT; committed under profiles/)."""
import os

import pytest
import torch

import parity_util as pu

pytestmark = pytest.mark.gpu

RATIO, OUTER = 8.0, 5e-5
record = pu.Recorder("parity_vocoder_unclipped.json",
                     {"bound": "rms(gpu - fp64 oracle) <= 8 x floor and <= 5e-5, floor = rms(fp32 oracle - fp64 oracle) per utterance; "
                               "rms(fused - separate) <= 16 x floor", "input": "mel = randn, s = tanh(0.05 randn)",
                      "cap": "clamped share of the fp64 reference <= 1 %"})


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def make_engine(sd, max_batch, max_frames, **env):
    """a context of its own: the switches are read when it is created"""
    from jyutvoice_amd.engine import JV_MODEL_HIFT, Engine
    switches = ("JV_NO_COMPACT", "JV_NO_HIFT_PAIR")
    saved = {k: os.environ.pop(k, None) for k in switches}
    try:
        os.environ.update(env)
        e = Engine("cuda:0", max_batch=max_batch, max_frames=max_frames, max_tokens=32)
        e.load_state_dict(JV_MODEL_HIFT, sd)
    finally:
        for k in switches:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    return e


def decode(eng, mel, s, lens):
    wav = eng.hift_decode(mel, s, None if lens is None else torch.tensor(lens, dtype=torch.int32))
    torch.cuda.synchronize()
    return wav.cpu()


def references(sd, mel, s, lens, tag):
    """per utterance (fp64 reference, floor); the cap is asserted here, on the reference alone, before anything is compared"""
    w32, w64 = pu.hift_folded(sd)
    out = []
    for b, L in enumerate(lens):
        r64, r32 = pu.hift_fp64(w64, mel[b:b + 1], s[b:b + 1], L), pu.hift_fp32(w32, mel[b:b + 1], s[b:b + 1], L)
        share = pu.clamp_share(r64)
        record(f"{tag} utt{b} ({L} frames)", clamped_share=share, reference_rms=float(r64.pow(2).mean().sqrt()))
        assert share <= pu.CLAMP_CAP, (tag, b, share)
        floor = pu.rms(r32, r64)
        assert 0.0 < floor < OUTER, (tag, b, floor)
        out.append((r64, floor))
    return out


def check_against_reference(wav, refs, lens, T, tag):
    failures = []
    for b, L in enumerate(lens):
        r64, floor = refs[b]
        err = pu.rms(wav[b:b + 1, :480 * L], r64)
        record(f"{tag} utt{b} ({L} frames)", floor=floor, error=err, ratio=err / floor)
        if err > RATIO * floor or err > OUTER:
            failures.append(f"{tag} utt{b}: rms {err:.3e} = {err / floor:.2f} x the oracle's own {floor:.3e}")
        if L < T:
            assert float(wav[b, 480 * L:].abs().max()) == 0.0, (tag, b)
    assert not failures, failures


def test_ragged_batch_equals_singles_unclipped(hift_sd):
    mel, s, lens = pu.quiet_vocoder_inputs("ragged_24")
    refs = references(hift_sd, mel, s, lens, "ragged_24")
    eng = make_engine(hift_sd, 4, 512)
    try:
        wav = decode(eng, mel, s, lens)
    finally:
        eng.close()
    assert torch.isfinite(wav).all()
    check_against_reference(wav, refs, lens, 24, "ragged_24")


@pytest.mark.parametrize("case,kind", [("pair_61", "tame"), ("pair_151", "tame"), ("pair_61", "hostile")])
def test_pair_matches_separate_launches_unclipped(case, kind):
    assert kind in pu.GPU_CHECKPOINTS.get(case, ("tame",))
    sd = pu.hift_checkpoint(kind)
    mel, s, lens = pu.quiet_vocoder_inputs(case)
    T, tag = mel.shape[2], f"{case} {kind}"
    refs = references(sd, mel, s, lens, tag)
    out, reports = {}, {}
    for name, env in (("fused", {}), ("separate", {"JV_NO_HIFT_PAIR": "1"})):
        eng = make_engine(sd, 4, 512, **env)
        try:
            out[name] = decode(eng, mel, s, lens)
            reports[name] = pu.profiled(lambda: decode(eng, mel, s, lens))
        finally:
            eng.close()
    # the two runs did take the two forms, at both channel counts
    pairs = lambda rep: sorted(k for k in rep if k.startswith("hiftpair_h3<"))
    assert any(k.endswith("x64,snake>") for k in pairs(reports["fused"])) and any(k.endswith("x128,snake>") for k in pairs(reports["fused"])), sorted(reports["fused"])
    assert not pairs(reports["separate"]), pairs(reports["separate"])
    fused, separate = out["fused"], out["separate"]
    assert torch.isfinite(fused).all() and torch.isfinite(separate).all()
    assert not torch.equal(fused, separate)      # (different code: identical bits would mean the switch does nothing)
    check_against_reference(fused, refs, lens, T, tag + " fused")
    check_against_reference(separate, refs, lens, T, tag + " separate")
    failures = []
    for b, L in enumerate(lens):
        d, floor = pu.rms(fused[b, :480 * L], separate[b, :480 * L]), refs[b][1]
        record(f"{tag} fused vs separate utt{b} ({L} frames)", floor=floor, error=d, ratio=d / floor)
        if d > 2 * RATIO * floor:
            failures.append(f"{tag} utt{b}: fused - separate rms {d:.3e} = {d / floor:.2f} x floor {floor:.3e}")
    assert not failures, failures


def test_compact_geometry_equals_uniform_unclipped(hift_sd):
    mel, s, lens = pu.quiet_vocoder_inputs("compact_70")
    T = 70
    refs = references(hift_sd, mel, s, lens, "compact_70")
    out, reports = {}, {}
    for name, env in (("compact", {}), ("uniform", {"JV_NO_COMPACT": "1"})):
        eng = make_engine(hift_sd, 8, 512, **env)
        try:
            out[name] = decode(eng, mel, s, lens)
            reports[name] = pu.profiled(lambda: decode(eng, mel, s, lens))
        finally:
            eng.close()
    pu.assert_compact_taken(reports["compact"], reports["uniform"], lens, T, "hiftpair_h3<", "x128,snake>")
    compact, uniform = out["compact"], out["uniform"]
    assert torch.isfinite(compact).all()
    assert torch.equal(compact, uniform), pu.md(compact, uniform)
    check_against_reference(compact, refs, lens, T, "compact_70")


@pytest.mark.parametrize("T", [1, 2, 5])
def test_tiny_unclipped(hift_sd, T):
    mel, s, lens = pu.quiet_vocoder_inputs(f"tiny_{T}")
    refs = references(hift_sd, mel, s, lens, f"tiny_{T}")
    eng = make_engine(hift_sd, 4, 64)
    try:
        wav = decode(eng, mel, s, None)
    finally:
        eng.close()
    assert torch.isfinite(wav).all()
    check_against_reference(wav, refs, lens, T, f"tiny_{T}")
