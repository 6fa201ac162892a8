"""GPU: streaming token-to-wav -- jv_hift_source_cont, jv_flow_encoder_fwd_partial / jv_flow_token2mel_partial, windowed decode,
`HiFTStream`, `Token2WavStream` and `infer.py --stream-hop`.

What is bit-exact is asserted with torch.equal (the source continuation over any split; a stream that receives everything at once
against `inference`).  What runs the same arithmetic in another launch geometry takes the bounds the project already holds that
property to: 5e-5 / 1e-3 for the encoder / the mel against the imported reference (G15, as G13 / G14), 2e-5 for the frames of an
aligned prefix against the one-shot mel (test_streaming_two_chunks), and for waveforms the rule of test_gpu_vocoder_unclipped.py:
rms <= 8 x floor (16 x between two GPU decodes) and <= 5e-5, floor = rms(fp32 oracle - fp64 oracle), on inputs whose fp64 reference
clamps at most 1 % of its samples.  Figures go to parity_stream.json in the output directory (JV_OUT; committed under profiles/)."""
import json
import os

import pytest
import torch

import parity_util as pu
import stream_ref as sr
import token2mel_cases as tc
from conftest import load_golden

pytestmark = pytest.mark.gpu

RATIO, OUTER = 8.0, 5e-5
record = pu.Recorder("parity_stream.json",
                     {"waveform bound": "rms(gpu - fp64 oracle) <= 8 x floor and <= 5e-5; rms(window - whole, both GPU) <= 16 x floor; floor = "
                                        "rms(fp32 oracle - fp64 oracle)",
                      "mel bound": "encoder 5e-5 and mel 1e-3 against G15; prefix frames against the one-shot mel 2e-5",
                      "f0 bound": "max abs(streamed f0 record - one-shot f0) <= 8 x max abs(fp32 oracle - fp64 oracle)",
                      "cap": "clamped share of the fp64 reference <= 1 %"})


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    torch.set_num_threads(min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def hift(hift_sd):
    import jyutvoice_amd
    h = jyutvoice_amd.build_default("cuda:0")[1]
    h.load_state_dict(hift_sd)
    return h


@pytest.fixture(scope="module")
def eng(hift):
    return hift._engine(2, 192)


@pytest.fixture(scope="module")
def folded(hift_sd):
    return pu.hift_folded(hift_sd)


@pytest.fixture(scope="module")
def flow(prompt_sd, tts_sd):
    from jyutvoice_amd.flow.flow import CausalMaskedDiffWithXvec
    from jyutvoice_amd.runtime import Runtime
    m = CausalMaskedDiffWithXvec(vocab_size=6561, input_frame_rate=25, runtime=Runtime("cuda:0"))
    m.load_state_dict(tc.flow_sd(prompt_sd, tts_sd))
    return m


def session_args(n):
    tok, ptok, feat, emb = sr.session_inputs()
    return tok[:, :n], torch.tensor([n]), ptok, torch.tensor([sr.P]), feat, torch.tensor([sr.F]), emb


@pytest.fixture(scope="module")
def oneshot(flow):
    """the one-shot streaming mel of the session case, [1, 80, 140]: computed once, shared, not modified"""
    mel, _ = flow.inference(*session_args(sr.N), True, True, n_timesteps=sr.N_TIMESTEPS)
    assert mel.shape == (1, 80, 2 * (sr.P + sr.N) - sr.F)
    return mel


# ---- 1. source continuation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
def test_source_continuation_is_bit_identical(eng, B):
    """37 frames with unvoiced frames and a near-zero one (the sequential path of frame_adds_exact), split 1 / 11 / 25 and 37 x 1"""
    f0, phase = sr.f0_case()
    f0, phase = f0[:B].cuda(), phase[:B].cuda()
    seed, call = 0x1234567890ABCDEF, 7
    whole = eng.hift_source_seeded(f0, phase, seed, call)
    assert whole.shape == (B, 1, 480 * 37) and torch.isfinite(whole).all()
    for split in ([1, 11, 25], [1] * 37):
        cum = torch.zeros(B, 9, dtype=torch.float64, device="cuda")
        pieces, t0 = [], 0
        for t in split:
            pieces.append(eng.hift_source_cont(f0[:, t0:t0 + t], phase, seed, call, 480 * t0, cum))
            t0 += t
        got = torch.cat(pieces, dim=2)
        assert torch.equal(got, whole), (B, split, pu.md(got, whole))
        assert float(cum.abs().max()) > 0.0
    # the counters are absolute: the same piece at another offset is another noise
    cum = torch.zeros(B, 9, dtype=torch.float64, device="cuda")
    assert not torch.equal(eng.hift_source_cont(f0[:, :5], phase, seed, call, 480, cum), whole[:, :, :2400])
    with pytest.raises(ValueError, match="cum must be a contiguous float64"):
        eng.hift_source_cont(f0, phase, seed, call, 0, torch.zeros(B, 9, device="cuda"))
    with pytest.raises(ValueError, match="sample0 must be non-negative"):
        eng.hift_source_cont(f0, phase, seed, call, -480, cum)


# ---- 2. partial flow ---------------------------------------------------------------------------------------------------------------
def test_partial_flow_against_reference(flow):
    """G15: m = 40 tokens (P = 7), L = 37 -- not a multiple of the chunk -- F = 14; the encoder to 5e-5, the mel (10 steps, as the
    reference solves) to 1e-3, both streaming values"""
    g = load_golden("G15_flow_partial")
    e = flow._rt().ensure(1, 256, 1)
    for tag, streaming in (("full", False), ("stream", True)):
        h, hl = e.flow_encoder_partial(g["prompt_token"], torch.tensor([7]), g["token"], torch.tensor([33]), streaming=streaming)
        assert h.shape == (1, 74, 80) and hl.tolist() == [74]
        err_h = pu.md(h, g["h_" + tag])
        mel, none = flow.inference_partial(g["token"], torch.tensor([33]), g["prompt_token"], torch.tensor([7]), g["prompt_feat"],
                                           torch.tensor([14]), g["embedding"], streaming)
        assert none is None and mel.dtype == torch.float32 and mel.shape == (1, 80, 60) and flow.mel_lengths.tolist() == [60]
        err_mel = pu.md(mel, g["mel_" + tag])
        record(f"G15 {tag}", encoder=err_h, mel=err_mel)
        assert err_h <= 5e-5, tag
        assert err_mel <= 1e-3, tag
    # the context is read: the whole-sequence entry on the same 37 tokens pads with zeros and lands elsewhere (the reference: 0.76)
    ids = torch.cat([g["prompt_token"], g["token"]], dim=1)
    hz, _ = e.flow_encoder(None, None, ids[:, :37], torch.tensor([37]), streaming=True)
    assert pu.md(hz, g["h_stream"]) > 1e-2


def test_partial_flow_prefix_is_final(flow, oneshot, prompt_sd, tts_sd, noise):
    """L = 25 and 50: inference_partial on the first L + 3 tokens = the first 2 L - F frames of the one-shot streaming mel, to 2e-5.
    Both routes' errors against the fp64 oracle are recorded beside it."""
    from oracle import token2mel as ot2m
    tok, ptok, feat, emb = sr.session_inputs()
    with torch.inference_mode():
        ref64, _ = ot2m.token2mel(tc.flow_sd(prompt_sd, tts_sd), noise, tok, torch.tensor([sr.N]), ptok, torch.tensor([sr.P]), feat,
                                  torch.tensor([sr.F]), emb, True, n_timesteps=sr.N_TIMESTEPS, dtype=torch.float64)
    failures = []
    for L in (25, 50):
        k = 2 * L - sr.F
        mel, _ = flow.inference_partial(*session_args(L + 3 - sr.P), True, n_timesteps=sr.N_TIMESTEPS)
        assert mel.shape == (1, 80, k)
        e = pu.md(mel, oneshot[:, :, :k])
        record(f"prefix L={L}", partial_vs_oneshot=e, partial_vs_fp64=pu.md(mel, ref64[:, :, :k]),
               oneshot_vs_fp64=pu.md(oneshot[:, :, :k], ref64[:, :, :k]))
        if e > 2e-5:
            failures.append((L, e))
    assert not failures, failures


# ---- 3. windowed decode ------------------------------------------------------------------------------------------------------------
def test_windowed_decode_matches_whole(eng, folded):
    w32, w64 = folded
    mel, s = sr.vocoder_inputs()
    r64, r32 = pu.hift_fp64(w64, mel, s, sr.T_VOC), pu.hift_fp32(w32, mel, s, sr.T_VOC)
    share, floor = pu.clamp_share(r64), pu.rms(r32, r64)
    record("windowed reference", clamped_share=share, floor=floor)
    assert share <= pu.CLAMP_CAP and 0.0 < floor < OUTER
    whole = eng.hift_decode(mel, s).cpu()
    record("windowed whole", error=pu.rms(whole, r64), ratio=pu.rms(whole, r64) / floor)
    failures = []
    for lo, hi in sr.KEPT:
        a, b = sr.window_of(lo, hi, 16, sr.T_VOC)
        win = eng.hift_decode(mel[:, :, a:b], s[:, :, 480 * a:480 * b]).cpu()[:, 480 * (lo - a):480 * (hi - a)]
        d = pu.rms(win, whole[:, 480 * lo:480 * hi])
        record(f"window [{a}, {b}) keeps [{lo}, {hi})", error=d, ratio=d / floor)
        if d > 2 * RATIO * floor or d > OUTER:
            failures.append(f"[{lo}, {hi}): rms {d:.3e} = {d / floor:.2f} x floor {floor:.3e}")
    assert not failures, failures


# ---- 4. HiFTStream -----------------------------------------------------------------------------------------------------------------
def check_wave(tag, wav, mel, s, folded):
    """waveform against the fp64 oracle's decode of (mel, the assembled s)"""
    w32, w64 = folded
    T = mel.shape[2]
    mel, s = mel.cpu(), s.cpu()
    r64, r32 = pu.hift_fp64(w64, mel, s, T), pu.hift_fp32(w32, mel, s, T)
    share, floor, err = pu.clamp_share(r64), pu.rms(r32, r64), pu.rms(wav, r64)
    record(tag, clamped_share=share, floor=floor, error=err, ratio=err / floor)
    assert share <= pu.CLAMP_CAP, (tag, share)
    assert 0.0 < floor < OUTER, (tag, floor)
    assert err <= RATIO * floor and err <= OUTER, f"{tag}: rms {err:.3e} = {err / floor:.2f} x the oracle's own {floor:.3e}"


@pytest.mark.parametrize("name,split", [("50_50_30", [50, 50, 30]), ("130x1", [1] * 130), ("7_123", [7, 123])])
def test_hift_stream(hift, eng, folded, name, split):
    mel, _ = sr.vocoder_inputs()
    hift.manual_seed(5)
    st = hift.stream()
    wavs, ss, t0 = [], [], 0
    for t in split:
        w, s = st.push(mel[:, :, t0:t0 + t])
        assert w.shape[0] == 1 and s.shape == (1, 1, w.shape[1]) and w.shape[1] % 480 == 0
        wavs.append(w)
        ss.append(s)
        t0 += t
    counts, rest = sr.hift_stream_counts(split)
    assert [w.shape[1] // 480 for w in wavs] == counts
    w, s = st.finish()
    assert w.shape[1] == 480 * rest
    wav, src = torch.cat(wavs + [w], dim=1), torch.cat(ss + [s], dim=2)
    assert wav.shape == (1, 62400) and src.shape == (1, 1, 62400) and torch.isfinite(wav).all()
    assert st.f0.shape == (1, 130) and st.received == st.sourced == st.emitted == 130
    # the assembled source is the one-shot source of the stream's own f0 record, bit for bit
    assert torch.equal(src, eng.hift_source_seeded(st.f0, st._phase, st._seed, st._call))
    # the f0 record against the one-shot f0
    w32, w64 = folded
    from oracle import hift as ohift
    with torch.inference_mode():
        f0_floor = pu.md(ohift.f0_predict(w32, mel), ohift.f0_predict(w64, mel.double()))
    f0_err = pu.md(st.f0, eng.hift_f0(mel))
    record(f"HiFTStream {name} f0", floor=f0_floor, error=f0_err)
    assert f0_floor > 0.0 and f0_err <= 8 * f0_floor, (f0_err, f0_floor)
    check_wave(f"HiFTStream {name}", wav.cpu(), mel, src, folded)
    with pytest.raises(RuntimeError, match="finish\\(\\) has been called"):
        st.push(mel[:, :, :1])


def test_hift_stream_all_at_once_is_inference(hift):
    """a stream opened after manual_seed(x) uses the draws `inference` uses after manual_seed(x): given the whole mel at once it
    computes f0, source and waveform on the same windows, so the same bits"""
    mel, _ = sr.vocoder_inputs()
    hift.manual_seed(11)
    wav, s = hift.inference(mel)
    hift.manual_seed(11)
    wav2, s2 = hift.stream().finish(mel)
    assert torch.equal(s, s2) and torch.equal(wav, wav2)


# ---- 5. Token2WavStream --------------------------------------------------------------------------------------------------------------
def test_token2wav_stream(flow, hift, oneshot, folded):
    from jyutvoice_amd.stream import Token2WavStream
    tok, ptok, feat, emb = sr.session_inputs()
    session = Token2WavStream(flow, hift, ptok, feat, emb, max_tokens=sr.N, n_timesteps=sr.N_TIMESTEPS, seed=3)
    caps = (flow._rt().caps, hift._engine(1, 1).max_frames)
    wavs, t0 = [], 0
    for n in sr.HOPS:
        wavs.append(session.push(tok[0, t0:t0 + n]))
        t0 += n
    assert t0 == sr.N
    wavs.append(session.finish())
    # 28 / 53 / 77 tokens: mel frames [0, 36), [36, 86), nothing, [86, 140); the vocoder trails by 21 frames
    assert [w.shape[1] for w in wavs] == [480 * 15, 480 * 50, 0, 480 * 75]
    assert (flow._rt().caps, hift._engine(1, 1).max_frames) == caps      # no push rebuilt a context
    wav = torch.cat(wavs, dim=1)
    assert wav.shape == (1, 67200) and session.mel.shape == (1, 80, 140) and session.source.shape == (1, 1, 67200)
    failures = []
    for lo, hi in ((0, 36), (36, 86), (86, 140)):
        e = pu.md(session.mel[:, :, lo:hi], oneshot[:, :, lo:hi])
        record(f"session mel [{lo}, {hi})", vs_oneshot=e)
        if e > 2e-5:
            failures.append((lo, hi, e))
    assert not failures, failures
    check_wave("Token2WavStream", wav.cpu(), session.mel, session.source, folded)
    with pytest.raises(ValueError, match="exceed the session's max_tokens"):
        Token2WavStream(flow, hift, ptok, feat, emb, max_tokens=5, n_timesteps=sr.N_TIMESTEPS).push(tok[0, :6])
    # pushes that complete no chunk past the prompt return empty tensors; the first that does returns audio -- the same audio
    again = Token2WavStream(flow, hift, ptok, feat, emb, max_tokens=sr.N, n_timesteps=sr.N_TIMESTEPS, seed=3)
    first, second = again.push(tok[0, :10]), again.push(tok[0, 10:21])
    assert first.shape == (1, 0) and torch.equal(second, wavs[0])
    with pytest.raises(NotImplementedError):
        flow.inference(*session_args(sr.N), True, False)


# ---- 6. CLI --------------------------------------------------------------------------------------------------------------------------
def test_cli_stream_hop(tmp_path):
    """the session route of infer.py writes files of the same length as the batch route"""
    import infer
    from jyutvoice_amd.utils.audio import load_wav
    tok, ptok, feat, emb = sr.session_inputs()
    reqs = [{"speech_token": tok[0, :55].tolist(), "embedding": emb[0].tolist(), "prompt_token": ptok[0].tolist(), "prompt_feat": feat[0].tolist()},
            {"speech_token": tok[0, 55:].tolist(), "embedding": emb[0].tolist()}]
    (tmp_path / "list.json").write_text(json.dumps(reqs))
    base = ["--token2wav", str(tmp_path / "list.json"), "--synthetic", "1", "--n_timesteps", "2", "--streaming"]
    infer.main(["--output", str(tmp_path / "a.wav")] + base)
    infer.main(["--output", str(tmp_path / "b.wav")] + base + ["--stream-hop", "25"])
    for b, frames in enumerate([2 * 62 - 14, 2 * 15]):
        one, rate = load_wav(str(tmp_path / f"a_{b:03d}.wav"))
        hop, rate2 = load_wav(str(tmp_path / f"b_{b:03d}.wav"))
        assert rate == rate2 == 24000 and one.shape[-1] == hop.shape[-1] == 480 * frames
        assert torch.isfinite(hop).all() and float(hop.abs().max()) > 1e-4
