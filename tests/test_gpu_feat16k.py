"""GPU: jv_fbank and jv_whisper_log_mel (feat16k.hip) -- `kaldi.fbank(x, num_mel_bins=80, dither=0, sample_frequency=16000)` minus its
mean over frames and `whisper.log_mel_spectrogram(x, n_mels=128)` (infer.py:98-163) for a ragged batch, one fused launch and one
finishing launch each -- against the fp64 restatements of tests/feat16k_ref.py.

Tolerance: the interval of feat16k_ref.py's error model per output -- |E_gpu - E| <= 8 c s in the energy domain, c the error of the
fp32 CPU chain on the same case, carried through the floor, the log, the mean over frames / the maximum -- asserted output by
output; before anything is compared every case asserts that at most 1 % of its intervals are wider than 1e-2.  Recorded per case
(parity_feat16k.json): c, the kernel's max |E_gpu - E| / s (recovered through the inverse of the log where off the floors), their
ratio, the share of wide intervals."""
import json

import numpy as np
import pytest
import torch

import feat16k_ref as ref
import resample_ref
from parity_util import Recorder

pytestmark = pytest.mark.gpu

FEATS = ["fbank", "whisper"]

REC = Recorder("parity_feat16k.json", {
    "what": "jv_fbank / jv_whisper_log_mel against the fp64 restatements (tests/feat16k_ref.py), per feature and case",
    "bound": "per output |E_gpu - E| <= 8 c s, s = sum_k M[m,k] |X_k| A_f + E, c = max |E32 - E| / s of the fp32 CPU chain on the case; "
             "asserted in the log domain by interval, output by output",
    "columns": "c = the fp32 CPU chain's, kernel = max |E_gpu - E| / s off the floors with E_gpu recovered from the STORED fp32 log (so it "
               "includes that value's own rounding, up to ln(10) |L| 2^-24 E, which the interval allows for separately), "
               "ratio = kernel / c (the bound allows 8 before that allowance), "
               "wide = share of the case's intervals wider than 1e-2 (allowed: 0.01)"})


@pytest.fixture
def eng():
    """the process's context with the Whisper filterbank loaded (looked up per test: re-loading weights replaces the context)"""
    from jyutvoice_amd.utils.audio import _engine16k
    return _engine16k(torch.device("cuda:0"))


def run(eng, feat, buf, lens=None, subtract_mean=True):
    if feat == "fbank":
        return eng.fbank(buf, lens, subtract_mean=subtract_mean)
    return eng.whisper_log_mel(buf, lens)


def rows(feat, out, b, T):
    """recording b's [T, 80] / [128, T] of a batch output, and what lies behind it"""
    if feat == "fbank":
        return out[b, :T], out[b, T:]
    return out[b, :, :T], out[b, :, T:]


def frames_of(feat, n):
    return ref.fbank_frames(n) if feat == "fbank" else ref.whisper_frames(n)


def pad_nan(recs, n=None):
    n = max(len(x) for x in recs) if n is None else n
    buf = torch.full((len(recs), n), float("nan"))
    for b, x in enumerate(recs):
        buf[b, : len(x)] = torch.from_numpy(np.ascontiguousarray(x))
    return buf, torch.tensor([len(x) for x in recs], dtype=torch.int32)


_runs = {}


def case_run(eng, feat, name):
    """the case's recordings in ONE call (NaN behind every length), computed once and shared: (out, out_lens, raw fbank out | None)"""
    if (feat, name) not in _runs:
        recs = ref.cases(feat)[name]
        buf, lens = pad_nan(recs)
        out, out_lens = run(eng, feat, buf, lens)
        raw = eng.fbank(buf, lens, subtract_mean=False)[0].cpu() if feat == "fbank" else None
        _runs[(feat, name)] = (out.cpu(), out_lens.cpu(), raw)
    return _runs[(feat, name)]


def check_case(eng, feat, name):
    recs = ref.cases(feat)[name]
    c, ivs = ref.case_intervals(feat, name)
    wide = ref.case_wide_share(feat, name)
    assert wide <= ref.WIDE_CAP, (feat, name, wide)      # the condition on the inputs, on the reference alone
    out, out_lens, raw = case_run(eng, feat, name)
    assert out_lens.dtype == torch.int32 and out_lens.tolist() == [frames_of(feat, len(x)) for x in recs]
    kernel, worst = 0.0, 0
    for b, (x, iv) in enumerate(zip(recs, ivs)):
        T = frames_of(feat, len(x))
        got, behind = rows(feat, out, b, T)
        assert torch.isfinite(got).all()
        assert torch.equal(behind, torch.zeros_like(behind)), (feat, name, b)
        if feat == "fbank":
            raw_got, raw_behind = rows(feat, raw, b, T)
            assert torch.equal(raw_behind, torch.zeros_like(raw_behind))
            g = raw_got.numpy().astype(np.float64)
            assert not ((g < iv.raw_lo) | (g > iv.raw_hi)).any(), (feat, name, b, "log values before the mean")
            kernel = max(kernel, iv.energy_ratio(g))
        else:
            kernel = max(kernel, iv.energy_ratio(got.numpy()))
        bad = iv.outside(got.numpy())
        worst = max(worst, int(bad.sum()))
        print(f"{feat} {name} [{b}]: {int(bad.sum())} of {bad.size} outputs outside their interval")
    REC(f"{feat} {name}", c=c, kernel=kernel, ratio=kernel / c, wide=wide)
    assert worst == 0, (feat, name, worst)


# ---- the intervals, at the shapes where the kernel can go wrong --------------------------------------------------------------------
@pytest.mark.parametrize("signal", ["speech", "uniform"])
@pytest.mark.parametrize("feat", FEATS)
def test_tile_seams(eng, feat, signal):
    """one recording of 20 011 samples (four tiles of 32 frames, the last one partial), EVERY output checked"""
    check_case(eng, feat, f"seams {signal}")


@pytest.mark.parametrize("feat", FEATS)
def test_recording_ends(eng, feat):
    """B = 40 in one call, NaN behind every length, the lengths crossing a frame-count step (fbank 5981 .. 6020: 6000; Whisper
    6061 .. 6100: 6080): every output in its interval, exact zeros behind, out_lens exact"""
    check_case(eng, feat, "ends")
    lens = ref.FBANK_ENDS if feat == "fbank" else ref.WHISPER_ENDS
    counts = {frames_of(feat, n) for n in lens}
    assert len(counts) == 2


def test_whisper_reflection_is_the_recordings_own(eng):
    """a row of the ends batch (its end inside the buffer, NaN behind) equals the same recording alone in a buffer that ends with it,
    bit for bit: the reflect index is taken at the recording's end, not the buffer's"""
    recs = ref.cases("whisper")["ends"]
    out, out_lens, _ = case_run(eng, "whisper", "ends")
    for b in (0, 19, 38):
        alone = eng.whisper_log_mel(torch.from_numpy(recs[b])[None]).cpu()
        T = int(out_lens[b])
        assert alone.shape == (1, 128, T) and torch.equal(alone[0], out[b, :, :T]), b


@pytest.mark.parametrize("feat", FEATS)
def test_smallest_recordings(eng, feat):
    """fbank at 399, 400, 559, 560 samples, Whisper at 200, 201, 319, 320, in one batch: 0, 1, 1, 2 frames, each in its interval; the
    zero-frame recording beside them changes nothing: the others equal themselves alone, bit for bit"""
    check_case(eng, feat, "smallest")
    recs = ref.cases(feat)["smallest"]
    out, out_lens, _ = case_run(eng, feat, "smallest")
    assert out_lens.tolist() == [0, 1, 1, 2]
    assert float(out[0].abs().sum()) == 0.0
    for b in (1, 2, 3):
        alone = run(eng, feat, torch.from_numpy(recs[b])[None]).cpu()
        T = int(out_lens[b])
        assert torch.equal(rows(feat, alone, 0, T)[0], rows(feat, out, b, T)[0]), b


@pytest.mark.parametrize("feat", FEATS)
def test_lengths_are_clamped(eng, feat):
    """negative lengths mean 0, over-long ones n (the header's "Lengths"), NaN behind each clamped length"""
    n = 2000
    x = ref.signal(31, 4 * n).reshape(4, n)
    lens = [-7, n + 1000, 1234, 0]
    buf = torch.from_numpy(x).clone()
    buf[2, 1234:] = float("nan")
    buf[0, :] = float("nan")
    buf[3, :] = float("nan")
    out, out_lens = run(eng, feat, buf, torch.tensor(lens, dtype=torch.int32))
    want, want_lens = run(eng, feat, buf, torch.tensor([0, n, 1234, 0], dtype=torch.int32))
    assert out_lens.tolist() == want_lens.tolist() == [0, frames_of(feat, n), frames_of(feat, 1234), 0]
    assert torch.equal(out, want) and torch.isfinite(out).all()
    full = run(eng, feat, torch.from_numpy(x[1:2]))
    T = frames_of(feat, n)
    assert torch.equal(rows(feat, out.cpu(), 1, T)[0], rows(feat, full.cpu(), 0, T)[0])


# ---- bit equality -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feat", FEATS)
def test_recording_alone_equals_its_row_in_a_batch_of_40(eng, feat):
    """mean-subtracted fbank and normalised Whisper of one recording alone, and at positions 0, 17 and 39 of a batch of 40 whose
    other members are longer, shorter and louder: the same bits (tiles start at the recording's frame 0; no atomics)"""
    x = ref.speech(7, 5555)
    alone = run(eng, feat, torch.from_numpy(x)[None]).cpu()
    T = frames_of(feat, x.size)
    others = ref.signal(8, 40 * 7000).reshape(40, 7000)
    recs = [others[b, : 3000 + 97 * b] for b in range(40)]
    for pos in (0, 17, 39):
        recs[pos] = x
    buf, lens = pad_nan(recs)
    out, out_lens = run(eng, feat, buf, lens)
    out = out.cpu()
    for pos in (0, 17, 39):
        assert int(out_lens[pos]) == T
        assert torch.equal(rows(feat, out, pos, T)[0], rows(feat, alone, 0, T)[0]), pos


def test_fbank_without_mean_plus_a_host_mean_agrees(eng):
    """subtract_mean = 0 is the log values themselves; minus their fp64 mean on the host they lie in the mean-subtracted intervals"""
    name = "seams speech"
    _, ivs = ref.case_intervals("fbank", name)
    _, _, raw = case_run(eng, "fbank", name)
    g = raw[0].numpy().astype(np.float64)
    assert not ivs[0].outside(g - g.mean(axis=0, keepdims=True)).any()


# ---- floors --------------------------------------------------------------------------------------------------------------------------
def test_quiet_fbank_sits_on_the_floor_and_in_its_intervals(eng):
    check_case(eng, "fbank", "quiet")
    _, _, raw = case_run(eng, "fbank", "quiet")
    on_floor = float((raw[0] == raw[0].min()).float().mean())
    assert on_floor > 0.05 and abs(float(raw[0].min()) - np.log(ref.EPS)) <= 4 * ref.U * (1 + abs(np.log(ref.EPS)))


def test_whisper_quiet(eng):
    check_case(eng, "whisper", "quiet")


def test_silence(eng):
    """an all-zero recording: fbank is log(eps) everywhere before the mean and 0 after it (to the mean's own rounding); Whisper is
    (-10 + 4) / 4 = -1.5 exactly"""
    z = torch.zeros(1, 6000)
    raw = eng.fbank(z, subtract_mean=False).cpu()
    le = float(np.log(ref.EPS))
    assert raw.shape == (1, 36, 80) and float((raw - le).abs().max()) <= 4 * ref.U * (1 + abs(le))
    assert bool((raw == raw[0, 0, 0]).all())
    sub = eng.fbank(z).cpu()
    assert float(sub.abs().max()) <= (36 + 2) * ref.U * abs(le) + ref.U * abs(le)
    w = eng.whisper_log_mel(z).cpu()
    assert w.shape == (1, 128, 37) and bool((w == -1.5).all())


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def test_errors_come_before_the_launch_and_leave_the_context_usable():
    """a context of its own: Whisper before its filters are loaded is JV_ERR_STATE; lens == NULL with n too short for a frame is
    JV_ERR_ARG; afterwards the same context computes what the shared one computes"""
    from jyutvoice_amd.engine import Engine, _ptr, _stream
    from jyutvoice_amd.utils.audio import whisper_filters
    fresh = Engine("cuda:0", 1, 64, 1)
    x = torch.from_numpy(ref.signal(41, 3000))[None].to(fresh.device)
    out = torch.empty(1, 128, 18, device=fresh.device)
    st = _stream(fresh.device)
    assert fresh.lib.jv_whisper_log_mel(fresh._h, _ptr(x), None, 1, 3000, _ptr(out), None, st) == 2      # JV_ERR_STATE
    assert b"jv_load_whisper_filters" in fresh.lib.jv_last_error()
    fresh.load_whisper_filters(whisper_filters())
    assert fresh.lib.jv_whisper_log_mel(fresh._h, _ptr(x), None, 1, 200, _ptr(out), None, st) == 1       # JV_ERR_ARG
    assert fresh.lib.jv_fbank(fresh._h, _ptr(x), None, 1, 399, 1, _ptr(out), None, st) == 1
    assert fresh.lib.jv_fbank(fresh._h, _ptr(x), None, -1, 3000, 1, _ptr(out), None, st) == 1
    bad = torch.zeros(5)
    assert fresh.lib.jv_load_whisper_filters(fresh._h, bad.data_ptr(), 5, 0, st) == 4                     # JV_ERR_SHAPE
    lens = torch.tensor([150], dtype=torch.int32, device=fresh.device)      # with lens the library cannot know: 0 frames, no error
    o, ol = fresh.whisper_log_mel(x, lens)
    assert ol.tolist() == [0] and float(o.abs().sum()) == 0.0
    from jyutvoice_amd.utils.audio import _engine16k
    shared = _engine16k(torch.device("cuda:0"))
    assert torch.equal(fresh.whisper_log_mel(x), shared.whisper_log_mel(x))
    assert torch.equal(fresh.fbank(x), shared.fbank(x))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_batch_extraction_at_mixed_rates_equals_resample_then_feature():
    """three recordings at 44 100, 16 000 and 24 000 Hz through extract_*_feat_batch(sample_rates=...): per recording the bits of
    `resample` alone followed by the single-recording feature"""
    from jyutvoice_amd.utils.audio import (extract_spk_feat, extract_spk_feat_batch, extract_token_feat_batch, log_mel_spectrogram,
                                           resample)
    rates, seconds = [44100, 16000, 24000], [0.63, 0.9, 0.5]
    gen = torch.Generator().manual_seed(23)
    wavs = [(torch.randn(1, int(s * r), generator=gen) * 0.2).clamp(-1, 1) for r, s in zip(rates, seconds)]
    fb, fb_len = extract_spk_feat_batch(wavs, sample_rates=rates)
    lm, lm_len = extract_token_feat_batch(wavs, sample_rates=rates)
    assert fb_len.dtype == torch.int32 and lm_len.dtype == torch.int32 and fb.shape[2] == 80 and lm.shape[1] == 128
    for b, (w, r) in enumerate(zip(wavs, rates)):
        w16 = resample(w, r, 16000)
        assert w16.shape == (1, resample_ref.out_length(w.shape[1], r, 16000))
        one_fb, one_lm = extract_spk_feat(w16), log_mel_spectrogram(w16[0])
        assert int(fb_len[b]) == one_fb.shape[0] == ref.fbank_frames(w16.shape[1])
        assert int(lm_len[b]) == one_lm.shape[1] == ref.whisper_frames(w16.shape[1])
        assert torch.equal(fb[b, : one_fb.shape[0]], one_fb) and float(fb[b, one_fb.shape[0]:].abs().sum()) == 0.0
        assert torch.equal(lm[b, :, : one_lm.shape[1]], one_lm) and float(lm[b, :, one_lm.shape[1]:].abs().sum()) == 0.0


def test_cli_dumps_the_reference_features(tmp_path, prompt_sd):
    """infer.py --dump-ref-features on a list of two cloning requests (44.1 kHz 24-bit stereo, 16 kHz 16-bit): the files hold what
    the API gives for the same recordings"""
    import infer
    from jyutvoice_amd import synth
    from jyutvoice_amd.flow.encoder import extract_flow_weights
    from jyutvoice_amd.utils.audio import extract_spk_feat_batch, extract_token_feat_batch, load_wav
    d = tmp_path
    torch.save(extract_flow_weights(dict(prompt_sd))[0], d / "flow_encoder.pt")
    torch.save({"state_dict": synth.tts_state_dict()}, d / "tts.ckpt")
    torch.save(synth.hift_state_dict(), d / "hift.pt")
    rng = np.random.default_rng(9)
    resample_ref.write_wav(d / "a.wav", rng.normal(0, 0.1, (30000, 2)).clip(-1, 1), 44100, 24)
    resample_ref.write_wav(d / "b.wav", rng.normal(0, 0.1, 12000).clip(-1, 1), 16000, 16)
    utts = []
    for b, name in enumerate(("a.wav", "b.wav")):
        u = synth.batch(1, 8 + 2 * b, first_index=b)
        tok, _ = synth.prompt_tokens(1, 20, first_index=b)
        obj = {k: u[k][0].tolist() for k in ("x", "lang", "tone", "word_pos", "syllable_pos")}
        obj.update({"interspersed": False, "spk_embed": u["spk_embed"][0].tolist(), "prompt_token": tok[0].tolist(),
                    "prompt_wav": str(d / name)})
        utts.append(obj)
    json.dump(utts, open(d / "list.json", "w"))
    infer.main(["--output", str(d / "o.wav"), "--tokens", str(d / "list.json"), "--dump-ref-features", str(d / "feats"),
                "--tts_checkpoint", str(d / "tts.ckpt"), "--hift", str(d / "hift.pt"), "--flow_encoder", str(d / "flow_encoder.pt"),
                "--n_timesteps", "2", "--seed", "7"])
    recs = [load_wav(str(d / name)) for name in ("a.wav", "b.wav")]
    fb, fb_len = extract_spk_feat_batch([w for w, _ in recs], [r for _, r in recs])
    lm, lm_len = extract_token_feat_batch([w for w, _ in recs], [r for _, r in recs])
    for b in range(2):
        f = np.load(d / "feats" / f"ref_{b:03d}_fbank.npy")
        m = np.load(d / "feats" / f"ref_{b:03d}_logmel.npy")
        assert f.dtype == np.float32 and f.shape == (int(fb_len[b]), 80) and m.shape == (128, int(lm_len[b]))
        assert np.array_equal(f, fb[b, : int(fb_len[b])].cpu().numpy()) and np.array_equal(m, lm[b, :, : int(lm_len[b])].cpu().numpy())
        assert (d / f"o_{b:03d}.wav").exists()
