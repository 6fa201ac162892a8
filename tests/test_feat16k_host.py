"""CPU: what of the 16 kHz reference-audio features (feat16k.hip: jv_fbank, jv_whisper_log_mel) needs no device -- the host-only
entry points against the definitions, the condition the GPU test's inputs must meet (feat16k_ref.py: at most 1 % of a case's
intervals wider than 1e-2), what those intervals catch (every mutant of the restatements lands outside them), the wrappers'
refusals, and the two ONNX-session mirrors against a fake session."""
import ctypes

import numpy as np
import pytest
import torch

import feat16k_ref as ref


@pytest.fixture(scope="module")
def lib():
    import os

    from jyutvoice_amd import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from jyutvoice_amd import _lib
    return _lib.load()


# ---- host-only entry points -------------------------------------------------------------------------------------------------------
def test_kaldi_mel_banks_match_the_fp64_formula(lib):
    """rounded once from fp64: at most 1 ulp of fp32 from the restatement's; bin 256 is zero in every row, no row is empty"""
    out = np.zeros((80, 257), dtype=np.float32)
    assert lib.jv_kaldi_mel_banks(out.ctypes.data_as(ctypes.c_void_p)) == 0
    want = ref.kaldi_banks()
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert (np.abs(out.astype(np.float64) - want) <= ulp).all()
    assert (out[:, 256] == 0).all() and (out.sum(axis=1) > 0).all() and (out >= 0).all()
    assert ((out > 0).sum(axis=1) >= 1).all()
    assert lib.jv_kaldi_mel_banks(None) != 0


def test_frame_counts(lib):
    for n, fb, wh in [(0, 0, 0), (199, 0, 0), (200, 0, 0), (201, 0, 1), (399, 0, 2), (400, 1, 2), (559, 1, 3), (560, 2, 3),
                      (16000, 98, 100)]:
        assert lib.jv_fbank_frames(n) == fb == ref.fbank_frames(n), n
        assert lib.jv_whisper_frames(n) == wh == ref.whisper_frames(n), n
    assert lib.jv_fbank_frames(-5) == 0 and lib.jv_whisper_frames(-5) == 0


def test_restatements_agree_with_their_own_shapes():
    x = ref.speech(1, 4000)
    assert ref.fbank64(x).shape == (ref.fbank_frames(4000), 80) and ref.whisper64(x).shape == (128, 25)
    assert np.abs(ref.fbank64(x).mean(axis=0)).max() < 1e-12
    w = ref.whisper64(x)
    assert w.max() - w.min() <= 2.0 + 1e-12      # the max - 8 clamp, divided by 4
    assert ref.fbank64(ref.signal(1, 399)).shape == (0, 80) and ref.whisper64(ref.signal(1, 200)).shape == (128, 0)


# ---- the condition on the inputs: asserted on the reference alone -------------------------------------------------------------------
@pytest.mark.parametrize("feat", ["fbank", "whisper"])
def test_wide_interval_condition_of_every_gpu_case(feat):
    for name in ref.cases(feat):
        c, ivs = ref.case_intervals(feat, name)
        share = ref.case_wide_share(feat, name)
        print(f"{feat} {name}: c = {c / ref.U:.2f} x 2^-24, intervals wider than 1e-2: {100 * share:.3f} %")
        assert 0 < c < 64 * ref.U, (feat, name, c)
        assert share <= ref.WIDE_CAP, (feat, name, share)
        for iv in ivs:
            assert (iv.lo <= iv.hi).all()


def test_quiet_signal_sits_on_the_floor():
    """on input in [-1, 1] the epsilon floor is not a corner case: a good part of the quiet case's fbank outputs is on it"""
    E = ref.fbank_energy(ref.quiet())[0]
    assert 0.05 < float((E < ref.EPS).mean()) < 0.9


# ---- what the intervals catch -------------------------------------------------------------------------------------------------------
def fbank_intervals(x):
    return ref.Intervals("fbank", x, ref.case_c("fbank", [x]))


def whisper_intervals(x):
    return ref.Intervals("whisper", x, ref.case_c("whisper", [x]))


@pytest.mark.parametrize("mutant", ref.FBANK_MUTANTS)
def test_fbank_mutants_land_outside(mutant):
    """the speech-like signal (the floor mutant on its quiet form, where outputs sit on the floor).  The definition itself is inside."""
    x = ref.quiet() if mutant == "floor_1e-10" else ref.speech(1, 6011)
    iv = fbank_intervals(x)
    assert not iv.outside(ref.fbank64(x)).any()
    bad = iv.outside(ref.fbank64(x, mutate=mutant, tmax=iv.lo.shape[0] + 3))
    print(f"{mutant}: {100 * bad.mean():.1f} % of the outputs outside")
    assert bad.any()


def test_preemphasis_pad_is_hidden_by_the_symmetric_window():
    """pre-emphasis with a[-1] = 0 differs from the replicate pad in element 0 of a frame alone (a[0] against 0.03 a[0]), and the
    symmetric Povey window is exactly 0 at i = 0: no output can tell the two apart, so no interval can either.  Shown rather than
    assumed: the conditioned frames are identical, and the difference exists before the window only."""
    x = ref.speech(1, 6011)
    assert ref.povey()[0] == 0.0
    good, slip = ref.fbank_conditioned(x), ref.fbank_conditioned(x, mutate="preemphasis_zero_pad")
    assert np.array_equal(good, slip) and np.array_equal(ref.fbank64(x), ref.fbank64(x, mutate="preemphasis_zero_pad"))
    frames = ref._frames(np.asarray(x, dtype=np.float64), 3)
    d = frames - frames.mean(axis=1, keepdims=True)
    assert (np.abs(d[:, 0] - 0.03 * d[:, 0]) > 0).all()      # before the window the two pads do differ


@pytest.mark.parametrize("mutant", ref.WHISPER_MUTANTS)
def test_whisper_mutants_land_outside(mutant):
    x = ref.speech(1, 6011)
    iv = whisper_intervals(x)
    assert not iv.outside(ref.whisper64(x)).any()
    if mutant == "last_frame_kept":      # one frame too many: the shape gives it away
        assert ref.whisper64(x, mutate=mutant).shape == (128, iv.lo.shape[1] + 1)
        return
    if mutant == "max_over_batch":       # beside a recording 100 times louder the quiet one's clamp rises
        x = (0.01 * x.astype(np.float64)).astype(np.float32)
        iv = whisper_intervals(x)
        loud = np.log10(np.maximum(ref.whisper_energy(ref.speech(1, 6011))[0], 1e-10)).max()
        bad = iv.outside(ref.whisper64(x, mutate=mutant, batch_max=loud))
    else:
        bad = iv.outside(ref.whisper64(x, mutate=mutant))
    print(f"{mutant}: {100 * bad.mean():.1f} % of the outputs outside")
    assert bad.any()


# ---- the wrappers' refusals (before any device work) ------------------------------------------------------------------------------
def test_wrappers_refuse_other_parameter_sets():
    from jyutvoice_amd.utils import audio
    x = torch.zeros(1, 1600)
    for kw in (dict(num_mel_bins=40), dict(dither=1.0), dict(sample_frequency=8000), dict(energy_floor=1.0), dict(frame_length=20.0)):
        with pytest.raises(NotImplementedError, match="num_mel_bins"):
            audio.fbank(x, **kw)
    for kw in (dict(n_mels=80), dict(padding=480000)):
        with pytest.raises(NotImplementedError, match="n_mels"):
            audio.log_mel_spectrogram(x[0], **kw)


def test_wrappers_refuse_what_the_reference_refuses():
    from jyutvoice_amd.utils import audio
    with pytest.raises(ValueError, match="more than 200"):
        audio.log_mel_spectrogram(torch.zeros(200))
    with pytest.raises(ValueError, match="recording 1"):
        audio.extract_token_feat_batch([torch.zeros(4000), torch.zeros(500)], sample_rates=[16000, 44100])      # 182 samples at 16 kHz
    with pytest.raises(ValueError, match="no recordings"):
        audio.extract_spk_feat_batch([])
    with pytest.raises(ValueError, match="sample rates"):
        audio.extract_token_feat_batch([torch.zeros(4000)], sample_rates=[16000, 16000])
    with pytest.raises(ValueError, match=r"\[n\] or \[B, n\]"):
        audio.fbank(torch.zeros(1, 1, 1600))
    with pytest.raises(ValueError, match="torch.Tensor or numpy.ndarray"):
        audio.extract_speech_token([0.0] * 400, FakeSession(["a", "b"], None))
    assert audio.fbank(torch.zeros(1, 399), device="cpu").shape == (0, 80)      # no frame: empty, as the reference


# ---- the two session mirrors ------------------------------------------------------------------------------------------------------
class FakeInput:
    def __init__(self, name):
        self.name = name


class FakeSession:
    """what infer.py:98-163 use of an onnxruntime session: .get_inputs()[i].name and .run(None, feeds)"""

    def __init__(self, names, result):
        self.names, self.result, self.feeds = names, result, None

    def get_inputs(self):
        return [FakeInput(n) for n in self.names]

    def run(self, outputs, feeds):
        assert outputs is None
        self.feeds = feeds
        return [self.result]


def test_session_mirrors_feed_what_the_reference_feeds(monkeypatch):
    """the features replaced by the fp64 restatement (no device here): names, shapes and dtypes of the feeds, shapes of the results"""
    from jyutvoice_amd.utils import audio
    x = ref.speech(5, 4000)
    monkeypatch.setattr(audio, "extract_spk_feat", lambda speech, device="cuda:0": torch.from_numpy(ref.fbank64(speech.numpy().reshape(-1))).float())
    monkeypatch.setattr(audio, "log_mel_spectrogram",
                        lambda a, n_mels=128, device="cuda:0": torch.from_numpy(ref.whisper64(a.numpy().reshape(-1))).float()[None])
    spk = FakeSession(["input"], np.arange(192, dtype=np.float32).reshape(1, 192))
    emb = audio.extract_spk_embedding(spk, torch.from_numpy(x)[None])
    assert list(spk.feeds) == ["input"] and spk.feeds["input"].shape == (1, 23, 80) and spk.feeds["input"].dtype == np.float32
    assert emb.shape == (1, 192) and emb.dtype == torch.float32 and emb[0, 5] == 5
    tok = FakeSession(["feats", "feats_length"], np.arange(12, dtype=np.int64).reshape(1, 12))
    for audio_in in (torch.from_numpy(x), x):
        token, token_len = audio.extract_speech_token(audio_in, tok)
        assert list(tok.feeds) == ["feats", "feats_length"]
        assert tok.feeds["feats"].shape == (1, 128, 25) and tok.feeds["feats"].dtype == np.float32
        assert tok.feeds["feats_length"].dtype == np.int32 and tok.feeds["feats_length"].tolist() == [25]
        assert token.shape == (1, 12) and token.dtype == torch.int32 and token_len.tolist() == [12] and token_len.dtype == torch.int32


def test_whisper_filters_are_the_published_construction():
    from jyutvoice_amd.utils.audio import slaney_mel_basis, whisper_filters
    f = whisper_filters()
    assert f.shape == (128, 201) and f.dtype == torch.float32 and bool((f >= 0).all()) and bool((f.sum(dim=1) > 0).all())
    try:
        import whisper  # noqa: F401
    except ImportError:
        assert np.array_equal(f.numpy(), slaney_mel_basis(16000, 400, 128, 0.0, 8000.0))
