"""`mel_spectrogram` / `extract_speech_feat` drop-ins (jyutvoice/utils/audio.py:18-63, infer.py:166-186): the prompt mel of
the voice-cloning branch, computed on the GPU by libjyutvoice_hip.so (jv_mel_spectrogram: STFT as a GEMM against a windowed
DFT basis, magnitude, mel projection, log) -- and what infer.py:368-382 does before it: `load_wav` reads the recording at whatever
rate the file has, `resample` converts it on the GPU (jv_resample: torchaudio.functional.resample with its defaults).

The mel filterbank is data handed to the library.  The reference takes it from `librosa.filters.mel`; when librosa is
importable it is used here too, otherwise `slaney_mel_basis` evaluates the same published construction (Slaney mel scale,
triangular filters on the FFT bin centres, area normalisation) so that the module works without it."""
from __future__ import annotations

import math
import struct

import numpy as np
import torch

from ..runtime import get_runtime

_PARAMS = dict(n_fft=1920, num_mels=80, sampling_rate=24000, hop_size=480, win_size=1920, fmin=0, fmax=8000)


def slaney_mel_basis(sr=24000, n_fft=1920, n_mels=80, fmin=0.0, fmax=8000.0) -> np.ndarray:
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, math.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp

    def hz_to_mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-30) / min_log_hz) / logstep, f / f_sp)

    def mel_to_hz(m):
        m = np.asarray(m, dtype=np.float64)
        return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)

    fftfreqs = np.linspace(0, float(sr) / 2, 1 + n_fft // 2)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    weights = np.zeros((n_mels, 1 + n_fft // 2), dtype=np.float32)
    for i in range(n_mels):
        weights[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    weights *= (2.0 / (mel_f[2: n_mels + 2] - mel_f[:n_mels]))[:, np.newaxis]
    return weights


def mel_basis() -> torch.Tensor:
    try:
        from librosa.filters import mel as librosa_mel_fn
        m = librosa_mel_fn(sr=24000, n_fft=1920, n_mels=80, fmin=0, fmax=8000)
    except ImportError:
        m = slaney_mel_basis()
    return torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32))


def mel_spectrogram(y, n_fft=1920, num_mels=80, sampling_rate=24000, hop_size=480, win_size=1920, fmin=0, fmax=8000,
                    center=False, device="cuda:0"):
    """y [B, n] -> log-mel [B, 80, T] on the GPU; only the parameter set `extract_speech_feat` uses is built"""
    got = dict(n_fft=n_fft, num_mels=num_mels, sampling_rate=sampling_rate, hop_size=hop_size, win_size=win_size, fmin=fmin,
               fmax=fmax)
    if got != _PARAMS or center:
        raise NotImplementedError(f"libjyutvoice_hip computes the prompt mel of infer.py:166-186 only ({_PARAMS}, center=False)")
    if float(y.min()) < -1.0:
        print("min value is ", float(y.min()))
    if float(y.max()) > 1.0:
        print("max value is ", float(y.max()))
    dev = y.device if y.is_cuda else torch.device(device)
    return _engine(dev).mel_spectrogram(y)


def _engine(dev):
    eng = get_runtime(dev).ensure(1, 64, 1)
    # the flag lives on the context's own object: id(eng) in a module-level set outlived the engine, and a rebuilt context that
    # got a freed engine's id was taken for one that had the filterbank
    if not getattr(eng, "mel_basis_loaded", False):
        eng.load_mel_basis(mel_basis())
        eng.mel_basis_loaded = True
    return eng


def extract_speech_feat(speech, device="cuda:0"):
    """infer.py:166-186: speech [1, n] at 24 kHz -> (speech_feat [1, T, 80], speech_feat_len [1] int32)"""
    feat = mel_spectrogram(speech, device=device, **_PARAMS).squeeze(dim=0).transpose(0, 1).unsqueeze(dim=0)
    return feat, torch.tensor([feat.shape[1]], dtype=torch.int32, device=feat.device)


def extract_speech_feat_batch(speeches, device="cuda:0", sample_rates=None, lengths=None):
    """`extract_speech_feat` of several recordings of different durations in one GPU pass (jv_mel_spectrogram_ragged):
    speeches = list of [1, n_b] or [n_b] tensors at 24 kHz -> (speech_feat [B, Tmax, 80], zero behind each recording's frames,
    speech_feat_len [B] int32).  Recording b's frames are those of `extract_speech_feat(speeches[b])`, bit for bit.

    sample_rates (one int per recording): the recordings come at rates of their own (infer.py:368-382).  They are grouped by
    rate, each group goes through one ragged `jv_resample` call to 24 kHz, and the lengths it leaves on the device feed the
    ragged mel pass: recording b's frames are those of `extract_speech_feat(resample(speeches[b], sample_rates[b], 24000))`,
    bit for bit.  None is the 24 kHz path above, untouched.

    lengths ([B] int32 on the device, what `condition_prompt` returns): recording b is speeches[b][:lengths[b]] and the rows may
    be longer; the lengths never come down to the host here."""
    wavs = [s.reshape(-1).to(torch.float32) for s in speeches]
    if not wavs:
        raise ValueError("extract_speech_feat_batch: no recordings")
    lengths = _device_lengths("extract_speech_feat_batch", lengths, len(wavs), torch.device(device))
    if sample_rates is not None:
        return _extract_resampled(wavs, [int(r) for r in sample_rates], torch.device(device), lengths)
    buf, lens = _rows_of(wavs, range(len(wavs)), lengths)
    mel, mel_lens = _engine(torch.device(device)).mel_spectrogram(buf, lens)
    return mel.transpose(1, 2).contiguous(), mel_lens


def _pad_rows(wavs):
    lens = torch.tensor([w.numel() for w in wavs], dtype=torch.int32)
    buf = torch.zeros(len(wavs), int(lens.max()), dtype=torch.float32)
    for b, w in enumerate(wavs):
        buf[b, : w.numel()] = w.cpu()
    return buf, lens


def _device_lengths(who, lengths, B, dev):
    if lengths is None:
        return None
    lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32)
    if lengths.shape != (B,):
        raise ValueError(f"{who}: lengths must have shape [{B}], got {tuple(lengths.shape)}")
    return lengths


def _rows_of(wavs, members, lengths):
    """the rows `members` as one padded batch and their lengths: from the rows' sizes on the host (`_pad_rows`), or -- with
    device lengths -- stacked where the rows are, the lengths gathered on the device"""
    members = list(members)
    if lengths is None:
        return _pad_rows([wavs[b] for b in members])
    buf = torch.zeros(len(members), max(wavs[b].numel() for b in members), device=lengths.device)
    for i, b in enumerate(members):
        buf[i, : wavs[b].numel()] = wavs[b]
    return buf, lengths[torch.tensor(members, device=lengths.device)]


def _extract_resampled(wavs, rates, dev, lengths=None):
    if len(rates) != len(wavs):
        raise ValueError(f"extract_speech_feat_batch: {len(wavs)} recordings, {len(rates)} sample rates")
    eng = _engine(dev)
    groups = {}
    for b, r in enumerate(rates):
        groups.setdefault(r, []).append(b)
    done = []
    for r, members in groups.items():      # one ragged launch per rate; nothing comes back to the host
        buf, lens = _rows_of(wavs, members, lengths)
        out, out_lens = eng.resample(buf, r, _PARAMS["sampling_rate"], lens)
        done.append((torch.tensor(members, device=out.device), out, out_lens))
    wav24 = torch.zeros(len(wavs), max(out.shape[1] for _, out, _ in done), device=done[0][1].device)
    lens24 = torch.zeros(len(wavs), dtype=torch.int32, device=wav24.device)
    for idx, out, out_lens in done:
        wav24[idx, : out.shape[1]] = out
        lens24[idx] = out_lens
    mel, mel_lens = eng.mel_spectrogram(wav24, lens24)
    return mel.transpose(1, 2).contiguous(), mel_lens


# ---- infer.py:368-382: the recording at its own rate, and its 16 / 24 kHz copies ----------------------------------------------
def resample_length(n, orig_freq, new_freq):
    """samples that n samples at orig_freq become at new_freq: ceil(new n / orig) in reduced integers (jv_resample_length)"""
    from .. import _lib
    got = int(_lib.load().jv_resample_length(int(n), int(orig_freq), int(new_freq)))
    if got < 0:
        raise ValueError(f"resample_length: need n >= 0 and positive rates, got n = {n}, {orig_freq} -> {new_freq}")
    return got


def resample(waveform, orig_freq, new_freq, lengths=None, device="cuda:0"):
    """`torchaudio.functional.resample(waveform, orig_freq, new_freq)` with its defaults -- what the two
    `torchaudio.transforms.Resample` of infer.py:368-382 compute -- on the GPU (jv_resample).  waveform [n] or [B, n] -> the same
    rank, resample_length(n) samples.  lengths ([B] sample counts): recordings of different durations in one call, recording b
    = waveform[b, :lengths[b]]; returns (out, out_lengths int32 [B]) with zeros behind each recording's samples."""
    if waveform.dim() not in (1, 2):
        raise ValueError(f"resample: waveform must be [n] or [B, n], got {tuple(waveform.shape)}")
    dev = waveform.device if waveform.is_cuda else torch.device(device)
    eng = get_runtime(dev).ensure(1, 64, 1)
    res = eng.resample(waveform if waveform.dim() == 2 else waveform.unsqueeze(0), orig_freq, new_freq, lengths)
    if lengths is not None:
        return res
    return res if waveform.dim() == 2 else res.squeeze(0)


# ---- levels: what a CosyVoice2 front-end does to a prompt before any feature, and programme loudness of the output ------------
def _level_rows(who, wavs, lens, device):
    if not isinstance(wavs, torch.Tensor):
        wavs = torch.as_tensor(np.asarray(wavs))
    if wavs.dim() not in (1, 2):
        raise ValueError(f"{who}: wavs must be [n] or [B, n], got {tuple(wavs.shape)}")
    if wavs.dim() == 1 and lens is not None:
        raise ValueError(f"{who}: lens needs wavs as [B, n]")
    dev = wavs.device if wavs.is_cuda else torch.device(device)
    return get_runtime(dev).ensure(1, 64, 1), wavs.reshape(-1, wavs.shape[-1]).to(dev), wavs.dim() == 1


def trim_silence(wavs, lens=None, top_db=60, frame_length=440, hop_length=220, device="cuda:0"):
    """`librosa.effects.trim(y, top_db, frame_length, hop_length)` (zero centre padding) of every row on the GPU (jv_trim_bounds,
    jv_level_apply): wavs [n] or [B, n], lens ([B] sample counts) or None -> (out, out_lens int32 [B] on the device); recording b
    is out[b, :out_lens[b]], exact zeros behind.  Nothing comes back to the host."""
    eng, w, single = _level_rows("trim_silence", wavs, lens, device)
    start, end = eng.trim_bounds(w, lens, top_db, frame_length, hop_length)
    out, out_lens = eng.level_apply(w, lens, start, end)
    return (out[0] if single else out), out_lens


def loudness(wavs, sample_rate, lens=None, device="cuda:0"):
    """integrated loudness after ITU-R BS.1770-4, mono, on the GPU (jv_loudness): wavs [n] or [B, n] -> [B] LUFS on the device
    (-inf for fewer than 400 ms or nothing above -70 LUFS)"""
    eng, w, _ = _level_rows("loudness", wavs, lens, device)
    return eng.loudness(w, sample_rate, lens)


def normalize_loudness(wavs, sample_rate, target=-23.0, peak=None, lens=None, device="cuda:0"):
    """bring every row to `target` LUFS, the gain limited so that no sample exceeds `peak` (None: no limit); a row without a
    loudness (-inf) or all zeros keeps gain 1 -> (out like wavs, lufs [B] as measured, gain [B] as applied), all on the device"""
    eng, w, single = _level_rows("normalize_loudness", wavs, lens, device)
    lufs = eng.loudness(w, sample_rate, lens)
    pk = eng.peak(w, lens) if peak is not None else None
    gain = eng.level_gain(lufs, pk, target, peak)
    out, _ = eng.level_apply(w, lens, gain=gain)
    return (out[0] if single else out), lufs, gain


def condition_prompt(speeches, sample_rates=None, top_db=60, peak=0.8, tail_seconds=0.2, device="cuda:0"):
    """what the CosyVoice2 front-ends do to a reference recording before any feature is taken: energy trim (`top_db` below the
    loudest frame, frame 440, hop 220 samples at whatever rate), scale down to a peak of `peak` (never up), append
    `tail_seconds` of silence.  Either of top_db / peak may be None to skip that part.

    speeches: a list of [n_b] / [1, n_b] recordings with sample_rates (one int per recording, or one int for all; None: one
    rate, tail at 24 kHz) -> (list of rows, lens int32 [B] on the device): row b holds the conditioned recording in
    [:lens[b]] and exact zeros behind.  A [B, n] tensor comes back as one padded batch [B, n + tail].  Grouped by rate, five
    launches' worth of calls per rate, nothing comes back to the host: rows and lens go to `extract_speech_feat_batch`,
    `extract_spk_feat_batch` and `extract_token_feat_batch` as (speeches, sample_rates, lengths=lens)."""
    who = "condition_prompt"
    batch = isinstance(speeches, torch.Tensor) and speeches.dim() == 2
    wavs = [torch.as_tensor(s).reshape(-1).to(torch.float32) for s in speeches]
    if not wavs:
        raise ValueError(f"{who}: no recordings")
    if sample_rates is None or isinstance(sample_rates, int):
        rates = [24000 if sample_rates is None else sample_rates] * len(wavs)
    else:
        rates = [int(r) for r in sample_rates]
    if len(rates) != len(wavs):
        raise ValueError(f"{who}: {len(wavs)} recordings, {len(rates)} sample rates")
    if any(r < 1 for r in rates):
        raise ValueError(f"{who}: sample rates must be positive, got {rates}")
    if not (isinstance(tail_seconds, (int, float)) and 0 <= tail_seconds < float("inf")):
        raise ValueError(f"{who}: tail_seconds must be >= 0 and finite, got {tail_seconds!r}")
    if peak is not None and not (isinstance(peak, (int, float)) and 0 < peak < float("inf")):
        raise ValueError(f"{who}: peak must be positive and finite (or None), got {peak!r}")
    if top_db is not None and not (isinstance(top_db, (int, float)) and 0 < top_db < float("inf")):
        raise ValueError(f"{who}: top_db must be positive and finite (or None), got {top_db!r}")
    dev = wavs[0].device if wavs[0].is_cuda else torch.device(device)
    eng = get_runtime(dev).ensure(1, 64, 1)
    groups = {}
    for b, r in enumerate(rates):
        groups.setdefault(r, []).append(b)
    rows = [None] * len(wavs)
    lens_out = torch.zeros(len(wavs), dtype=torch.int32, device=dev)
    for r, members in groups.items():
        buf, lens = _pad_rows([wavs[b] for b in members])
        buf = buf.to(dev)
        start, end = eng.trim_bounds(buf, lens, top_db) if top_db is not None else (None, None)
        gain = eng.level_gain(None, eng.peak(buf, lens, start, end), ceiling=peak) if peak is not None else None
        out, out_lens = eng.level_apply(buf, lens, start, end, gain, int(round(tail_seconds * r)))
        lens_out[torch.tensor(members, device=dev)] = out_lens
        for i, b in enumerate(members):
            rows[b] = out[i]
    return (torch.stack(rows) if batch else rows), lens_out


_PCM, _FLOAT, _EXTENSIBLE = 1, 3, 0xFFFE


def load_wav(path):
    """RIFF/WAVE file -> (wav [1, n] float32 in [-1, 1), sample_rate): the `torchaudio.load` of infer.py:368.  Format tags 1 (PCM:
    8-bit unsigned, 16 / 24 / 32-bit signed, scaled by 2^-(bits - 1)), 3 (float32 / float64) and 0xFFFE (extensible: the sub-format
    is the first two bytes of its GUID); chunks other than `fmt ` and `data` are skipped, pad byte included; a data size of 0 or
    0xFFFFFFFF (a streamed file) reads to the end of the file.

    Several channels are AVERAGED to one.  `torchaudio.load` keeps them as [channels, n], which the reference then passes on as
    if the channels were a batch (infer.py:371-392 index row 0 in some places and all rows in others); a mono prompt is what that
    path means."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    pos, fmt, pcm = 12, None, None
    while pos + 8 <= len(data) and pcm is None:
        tag, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = pos + 8
        if tag == b"fmt ":
            if size < 16 or body + 16 > len(data):
                raise ValueError(f"{path}: truncated fmt chunk")
            code, channels, rate, _, align, bits = struct.unpack("<HHIIHH", data[body:body + 16])
            if code == _EXTENSIBLE:
                if size < 40 or body + 26 > len(data):
                    raise ValueError(f"{path}: extensible format without its sub-format")
                code = struct.unpack("<H", data[body + 24:body + 26])[0]
            fmt = (code, channels, rate, bits)
        elif tag == b"data":
            if fmt is None:
                raise ValueError(f"{path}: data chunk before the fmt chunk")
            pcm = data[body:] if size in (0, 0xFFFFFFFF) else data[body:body + size]
        pos = body + size + (size & 1)
    if fmt is None or pcm is None:
        raise ValueError(f"{path}: no {'fmt' if fmt is None else 'data'} chunk")
    code, channels, rate, bits = fmt
    if channels < 1 or rate < 1:
        raise ValueError(f"{path}: {channels} channels at {rate} Hz")
    if code == _PCM and bits in (8, 16, 24, 32):
        width = bits // 8
        raw = np.frombuffer(pcm, dtype=np.uint8, count=len(pcm) // width * width)
        if bits == 8:
            x = (raw.astype(np.float64) - 128.0) / 128.0
        elif bits == 24:
            b3 = raw.reshape(-1, 3).astype(np.int32)
            x = (((b3[:, 0] | (b3[:, 1] << 8) | (b3[:, 2] << 16)) ^ 0x800000) - 0x800000).astype(np.float64) / float(1 << 23)
        else:
            x = raw.view("<i2" if bits == 16 else "<i4").astype(np.float64) / float(1 << (bits - 1))
    elif code == _FLOAT and bits in (32, 64):
        width = bits // 8
        x = np.frombuffer(pcm, dtype="<f4" if bits == 32 else "<f8", count=len(pcm) // width).astype(np.float64)
    else:
        raise ValueError(f"{path}: format tag {code} with {bits} bits per sample is not supported (PCM 8/16/24/32, float 32/64)")
    x = x[: x.size // channels * channels].reshape(-1, channels).mean(axis=1)
    return torch.from_numpy(x.astype(np.float32)).unsqueeze(0), int(rate)


# ---- infer.py:98-163: what the two ONNX sessions consume, from the 16 kHz copy ---------------------------------------------------
_FBANK = dict(num_mel_bins=80, dither=0, sample_frequency=16000)
_LOGMEL = dict(n_mels=128, padding=0)


def whisper_filters() -> torch.Tensor:
    """the [128, 201] filterbank of whisper.log_mel_spectrogram(n_mels=128): whisper ships it as data computed by
    librosa.filters.mel(sr=16000, n_fft=400, n_mels=128); taken from whisper when importable, else the same construction"""
    try:
        from whisper.audio import mel_filters
        return mel_filters("cpu", 128).to(torch.float32).contiguous()
    except ImportError:
        return torch.from_numpy(np.ascontiguousarray(slaney_mel_basis(16000, 400, 128, 0.0, 8000.0), dtype=np.float32))


def _engine16k(dev):
    eng = get_runtime(dev).ensure(1, 64, 1)
    if not getattr(eng, "whisper_filters_loaded", False):      # (on the context's own object, as in `_engine`)
        eng.load_whisper_filters(whisper_filters())
        eng.whisper_filters_loaded = True
    return eng


def _rows16k(who, x):
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x))
    if x.dim() not in (1, 2):
        raise ValueError(f"{who}: expected [n] or [B, n], got {tuple(x.shape)}")
    return x.to(torch.float32), x.dim() == 1


def fbank(waveform, num_mel_bins=80, dither=0, sample_frequency=16000, device="cuda:0", **kw):
    """`torchaudio.compliance.kaldi.fbank(waveform, num_mel_bins=80, dither=0, sample_frequency=16000)` on the GPU (jv_fbank):
    waveform [1, n] (or [B, n]: every row a recording of n samples) in [-1, 1] -> [T, 80] (or [B, T, 80]), T = 1 + (n - 400) // 160,
    no mean subtracted.  n < 400 gives [0, 80], as the reference does.  Only this parameter set is built."""
    got = dict(num_mel_bins=num_mel_bins, dither=dither, sample_frequency=sample_frequency)
    if got != _FBANK or kw:
        raise NotImplementedError(f"libjyutvoice_hip computes the fbank of infer.py:148-163 only ({_FBANK}, every other parameter at "
                                  f"its default); got {dict(got, **kw)}")
    w, single = _rows16k("fbank", waveform)
    if single:
        w = w.unsqueeze(0)
    dev = w.device if w.is_cuda else torch.device(device)
    if w.shape[1] < 400:
        out = torch.zeros(w.shape[0], 0, 80, device=dev)
    else:
        out = _engine16k(dev).fbank(w, subtract_mean=False)
    return out[0] if out.shape[0] == 1 else out


def log_mel_spectrogram(audio, n_mels=128, padding=0, device="cuda:0", **kw):
    """`whisper.log_mel_spectrogram(audio, n_mels=128)` on the GPU (jv_whisper_log_mel): audio [n] -> [128, n // 160], [B, n] ->
    [B, 128, n // 160] with the max - 8 clamp per row.  ValueError for n <= 200, where the reference's reflect pad raises.  Only
    this parameter set is built."""
    got = dict(n_mels=n_mels, padding=padding)
    if got != _LOGMEL or kw:
        raise NotImplementedError(f"libjyutvoice_hip computes the log-mel of infer.py:98-145 only ({_LOGMEL}); got {dict(got, **kw)}")
    w, single = _rows16k("log_mel_spectrogram", audio)
    if w.shape[-1] <= 200:
        raise ValueError(f"log_mel_spectrogram: {w.shape[-1]} samples; the reflect padding needs more than 200")
    dev = w.device if w.is_cuda else torch.device(device)
    out = _engine16k(dev).whisper_log_mel(w.unsqueeze(0) if single else w)
    return out[0] if single else out


def extract_spk_feat(speech, device="cuda:0"):
    """infer.py:150-151: speech [1, n] at 16 kHz -> fbank minus its mean over frames, [T, 80]"""
    w, single = _rows16k("extract_spk_feat", speech)
    w = w.reshape(1, -1)
    dev = w.device if w.is_cuda else torch.device(device)
    if w.shape[1] < 400:      # no frame: the reference returns an empty feature here too
        return torch.zeros(0, 80, device=dev)
    return _engine16k(dev).fbank(w, subtract_mean=True)[0]


def _to16k_batch(who, speeches, sample_rates, dev, min_len, lengths=None):
    """recordings at rates of their own -> ([B, n] at 16 kHz on the device, lens int32 [B] on the device); grouped by rate, one
    ragged `jv_resample` per rate, nothing comes back to the host (as `_extract_resampled` does for 24 kHz)"""
    wavs = [torch.as_tensor(s).reshape(-1).to(torch.float32) for s in speeches]
    if not wavs:
        raise ValueError(f"{who}: no recordings")
    rates = [16000] * len(wavs) if sample_rates is None else [int(r) for r in sample_rates]
    if len(rates) != len(wavs):
        raise ValueError(f"{who}: {len(wavs)} recordings, {len(rates)} sample rates")
    lengths = _device_lengths(who, lengths, len(wavs), dev)
    for b, (w, r) in enumerate(zip(wavs, rates)):      # the lengths are on the host here: refuse what the reference would
        if lengths is None and min_len and resample_length(w.numel(), r, 16000) < min_len:
            raise ValueError(f"{who}: recording {b}: {w.numel()} samples at {r} Hz are fewer than {min_len} at 16 kHz")
    eng = _engine16k(dev)
    if all(r == 16000 for r in rates):
        buf, lens = _rows_of(wavs, range(len(wavs)), lengths)
        return eng, buf.to(dev), lens.to(dev)
    groups = {}
    for b, r in enumerate(rates):
        groups.setdefault(r, []).append(b)
    done = []
    for r, members in groups.items():
        buf, lens = _rows_of(wavs, members, lengths)
        out, out_lens = eng.resample(buf, r, 16000, lens)
        done.append((torch.tensor(members, device=out.device), out, out_lens))
    wav16 = torch.zeros(len(wavs), max(out.shape[1] for _, out, _ in done), device=done[0][1].device)
    lens16 = torch.zeros(len(wavs), dtype=torch.int32, device=wav16.device)
    for idx, out, out_lens in done:
        wav16[idx, : out.shape[1]] = out
        lens16[idx] = out_lens
    return eng, wav16, lens16


def extract_spk_feat_batch(speeches, sample_rates=None, device="cuda:0", lengths=None):
    """`extract_spk_feat` of several recordings in one GPU pass: -> (spk_feat [B, Tmax, 80], exact zeros behind each recording's
    frames, lens int32 [B]).  sample_rates (one int per recording; None: all 16 kHz): grouped by rate and resampled to 16 kHz
    on the GPU; recording b's rows are those of `extract_spk_feat(resample(speeches[b], sample_rates[b], 16000))`, bit for bit.
    A recording of fewer than 400 samples at 16 kHz has no frame: a zero row and length 0, as the reference's empty feature.
    lengths: as in `extract_speech_feat_batch`."""
    eng, wav16, lens16 = _to16k_batch("extract_spk_feat_batch", speeches, sample_rates, torch.device(device), 0, lengths)
    return eng.fbank(wav16, lens16, subtract_mean=True)


def extract_token_feat_batch(speeches, sample_rates=None, device="cuda:0", lengths=None):
    """`log_mel_spectrogram` of several recordings in one GPU pass: -> (feat [B, 128, Tmax], zeros behind, lens int32 [B]); the
    max - 8 clamp is each recording's own.  sample_rates as in `extract_spk_feat_batch`; lengths as in `extract_speech_feat_batch`
    (with them a recording too short for the reflect padding is not refused here: it gets a zero row and length 0)."""
    eng, wav16, lens16 = _to16k_batch("extract_token_feat_batch", speeches, sample_rates, torch.device(device), 201, lengths)
    return eng.whisper_log_mel(wav16, lens16)


def extract_spk_embedding(spk_model, speech, device="cuda:0"):
    """infer.py:148-163 with the feature on the GPU.  spk_model: anything with .run() and .get_inputs() (an onnxruntime session of
    campplus.onnx in the reference; onnxruntime is not imported here) -> embedding [1, D]"""
    spk_feat = extract_spk_feat(speech, device)
    embedding = spk_model.run(None, {spk_model.get_inputs()[0].name: spk_feat.unsqueeze(dim=0).cpu().numpy()})[0].flatten().tolist()
    return torch.tensor([embedding])


def extract_speech_token(audio, speech_tokenizer_session, device="cuda:0"):
    """infer.py:98-145 with the feature on the GPU.  audio: [n] at 16 kHz (tensor or ndarray); the session is anything with .run()
    and .get_inputs() -> (speech_token int32 [1, K], speech_token_len int32 [1])"""
    if not isinstance(audio, (torch.Tensor, np.ndarray)):
        raise ValueError("Audio must be torch.Tensor or numpy.ndarray")
    feat = log_mel_spectrogram(torch.as_tensor(audio).float().reshape(1, -1), n_mels=128, device=device)
    inputs = speech_tokenizer_session.get_inputs()
    token = speech_tokenizer_session.run(None, {inputs[0].name: feat.detach().cpu().numpy(),
                                                inputs[1].name: np.array([feat.shape[2]], dtype=np.int32)})[0].flatten().tolist()
    speech_token = torch.tensor([token], dtype=torch.int32)
    return speech_token, torch.tensor([len(speech_token[0])], dtype=torch.int32)
