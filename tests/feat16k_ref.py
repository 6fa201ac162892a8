"""TEST INFRASTRUCTURE (nothing under jyutvoice_amd/ imports it): the fp64 restatements of the two 16 kHz reference-audio
features -- `kaldi.fbank(x, num_mel_bins=80, dither=0, sample_frequency=16000)` [minus its mean over frames] and
`whisper.log_mel_spectrogram(x, n_mels=128)` -- that test_feat16k_host.py checks for itself and test_gpu_feat16k.py checks the
kernel against, the same chains in fp32 on the CPU (the yardstick of the error model), the shared inputs, and the intervals.

Unpinned: torchaudio and whisper are not part of this build, so both are restated from their definitions (include/jyutvoice_hip.h,
DESIGN.md section 3).

Error model.  For output (f, m) with fp64 mel energy E, s = sum_k M[m, k] |X_k| A_f + E, A_f = sum_i |a_i| the L1 norm of the
conditioned frame: the first-order error scale of |X|^2.  Per case c = max over outputs of |E32 - E| / s, E32 the fp32 CPU chain
below (numpy / torch fp32, an fp32 FFT) -- never the kernel.  The kernel must satisfy |E_gpu - E| <= 8 c s per output, checked in the
log domain by interval: the stored value lies in [g(E - 8 c s), g(E + 8 c s)], g the floor-then-log, each end widened by
4 2^-24 (1 + |end|) for the device's logf.  The fbank mean over frames and the Whisper maximum are carried as intervals (the mean's
widened by (m + 2) 2^-24 mean|v| for its fp32 summation), and every fp32 operation that follows the log (fbank: the subtraction;
Whisper: the + 4) adds one rounding, 2^-24 |end|.  Condition on the inputs: at most 1 % of a case's outputs may have an interval
wider than 1e-2 (WIDE_CAP), asserted on the reference alone.

`mutate=` builds what a slip in a restatement would give (FBANK_MUTANTS, WHISPER_MUTANTS)."""
import numpy as np
import torch

import resample_ref

EPS = 2.0 ** -23          # kaldi's floor: fp32 machine epsilon
U = 2.0 ** -24            # unit roundoff of fp32
MARGIN = 8.0              # the margin test_gpu_fused_ops.py and test_gpu_vocoder_unclipped.py give an fp32 chain
WIDE, WIDE_CAP = 1e-2, 0.01

FBANK_MUTANTS = ("povey_exponent_1", "periodic_window", "no_dc_removal", "banks_shifted_one_bin", "low_freq_0", "floor_1e-10",
                 "mean_over_tmax")
# pre-emphasis with a[-1] = 0 instead of a[0] changes element 0 of a frame alone, and the symmetric Povey window is exactly 0 there:
# the slip cannot show in any output, so no interval can catch it; test_feat16k_host.py asserts that instead
FBANK_SILENT_MUTANTS = ("preemphasis_zero_pad",)
WHISPER_MUTANTS = ("symmetric_window", "natural_log", "last_frame_kept", "max_over_batch")

SEAM_SAMPLES = 20011
ENDS_B = 40
FBANK_ENDS = list(range(5981, 6021))        # the frame count steps from 35 to 36 at 6000
WHISPER_ENDS = list(range(6061, 6101))      # ... and from 37 to 38 at 6080
FBANK_SMALL = [399, 400, 559, 560]
WHISPER_SMALL = [200, 201, 319, 320]
QUIET_SAMPLES = 8000


def speech(seed, n):
    """speech-like fp32 samples: a 120 +- 30 Hz harmonic stack (29 harmonics at 1 / h) under a max(sin 2 pi 1.3 t, 0)^2 envelope, peak
    0.5, plus Gaussian noise of sigma 0.003, clipped to [-1, 1]"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / 16000.0
    f0 = 120.0 + 30.0 * np.sin(2.0 * np.pi * 0.7 * t + rng.uniform(0, 2 * np.pi))
    phase = 2.0 * np.pi * np.cumsum(f0) / 16000.0
    ph = rng.uniform(0, 2 * np.pi, 29)
    v = sum(np.sin(h * phase + ph[h - 1]) / h for h in range(1, 30))
    v *= np.maximum(np.sin(2.0 * np.pi * 1.3 * t), 0.0) ** 2
    v *= 0.5 / max(float(np.abs(v).max()), 1e-30)
    return np.clip(v + rng.normal(0.0, 0.003, n), -1.0, 1.0).astype(np.float32)


def quiet():
    return (0.01 * speech(3, QUIET_SAMPLES).astype(np.float64)).astype(np.float32)


signal = resample_ref.signal      # uniform(-1, 1)


def cases(feat):
    """name -> list of recordings (fp32 arrays): the inputs of the GPU test's interval cases.  A list is one ragged batch."""
    ends = FBANK_ENDS if feat == "fbank" else WHISPER_ENDS
    small = FBANK_SMALL if feat == "fbank" else WHISPER_SMALL
    seed = 11 if feat == "fbank" else 12
    full = signal(seed, ENDS_B * ends[-1]).reshape(ENDS_B, ends[-1])
    tiny = signal(seed + 2, len(small) * small[-1]).reshape(len(small), small[-1])
    return {
        "seams speech": [speech(1, SEAM_SAMPLES)],
        "seams uniform": [signal(2, SEAM_SAMPLES)],
        "ends": [full[b, :n] for b, n in enumerate(ends)],
        "smallest": [tiny[b, :n] for b, n in enumerate(small)],
        "quiet": [quiet()],
    }


def fbank_frames(n):
    return 0 if n < 400 else 1 + (n - 400) // 160


def whisper_frames(n):
    return 0 if n <= 200 else n // 160


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def kaldi_mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def kaldi_banks(low=20.0, shift=0):
    """[80, 257] in fp64: triangles equally spaced in mel between mel(low) and mel(8000); bin 256 has weight 0"""
    lo, hi = float(kaldi_mel(low)), float(kaldi_mel(8000.0))
    d = (hi - lo) / 81.0
    b = np.arange(80, dtype=np.float64)[:, None]
    left, centre, right = lo + b * d, lo + (b + 1) * d, lo + (b + 2) * d
    m = kaldi_mel(31.25 * (np.arange(257, dtype=np.float64) - shift))[None, :]
    w = np.maximum(0.0, np.minimum((m - left) / (centre - left), (right - m) / (right - centre)))
    if not shift:
        w[:, 256] = 0.0
    return w


def povey(exponent=0.85, periodic=False):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(400, dtype=np.float64) / (400.0 if periodic else 399.0))) ** exponent


def hann(periodic=True):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(400, dtype=np.float64) / (400.0 if periodic else 399.0))


def whisper_filters():
    """[128, 201] fp32: the data the library is handed (jyutvoice_amd.utils.audio.whisper_filters)"""
    from jyutvoice_amd.utils.audio import whisper_filters as wf
    return wf().numpy()


# ---- the chains: conditioned frames -> energies, in fp64 or fp32 ------------------------------------------------------------------
def _frames(x, m):
    return np.lib.stride_tricks.as_strided(x, shape=(m, 400), strides=(160 * x.strides[0], x.strides[0]))


def _power(a, nfft, dtype):
    """|rfft|^2 of the rows of a, zero-padded to nfft: fp64 through numpy, fp32 through torch's single-precision FFT"""
    if dtype == np.float64:
        X = np.fft.rfft(a, n=nfft, axis=1)
        return X.real ** 2 + X.imag ** 2
    X = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(a)), n=nfft, dim=1)
    return (X.real * X.real + X.imag * X.imag).numpy()


def fbank_conditioned(x, dtype=np.float64, mutate=None):
    """[m, 400] conditioned frames of one recording (steps 1-5)"""
    x = np.asarray(x, dtype=dtype)
    m = fbank_frames(x.size)
    if m == 0:
        return np.zeros((0, 400), dtype=dtype)
    a = _frames(x, m).copy()
    if mutate != "no_dc_removal":
        a = a - a.mean(axis=1, keepdims=True, dtype=dtype)
    first = np.zeros_like(a[:, :1]) if mutate == "preemphasis_zero_pad" else a[:, :1]
    a = a - dtype(0.97) * np.concatenate([first, a[:, :-1]], axis=1)
    w = povey(1.0 if mutate == "povey_exponent_1" else 0.85, periodic=mutate == "periodic_window")
    return (a * w.astype(dtype)).astype(dtype)


def fbank_energy(x, dtype=np.float64, mutate=None):
    """(E [m, 80], s [m, 80]) of one recording in `dtype` (s only means something in fp64)"""
    a = fbank_conditioned(x, dtype, mutate)
    banks = kaldi_banks(0.0 if mutate == "low_freq_0" else 20.0, 1 if mutate == "banks_shifted_one_bin" else 0)
    if a.shape[0] == 0:
        return np.zeros((0, 80), dtype=dtype), np.zeros((0, 80), dtype=dtype)
    P = _power(a, 512, dtype)
    M = banks.astype(dtype)
    E = P @ M.T
    s = (np.sqrt(P) @ M.T) * np.abs(a).sum(axis=1, keepdims=True) + E
    return E.astype(dtype), s


def whisper_conditioned(x, dtype=np.float64, mutate=None):
    """[T, 400] windowed frames of one recording (steps 1-3)"""
    x = np.asarray(x, dtype=dtype)
    T = whisper_frames(x.size)
    if T == 0:
        return np.zeros((0, 400), dtype=dtype)
    xp = np.concatenate([x[200:0:-1], x, x[-2:-202:-1]])
    keep = T + 1 if mutate == "last_frame_kept" else T
    w = hann(periodic=mutate != "symmetric_window")
    return (_frames(np.ascontiguousarray(xp), keep) * w.astype(dtype)).astype(dtype)


def whisper_energy(x, dtype=np.float64, mutate=None):
    """(E [128, T], s [128, T])"""
    a = whisper_conditioned(x, dtype, mutate)
    if a.shape[0] == 0:
        return np.zeros((128, 0), dtype=dtype), np.zeros((128, 0), dtype=dtype)
    P = _power(a, 400, dtype)
    M = whisper_filters().astype(dtype)
    E = M @ P.T
    s = (M @ np.sqrt(P).T) * np.abs(a).sum(axis=1)[None, :] + E
    return E.astype(dtype), s


# ---- the definitions' outputs in fp64 ---------------------------------------------------------------------------------------------
def fbank64(x, subtract_mean=True, mutate=None, tmax=None):
    E = fbank_energy(x, np.float64, mutate)[0]
    v = np.log(np.maximum(E, 1e-10 if mutate == "floor_1e-10" else EPS))
    if subtract_mean and v.shape[0]:
        v = v - v.sum(axis=0, keepdims=True) / (tmax if mutate == "mean_over_tmax" else v.shape[0])
    return v


def whisper64(x, mutate=None, batch_max=None):
    E = whisper_energy(x, np.float64, mutate)[0]
    L = np.log(np.maximum(E, 1e-10)) if mutate == "natural_log" else np.log10(np.maximum(E, 1e-10))
    if L.size:
        L = np.maximum(L, (batch_max if mutate == "max_over_batch" else L.max()) - 8.0)
    return (L + 4.0) / 4.0


# ---- intervals ------------------------------------------------------------------------------------------------------------------
def _wlo(v, k=4.0):
    return v - k * U * (1.0 + np.abs(v))


def _whi(v, k=4.0):
    return v + k * U * (1.0 + np.abs(v))


class Intervals:
    """of one recording: c of the case, [lo, hi] per output of the final feature, [raw_lo, raw_hi] of the log values before the
    mean (fbank), and what recovering the kernel's energy error needs"""

    def __init__(self, feat, x, c, subtract_mean=True):
        self.feat, self.c = feat, c
        E, s = (fbank_energy if feat == "fbank" else whisper_energy)(x)
        self.E, self.s = E, s
        r = MARGIN * c * s
        if feat == "fbank":
            g = lambda e: np.log(np.maximum(e, EPS))
            lo, hi = _wlo(g(E - r)), _whi(g(E + r))
            self.raw_lo, self.raw_hi = lo, hi
            if subtract_mean and E.shape[0]:
                m, v = E.shape[0], g(E)
                w = (m + 2) * U * np.abs(v).mean(axis=0, keepdims=True)
                mean_lo, mean_hi = lo.mean(axis=0, keepdims=True) - w, hi.mean(axis=0, keepdims=True) + w
                lo, hi = lo - mean_hi, hi - mean_lo
                lo, hi = lo - U * np.abs(lo), hi + U * np.abs(hi)
        else:
            g = lambda e: np.log10(np.maximum(e, 1e-10))
            lo, hi = _wlo(g(E - r)), _whi(g(E + r))
            self.raw_lo, self.raw_hi = lo, hi
            if E.size:
                lo, hi = np.maximum(lo, lo.max() - 8.0), np.maximum(hi, hi.max() - 8.0)
                lo, hi = lo + 4.0, hi + 4.0
                lo, hi = (lo - U * np.abs(lo)) / 4.0, (hi + U * np.abs(hi)) / 4.0
        self.lo, self.hi = lo, hi

    def wide_share(self):
        return float(((self.hi - self.lo) > WIDE).mean()) if self.lo.size else 0.0

    def outside(self, got):
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == self.lo.shape, (got.shape, self.lo.shape)
        return (got < self.lo) | (got > self.hi)

    def energy_ratio(self, got):
        """max |E_gpu - E| / s over the outputs off the floors, E_gpu recovered through the inverse of g.  `got` is the raw fbank
        log (subtract_mean = 0) or the normalised Whisper value; 0.0 when nothing is off the floors"""
        got = np.asarray(got, dtype=np.float64)
        if got.size == 0:
            return 0.0
        if self.feat == "fbank":
            off = self.E > 4.0 * EPS
            Eg = np.exp(got)
        else:
            L = 4.0 * got - 4.0
            off = (self.E > 4e-10) & (L > L.max() - 7.99)
            Eg = 10.0 ** L
        if not off.any():
            return 0.0
        return float((np.abs(Eg - self.E)[off] / self.s[off]).max())


def case_c(feat, recordings):
    """c of a case: max over its recordings' outputs of |E32 - E| / s, E32 the fp32 CPU chain"""
    fn = fbank_energy if feat == "fbank" else whisper_energy
    c = 0.0
    for x in recordings:
        E, s = fn(x)
        if E.size:
            E32 = fn(x, np.float32)[0].astype(np.float64)
            c = max(c, float((np.abs(E32 - E) / s).max()))
    return c


_cache = {}


def case_intervals(feat, name, subtract_mean=True):
    """(c, [Intervals per recording]) of a case of `cases(feat)`; computed once and shared"""
    key = (feat, name, subtract_mean)
    if key not in _cache:
        recs = cases(feat)[name]
        c = case_c(feat, recs)
        _cache[key] = (c, [Intervals(feat, x, c, subtract_mean) for x in recs])
    return _cache[key]


def case_wide_share(feat, name):
    ivs = case_intervals(feat, name)[1]
    n = sum(iv.lo.size for iv in ivs)
    return sum(float(((iv.hi - iv.lo) > WIDE).sum()) for iv in ivs) / max(n, 1)
