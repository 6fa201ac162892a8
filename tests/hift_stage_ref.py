"""One plain reference per stage of the vocoder's decode outside its ResBlock kernels (hift.hip hift_decode, hiftops.hip), shared by
test_gpu_hift_stages.py (the stages of jv_hift_decode_tap against them) and test_hift_stage_refs_host.py (the references against
oracle.hift.decode, and what mistakes they catch).  A plain module, not a conftest.

Plain torch in `dtype`: fp64 is the reference, fp32 on the CPU the floor.  Every function maps the PREVIOUS stage's tensors of ONE
utterance, cut to its own length ([1, C, positions], channels first), to its stage; `mut` is one deliberate mistake.  The
weight-free stages are the formulas themselves -- a 16 x 18 DFT basis on explicitly reflected, windowed frames; the inverse basis;
an overlap-add that divides by the squared-window sum of the frames that exist -- so that the fp32 floor is the same direct
formula in fp32 and not an FFT, which may simply be more accurate.  The convolutions are F.conv1d / F.conv_transpose1d with the
constants of spec.py; the ResBlocks are oracle.hift.resblock; the weights are oracle.hift.fold_weight_norm's (parity_util.hift_folded)."""
import functools
import math

import torch
import torch.nn.functional as F

from jyutvoice_amd import spec
from oracle import hift as ohift

import parity_util as pu

NFFT, HOP, NB = spec.HIFT_NFFT, spec.HIFT_HOP, spec.HIFT_NFFT // 2 + 1
LN100 = math.log(100.0)

LEVEL_TAPS = ("UP", "SI", "XS", "X")
TAPS = ("STFT", "PRE") + tuple(f"{n}{i}" for i in range(3) for n in LEVEL_TAPS) + ("POST", "FRAMES")      # execution order
# positions of a tap per mel frame, and on top of them
POSITIONS = {"STFT": (120, 1), "PRE": (1, 0), "POST": (120, 1), "FRAMES": (120, 1)}
for _i, _m in enumerate(((8, 0), (40, 0), (120, 1))):
    for _n in LEVEL_TAPS:
        POSITIONS[f"{_n}{_i}"] = _m
# what each stage reads: earlier taps, "mel" [1, 80, L] or "s" (the utterance's whole source row [1, 480 T]: what lies behind its
# length is there to be read by a wrong reflection)
SOURCES = {"STFT": ("s",), "PRE": ("mel",), "UP0": ("PRE",), "UP1": ("X0",), "UP2": ("X1",), "POST": ("X2",), "FRAMES": ("POST",),
           "WAV": ("FRAMES",)}
for _i in range(3):
    SOURCES[f"SI{_i}"] = ("STFT",)
    SOURCES[f"XS{_i}"] = (f"UP{_i}", f"SI{_i}")
    SOURCES[f"X{_i}"] = (f"XS{_i}",)


def live(tap, L):
    """positions of a tap (or of "WAV") that an utterance of L frames owns"""
    if tap == "WAV":
        return 480 * L
    mul, add = POSITIONS[tap]
    return L * mul + add if L > 0 else 0


# ---------------------------------------------------------------------------------------------------------------------------------
# cases: name -> (seed, T, lengths).  mel = randn, s = tanh(0.05 randn): the quiet recipe of parity_util
CASES = {
    "t1": (901, 1, (1,)),               # both neighbours of every polyphase tap are gap rows; the reflections fold inside 480 samples
    "t2": (902, 2, (2,)),
    "t3": (903, 3, (3,)),
    "ragged7": (907, 7, (7, 1, 4)),     # compact geometry: 28 mel-level rows against 37
    "empty5": (905, 5, (5, 0, 3)),      # a dead utterance between live ones: 24 against 31
    "tiles33": (933, 33, (33, 20)),     # utterance ends inside and across the convolutions' tiles at the last level: 65 against 78
    "mags": (977, 7, (7, 7, 7)),        # mel of the three utterances scaled by MAG_SCALES
    "clamp": (955, 5, (5, 3)),          # conv_post.bias[:9] + CLAMP_BIAS: log-magnitudes above ln 100
}
MAG_SCALES = (1.0, 1.4, 0.003)
CLAMP_BIAS = 4.0
COMPACT_CASES = ("ragged7", "empty5", "tiles33", "clamp")      # where hift_decode's 8 % rule takes the compact geometry


def compact_rows(T, lens):
    """(compact, uniform) mel-level rows of a batch, as hift_decode counts them (guard 4, gap 4; compact when <= 92 %)"""
    return 4 + sum(min(max(n, 0), T) + 4 for n in lens), 4 + len(lens) * (T + 4)


def inputs(name):
    seed, T, lens = CASES[name]
    g = torch.Generator().manual_seed(seed)
    mel = torch.randn(len(lens), 80, T, generator=g)
    s = torch.tanh(torch.randn(len(lens), 1, 480 * T, generator=g) * 0.05)
    if name == "mags":
        mel = mel * torch.tensor(MAG_SCALES)[:, None, None]
    return mel, s, lens


@functools.lru_cache(maxsize=None)
def checkpoint(name):
    """the state dict a case runs on: synth.hift_state_dict(), for "clamp" a copy with a constant on the log-magnitude biases"""
    from jyutvoice_amd import synth
    sd = synth.hift_state_dict()
    if name == "clamp":
        sd = {k: v.clone() for k, v in sd.items()}
        sd["conv_post.bias"][:NB] += CLAMP_BIAS
    return sd


@functools.lru_cache(maxsize=None)
def weights(name):
    """{dtype: folded weights} of a case's checkpoint"""
    w32, w64 = pu.hift_folded(checkpoint(name))
    return {torch.float32: w32, torch.float64: w64}


# ---------------------------------------------------------------------------------------------------------------------------------
# the weight-free stages
def window(dtype, mut=None):
    """periodic Hann, scipy get_window("hann", 16, fftbins=True): 0.5 - 0.5 cos(2 pi n / 16), rounded to fp32 -- the model keeps
    its window as an fp32 buffer (generator.py, oracle.hift._window), so those sixteen values are the operation's, in any dtype"""
    n = torch.arange(NFFT, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(2 * math.pi * n / (NFFT - 1 if mut == "hann_symmetric" else NFFT))).float().to(dtype)


def _angles():
    k, f = torch.arange(NFFT)[:, None], torch.arange(NB)[None, :]
    return 2 * math.pi * ((k * f) % NFFT).double() / NFFT      # [16 samples, 9 bins]


def stft(s_row, L, dtype, mut=None):
    """s_row [1, 480 T], the utterance's first L frames -> [1, 18, 120 L + 1] = 9 real | 9 imaginary.  torch.stft(16, hop 4,
    center, reflect): frame tau holds samples 4 tau - 8 + k, mirrored about sample 0 and about the utterance's own LAST sample"""
    s = s_row.to(dtype)[0]
    nvalid = s.shape[0] if mut == "stft_reflect_T" else 480 * L
    i = (4 * torch.arange(120 * L + 1)[:, None] - NFFT // 2 + torch.arange(NFFT)[None, :]).abs()
    mirrored = (2 * nvalid - i).clamp(max=nvalid - 1) if mut == "reflect_nvalid" else 2 * (nvalid - 1) - i
    i = torch.where(i >= nvalid, mirrored, i)
    x = s[i] * window(dtype, mut)      # [frames, 16]
    a = _angles()
    basis = torch.cat([torch.cos(a), torch.sin(a) if mut == "imag_sign" else -torch.sin(a)], dim=1).to(dtype)
    return (x @ basis).T[None]


def frames(post, dtype, mut=None):
    """conv_post's rows [1, 18, n] = 9 log-magnitudes | 9 phases -> the windowed inverse-DFT frames [1, 16, n]:
    x[k] = (1/16) (Re X0 + (-1)^k Re X8 + 2 sum_{f = 1..7} (Re Xf cos(2 pi f k / 16) - Im Xf sin(2 pi f k / 16))) hann[k]"""
    p = post.to(dtype)[0]
    mag = torch.exp(p[:NB])
    if mut != "no_clamp":
        mag = mag.clamp(max=100.0)
    ph = p[NB:] if mut == "no_sin" else torch.sin(p[NB:])
    re, im = mag * torch.cos(ph), mag * torch.sin(ph)
    coef = torch.tensor([1.0] + [2.0] * (NB - 2) + [2.0 if mut == "bin8_doubled" else 1.0], dtype=torch.float64) / NFFT
    a = _angles()
    x = (torch.cos(a) * coef).to(dtype) @ re - (torch.sin(a) * coef).to(dtype) @ im
    return (x * window(dtype)[:, None])[None]


def ola(fr, dtype, mut=None, clip=True):
    """frames [1, 16, n] -> [1, 4 (n - 1)]: overlap-add at hop 4, divided by the squared-window sum of the frames that exist (at
    both ends fewer than four), the centre padding of 8 samples cut from both ends, clipped to +-0.99"""
    f = fr.to(dtype)[0]
    n = f.shape[1]
    # the envelope is the MODEL's: torch.istft squares its fp32 window buffer and sums the frames' shares in fp32, in time order
    # (k descending), whatever the frames' dtype
    w2 = window(torch.float32) ** 2
    num, den = torch.zeros(4 * n + 12, dtype=dtype), torch.zeros(4 * n + 12, dtype=torch.float32)
    for k in reversed(range(NFFT)):
        num[k:k + 4 * n:4] += f[k]
        den[k:k + 4 * n:4] += w2[k]
    den = den.to(dtype)
    if mut == "envelope_const":
        den = torch.full_like(den, 1.5)
    v = (num / den)[NFFT // 2:NFFT // 2 + 4 * (n - 1)]
    if clip:
        lim = 1.0 if mut == "clip_1" else spec.HIFT_AUDIO_LIMIT
        v = v.clamp(-lim, lim)
    return v[None]


# ---------------------------------------------------------------------------------------------------------------------------------
# the convolution stages
def conv_pre(w, mel):
    return F.conv1d(mel, w["conv_pre.weight"], w["conv_pre.bias"], padding=3)


def up(w, i, x, mut=None):
    """leaky_relu(0.1) -> ConvTranspose1d(stride u, padding (k - u) // 2); behind the last one ReflectionPad1d((1, 0))"""
    u, k = spec.HIFT_UP_RATES[i], spec.HIFT_UP_KERNELS[i]
    W = w[f"ups.{i}.weight"]
    if mut == "polyphase_off":
        W = torch.roll(W, 1, dims=2)
    pad = (k - u) // 2 + (1 if mut == "up_pad_plus1" else 0)
    y = F.conv_transpose1d(F.leaky_relu(x, spec.HIFT_LRELU_SLOPE), W, w[f"ups.{i}.bias"], stride=u, padding=pad)
    if mut == "up_pad_plus1":
        y = F.pad(y, (0, 2))
    if i == 2:
        if mut == "reflect_tau1":
            y = F.pad(y, (1, 0), mode="replicate")
        elif mut == "reflect_missing":
            y = F.pad(y, (1, 0))
        else:
            y = F.pad(y, (1, 0), mode="reflect")
    return y


def source_down(w, i, st, mut=None):
    k, stride, pad = spec.HIFT_SRC_DOWNS[i]
    if mut == "sd0_pad8" and i == 0:
        pad = 8
    if mut == "sd1_pad0" and i == 1:
        pad = 0
    y = F.conv1d(st, w[f"source_downs.{i}.weight"], w[f"source_downs.{i}.bias"], stride=stride, padding=pad)
    want = (st.shape[2] - 1) // 120 * (8, 40, 120)[i] + (1 if i == 2 else 0)
    return F.pad(y, (0, want - y.shape[2]))


def xs(w, i, x_up, si):
    return x_up + ohift.resblock(w, f"source_resblocks.{i}.", si, spec.HIFT_SRC_RB_KERNELS[i])


def mrf(w, i, x, mut=None):
    out = sum(ohift.resblock(w, f"resblocks.{3 * i + j}.", x, rk) for j, rk in enumerate(spec.HIFT_RB_KERNELS))
    return out if mut == "mrf_no_div" else out / 3


def conv_post(w, x, mut=None):
    x = F.leaky_relu(x, spec.HIFT_LRELU_SLOPE if mut == "post_lrelu_01" else 0.01)
    return F.conv1d(x, w["conv_post.weight"], w["conv_post.bias"], padding=3)


def evaluate(tap, ws, src, L, dtype, mut=None):
    """stage `tap` (a name of TAPS, or "WAV") of one utterance of L frames from src = {name: tensor} (SOURCES[tap], any dtype),
    in `dtype`; ws = weights(case)"""
    w = ws[dtype]
    g = lambda n: src[n].to(dtype)
    with torch.inference_mode():
        if tap == "STFT":
            return stft(src["s"], L, dtype, mut)
        if tap == "PRE":
            return conv_pre(w, g("mel"))
        if tap == "POST":
            return conv_post(w, g("X2"), mut)
        if tap == "FRAMES":
            return frames(src["POST"], dtype, mut)
        if tap == "WAV":
            return ola(src["FRAMES"], dtype, mut)
        i = int(tap[-1])
        if tap.startswith("UP"):
            return up(w, i, g(SOURCES[tap][0]), mut)
        if tap.startswith("SI"):
            return source_down(w, i, g("STFT"), mut)
        if tap.startswith("XS"):
            return xs(w, i, g(f"UP{i}"), g(f"SI{i}"))
        return mrf(w, i, g(f"XS{i}"), mut)


def chain(ws, mel, s_row, L, dtype=torch.float64):
    """every stage of one utterance from its inputs, each fed the previous one in `dtype`: {tap: tensor}, "WAV" and "WAV_RAW" (ahead
    of the clip) included"""
    out = {"mel": mel[:, :, :L], "s": s_row}
    for tap in TAPS + ("WAV",):
        out[tap] = evaluate(tap, ws, out, L, dtype)
    out["WAV_RAW"] = ola(out["FRAMES"], dtype, clip=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_chain(name, b):
    """the fp64 chain of utterance b of a case (host test; the conditions on the cases)"""
    mel, s, lens = inputs(name)
    return chain(weights(name), mel[b:b + 1], s[b, :, :], lens[b])


def f0(ws, mel, dtype):
    with torch.inference_mode():
        return ohift.f0_predict(ws[dtype], mel.to(dtype))


# ---------------------------------------------------------------------------------------------------------------------------------
# the error measure: test_gpu_fused_ops.distances on rows = one time position's channel vector (taps) / one mel frame's 480
# samples (waveform)
def rows_of(tap, t):
    """[1, C, n] -> [n, C];  waveform [1, 480 L] -> [L, 480]"""
    return t[0].reshape(-1, 480) if tap == "WAV" else t[0].T
