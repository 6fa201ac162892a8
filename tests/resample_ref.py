"""TEST INFRASTRUCTURE (nothing under jyutvoice_amd/ imports it): the fp64 restatement of `torchaudio.functional.resample(x, orig,
new)` with its defaults (sinc_interp_hann, lowpass_filter_width = 6, rolloff = 0.99) that test_resample_host.py checks for itself
and test_gpu_resample.py checks the kernel against -- plus the shared inputs and the derived bound of the GPU test, so that the host
test can show what that bound catches.

Unpinned: torchaudio is not part of this build, so the algorithm is restated from its published definition.
With g = gcd(orig, new), o = orig / g, n = new / g:

    base = rolloff min(o, n),  width = ceil(6 o / base),  K = 2 width + o
    h(tau) = (base / o) sinc(base tau) cos^2(pi base tau / 12) for |base tau| <= 6, else 0;  sinc(u) = sin(pi u) / (pi u)
    tab[p][k] = h((k - width) / o - p / n)
    y[i n + p] = sum_k tab[p][k] x[i o + k - width],  x = 0 outside [0, L),  for the first ceil(n L / o) samples

`table(..., mutate=...)` builds the wrong tables a slip in a restatement would give (MUTANTS)."""
import math
import struct

import numpy as np

# the GPU test's rate pairs: n < o, n > o, n = 1, o = 1, n >= 64, K > 128
PAIRS = [(48000, 24000), (24000, 48000), (16000, 24000), (24000, 16000), (24000, 8000), (44100, 24000), (24000, 44100),
         (22050, 24000)]
GEOMETRY = {(48000, 24000): (2, 1, 28), (24000, 48000): (1, 2, 15), (16000, 24000): (2, 3, 16), (24000, 16000): (3, 2, 23),
            (24000, 8000): (3, 1, 41), (44100, 24000): (147, 80, 171), (24000, 44100): (80, 147, 94), (22050, 24000): (147, 160, 161)}
STANDARD_RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000]
TABLE_CAP = 1 << 20

# a dropped base / o scale; the table's centre one tap off the indexing (width off by one); p / n added instead of subtracted;
# rolloff = 1; no Hann window
MUTANTS = ("no_scale", "width_off_by_one", "phase_sign", "rolloff_1", "rectangular")

SEAM_SAMPLES = 20011            # one recording, several tiles of output: every tile seam is inside
ENDS_B, ENDS_N = 40, 6040       # lens = 6001 .. 6040 in one call


def geometry(orig, new, rolloff=0.99):
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = rolloff * min(o, n)
    width = math.ceil(6 * o / base)
    return o, n, width, 2 * width + o, base


def out_length(L, orig, new):
    g = math.gcd(orig, new)
    return -(-(new // g) * L // (orig // g))


def table(orig, new, mutate=None):
    """tab [n, K] in fp64"""
    o, n, width, K, base = geometry(orig, new, rolloff=1.0 if mutate == "rolloff_1" else 0.99)
    centre = width + 1 if mutate == "width_off_by_one" else width
    sign = 1 if mutate == "phase_sign" else -1
    # tau over the common denominator o n: the numerator is an exact integer
    num = (np.arange(K, dtype=np.int64)[None, :] - centre) * n + sign * np.arange(n, dtype=np.int64)[:, None] * o
    u = base * (num.astype(np.float64) / float(o * n))
    pu = np.pi * u
    sinc = np.where(num == 0, 1.0, np.sin(pu) / np.where(num == 0, 1.0, pu))
    window = 1.0 if mutate == "rectangular" else np.cos(np.pi * u / 12.0) ** 2
    scale = 1.0 if mutate == "no_scale" else base / o
    return np.where(np.abs(u) <= 6.0, scale * sinc * window, 0.0)


def _frames(x, o, width, K, count):
    """X[i, k] = x[i o + k - width] with zeros outside the recording, i < count"""
    xp = np.concatenate([np.zeros(width), np.asarray(x, dtype=np.float64), np.zeros(count * o + K)])
    return np.lib.stride_tricks.as_strided(xp, shape=(count, K), strides=(o * xp.strides[0], xp.strides[0]))


def resample64(x, orig, new, tab=None):
    """the definition in fp64: x [L] -> y [ceil(n L / o)]; tab: another table in its place (a mutant, or |tab| with |x| for the bound)"""
    x = np.asarray(x, dtype=np.float64)
    if orig == new:
        return x.copy()
    o, n = geometry(orig, new)[:2]
    tab = table(orig, new) if tab is None else tab
    K = tab.shape[1]                    # (a mutant's rolloff brings a width of its own)
    width = (K - o) // 2
    L_out = out_length(x.size, orig, new)
    count = -(-L_out // n)
    if count == 0:
        return np.zeros(0)
    return (_frames(x, o, width, K, count) @ tab.T).reshape(-1)[:L_out]


def bound(x, orig, new):
    """the GPU test's bound per output sample: (K + 3) 2^-24 sum_k |tab[p][k]| |x[i o + k - width]| -- K fused multiply-adds of
    relative error 2^-24 each, the table's one rounding to fp32, and headroom.  Derived, not measured."""
    K = geometry(orig, new)[3]
    return (K + 3) * 2.0 ** -24 * resample64(np.abs(np.asarray(x, dtype=np.float64)), orig, new, tab=np.abs(table(orig, new)))


def signal(seed, n):
    """uniform(-1, 1) fp32 samples: the inputs of the GPU test (and of the host test's mutation check)"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)


def pair_seed(orig, new):
    return orig * 7 + new


# ---- RIFF/WAVE files for the reader's tests and the CLI's -------------------------------------------------------------------
def riff(fmt_body, data_body, extra_before=b"", extra_after=b"", data_size=None):
    def chunk(tag, body, size=None):
        return tag + struct.pack("<I", len(body) if size is None else size) + body + (b"\0" if len(body) & 1 else b"")
    body = b"WAVE" + chunk(b"fmt ", fmt_body) + extra_before + chunk(b"data", data_body, data_size) + extra_after
    return b"RIFF" + struct.pack("<I", len(body)) + body


def fmt16(code, channels, rate, bits):
    return struct.pack("<HHIIHH", code, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)


def fmt_ext(sub, channels, rate, bits):
    guid = struct.pack("<H", sub) + bytes.fromhex("000000001000800000aa00389b71")
    return fmt16(0xFFFE, channels, rate, bits) + struct.pack("<HHI", 22, bits, 0) + guid


def pcm_bytes(ints, bits):
    if bits == 8:
        return bytes((int(v) + 128) & 0xFF for v in ints)
    if bits == 24:
        return b"".join(struct.pack("<i", int(v))[:3] for v in ints)
    return np.asarray(ints, dtype="<i2" if bits == 16 else "<i4").tobytes()


def write_wav(path, x, rate, bits, code=1):
    """x [n] or [n, channels] in [-1, 1) -> a RIFF/WAVE file: PCM of `bits` bits (code 1; 8-bit unsigned) or float32 (code 3)"""
    x = np.asarray(x, dtype=np.float64)
    channels = 1 if x.ndim == 1 else x.shape[1]
    if code == 3:
        body = x.astype("<f4").tobytes()
    else:
        top = 1 << (bits - 1)
        body = pcm_bytes(np.clip(np.round(x.reshape(-1) * top), -top, top - 1).astype(np.int64), bits)
    with open(path, "wb") as f:
        f.write(riff(fmt16(code, channels, rate, bits), body))
