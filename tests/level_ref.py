"""TEST INFRASTRUCTURE (nothing under jyutvoice_amd/ imports it; numpy only): the fp64 restatements of the level definitions of
include/jyutvoice_hip.h -- the energy trim (librosa.effects.trim's contract with zero centre padding), the sample peak, the
integrated loudness of ITU-R BS.1770-4 (mono) and the gain rules -- that test_level_host.py checks for itself and
test_gpu_level.py checks the kernels against, plus the signal recipes, the case lists and the bound of the GPU test, so that the host
test can assert the conditions on the inputs without a GPU.

The loudness bound.  `lufs32_seq` is the same meter with the K-weighting as a sequential direct-form recurrence in fp32 with
fp32-rounded coefficients (block means in fp64): its distance from `lufs64` is the FLOOR, what single precision costs a plain
implementation.  The kernel must stay within MARGIN = 8 floors (the largest floor over the cases of a rate), the margin this project
gives a different summation order; the floor is measured by `lufs32_seq`, never by the kernel."""
import functools
import math

import numpy as np

MARGIN = 8.0
RATES = (16000, 22050, 24000, 48000)
SEEDS = (100, 101, 102, 103)
LEVELS = ((0.1, 7.3), (0.004, 5.1), (1e-5, 6.7), (0.05, 4.9))      # (sigma, length in units of h) of the four-level signal
TABLE_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)
ABS_GATE, OFFSET = -70.0, -0.691

# the kernel's own seams (level.hip: LV_SEG samples per lane, 64 lanes per wave, 4 waves per workgroup)
SEG, WAVE_SPAN, GROUP_SPAN = 32, 2048, 8192

TRIM_F, TRIM_H, TRIM_DB = 440, 220, 60.0
TRIM_LEADS = range(1000, 1221)      # lead l, tail l - 100: every residue modulo TRIM_H for both
TRIM_CHUNK = 37                     # recordings per ragged call (6 calls)


def hop(fs):
    return (fs + 5) // 10


def blocks(n, fs):
    h = hop(fs)
    return 0 if n < 4 * h else (n - 4 * h) // h + 1


def kweight(fs):
    """[shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2] in fp64"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    return np.array(shelf + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])


def biquad(x, c, dtype=np.float64):
    """direct form I, zero state, sequential, every operation rounded to `dtype`"""
    b0, b1, b2, a1, a2 = (dtype(v) for v in c)
    y = np.empty(len(x), dtype=dtype)
    x1 = x2 = y1 = y2 = dtype(0)
    for i, xi in enumerate(np.asarray(x, dtype=dtype)):
        yi = b0 * xi + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1, y2, y1 = x1, xi, y1, yi
        y[i] = yi
    return y


def kfilter(x, fs, dtype=np.float64, coeff_fs=None):
    c = kweight(coeff_fs or fs)
    return biquad(biquad(x, c[:5], dtype), c[5:], dtype)


def gate(y, fs, rel_gate=True, overlap_hops=1, offset=OFFSET):
    """(L, z, (margin to the absolute gate, margin to the relative gate) in LU) from the K-weighted signal"""
    h, n = hop(fs), len(y)
    step = h * overlap_hops
    nb = 0 if n < 4 * h else (n - 4 * h) // step + 1
    sq = np.asarray(y, dtype=np.float64) ** 2
    z = np.array([sq[j * step: j * step + 4 * h].mean() for j in range(nb)])
    if nb == 0:
        return -math.inf, z, (math.inf, math.inf)
    with np.errstate(divide="ignore"):
        l = offset + 10.0 * np.log10(z)
    m_abs = float(np.abs(l - ABS_GATE).min())
    keep = z > 10.0 ** ((ABS_GATE - offset) / 10.0)
    if not keep.any():
        return -math.inf, z, (m_abs, math.inf)
    if not rel_gate:
        return offset + 10.0 * math.log10(z[keep].mean()), z, (m_abs, math.inf)
    gamma = offset + 10.0 * math.log10(z[keep].mean()) - 10.0
    m_rel = float(np.abs(l[keep] - gamma).min())
    both = keep & (z > 0.1 * z[keep].mean())
    return offset + 10.0 * math.log10(z[both].mean()), z, (m_abs, m_rel)


def lufs64(x, fs, **variant):
    """the definition in fp64 -> (L, z_j, gate margins).  variant: rel_gate=False, overlap_hops=2 (50 % overlap), offset=0.0,
    coeff_fs=48000 -- the mistakes test_level_host.py shows to land outside the bound"""
    coeff_fs = variant.pop("coeff_fs", None)
    return gate(kfilter(np.asarray(x, dtype=np.float64), fs, coeff_fs=coeff_fs), fs, **variant)


def lufs32_seq(x, fs):
    return gate(kfilter(x, fs, dtype=np.float32).astype(np.float64), fs)[0]


def trim64(x, top_db=TRIM_DB, F=TRIM_F, H=TRIM_H, pad="constant"):
    """(start, end, m_t / (M thr) per frame)"""
    x = np.asarray(x, dtype=np.float64)
    N = x.size
    span = N + 2 * (F // 2) - F
    if N == 0 or span < 0:
        return 0, 0, np.zeros(0)
    T = 1 + span // H
    xp = np.pad(x, F // 2, mode=pad)
    ms = np.array([np.mean(xp[t * H: t * H + F] ** 2) for t in range(T)])
    m = np.maximum(1e-10, ms)
    ratio = m / (m.max() * 10.0 ** (-top_db / 10.0))
    loud = np.nonzero(ratio > 1.0)[0]
    if loud.size == 0:
        return 0, 0, ratio
    return int(H * loud[0]), int(min(N, H * (loud[-1] + 1))), ratio


def peak(x, start=None, end=None):
    x = np.asarray(x)[slice(start, end)]
    return float(np.abs(x).max()) if x.size else 0.0


def gain64(L, pk, target=-23.0, ceiling=None):
    """L None: the prompt rule"""
    if L is None:
        return ceiling / pk if pk > ceiling else 1.0
    if L == -math.inf or pk == 0.0:
        return 1.0
    g = 10.0 ** ((target - L) / 20.0)
    return min(g, ceiling / pk) if ceiling else g


# ---- recipes -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def four_level(fs, seed):
    rng, h = np.random.default_rng(seed), hop(fs)
    return np.concatenate([s * rng.standard_normal(int(k * h)) for s, k in LEVELS]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def one_level(n, seed=7, sigma=0.05):
    return (sigma * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sine997(fs=48000, seconds=5):
    return np.sin(2.0 * math.pi * 997.0 * np.arange(fs * seconds) / fs).astype(np.float32)


def seam_lengths(fs=24000):
    """the lengths of the 'lengths and seams' case: around 4 h and 5 h, and on either side of the first segment / wave / workgroup
    seam at or behind 4 h (a shorter recording has no block)"""
    h = hop(fs)
    out = {4 * h - 1, 4 * h, 4 * h + 1, 5 * h - 1, 5 * h, 5 * h + 1}
    for span in (SEG, WAVE_SPAN, GROUP_SPAN):
        at = -(-4 * h // span) * span
        out |= {at - 1, at, at + 1}
    return sorted(out)


@functools.lru_cache(maxsize=None)
def trim_recording(lead, tail=None, seed=None):
    tail = lead - 100 if tail is None else tail
    rng = np.random.default_rng(1000 + lead if seed is None else seed)
    x = 1e-4 * rng.standard_normal(lead + 3000 + tail)
    x[lead: lead + 3000] = 0.3 * rng.standard_normal(3000)
    return x.astype(np.float32)


def trim_edge_cases():
    """name -> (x, F, H): the edges of the trim"""
    H, F = TRIM_H, TRIM_F
    rng = np.random.default_rng(11)
    noise = lambda n: (0.1 * rng.standard_normal(n)).astype(np.float32)
    spike = lambda n, i: np.where(np.arange(n) == i, np.float32(0.9), np.float32(1e-6) * rng.standard_normal(n).astype(np.float32))
    return {
        "n0": (np.zeros(0, np.float32), F, H), "n1": (noise(1), F, H), "n_h_minus_1": (noise(H - 1), F, H), "n_h": (noise(H), F, H),
        "n_5h": (noise(5 * H), F, H), "zeros": (np.zeros(3000, np.float32), F, H),
        "below_amin": (np.full(3000, 1e-6, np.float32), F, H), "spike_first": (spike(3000, 0), F, H),
        "spike_last": (spike(3000, 2999), F, H), "spike_at_hop": (spike(3000, H), F, H), "odd_frame": (trim_recording(1100), 441, H), "frame_beyond_n": (noise(300), F, H),
    }


@functools.lru_cache(maxsize=None)
def gate_case(fs, seed):
    """(x, L64, margins, floor) of a four-level case"""
    x = four_level(fs, seed)
    L, _, margins = lufs64(x, fs)
    return x, L, margins, abs(lufs32_seq(x, fs) - L)


def rate_bound(fs):
    """MARGIN x the largest floor over the rate's four-level cases"""
    return MARGIN * max(gate_case(fs, s)[3] for s in SEEDS)
