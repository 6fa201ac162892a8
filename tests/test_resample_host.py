"""CPU: the host half of the resampler (jv_resample_table, jv_resample_length, the 2^20-entry cap: no device needed), the fp64
restatement the GPU test trusts (tests/resample_ref.py) checked for itself, and the WAV reader."""
import ctypes as C
import itertools
import math
import os
import struct

import numpy as np
import pytest
import torch

import resample_ref as ref

EXTRA_PAIRS = [(11025, 32000)]      # the largest table of the standard rates: n K = 1280 x 455


@pytest.fixture(scope="module")
def lib():
    from jyutvoice_amd import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from jyutvoice_amd import _lib
    return _lib.load()


def lib_table(lib, orig, new):
    o, n, w = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.jv_resample_table(orig, new, None, 0, C.byref(o), C.byref(n), C.byref(w)) == 0
    K = 2 * w.value + o.value
    tab = np.zeros((n.value, K), dtype=np.float32)
    assert lib.jv_resample_table(orig, new, tab.ctypes.data, tab.size, None, None, None) == 0
    return tab, (o.value, n.value, w.value, K)


# ---- the library's table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", ref.PAIRS + EXTRA_PAIRS)
def test_table_matches_fp64_formula(lib, orig, new):
    """o, n, width exact; every entry within 2^-23 max |tab| of the fp64 formula (one rounding to fp32 is 2^-24 relative; a libm
    sin may differ from numpy's in the last fp64 bit before it)"""
    tab, geo = lib_table(lib, orig, new)
    o, n, width, K, _ = ref.geometry(orig, new)
    assert geo == (o, n, width, K)
    if (orig, new) in ref.GEOMETRY:
        assert (o, n, K) == ref.GEOMETRY[(orig, new)]
    want = ref.table(orig, new)
    assert tab.shape == want.shape
    err = float(np.abs(tab.astype(np.float64) - want).max())
    assert err <= 2.0 ** -23 * float(np.abs(want).max()), err


def test_table_geometry_examples(lib):
    assert lib_table(lib, 44100, 24000)[1] == (147, 80, 12, 171)
    assert lib_table(lib, 11025, 32000)[1][1] * lib_table(lib, 11025, 32000)[1][3] == 1280 * 455 == 582400


def test_equal_reduced_ratios_share_a_table(lib):
    a, ga = lib_table(lib, 48000, 24000)
    b, gb = lib_table(lib, 32000, 16000)
    assert ga == gb and np.array_equal(a, b)
    a, ga = lib_table(lib, 44100, 24000)
    b, gb = lib_table(lib, 88200, 48000)
    assert ga == gb and np.array_equal(a, b)


def test_table_capacity_and_bad_rates(lib):
    small = np.zeros(10, dtype=np.float32)
    assert lib.jv_resample_table(48000, 24000, small.ctypes.data, small.size, None, None, None) == 4      # JV_ERR_SHAPE
    assert not small.any()
    for bad in ((0, 24000), (24000, 0), (-1, 24000), (24000, -5)):
        assert lib.jv_resample_table(bad[0], bad[1], None, 0, None, None, None) == 1      # JV_ERR_ARG


# ---- lengths ----------------------------------------------------------------------------------------------------------------
def test_lengths_are_exact_integer_ceilings(lib):
    f = lib.jv_resample_length
    near = [2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 31 + 147]
    for orig, new in ref.PAIRS + EXTRA_PAIRS + [(24000, 24000), (192000, 8000), (8000, 192000)]:
        for n in list(range(0, 400)) + near:
            want = -(-new * n // orig)      # Python integers: exact
            assert f(n, orig, new) == want, (n, orig, new)
            assert want == ref.out_length(n, orig, new)
    assert f(12345, 24000, 24000) == 12345
    assert f(2 ** 62, 1, 3) == -1      # beyond int64
    for bad in ((-1, 24000, 16000), (10, 0, 16000), (10, 24000, 0), (10, -3, 16000)):
        assert f(*bad) == -1


# ---- the cap ----------------------------------------------------------------------------------------------------------------
def test_cap_admits_every_standard_pair_and_rejects_near_coprime(lib):
    pairs = list(itertools.permutations(ref.STANDARD_RATES, 2))
    assert len(pairs) == 156
    largest = 0
    for orig, new in pairs:
        o, n, w = C.c_int32(), C.c_int32(), C.c_int32()
        assert lib.jv_resample_table(orig, new, None, 0, C.byref(o), C.byref(n), C.byref(w)) == 0, (orig, new)
        assert (o.value, n.value, w.value) == ref.geometry(orig, new)[:3]
        entries = n.value * (2 * w.value + o.value)
        assert entries <= ref.TABLE_CAP
        largest = max(largest, entries)
    assert largest == 582400
    from jyutvoice_amd._lib import JvError, check
    rc = lib.jv_resample_table(44101, 24000, None, 0, None, None, None)
    assert rc == 1
    with pytest.raises(JvError, match=r"o = 44101, n = 24000.*1048576"):
        check(rc)


# ---- the restatement itself -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", ref.PAIRS)
def test_restatement_is_upfirdn_of_the_sampled_prototype(orig, new):
    """y[j] = sum_m h(m / o - j / n) x[m]: the prototype sampled on the 1 / (o n) grid, applied by scipy's polyphase
    upfirdn(up = n) and decimated by o"""
    signal = pytest.importorskip("scipy.signal")
    o, n, width, K, base = ref.geometry(orig, new)
    half = -(-math.ceil(6 * o * n / base) // o) * o      # support of h on the fine grid, rounded up to whole output samples
    q = np.arange(-half, half + 1, dtype=np.float64)
    u = base * q / (o * n)
    pu = np.pi * u
    hg = np.where(np.abs(u) <= 6.0, (base / o) * np.where(q == 0, 1.0, np.sin(pu) / np.where(q == 0, 1.0, pu)) *
                  np.cos(np.pi * u / 12.0) ** 2, 0.0)
    x = ref.signal(3, 1500).astype(np.float64)
    full = signal.upfirdn(hg, x, up=n, down=o)
    got = ref.resample64(x, orig, new)
    first = half // o
    err = float(np.abs(full[first:first + got.size] - got).max())
    assert err <= 1e-12, err


@pytest.mark.parametrize("orig,new", ref.PAIRS)
def test_restatement_reproduces_a_sinusoid(orig, new):
    """amplitude 0.5 at 0.1 min(orig, new) Hz comes back within 1e-3, 200 samples away from the ends (the definition's own figures
    are 2.0e-4 .. 4.3e-4; the cap catches a wrong rolloff, width or scale)"""
    f, L = 0.1 * min(orig, new), 3000
    x = 0.5 * np.sin(2 * np.pi * f * np.arange(L) / orig)
    y = ref.resample64(x, orig, new)
    want = 0.5 * np.sin(2 * np.pi * f * np.arange(y.size) / new)
    assert y.size == ref.out_length(L, orig, new) > 600
    err = float(np.abs(y - want)[200:-200].max())
    print(f"{orig} -> {new}: sinusoid reproduced to {err:.2e}")
    assert err <= 1e-3, err


@pytest.mark.parametrize("orig,new", ref.PAIRS)
def test_gpu_bound_catches_a_wrong_restatement(orig, new):
    """on the GPU test's own input (the seam recording) each slip lands OUTSIDE the bound the kernel is held to, so a kernel that
    passes cannot have been compared against a table with that slip.  (With n = 1 there is one phase, p = 0, and the sign of p / n
    is not a slip that exists: the table is the same, which is asserted instead.)"""
    x = ref.signal(ref.pair_seed(orig, new), ref.SEAM_SAMPLES)
    good, bnd = ref.resample64(x, orig, new), ref.bound(x, orig, new)
    assert good.size == bnd.size and float(bnd.min()) > 0.0
    for m in ref.MUTANTS:
        tab = ref.table(orig, new, mutate=m)
        if m == "phase_sign" and ref.geometry(orig, new)[1] == 1:
            assert np.array_equal(tab, ref.table(orig, new))
            continue
        ratio = np.abs(ref.resample64(x, orig, new, tab=tab) - good) / bnd
        print(f"{orig} -> {new} {m}: max |mutant - definition| / bound = {ratio.max():.3g}, outside for {np.mean(ratio > 1):.3f} of the samples")
        assert float(ratio.max()) > 1.0, (m, float(ratio.max()))


def test_fp32_evaluation_sits_inside_the_bound():
    """the bound is a bound: the same sums in fp32 (numpy's own order) stay below it for every pair"""
    for orig, new in ref.PAIRS:
        x = ref.signal(ref.pair_seed(orig, new), 4001)
        o, n, width, K, _ = ref.geometry(orig, new)
        L_out = ref.out_length(x.size, orig, new)
        X = ref._frames(x, o, width, K, -(-L_out // n)).astype(np.float32)
        t32 = ref.table(orig, new).astype(np.float32)
        y32 = np.zeros((X.shape[0], n), dtype=np.float32)
        for k in range(K):      # one fp32 multiply and add per tap, ascending: no better than the kernel's fused chain
            y32 += X[:, k:k + 1] * t32[None, :, k]
        err = np.abs(y32.reshape(-1)[:L_out].astype(np.float64) - ref.resample64(x, orig, new))
        assert float((err / ref.bound(x, orig, new)).max()) < 1.0


# ---- the WAV reader ---------------------------------------------------------------------------------------------------------
riff, fmt16, fmt_ext, pcm_bytes = ref.riff, ref.fmt16, ref.fmt_ext, ref.pcm_bytes


def load(tmp_path, blob):
    from jyutvoice_amd.utils.audio import load_wav
    path = tmp_path / "t.wav"
    path.write_bytes(blob)
    return load_wav(str(path))


@pytest.mark.parametrize("bits", [8, 16, 24, 32])
def test_wav_pcm_round_trip(tmp_path, bits):
    top = 1 << (bits - 1)
    ints = [0, 1, -1, top - 1, -top, top // 3, -(top // 5), 77 % top, -(99 % top)]
    wav, rate = load(tmp_path, riff(fmt16(1, 1, 16000, bits), pcm_bytes(ints, bits)))
    assert rate == 16000 and wav.dtype == torch.float32 and wav.shape == (1, len(ints))
    want = torch.tensor([v / top for v in ints], dtype=torch.float64).float()
    assert torch.equal(wav[0], want)


def test_wav_float_formats(tmp_path):
    vals = np.array([0.0, 0.25, -0.5, 0.999, -1.0, 1e-3], dtype=np.float32)
    wav, rate = load(tmp_path, riff(fmt16(3, 1, 48000, 32), vals.astype("<f4").tobytes()))
    assert rate == 48000 and torch.equal(wav[0], torch.from_numpy(vals))
    wav, rate = load(tmp_path, riff(fmt16(3, 1, 44100, 64), vals.astype("<f8").tobytes()))
    assert rate == 44100 and torch.equal(wav[0], torch.from_numpy(vals))


def test_wav_extensible(tmp_path):
    ints = [5, -6, 70000, -80000]
    wav, rate = load(tmp_path, riff(fmt_ext(1, 1, 44100, 24), pcm_bytes(ints, 24)))
    assert rate == 44100 and torch.equal(wav[0], torch.tensor([v / (1 << 23) for v in ints], dtype=torch.float64).float())
    vals = np.array([0.5, -0.125], dtype=np.float32)
    wav, rate = load(tmp_path, riff(fmt_ext(3, 1, 96000, 32), vals.tobytes()))
    assert rate == 96000 and torch.equal(wav[0], torch.from_numpy(vals))


def test_wav_stereo_is_averaged(tmp_path):
    left, right = [1000, -2000, 30000], [3000, 2000, -30000]
    inter = [v for pair in zip(left, right) for v in pair]
    wav, rate = load(tmp_path, riff(fmt16(1, 2, 22050, 16), pcm_bytes(inter, 16)))
    assert rate == 22050 and wav.shape == (1, 3)
    assert torch.equal(wav[0], torch.tensor([(a + b) / 2 / 32768 for a, b in zip(left, right)], dtype=torch.float64).float())


def test_wav_unknown_and_odd_chunks_are_skipped(tmp_path):
    """a LIST chunk of odd size (with its pad byte) before the data, an 8-bit data chunk of odd size and a chunk behind it"""
    ints = [1, -2, 3, -4, 5]
    odd = b"LIST" + struct.pack("<I", 7) + b"INFOabc" + b"\0"
    tail = b"cue " + struct.pack("<I", 4) + b"\0\0\0\0"
    wav, rate = load(tmp_path, riff(fmt16(1, 1, 8000, 8), pcm_bytes(ints, 8), extra_before=odd, extra_after=tail))
    assert rate == 8000 and torch.equal(wav[0], torch.tensor([v / 128 for v in ints]))


@pytest.mark.parametrize("size", [0, 0xFFFFFFFF])
def test_wav_streamed_data_size_reads_to_the_end(tmp_path, size):
    ints = list(range(-50, 50))
    wav, _ = load(tmp_path, riff(fmt16(1, 1, 16000, 16), pcm_bytes(ints, 16), data_size=size))
    assert torch.equal(wav[0], torch.tensor([v / 32768 for v in ints]))


def test_wav_bad_files_raise(tmp_path):
    good_fmt, data = fmt16(1, 1, 16000, 16), pcm_bytes([1, 2, 3], 16)
    bad = {
        "not RIFF": b"RIFX" + riff(good_fmt, data)[4:],
        "not WAVE": riff(good_fmt, data)[:8] + b"AVI " + riff(good_fmt, data)[12:],
        "short": b"RIFF\0\0",
        "no data": riff(good_fmt, data)[:12 + 8 + 16],
        "mu-law": riff(fmt16(7, 1, 8000, 8), b"\0" * 8),
        "12-bit": riff(fmt16(1, 1, 8000, 12), b"\0" * 8),
        "float16": riff(fmt16(3, 1, 8000, 16), b"\0" * 8),
        "no channels": riff(fmt16(1, 0, 8000, 16), data),
        "truncated fmt": b"RIFF" + struct.pack("<I", 20) + b"WAVEfmt " + struct.pack("<I", 16) + b"\1\0\1\0",
        "extensible without sub-format": riff(fmt16(0xFFFE, 1, 8000, 16), data),
    }
    for name, blob in bad.items():
        with pytest.raises(ValueError):
            load(tmp_path, blob)
            pytest.fail(name)
    data_first = b"WAVE" + b"data" + struct.pack("<I", len(data)) + data + b"fmt " + struct.pack("<I", 16) + good_fmt
    with pytest.raises(ValueError, match="before the fmt"):
        load(tmp_path, b"RIFF" + struct.pack("<I", len(data_first)) + data_first)
    with pytest.raises(OSError):
        from jyutvoice_amd.utils.audio import load_wav
        load_wav(str(tmp_path / "missing.wav"))
