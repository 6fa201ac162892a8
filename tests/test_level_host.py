"""CPU: the host half of the level kernels (jv_kweight_coeffs, jv_loudness_blocks: no device needed), the fp64 restatements the GPU
test trusts (tests/level_ref.py) checked for themselves, the conditions on the GPU test's inputs asserted on the reference alone, what
lands outside its bound, and the argument validation of the Python wrappers and of infer.py's flags."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import level_ref as ref


@pytest.fixture(scope="module")
def lib():
    import os

    from jyutvoice_amd import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from jyutvoice_amd import _lib
    return _lib.load()


def coeffs(lib, fs):
    out = (C.c_double * 10)()
    assert lib.jv_kweight_coeffs(fs, out) == 0
    return np.array(out[:])


def test_reference_filter_equals_scipy_lfilter():
    from scipy.signal import lfilter
    x = ref.one_level(5000).astype(np.float64)
    for fs in (16000, 22050, 48000):
        c = ref.kweight(fs)
        want = lfilter(c[5:8], [1.0, c[8], c[9]], lfilter(c[:3], [1.0, c[3], c[4]], x))
        got = ref.kfilter(x, fs)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_kweight_coeffs_match_the_standard_and_the_reference(lib):
    assert np.abs(coeffs(lib, 48000) - np.array(ref.TABLE_48K)).max() <= 1e-12
    for fs in (16000, 22050, 24000, 44100, 48000):
        assert np.abs(coeffs(lib, fs) - ref.kweight(fs)).max() <= 1e-14, fs
    out = (C.c_double * 10)()
    for bad in (0, -1, 7999, 192001):
        assert lib.jv_kweight_coeffs(bad, out) == 1      # JV_ERR_ARG
        assert lib.jv_loudness_blocks(48000, bad) == -1
    assert lib.jv_kweight_coeffs(8000, out) == 0 and lib.jv_kweight_coeffs(192000, out) == 0
    assert lib.jv_kweight_coeffs(48000, None) == 1


def test_loudness_blocks_around_four_hops(lib):
    for fs in (8000, 16000, 22050, 24000, 44100, 48000, 192000):
        h = ref.hop(fs)
        assert h == (fs + 5) // 10
        for n in (0, 1, 4 * h - 1, 4 * h, 4 * h + 1, 5 * h - 1, 5 * h, 5 * h + 1, 60 * fs, 1400000):
            want = 0 if n < 4 * h else (n - 4 * h) // h + 1
            assert lib.jv_loudness_blocks(n, fs) == want == ref.blocks(n, fs), (fs, n)
    assert ref.hop(22050) == 2205 and ref.hop(22050) % 2 == 1


def test_calibration_sine():
    """the standard's calibration point: a full-scale 997 Hz sine at 48 kHz measures -3.01 LUFS"""
    assert abs(ref.lufs64(ref.sine997(), 48000)[0] - -3.010) <= 1e-3


def test_four_level_sizes():
    assert ref.four_level(16000, 100).size == 38399 and ref.four_level(24000, 100).size == 57600


# ---- the conditions on the GPU test's inputs, on the reference alone ----------------------------------------------------------------
def test_trim_cases_have_no_frame_near_the_threshold():
    worst = math.inf
    for lead in ref.TRIM_LEADS:
        s, e, ratio = ref.trim64(ref.trim_recording(lead))
        assert s % ref.TRIM_H == 0 and lead - 2 * ref.TRIM_H < s <= lead and lead + 3000 <= e <= ref.trim_recording(lead).size
        worst = min(worst, float(np.abs(ratio - 1.0).min()))
    for name, (x, F, H) in ref.trim_edge_cases().items():
        ratio = ref.trim64(x, ref.TRIM_DB, F, H)[2]
        if ratio.size:
            worst = min(worst, float(np.abs(ratio - 1.0).min()))
    assert worst >= 1e-3, worst
    assert {l % ref.TRIM_H for l in ref.TRIM_LEADS} == {(l - 100) % ref.TRIM_H for l in ref.TRIM_LEADS} == set(range(ref.TRIM_H))


def test_trim_edges_by_the_definition():
    cases = ref.trim_edge_cases()
    got = {k: ref.trim64(x, ref.TRIM_DB, F, H)[:2] for k, (x, F, H) in cases.items()}
    assert got["n0"] == (0, 0) and got["n1"] == (0, 1) and got["n_h_minus_1"] == (0, 219) and got["n_h"] == (0, 220)
    assert got["n_5h"] == (0, 1100) and got["zeros"] == (0, 3000) and got["below_amin"] == (0, 3000)      # nothing trimmed
    assert got["spike_first"] == (0, 440) and got["spike_last"] == (2860, 3000)      # (a sample lies in two frames)
    assert got["frame_beyond_n"] == (0, 300)
    assert got["spike_at_hop"] == (220, 660)      # (reflect padding would mirror it into frame 0: start 0)


@pytest.mark.parametrize("fs", ref.RATES)
def test_loudness_cases_keep_their_distance_from_the_gates(fs):
    for seed in ref.SEEDS:
        _, L, (m_abs, m_rel), floor = ref.gate_case(fs, seed)
        assert math.isfinite(L) and m_abs >= 0.1 and m_rel >= 0.1, (fs, seed, m_abs, m_rel)
        assert floor > 0
    # the kernel rounds L to fp32 once: half an ulp at |L| < 32 is 2^-20, which must fit the bound with room to spare
    assert ref.rate_bound(fs) >= 4 * 2.0 ** -20
    assert ref.rate_bound(fs) <= 1e-3      # ... and a mistake in a gate or a seam (0.01 LU and up) cannot hide in it


def test_seam_lengths_cover_the_kernel_constants():
    h = ref.hop(24000)
    lens = ref.seam_lengths()
    for span in (ref.SEG, ref.WAVE_SPAN, ref.GROUP_SPAN):
        assert any(n % span == 0 and n >= 4 * h and n - 1 in lens and n + 1 in lens for n in lens), span
    for n in lens[1:]:
        L, _, (m_abs, m_rel) = ref.lufs64(ref.one_level(n), 24000)
        assert math.isfinite(L) and m_abs >= 0.1 and m_rel >= 0.1, n
    assert ref.lufs64(ref.one_level(4 * h - 1), 24000)[0] == -math.inf
    assert ref.lufs64(np.zeros(3 * 24000), 24000)[0] == -math.inf
    assert ref.lufs64(ref.one_level(3 * 24000, sigma=1e-5), 24000)[0] == -math.inf      # below the absolute gate


# ---- what lands outside the bound ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [dict(rel_gate=False), dict(overlap_hops=2), dict(offset=0.0), dict(coeff_fs=48000)],
                         ids=["no_relative_gate", "half_overlap", "no_offset", "coefficients_of_48k"])
def test_mistaken_meters_miss_the_bound(variant):
    fs = 24000
    for seed in ref.SEEDS:
        x, L, _, _ = ref.gate_case(fs, seed)
        assert abs(ref.lufs64(x, fs, **variant)[0] - L) > ref.rate_bound(fs), (variant, seed)


def test_reflect_padding_moves_a_trim_bound():
    moved = 0
    for name, (x, F, H) in ref.trim_edge_cases().items():
        if x.size > F // 2:      # (numpy's reflect needs more samples than the pad)
            moved += ref.trim64(x, ref.TRIM_DB, F, H)[:2] != ref.trim64(x, ref.TRIM_DB, F, H, pad="reflect")[:2]
    assert moved >= 1
    x, F, H = ref.trim_edge_cases()["spike_at_hop"]
    assert ref.trim64(x, ref.TRIM_DB, F, H, pad="reflect")[0] == 0 != ref.trim64(x, ref.TRIM_DB, F, H)[0]


def test_gain_rules():
    assert ref.gain64(-math.inf, 0.5) == 1.0 and ref.gain64(-20.0, 0.0, ceiling=0.9) == 1.0
    assert abs(ref.gain64(-29.0, 0.1, -23.0) - 10.0 ** 0.3) < 1e-15
    assert ref.gain64(-29.0, 0.6, -23.0, 0.9) == 0.9 / 0.6      # the ceiling binds
    assert ref.gain64(None, 0.95, ceiling=0.8) == 0.8 / 0.95 and ref.gain64(None, 0.5, ceiling=0.8) == 1.0


# ---- argument validation that needs no device ----------------------------------------------------------------------------------------
class _NoDeviceEngine:
    """Engine's validation runs before the library is called: an object with the methods and no context shows it"""
    device = torch.device("cpu")

    def __getattr__(self, name):
        from jyutvoice_amd.engine import Engine
        return getattr(Engine, name).__get__(self)


def test_engine_wrappers_name_the_bad_argument():
    eng, x = _NoDeviceEngine(), torch.zeros(2, 100)
    with pytest.raises(ValueError, match="wav must be"):
        eng.trim_bounds(torch.zeros(100))
    with pytest.raises(ValueError, match="lens must have shape"):
        eng.trim_bounds(x, torch.zeros(3, dtype=torch.int32))
    for kw, what in ((dict(top_db=0), "top_db"), (dict(top_db=float("inf")), "top_db"), (dict(frame_length=0), "frame_length"),
                     (dict(frame_length=8193), "frame_length"), (dict(hop_length=0), "hop_length")):
        with pytest.raises(ValueError, match=what):
            eng.trim_bounds(x, **kw)
    for rate in (7999, 192001, 24000.0):
        with pytest.raises(ValueError, match="sample_rate"):
            eng.loudness(x, rate)
    with pytest.raises(ValueError, match="start must have shape"):
        eng.peak(x, start=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="ceiling"):
        eng.level_gain(torch.zeros(2), torch.ones(2), ceiling=-1.0)
    with pytest.raises(ValueError, match="ceiling needs peak"):
        eng.level_gain(torch.zeros(2), None, ceiling=0.9)
    with pytest.raises(ValueError, match="prompt rule"):
        eng.level_gain(None, torch.ones(2))
    with pytest.raises(ValueError, match="target"):
        eng.level_gain(torch.zeros(2), None, target=float("nan"))
    with pytest.raises(ValueError, match="tail"):
        eng.level_apply(x, tail=-1)
    with pytest.raises(ValueError, match="gain must have shape"):
        eng.level_apply(x, gain=torch.ones(3))


def test_condition_prompt_validates_on_the_host():
    from jyutvoice_amd.utils.audio import condition_prompt
    x = [torch.zeros(1, 1000), torch.zeros(2000)]
    for kw, what in ((dict(sample_rates=[16000]), "2 recordings, 1 sample rates"), (dict(peak=0.0), "peak"), (dict(top_db=-3), "top_db"),
                     (dict(tail_seconds=-0.1), "tail_seconds"), (dict(sample_rates=[16000, 0]), "positive")):
        with pytest.raises(ValueError, match=what):
            condition_prompt(x, **kw)
    with pytest.raises(ValueError, match="no recordings"):
        condition_prompt([])


def test_server_submit_validates_loudness():
    from jyutvoice_amd.serve import SynthServer
    srv = SynthServer.__new__(SynthServer)      # submit() is host only: no context is needed to refuse a request
    srv._next_rid, srv.max_tokens, srv.max_frames, srv.row_capacity = 0, 64, 256, 10 ** 6
    ids = torch.zeros(1, 4, dtype=torch.int64)
    common = (ids, torch.tensor([4]), ids, ids, ids, ids, torch.zeros(1, 192))
    for kw, what in ((dict(loudness=float("nan")), "loudness"), (dict(loudness="loud"), "loudness"), (dict(loudness=-20, peak=0.0), "peak"),
                     (dict(peak=0.9), "give loudness too")):
        with pytest.raises(ValueError, match=what):
            srv.submit(*common, **kw)


def test_infer_flag_conflicts(capsys):
    import infer
    for extra in (["--stream-hop", "4"], ["--stream-hop", "4", "--stream-sessions", "2"]):
        with pytest.raises(SystemExit) as e:
            infer.main(["--output", "x.wav", "--token2wav", "list.json", "--loudness", "-23"] + extra)
        assert e.value.code == 2
        assert "integrated loudness needs the whole utterance" in capsys.readouterr().err
    for flags, what in ((["--peak", "0.9"], "--loudness"), (["--loudness", "nan"], "finite"), (["--loudness", "-23", "--peak", "0"], "--peak"),
                        (["--prompt-trim-db", "-1"], "--prompt-trim-db"), (["--prompt-tail", "-1"], "--prompt-tail")):
        with pytest.raises(SystemExit) as e:
            infer.main(["--output", "x.wav", "--synthetic", "4"] + flags)
        assert e.value.code == 2 and what in capsys.readouterr().err
