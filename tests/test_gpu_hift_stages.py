"""GPU: every stage of the vocoder's decode outside its ResBlock kernels, read through jv_hift_decode_tap -- the 16-point STFT rows,
conv_pre, the three polyphase up-convolutions (the last behind its reflection pad), the strided source convolutions, the source
ResBlock sum, the MRF mean, conv_post, the inverse-DFT frames -- and the overlap-added waveform, each held to the plain fp64
reference of ITS OWN operation (tests/hift_stage_ref.py) evaluated on the GPU's own previous tap, so that an error is charged to
the stage that made it and the failure names the stage, the utterance and the row.

The bound is test_gpu_fused_ops.py's, unchanged (fo.distances, RATIO = 8): the worst row of |kernel - fp64| over that row's own fp64
magnitude may be 8 x the same figure of the fp32 evaluation of the same formula on the CPU, and that floor must be > 0.  A row is
one time position's channel vector of one utterance over its live positions (taps), or the 480 samples of one mel frame
(waveform: the first and the last frame stand alone).  Every figure goes to parity_hift_stages.json (committed under profiles/).

The cases (hift_stage_ref.CASES) are the smallest at which these stages can go wrong: T = 1, 2, 3 (every polyphase tap of the one
frame reads gap rows; both reflections fold inside 480 samples), ragged batches that take the compact geometry, a dead utterance
between live ones, utterance ends inside and across the last level's tiles, utterances of very different magnitude (the
per-utterance fp16x3 bounds) and a checkpoint whose log-magnitudes cross the clamp at ln 100.  The conditions those last two are
built on are asserted on the fp64 reference alone, without a GPU, in test_hift_stage_refs_host.py, which also shows that the
bound catches seventeen plausible mistakes on these cases.

MAG_SCALES.  Mel scales of 1 / 30 / 0.03 were the first choice; at 30 the fp64 reference clips 92 % of its samples (at 4: 55 %,
at 1.5: 1.07 %), which parity_util.CLAMP_CAP forbids, and conv_pre's bias keeps the small utterance's maximum at 0.08 whatever the
scale.  1 / 1.4 / 0.003 keeps the clipped share below 1 % with conv_pre maxima of 3.4 / 5.2 / 0.08 (65 x apart; >= 8 x asserted)."""
import functools
import math

import pytest
import torch

import hift_stage_ref as hs
import parity_util as pu
import test_gpu_fused_ops as fo      # distances / RATIO (a module object: none of its tests is collected here)
from test_gpu_vocoder_unclipped import make_engine

pytestmark = pytest.mark.gpu

RATIO = fo.RATIO
GEOMETRIES = ("default", "uniform")      # default: the compact geometry where hift_decode's rule takes it; uniform: JV_NO_COMPACT=1
STAGES = hs.TAPS + ("WAV",)
record = pu.Recorder("parity_hift_stages.json", {
    "what": "per case / geometry / utterance / stage: worst row of |kernel - fp64| / max |fp64 row| (kernel), of the same formula in fp32 "
            "torch on the CPU (floor), and their ratio; the reference of a stage is evaluated on the GPU's own previous tap",
    "bound": "kernel <= 8 x floor, floor > 0", "rows": "taps: one time position's channels; WAV: the 480 samples of one mel frame",
    "cases": {k: {"T": v[1], "lens": list(v[2])} for k, v in hs.CASES.items()},
    "mag_scales": list(hs.MAG_SCALES), "clamp_bias": hs.CLAMP_BIAS})


@pytest.fixture(scope="module", autouse=True)
def engines():
    """(checkpoint, geometry) -> a context of its own, made when first asked for, closed behind the module"""
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    made = {}

    def get(case, geometry):
        key = ("clamp" if case == "clamp" else "tame", geometry)
        if key not in made:
            made[key] = make_engine(hs.checkpoint(case), 4, 64, **({"JV_NO_COMPACT": "1"} if geometry == "uniform" else {}))
        return made[key]

    _STATE["engine"] = get
    yield get
    _STATE.clear()
    run.cache_clear()
    references.cache_clear()
    for e in made.values():
        e.close()


_STATE = {}


def lens_tensor(lens):
    return torch.tensor(lens, dtype=torch.int32)


def tapped(eng, mel, s, lens):
    """every tap, the waveform and f0 of one batch, on the CPU"""
    out = {tap: eng.hift_decode_tap(mel, s, lens_tensor(lens), tap).cpu() for tap in hs.TAPS}
    out["WAV"] = eng.hift_decode(mel, s, lens_tensor(lens)).cpu()
    out["F0"] = eng.hift_f0(mel, lens_tensor(lens)).cpu()
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def run(case, geometry):
    mel, s, lens = hs.inputs(case)
    return tapped(_STATE["engine"](case, geometry), mel, s, lens)


def utterance(got, case, b):
    """the live part of utterance b of a run: {stage: [1, C, live]} (waveform [1, 480 L]), + its mel and whole source row"""
    mel, s, lens = hs.inputs(case)
    L = lens[b]
    out = {k: got[k][b:b + 1, ..., :hs.live(k, L)] for k in STAGES}
    out["mel"], out["s"] = mel[b:b + 1, :, :L], s[b]
    return out


@functools.lru_cache(maxsize=None)
def references(case, geometry, b, stage):
    """(fp64 reference rows, fp32 floor rows, the mask of compared entries or None) of a stage of utterance b, from the previous
    taps of the run in `geometry`; the uniform run shares the default run's when its previous taps hold the same bits"""
    u, L = utterance(run(case, geometry), case, b), hs.CASES[case][2][b]
    if geometry != "default":
        d = utterance(run(case, "default"), case, b)
        if all(torch.equal(u[n], d[n]) for n in hs.SOURCES[stage]):
            return references(case, "default", b, stage)
    ws = hs.weights(case)
    r64, r32 = (hs.evaluate(stage, ws, u, L, dt).double() for dt in (torch.float64, torch.float32))
    keep = None
    if case == "clamp" and stage == "WAV":      # where the reference reads the clip, both sides read 0.99 whatever was computed
        keep = hs.rows_of(stage, hs.ola(u["FRAMES"], torch.float64, clip=False).abs() < pu.AUDIO_LIMIT)
    return hs.rows_of(stage, r64), hs.rows_of(stage, r32), keep


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("case", list(hs.CASES))
def test_stage_parity(case, geometry):
    """1. every tap and the waveform of every utterance against the fp64 reference of its stage, in both geometries"""
    got, lens = run(case, geometry), hs.CASES[case][2]
    failures = []
    for b, L in enumerate(lens):
        if L == 0:
            continue
        u = utterance(got, case, b)
        for stage in STAGES:
            r64, r32, keep = references(case, geometry, b, stage)
            rows = hs.rows_of(stage, u[stage]).double()
            assert rows.shape == r64.shape, (case, b, stage, rows.shape, r64.shape)
            if keep is not None:
                rows, r64, r32 = rows * keep, r64 * keep, r32 * keep
            kd, fl = fo.distances(rows, r64, r32, slice(None))
            worst = int(((rows - r64).abs().amax(dim=1) / r64.abs().amax(dim=1).clamp_min(1e-30)).argmax())
            record(f"{case}/{geometry}/utt{b}/{stage}", kernel=kd, floor=fl, ratio=kd / fl if fl > 0 else float("inf"), worst_row=worst)
            if not (fl > 0.0 and math.isfinite(kd) and kd <= RATIO * fl):
                failures.append(f"{case}/{geometry} utt{b} ({L} frames) {stage}: row {worst} of {rows.shape[0]}: "
                                f"kernel {kd:.3e} = {kd / max(fl, 1e-300):.2f} x floor {fl:.3e}")
    assert not failures, failures


@pytest.mark.parametrize("case", list(hs.CASES))
def test_geometries_give_the_same_bits(case):
    """2. every tap, the waveform and f0 are bit-equal between the compact and the uniform run (whole tensors: the zeros too), and
    the default run did lay its rows out compactly where the 8 % rule says so"""
    a, u = run(case, "default"), run(case, "uniform")
    for k in STAGES + ("F0",):
        assert torch.equal(a[k], u[k]), (case, k, pu.md(a[k], u[k]))
    if case in hs.COMPACT_CASES:
        mel, s, lens = hs.inputs(case)
        reports = [pu.profiled(lambda g=g: _STATE["engine"](case, g).hift_decode(mel, s, lens_tensor(lens))) for g in GEOMETRIES]
        pu.assert_compact_taken(reports[0], reports[1], lens, mel.shape[2], "hiftpair_h3<", "x128,snake>")


@pytest.mark.parametrize("case", ["ragged7", "mags"])
def test_utterances_do_not_see_their_batch(case):
    """3. every tap of each utterance equals the same utterance decoded alone at B = 1, bit for bit"""
    mel, s, lens = hs.inputs(case)
    got = run(case, "default")
    for b, L in enumerate(lens):
        alone = tapped(_STATE["engine"](case, "default"), mel[b:b + 1, :, :L], s[b:b + 1, :, :480 * L], (L,))
        for k in STAGES:
            assert torch.equal(got[k][b:b + 1, ..., :hs.live(k, L)], alone[k]), (case, b, k)


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("case", list(hs.CASES))
def test_zeros_behind_the_lengths(case, geometry):
    """4. positions behind a length, and a dead utterance, are exactly zero in every tap and in the waveform; all is finite"""
    got, lens = run(case, geometry), hs.CASES[case][2]
    for k in STAGES:
        assert torch.isfinite(got[k]).all(), (case, k)
        assert got[k].shape[-1] == hs.live(k, hs.CASES[case][1]), (case, k, got[k].shape)
        for b, L in enumerate(lens):
            tail = got[k][b, ..., hs.live(k, L):]
            assert float(tail.abs().max() if tail.numel() else 0.0) == 0.0, (case, b, k)
            if L > 0:      # (a tap that copied nothing would pass the line above)
                assert float(got[k][b, ..., :hs.live(k, L)].abs().max()) > 0.0, (case, b, k)
    assert torch.isfinite(got["F0"]).all()


def test_the_tap_changes_nothing():
    """5. the waveform behind a series of tapped calls is the waveform ahead of them; a tap twice gives the same bits; an output
    buffer that is too small and a tap that does not exist are errors"""
    from jyutvoice_amd._lib import HIFT_TAPS, JvError
    assert sorted(HIFT_TAPS) == sorted(hs.TAPS) and sorted(v[0] for v in HIFT_TAPS.values()) == list(range(16))
    for tap, (_, C, mul, add) in HIFT_TAPS.items():
        assert (mul, add) == hs.POSITIONS[tap], tap
    case = "ragged7"
    mel, s, lens = hs.inputs(case)
    eng, lt = _STATE["engine"](case, "default"), lens_tensor(lens)
    before = eng.hift_decode(mel, s, lt).cpu()
    first = {tap: eng.hift_decode_tap(mel, s, lt, tap).cpu() for tap in hs.TAPS}
    for tap in reversed(hs.TAPS):
        assert torch.equal(eng.hift_decode_tap(mel, s, lt, tap).cpu(), first[tap]), tap
    assert torch.equal(eng.hift_decode(mel, s, lt).cpu(), before)
    assert torch.equal(before, run(case, "default")["WAV"])
    small = torch.full((first["UP1"].numel() - 1,), 7.0, device="cuda:0")
    with pytest.raises(JvError) as err:
        eng.hift_decode_tap(mel, s, lt, "UP1", out=small)
    assert err.value.code == 4      # JV_ERR_SHAPE
    assert float((small - 7.0).abs().max()) == 0.0      # rejected ahead of the first launch
    for bad in (-1, 16):
        with pytest.raises(JvError) as err:
            eng.hift_decode_tap(mel, s, lt, bad)
        assert err.value.code == 1      # JV_ERR_ARG
    assert torch.equal(eng.hift_decode(mel, s, lt).cpu(), before)


@pytest.mark.parametrize("case", list(hs.CASES))
def test_f0_predictor(case):
    """6. the five convolutions and the head of the F0 predictor against oracle.hift.f0_predict in fp64: every frame against the
    utterance's own max |f0|, 8 x the fp32 floor"""
    mel, s, lens = hs.inputs(case)
    ws, failures = hs.weights(case), []
    for geometry in GEOMETRIES:
        got = run(case, geometry)["F0"]
        for b, L in enumerate(lens):
            if L == 0:
                continue
            r64, r32 = (hs.f0(ws, mel[b:b + 1, :, :L], dt).double() for dt in (torch.float64, torch.float32))
            scale = float(r64.abs().max())
            kd, fl = float((got[b:b + 1, :L].double() - r64).abs().max()) / scale, float((r32 - r64).abs().max()) / scale
            record(f"{case}/{geometry}/utt{b}/F0", kernel=kd, floor=fl, ratio=kd / fl if fl > 0 else float("inf"))
            if not (fl > 0.0 and math.isfinite(kd) and kd <= RATIO * fl):
                failures.append(f"{case}/{geometry} utt{b} ({L} frames) F0: kernel {kd:.3e} = {kd / max(fl, 1e-300):.2f} x floor {fl:.3e}")
    assert not failures, failures
