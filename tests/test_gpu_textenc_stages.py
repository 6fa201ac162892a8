"""GPU: every stage of the text encoder and the duration predictor, read through jv_encoder_fwd_tap -- the embedding sum, the three
prenet convolutions with their channel LayerNorm, the projection + residual + concat, and per layer the RoPE'd q | k | v, the
attention, both LayerNorms and the feed-forward's hidden rows; the duration predictor's input and its two conv + ReLU + LN rows --
and the outputs x, mu_x, logw and the speaker projection, each held to the plain fp64 reference of ITS OWN operation
(tests/textenc_stage_ref.py) evaluated on the GPU's own previous taps, so that an error is charged to the stage that made it and
the failure names the case, the route, the utterance, the stage and the row.

The bound is test_gpu_fused_ops.py's (fo.distances, RATIO = 8; two derived departures, textenc_stage_ref.LONG_K / FLOOR_MIN, stated
there and recorded in the JSON: 10.4 x for the FF stages, whose K = 1728 chain test_long_contraction_alone shows to be conv_gemm's
own arithmetic, and a floor of at least half an ulp for the one-number rows of logw): the worst row of |kernel - fp64| over that row's own fp64
magnitude may be 8 x the same figure of the fp32 evaluation of the same formula on the CPU, and that floor must be > 0.  A row is one
token's channel vector of one utterance, over its live tokens.  Stages that only move data have a floor of zero and are held
torch.equal instead: columns 192:576 of H0 (the raw speaker vector and the language embedding), x against the last layer's N2 tap,
and the attention of a one-token utterance (softmax over one key is 1: att = v).  Every figure goes to parity_textenc_stages.json
(committed under profiles/).

Both attention routes run every case up to 512 tokens: "auto" (the four launches around a score buffer) and "fused" (encattn.hip's
one launch, forced with set_encoder_attention); long513 has the fused route alone.  The cases (textenc_stage_ref.CASES) are the
smallest at which these kernels can go wrong; test_textenc_stage_refs_host.py asserts their conditions on the fp64 reference alone
and shows that the bound catches each of forty-seven (mistake, stage) pairs on them."""
import functools
import math

import pytest
import torch

import parity_util as pu
import test_gpu_fused_ops as fo      # distances / RATIO (a module object: none of its tests is collected here)
import textenc_stage_ref as ts

pytestmark = pytest.mark.gpu

assert ts.RATIO == fo.RATIO
ROUTES = ("auto", "fused")
record = pu.Recorder("parity_textenc_stages.json", {
    "what": "per case / route / utterance / stage: worst row of |kernel - fp64| / max |fp64 row| (kernel), of the same formula in fp32 "
            "torch on the CPU (floor), and their ratio; the reference of a stage is evaluated on the GPU's own previous taps",
    "bound": "kernel <= 8 x floor, floor > 0; data-moving stages (H0 columns 192:576, X, one-token attention): torch.equal",
    "margins": {"FFi": "8 x sqrt(1728 / 1024) = 10.4 x floor: conv_1 contracts K = 1728 products in one fp32 chain inside the MFMAs, whose "
                       "rounding error grows as sqrt(K); 8 x was established up to K = 1024 (textenc_stage_ref.LONG_K)",
                "LOGW": "floor taken as at least 2^-24: a row is one number, half an ulp is what storing it in fp32 costs "
                        "(textenc_stage_ref.FLOOR_MIN)"},
    "rows": "one token's channel vector", "cases": {k: {"Tt": v[1], "lens": list(v[2])} for k, v in ts.CASES.items()},
    "mag_scales": list(ts.MAG_SCALES)})

_STATE = {}


def make_engine(max_batch, max_tokens):
    from jyutvoice_amd.engine import JV_MODEL_TTS, Engine
    e = Engine("cuda:0", max_batch=max_batch, max_frames=64, max_tokens=max_tokens)
    e.load_state_dict(JV_MODEL_TTS, ts.checkpoint())
    return e


@pytest.fixture(scope="module", autouse=True)
def engines():
    """a context for the cases up to 129 tokens and one for long513, made when first asked for, closed behind the module"""
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    made = {}

    def get(case):
        key = "long" if case == "long513" else "short"
        if key not in made:
            made[key] = make_engine(1, 513) if key == "long" else make_engine(3, 130)
        return made[key]

    _STATE["engine"] = get
    yield get
    _STATE.clear()
    run.cache_clear()
    references.cache_clear()
    for e in made.values():
        e.close()


def args_of(b):
    return b["x"], b["x_lengths"], b["lang"], b["tone"], b["word_pos"], b["syllable_pos"], b["spk_embed"]


def tapped(eng, b, route, taps=ts.TAPS):
    """every tap and the outputs of one batch in one route, on the CPU"""
    eng.set_encoder_attention(route)
    try:
        out = {tap: eng.encoder_tap(*args_of(b), tap).cpu() for tap in taps}
        h, mu_x, logw, c = eng.encoder(*args_of(b))
        out.update(X=h.cpu(), MU=mu_x.cpu(), LOGW=logw.cpu(), SPK=c.cpu()[:, :, None])
        torch.cuda.synchronize()
    finally:
        eng.set_encoder_attention("auto")
    return out


def taps_of(case):
    return tuple(s for s in ts.stages_of(case) if s not in ts.OUTPUTS)


def routes_of(case):
    return ("fused",) if case == "long513" else ROUTES


RUNS = [(c, r) for c in ts.CASES for r in routes_of(c)]


@functools.lru_cache(maxsize=None)
def run(case, route):
    return tapped(_STATE["engine"](case), ts.inputs(case), route, taps_of(case))


def sources(got, case, stage):
    src = {n: got[n] for n in ts.SOURCES[stage] if n != "in"}
    src["in"] = ts.inputs(case)
    return src


@functools.lru_cache(maxsize=None)
def references(case, route, stage):
    """(fp64 reference, fp32 floor) [B, C, Tt] of a stage from the previous taps of the run in `route`; the fused run shares the
    auto run's when its previous taps hold the same bits"""
    got = run(case, route)
    if route != routes_of(case)[0]:
        first = run(case, routes_of(case)[0])
        if all(torch.equal(got[n], first[n]) for n in ts.SOURCES[stage] if n != "in"):
            return references(case, routes_of(case)[0], stage)
    src, lens = sources(got, case, stage), ts.CASES[case][2]
    return tuple(ts.evaluate(stage, ts.weights(), src, lens, dt).double() for dt in (torch.float64, torch.float32))


def compared(case):
    return tuple(s for s in ts.stages_of(case) if s not in ts.LONG_SOURCE_ONLY or case != "long513")


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,route", RUNS)
def test_stage_parity(case, route):
    """1. every tap and every output of every live utterance against the fp64 reference of its stage, in both routes"""
    got, lens = run(case, route), ts.CASES[case][2]
    failures = []
    for stage in compared(case):
        r64, r32 = references(case, route, stage)
        assert got[stage].shape == r64.shape, (case, stage, got[stage].shape, r64.shape)
        mv = ts.moved(stage)
        for b, L in enumerate(lens):
            if L == 0:
                continue
            n = ts.live(stage, L)
            rows, a, f = ts.rows_of(got[stage], b, n).double(), ts.rows_of(r64, b, n), ts.rows_of(r32, b, n)
            where = f"{case}/{route} utt{b} ({L} tokens) {stage}"
            if mv is not None:
                if not torch.equal(rows[:, mv], a[:, mv]):
                    failures.append(f"{where}: columns {mv.start}:{mv.stop} only move data and differ by {pu.md(rows[:, mv], a[:, mv]):.3e}")
                if stage == "X":
                    continue
                keep = torch.ones(a.shape[1], dtype=torch.bool)
                keep[mv] = False
                rows, a, f = rows[:, keep], a[:, keep], f[:, keep]
            if ts.one_token_attention(stage, L):
                if not torch.equal(rows, a):
                    failures.append(f"{where}: one key, att = v: differs by {pu.md(rows, a):.3e}")
                continue
            kd, fl = fo.distances(rows, a, f, slice(None))
            ratio, fl = ts.ratio_of(stage), ts.floor_of(stage, fl)
            worst = int(((rows - a).abs().amax(dim=1) / a.abs().amax(dim=1).clamp_min(1e-30)).argmax())
            record(f"{case}/{route}/utt{b}/{stage}", kernel=kd, floor=fl, ratio=kd / fl if fl > 0 else float("inf"), worst_row=worst)
            if not (fl > 0.0 and math.isfinite(kd) and kd <= ratio * fl):
                failures.append(f"{where}: row {worst} of {n}: kernel {kd:.3e} = {kd / max(fl, 1e-300):.2f} x floor {fl:.3e}")
    assert not failures, failures


@pytest.mark.parametrize("case", ["ragged37", "lanes129"])
def test_long_contraction_alone(case, monkeypatch):
    """1b. FF0 is conv_gemm's arithmetic and nothing else: jv_op_conv_gemm alone (the bf16x6 loop, the same M, K = 3 x 576 and
    N = 768) on the rows of the run's own N10 tap returns the bits of the FF0 tap -- the ground of the FF stages' margin
    (textenc_stage_ref.LONG_K)"""
    from jyutvoice_amd.engine import op_conv_gemm
    monkeypatch.setenv("JV_OP_X6", "1")
    monkeypatch.delenv("JV_NO_X6", raising=False)
    got, (_, Tt, lens), sd = run(case, "auto"), ts.CASES[case], ts.weights()[torch.float32]
    G, S = 4, Tt + 4      # encoder.hip: E_G leading rows, E_GAP rows behind every utterance
    rows = G + len(lens) * S
    A = torch.zeros(rows, 576)
    for b, L in enumerate(lens):
        A[G + b * S:G + b * S + L] = ts.rows_of(got["N10"], b, L)
    w = sd["encoder.encoder.ffn_layers.0.conv_1.weight"]
    W = w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()      # [Cout, k Cin] tap-major: the library's GEMM operand
    out = op_conv_gemm(A.cuda(), W.cuda(), sd["encoder.encoder.ffn_layers.0.conv_1.bias"].cuda(), ntaps=3, tap_row0=-1, M=rows,
                       act="relu").cpu()
    for b, L in enumerate(lens):
        alone, stage = out[G + b * S:G + b * S + L], ts.rows_of(got["FF0"], b, L)
        assert torch.equal(alone, stage), (case, b, pu.md(alone, stage))


@pytest.mark.parametrize("case", ts.SHORT_CASES)
def test_routes_share_everything_but_the_attention(case):
    """2. every tap ahead of ATT0 is bit-equal between the two routes (the inputs of the first attention are identical); what
    follows is held by test 1 in each route"""
    a, f = run(case, "auto"), run(case, "fused")
    for tap in ts.TAPS[:ts.TAPS.index("ATT0")] + ("SPK",):
        assert torch.equal(a[tap], f[tap]), (case, tap, pu.md(a[tap], f[tap]))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", ["ragged37", "mags"])
def test_utterances_do_not_see_their_batch(case, route):
    """3. every tap and every output of each utterance equals the same utterance run alone at the same Tt, bit for bit"""
    got, b = run(case, route), ts.inputs(case)
    for i in range(len(ts.CASES[case][2])):
        alone = tapped(_STATE["engine"](case), ts.only(b, i), route)
        for k in ts.STAGES:
            assert torch.equal(got[k][i:i + 1], alone[k]), (case, route, i, k, pu.md(got[k][i:i + 1], alone[k]))


@pytest.mark.parametrize("case,route", RUNS)
def test_zeros_behind_the_lengths(case, route):
    """4a. positions at and behind a length, and a dead utterance, are exactly zero in every tap and output; all is finite"""
    got, (_, Tt, lens) = run(case, route), ts.CASES[case]
    for k in ts.stages_of(case):
        assert torch.isfinite(got[k]).all(), (case, k)
        assert tuple(got[k].shape) == (len(lens), ts.CHANNELS[k], ts.live(k, Tt)), (case, k, got[k].shape)
        for b, L in enumerate(lens):
            tail = got[k][b, :, ts.live(k, L):]
            assert float(tail.abs().max() if tail.numel() else 0.0) == 0.0, (case, b, k)
            if L > 0:      # (a tap that copied nothing would pass the line above)
                assert float(got[k][b, :, :ts.live(k, L)].abs().max()) > 0.0, (case, b, k)


@pytest.mark.parametrize("route", ROUTES)
def test_stale_workspace_is_not_read(route):
    """4b. t2 behind lanes129 on one context equals t2 on that context while it was fresh: the gap rows and the padded rows of
    e0, qkv, scores and vt then hold the larger call's values, and none of them is read"""
    eng = make_engine(3, 130)
    try:
        fresh = tapped(eng, ts.inputs("t2"), route)
        tapped(eng, ts.inputs("lanes129"), route, ("D2",))
        again = tapped(eng, ts.inputs("t2"), route)
    finally:
        eng.close()
    for k in ts.STAGES:
        assert torch.equal(fresh[k], again[k]), (route, k, pu.md(fresh[k], again[k]))
        assert torch.equal(fresh[k], run("t2", route)[k]), (route, k)


def test_the_tap_changes_nothing():
    """5. encoder()'s outputs behind a sweep of tapped calls are its outputs ahead of them, and the tapped run's own; a tap twice
    gives the same bits; an output buffer that is too small and a tap that does not exist are errors"""
    from jyutvoice_amd._lib import ENC_TAPS, JvError
    assert tuple(sorted(ENC_TAPS, key=lambda k: ENC_TAPS[k][0])) == ts.TAPS and [ENC_TAPS[k][0] for k in ts.TAPS] == list(range(38))
    assert all(ENC_TAPS[k][1] == ts.CHANNELS[k] for k in ts.TAPS)
    case = "ragged37"
    b, eng = ts.inputs(case), _STATE["engine"](case)
    before = [t.cpu() for t in eng.encoder(*args_of(b))]
    first = {tap: eng.encoder_tap(*args_of(b), tap).cpu() for tap in ts.TAPS}
    for tap in reversed(ts.TAPS):
        assert torch.equal(eng.encoder_tap(*args_of(b), tap).cpu(), first[tap]), tap
    after = [t.cpu() for t in eng.encoder(*args_of(b))]
    got = run(case, "auto")
    for x, y, k in zip(before, after, ("X", "MU", "LOGW", "SPK")):
        assert torch.equal(x, y), k
        assert torch.equal(x.reshape(got[k].shape), got[k]), k
    for tap in ts.TAPS:
        assert torch.equal(first[tap], got[tap]), tap
    small = torch.full((first["FF1"].numel() - 1,), 7.0, device="cuda:0")
    with pytest.raises(JvError) as err:
        eng.encoder_tap(*args_of(b), "FF1", out=small)
    assert err.value.code == 4      # JV_ERR_SHAPE
    assert float((small - 7.0).abs().max()) == 0.0      # rejected ahead of the first launch
    for bad in (-1, 38):
        with pytest.raises(JvError) as err:
            eng.encoder_tap(*args_of(b), bad)
        assert err.value.code == 1      # JV_ERR_ARG
    assert all(torch.equal(x, t.cpu()) for x, t in zip(before, eng.encoder(*args_of(b))))
