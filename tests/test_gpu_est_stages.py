"""GPU: every stage of the CFM estimator's trunk (estimator.hip Est::run), read through jv_flow_estimator_tap in both of its modes --
the three time-MLP stages and the 14 projections, the assembled input, per stage the resnet and each of its four transformer blocks,
the down / up convolutions, the final block and the projection: 79 taps -- each held to the plain fp64 reference of ITS OWN operation
(tests/est_stage_ref.py) evaluated on the GPU's own previous taps, so that an error is charged to the stage that made it and the
failure names the route, the mode, the case, the sample, the stage and the row.  What the operator tests cannot see is what this
holds: which buffer feeds which launch, the skip / concat columns, the w.h / w.h2 alternation of the whole-resnet launch, the norm1 /
q | k | v hand-offs between launches, the per-stage slice of the time embedding, the twin rows, the compact row tables, the chunk mask.

The bound is test_gpu_fused_ops.py's (fo.distances, RATIO = 8): the worst row of |kernel - fp64| over that row's own fp64 magnitude
may be 8 x the same figure of the fp32 evaluation of the same formula on the CPU, and that floor must be > 0.  A row is one frame's
channel vector of one sample, over its live frames; a time tap is one block of n rows.  Stages read behind a contraction of more
than 1024 products take the project's rule for those, 8 x sqrt(K / 1024) (est_stage_ref.LONG_K), which test_long_contraction_alone
grounds.  XIN only moves data and is held torch.equal to the reference.  Every figure goes to parity_est_stages.json (committed under
profiles/).

Routes (est_route decides them; each runs on a context of its own, created under its switches, and the route taken is asserted from
the in-library profiler): the split-K tiles (default at M <= 2048) with fp16x3 and with bf16x6 operands, the tile kernels without
split-K (bf16x6 at the smallest M above 2048), the row-owning kernels at forced tile heights with q | k | v in a launch of its own and
riding in the block launch, the whole-resnet launch with q | k | v folded in (the step mode of the latter), the compact geometry (the
step mode on a ragged batch), and the streaming chunk mask.  Not repeated here: the FP16 mode (its own error model,
test_gpu_fp16_ops.py), the JV_NO_* A/B switches test_gpu_pipeline.py pins bit-equal to the default, and attn64_s, which needs a
full-chip batch and is pinned bit for bit to attn64_pl in test_gpu_ops.py.

The cases (est_stage_ref.CASES) are the smallest at which the wiring can go wrong; test_est_stage_refs_host.py asserts their
conditions on the fp64 reference alone and shows that the bound catches each of a list of deliberate mistakes on them."""
import math

import pytest
import torch

import est_stage_ref as es
import parity_util as pu
import test_gpu_fused_ops as fo      # distances / RATIO (a module object: none of its tests is collected here)

pytestmark = pytest.mark.gpu

assert es.RATIO == fo.RATIO
SWITCHES = ("JV_ROWGEMM_RT", "JV_NO_QKV_SPLIT", "JV_NO_COMPACT")
# route -> (environment at context creation and during its calls, exact-range mode)
ROUTES = {
    "sk": ({}, False),                 # split-K tiles, fp16x3 operands where a bound is known
    "sk_x6": ({}, True),               # split-K tiles, bf16x6 everywhere
    "tiles_x6": ({}, True),            # above 2048 rows in exact-range mode: the tile kernels without split-K
    "ride2_uniform": ({"JV_ROWGEMM_RT": "2", "JV_NO_QKV_SPLIT": "1", "JV_NO_COMPACT": "1"}, False),
}
for _rt in "2345":      # row-owning kernels at a forced tile height: q | k | v in its own launch / riding in the block launch
    ROUTES["rows" + _rt] = ({"JV_ROWGEMM_RT": _rt}, False)
    ROUTES["ride" + _rt] = ({"JV_ROWGEMM_RT": _rt, "JV_NO_QKV_SPLIT": "1"}, False)
SHORT = ("t1", "t2", "ragged37", "dead", "seam", "mags")
RUNS = ([("sk", m, c) for m in ("entry", "step") for c in SHORT + ("chunk",)]
        + [("sk_x6", "entry", "ragged37"), ("sk_x6", "step", "mags"), ("tiles_x6", "entry", "big260")]
        + [("rows2", m, c) for m in ("entry", "step") for c in SHORT] + [("rows2", "entry", "chunk")]
        + [("rows5", m, c) for m in ("entry", "step") for c in ("ragged37", "dead", "seam")]
        + [("ride2", "entry", c) for c in ("ragged37", "seam")] + [("ride2", "step", c) for c in SHORT]
        + [("ride5", "entry", "seam")] + [("ride5", "step", c) for c in ("ragged37", "seam", "mags")])

record = pu.Recorder("parity_est_stages.json", {
    "what": "per route / mode / case and stage: over the live samples the worst row of |kernel - fp64| / max |fp64 row| (kernel) against "
            "the same formula in fp32 torch on the CPU (floor), as their ratio; the reference of a stage is evaluated on the GPU's own "
            "previous taps",
    "bound": "kernel <= 8 x floor, floor > 0; XIN (moves data): torch.equal",
    "margins": {k: f"8 x sqrt({v} / 1024) = {es.ratio_of(k):.1f} x floor: read behind a contraction of K = {v} products in one fp32 chain "
                   "inside the MFMAs, whose rounding error grows as sqrt(K); 8 x was established up to K = 1024 (est_stage_ref.LONG_K; "
                   "test_long_contraction_alone)" for k, v in es.LONG_K.items()},
    "rows": "one frame's channel vector of one sample; a time tap: one timestep's row",
    "layout": "measured[route/mode/case][stage] = [ratio, floor, sample of the worst ratio, its worst row]; kernel = ratio x floor",
    "routes": {k: dict(v[0], exact_range=v[1]) for k, v in ROUTES.items()},
    "cases": {k: {"T": v["T"], "lens": list(v["lens"]), "chunk": v.get("chunk", 0)} for k, v in es.CASES.items()}},
    columns=("ratio", "floor", "sample", "worst_row"))

_ENGINES, _RUNS, _REFS = {}, {}, {}


def make_engine(route, monkeypatch):
    """a context of its own for the route, created under the route's switches (some are read at creation, JV_ROWGEMM_RT at every call)"""
    from jyutvoice_amd import synth
    from jyutvoice_amd.engine import JV_MODEL_TTS, Engine
    set_env(route, monkeypatch)
    big = route == "tiles_x6"
    e = Engine("cuda:0", max_batch=4 if big else 3, max_frames=264 if big else 80, max_tokens=16)
    e.load_state_dict(JV_MODEL_TTS, synth.tts_state_dict())
    e.load_noise(synth.rand_noise())
    e.set_exact_range(ROUTES[route][1])
    return e


def set_env(route, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route][0].items():
        monkeypatch.setenv(k, v)


def engine_of(route, monkeypatch):
    if route not in _ENGINES:
        _ENGINES[route] = make_engine(route, monkeypatch)
    set_env(route, monkeypatch)
    return _ENGINES[route]


@pytest.fixture(scope="module", autouse=True)
def engines():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    yield
    _RUNS.clear()
    _REFS.clear()
    while _ENGINES:
        _ENGINES.popitem()[1].close()


def call_args(inp, mode):
    dev = lambda v: v.cuda()
    t = inp["t"] if mode == "entry" else torch.tensor([es.T_STEP])
    return mode, dev(inp["x"]), dev(inp["lens"]), dev(inp["mu"]), dev(t), dev(inp["spks"]), dev(inp["cond"])


def tapped(eng, inp, mode, taps=es.TAPS):
    """{tap: its tensor on the CPU} of one batch in one mode"""
    eng.set_streaming(inp["chunk"])
    try:
        args = call_args(inp, mode)
        out = {tap: eng.flow_estimator_tap(*args, tap) for tap in taps}
        torch.cuda.synchronize()
    finally:
        eng.set_streaming(0)
    return {k: v.cpu() for k, v in out.items()}


def run(route, mode, case, monkeypatch):
    key = (route, mode, case)
    if key not in _RUNS:
        _RUNS[key] = tapped(engine_of(route, monkeypatch), es.inputs(case), mode)
    return _RUNS[key]


def report_of(route, mode, case, monkeypatch):
    """the profiler's report of the launches up to the D tap"""
    eng, inp = engine_of(route, monkeypatch), es.inputs(case)
    eng.set_streaming(inp["chunk"])
    try:
        args = call_args(inp, mode)
        return pu.profiled(lambda: eng.flow_estimator_tap(*args, "D"))
    finally:
        eng.set_streaming(0)


def launches(report, prefix, suffix=">"):
    return sum(v["launches"] for k, v in report.items() if k.startswith(prefix) and k.endswith(suffix))


def assert_route(route, mode, case, report):
    """the launches say which route the call took"""
    names = sorted(report)
    rt = ROUTES[route][0].get("JV_ROWGEMM_RT")
    if rt is None:
        assert not any(k.startswith(("rowgemm_", "rowblock_", "rowconv_", "rowres_", "rowffn_")) for k in names), names
        assert ("splitk_reduce" in report) == (route != "tiles_x6"), names
        has_h3 = any("_h3<" in k for k in names)
        assert has_h3 == (not ROUTES[route][1]), names
        return
    tile = f"<{16 * int(rt)}x256"
    assert "splitk_reduce" not in report and any(k.startswith("rowblock_h3" + tile) for k in names), names
    ln, riding = launches(report, "rowblock_h3<", ",ln>"), launches(report, "rowblock_h3<", ",qkv>")
    if route.startswith("rows"):      # the blocks hand their LayerNorm planes to a q | k | v launch of 80-row tiles
        assert ln > 0 and riding == 0 and "rowgemm_h3<80x256,qkv>" in report, names
    else:
        assert ln == 0 and riding > 0, names
    res_one = launches(report, "rowres_h3" + tile)
    if mode == "step":
        # the whole-resnet launch in the twelve mid stages and the up stage: an even number of alternations between w.h and w.h2,
        # so the trunk is back in w.h (Est::run refuses to go on otherwise, and RESi is read from the buffer the stage wrote)
        assert res_one == 13, (res_one, names)
        assert (launches(report, "rowres_h3" + tile, ",qkv>") == 13) == route.startswith("ride"), names
    else:
        assert res_one == 0, names      # the entry makes the time embedding per sample: no whole-resnet launch


def references(case, mode, tap, got, geo):
    """(fp64 reference, fp32 floor) of a stage from the previous taps of a run; runs of one case whose sources hold the same bits
    share one evaluation"""
    src = {n: got[n] for n in es.sources_of(tap) if n != "in"}
    for s, refs in _REFS.setdefault((case, mode, tap), []):
        if all(torch.equal(s[n], src[n]) for n in src):
            return refs
    with torch.inference_mode():
        refs = tuple(es.evaluate(tap, es.weights(), dict(src, **{"in": es.inputs(case)}), geo, dt).double()
                     for dt in (torch.float64, torch.float32))
    _REFS[(case, mode, tap)].append((src, refs))
    return refs


def worst_row(rows, a):
    return int(((rows - a).abs().amax(dim=1) / a.abs().amax(dim=1).clamp_min(1e-30)).argmax())


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,mode,case", RUNS)
def test_stage_parity(route, mode, case, monkeypatch):
    """1. every stage of every live sample against the fp64 reference of its stage, on the route the profiler confirms"""
    got, geo = run(route, mode, case, monkeypatch), es.geometry(es.inputs(case), mode)
    assert_route(route, mode, case, report_of(route, mode, case, monkeypatch))
    failures, figures = [], {}
    for tap in es.TAPS:
        r64, r32 = references(case, mode, tap, got, geo)
        assert tuple(got[tap].shape) == tuple(r64.shape) == es.shape_of(tap, geo), (case, tap, got[tap].shape, r64.shape)
        where = f"{route}/{mode}/{case} {tap}"
        if es.moves_data(tap):
            if not torch.equal(got[tap].double(), r64):
                failures.append(f"{where}: only moves data and differs by {pu.md(got[tap], r64):.3e}")
            continue
        if tap in es.TIME_TAPS:
            blocks = [(-1, got[tap].double(), r64, r32)]
        else:
            blocks = [(b, es.rows_of(got[tap], b, L).double(), es.rows_of(r64, b, L), es.rows_of(r32, b, L))
                      for b, L in enumerate(geo["L"]) if L > 0]
        for b, rows, a, f in blocks:
            kd, fl = fo.distances(rows, a, f, slice(None))
            ratio = kd / fl if fl > 0 else float("inf")
            if ratio >= figures.get(tap, dict(ratio=-1.0))["ratio"]:
                figures[tap] = dict(ratio=ratio, floor=fl, sample=b, worst_row=worst_row(rows, a))
            if not (fl > 0.0 and math.isfinite(kd) and kd <= es.ratio_of(tap) * fl):
                failures.append(f"{where} sample {b} ({rows.shape[0]} rows): row {worst_row(rows, a)}: kernel {kd:.3e} = "
                                f"{kd / max(fl, 1e-300):.2f} x floor {fl:.3e}")
    summarise(f"{route}/{mode}/{case}", figures)
    assert not failures, failures


def summarise(key, figures):
    """the run's figures as one entry, and over everything measured so far the worst ratio at the plain bound and behind a long
    contraction"""
    record.table(key, figures)
    worst, n = {}, 0
    for k, rows in record.doc["measured"].items():
        for tap, (ratio, _, _, _) in rows.items():
            n += 1
            group = "long contraction" if tap in es.LONG_K else "plain bound"
            if ratio > worst.get(group, {"ratio": -1.0})["ratio"]:
                worst[group] = {"where": f"{k}/{tap}", "ratio": ratio}
    record.doc["summary"] = {"worst": worst, "figures": n}
    record.write()


def packed(t, geo, C):
    """(rows [4 + S (T + 4), C] of a row tap in the estimator's uniform geometry, its row mask, [(first row, live rows)])"""
    S = geo["T"] + 4
    A = torch.zeros(4 + geo["S"] * S, C)
    mask = torch.zeros(A.shape[0], dtype=torch.uint8)
    for b, L in enumerate(geo["L"]):
        A[4 + b * S:4 + b * S + L] = es.rows_of(t, b, L)
        mask[4 + b * S:4 + b * S + L] = 1
    return A, mask, [(4 + b * S, L) for b, L in enumerate(geo["L"])]


def test_long_contraction_alone(monkeypatch):
    """1b. RES13's margin rests on its first contraction, K = 3 x 512 over cat[BLK12_3, BLK0_3]: the resnet is conv_gemm's arithmetic
    and nothing else.  jv_op_conv_gemm alone (the bf16x6 loop, the same K, LayerNorm, Mish and row mask) on the run's own source taps,
    three calls chained as the tile route chains them -- block1 (+ the stage's slice of the TEMB tap), res_conv, block2 + residual --
    returns the bits of the RES13 tap (exact-range mode above 2048 rows: the tile kernels without split-K)"""
    from jyutvoice_amd.engine import op_conv_gemm
    monkeypatch.setenv("JV_OP_X6", "1")
    monkeypatch.delenv("JV_NO_X6", raising=False)
    got, geo = run("tiles_x6", "entry", "big260", monkeypatch), es.geometry(es.inputs("big260"), "entry")
    sd, pre = es.weights()[torch.float32], es.stage_prefix(es.NRES - 1) + "0."
    A, mask, at = packed(torch.cat([got["BLK12_3"], got["BLK0_3"]], dim=1), geo, 512)
    flat = lambda w: w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous().cuda()      # [Cout, k Cin] tap-major
    ln = lambda p: (sd[p + "block.2.weight"].cuda(), sd[p + "block.2.bias"].cuda())
    kw = dict(M=A.shape[0], rowmask=mask.cuda())
    h = op_conv_gemm(A.cuda(), flat(sd[pre + "block1.block.0.weight"]), sd[pre + "block1.block.0.bias"].cuda(), ntaps=3, tap_row0=-2,
                     act="mish", ln=ln(pre + "block1."), **kw)
    temb = torch.zeros(A.shape[0], 256)
    for b, (row0, L) in enumerate(at):
        temb[row0:row0 + L] = got["TEMB"][b, 256 * (es.NRES - 1):]
    h = h + temb.cuda()      # one fp32 addition per element, as the epilogue's
    res = op_conv_gemm(A.cuda(), flat(sd[pre + "res_conv.weight"]), sd[pre + "res_conv.bias"].cuda(), **kw)
    out = op_conv_gemm(h, flat(sd[pre + "block2.block.0.weight"]), sd[pre + "block2.block.0.bias"].cuda(), ntaps=3, tap_row0=-2,
                       act="mish", ln=ln(pre + "block2."), res=res, **kw).cpu()
    for b, (row0, L) in enumerate(at):
        alone, tap = out[row0:row0 + L], es.rows_of(got["RES13"], b, L)
        assert torch.equal(alone, tap), (b, pu.md(alone, tap))


@pytest.mark.parametrize("case", ["ragged37", "mags"])
def test_modes_share_everything_ahead_of_the_first_attention(case, monkeypatch):
    """2. where the two modes coincide -- the entry handed the step's 2 B samples and the step's t for every sample -- the time taps
    (every row of the entry's is the step's one row), XIN and RES0 hold the same bits; and so does everything behind them on the
    split-K route, whose launches are the same in both modes"""
    eng = engine_of("sk", monkeypatch)
    step = run("sk", "step", case, monkeypatch)
    entry = tapped(eng, es.step_as_entry(es.inputs(case)), "entry")
    for tap in es.TAPS:
        want = step[tap].expand_as(entry[tap]) if tap in es.TIME_TAPS else step[tap]
        assert torch.equal(entry[tap], want), (case, tap, pu.md(entry[tap], want))


@pytest.mark.parametrize("route,mode,case", [("sk", "entry", "ragged37"), ("sk", "step", "mags"), ("rows2", "entry", "mags"),
                                             ("rows5", "step", "ragged37"), ("ride2", "step", "mags"), ("ride5", "entry", "seam"),
                                             ("sk", "entry", "chunk")])
def test_samples_do_not_see_their_batch(route, mode, case, monkeypatch):
    """3. every tap of each utterance equals the same utterance run alone at the same width, bit for bit (step: the utterance and
    its twin; a ragged batch there is compact and the utterance alone uniform)"""
    got, inp = run(route, mode, case, monkeypatch), es.inputs(case)
    eng = engine_of(route, monkeypatch)
    for i in range(inp["B"]):
        alone = tapped(eng, es.only(inp, i), mode)
        for k in es.TAPS:
            if k in es.TIME_TAPS:
                whole = got[k] if mode == "step" else got[k][i:i + 1]
            else:
                whole = got[k][i:i + 1] if mode == "entry" else torch.cat([got[k][i:i + 1], got[k][inp["B"] + i:inp["B"] + i + 1]])
            assert torch.equal(whole, alone[k]), (route, mode, case, i, k, pu.md(whole, alone[k]))


@pytest.mark.parametrize("case", ["ragged37", "dead", "mags"])
def test_compact_equals_uniform(case, monkeypatch):
    """4. the step mode lays a ragged batch out compactly exactly where a solve does (the launches account for the clamped lengths'
    sum, against B T under JV_NO_COMPACT=1), and every tap holds the same bits in both geometries"""
    compact, uniform = run("ride2", "step", case, monkeypatch), run("ride2_uniform", "step", case, monkeypatch)
    inp = es.inputs(case)
    lens2 = inp["lens"].tolist() * 2
    pu.assert_compact_taken(report_of("ride2", "step", case, monkeypatch), report_of("ride2_uniform", "step", case, monkeypatch),
                            lens2, inp["T"], "rowblock_h3<")
    for k in es.TAPS:
        assert torch.equal(compact[k], uniform[k]), (case, k, pu.md(compact[k], uniform[k]))


@pytest.mark.parametrize("family", ["rows", "ride"])
@pytest.mark.parametrize("mode,case", [("entry", "seam"), ("step", "seam"), ("step", "ragged37")])
def test_tile_heights_agree(family, mode, case, monkeypatch):
    """5. every tap is bit-equal across the forced tile heights 2 .. 5 (an utterance's bits depend on neither the tile
    height nor its position in a tile), with q | k | v in its own launch and riding"""
    base = run(family + "2", mode, case, monkeypatch)
    for rt in "345":
        other = run(family + rt, mode, case, monkeypatch)
        for k in es.TAPS:
            assert torch.equal(base[k], other[k]), (family, rt, mode, case, k, pu.md(base[k], other[k]))


@pytest.mark.parametrize("route,mode,case", RUNS)
def test_zeros_behind_the_lengths(route, mode, case, monkeypatch):
    """6a. positions at and behind a clamped length, and a dead sample, are exactly zero in every row tap; every tap is finite,
    nonzero where live, and of the declared shape and id"""
    from jyutvoice_amd._lib import EST_TAPS
    got, geo = run(route, mode, case, monkeypatch), es.geometry(es.inputs(case), mode)
    for k in es.TAPS:
        assert torch.isfinite(got[k]).all(), (case, k)
        assert tuple(got[k].shape) == es.shape_of(k, geo), (case, k, got[k].shape)
        assert EST_TAPS[k] == (es.TAPS.index(k), es.channels_of(k)), k
        if k in es.TIME_TAPS:
            assert float(got[k].abs().amax(dim=1).min()) > 0.0, (case, k)
            continue
        for b, L in enumerate(geo["L"]):
            tail = got[k][b, :, L:]
            assert float(tail.abs().max() if tail.numel() else 0.0) == 0.0, (case, b, k)
            if L > 0:      # (a tap that copied nothing would pass the line above)
                assert float(got[k][b, :, :L].abs().amax(dim=0).min()) > 0.0, (case, b, k)


@pytest.mark.parametrize("route", ["sk", "rows2", "ride5"])
def test_stale_workspace_is_not_read(route, monkeypatch):
    """6b. t1 behind seam on one context equals t1 on a context that ran nothing else, in both modes: the gap rows, and what seam left
    in w.ln / w.qkv / w.cat / w.h2 behind t1's rows, are not read"""
    eng = make_engine(route, monkeypatch)
    try:
        fresh = {m: tapped(eng, es.inputs("t1"), m) for m in ("entry", "step")}
    finally:
        eng.close()
    eng = make_engine(route, monkeypatch)
    try:
        for m in ("entry", "step"):
            tapped(eng, es.inputs("seam"), m, ("D",))
            again = tapped(eng, es.inputs("t1"), m)
            for k in es.TAPS:
                assert torch.equal(fresh[m][k], again[k]), (route, m, k, pu.md(fresh[m][k], again[k]))
    finally:
        eng.close()


@pytest.mark.parametrize("route", ["sk", "ride2"])
def test_the_tap_changes_nothing(route, monkeypatch):
    """7. the D tap is the untapped entry's output; flow_estimator and a 2-step cfm_solve return the same bits behind a sweep of
    tapped calls as ahead of it; a tap twice gives the same bits; an unknown tap or mode and an output buffer that is too small are
    errors that leave `out` untouched"""
    from jyutvoice_amd._lib import EST_TAPS, JvError
    assert tuple(sorted(EST_TAPS, key=lambda k: EST_TAPS[k][0])) == es.TAPS and [EST_TAPS[k][0] for k in es.TAPS] == list(range(79))
    eng, inp = engine_of(route, monkeypatch), es.inputs("ragged37")
    dev = lambda v: v.cuda()
    entry = lambda: eng.flow_estimator(dev(inp["x"]), dev(inp["lens"]), dev(inp["mu"]), dev(inp["t"]), dev(inp["spks"]), dev(inp["cond"])).cpu()
    solve = lambda: eng.cfm_solve(dev(inp["mu"]), dev(inp["lens"]), dev(inp["spks"]), dev(inp["cond"]), 2).cpu()
    before = entry(), solve()
    for mode in ("entry", "step"):
        first = tapped(eng, inp, mode)
        args = call_args(inp, mode)
        for tap in reversed(es.TAPS):
            assert torch.equal(eng.flow_estimator_tap(*args, tap).cpu(), first[tap]), (mode, tap)
        for tap in es.TAPS:
            assert torch.equal(first[tap], run(route, mode, "ragged37", monkeypatch)[tap]), (mode, tap)
    after = entry(), solve()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert torch.equal(before[0], run(route, "entry", "ragged37", monkeypatch)["D"])
    args = call_args(inp, "entry")
    for mode, tap in (("entry", "BLK3_1"), ("step", "XIN"), ("step", "TEMB"), ("entry", "T1")):
        a = call_args(inp, mode)
        small = torch.full((run(route, mode, "ragged37", monkeypatch)[tap].numel() - 1,), 7.0, device="cuda:0")
        with pytest.raises(JvError) as err:
            eng.flow_estimator_tap(*a, tap, out=small)
        assert err.value.code == 4, tap      # JV_ERR_SHAPE
        assert float((small - 7.0).abs().max()) == 0.0, tap      # rejected ahead of the first launch
    out = torch.full((6 * 320 * 37,), 7.0, device="cuda:0")
    for bad in (-1, 79):
        for mode in ("entry", "step"):
            with pytest.raises(JvError) as err:
                eng.flow_estimator_tap(mode, *args[1:], bad, out=out)
            assert err.value.code == 1      # JV_ERR_ARG
    with pytest.raises(JvError) as err:
        eng.flow_estimator_tap(2, *args[1:], "D", out=out)      # no such mode
    assert err.value.code == 1
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0
    assert torch.equal(before[0], entry())
