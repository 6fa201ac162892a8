"""GPU: every stage of the up-sampling conformer encoder (prompt.hip encoder_stages), read through jv_upsample_encoder_tap in each
of its four entry modes -- the embedding, Linear + LayerNorm x sqrt 512 and the device-built position table, the two look-ahead
convolutions, per block both LayerNorms, q | k | v, linear_pos of the table, the attention, both residual sums and the feed-forward's
hidden rows, then nearest x 2, the k5 convolution, the second embed and table, four more blocks, after_norm and the projection --
each held to the plain fp64 reference of ITS OWN operation (tests/upsample_stage_ref.py) evaluated on the GPU's own previous taps, so
that an error is charged to the stage that made it and the failure names the case, the mode, the utterance, the stage and the row.

The bound is test_gpu_fused_ops.py's (fo.distances, RATIO = 8): the worst row of |kernel - fp64| over that row's own fp64 magnitude
may be 8 x the same figure of the fp32 evaluation of the same formula on the CPU, and that floor must be > 0.  A row is one
position's channel vector of one utterance, over its live positions; a table is one block of 2T - 1 rows.  C1, UP and X2 are read
straight behind contractions of K = 2048 / 2560 / 2048 products and take the project's rule for those, 8 x sqrt(K / 1024)
(upsample_stage_ref.LONG_K), which test_long_contraction_alone grounds for C1, UP and the X2 of every block: jv_op_conv_gemm alone
on the run's own source tap returns the stage's bits.  Stages that only move data have a floor of zero and are held torch.equal: EMB, REP, the token-rate attention of a
one-token utterance (softmax over one key is 1: att = v) and the one-row table of T = 1.  Every figure goes to
parity_upsample_stages.json (committed under profiles/).

The cases (upsample_stage_ref.CASES) are the smallest at which these kernels can go wrong; test_upsample_stage_refs_host.py asserts
their conditions on the fp64 reference alone and shows that the bound catches each of a list of deliberate mistakes on them."""
import functools
import math

import pytest
import torch

import parity_util as pu
import test_gpu_fused_ops as fo      # distances / RATIO (a module object: none of its tests is collected here)
import upsample_stage_ref as us

pytestmark = pytest.mark.gpu

assert us.RATIO == fo.RATIO
record = pu.Recorder("parity_upsample_stages.json", {
    "what": "per case / mode / utterance (or table) / stage: worst row of |kernel - fp64| / max |fp64 row| (kernel), of the same formula "
            "in fp32 torch on the CPU (floor), and their ratio; the reference of a stage is evaluated on the GPU's own previous taps",
    "bound": "kernel <= 8 x floor, floor > 0; data-moving stages (EMB, REP, token-rate attention of a one-token utterance, the table "
             "of T = 1): torch.equal",
    "margins": {k: f"8 x sqrt({v} / 1024) = {us.ratio_of(k):.1f} x floor: read straight behind a contraction of K = {v} products in one "
                   "fp32 chain inside the MFMAs, whose rounding error grows as sqrt(K); 8 x was established up to K = 1024 "
                   "(upsample_stage_ref.LONG_K; test_long_contraction_alone)" for k, v in us.LONG_K.items()},
    "rows": "one position's channel vector; a table: one relative position",
    "layout": "measured[case/mode/utterance or table][stage] = [ratio, floor, worst row]; kernel = ratio x floor",
    "cases": {k: {"P": v["P"], "N": v["N"], "plens": list(v.get("plens", ())), "tlens": list(v["tlens"]), "ctx": list(v.get("ctx", ()))}
              for k, v in us.CASES.items()}}, columns=("ratio", "floor", "worst_row"))

_STATE = {}


def make_engine():
    """one context for every case: 3 utterances, 2 x 300 mel-rate rows (the prompt workspace is sized by the calls themselves)"""
    from jyutvoice_amd.engine import JV_MODEL_PROMPT, Engine
    from jyutvoice_amd.flow.encoder import DIV_TERM_KEY
    e = Engine("cuda:0", max_batch=3, max_frames=640, max_tokens=16)
    e.load_state_dict(JV_MODEL_PROMPT, dict(us.checkpoint(), **{DIV_TERM_KEY: us.div_term()}))
    return e


@pytest.fixture(scope="module", autouse=True)
def engine():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    _STATE["engine"] = make_engine()
    yield _STATE["engine"]
    run.cache_clear()
    references.cache_clear()
    _STATE.pop("engine").close()


def tap_args(inp, mode):
    kw = {"ctx_lens": torch.tensor(inp["ctx"], dtype=torch.int32)} if mode == "ctx" else {}
    return (mode, inp["ptok"], inp["plen"], inp["tok"], inp["tlen"]), kw


def tapped(eng, inp, mode, streaming, taps=us.TAPS):
    """{tap: its tensor on the CPU} of one batch in one mode"""
    args, kw = tap_args(inp, mode)
    out = {tap: eng.upsample_encoder_tap(*args, tap, streaming=streaming, **kw).cpu() for tap in taps}
    torch.cuda.synchronize()
    return out


def entry(eng, inp, mode, streaming):
    """the untapped entry's h as the H tap lays it out: [B, 80, 2 W], zeros behind what the entry returns"""
    if mode == "prompt":
        h = eng.prompt_encoder(inp["tok"], inp["tlen"])
    elif mode == "flow":
        h, _ = eng.flow_encoder(inp["ptok"], inp["plen"], inp["tok"], inp["tlen"], streaming=streaming)
    elif mode == "partial":
        h, _ = eng.flow_encoder_partial(inp["ptok"], inp["plen"], inp["tok"], inp["tlen"], streaming=streaming)
    else:
        h, _ = eng.flow_encoder_ctx(inp["ptok"], inp["plen"], inp["tok"], inp["tlen"], torch.tensor(inp["ctx"], dtype=torch.int32),
                                    streaming=streaming)
    h = h.cpu().transpose(1, 2)
    return torch.nn.functional.pad(h, (0, 2 * (inp["P"] + inp["N"]) - h.shape[2]))


@functools.lru_cache(maxsize=None)
def run(case, mode, streaming):
    return tapped(_STATE["engine"], us.inputs(case), mode, streaming, us.stages_of(case))


def geo_of(case, mode, streaming):
    return us.geometry(us.inputs(case), mode, streaming)


_REFS = {}      # (case, stage) -> [(geometry that matters, sources, (fp64, fp32))]: runs whose sources hold the same bits share


@functools.lru_cache(maxsize=None)
def references(case, mode, streaming, stage):
    """(fp64 reference, fp32 floor) of a stage from the previous taps of a run; runs of one case whose sources hold the same bits
    (the modes ahead of the first attention, the streaming values outside the attentions) share one evaluation"""
    got, geo = run(case, mode, streaming), geo_of(case, mode, streaming)
    src = {n: got[n] for n in us.sources_of(stage) if n != "in"}
    key = (geo["T"], tuple(geo["L"]), tuple(geo["ctx"]), geo["streaming"] if us.kind_of(stage) == "ATT" else None)
    for k, s, refs in _REFS.setdefault((case, stage), []):
        if k == key and all(torch.equal(s[n], src[n]) for n in src):
            return refs
    refs = tuple(us.evaluate(stage, us.weights(), dict(src, **{"in": us.inputs(case)}), geo, dt).double()
                 for dt in (torch.float64, torch.float32))
    _REFS[(case, stage)].append((key, src, refs))
    return refs


def tag(mode, streaming):
    return mode + ("+stream" if streaming else "")


def worst_row(rows, a):
    return int(((rows - a).abs().amax(dim=1) / a.abs().amax(dim=1).clamp_min(1e-30)).argmax())


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode,streaming", us.RUNS)
def test_stage_parity(case, mode, streaming):
    """1. every stage of every live utterance, and every table, against the fp64 reference of its stage"""
    got, geo = run(case, mode, streaming), geo_of(case, mode, streaming)
    failures, figures = [], {}
    for stage in us.compared(case):
        r64, r32 = references(case, mode, streaming, stage)
        assert tuple(got[stage].shape) == tuple(r64.shape) == us.shape_of(stage, geo), (case, stage, got[stage].shape, r64.shape)
        if us.is_table(stage):
            blocks = [(None, got[stage].double(), r64, r32)]
        else:
            blocks = [(b, us.rows_of(got[stage], b, n).double(), us.rows_of(r64, b, n), us.rows_of(r32, b, n))
                      for b, n in ((b, us.live(stage, geo, b)) for b, L in enumerate(geo["L"]) if L > 0)]
        for b, rows, a, f in blocks:
            who = "table" if b is None else f"utt{b}"
            where = f"{case}/{tag(mode, streaming)} {who} ({'' if b is None else geo['L'][b]} tokens) {stage}"
            if us.moves_data(stage, geo, b):
                if not torch.equal(rows, a):
                    failures.append(f"{where}: only moves data and differs by {pu.md(rows, a):.3e} (row {worst_row(rows, a)})")
                continue
            kd, fl = fo.distances(rows, a, f, slice(None))
            worst = worst_row(rows, a)
            figures.setdefault(f"{case}/{tag(mode, streaming)}/{who}", {})[stage] = dict(
                ratio=kd / fl if fl > 0 else float("inf"), floor=fl, worst_row=worst)
            if not (fl > 0.0 and math.isfinite(kd) and kd <= us.ratio_of(stage) * fl):
                failures.append(f"{where}: row {worst} of {rows.shape[0]}: kernel {kd:.3e} = {kd / max(fl, 1e-300):.2f} x floor {fl:.3e}")
    summarise(figures)
    assert not failures, failures


def summarise(figures):
    """the run's figures, one entry per utterance or table, and over everything measured so far the worst ratio at the plain bound
    and behind a long contraction"""
    for key, rows in figures.items():
        record.table(key, rows)
    worst, n = {}, 0
    for key, rows in record.doc["measured"].items():
        for stage, (ratio, _, _) in rows.items():
            n += 1
            group = "long contraction" if us.kind_of(stage) in us.LONG_K else "plain bound"
            if ratio > worst.get(group, {"ratio": -1.0})["ratio"]:
                worst[group] = {"where": f"{key}/{stage}", "ratio": ratio}
    record.doc["summary"] = {"worst": worst, "figures": n}
    record.write()


def alone_conv(A, w, bias, ntaps, tap_row0, rowmask, **kw):
    from jyutvoice_amd.engine import op_conv_gemm
    W = w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous() if w.dim() == 3 else w      # [Cout, k Cin] tap-major
    return op_conv_gemm(A.cuda(), W.cuda(), bias.cuda(), ntaps=ntaps, tap_row0=tap_row0, M=A.shape[0], rowmask=rowmask.cuda(), **kw).cpu()


@pytest.mark.parametrize("case,mode,streaming", [("lanes65", "flow", False), ("part30", "partial", True), ("ctxmix", "ctx", False)])
def test_long_contraction_alone(case, mode, streaming, monkeypatch):
    """1b. C1, UP and X2 are conv_gemm's arithmetic and nothing else: jv_op_conv_gemm alone (the bf16x6 loop, the same K and row mask)
    on the rows of the run's own source tap returns the bits of the stage's tap -- the ground of their margin
    (upsample_stage_ref.LONG_K)"""
    monkeypatch.setenv("JV_OP_X6", "1")
    monkeypatch.delenv("JV_NO_X6", raising=False)
    got, geo, sd = run(case, mode, streaming), geo_of(case, mode, streaming), us.checkpoint()
    G, GAP = 8, 8      # prompt.hip: P_G leading rows, P_GAP rows behind every utterance

    def packed(stage, rate, lens):
        """(rows [G + B S, C] of a tap in the encoder's geometry, its row mask, [(first row, live rows)])"""
        S = rate * geo["T"] + GAP
        A = torch.zeros(G + geo["B"] * S, us.channels_of(stage))
        mask = torch.zeros(A.shape[0], dtype=torch.uint8)
        for b, n in enumerate(lens):
            A[G + b * S:G + b * S + n] = us.rows_of(got[stage], b, n)
            mask[G + b * S:G + b * S + n] = 1
        return A, mask, [(G + b * S, rate * L) for b, L in enumerate(geo["L"])]

    e = "encoder."
    checks = []
    A, mask, at = packed("E0", 1, [L + c for L, c in zip(geo["L"], geo["ctx"])])      # the context rows are live to conv1 alone
    checks.append(("C1", alone_conv(A, sd[e + "pre_lookahead_layer.conv1.weight"], sd[e + "pre_lookahead_layer.conv1.bias"], 4, 0, mask), at))
    A, mask, at = packed("REP", 2, [2 * L for L in geo["L"]])
    checks.append(("UP", alone_conv(A, sd[e + "up_layer.conv.weight"], sd[e + "up_layer.conv.bias"], 5, -4, mask), at))
    for sfx, pre, rate in ([(f"_{i}", e + f"encoders.{i}.", 1) for i in range(us.BLOCKS)]
                           + [(f"_u{i}", e + f"up_encoders.{i}.", 2) for i in range(us.UP_BLOCKS)]):      # every block's X2
        lens = [rate * L for L in geo["L"]]
        A, mask, at = packed("FF" + sfx, rate, lens)
        res = packed("X1" + sfx, rate, lens)[0]
        checks.append(("X2" + sfx, alone_conv(A, sd[pre + "feed_forward.w_2.weight"], sd[pre + "feed_forward.w_2.bias"], 1, 0, mask,
                                              res=res.cuda()), at))
    for stage, out, at in checks:
        for b, (row0, n) in enumerate(at):
            alone, tap = out[row0:row0 + n], us.rows_of(got[stage], b, n)
            assert torch.equal(alone, tap), (case, stage, b, pu.md(alone, tap))


AHEAD_OF_ATT0 = us.TAPS[:us.TAPS.index("ATT_0")]


@pytest.mark.parametrize("case", [c for c, v in us.CASES.items() if {("prompt", False), ("flow", False)} <= set(v["runs"])])
def test_entries_share_everything_ahead_of_the_first_attention(case):
    """2a. every tap ahead of ATT_0 is bit-equal between the prompt entry and the flow entry (P = 0, not streaming)"""
    a, f = run(case, "prompt", False), run(case, "flow", False)
    for tap in AHEAD_OF_ATT0:
        assert torch.equal(a[tap], f[tap]), (case, tap, pu.md(a[tap], f[tap]))


@pytest.mark.parametrize("case,mode", [(c, m) for c, v in us.CASES.items() for m in ("flow", "partial", "ctx")
                                       if {(m, False), (m, True)} <= set(v["runs"])])
def test_streaming_changes_only_the_attention(case, mode):
    """2b. every tap ahead of ATT_0 is bit-equal between the two streaming values; so are the tables and linear_pos of them in
    every block (chunk masks touch nothing else; what follows an attention is held by test 1 in each)"""
    a, s = run(case, mode, False), run(case, mode, True)
    for tap in us.stages_of(case):
        if tap in AHEAD_OF_ATT0 or us.is_table(tap):
            assert torch.equal(a[tap], s[tap]), (case, mode, tap, pu.md(a[tap], s[tap]))
    assert not torch.equal(a["ATT_0"], s["ATT_0"]) and not torch.equal(a["ATT_u0"], s["ATT_u0"]), (case, mode)


@pytest.mark.parametrize("case,mode,streaming", [("split37", "flow", False), ("split37", "flow", True), ("ctxmix", "ctx", False),
                                                 ("ctxmix", "ctx", True)])
def test_utterances_do_not_see_their_batch(case, mode, streaming):
    """3. every tap of each utterance equals the same utterance run alone at the same width, bit for bit"""
    got, inp = run(case, mode, streaming), us.inputs(case)
    for i in range(inp["B"]):
        alone = tapped(_STATE["engine"], us.only(inp, i), mode, streaming)
        for k in us.TAPS:
            whole = got[k] if us.is_table(k) else got[k][i:i + 1]
            assert torch.equal(whole, alone[k]), (case, mode, streaming, i, k, pu.md(whole, alone[k]))


@pytest.mark.parametrize("case,mode,streaming", us.RUNS)
def test_zeros_behind_the_lengths(case, mode, streaming):
    """4a. positions at and behind a live length, and a dead utterance, are exactly zero in every tap; every tap is finite, nonzero
    where live, and of the declared shape.  (The zeros are the tap's contract: rows_to_cf writes them itself, so this says that the
    live lengths -- L_b, 2 L_b, L_b + ctx_b for E0 -- are the right ones, not what the workspace holds behind them; that nothing
    behind a length is READ is what the stage parity, the batch independence and the stale-workspace tests show)"""
    from jyutvoice_amd._lib import UPS_TAPS
    got, geo = run(case, mode, streaming), geo_of(case, mode, streaming)
    for k in us.stages_of(case):
        assert torch.isfinite(got[k]).all(), (case, k)
        assert tuple(got[k].shape) == us.shape_of(k, geo), (case, k, got[k].shape)
        assert UPS_TAPS[k][1:] == (us.channels_of(k), us.rate_of(k)), k
        if us.is_table(k):
            assert float(got[k].abs().amax(dim=1).min()) > 0.0, (case, k)
            continue
        for b, L in enumerate(geo["L"]):
            n = us.live(k, geo, b)
            tail = got[k][b, :, n:]
            assert float(tail.abs().max() if tail.numel() else 0.0) == 0.0, (case, b, k)
            if L > 0:      # (a tap that copied nothing would pass the line above)
                assert float(got[k][b, :, :n].abs().amax(dim=0).min()) > 0.0, (case, b, k)


def test_stale_workspace_is_not_read():
    """4b. t1 and part4 behind lanes65 on one context equal the same cases on a fresh context, and the shared context's: the gap
    rows, the rows of pe / p beyond 2T - 1 and the padding of ac / bd / vt then hold the larger call's values, and none of them is
    read.  The other order: every call on the first context up to lanes65 is a flow or partial one, so its workspace holds no
    qu / qv / ac / bd / vt (prompt.hip ensure_ws, quad = false) until lanes65 arrives through the prompt entry and it regrows with
    them; t1 through the prompt entry follows on the regrown buffers and is held to a second context that ran nothing else"""
    small = (("t1", "flow", False), ("part4", "partial", False))
    t1p = ("t1", "prompt", False)
    eng = make_engine()
    try:
        fresh = {r: tapped(eng, us.inputs(r[0]), r[1], r[2]) for r in small}
        tapped(eng, us.inputs("lanes65"), "flow", False, ("H",))
        again = {r: tapped(eng, us.inputs(r[0]), r[1], r[2]) for r in small}
        regrown = tapped(eng, us.inputs("lanes65"), "prompt", False, us.stages_of("lanes65"))      # the first prompt-entry call here
        again[t1p] = tapped(eng, us.inputs("t1"), "prompt", False)
    finally:
        eng.close()
    eng = make_engine()
    try:
        fresh[t1p] = tapped(eng, us.inputs("t1"), "prompt", False)
    finally:
        eng.close()
    for r in small + (t1p,):
        for k in us.TAPS:
            assert torch.equal(fresh[r][k], again[r][k]), (r, k, pu.md(fresh[r][k], again[r][k]))
            assert torch.equal(fresh[r][k], run(*r)[k]), (r, k)
    for k in us.stages_of("lanes65"):
        assert torch.equal(regrown[k], run("lanes65", "prompt", False)[k]), (k, pu.md(regrown[k], run("lanes65", "prompt", False)[k]))


def test_the_tap_changes_nothing():
    """5. the four entries' outputs behind a sweep of tapped calls are their outputs ahead of it, and the H tap; a tap twice gives the
    same bits; an output buffer that is too small and a tap that does not exist are errors that leave `out` untouched"""
    from jyutvoice_amd._lib import UPS_TABLES, UPS_TAPS, JvError
    assert tuple(sorted(UPS_TAPS, key=lambda k: UPS_TAPS[k][0])) == us.TAPS and [UPS_TAPS[k][0] for k in us.TAPS] == list(range(93))
    assert UPS_TABLES == {k for k in us.TAPS if us.is_table(k)}
    eng = _STATE["engine"]
    runs = (("dead", "prompt", False), ("split37", "flow", True), ("part30", "partial", True), ("ctxmix", "ctx", False))
    before = {r: entry(eng, us.inputs(r[0]), r[1], r[2]) for r in runs}
    for r in runs:
        inp = us.inputs(r[0])
        first = tapped(eng, inp, r[1], r[2])
        args, kw = tap_args(inp, r[1])
        for tap in reversed(us.TAPS):
            assert torch.equal(eng.upsample_encoder_tap(*args, tap, streaming=r[2], **kw).cpu(), first[tap]), (r, tap)
        for tap in us.TAPS:
            assert torch.equal(first[tap], run(*r)[tap]), (r, tap)
    for r in runs:
        after = entry(eng, us.inputs(r[0]), r[1], r[2])
        assert torch.equal(before[r], after), r
        assert torch.equal(before[r], run(*r)["H"]), r
    inp = us.inputs("split37")
    args, kw = tap_args(inp, "flow")
    for tap in ("FF_1", "POS_u0", "E0"):
        small = torch.full((run("split37", "flow", False)[tap].numel() - 1,), 7.0, device="cuda:0")
        with pytest.raises(JvError) as err:
            eng.upsample_encoder_tap(*args, tap, out=small)
        assert err.value.code == 4, tap      # JV_ERR_SHAPE
        assert float((small - 7.0).abs().max()) == 0.0, tap      # rejected ahead of the first launch
    out = torch.full((3 * 2048 * 74,), 7.0, device="cuda:0")
    for bad in (-1, 93):
        with pytest.raises(JvError) as err:
            eng.upsample_encoder_tap(*args, bad, out=out)
        assert err.value.code == 1      # JV_ERR_ARG
    with pytest.raises(JvError) as err:
        eng.upsample_encoder_tap(4, *args[1:], "EMB", out=out)      # no such mode
    assert err.value.code == 1
    cm = us.inputs("ctxmix")      # the entry's own checks come first: a context of 2 tokens AND a short out is the entry's JV_ERR_ARG
    with pytest.raises(JvError) as err:
        eng.upsample_encoder_tap(*tap_args(cm, "ctx")[0], "EMB", ctx_lens=torch.tensor([3, 2, 3], dtype=torch.int32), out=out[:8])
    assert err.value.code == 1
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0
    assert torch.equal(before[runs[1]], entry(eng, us.inputs("split37"), "flow", True))
