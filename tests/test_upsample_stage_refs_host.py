"""CPU: the stage references of tests/upsample_stage_ref.py, without a GPU.

(a) They are the model: the fp64 chain of the per-stage formulas equals oracle.prompt.flow_encoder(dtype=float64) to 1e-10 on every
    case of test_gpu_upsample_stages.py, both streaming values (table="oracle": the oracle's fp64 run multiplies by fp32-rounded
    sin / cos; the references' default table takes them in fp64 of the same fp32 angle, and the two differ by no more than that one
    rounding -- asserted here).  The context path has no oracle: there the chain is held to the committed fixture G15_flow_partial's
    `h` (recorded from the imported reference modules in fp32), at that fixture's fp32 accuracy -- the larger of the fp32 chain's own
    distance to it and the standing 5e-5 -- and the per-utterance context mode (wider tables, the same stages) to the same chain at 1e-10.
(b) They can tell: each plausible mistake, applied to the fp32 evaluation of ONE stage fed the same fp32 taps, lands more than
    the bound (upsample_stage_ref.ratio_of x the fp32 floor: 8 x, behind the long contractions 8 x sqrt(K / 1024)) from the fp64 stage
    on at least one utterance of the short cases -- the bound test_gpu_upsample_stages.py holds the kernels to.  Rows behind a
    length are compared too (the reference is zero there: a stage that is not masked shows).
(c) The conditions the cases are built on hold on the fp64 reference alone: every compared stage has a floor > 0 on every live
    utterance (the data-moving ones exactly zero), every streaming case has a query whose chunk mask removes a live key in each stage,
    and every context case's C1 differs from the zero-padded C1 by far more than the bound."""
import pytest
import torch

import test_gpu_fused_ops as fo      # distances / RATIO (a module object: none of its tests is collected here)
import upsample_stage_ref as us
from conftest import load_golden

assert us.RATIO == fo.RATIO
ORACLE_CASES = tuple(k for k in us.CASES if "ctx" not in us.CASES[k])
SHORT_RUNS = tuple(r for r in us.RUNS if r[0] != "long300")


@pytest.fixture(scope="module", autouse=True)
def threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


@pytest.mark.parametrize("streaming", [False, True])
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_references_are_the_oracle(name, streaming):
    from oracle import prompt as oprompt
    inp = us.inputs(name)
    geo = us.geometry(inp, "flow", streaming)
    got = us.chain(inp, geo, table="oracle")
    ids = torch.zeros(geo["B"], geo["W"], dtype=torch.int64)
    for b, v in enumerate(inp["ids"]):
        ids[b, :len(v)] = v
    with torch.inference_mode():
        h, _ = oprompt.flow_encoder(us.weights()[torch.float64], ids, torch.tensor(geo["L"]), streaming=streaming, dtype=torch.float64)
    assert got["H"].shape == (geo["B"], 80, 2 * geo["W"])
    assert float((got["H"].transpose(1, 2) - h).abs().max()) <= 1e-10
    # the default table: sin / cos of the same fp32 angle, not rounded to fp32 -- one rounding (2^-24) of numbers of at most 1
    for pe in ("PE1", "PE2"):
        exact = us.evaluate(pe, us.weights(), got, geo, torch.float64)
        assert float((exact - got[pe]).abs().max()) <= 2.0 ** -24
    for stage in us.TAPS:
        assert tuple(got[stage].shape) == us.shape_of(stage, geo), stage


@pytest.mark.parametrize("tag,streaming", [("full", False), ("stream", True)])
def test_context_chain_is_the_fixture(tag, streaming):
    """G15: m = 40 tokens (P = 7), the last three context only, L = 37"""
    g = load_golden("G15_flow_partial")
    want = g["h_" + tag].double()
    inp = us.make_inputs(g["prompt_token"], torch.tensor([7]), g["token"], torch.tensor([33]), ctx=[3])
    geo = us.geometry(inp, "partial", streaming)
    assert geo["L"] == [37] and geo["T"] == 37 and geo["W"] == 40
    h64 = us.chain(inp, geo, table="oracle")["H"]
    h32 = us.chain(inp, geo, torch.float32, table="oracle")["H"].double()
    assert float(h64[:, :, 74:].abs().max()) == 0.0
    own = float((h32[:, :, :74].transpose(1, 2) - want).abs().max())      # two fp32 evaluations of one model
    err = float((h64[:, :, :74].transpose(1, 2) - want).abs().max())
    print(f"G15 {tag}: fp64 chain - fixture {err:.3e}, fp32 chain - fixture {own:.3e}")
    assert err <= max(own, 5e-5), (err, own)
    # the per-utterance mode at the whole width computes the same stages (its tables are wider: T = 40)
    geo_c = us.geometry(inp, "ctx", streaming)
    assert geo_c["L"] == [37] and geo_c["T"] == 40
    hc = us.chain(inp, geo_c, table="oracle")["H"]
    assert float((hc - h64).abs().max()) <= 1e-10


# mistake -> the stages it is applied to
# LayerNorm eps.  1e-4 (the text encoder's) in place of 1e-5 moves a row by 4.5e-5 / variance of its input: visible at E0, whose
# input (embed.out.0) has a variance of 2e-3 to 3e-3.  Every other LayerNorm reads rows of variance 120 to 940 (they descend from an
# embedding x sqrt 512; measured on lanes65), where that mistake is 5e-8 to 4e-7 of the row -- at or under the fp32 floor, so no
# fp32 comparison can see it; there the mistake shown is an eps of 1e-1 ("ln_eps_big").
# c2_ctx (conv2 and its residual take the context rows for live ones) shows ONLY in rows behind a length: conv2 is causal, so a
# context row, which lies behind the last encoded one, cannot reach a live row of LA.  The GPU parity test compares live rows and
# a tap writes zeros behind them, so such a leak is not observable through the taps -- and is harmless: those rows are masked as
# keys and as inputs of the up-convolution.  It stays in the list as the issue names it; the GPU file claims no coverage of it.
MUTANTS = ([("ln_eps", "E0")] + [("ln_eps_big", t) for t in ("LN1_0", "LN2_3", "U0", "LN1_u0", "LN2_u3", "AN")]
           + [("ln_unbiased", t) for t in ("E0", "LN2_0", "U0", "LN1_u2", "AN")]
           + [("no_sqrt", "E0"), ("no_sqrt", "U0"), ("lrelu_slope", "LA"), ("c1_zero_ctx", "C1"), ("c2_ctx", "LA")]
           + [("tap_off", t) for t in ("C1", "LA", "UP")] + [("up_cross", "UP"), ("rep_round", "REP")]
           + [(m, t) for m in ("rel_shift_off", "uv_swap", "scale_512", "chunk_line") for t in ("ATT_0", "ATT_u0", "ATT_u3")]
           + [("chunk_25", "ATT_u0"), ("chunk_25", "ATT_u2"), ("keys_L", "ATT_u0"), ("keys_L", "ATT_u3")]
           + [("silu_sigmoid", "FF_0"), ("silu_sigmoid", "FF_u1")]
           + [("no_residual", t) for t in ("LA", "X1_0", "X2_0", "X1_u1", "X2_u3")]
           + [(m, t) for m in ("angle_fp64", "sincos_swap") for t in ("PE1", "PE2")] + [("table_half", "PE2")])


def blocks(stage, geo, t):
    """[(utterance or None, rows [n, C] over EVERY position of it)] of a stage: the tables are one block"""
    if us.is_table(stage):
        return [(None, t)]
    return [(b, us.rows_of(t, b, t.shape[2])) for b, L in enumerate(geo["L"]) if L > 0]


@pytest.mark.parametrize("mut,tap", MUTANTS)
def test_reference_catches(mut, tap):
    seen = {}
    for name, mode, streaming in SHORT_RUNS:
        inp, ws, ref = us.inputs(name), us.weights(), us.tap_chain(name, mode, streaming)
        geo = us.geometry(inp, mode, streaming)
        r64 = us.evaluate(tap, ws, ref, geo, torch.float64)
        r32 = us.evaluate(tap, ws, ref, geo, torch.float32).double()
        bad = us.evaluate(tap, ws, ref, geo, torch.float32, mut).double()
        for (b, a), (_, f), (_, m) in zip(blocks(tap, geo, r64), blocks(tap, geo, r32), blocks(tap, geo, bad)):
            md, fl = fo.distances(m, a, f, slice(None))
            assert fl > 0.0 or us.moves_data(tap, geo, b), (name, mode, b)
            bound = us.ratio_of(tap) * fl      # (the GPU file's, margins included; a data-moving stage: any difference)
            seen[(name, mode, streaming, b)] = (md, bound)
            if md > bound:
                return
    assert False, (mut, tap, seen)


@pytest.mark.parametrize("name,mode,streaming", us.RUNS)
def test_case_conditions(name, mode, streaming):
    inp, ws, ref = us.inputs(name), us.weights(), us.tap_chain(name, mode, streaming)
    geo = us.geometry(inp, mode, streaming)
    if streaming:      # a query of the first chunk with a live key behind the chunk line, at both rates
        assert max(geo["L"]) > us.CHUNK and 2 * max(geo["L"]) > 2 * us.CHUNK, geo["L"]
        for att in ("ATT_0", "ATT_u0"):
            free = us.evaluate(att, ws, ref, dict(geo, streaming=False), torch.float64)
            assert float((free - us.evaluate(att, ws, ref, geo, torch.float64)).abs().max()) > 1e-3, att
    for stage in us.compared(name):
        r64 = us.evaluate(stage, ws, ref, geo, torch.float64)
        r32 = us.evaluate(stage, ws, ref, geo, torch.float32).double()
        assert tuple(r64.shape) == us.shape_of(stage, geo), stage
        assert torch.isfinite(r64).all() and torch.isfinite(r32).all(), stage
        if us.is_table(stage):
            _, fl = fo.distances(r64, r64, r32, slice(None))
            assert (fl == 0.0 and torch.equal(r64, r32)) if us.moves_data(stage, geo) else fl > 0.0, stage
            continue
        for b, L in enumerate(geo["L"]):
            n = us.live(stage, geo, b)
            tail = r64[b, :, n:]
            assert float(tail.abs().max() if tail.numel() else 0.0) == 0.0, (stage, b)
            if L == 0:
                assert float(r64[b].abs().max()) == 0.0, (stage, b)      # the dead utterance: zeros everywhere
                continue
            a, f = us.rows_of(r64, b, n), us.rows_of(r32, b, n)
            assert float(a.abs().amax(dim=1).min()) >= 1e-20, (stage, b)
            _, fl = fo.distances(a, a, f, slice(None))
            if us.moves_data(stage, geo, b):
                assert fl == 0.0 and torch.equal(a, f), (stage, b)
            else:
                assert fl > 0.0, (stage, b)
    if any(geo["ctx"]):      # the context is not a detail: zero padding in its place lands far outside the bound
        r64 = us.evaluate("C1", ws, ref, geo, torch.float64)
        r32 = us.evaluate("C1", ws, ref, geo, torch.float32).double()
        zero = us.evaluate("C1", ws, ref, geo, torch.float64, "c1_zero_ctx")
        for b, c in enumerate(geo["ctx"]):
            if c:
                n = us.live("C1", geo, b)
                md, fl = fo.distances(us.rows_of(zero, b, n), us.rows_of(r64, b, n), us.rows_of(r32, b, n), slice(None))
                assert md > 1000.0 * us.ratio_of("C1") * fl, (b, md, fl)
        # and the one-token attention of part4 / ctxmix is its value row
    for b, L in enumerate(geo["L"]):
        if L == 1:
            assert torch.equal(us.rows_of(ref["ATT_0"], b, 1), us.rows_of(ref["QKV_0"], b, 1)[:, 1024:]), b
