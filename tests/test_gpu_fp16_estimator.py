"""GPU: the estimator's FP16 mode (jv_flow_set_precision(JV_PRECISION_FP16), Engine.set_precision("fp16")) end to end.

In the mode every contraction that runs fp16x3 by default issues its hi x hi product alone.  tests/fp16_ref.py restates the oracle's
estimator with that rounding; tests/golden/G17_fp16.npz (make_golden_fp16.py, README_fp16.md) holds the fp64 oracle's results for
the cases of fp16_ref.CASES and the distance of the emulation from them, both computed without the library:

    i    B = 1, T = 64, 57 frames               split-K tile regime              one evaluation, a 10-step solve
    ii   B = 11, T = 120, lengths 70 .. 119     row-owning regime, two geometries one evaluation, a 3-step solve padded and compact
    iii  case i with set_streaming(50)          chunk mask in attention64_planes one evaluation, a 10-step solve
    (ii has eleven utterances, not nine: with nine the compact geometry has 1796 rows, below the 2048 of the split-K regime, and a
    ragged batch then keeps the padded geometry.  Eleven give 2168 compact and 2732 padded rows, tile height 2 in both.)

With d = max abs over valid frames:
  * parity             d(GPU fp16, fp64 oracle) <= 4 x d(fp16_ref, fp64 oracle) -- the emulation and the kernels drop the same operand
                       bits; the factor pays for the border contractions whose bound the emulation does not know and for elements
                       that per-utterance measured scales move across fp16's subnormal line;
  * the mode took effect   d(GPU fp16, GPU fp32) > 8 x d(GPU fp32, fp64 oracle);
  * invariances inside the mode: a batch row equals its B = 1 run under the same tile override bit for bit, compact equals padded bit
    for bit, and a solve after set_precision("fp32") equals, bit for bit, one taken before the mode was ever switched on;
  * a checkpoint with an unusable bound keeps that layer on bf16x6: contraction_info() does not change with the mode, the result is
    finite and inside the same 4 x bound;
  * the seam object HipEstimator(engine, fp16=True) returns jv_flow_estimator_masked's FP16-mode result bit for bit, and so does the
    reference-side stub of INTEGRATION.md section 2 with its fp16 lines, executed as printed.
Every distance goes to parity_fp16.json in the output directory (committed as profiles/parity_fp16.json), with whether the 10-step mel
of the mode meets the north star's 1e-3 (recorded, not asserted)."""
import ctypes as C
import os
import re

import pytest
import torch

import fp16_ref as fr
import parity_util as pu
from conftest import REPO, load_golden

pytestmark = pytest.mark.gpu

PARITY, EFFECT = 4.0, 8.0
record = pu.Recorder("parity_fp16.json", {
    "what": "max abs over valid frames: FP16 mode and fp32 mode against the fp64 oracle, against each other, and the emulation's distance "
            "(tests/golden/G17_fp16.npz)",
    "bounds": "fp16 <= 4 x emulation; fp16 vs fp32 > 8 x fp32 vs oracle", "north_star_mel": 1e-3})


@pytest.fixture(scope="module")
def gold():
    return load_golden("G17_fp16")


def _engine(sd, noise, batch=22, frames=128):
    from jyutvoice_amd.engine import JV_MODEL_TTS, Engine
    e = Engine("cuda:0", max_batch=batch, max_frames=frames, max_tokens=32)
    e.load_state_dict(JV_MODEL_TTS, sd)
    e.load_noise(noise)
    return e


def solve(eng, c, rows=None):
    idx = list(range(len(c["lens"]))) if rows is None else list(rows)
    mu = c["mu"][idx].cuda()
    mel = eng.cfm_solve(mu, c["lens"][idx], c["spks"][idx].cuda(), torch.zeros_like(mu), c["steps"], 1.0)
    torch.cuda.synchronize()
    return mel.cpu()


def evaluate(eng, c):
    x, mask, mu, t, spks, cond = fr.cfg_batch(c)
    lens = torch.cat([c["lens"], c["lens"]])
    out = eng.flow_estimator(x.cuda(), lens, mu.cuda(), t.cuda(), spks.cuda(), cond.cuda())
    torch.cuda.synchronize()
    return out.cpu()


@pytest.fixture(scope="module")
def ctx(tts_sd, noise):
    """two contexts (JV_NO_COMPACT is read when a context is created), and case i's fp32 solve taken on the first before the FP16
    mode was ever switched on"""
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    saved = {k: os.environ.pop(k, None) for k in ("JV_NO_COMPACT", "JV_EST_FP16", "JV_EXACT_RANGE")}
    engines = {}
    try:
        engines["compact"] = _engine(tts_sd, noise)
        os.environ["JV_NO_COMPACT"] = "1"
        engines["padded"] = _engine(tts_sd, noise)
        os.environ.pop("JV_NO_COMPACT")
        engines["before"] = solve(engines["compact"], fr.case_inputs("i"))
        yield engines
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        for e in engines.values():
            if hasattr(e, "close"):
                e.close()


def both_modes(eng, fn):
    """fn() in fp32 mode, then in FP16 mode; the context is left in fp32 mode"""
    eng.set_precision("fp32")
    a = fn()
    try:
        eng.set_precision("fp16")
        assert eng.contraction_info(with_precision=True)["precision"] == "fp16"
        b = fn()
    finally:
        eng.set_precision("fp32")
    return a, b


def hold(key, got16, got32, want64, floor, lens, north_star=False):
    d16, d32, dmode = fr.valid_dist(got16, want64, lens), fr.valid_dist(got32, want64, lens), fr.valid_dist(got16, got32, lens)
    vals = dict(fp16_vs_oracle=d16, fp32_vs_oracle=d32, fp16_vs_fp32=dmode, emulation_vs_oracle=floor, parity_ratio=d16 / floor)
    if north_star:
        vals["meets_north_star_1e-3"] = float(d16 <= 1e-3)
    record(key, **vals)
    assert torch.isfinite(got16).all(), key
    assert d16 <= PARITY * floor, (key, d16, floor, d16 / floor)
    assert dmode > EFFECT * d32, (key, dmode, d32)


@pytest.mark.parametrize("name", ["i", "iii"])
def test_single_utterance_parity(ctx, gold, name):
    """cases i and iii: the split-K tile regime (252 rows), full and chunk-causal attention"""
    c = fr.case_inputs(name)
    eng = ctx["compact"]
    assert pu.rowgemm_tile(pu.flow_rows([c["T"]])) == 0
    eng.set_streaming(c["chunk"])
    try:
        e32, e16 = both_modes(eng, lambda: evaluate(eng, c))
        m32, m16 = both_modes(eng, lambda: solve(eng, c))
    finally:
        eng.set_streaming(0)
    lens = c["lens"]
    hold(f"{name}/estimator", e16, e32, gold[name + "_est"], float(gold[name + "_est_floor"]), torch.cat([lens, lens]))
    hold(f"{name}/mel{c['steps']}", m16, m32, gold[name + "_mel"], float(gold[name + "_mel_floor"]), lens, north_star=True)


def test_batch_parity_and_invariances(ctx, gold, monkeypatch):
    """case ii: the row-owning regime in both geometries; compact == padded, a row == its B = 1 run under the same tile override"""
    c = fr.case_inputs("ii")
    lens, T, utts = c["lens"], c["T"], list(c["utts"])
    tile = pu.rowgemm_tile(pu.flow_rows(lens.tolist()))
    assert tile > 0 and pu.rowgemm_tile(pu.flow_rows(lens.tolist(), T)) == tile      # past the split-K limit in both geometries
    assert all(int(n) % 16 for n in lens)
    pad, cmp_ = ctx["padded"], ctx["compact"]
    e32, e16 = both_modes(pad, lambda: evaluate(pad, c))
    rows = utts + [len(lens) + u for u in utts]      # the oracle's utterances: conditional rows, then their twins
    hold("ii/estimator", e16[rows], e32[rows], gold["ii_est"], float(gold["ii_est_floor"]), torch.cat([lens[utts], lens[utts]]))
    m32, m16 = both_modes(pad, lambda: solve(pad, c))
    hold("ii/mel3/padded", m16[utts], m32[utts], gold["ii_mel"], float(gold["ii_mel_floor"]), lens[utts])
    c32, c16 = both_modes(cmp_, lambda: solve(cmp_, c))
    hold("ii/mel3/compact", c16[utts], c32[utts], gold["ii_mel"], float(gold["ii_mel_floor"]), lens[utts])
    # the compact run did lay its rows out compactly: its launches account for the real frames
    rep_c = pu.profiled(lambda: (cmp_.set_precision("fp16"), solve(cmp_, c), cmp_.set_precision("fp32")))
    frames = {round(v["flops"] / (v["launches"] * 2.0 * (256.0 * 512 + 2.0 * 256 * 1024))) for k, v in rep_c.items()
              if k.startswith("rowblock_h3<") and k.endswith(",ln,np1>")}
    assert frames == {2 * int(lens.sum())}, (frames, sorted(rep_c))
    assert torch.equal(c16, m16), pu.md(c16, m16)                                   # compact == padded, bit for bit
    monkeypatch.setenv("JV_ROWGEMM_RT", str(tile))
    pad.set_precision("fp16")
    try:
        batch = solve(pad, c)
        assert torch.equal(batch, m16)                                              # (the override names the tile the batch takes)
        for b in (0, 1, len(lens) - 1):
            one = solve(pad, c, rows=[b])
            n = int(lens[b])
            assert torch.equal(one[0, :, :n], batch[b, :, :n]), (b, pu.md(one[0, :, :n], batch[b, :, :n]))
    finally:
        pad.set_precision("fp32")


def test_fp32_after_a_round_trip_is_bit_identical(ctx):
    """what the switch leaves behind: nothing.  `before` was taken when the context had never seen the mode"""
    eng = ctx["compact"]
    c = fr.case_inputs("i")
    _, m16 = both_modes(eng, lambda: solve(eng, c))
    after = solve(eng, c)
    assert torch.equal(after, ctx["before"]), pu.md(after, ctx["before"])
    assert not torch.equal(m16, after)


def test_setters_contradict(ctx):
    from jyutvoice_amd._lib import JvError
    eng = ctx["compact"]
    eng.set_exact_range(True)
    try:
        with pytest.raises(JvError) as ei:
            eng.set_precision("fp16")
        assert "JV_PRECISION_FP16" in str(ei.value) and "exact_range" in str(ei.value)
    finally:
        eng.set_exact_range(False)
    eng.set_precision("fp16")
    try:
        with pytest.raises(JvError) as ei:
            eng.set_exact_range(True)
        assert "JV_PRECISION_FP16" in str(ei.value) and "exact_range" in str(ei.value)
    finally:
        eng.set_precision("fp32")
    assert ei.value.code == 2      # JV_ERR_STATE


def test_unusable_bound_stays_on_bf16x6(gold, noise):
    """the checkpoint of tests/test_gpu_hostile.py::test_unusable_bound_costs_that_layer_only (its recipe, imported): the block
    without a usable bound keeps bf16x6 in FP16 mode -- were its fp16x3 path taken, the 1e31 channel would overflow the planes"""
    import test_gpu_hostile as th      # noqa: F401  (the recipe's home; the checkpoint itself comes from fr.case_state_dict)
    c = fr.case_inputs("hostile")
    eng = _engine(fr.case_state_dict("hostile"), noise, batch=2)
    try:
        info32 = eng.contraction_info()
        m32, m16 = both_modes(eng, lambda: solve(eng, c))
        eng.set_precision("fp16")
        info16 = eng.contraction_info()
        eng.set_precision("fp32")
        assert info16 == info32 == {"blocks": 56, "blocks_all_h3": 55, "linears_h3": 222, "attention_h3": 55}, (info32, info16)
        hold("hostile/mel10", m16, m32, gold["hostile_mel"], float(gold["hostile_mel_floor"]), c["lens"], north_star=True)
    finally:
        eng.close()


def test_seam_object_runs_the_fp16_plan(ctx):
    """HipEstimator(engine, fp16=True) through the call sequence of ConditionalCFM.forward_estimator's TensorRT branch
    (tests/test_gpu_seam.py::test_trt_seam_protocol): jv_flow_estimator_masked's FP16-mode result, bit for bit, fp32 at the addresses"""
    from jyutvoice_amd._lib import check
    from jyutvoice_amd.flow.estimator import HipEstimator
    eng = ctx["compact"]
    c = fr.case_inputs("i")
    host = fr.cfg_batch(c)
    try:
        est = HipEstimator(eng, fp16=True)
        assert eng.contraction_info(with_precision=True)["precision"] == "fp16"
        x, mask, mu, t, spks, cond = (v.cuda().contiguous() for v in host)
        want = torch.empty_like(x)
        p = lambda v: C.c_void_p(v.data_ptr())
        check(eng.lib.jv_flow_estimator_masked(eng._h, p(x), p(mask), p(mu), p(t), p(spks), p(cond), x.shape[0], x.shape[2], p(want),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        [context, stream], engine = est.acquire_estimator()
        with stream:
            for name, v in zip(("x", "mask", "mu", "t", "spks", "cond"), (x, mask, mu, t, spks, cond)):
                assert context.set_input_shape(name, tuple(v.shape))
            for i, ptr in enumerate([v.data_ptr() for v in (x, mask, mu, t, spks, cond)] + [x.data_ptr()]):
                assert context.set_tensor_address(engine.get_tensor_name(i), ptr)
            assert context.execute_async_v3(torch.cuda.current_stream().cuda_stream) is True
            torch.cuda.current_stream().synchronize()
        est.release_estimator(context, stream)
        assert x.dtype == torch.float32 and torch.equal(x, want)
        eng.set_precision("fp32")
        fp32 = evaluate(eng, c)
        assert not torch.equal(fp32, want.cpu())
    finally:
        eng.set_precision("fp32")


def test_integration_md_fp16_stub_runs_verbatim(ctx, monkeypatch):
    """INTEGRATION.md section 2(b) and its fp16 continuation, executed exactly as printed (as
    tests/test_gpu_seam.py::test_integration_md_stub_runs_verbatim executes the first block): the module's result is the library's
    FP16-mode evaluation bit for bit, and differs from the fp32 mode's"""
    import ctypes
    from jyutvoice_amd import _lib
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    sec = text[text.index("## 2. Operator-level seam"):text.index("## 3. C ABI summary")]
    blocks = re.findall(r"```python\n(.*?)```", sec, flags=re.S)
    stub = [b for b in blocks if "reference-side stub" in b]
    fp16 = [b for b in blocks if "class HipEstimatorFp16" in b]
    assert len(stub) == 1 and len(fp16) == 1
    real = ctypes.CDLL
    monkeypatch.setattr(ctypes, "CDLL", lambda name, *a, **k: real(_lib.LIB_PATH if name == "libjyutvoice_hip.so" else name, *a, **k))
    eng = ctx["compact"]
    c = fr.case_inputs("i")
    args = [v.cuda() for v in fr.cfg_batch(c)]
    ns = {}
    exec(compile(stub[0], "INTEGRATION.md#2b", "exec"), ns)
    exec(compile(fp16[0], "INTEGRATION.md#2b-fp16", "exec"), ns)
    try:
        fp32 = evaluate(eng, c)
        mod = ns["HipEstimatorFp16"](eng._h)
        assert isinstance(mod, torch.nn.Module) and eng.contraction_info(with_precision=True)["precision"] == "fp16"
        got = mod(*args).cpu()
        want = evaluate(eng, c)      # the library's own entry, the context still in FP16 mode
        assert torch.equal(got, want)
        assert not torch.equal(got, fp32)
    finally:
        eng.set_streaming(0)
        eng.set_precision("fp32")
