"""CPU: the stage references of tests/est_stage_ref.py, without a GPU.

(a) They are the model: the fp64 chain of the per-stage formulas equals oracle.flow.estimator in fp64 to 1e-10 on every case of
    test_gpu_est_stages.py in both modes, streaming included (table="oracle": the oracle handed t in fp64 takes this build's fp32
    torch.exp table and the angle in fp64; the references' default takes the correctly rounded table and the fp32 angle).  The local
    forms that exist for the mistakes are the oracle's functions when no mistake is set.
(b) The frequency table: in how many of its 160 entries this build's torch.exp differs from the correctly rounded one, and by how
    much that moves TSIN and TEMB (printed; the differences are held to one ulp).
(c) They can tell: each listed mistake, applied to the fp32 evaluation of ONE stage fed the same fp32 taps, lands more than the bound
    (est_stage_ref.ratio_of x the fp32 floor) from the fp64 stage on at least one sample of the short cases -- the bound
    test_gpu_est_stages.py holds the kernels to.
(d) The conditions the cases are built on hold on the fp64 reference alone.

Mistakes no tap can show.  The masks are prefix masks, every convolution of the trunk is causal or 1 x 1, and a tap is zero behind a
length: a live output row never depends on an input row behind its own sample's length, so `res_conv` on the unmasked input and `DOWN`
/ `D` reading unmasked rows change rows behind a length only -- rows the tap zeroes and every consumer masks again (asserted below:
the live rows are BIT-equal with and without the mistake).  What an unmasked read can do to a live row is reach the rows AHEAD of the
sample's first frame -- in the row layout the guard / gap rows, which hold whatever the producer left there.  The visible variant is
that: "halo", the two frames of left context taken from the previous sample's buffer instead of zeros.
LayerNorm eps 1e-6 for 1e-5 moves a row by 4.5e-6 / variance of the LayerNorm's input.  It shows behind the convolutions (RESi, FIN:
10 to 10^4 x the floor) and in the first block of the trunk (BLK0_0: 23 x); the later blocks normalise a residual stream whose
rows have grown, and there the mistake is 1.3 to 1.6 x the fp32 floor -- no fp32 comparison can see it
(test_eps_is_under_the_floor_in_the_late_blocks), so those stages take "ln_eps_big" (1e-1), as the up-sampling file did."""
import math

import pytest
import torch

import est_stage_ref as es
import test_gpu_fused_ops as fo      # distances / RATIO (a module object: none of its tests is collected here)
from oracle import flow as oflow

assert es.RATIO == fo.RATIO
MODES = ("entry", "step")
SHORT_CASES = tuple(k for k in es.CASES if k != "big260")


@pytest.fixture(scope="module", autouse=True)
def threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(es.CASES))
def test_references_are_the_oracle(name, mode):
    inp = es.inputs(name)
    geo = es.geometry(inp, mode)
    got = es.chain(inp, geo, table="oracle")
    x, mu, spks, cond, t = es.samples(inp, mode)
    mask = es.mask_of(geo, torch.float64)
    with torch.inference_mode():
        want = oflow.estimator(es.weights()[torch.float64], x.double(), mask, mu.double(), t.double().expand(geo["S"]), spks.double(),
                               cond.double(), streaming=geo["chunk"] > 0, chunk=max(geo["chunk"], 1))
    assert got["D"].shape == want.shape == (geo["S"], 80, geo["T"])
    assert float((got["D"] - want).abs().max()) <= 1e-10
    for tap in es.TAPS:
        assert tuple(got[tap].shape) == es.shape_of(tap, geo), tap
    # the default table and angle against the oracle's: one rounding of the angle (2^-24 x 1000 t) and the table's ulps
    exact = es.evaluate("TSIN", es.weights(), got, geo, torch.float64)
    assert float((exact - got["TSIN"]).abs().max()) <= 1000.0 * 2.0 ** -22


def test_local_forms_are_the_oracles():
    """_cblock / _tblock / _resnet without a mistake are oracle.flow's causal_block / transformer_block / resnet"""
    inp = es.inputs("chunk")
    geo = es.geometry(inp, "entry")
    sd, ref = es.weights()[torch.float64], es.chain(inp, geo)
    mask = es.mask_of(geo, torch.float64)
    pre = es.stage_prefix(3)
    with torch.inference_mode():
        x = ref["BLK2_3"]
        assert torch.equal(es._cblock(sd, pre + "0.block1.", x, mask, "none"), oflow.causal_block(sd, pre + "0.block1.", x, mask))
        ok = es.allowed_keys(geo)
        h = ref["RES3"].transpose(1, 2)
        assert torch.equal(es._tblock(sd, pre + "1.0.", h, ok, "none"), oflow.transformer_block(sd, pre + "1.0.", h, (1.0 - ok.double()) * -1.0e10))
        # oracle.flow.resnet takes the time MLP's output and projects it itself: the same thing as the TEMB slice
        tm = torch.randn(geo["S"], 1024, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        temb = torch.nn.functional.linear(torch.nn.functional.mish(tm), sd[pre + "0.mlp.1.weight"], sd[pre + "0.mlp.1.bias"])
        for mut in (None, "none"):
            assert float((es._resnet(sd, pre + "0.", x, mask, temb, mut) - oflow.resnet(sd, pre + "0.", x, mask, tm)).abs().max()) <= 1e-12


def test_frequency_table():
    """(b) torch.exp in fp32 against the correctly rounded table, and what a one-ulp table does to TSIN / TEMB"""
    exact, here = es.freq_table(), es.freq_table("torch")
    ulp = torch.nextafter(exact, torch.full_like(exact, 2.0)) - exact
    off = (here != exact)
    assert float(((here - exact).abs() / ulp).max()) <= 1.0      # never more than one ulp
    print(f"torch.exp differs from the correctly rounded table in {int(off.sum())} of {es.HALF} entries")
    ws = es.weights()
    for t in (0.3, es.T_STEP):
        inp = dict(es.inputs("t1"), t=torch.tensor([t]))
        geo = es.geometry(inp, "entry")
        src = {"in": inp}
        fig = {}
        for kind, mut in (("exact", None), ("ulp", "freq_ulp")):
            s = dict(src)
            for tap in es.TIME_TAPS:
                s[tap] = es.evaluate(tap, ws, s, geo, torch.float64, mut if tap == "TSIN" else None)
            fig[kind] = s
        a = ((1000.0 * torch.tensor([t])).unsqueeze(1) * here.unsqueeze(0)).double()
        tsin_here = torch.cat([a.sin(), a.cos()], dim=-1)
        floor = float((es.evaluate("TSIN", ws, src, geo, torch.float32).double() - fig["exact"]["TSIN"]).abs().max())
        d_sin = float((fig["ulp"]["TSIN"] - fig["exact"]["TSIN"]).abs().max())
        d_emb = float((fig["ulp"]["TEMB"] - fig["exact"]["TEMB"]).abs().max())
        d_here = float((tsin_here - fig["exact"]["TSIN"]).abs().max())
        print(f"t = {t}: one ulp in every entry moves TSIN by {d_sin:.2e} (fp32 floor {floor:.2e}) and TEMB by {d_emb:.2e} of "
              f"{float(fig['exact']['TEMB'].abs().max()):.2f}; this build's torch.exp moves TSIN by {d_here:.2e}")
        assert d_sin > es.RATIO * floor      # an ulp of the table is far outside the bound of TSIN
        assert d_here <= d_sin


# mistake -> the stages it is applied to (the docstring says which mistakes no tap can show)
LATE_BLOCKS = ("BLK7_2", "BLK13_3")
MUTANTS = ([("ln_eps", t) for t in ("RES0", "RES6", "RES13", "FIN", "BLK0_0")] + [("ln_eps_big", t) for t in LATE_BLOCKS]
           + [("gelu_tanh", t) for t in ("BLK0_0", "BLK5_1", "BLK13_3")]
           + [("mish_silu", t) for t in ("RES0", "RES4", "RES13", "FIN")] + [("temb_silu", "TMISH"), ("temb_no_mish", "TMISH")]
           + [("temb_late", t) for t in ("RES0", "RES9", "RES13")]
           + [("temb_next", "RES0"), ("temb_prev", "RES1"), ("temb_next", "RES1"), ("temb_prev", "RES7"), ("temb_next", "RES12"), ("temb_prev", "RES13")]
           + [("halo", t) for t in ("RES0", "RES2", "RES13", "FIN")]
           + [("tap_off", t) for t in ("RES0", "RES3", "RES13", "DOWN", "UPC", "FIN")] + [("cat_swap", "RES13")]
           + [(m, t) for m in ("scale_512", "keys_unmasked", "chunk_off") for t in ("BLK0_0", "BLK6_3", "BLK13_1")]
           + [(m, "TSIN") for m in ("no_1000", "sincos_swap", "over160", "freq_ulp")] + [("twin_mu", "XIN")])


def sample_blocks(tap, geo, t):
    """[(sample or None, rows [n, C] over EVERY position of it)]: a time tap is one block"""
    if tap in es.TIME_TAPS:
        return [(None, t)]
    return [(b, es.rows_of(t, b, t.shape[2])) for b, L in enumerate(geo["L"]) if L > 0]


def runs_for(mut):
    cases = ("chunk",) if mut == "chunk_off" else SHORT_CASES
    return [(c, m) for c in cases for m in (("step",) if mut == "twin_mu" else MODES)]


@pytest.mark.parametrize("mut,tap", MUTANTS)
def test_reference_catches(mut, tap):
    seen = {}
    ws = es.weights()
    with torch.inference_mode():
        for name, mode in runs_for(mut):
            inp, ref = es.inputs(name), es.tap_chain(name, mode)
            geo = es.geometry(inp, mode)
            r64 = es.evaluate(tap, ws, ref, geo, torch.float64)
            r32 = es.evaluate(tap, ws, ref, geo, torch.float32).double()
            bad = es.evaluate(tap, ws, ref, geo, torch.float32, mut).double()
            for (b, a), (_, f), (_, m) in zip(sample_blocks(tap, geo, r64), sample_blocks(tap, geo, r32), sample_blocks(tap, geo, bad)):
                md, fl = fo.distances(m, a, f, slice(None))
                assert fl > 0.0 or es.moves_data(tap), (name, mode, b)
                seen[(name, mode, b)] = (md, es.ratio_of(tap) * fl)
                if md > es.ratio_of(tap) * fl:
                    return
    assert False, (mut, tap, seen)


@pytest.mark.parametrize("tap", LATE_BLOCKS)
def test_eps_is_under_the_floor_in_the_late_blocks(tap):
    """eps 1e-6 in a late block stays inside the bound on every sample of every short case: why those stages show 1e-1 instead"""
    ws = es.weights()
    with torch.inference_mode():
        for name, mode in runs_for("ln_eps"):
            inp, ref = es.inputs(name), es.tap_chain(name, mode)
            geo = es.geometry(inp, mode)
            r64, r32, bad = (es.evaluate(tap, ws, ref, geo, dt, mut).double() for dt, mut in
                             ((torch.float64, None), (torch.float32, None), (torch.float32, "ln_eps")))
            for (b, a), (_, f), (_, m) in zip(sample_blocks(tap, geo, r64), sample_blocks(tap, geo, r32), sample_blocks(tap, geo, bad)):
                md, fl = fo.distances(m, a, f, slice(None))
                assert md <= es.RATIO * fl, (name, mode, b, md / fl)


@pytest.mark.parametrize("mut,tap", [("res_unmasked", "RES0"), ("res_unmasked", "RES13"), ("in_unmasked", "DOWN"), ("in_unmasked", "D")])
def test_mistakes_no_tap_can_show(mut, tap):
    """an unmasked read of a causal or 1 x 1 stage behind prefix masks: the stage's tap holds the same bits (module docstring); the
    source is made nonzero behind the lengths first, as a buffer is"""
    ws = es.weights()
    with torch.inference_mode():
        for name in ("ragged37", "dead"):
            inp, ref = es.inputs(name), dict(es.tap_chain(name, "entry"))
            geo = es.geometry(inp, "entry")
            for k in es.sources_of(tap):
                if k not in es.TIME_TAPS:
                    ref[k] = ref[k] + 3.0 * (1.0 - es.mask_of(geo, torch.float32))
            good = es.evaluate(tap, ws, ref, geo, torch.float64)
            assert torch.equal(good, es.evaluate(tap, ws, ref, geo, torch.float64, mut)), (name, tap)
            assert torch.equal(good, es.evaluate(tap, ws, es.tap_chain(name, "entry"), geo, torch.float64)), (name, tap)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SHORT_CASES)
def test_case_conditions(name, mode):
    inp, ws, ref = es.inputs(name), es.weights(), es.tap_chain(name, mode)
    geo = es.geometry(inp, mode)
    with torch.inference_mode():
        if geo["chunk"]:      # at least two chunk lines inside the longest sample, and the mask removes live keys in every stage
            assert max(geo["L"]) > 2 * geo["chunk"]
            for tap in ("BLK0_0", "BLK13_3"):
                free = es.evaluate(tap, ws, ref, dict(geo, chunk=0), torch.float64)
                assert float((free - es.evaluate(tap, ws, ref, geo, torch.float64)).abs().max()) > 1e-3, tap
        for tap in es.TAPS:
            r64 = es.evaluate(tap, ws, ref, geo, torch.float64)
            r32 = es.evaluate(tap, ws, ref, geo, torch.float32).double()
            assert tuple(r64.shape) == es.shape_of(tap, geo), tap
            assert torch.isfinite(r64).all() and torch.isfinite(r32).all(), tap
            if tap in es.TIME_TAPS:
                _, fl = fo.distances(r64, r64, r32, slice(None))
                assert fl > 0.0, tap
                continue
            for b, L in enumerate(geo["L"]):
                assert float(r64[b, :, L:].abs().max() if L < geo["T"] else 0.0) == 0.0, (tap, b)
                if L == 0:
                    assert float(r64[b].abs().max()) == 0.0, (tap, b)
                    continue
                a, f = es.rows_of(r64, b, L), es.rows_of(r32, b, L)
                assert float(a.abs().amax(dim=1).min()) >= 1e-20, (tap, b)
                _, fl = fo.distances(a, a, f, slice(None))
                assert (fl == 0.0 and torch.equal(a, f)) if es.moves_data(tap) else fl > 0.0, (tap, b)


def test_case_geometry():
    """the row arithmetic the cases are named for (flow.hip: 4 guard rows, 4 gap rows behind every sample)"""
    row0 = lambda name, b: 4 + b * (es.CASES[name]["T"] + 4)
    assert row0("seam", 1) % 32 not in (0,) and row0("seam", 1) % 80 not in (0,) and row0("seam", 2) % 160 == 0
    assert row0("big260", 8) == 2116 and row0("big260", 8) - 264 <= 2048 < row0("big260", 8)      # the smallest B2 x 264 above 2048
    for name in SHORT_CASES:      # everything else stays on the short side in both modes
        assert 4 + 2 * len(es.CASES[name]["lens"]) * (es.CASES[name]["T"] + 4) <= 2048, name
    assert es.CASES["ragged37"]["lens"][1] == es.CASES["ragged37"]["T"] - 1
    assert [es.TAPS.index(t) for t in ("TSIN", "XIN", "RES0", "DOWN", "RES1", "RES13", "BLK13_3", "UPC", "FIN", "D")] == [0, 4, 5, 10, 11, 71, 75, 76, 77, 78]
    assert len(es.TAPS) == 79
    s = es.inputs("mags")
    assert float(s["x"][1].abs().max() / s["x"][2].abs().max()) > 500.0
    # the step mode's twins: x of the utterance, zeros elsewhere
    xin = es.evaluate("XIN", es.weights(), {"in": s}, es.geometry(s, "step"), torch.float32)
    assert torch.equal(xin[3:, :80], xin[:3, :80]) and float(xin[3:, 80:].abs().max()) == 0.0 and float(xin[:3, 80:].abs().max()) > 0.0
    assert math.isclose(es.T_STEP, 0.9045)
