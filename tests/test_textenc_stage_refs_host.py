"""CPU: the stage references of tests/textenc_stage_ref.py and the restated length-regulation rule, without a GPU.

(a) They are the model: the fp64 chain of the per-stage formulas equals oracle.textenc.text_encoder + duration_predictor (and the
    speaker projection of oracle.tts) in fp64 to 1e-10 on every case of test_gpu_textenc_stages.py.  (table="oracle": the oracle's
    fp64 run multiplies by fp32-rounded cos / sin; the references' default table takes them in fp64 of the same fp32 angle, and the
    two differ by no more than that one rounding -- asserted here.)
(b) They can tell: each plausible mistake, applied to the fp32 evaluation of ONE stage fed the same fp32 taps, lands more than
    the bound (textenc_stage_ref.ratio_of x the fp32 floor: 8 x, for the FF stages 10.4 x) from the fp64 stage on at least one
    utterance of those cases -- the bound test_gpu_textenc_stages.py holds the kernels to.  Rows behind a length are compared too (the reference is zero there: a stage that is not masked shows).
(c) The conditions the cases are built on hold on the fp64 reference alone: `mags` spreads the H0 row maxima over 8 x or more
    (measured: 7.37 / 88.3 / 7.03, 12.6 x), every arithmetic stage has a floor > 0, and no live row of any stage is (near) zero.
(d) Length regulation: every generated logw keeps exp(logw) 0.25 (less the fp32 rounding of the logarithm) from an integer; the
    restated rule equals oracle.textenc.length_regulate wherever the fp64 sum lies more than 4 fp32 ulps from an integer, which is at least 90 % of the
    random sweep and all of it at the scales 1.0 / 2.0 / 0.5; the band batches put at least 50 utterances inside the band."""
import numpy as np
import pytest
import torch

import test_gpu_fused_ops as fo      # distances / RATIO (a module object: none of its tests is collected here)
import textenc_stage_ref as ts

assert ts.RATIO == fo.RATIO


@pytest.fixture(scope="module", autouse=True)
def threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


@pytest.mark.parametrize("name", list(ts.CASES))
def test_references_are_the_oracle(name):
    import torch.nn.functional as F
    from oracle import textenc as otext
    b, sd = ts.inputs(name), ts.weights()[torch.float64]
    got = ts.chain(name, table="oracle")
    spk = b["spk_embed"].double()
    with torch.inference_mode():
        x, mu, m = otext.text_encoder(sd, b["x"], b["x_lengths"], b["lang"], b["tone"], b["word_pos"], b["syllable_pos"], spk)
        logw = otext.duration_predictor(sd, x, m, spk)
        c = F.linear(F.normalize(spk, dim=1), sd["spk_embed_affine_layer.weight"], sd["spk_embed_affine_layer.bias"])
    for k, want in (("X", x), ("MU", mu), ("LOGW", logw), ("SPK", c[:, :, None])):
        assert got[k].shape == want.shape, (k, got[k].shape)
        assert float((got[k] - want).abs().max()) <= 1e-10, k
    # the default table: cos / sin of the same fp32 angle, not rounded to fp32 -- one rounding (2^-24) of each product's factor
    exact = ts.evaluate("QKV0", ts.weights(), got, ts.CASES[name][2], torch.float64)
    assert float((exact - got["QKV0"]).abs().max()) <= 2.0 ** -23 * float(got["QKV0"].abs().max())
    for stage in ts.STAGES:
        assert got[stage].shape[1] == ts.CHANNELS[stage], stage


# mistake -> the stage references it is applied to
MUTANTS = ([("ln_eps", t) for t in ("PRE0", "PRE2", "N10", "N23", "N25", "D1", "D2")]
           + [("ln_unbiased", t) for t in ("PRE1", "N10", "N25", "D2")]
           + [("relu_first", t) for t in ("PRE0", "PRE1", "PRE2")] + [("relu_after_ln", t) for t in ("D1", "D2")]
           + [("no_sqrt", "EMB"), ("no_residual", "H0"), ("no_proj_bias", "H0"), ("spk_normalised", "H0"), ("spk_raw", "SPK")]
           + [(m, t) for m in ("rope_interleaved", "rope_all", "rope_exp288", "rope_sin_sign", "rope_pos1") for t in ("QKV0", "QKV3")]
           + [(m, t) for m in ("scale_576", "keys_unmasked") for t in ("ATT0", "ATT5")]
           + [("tap_off", t) for t in ("PRE0", "FF0", "N20", "D1")]
           + [("unmasked", t) for t in ("PRE1", "FF0", "N20", "D1", "D2")]
           + [("relu_moved", "FF0"), ("relu_moved", "N20"), ("mu_unmasked", "MU")])


@pytest.mark.parametrize("mut,tap", MUTANTS)
def test_reference_catches(mut, tap):
    seen = {}
    for name in ts.SHORT_CASES:
        lens, ws, ref = ts.CASES[name][2], ts.weights(), ts.tap_chain(name)
        T = ts.CASES[name][1]
        r64 = ts.evaluate(tap, ws, ref, lens, torch.float64)
        r32 = ts.evaluate(tap, ws, ref, lens, torch.float32).double()
        bad = ts.evaluate(tap, ws, ref, lens, torch.float32, mut).double()
        for b, L in enumerate(lens):
            if L == 0:
                continue
            n = ts.live(tap, T)      # every position, the ones behind the length too
            md, fl = fo.distances(ts.rows_of(bad, b, n), ts.rows_of(r64, b, n), ts.rows_of(r32, b, n), slice(None))
            assert fl > 0.0 or ts.one_token_attention(tap, L), (name, b)
            bound = ts.ratio_of(tap) * ts.floor_of(tap, fl)      # (the GPU file's, margins included)
            seen[(name, b)] = (md, bound)
            if fl > 0.0 and md > bound:
                return
    assert False, (mut, tap, seen)


@pytest.mark.parametrize("name", list(ts.CASES))
def test_case_conditions(name):
    _, T, lens = ts.CASES[name]
    ws, ref = ts.weights(), ts.tap_chain(name)
    if name == "mags":
        peak = [float(ref["H0"][b].double().abs().max()) for b in range(len(lens))]
        assert max(peak) >= 8.0 * min(peak), peak
    for stage in ts.STAGES:
        r64 = ts.evaluate(stage, ws, ref, lens, torch.float64)
        r32 = ts.evaluate(stage, ws, ref, lens, torch.float32).double()
        assert torch.isfinite(r64).all() and torch.isfinite(r32).all(), stage
        mv = ts.moved(stage)
        for b, L in enumerate(lens):
            n = ts.live(stage, L)
            tail = r64[b, :, n:]
            assert float(tail.abs().max() if tail.numel() else 0.0) == 0.0, (stage, b)
            if L == 0:
                assert stage == "SPK" or float(r64[b].abs().max()) == 0.0, (stage, b)      # the dead utterance: zeros everywhere
                continue
            a, f = ts.rows_of(r64, b, n), ts.rows_of(r32, b, n)
            assert float(a.abs().amax(dim=1).min()) >= 1e-20, (stage, b)
            if mv is not None:      # the columns that only move data: the fp32 evaluation is the fp64 one, to the bit
                assert torch.equal(a[:, mv], f[:, mv]), (stage, b)
                if stage == "X":
                    continue
                keep = torch.ones(a.shape[1], dtype=torch.bool)
                keep[mv] = False
                a, f = a[:, keep], f[:, keep]
            _, fl = fo.distances(a, a, f, slice(None))
            if ts.one_token_attention(stage, L):
                assert fl == 0.0 and torch.equal(a, ts.rows_of(ref[f"QKV{stage[-1]}"].double(), b, n)[:, 1152:]), (stage, b)
            else:
                assert fl > 0.0, (stage, b)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_length_regulation_rule_and_the_oracle():
    """(d) of the module docstring"""
    eligible = total = band_total = 0
    disagree = []
    for key, seed, B, Tt, scale, band in ts.lr_sweep():
        logw, lens, mu_x = ts.lr_inputs(seed, B, Tt, band)
        assert ts.lr_margin(logw) >= ts.LR_MARGIN, key
        assert int(lens.min()) >= 1 and int(lens.max()) == Tt and (B == 1 or int(lens[-1]) == 1), key
        w, ylen, attn, mu_y, sum64, cum = ts.lr_rule(logw, lens, mu_x, scale)
        w_o, ylen_o, attn_o, mu_y_o = ts.lr_oracle(logw, lens, mu_x, scale)
        assert torch.equal(w, w_o), key
        assert torch.equal(torch.from_numpy(cum), torch.cumsum(w_o[:, 0], 1)), key      # the prefixes agree everywhere
        inband = ts.lr_in_band(sum64)
        if band:
            assert np.all(np.abs(sum64 - np.rint(sum64)) < 1e-3), key      # the construction: the real sum is an integer
            band_total += int(inband.sum())
        else:
            total += B
            eligible += B if scale in ts.LR_EXACT_SCALES else int((~inband).sum())      # (exact terms and sums: no band)
        for b in range(B):
            exact = scale in ts.LR_EXACT_SCALES
            if not inband[b] or exact:
                yo, yr = int(ylen_o[b]), int(ylen[b])
                ok = (yo == yr and torch.equal(attn[b, :, :yr], attn_o[b, :, :yr]) and torch.equal(mu_y[b, :, :yr], mu_y_o[b, :, :yr])
                      and float(attn_o[b, :, yr:].abs().max() if attn_o.shape[2] > yr else 0.0) == 0.0)
                if not ok:
                    disagree.append((key, b, float(sum64[b]), yr, yo))
    assert not disagree, disagree
    assert eligible >= 0.9 * total, (eligible, total)
    assert band_total >= 50, band_total
