"""GPU: jv_length_regulate (encops.hip durations_kernel, path_kernel, expand_mu_kernel) against its own documented rule and, where
the rule and the reference model can be told to agree, against oracle.textenc.length_regulate.

The kernel's rule (textenc_stage_ref.lr_rule restates it in numpy): w_ceil = ceil(exp(logw) mask) scale in fp32; the prefixes are
the sequential fp64 sum of w_ceil, each rounded to fp32; y_len = max(long(float(sum64)), 1); attn and mu_y follow from the fp32
prefixes and y_len.  The reference model's y_len is long(torch.sum(w_ceil) in fp32): the order of that fp32 sum is a property of
the torch build, not of the model, so where the real sum lies within a few fp32 ulps of an integer -- fractional scales only -- the
two may land on either side of it.  What is held, per utterance:

(a) the kernel equals the restated rule exactly: w_ceil, y_lengths, attn (as uint8), mu_y bit for bit -- everywhere;
(b) the kernel equals the oracle exactly wherever the fp64 sum lies more than 4 fp32 ulps of itself from the nearest integer, and
    everywhere at the scales 1.0 / 2.0 / 0.5 (every term and sum exact).  test_textenc_stage_refs_host.py shows on the CPU that this
    is at least 90 % of the random sweep;
(c) inside the band (batches whose ceil-sum is a multiple of 10 at scales 0.9 and 1.1: the real sum is an integer) y_len is one of
    the two integers adjacent to the fp64 sum, y_len <= the last prefix so that every column j < y_len of attn is one-hot over the
    live tokens, and mu_y is that gather; how many band utterances agree and disagree with the oracle is recorded;
(d) logw from the encoder's own output on `ragged37`, at scale 1.0, against the oracle.

Inputs are logw = log(k + u), k an integer in [0, 12), u in [0.25, 0.75]: exp(logw) stays a quarter away from every integer, so an
ulp between the GPU's expf and the CPU's cannot move a ceil (asserted on the CPU in fp64 for every input, here and in the host file)."""
import numpy as np
import pytest
import torch

import test_gpu_textenc_stages as stages      # its Recorder: one parity_textenc_stages.json (a module object: no test is collected here)
import textenc_stage_ref as ts

pytestmark = pytest.mark.gpu

record = stages.record


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from jyutvoice_amd.engine import JV_MODEL_TTS, Engine
    e = Engine("cuda:0", max_batch=65, max_frames=64, max_tokens=130)      # durations_kernel: one lane per utterance, blocks of 64
    e.load_state_dict(JV_MODEL_TTS, ts.checkpoint())
    yield e
    e.close()


def regulate(eng, logw, lens, mu_x, scale):
    w, ylen, attn, mu_y = eng.length_regulate(logw.cuda(), lens, mu_x.cuda(), length_scale=scale)
    torch.cuda.synchronize()
    return w.cpu(), ylen.cpu(), attn.cpu(), mu_y.cpu()


def one_hot_gather(attn_b, mu_x_b, L, y):
    """columns j < y of attn [Tt, Ty] are one-hot over the L live tokens; -> the gather they describe [80, y]"""
    a = attn_b[:, :y]
    assert torch.equal(a, (a != 0).float()) and float(a[L:].abs().max() if a.shape[0] > L else 0.0) == 0.0
    assert torch.equal(a.sum(0), torch.ones(y))
    tok = a.argmax(0)
    assert bool((tok[1:] >= tok[:-1]).all())      # monotonic
    return mu_x_b[:, tok]


def test_sweep(eng):
    """(a), (b), (c) over textenc_stage_ref.lr_sweep()"""
    counts = {"utterances": 0, "held_to_oracle": 0, "band": 0, "band_agree": 0, "band_disagree": 0}
    failures = []
    for key, seed, B, Tt, scale, band in ts.lr_sweep():
        logw, lens, mu_x = ts.lr_inputs(seed, B, Tt, band)
        assert ts.lr_margin(logw) >= ts.LR_MARGIN, key
        w, ylen, attn, mu_y = regulate(eng, logw, lens, mu_x, scale)
        w_r, ylen_r, attn_r, mu_y_r, sum64, cum = ts.lr_rule(logw, lens, mu_x, scale)
        w_o, ylen_o, attn_o, mu_y_o = ts.lr_oracle(logw, lens, mu_x, scale)
        inband = ts.lr_in_band(sum64)
        # (a) the rule, whole tensors: zeros behind every y_len and every length included
        for name, g, r in (("w_ceil", w, w_r), ("y_lengths", ylen, ylen_r), ("attn", attn.to(torch.uint8), attn_r.to(torch.uint8)),
                           ("mu_y", mu_y, mu_y_r)):
            if g.shape != r.shape or not torch.equal(g, r):
                failures.append(f"(a) {key} {name}: kernel differs from its rule")
        assert torch.equal(attn, attn.to(torch.uint8).float()), key      # (attn holds 0 and 1 alone)
        for b in range(B):
            L, y, counts["utterances"] = int(lens[b]), int(ylen[b]), counts["utterances"] + 1
            exact = scale in ts.LR_EXACT_SCALES
            if exact or not inband[b]:      # (b)
                counts["held_to_oracle"] += 1
                yo = int(ylen_o[b])
                if not (y == yo and torch.equal(attn[b, :, :y], attn_o[b, :, :y]) and torch.equal(mu_y[b, :, :y], mu_y_o[b, :, :y])
                        and float(attn[b, :, y:].abs().max() if attn.shape[2] > y else 0.0) == 0.0 and torch.equal(w[b], w_o[b])):
                    failures.append(f"(b) {key} utt{b}: sum {sum64[b]!r}: kernel y_len {y}, oracle {yo}")
            if inband[b] and not exact:      # (c)
                counts["band"] += 1
                counts["band_agree" if y == int(ylen_o[b]) else "band_disagree"] += 1
                if not (y in (int(np.floor(sum64[b])), int(np.ceil(sum64[b]))) and float(y) <= float(cum[b, L - 1])):
                    failures.append(f"(c) {key} utt{b}: sum {sum64[b]!r}: y_len {y}, last prefix {cum[b, L - 1]!r}")
                    continue
                if not torch.equal(mu_y[b, :, :y], one_hot_gather(attn[b], mu_x[b], L, y)):
                    failures.append(f"(c) {key} utt{b}: mu_y is not the gather of attn")
    record("length_regulation", **counts)
    assert not failures, failures
    assert counts["band"] >= 50, counts
    assert counts["held_to_oracle"] >= 0.9 * (counts["utterances"] - counts["band"]), counts


def test_the_encoders_own_logw(eng):
    """(d) logw of `ragged37` from jv_encoder_fwd itself, scale 1.0: the oracle's w_ceil, y_lengths, attn and mu_y"""
    b = ts.inputs("ragged37")
    _, mu_x, logw, _ = eng.encoder(b["x"], b["x_lengths"], b["lang"], b["tone"], b["word_pos"], b["syllable_pos"], b["spk_embed"])
    logw, mu_x = logw.cpu(), mu_x.cpu()
    live = ts.x_mask(ts.CASES["ragged37"][2], 37, torch.float64)[:, 0] > 0
    e = torch.exp(logw.double())[:, 0]
    assert float((e - e.round()).abs()[live].min()) > 1e-4      # no live exp(logw) sits on an integer: the ceil is not an ulp's toss
    got = regulate(eng, logw, b["x_lengths"], mu_x, 1.0)
    want = ts.lr_oracle(logw, b["x_lengths"], mu_x, 1.0)
    for name, g, o in zip(("w_ceil", "y_lengths", "attn", "mu_y"), got, want):
        assert g.shape == o.shape and torch.equal(g, o), name
