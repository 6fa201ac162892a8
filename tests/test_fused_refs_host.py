"""CPU: can the bound of tests/test_gpu_fused_ops.py -- a kernel may lie 8 x the fp32 chain's distance from the fp64 reference --
catch a subtly wrong kernel on the inputs that file uses?  Each reference is evaluated with ONE plausible mistake at a time, in
fp64, and must land more than 8 x the fp32 floor from the true fp64 result on at least one row the GPU test compares, in at
least one output the GPU test compares.  A mistake that hid under the bound would be answered by changing the inputs, never the
margin: that is why the GPU file's LayerNorm gains spread over [0.5, 2.5] with offsets, every bias is non-zero, the residual rows
span six decades (a LayerNorm eps of 1e-6 shows on the small ones), to_v's rows are 8 x to_k's (their plane scales differ, so a
swap shows), the utterances' masked tails sit one or two rows ahead of live frames (a causal window reads them), and the masked
rows of the rowres input hold finite values of their utterance's magnitude in these mutants (the GPU run holds NaN there).

Two mistakes of the list are algebraically invisible in their literal form, so their nearest observable form is used:
  * "mask before instead of after the activation": Mish(0) = 0 and Snake(0) = 0, so masking on either side of the activation
    alone gives the same values.  Used instead: block1's mask ahead of LayerNorm -> Mish (rowres: a masked h2 row then reads as
    Mish(ln1_b) + temb in block2's causal window), and the intermediate's mask ahead of its bias (hiftpair: a masked row then
    reads as Snake2(b1)).
  * "time embedding added before the mask": h2 leaves rowres only through block2, which reads h2 * mask, so (Mish + temb) * mask
    is what block2 sees either way.  Used instead: the embedding added ahead of Mish and the mask.
"res_conv reading the unmasked x" changes masked rows only (a 1 x 1 convolution is row-local); the GPU test compares `out` on
every row below M -- a masked row stores res_conv's bias -- so that is where it is looked for."""
import pytest
import torch

import test_gpu_fused_ops as fo      # the references and inputs under test (a module object: none of its tests is collected here)

RATIO = fo.RATIO


def detected(kind, key, mut, outputs, rows):
    """{output: (distance of the mutant, 8 x floor)}; asserts that at least one output shows the mutant beyond the bound"""
    p, r64, r32 = fo.refs(kind, *key)
    f = {"rowblock": fo.ref_rowblock, "rowffn": fo.ref_rowffn, "rowres": fo.ref_rowres, "hiftpair": fo.ref_hiftpair}[kind]
    bad = f(p, torch.float64, mut)
    seen = {}
    for n in outputs:
        md, fl = fo.distances(bad[n], r64[n], r32[n], rows)
        assert fl > 0.0
        seen[n] = (md, RATIO * fl)
    assert any(md > lim for md, lim in seen.values()), (kind, key, mut, seen)
    return seen


M_BLOCK = fo.geometry()["M"]


@pytest.mark.parametrize("mut", ["drop_bo", "drop_b1", "drop_b2", "ln_eps", "gelu_tanh", "kv_scales_swapped"])
def test_rowblock_reference_catches(mut):
    sel = fo.live(fo.geometry())
    detected("rowblock", (M_BLOCK,), mut, ("h", "out", "ln", "q", "k", "v"), sel)


@pytest.mark.parametrize("mut", ["drop_b1", "drop_b2", "ln_eps", "gelu_tanh"])
def test_rowffn_reference_catches(mut):
    sel = fo.live(fo.geometry())
    detected("rowffn", (M_BLOCK,), mut, ("out", "ln"), sel)


@pytest.mark.parametrize("cin", [256, 512])
@pytest.mark.parametrize("layout", ["uniform", "compact"])
@pytest.mark.parametrize("mut", ["drop_b1", "drop_b2", "drop_br", "ln_eps", "mish_silu", "tap_shift", "mask_before_ln",
                                 "temb_before_mish", "res_unmasked_x", "kv_scales_swapped"])
def test_rowres_reference_catches(mut, layout, cin):
    key = (layout, 46, cin)
    geo = fo.refs("rowres", *key)[0]["geo"]
    if mut == "res_unmasked_x":      # row-local: shows on the masked rows; the GPU test holds `out` on EVERY row below M to one floor
        every = torch.ones(geo["M"], dtype=torch.bool)
        detected("rowres", key, mut, ("out",), every)
    else:
        detected("rowres", key, mut, ("out", "ln", "q", "k", "v"), fo.live(geo))


PAIR_MUTANTS = [(mut, C, k, dil) for (C, k, dil) in [(64, 3, 1), (128, 7, 3), (64, 11, 5), (128, 3, 5)]
                for mut in ["drop_b1", "drop_b2", "tap_shift", "mask_before_bias", "snake2_alpha1", "conv2_dilation", "res_after_scale"]
                if not (mut == "conv2_dilation" and dil == 1)]      # (a first dilation of 1: the same convolution)


@pytest.mark.parametrize("mut,C,k,dil", PAIR_MUTANTS)
def test_hiftpair_reference_catches(mut, C, k, dil):
    geo = fo.refs("hiftpair", C, k, dil)[0]["geo"]
    detected("hiftpair", (C, k, dil), mut, ("out",), fo.live(geo))


def test_fp32_chain_is_a_sane_floor():
    """the floor itself: the fp32 chains sit within a few hundred fp32 ulps of fp64 per row and are not exact -- a degenerate floor
    (zero, or percent-level) would make the 8 x bound meaningless"""
    sel = fo.live(fo.geometry())
    p, r64, r32 = fo.refs("rowblock", M_BLOCK)
    for n in ("h", "out", "ln", "q", "k", "v"):
        _, fl = fo.distances(r32[n], r64[n], r32[n], sel)
        assert 1e-8 < fl < 1e-4, (n, fl)
    p, r64, r32 = fo.refs("rowres", "uniform", 46, 256)
    for n in ("out", "ln", "q", "k", "v"):
        _, fl = fo.distances(r32[n], r64[n], r32[n], fo.live(p["geo"]))
        assert 1e-8 < fl < 1e-4, (n, fl)
    p, r64, r32 = fo.refs("hiftpair", 64, 7, 3)
    _, fl = fo.distances(r32["out"], r64["out"], r32["out"], fo.live(p["geo"]))
    assert 1e-8 < fl < 1e-4, fl
