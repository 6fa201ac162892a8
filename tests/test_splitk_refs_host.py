"""CPU: can the bound of tests/test_gpu_splitk_ops.py -- the kernel may lie 8 x the fp32 chain's distance from the fp64 reference --
catch a subtly wrong split-K launch on the inputs that file uses?  ref_splitk is evaluated with ONE plausible mistake at a time, in
fp64, and must land more than 8 x the fp32 floor from the true fp64 result on at least one row the GPU test compares (`out`: every
row below M; `out2`: the live rows), in EVERY case listed for the mistake below.  A distance that is not finite counts as caught: the
GPU test asserts a finite distance before it asserts the bound.  A mistake that hid under the bound would be answered by changing the
inputs, never the margin: that is why the convolutions' bias is of order 0.02 (the 1e-3 utterance then reaches LayerNorm with a
variance near 4e-4, where eps 1e-6 shows), to_out's and ff.net.2's rows are rowblock_inputs' (stored rows with a variance near 1e-3 for
the second LayerNorm's eps), the residual rows span seven decades and the utterances' magnitudes are 1 / 30 / 1e-3.

Mistakes whose literal form is invisible, and what stands in for them:
  * mask_before_ln: Mish(0) = 0, so a mask on either side of the activation ALONE stores the same values.  Used: the mask moved ahead
    of LayerNorm -> Mish; a masked row then stores Mish(ln_b) + rowvec + res, which the GPU test sees because it compares `out` on the
    masked rows too (they must hold exactly rowvec + res).  On the live rows this form changes nothing.
  * amax_wrong_slot: a launch that staged AND un-scaled utterance b with utterance b - 1's power of two returns the same real number
    wherever nothing overflows or underflows fp16; what differs is the grid.  Modelled as the two fp16 planes (fp16_ref.round_h, twice)
    of A under the neighbour's scale: the x 30 utterance under the x 1 utterance's scale overflows to inf (caught as a non-finite
    distance); the x 1e-3 utterance under the x 30 one's keeps about 22 bits and stays inside the bound -- the case is carried by
    the overflow, which is why the magnitudes ascend from utterance 0 to 1.
  * drop_chunk / double_chunk exist only where a share has two chunks: Cin = 320 (shares 1,1,1,2,1,1,1,2); the second chunk of the first
    two-chunk share is left out / contracted twice, in all three taps."""
import math

import pytest
import torch

import test_gpu_splitk_ops as sk      # the reference and inputs under test (a module object: none of its tests is collected here)

RATIO = sk.RATIO

FIRST = [k for k in sk.CONV_FIRST if k[1] != "one"]
TRUNK = [k for k in sk.CONV_TRUNK if k[1] != "one"]
TRUNK_RES = [k for k in TRUNK if k[2][1]]
LINEAR = [k for k in sk.TO_OUT + sk.FF2 if k[1] != "one"]
# mistake -> the cases it must show in.  ("one": a single live row of magnitude 1 -- no small-variance row, no second utterance, no live
# row behind another -- is left to the mistakes that need none of these: see test_single_frame_catches)
MUTANTS = {
    "drop_bias": FIRST + TRUNK + LINEAR + sk.CLAMP,
    "ln_eps": FIRST + TRUNK,
    "mish_silu": FIRST + TRUNK,
    "mask_before_ln": FIRST + TRUNK,
    "temb_before_mish": FIRST,
    "tap_shift": FIRST + TRUNK,
    "drop_chunk": FIRST,
    "double_chunk": FIRST,
    "ln2_before_res": TRUNK_RES + [k for k in LINEAR if k[2] != 512],
    "ln2_eps": [k for k in LINEAR if k[2] != 512],
    "amax_wrong_slot": TRUNK,
    "res_dropped": TRUNK_RES + LINEAR,
}
PAIRS = [(mut, key) for mut, keys in MUTANTS.items() for key in keys]


def shown(key, mut):
    """{output: (distance of the mutant, 8 x floor)} over the rows the GPU test compares"""
    p, r64, r32 = sk.refs(*key)
    bad = sk.ref_splitk(p, torch.float64, mut)
    M = p["geo"]["M"]
    seen = {}
    for n, rows in (("out", slice(0, M)), ("out2", sk.fo.live(p["geo"]))):
        if n in r64:
            md, fl = sk.fo.distances(bad[n], r64[n], r32[n], rows)
            assert fl > 0.0
            seen[n] = (md, RATIO * fl)
    return seen


@pytest.mark.parametrize("mut,key", PAIRS, ids=[f"{m}-{sk.case_id(k)}" for m, k in PAIRS])
def test_reference_catches(mut, key):
    seen = shown(key, mut)
    assert any(not math.isfinite(md) or md > lim for md, lim in seen.values()), (mut, key, seen)


@pytest.mark.parametrize("mut,key", [(m, k) for m, k in [("drop_bias", ("conv3_first", "one", "per_utt")), ("tap_shift", ("conv3_trunk", "one", (256, True))),
                                                         ("mish_silu", ("conv3_trunk", "one", (512, False))), ("res_dropped", ("to_out", "one", None)),
                                                         ("drop_chunk", ("conv3_first", "one", "shared")), ("ln2_before_res", ("ff2", "one", 256))]])
def test_single_frame_catches(mut, key):
    """the nine-row geometry: the mistakes that need neither a small row, a second utterance nor a live row behind another"""
    seen = shown(key, mut)
    assert any(not math.isfinite(md) or md > lim for md, lim in seen.values()), (mut, key, seen)


def test_unmutated_reference_is_inside():
    """the measure itself: without a mistake the distance is zero, and the floors are fp32-sized -- not zero, not percent-level"""
    for key in FIRST[:1] + TRUNK[:1] + LINEAR[:1] + sk.CLAMP[:1] + [("ff2", "edge2048", 256)]:
        for n, (md, lim) in shown(key, None).items():
            assert md == 0.0 and 8e-8 < lim < 8e-4, (key, n, md, lim)


def test_every_mutant_of_the_issue_is_listed():
    assert sorted(MUTANTS) == sorted(["drop_bias", "ln_eps", "mish_silu", "mask_before_ln", "temb_before_mish", "tap_shift", "drop_chunk",
                                      "double_chunk", "ln2_before_res", "ln2_eps", "amax_wrong_slot", "res_dropped"])
