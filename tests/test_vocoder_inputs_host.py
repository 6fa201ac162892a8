"""No GPU: the inputs of the unclipped vocoder tests really are unclipped.

test_gpu_vocoder_unclipped.py and the vocoder part of test_gpu_positions.py compare waveforms sample by sample; a sample on
+-HIFT_AUDIO_LIMIT reads the clamp on both sides whatever the kernels computed.  Their condition -- at most 1 % of the fp64
reference's samples with |w| >= 0.99 -- is asserted here on the reference alone, for the exact inputs and seeds of every GPU
case (parity_util.VOCODER_CASES), each utterance cut to its own length as the GPU cases compare it, on both synthetic
checkpoints: the cap is known to hold before a GPU is involved."""
import pytest
import torch

import parity_util as pu


@pytest.mark.parametrize("kind", ["tame", "hostile"])
def test_quiet_recipe_keeps_the_reference_off_the_clamp(kind):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    _, w64 = pu.hift_folded(pu.hift_checkpoint(kind))
    shares = {}
    for name in pu.VOCODER_CASES:
        mel, s, lens = pu.quiet_vocoder_inputs(name)
        for b, L in enumerate(lens):
            ref = pu.hift_fp64(w64, mel[b:b + 1], s[b:b + 1], L)
            assert ref.dtype == torch.float64 and ref.shape == (1, 480 * L) and torch.isfinite(ref).all()
            shares[f"{name}[{b}] ({L} frames)"] = pu.clamp_share(ref)
            assert float(ref.pow(2).mean().sqrt()) > 0.02, (name, b)      # audible: the cap is not met by silence
    print(f"clamped share of the fp64 reference, {kind} checkpoint:")
    for k, v in shares.items():
        print(f"  {k}: {100 * v:.3f} %")
    worst = max(shares, key=shares.get)
    assert shares[worst] <= pu.CLAMP_CAP, (worst, shares[worst])


def test_the_older_recipe_is_mostly_clamp():
    """the measurement that motivates the new cases, kept as a test: test_hift_pair_matches_separate_launches' own inputs (seed
    123, mel = 1.5 randn, s = tanh(0.3 randn)) put most of the reference on the clamp"""
    g = torch.Generator().manual_seed(123)
    T = 61
    mel = torch.randn(3, 80, T, generator=g) * 1.5
    s = torch.tanh(torch.randn(3, 1, 480 * T, generator=g) * 0.3)
    w32, _ = pu.hift_folded(pu.hift_checkpoint("tame"))
    share = pu.clamp_share(pu.hift_fp32(w32, mel[:1], s[:1], T))
    print(f"clamped share with the older recipe: {100 * share:.1f} %")
    assert share > 0.5
