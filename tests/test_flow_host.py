"""Host-side checks of the token-to-mel route (no GPU): the fp64 restatement of the relative-position attention against what the
imported reference module computed (G13), the state-dict split, and every error `CausalMaskedDiffWithXvec` raises before it
touches the device."""
import pytest
import torch

import relattn_ref as ref
from conftest import load_golden


def flow_sd(prompt_sd, tts_sd):
    sd = dict(prompt_sd)
    sd.update({k: v for k, v in tts_sd.items() if k.startswith(("decoder.", "spk_embed_affine_layer."))})
    return sd


def new_flow(**kw):
    from jyutvoice_amd.flow.flow import CausalMaskedDiffWithXvec
    return CausalMaskedDiffWithXvec(vocab_size=6561, input_frame_rate=25, **kw)


def test_restated_attention_matches_reference_module(prompt_sd):
    """tests/relattn_ref.py (fp64, rel_shift by indexing, the chunk mask as a key limit) against the outputs of the imported
    RelPositionMultiHeadedAttention (encoders.0.self_attn) on the G13 run: 93 tokens, full attention and static chunks of 25.
    The fixture is fp32 arithmetic: four chained contractions of 512 / 64 / 93 / 512 terms of order-one operands, each within
    ~sqrt(K) * 6e-8 of exact, on outputs of order one -- 2e-5 leaves a decade over that and is four decades below the
    difference the mask makes."""
    g = load_golden("G13_flow_encoder")
    pre = "encoder.encoders.0.self_attn."
    w = {k[len(pre):]: v for k, v in prompt_sd.items() if k.startswith(pre)}
    x = g["attn_x"][0]
    full = ref.mha(x, w, 93, 0)
    stream = ref.mha(x, w, 93, 25)
    e_full = float((full - g["attn_out_full"][0].double()).abs().max())
    e_stream = float((stream - g["attn_out_stream"][0].double()).abs().max())
    print(f"restated attention vs reference module: full {e_full:.3e}  streaming {e_stream:.3e}  "
          f"|out| {float(full.abs().max()):.3f}")
    assert e_full <= 2e-5 and e_stream <= 2e-5
    assert float((full - stream).abs().max()) > 1e-2                 # the mask is not a no-op
    assert float((full[75:] - stream[75:]).abs().max()) <= 1e-12     # ... except in the last chunk, which sees every key


def test_key_limit_is_the_reference_mask():
    """subsequent_chunk_mask(size, chunk) with all left chunks (utils/mask.py:91-126): row i sees columns < (i // chunk + 1) * chunk"""
    for T, chunk in ((93, 25), (186, 50), (7, 25)):
        want = torch.zeros(T, T, dtype=torch.bool)
        for i in range(T):
            want[i, :min((i // chunk + 1) * chunk, T)] = True
        got = torch.tensor([[j < ref.key_limit(i, T, chunk) for j in range(T)] for i in range(T)])
        assert torch.equal(got, want)
    assert ref.key_limit(5, 3, 0) == 3 and ref.key_limit(5, 9, 4) == 8 and ref.key_limit(30, 28, 25) == 28


def test_state_dict_split(prompt_sd, tts_sd):
    from jyutvoice_amd import spec
    from jyutvoice_amd.flow.encoder import extract_flow_weights
    sd = flow_sd(prompt_sd, tts_sd)
    assert len(sd) == 1121 and set(sd) == set(spec.FLOW_INVENTORY)
    enc, dec = extract_flow_weights(sd)
    assert set(enc) == set(spec.PROMPT_INVENTORY) and len(enc) == 206 + 3
    assert set(dec) == set(spec.FLOW_DECODER_INVENTORY) and len(dec) == 910 + 2
    assert all(tuple(sd[k].shape) == tuple(s) for k, s in spec.FLOW_INVENTORY.items())


def test_load_errors_name_keys_and_shapes(prompt_sd, tts_sd):
    sd = flow_sd(prompt_sd, tts_sd)
    flow = new_flow()
    short = dict(sd)
    del short["encoder_proj.bias"]
    with pytest.raises(RuntimeError, match=r"Error\(s\) in loading state_dict for CausalMaskedDiffWithXvec: Missing key\(s\): "
                                             r"\['encoder_proj.bias'\]"):
        flow.load_state_dict(short)
    extra = dict(sd)
    extra["dp.proj.bias"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match=r"Unexpected key\(s\): \['dp.proj.bias'\]"):
        flow.load_state_dict(extra)
    bad = dict(sd)
    bad["spk_embed_affine_layer.weight"] = torch.zeros(80, 191)
    with pytest.raises(RuntimeError, match=r"size mismatch for spk_embed_affine_layer.weight: copying a param with shape \(80, 191\) "
                                             r"from checkpoint, the shape in current model is \(80, 192\)"):
        flow.load_state_dict(bad)
    with pytest.raises(ValueError):
        flow.load_state_dict(sd, decoder="borrowed")


def test_constructor_rejects_other_architectures():
    from jyutvoice_amd.flow.flow import CausalMaskedDiffWithXvec
    with pytest.raises(NotImplementedError):
        CausalMaskedDiffWithXvec()                                   # the reference's default vocab_size = 4096
    with pytest.raises(NotImplementedError):
        new_flow(output_size=100)
    with pytest.raises(NotImplementedError):
        new_flow(pre_lookahead_len=4)
    from types import SimpleNamespace as NS
    with pytest.raises(NotImplementedError):
        new_flow(encoder=NS(static_chunk_size=16))
    assert new_flow(encoder=NS(static_chunk_size=25)).token_mel_ratio == 2


def _args(B=1, N=6, P=3, F=6):
    return dict(token=torch.zeros(B, N, dtype=torch.int64), token_len=torch.full((B,), N), prompt_token=torch.zeros(B, P, dtype=torch.int64),
                prompt_token_len=torch.full((B,), P), prompt_feat=torch.zeros(B, F, 80), prompt_feat_len=torch.full((B,), F),
                embedding=torch.zeros(B, 192))


def test_inference_errors_before_the_device():
    flow = new_flow()
    with pytest.raises(AssertionError):
        flow.inference(**_args(B=2), streaming=False, finalize=True)
    with pytest.raises(NotImplementedError, match="the reference itself raises TypeError"):
        flow.inference(**_args(), streaming=False, finalize=False)
    # f_b beyond the prompt mel, beyond the utterance, negative: each names the utterance
    a = _args(B=3)
    a["prompt_feat_len"] = torch.tensor([6, 7, 6])
    with pytest.raises(ValueError, match=r"utterance 1: prompt_feat length 7 outside \[0, min\(prompt_feat frames = 6"):
        flow.inference(**a, streaming=False, finalize=True, batched=True)
    a = _args(B=2, N=6, P=3, F=40)
    a["token_len"], a["prompt_token_len"], a["prompt_feat_len"] = torch.tensor([6, 1]), torch.tensor([3, 0]), torch.tensor([18, 3])
    with pytest.raises(ValueError, match=r"utterance 1: prompt_feat length 3 outside \[0, min\(prompt_feat frames = 40, 2 \* tokens = 2\)"):
        flow.inference(**a, streaming=False, finalize=True, batched=True)
    a = _args(B=2)
    a["prompt_feat_len"] = torch.tensor([0, -1])
    with pytest.raises(ValueError, match="utterance 1: prompt_feat length -1"):
        flow.inference(**a, streaming=False, finalize=True, batched=True)
    a = _args(B=2)
    a["token_len"] = torch.tensor([6, 9])
    with pytest.raises(ValueError, match=r"utterance 1: token_len 9 outside \[0, 6\]"):
        flow.inference(**a, streaming=False, finalize=True, batched=True)
    # B = 1 as the reference: mel_len1 = prompt_feat.shape[1], which must fit the sequence
    with pytest.raises(ValueError, match="utterance 0: prompt_feat length 40"):
        flow.inference(**_args(F=40), streaming=False, finalize=True)
    with pytest.raises(RuntimeError, match="load_state_dict"):
        flow.inference(**_args(), streaming=False, finalize=True)      # everything valid, no weights
