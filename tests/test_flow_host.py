"""Host-side checks of the token-to-mel route (no GPU): the fp64 restatement of the relative-position attention against what the
imported reference module computed (G13), the state-dict split, every error `CausalMaskedDiffWithXvec` raises before it
touches the device, and the oracle the GPU tests of the route are held to (oracle/prompt.py with its chunk masks,
oracle/token2mel.py) against what the imported reference computed (G13, G14)."""
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


# ---- the oracle of the token-to-mel route (oracle/prompt.py with streaming, oracle/token2mel.py), pinned on the CPU ---------------

def _md(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.fixture(scope="module")
def g13():
    return load_golden("G13_flow_encoder")


@pytest.fixture(scope="module")
def oracle_h93(prompt_sd, g13):
    """oracle.prompt.flow_encoder on G13's 93 tokens: (streaming, dtype) -> h, computed once"""
    from oracle import prompt as oprompt
    return {(s, d): oprompt.flow_encoder(prompt_sd, g13["tok"], torch.tensor([93]), streaming=s, dtype=d)[0]
            for s in (False, True) for d in (torch.float32, torch.float64)}


def test_oracle_encoder_against_reference(oracle_h93, g13):
    """the restated encoder, with and without its chunk masks (25 tokens / 50 frames), against what the imported
    UpsampleConformerEncoder computed on G13's 93 tokens.  5e-5: the bound the GPU is held to against the same fixture"""
    for tag, streaming in (("full", False), ("stream", True)):
        h = oracle_h93[(streaming, torch.float32)]
        assert h.dtype == torch.float32 and h.shape == (1, 186, 80)
        e = _md(h, g13["h_" + tag])
        print(f"oracle flow_encoder vs G13 ({tag}): {e:.3e}")
        assert e <= 5e-5, tag
    assert _md(oracle_h93[(False, torch.float32)], oracle_h93[(True, torch.float32)]) > 1e-2      # the reference's modes differ by 0.14


def test_oracle_encoder_default_is_unchanged(prompt_sd, g13, oracle_h93):
    """the call bench.py and test_gpu_prompt.py make (no streaming, no dtype) is the fp32 full-context one, bit for bit, and
    ragged batches still loop over the utterances"""
    from oracle import prompt as oprompt
    h, hl = oprompt.flow_encoder(prompt_sd, g13["tok"], torch.tensor([93]))
    assert h.dtype == torch.float32 and hl.tolist() == [186]
    assert torch.equal(h, oracle_h93[(False, torch.float32)])
    two = torch.zeros(2, 30, dtype=torch.int64)
    two[0, :30], two[1, :7] = g13["tok"][0, :30], g13["tok"][0, 40:47]
    hb, hbl = oprompt.flow_encoder(prompt_sd, two, torch.tensor([30, 7]), streaming=True)
    h7, _ = oprompt.flow_encoder(prompt_sd, two[1:, :7], torch.tensor([7]), streaming=True)
    assert hbl.tolist() == [60, 14] and torch.equal(hb[1:, :14], h7) and float(hb[1, 14:].abs().max()) == 0.0


def test_oracle_streaming_property(prompt_sd, g13, oracle_h93):
    """test_streaming_property's numbers on the oracle: rows [0, 100) of 60 vs 93 tokens agree to <= 2e-5 with streaming (the
    reference's own figure is 1.9e-6) and differ by > 1e-3 without (the reference: 5.1e-2)"""
    from oracle import prompt as oprompt
    got = {}
    for streaming in (True, False):
        h60, _ = oprompt.flow_encoder(prompt_sd, g13["tok"][:, :60], torch.tensor([60]), streaming=streaming)
        got[streaming] = _md(h60[:, :100], oracle_h93[(streaming, torch.float32)][:, :100])
    print(f"oracle rows [0, 100) of 60 vs 93 tokens: streaming {got[True]:.3e}  full {got[False]:.3e}")
    assert got[True] <= 2e-5
    assert got[False] > 1e-3


def test_oracle_fp64_form_against_fp32_form(oracle_h93, g13):
    """dtype=float64 is the same statement at higher precision: 2e-5 from the fp32 form in both modes, the bound and the argument
    of test_restated_attention_matches_reference_module (fp32 contractions of order-one operands, outputs of order one; ten
    blocks chained behind LayerNorms do not compound beyond a few 1e-6)"""
    for tag, streaming in (("full", False), ("stream", True)):
        h64 = oracle_h93[(streaming, torch.float64)]
        assert h64.dtype == torch.float64
        e = _md(h64, oracle_h93[(streaming, torch.float32)])
        print(f"oracle flow_encoder fp64 vs fp32 ({tag}): {e:.3e};  fp64 vs G13: {_md(h64, g13['h_' + tag]):.3e}")
        assert e <= 2e-5, tag


def test_oracle_token2mel_against_reference(prompt_sd, tts_sd, noise):
    """oracle.token2mel against the mel of the imported CausalMaskedDiffWithXvec (G14: prompt 33 + 60 tokens, prompt_feat 66
    frames, ten steps), both modes.  1e-3 is the project's mel tolerance, the bound the GPU is held to against this oracle; it
    means something there only because the oracle alone sits far inside it (recorded in tests/golden/README_flow.md)"""
    import token2mel_cases as tc
    from oracle import token2mel as ot2m
    g = load_golden("G14_token2mel")
    sd = tc.flow_sd(prompt_sd, tts_sd)
    for tag, streaming in (("full", False), ("stream", True)):
        mel, ml = ot2m.token2mel(sd, noise, g["token"], torch.tensor([60]), g["prompt_token"], torch.tensor([33]), g["prompt_feat"],
                                 torch.tensor([66]), g["embedding"], streaming)
        assert mel.shape == (1, 80, 120) and mel.dtype == torch.float32 and ml.tolist() == [120]
        e = _md(mel, g["mel_" + tag])
        print(f"oracle token2mel vs G14 ({tag}): {e:.3e}  |mel| {float(mel.abs().max()):.2f}")
        assert e <= 1e-3, tag


@pytest.mark.parametrize("streaming", [False, True])
def test_split_cases_discriminate(prompt_sd, tts_sd, noise, streaming):
    """the f != 2p cases of test_gpu_token2mel_shapes.py can see the bug they exist for: on the oracle alone, the mel with the
    split taken at 2 p_b instead of f_b differs from the right one by more than 1e-2 (ten times the bound the GPU is held to),
    over the frames both return"""
    import token2mel_cases as tc
    sd = tc.flow_sd(prompt_sd, tts_sd)
    for P, N, F in tc.SINGLES:
        assert F != 2 * P
        tok, ptok, feat, emb = tc.single_inputs(P, N, F)
        right, yr = tc.oracle_mel(sd, noise, tok, [N], ptok, [P], feat, [F], emb, streaming)
        wrong, yw = tc.oracle_mel(sd, noise, tok, [N], ptok, [P], feat, [F], emb, streaming, moved_split=True)
        assert yr.tolist() == [2 * (P + N) - F] and yw.tolist() == [2 * N]
        w = min(int(yr[0]), int(yw[0]))
        d = _md(right[:, :, :w], wrong[:, :, :w])
        print(f"(P, N, F) = {(P, N, F)} streaming={streaming}: right vs moved split {d:.3e}")
        assert d > 1e-2, (P, N, F)
    c = tc.BATCH
    tok, ptok, feat, emb = tc.batch_inputs()
    right, yr = tc.oracle_mel(sd, noise, tok, c["n"], ptok, c["p"], feat, c["f"], emb, streaming)
    wrong, yw = tc.oracle_mel(sd, noise, tok, c["n"], ptok, c["p"], feat, c["f"], emb, streaming, moved_split=True)
    assert yr.tolist() == c["y"]
    for b in range(3):
        if c["f"][b] == 2 * c["p"][b]:
            continue
        w = min(int(yr[b]), int(yw[b]))
        d = _md(right[b, :, :w], wrong[b, :, :w])
        print(f"batch utterance {b} streaming={streaming}: right vs moved split {d:.3e}")
        assert d > 1e-2, b
