#!/usr/bin/env python3
"""Generate the token-to-mel fixtures by running the REFERENCE's own `CausalMaskedDiffWithXvec` (jyutvoice/flow/flow.py:187-358)
on the CPU (build container only, like make_golden.py, whose import stubs and module construction this script reuses).

    python tests/golden/make_golden_flow.py            # needs the reference tree; writes G13_flow_encoder.npz, G14_token2mel.npz

flow.py imports `omegaconf.DictConfig` for a default argument only; omegaconf is absent here, so a one-line stub
(`DictConfig = dict`) stands in.  The class is built around the imported UpsampleConformerEncoder and the imported
CausalConditionalCFM, and loads `synth.prompt_state_dict()` plus the `decoder.*` / `spk_embed_affine_layer.*` tensors of
`synth.tts_state_dict()` with strict=True: 1121 keys = 206 encoder + 910 decoder + 5.

G13  h = encoder_proj(encoder(embedding(token) * mask, streaming)) for 93 tokens (three chunks of 25, the last one partial), both
     streaming values; and, for the CPU test of tests/relattn_ref.py, what the first block's RelPositionMultiHeadedAttention
     (encoders.0.self_attn) received and returned in both runs: its input x (the same in both), out_full, out_stream.
G14  inference(token 60, prompt_token 33, prompt_feat 66 frames, embedding, streaming, finalize=True) for both streaming values,
     with the inputs.
"""
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg      # noqa: E402  (also puts the repository root on sys.path)


def build_flow():
    """the imported CausalMaskedDiffWithXvec with the synthetic weights, and the two state-dicts it was loaded from"""
    _, _, cfm, _ = mg.build_reference()
    omegaconf = types.ModuleType("omegaconf")
    omegaconf.DictConfig = dict
    sys.modules["omegaconf"] = omegaconf
    from jyutvoice.flow.flow import CausalMaskedDiffWithXvec
    from jyutvoice.transformer.upsample_encoder import UpsampleConformerEncoder

    from jyutvoice_amd import synth
    uce = UpsampleConformerEncoder(output_size=512, attention_heads=8, linear_units=2048, num_blocks=6, dropout_rate=0.1,
                                   positional_dropout_rate=0.1, attention_dropout_rate=0.1, normalize_before=True,
                                   input_layer="linear", pos_enc_layer_type="rel_pos_espnet",
                                   selfattention_layer_type="rel_selfattn", input_size=512, use_cnn_module=False,
                                   macaron_style=False, static_chunk_size=25)
    flow = CausalMaskedDiffWithXvec(input_size=512, output_size=80, spk_embed_dim=192, output_type="mel", vocab_size=6561,
                                    input_frame_rate=25, only_mask_loss=True, token_mel_ratio=2, pre_lookahead_len=3,
                                    encoder=uce, decoder=cfm).eval()
    psd, tsd = synth.prompt_state_dict(), synth.tts_state_dict()
    sd = dict(psd)
    sd.update({k: v for k, v in tsd.items() if k.startswith(("decoder.", "spk_embed_affine_layer."))})
    assert len(sd) == 1121, len(sd)
    flow.load_state_dict(sd, strict=True)
    return flow, sd


@torch.inference_mode()
def main():
    from jyutvoice_amd import synth
    torch.manual_seed(20240608)
    flow, _ = build_flow()
    from jyutvoice.utils.mask import make_pad_mask      # (importable once build_reference has installed the package stubs)

    # ---- G13 ------------------------------------------------------------------------------------------------------------
    tok, lens = synth.prompt_tokens(1, 93, first_index=13)
    seen = {}
    att = flow.encoder.encoders[0].self_attn
    hook = att.register_forward_hook(lambda m, args, kwargs, out: seen.setdefault("calls", []).append((args, kwargs, out)),
                                     with_kwargs=True)
    g13 = {"tok": tok}
    for tag, streaming in (("full", False), ("stream", True)):
        m = (~make_pad_mask(lens)).float().unsqueeze(-1)
        h, _ = flow.encoder(flow.input_embedding(torch.clamp(tok, min=0)) * m, lens, streaming=streaming)
        g13["h_" + tag] = flow.encoder_proj(h)
        args, kwargs, out = seen["calls"][-1]
        x = args[0] if args else kwargs["query"]
        g13["attn_out_" + tag] = out[0]
        if "attn_x" in g13:
            assert torch.equal(g13["attn_x"], x)      # the first block's input does not depend on the mask
        g13["attn_x"] = x
    hook.remove()
    assert g13["h_full"].shape == (1, 186, 80)
    print("G13 streaming vs full, max abs:", mg.maxdiff(g13["h_full"], g13["h_stream"]))
    print("G13 streaming property: rows [0, 100) of 60 vs 93 tokens:")
    for streaming in (False, True):
        m60 = (~make_pad_mask(torch.tensor([60]))).float().unsqueeze(-1)
        h60, _ = flow.encoder(flow.input_embedding(torch.clamp(tok[:, :60], min=0)) * m60, torch.tensor([60]), streaming=streaming)
        h60 = flow.encoder_proj(h60)
        print("   streaming =", streaming, mg.maxdiff(h60[:, :100], g13["h_stream" if streaming else "h_full"][:, :100]))
    mg.save("G13_flow_encoder", **g13)

    # ---- G14 ------------------------------------------------------------------------------------------------------------
    ptok, _ = synth.prompt_tokens(1, 33, first_index=14)
    tok14, _ = synth.prompt_tokens(1, 60, first_index=15)
    g = torch.Generator().manual_seed(14)
    prompt_feat = torch.randn(1, 66, 80, generator=g)
    embedding = torch.randn(1, 192, generator=g)
    g14 = {"prompt_token": ptok, "token": tok14, "prompt_feat": prompt_feat, "embedding": embedding}
    for tag, streaming in (("full", False), ("stream", True)):
        mel, _ = flow.inference(tok14, torch.tensor([60]), ptok, torch.tensor([33]), prompt_feat, torch.tensor([66]), embedding,
                                streaming, True)
        assert mel.shape == (1, 80, 120)
        g14["mel_" + tag] = mel
    print("G14 streaming vs full, max abs:", mg.maxdiff(g14["mel_full"], g14["mel_stream"]))
    try:
        flow.inference(tok14, torch.tensor([60]), ptok, torch.tensor([33]), prompt_feat, torch.tensor([66]), embedding, False, False)
    except TypeError as e:
        print("finalize=False:", type(e).__name__, e)
    mg.save("G14_token2mel", **g14)


if __name__ == "__main__":
    main()
