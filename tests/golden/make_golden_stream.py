#!/usr/bin/env python3
"""Generate the partial token-to-mel fixture by composing the REFERENCE's own modules the way its `finalize=False` branch intends
(jyutvoice/flow/flow.py:327-336; the branch itself raises TypeError, see make_golden_flow.py).  Build container only.

    python tests/golden/make_golden_stream.py            # needs the reference tree; writes G15_flow_partial.npz

`make_golden_flow.build_flow()` builds the imported CausalMaskedDiffWithXvec with the synthetic weights.  On m = 40 tokens (P = 7
prompt tokens + 33), so L = 37 encoded tokens -- deliberately not a multiple of the 25-token chunk -- the imported modules are called
in the order of UpsampleConformerEncoder.forward (upsample_encoder.py:332-375), with the one change the branch asks for:

    xs, pos_emb, masks = encoder.embed(all 40 embedded tokens)              row-wise, as forward_chunk embeds its context (:446-453)
    xs, context = xs[:, :L], xs[:, L:]
    chunk masks on L                                                        add_optional_chunk_mask (:338-346)
    xs, _ = encoder.pre_lookahead_layer(xs, context=context)                context in place of the zero padding (:110-121)
    forward_layers, up_layer, up_embed, chunk masks on 2 L, forward_up_layers, after_norm; flow.encoder_proj

for both streaming values; then the imported decoder as flow.py:341-356 does, with F = 14 prompt frames.

G15  token [1,33], prompt_token [1,7], prompt_feat [1,14,80], embedding [1,192]; h_full / h_stream [1,74,80];
     mel_full / mel_stream [1,80,60].
"""
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg            # noqa: E402
import make_golden_flow as mgf      # noqa: E402


def partial_encoder(flow, ids, streaming, lookahead=3):
    """h [1, 2 L, 80] of the first L = m - 3 tokens with the last three as the look-ahead layer's context"""
    from jyutvoice.utils.mask import add_optional_chunk_mask, make_pad_mask
    enc = flow.encoder
    m = ids.shape[1]
    L = m - lookahead
    x = flow.input_embedding(torch.clamp(ids, min=0))
    xs, pos_emb, masks = enc.embed(x[:, :L], ~make_pad_mask(torch.tensor([L]), L).unsqueeze(1))
    context, _, _ = enc.embed(x[:, L:], torch.ones(1, 1, lookahead, dtype=torch.bool))
    chunk_masks = add_optional_chunk_mask(xs, masks, False, False, 0, enc.static_chunk_size if streaming else 0, -1)
    xs, _ = enc.pre_lookahead_layer(xs, context=context)
    xs = enc.forward_layers(xs, chunk_masks, pos_emb, masks)
    xs, lens, _ = enc.up_layer(xs.transpose(1, 2).contiguous(), torch.tensor([L]))
    xs = xs.transpose(1, 2).contiguous()
    masks = ~make_pad_mask(lens, xs.size(1)).unsqueeze(1)
    xs, pos_emb, masks = enc.up_embed(xs, masks)
    chunk_masks = add_optional_chunk_mask(xs, masks, False, False, 0, enc.static_chunk_size * enc.up_layer.stride if streaming else 0, -1)
    xs = enc.forward_up_layers(xs, chunk_masks, pos_emb, masks)
    if enc.normalize_before:
        xs = enc.after_norm(xs)
    return flow.encoder_proj(xs)


def partial_mel(flow, h, prompt_feat, embedding, streaming):
    """flow.py:315-316, 337-356 on h"""
    from jyutvoice.utils.mask import make_pad_mask
    emb = flow.spk_embed_affine_layer(F.normalize(embedding, dim=1))
    len1, total = prompt_feat.shape[1], h.shape[1]
    conds = torch.zeros(1, total, flow.output_size)
    conds[:, :len1] = prompt_feat
    mask = (~make_pad_mask(torch.tensor([total]))).to(h)
    feat, _ = flow.decoder(mu=h.transpose(1, 2).contiguous(), mask=mask.unsqueeze(1), spks=emb, cond=conds.transpose(1, 2),
                           n_timesteps=10, streaming=streaming)
    return feat[:, :, len1:].float()


@torch.inference_mode()
def main():
    from jyutvoice_amd import synth
    torch.manual_seed(20240615)
    flow, _ = mgf.build_flow()
    ptok, _ = synth.prompt_tokens(1, 7, first_index=16)
    tok, _ = synth.prompt_tokens(1, 33, first_index=17)
    g = torch.Generator().manual_seed(15)
    prompt_feat = torch.randn(1, 14, 80, generator=g)
    embedding = torch.randn(1, 192, generator=g)
    ids = torch.cat([ptok, tok], dim=1)
    g15 = {"prompt_token": ptok, "token": tok, "prompt_feat": prompt_feat, "embedding": embedding}
    for tag, streaming in (("full", False), ("stream", True)):
        h = partial_encoder(flow, ids, streaming)
        assert h.shape == (1, 74, 80)
        g15["h_" + tag] = h
        g15["mel_" + tag] = partial_mel(flow, h, prompt_feat, embedding, streaming)
        assert g15["mel_" + tag].shape == (1, 80, 60)
        # what the context buys: the same 37 tokens through the module's own forward(), zero padding behind the end
        hz, _ = flow.encoder(flow.input_embedding(torch.clamp(ids[:, :37], min=0)), torch.tensor([37]), streaming=streaming)
        print(f"G15 {tag}: h with context vs zero padding, max abs {mg.maxdiff(h, flow.encoder_proj(hz)):.3e}")
    print("G15 streaming vs full, max abs: h", mg.maxdiff(g15["h_full"], g15["h_stream"]), "mel", mg.maxdiff(g15["mel_full"], g15["mel_stream"]))
    mg.save("G15_flow_partial", **g15)


if __name__ == "__main__":
    main()
