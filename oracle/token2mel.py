"""Oracle (test infrastructure): token-to-mel inference of the CosyVoice2 flow -- speech tokens -> mel.

Follows jyutvoice/flow/flow.py:300-358 (CausalMaskedDiffWithXvec.inference, finalize=True), stated as the per-utterance loop
that jyutvoice_amd/flow/flow.py documents for `batched=True`: the reference asserts B = 1, and utterance b of a batch is that
B = 1 call on tensors cut to the utterance's own lengths.

    :315-316  embedding = spk_embed_affine_layer(F.normalize(embedding))
    :319-324  tokens = [prompt_token[:p_b] | token[:n_b]], embedded with ids clamped at 0
    :328,338  h = encoder_proj(encoder(tokens, streaming))                    -> prompt.flow_encoder, T_b = 2 (p_b + n_b) frames
    :337      mel_len1 = f_b (B = 1 reference: prompt_feat.shape[1]), mel_len2 = T_b - f_b
    :341-345  cond = [prompt_feat[:f_b] | 0]
    :347-355  decoder(mu = h, mask = ones, spks, cond, streaming)             -> flow.cfm_solve with flow.estimator(streaming)
    :356      the frames f_b .. T_b - 1 come back

The solver's t_span is the cosine schedule of flow_matching.py:387-389 (`flow.t_span`), its noise the fixed tensor's prefix.
"""
from functools import partial

import torch
import torch.nn.functional as F

from . import flow, prompt


def token2mel(sd, noise, token, token_len, prompt_token, prompt_token_len, prompt_feat, prompt_feat_len, embedding, streaming,
              n_timesteps=10, temperature=1.0, dtype=torch.float32):
    """sd: the module's 1121 keys (`encoder.*`, `input_embedding.weight`, `encoder_proj.*`, `spk_embed_affine_layer.*`,
    `decoder.estimator.*`).  token [B,N], prompt_token [B,P] (or None) int64; prompt_feat [B,F,80] (or None); embedding [B,192];
    the three length vectors hold n_b, p_b, f_b.  -> (mel [B, 80, max_b y_b] float32 with utterance b in [:y_b], zeros behind;
    mel_lengths [B] = y_b = 2 (p_b + n_b) - f_b).  Nothing behind a length is read."""
    B = token.shape[0]
    n = [int(v) for v in token_len]
    p = [int(v) for v in prompt_token_len] if prompt_token is not None and prompt_token.shape[1] > 0 else [0] * B
    f = [int(v) for v in prompt_feat_len] if prompt_feat is not None and prompt_feat.shape[1] > 0 else [0] * B
    if dtype != torch.float32:
        sd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}
    est = partial(flow.estimator, streaming=bool(streaming))
    outs = []
    for b in range(B):
        T = 2 * (p[b] + n[b])
        assert 0 <= f[b] <= T, (b, f[b], T)
        if T == 0:
            outs.append(torch.zeros(80, 0))
            continue
        ids = token[b : b + 1, : n[b]]
        if p[b] > 0:
            ids = torch.cat([prompt_token[b : b + 1, : p[b]], ids], dim=1)
        h, _ = prompt.flow_encoder(sd, ids, torch.tensor([p[b] + n[b]]), streaming=bool(streaming), dtype=dtype)
        spk = F.linear(F.normalize(embedding[b : b + 1].to(dtype), dim=1), sd["spk_embed_affine_layer.weight"],
                       sd["spk_embed_affine_layer.bias"])
        cond = torch.zeros(1, T, 80, dtype=dtype)
        if f[b] > 0:
            cond[:, : f[b]] = prompt_feat[b, : f[b]].to(dtype)
        mask = torch.ones(1, 1, T, dtype=dtype)
        x = flow.cfm_solve(sd, noise.to(dtype), h.to(dtype).transpose(1, 2).contiguous(), mask, spk, cond.transpose(1, 2).contiguous(),
                           n_timesteps, temperature, est=est)
        outs.append(x[0, :, f[b] :])
    y = [o.shape[1] for o in outs]
    mel = torch.zeros(B, 80, max(y))
    for b in range(B):
        mel[b, :, : y[b]] = outs[b]
    return mel, torch.tensor(y)
