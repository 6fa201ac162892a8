"""Inputs of the token-to-mel shape cases, shared by the host test that checks on the oracle alone that they can tell a wrong
condition split from the right one (test_flow_host.py) and the GPU test that holds jv_flow_token2mel to the oracle on them
(test_gpu_token2mel_shapes.py).  Deterministic: tokens from synth.prompt_tokens, the rest from seeded generators."""
import torch

N_TIMESTEPS = 2

# (P, N, F) at B = 1 with the reference's semantics f = prompt_feat.shape[1]: F < 2P, F > 2P, a condition without prompt tokens,
# prompt tokens without a condition.  52 to 60 frames: across the estimator's chunk of 50
SINGLES = [(12, 18, 10), (12, 18, 40), (0, 26, 20), (12, 18, 0)]

# batched=True: totals 51 / 26 / 30 tokens, y_b = 2 (p_b + n_b) - f_b = 62 / 52 / 30
BATCH = dict(P=33, N=26, F=40, p=[33, 0, 12], n=[18, 26, 18], f=[40, 0, 30], y=[62, 52, 30])


def flow_sd(prompt_sd, tts_sd):
    sd = dict(prompt_sd)
    sd.update({k: v for k, v in tts_sd.items() if k.startswith(("decoder.", "spk_embed_affine_layer."))})
    return sd


def single_inputs(P, N, F):
    """-> token [1,N], prompt_token [1,P], prompt_feat [1,F,80], embedding [1,192]"""
    from jyutvoice_amd import synth
    tok, _ = synth.prompt_tokens(1, N, first_index=41 + P)
    ptok, _ = synth.prompt_tokens(1, P, first_index=51 + N)
    g = torch.Generator().manual_seed(100 * P + 10 * N + F)
    return tok, ptok, torch.randn(1, F, 80, generator=g), torch.randn(1, 192, generator=g)


def batch_inputs():
    """-> token [3,N], prompt_token [3,P], prompt_feat [3,F,80], embedding [3,192] (zero ids / random frames behind the lengths)"""
    from jyutvoice_amd import synth
    c = BATCH
    tok, _ = synth.prompt_tokens(3, c["N"], lengths=c["n"], first_index=61)
    ptok, _ = synth.prompt_tokens(3, c["P"], lengths=c["p"], first_index=71)
    g = torch.Generator().manual_seed(8)
    return tok, ptok, torch.randn(3, c["F"], 80, generator=g), torch.randn(3, 192, generator=g)


def oracle_mel(sd, noise, tok, n, ptok, p, feat, f, emb, streaming, moved_split=False):
    """oracle.token2mel on the case.  moved_split: the bug the f != 2p cases exist for -- the split between condition and
    generated frames taken at the prompt's 2 p_b frames instead of f_b (prompt_feat cut there, or continued with zeros)"""
    from oracle import token2mel as ot2m
    if moved_split:
        f = [2 * v for v in p]
        wide = torch.zeros(feat.shape[0], max(max(f), feat.shape[1]), 80)
        wide[:, :feat.shape[1]] = feat
        feat = wide
    return ot2m.token2mel(sd, noise, tok, torch.tensor(n), ptok, torch.tensor(p), feat, torch.tensor(f), emb, streaming,
                          n_timesteps=N_TIMESTEPS)
