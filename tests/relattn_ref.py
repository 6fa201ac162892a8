"""fp64 restatement of the UpsampleConformer blocks' relative-position attention (jyutvoice/transformer/attention.py:204-334 with
the masks of utils/mask.py:91-126, 192-198), for the tests of relattn.hip and of the token-to-mel route.  torch on the CPU only.

    s[h, i, j] = ((q_i + u_h) . k_j + (q_i + v_h) . p_h[T - 1 - i + j]) / sqrt(64)
    over keys j < min(L, (i // chunk + 1) * chunk)   (chunk = 0: j < L);   out[i] = softmax_j(s) V

`rel_shift` is done by indexing: column j of the shifted matrix_bd row i is column T - 1 - i + j of the unshifted one."""
import math

import torch

HEADS, DK = 8, 64


def rel_pos_emb(T: int, d: int = 512) -> torch.Tensor:
    """EspnetRelPositionalEncoding's pos_emb for T frames (embedding.py:224-254, 272-296): [2T-1, d], row m holds relative position
    T - 1 - m; the frequencies in fp32 as the reference computes them, the angles and sin / cos in fp64"""
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d)).double()
    r = (T - 1 - torch.arange(2 * T - 1)).double().unsqueeze(1)
    pe = torch.zeros(2 * T - 1, d, dtype=torch.float64)
    pe[:, 0::2] = torch.sin(r * div)
    pe[:, 1::2] = torch.cos(r * div)
    return pe


def key_limit(i: int, L: int, chunk: int) -> int:
    """keys query i sees: subsequent_chunk_mask with all left chunks, ANDed with the padding mask"""
    return min(L, (i // chunk + 1) * chunk) if chunk > 0 else L


def rel_attention_one(q, k, v, p, u, vb, L: int, chunk: int = 0) -> torch.Tensor:
    """q, k, v [T, 512], p [2T-1, 512], u, vb [8, 64] -> out [T, 512] in fp64; rows i >= L are zeros"""
    T = q.shape[0]
    q, k, v, p, u, vb = (t.double() for t in (q, k, v, p, u, vb))
    out = torch.zeros(T, HEADS * DK, dtype=torch.float64)
    if L <= 0:
        return out
    idx = (T - 1 - torch.arange(T).unsqueeze(1) + torch.arange(T).unsqueeze(0))          # [i, j] -> row of p
    jj = torch.arange(T).unsqueeze(0)
    lim = torch.tensor([key_limit(i, L, chunk) for i in range(T)]).unsqueeze(1)
    visible = jj < lim
    for h in range(HEADS):
        sl = slice(h * DK, (h + 1) * DK)
        ac = (q[:, sl] + u[h]) @ k[:, sl].T
        bd_full = (q[:, sl] + vb[h]) @ p[:, sl].T                                        # [T, 2T-1]
        s = (ac + torch.gather(bd_full, 1, idx)) / math.sqrt(DK)
        s = s.masked_fill(~visible, float("-inf"))
        w = torch.softmax(s[:L], dim=-1)
        out[:L, sl] = w @ v[:, sl]
    return out


def rel_attention(qkv, p, u, vb, lens, B: int, T: int, G: int, S: int, len_mul: int = 1, chunk: int = 0) -> torch.Tensor:
    """the operator on row buffers: qkv [rows, 1536] with utterance b's frame t at row G + b*S + t -> out [rows, 512] (fp64);
    utterance b has min(lens[b] * len_mul, T) frames; rows of no utterance stay NaN"""
    qkv = qkv.detach().cpu()
    out = torch.full((qkv.shape[0], 512), float("nan"), dtype=torch.float64)
    for b in range(B):
        L = max(0, min(int(lens[b]) * len_mul, T))
        r = slice(G + b * S, G + b * S + T)
        x = torch.nan_to_num(qkv[r].double())         # what lies behind L is never used: rows >= L get zero weight / zero output
        out[r] = rel_attention_one(x[:, :512], x[:, 512:1024], x[:, 1024:], p.detach().cpu(), u.detach().cpu(), vb.detach().cpu(), L,
                                   chunk)
    return out


def mha(x, w, L: int, chunk: int = 0) -> torch.Tensor:
    """RelPositionMultiHeadedAttention.forward(x, x, x, mask, pos_emb) for one utterance: x [T, 512]; w: the block's tensors by
    their state-dict suffix (linear_q.weight ... pos_bias_v) -> [T, 512] fp64"""
    T = x.shape[0]
    x = x.double()
    lin = lambda n: x @ w[n + ".weight"].double().T + w[n + ".bias"].double()
    p = rel_pos_emb(T) @ w["linear_pos.weight"].double().T
    o = rel_attention_one(lin("linear_q"), lin("linear_k"), lin("linear_v"), p, w["pos_bias_u"], w["pos_bias_v"], L, chunk)
    return o @ w["linear_out.weight"].double().T + w["linear_out.bias"].double()
