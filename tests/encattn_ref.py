"""fp64 restatement of the text encoder's attention core (jyutvoice/models/text_encoder.py:235-248, oracle/textenc.py::mha: scores,
masked_fill(-1e4), softmax, P V) on the row-buffer layout of encoder.hip, for the tests of encattn.hip.  torch on the CPU only.

    s[h, i, j] = q_i . k_j / sqrt(288), masked_fill(mask2d == 0, -1e4), mask2d[i, j] = [i < L] [j < L];  out[i] = softmax_j(s) V

q, k, v are what lies in the qkv buffer: RoPE has been applied (rope_qk is a pass of its own in front of both routes).  The
reference's mask is kept as it is, -1e4 and all: for a query i < L a masked key's probability underflows to exactly 0, in fp64 too,
so the rows i < L of the result read nothing at or behind L.  Rows i >= L are zeros here (the reference leaves an average of V there,
which every consumer masks).

`enc_attention(..., dtype=torch.float32)` is the same expression in fp32 torch: the reference's own arithmetic, the yardstick
where the four-launch route does not reach (T > 512)."""
import math

import torch

HEADS, DK = 2, 288
LDQ, LDO = 3 * HEADS * DK, HEADS * DK      # 1728, 576


def row(G: int, S: int, b: int, t: int) -> int:
    """row of utterance b's token t in a row buffer with G guard rows and utterance stride S"""
    return G + b * S + t


def n_rows(G: int, S: int, B: int) -> int:
    return G + B * S


def split_heads(qkv: torch.Tensor):
    """[T, 1728] -> q, k, v [2, T, 288]: q of head h at columns h*288, k at 576 + h*288, v at 1152 + h*288"""
    T = qkv.shape[0]
    return tuple(qkv[:, o:o + LDO].reshape(T, HEADS, DK).transpose(0, 1) for o in (0, LDO, 2 * LDO))


def enc_attention_one(qkv: torch.Tensor, L: int, dtype=torch.float64) -> torch.Tensor:
    """qkv [T, 1728] -> out [T, 576] in `dtype`; rows i >= L are zeros"""
    T = qkv.shape[0]
    out = torch.zeros(T, LDO, dtype=dtype)
    if L <= 0:
        return out
    q, k, v = split_heads(qkv.to(dtype))
    valid = (torch.arange(T) < L)
    mask2d = valid.unsqueeze(0) & valid.unsqueeze(1)
    s = q @ k.transpose(-2, -1) / math.sqrt(DK)
    s = s.masked_fill(~mask2d, -1e4)
    p = torch.softmax(s, dim=-1)
    o = (p @ v).transpose(0, 1).reshape(T, LDO)
    out[:L] = o[:L]
    return out


def enc_attention(qkv, lens, B: int, T: int, G: int, S: int, dtype=torch.float64) -> torch.Tensor:
    """the operator on row buffers: qkv [rows, 1728] -> out [rows, 576]; utterance b has min(lens[b], T) tokens; rows of no
    utterance stay NaN.  What lies at and behind a length never counts (NaN there is read as 0)."""
    qkv = qkv.detach().cpu()
    out = torch.full((qkv.shape[0], LDO), float("nan"), dtype=dtype)
    for b in range(B):
        L = max(0, min(int(lens[b]), T))
        r = slice(row(G, S, b, 0), row(G, S, b, T))
        x = qkv[r].clone()
        x[L:] = 0.0
        out[r] = enc_attention_one(torch.nan_to_num(x), L, dtype)
    return out
