"""CPU: tests/encattn_ref.py (the fp64 restatement the GPU tests of encattn.hip measure against) is the reference's attention.

The restatement covers text_encoder.py:235-248 on the row-buffer layout; oracle.textenc.mha is the whole of :216-248.  The test
feeds both the same activations through a layer's real conv_q / conv_k / conv_v (and conv_o behind) and compares.

Tolerance: the oracle runs in fp32.  Its contractions are 576 (q, k, v), 288 (scores), T (P V) and 576 (conv_o) terms of order one
or below, each accumulating about eps * sqrt(n) = 6e-8 * 24 = 1.5e-6 of relative error; 1e-4 absolute on outputs of order one is a
generous ceiling for that and four orders of magnitude below what a wrong column, head or mask gives."""
import torch
import torch.nn.functional as F

import encattn_ref as ref

PRE = "encoder.encoder.attn_layers.0."


def roped_qkv_rows(sd, x):
    """x [1, 576, T] -> the [T, 1728] row buffer rope_qk leaves: q | k | v, each 2 heads of 288, RoPE on the first 144 dims of q, k"""
    from oracle import textenc as otext
    T = x.shape[2]
    lin = lambda n: F.conv1d(x, sd[PRE + n + ".weight"], sd[PRE + n + ".bias"])
    sp = lambda z: z.view(1, 2, 288, T).transpose(2, 3)                   # b h t c
    q, k, v = sp(lin("conv_q")), sp(lin("conv_k")), sp(lin("conv_v"))
    q, k = otext.rope(q, 144), otext.rope(k, 144)
    flat = lambda z: z[0].transpose(0, 1).reshape(T, 576)                 # t, (h c)
    return torch.cat([flat(q), flat(k), flat(v)], dim=1)


def test_restatement_is_the_oracles_attention(tts_sd):
    from oracle import textenc as otext
    g = torch.Generator().manual_seed(3)
    for T, L in ((1, 1), (37, 37), (70, 41)):
        valid = (torch.arange(T) < L).float()
        x = torch.randn(1, 576, T, generator=g) * valid
        mask2d = (valid.unsqueeze(0) * valid.unsqueeze(1)).view(1, 1, T, T)
        want = otext.mha(tts_sd, PRE, x, mask2d)[0].transpose(0, 1)       # [T, 576]
        att = ref.enc_attention_one(roped_qkv_rows(tts_sd, x), L)
        got = att @ tts_sd[PRE + "conv_o.weight"][:, :, 0].double().T + tts_sd[PRE + "conv_o.bias"].double()
        err = float((got[:L] - want[:L].double()).abs().max())
        print(f"T={T} L={L}: restatement against oracle.textenc.mha {err:.3e}")
        assert err <= 1e-4
        assert float(att[L:].abs().max()) == 0.0 if L < T else True
        # the fp32 form is the same expression
        att32 = ref.enc_attention_one(roped_qkv_rows(tts_sd, x), L, torch.float32)
        assert att32.dtype == torch.float32 and float((att32.double() - att).abs().max()) <= 1e-5


def test_masked_keys_have_exactly_zero_weight():
    """what lies at and behind L cannot reach a row in front of it: the -1e4 fill underflows to probability 0, in fp64 too"""
    g = torch.Generator().manual_seed(4)
    T, L = 50, 33
    qkv = torch.randn(T, ref.LDQ, generator=g)
    other = qkv.clone()
    other[L:] = torch.randn(T - L, ref.LDQ, generator=g) * 3.0
    assert torch.equal(ref.enc_attention_one(qkv, L)[:L], ref.enc_attention_one(other, L)[:L])


def test_row_layout_helpers():
    G, S, B, T = 4, 14, 3, 10
    assert ref.row(G, S, 0, 0) == 4 and ref.row(G, S, 2, 9) == 4 + 28 + 9 and ref.n_rows(G, S, B) == 46
    qkv = torch.full((ref.n_rows(G, S, B), ref.LDQ), float("nan"))
    g = torch.Generator().manual_seed(5)
    for b in range(B):
        qkv[ref.row(G, S, b, 0):ref.row(G, S, b, T)] = torch.randn(T, ref.LDQ, generator=g)
    lens = [10, 0, 4]
    out = ref.enc_attention(qkv, lens, B, T, G, S)
    assert out.shape == (46, ref.LDO)
    own = torch.zeros(46, dtype=torch.bool)
    for b in range(B):
        own[ref.row(G, S, b, 0):ref.row(G, S, b, T)] = True
    assert torch.isnan(out[~own]).all() and torch.isfinite(out[own]).all()
    for b, L in enumerate(lens):
        r0 = ref.row(G, S, b, 0)
        assert float(out[r0 + L:r0 + T].abs().max()) == 0.0 if L < T else True
        if L:      # an utterance alone, T = L (fp64 rounding of another matmul shape)
            assert float((out[r0:r0 + L] - ref.enc_attention_one(qkv[r0:r0 + L], L)).abs().max()) <= 1e-12
    q, k, v = ref.split_heads(qkv[4:14])
    assert q.shape == (2, 10, 288) and torch.equal(k[1, 3], qkv[7, 576 + 288:576 + 576]) and torch.equal(v[0, 0], qkv[4, 1152:1440])
