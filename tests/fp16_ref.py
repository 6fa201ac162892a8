"""Test infrastructure: the estimator of oracle/flow.py restated with the operand rounding of the library's FP16 mode
(jv_flow_set_precision(JV_PRECISION_FP16), Engine.set_precision("fp16")), evaluated in fp64.

In that mode every contraction that runs fp16x3 by default issues the hi x hi product alone: both operands are rounded to fp16 under
exact power-of-two scales and multiplied exactly, the sum is accumulated in fp32.  Here: `round_h` on both operands of every such
contraction, everything else as the oracle computes it --
  * the transformer linears (to_q | to_k | to_v, to_out, ff.net.0, ff.net.2): LayerNorm output / attention output / GELU output
    and the weight rows;
  * attention: Q with its prescale log2(e) / 8 (attention_common.h q_prescale), K, V, and P as the kernel keeps it -- exp of the
    score less the row maximum, a power-of-two multiple of p * 2^10 -- while the normaliser sums the unrounded P (attention_pl.hip);
  * the trunk convolutions: a resnet's block1 / res_conv (not the first resnet's, whose input xin has no tracked bound and stays on
    bf16x6), block2, the down / up / final convolutions and the final projection (masked input rows, weights).
Left alone, as the library leaves them: the time MLP, the resnets' time projections, the first resnet's block1 and res_conv.

The scales are powers of two, so rounding to fp16 under a scale is rounding to 11 significant bits (round to nearest even) --
except below 2^-14 of the scaled range, where fp16 is subnormal and the grid stops shrinking at 2^-24.  `round_h(x, scale)` does
both; the estimator below passes no scale (elements 2^-30 of an operand's bound contribute nothing measurable, and the library's
per-utterance measured scales are not known here: tests/test_gpu_fp16_estimator.py's factor 4 names this).

`estimator(..., R=lambda x: x)` is oracle.flow.estimator (tests/test_fp16_host.py holds the two together)."""
import math

import torch
import torch.nn.functional as F

from oracle import flow as oflow

HEADS = 8
FP16_MAX = 65504.0


def round_h(x, scale=None):
    """x rounded as the hi plane of the fp16x3 split holds it: fp16(x * scale) / scale, computed in fp64 WITHOUT torch's half type
    (round to nearest even on a grid of 2^(e - 11) for |x| in [2^(e-1), 2^e), 2^-24 below 2^-14; beyond 65504 + half a step:
    inf).  scale: a power of two (float or a tensor that broadcasts); None: 11 significant bits, no subnormal range, no overflow."""
    dtype = x.dtype
    x = x.double()
    if scale is not None:
        x = x * scale
    _, e = torch.frexp(x)                      # |x| in [2^(e-1), 2^e)
    if scale is not None:
        e = e.clamp(min=-13)                   # subnormal: the grid of the smallest normal binade
    ulp = torch.ldexp(torch.ones_like(x), e - 11)
    r = torch.round(x / ulp) * ulp             # torch.round: half to even
    if scale is not None:
        r = torch.where(r.abs() > FP16_MAX, torch.copysign(torch.full_like(r, float("inf")), r), r)
        r = r / scale
    return r.to(dtype)      # (exact: 11 bits fit every floating type used here)


def weight_scale(W):
    """registry.hip split2h_kernel: per output row n the power of two with max_k |W[n][k]| * 2^e_n in [2^13, 2^14)"""
    am = W.double().reshape(W.shape[0], -1).abs().amax(dim=1)
    _, ex = torch.frexp(am)
    sc = torch.ldexp(torch.ones_like(am), (14 - ex).clamp(-60, 60))
    sc = torch.where(am > 0, sc, torch.ones_like(sc))
    return sc.reshape((-1,) + (1,) * (W.dim() - 1))


_rounded = {}      # (storage address, shape) -> (the weight, its rounding): a solve rounds every weight once, not once per step


def round_w(W):
    """the weight as its hi plane holds it (per-row scales, through torch's half type like round_fast: test_fp16_host.py holds it to
    round_h), rounded once per tensor"""
    key = (W.data_ptr(), tuple(W.shape), W.dtype)
    hit = _rounded.get(key)
    if hit is None or hit[0] is not W:
        sc = weight_scale(W).to(W.dtype)
        hit = _rounded[key] = (W, (W * sc).float().half().to(W.dtype) / sc)
    return hit[1]


def h3_scale(bound):
    """registry.hip h3_scale_for_bound"""
    s = 2.0 ** min(max(math.floor(math.log2(60000.0 / bound)), -24), 24)
    while bound * s > 60000.0:
        s *= 0.5
    return s


def round_fast(x):
    """round_h under one power-of-two scale for the whole tensor (its largest magnitude into [2^13, 2^14), as weight_scale does per
    row), through torch's half type: what the estimator below uses, because round_h's fp64 grid arithmetic on every activation of
    70 blocks takes minutes.  tests/test_fp16_host.py holds it to round_h."""
    am = float(x.detach().abs().max())
    if not (am > 0.0 and math.isfinite(am)):
        return x
    sc = 2.0 ** min(max(14 - math.frexp(am)[1], -60), 60)
    return ((x * sc).float().half().to(x.dtype)) / sc


def _causal_conv(x, w, b, R, Rw):
    return F.conv1d(F.pad(R(x), (w.shape[2] - 1, 0)), Rw(w), b)


def _causal_block(sd, pre, x, mask, R, Rw):
    h = _causal_conv(x * mask, sd[pre + "block.0.weight"], sd[pre + "block.0.bias"], R, Rw)
    h = F.layer_norm(h.transpose(1, 2), (h.shape[1],), sd[pre + "block.2.weight"], sd[pre + "block.2.bias"], 1e-5)
    return F.mish(h.transpose(1, 2)) * mask


def _resnet(sd, pre, x, mask, temb, R, Rw, first):
    ident = lambda z: z
    R1, Rw1 = (ident, ident) if first else (R, Rw)          # the first resnet reads xin: bf16x6 in both modes
    h = _causal_block(sd, pre + "block1.", x, mask, R1, Rw1)
    h = h + F.linear(F.mish(temb), sd[pre + "mlp.1.weight"], sd[pre + "mlp.1.bias"]).unsqueeze(-1)
    h = _causal_block(sd, pre + "block2.", h, mask, R, Rw)
    return h + F.conv1d(R1(x * mask), Rw1(sd[pre + "res_conv.weight"]), sd[pre + "res_conv.bias"])


def _transformer_block(sd, pre, h, bias, R, Rw):
    B, T, C = h.shape
    R3, Rw3 = R, Rw
    # registry.hip: a block whose LayerNorm1 bound sqrt(255) max|g| + max|b| is unusable (beyond 1e30) keeps its q | k | v, attention
    # and to_out on bf16x6 -- in FP16 mode too (jv_flow_contraction_info)
    if not float(math.sqrt(255.0) * sd[pre + "norm1.weight"].abs().max() + sd[pre + "norm1.bias"].abs().max()) < 1e30:
        R = Rw = lambda z: z
    n = R(F.layer_norm(h, (C,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], 1e-5))
    q = F.linear(n, Rw(sd[pre + "attn1.to_q.weight"]))
    k = F.linear(n, Rw(sd[pre + "attn1.to_k.weight"]))
    v = F.linear(n, Rw(sd[pre + "attn1.to_v.weight"]))
    hd = q.shape[-1] // HEADS
    sp = lambda z: z.view(B, T, HEADS, hd).transpose(1, 2)
    c = 0.125 * 1.44269504088896340736                     # q_prescale without its power-of-two q_scale: scores in base-2 units
    s = (R(sp(q) * c) @ R(sp(k)).transpose(-2, -1)) / 1.44269504088896340736 + bias
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    o = (R(p) @ R(sp(v))) / p.sum(dim=-1, keepdim=True)
    o = o.transpose(1, 2).reshape(B, T, HEADS * hd)
    h = h + F.linear(R(o), Rw(sd[pre + "attn1.to_out.0.weight"]), sd[pre + "attn1.to_out.0.bias"])
    R, Rw = R3, Rw3
    n = R(F.layer_norm(h, (C,), sd[pre + "norm3.weight"], sd[pre + "norm3.bias"], 1e-5))
    f = F.gelu(F.linear(n, Rw(sd[pre + "ff.net.0.proj.weight"]), sd[pre + "ff.net.0.proj.bias"]))
    return h + F.linear(R(f), Rw(sd[pre + "ff.net.2.weight"]), sd[pre + "ff.net.2.bias"])


def estimator(sd, x, mask, mu, t, spks, cond, pre="decoder.estimator.", streaming=False, chunk=50, R=round_fast, Rw=None):
    """oracle.flow.estimator with R on the activation operand and Rw (default: round_w; with R the identity: the identity) on the
    weight operand of every contraction the FP16 mode covers.  Same arguments and result."""
    if Rw is None:
        Rw = round_w if R in (round_h, round_fast) else R
    temb = oflow.time_embedding(sd, t, pre)
    T = x.shape[2]
    h = torch.cat([x, mu, spks.unsqueeze(-1).expand(-1, -1, T), cond], dim=1)
    allowed = mask.bool().unsqueeze(1)
    if streaming:
        i = torch.arange(T)
        allowed = allowed & (i[None, :] < ((i // chunk + 1) * chunk)[:, None])[None, None]
    bias = (1.0 - allowed.to(x.dtype)) * -1.0e10

    def stage(prefix, h, first=False):
        h = _resnet(sd, prefix + "0.", h, mask, temb, R, Rw, first)
        g = h.transpose(1, 2).contiguous()
        for j in range(4):
            g = _transformer_block(sd, prefix + f"1.{j}.", g, bias, R, Rw)
        return g.transpose(1, 2).contiguous()

    h = stage(pre + "down_blocks.0.", h, first=True)
    skip = h
    h = _causal_conv(h * mask, sd[pre + "down_blocks.0.2.weight"], sd[pre + "down_blocks.0.2.bias"], R, Rw)
    n_mid = 1 + max(int(k[len(pre):].split(".")[1]) for k in sd if k.startswith(pre + "mid_blocks."))
    for i in range(n_mid):
        h = stage(pre + f"mid_blocks.{i}.", h)
    h = stage(pre + "up_blocks.0.", torch.cat([h, skip], dim=1))
    h = _causal_conv(h * mask, sd[pre + "up_blocks.0.2.weight"], sd[pre + "up_blocks.0.2.bias"], R, Rw)
    h = _causal_block(sd, pre + "final_block.", h, mask, R, Rw)
    out = F.conv1d(R(h * mask), Rw(sd[pre + "final_proj.weight"]), sd[pre + "final_proj.bias"])
    return out * mask


def decoder64(sd):
    return {k: v.double() for k, v in sd.items() if k.startswith("decoder.")}


def streaming_est(est, chunk=50):
    """est with streaming=True bound (oracle.flow.cfm_solve passes `pre` only)"""
    return lambda sd, x, mask, mu, t, spks, cond, pre="decoder.estimator.": est(sd, x, mask, mu, t, spks, cond, pre=pre, streaming=True,
                                                                                chunk=chunk)


# ---- the cases of tests/test_gpu_fp16_estimator.py and tests/golden/make_golden_fp16.py ------------------------------------------
T_EST = 0.35                     # the timestep of the single estimator evaluations
CASES = {
    # name: (seed, T, lengths, Euler steps, streaming chunk, utterances the fp64 oracle is run on)
    "i": (101, 64, (57,), 10, 0, (0,)),
    "ii": (202, 120, (70, 119, 83, 101, 77, 110, 94, 89, 117, 105, 73), 3, 0, (0, 1)),
    "iii": (101, 64, (57,), 10, 50, (0,)),
    # on synth.hostile_tts_state_dict(fixed_duration=1.5, unusable_bound=True), the checkpoint of tests/test_gpu_hostile.py
    "hostile": (303, 64, (57,), 10, 0, (0,)),
}


def case_state_dict(name):
    from jyutvoice_amd import synth
    return synth.hostile_tts_state_dict(fixed_duration=1.5, unusable_bound=True) if name == "hostile" else synth.tts_state_dict()


def case_inputs(name):
    """seeded fp32 inputs of a case: x (the evaluation's noisy mel), mu [B,80,T], spks [B,80], lens"""
    seed, T, lens, steps, chunk, utts = CASES[name]
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    return {"x": torch.randn(B, 80, T, generator=g), "mu": torch.randn(B, 80, T, generator=g), "spks": torch.randn(B, 80, generator=g),
            "lens": torch.tensor(lens, dtype=torch.int32), "T": T, "steps": steps, "chunk": chunk, "utts": utts}


def cfg_batch(c, utts=None, dtype=torch.float32):
    """the 2 B rows a solve evaluates -- conditional rows, then their unconditional twins (mu = spks = cond = 0) -- of the
    utterances `utts` (default all): x, mask, mu, t, spks, cond"""
    idx = list(range(len(c["lens"]))) if utts is None else list(utts)
    x, mu, spks = (c[k][idx].to(dtype) for k in ("x", "mu", "spks"))
    T = c["T"]
    mask = (torch.arange(T)[None, :] < c["lens"][idx][:, None]).to(dtype).unsqueeze(1)
    z = torch.zeros_like(mu)
    return (torch.cat([x, x]), torch.cat([mask, mask]), torch.cat([mu, z]), torch.full((2 * len(idx),), T_EST, dtype=dtype),
            torch.cat([spks, torch.zeros_like(spks)]), torch.cat([z, z]))


def valid_dist(a, b, lens):
    """max |a - b| over the valid frames of [n, 80, T] tensors (lens [n])"""
    T = a.shape[2]
    m = (torch.arange(T)[None, :] < torch.as_tensor(lens)[:, None]).unsqueeze(1)
    return float(((a.double().cpu() - b.double().cpu()).abs() * m).max())
