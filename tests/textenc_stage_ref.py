"""One plain reference per stage of the text encoder and the duration predictor (encoder.hip encoder_fwd, encops.hip), shared by
test_gpu_textenc_stages.py (the stages of jv_encoder_fwd_tap against them) and test_textenc_stage_refs_host.py (the references
against oracle.textenc, and what mistakes they catch).  A plain module, not a conftest; it does not import the engine.

Plain torch in `dtype`: fp64 is the reference, fp32 on the CPU the floor.  Every function maps the PREVIOUS stages' tensors of one
batch ([B, C, Tt], channels first, zeros at and behind every length: what a tap returns) to its stage, masked the same way; `mut`
is one deliberate mistake.  Convolutions are F.conv1d, embeddings F.embedding, the norms oracle.textenc.channel_layernorm, attention
the masked softmax expression.

RoPE's angle table.  The model computes theta = 1 / 10000^(2i/144) and the angle t theta in fp32 (text_encoder.py:119,
oracle.textenc.rope) and rope_kernel mirrors that, so the fp32 angle is part of the OPERATION, in any dtype: the fp64 reference of
QKVi takes cos / sin in fp64 OF THE FP32 ANGLE (table="exact", the default).  An angle computed in fp64 would differ from the fp32
one by up to 2^-24 t theta -- 3e-5 rad at t = 512 -- and the stage's floor would then measure that rounding and not the kernel.  The
fp32 evaluation (the floor) takes cosf / sinf of the same fp32 angle, which is oracle.textenc.rope to the bit.  oracle.textenc.rope
in fp64 multiplies fp64 activations by the FP32-rounded cos / sin: table="oracle" does that, so that the composition test can hold
the chain of these formulas to the oracle at 1e-10; the two tables differ by one fp32 rounding of cos / sin, which the host test
bounds."""
import functools
import math

import torch
import torch.nn.functional as F

from jyutvoice_amd import spec, synth
from oracle import textenc as otext

LAYERS, HEADS, HEAD_DIM, ROPE_DIM = spec.ENC_LAYERS, spec.ENC_HEADS, spec.ENC_HEAD_DIM, spec.ENC_ROPE_DIM
LAYER_TAPS = ("QKV", "ATT", "N1", "FF", "N2")
TAPS = (("EMB", "PRE0", "PRE1", "PRE2", "H0") + tuple(f"{n}{i}" for i in range(LAYERS) for n in LAYER_TAPS)
        + ("XD", "D1", "D2"))      # execution order: the ids 0 .. 37 of JV_ENC_TAP_*
OUTPUTS = ("X", "MU", "LOGW", "SPK")      # jv_encoder_fwd's own outputs (SPK: the speaker projection [B, 80], kept as [B, 80, 1])
STAGES = TAPS + OUTPUTS
CHANNELS = {"EMB": 192, "PRE0": 192, "PRE1": 192, "PRE2": 192, "H0": 576, "XD": 576, "D1": 256, "D2": 256, "X": 576, "MU": 80,
            "LOGW": 1, "SPK": 80}
for _i in range(LAYERS):
    CHANNELS.update({f"QKV{_i}": 1728, f"ATT{_i}": 576, f"N1{_i}": 576, f"FF{_i}": 768, f"N2{_i}": 576})
# what each stage reads: earlier stages, or "in" (the ids, the lengths and the speaker vectors of the batch)
SOURCES = {"EMB": ("in",), "PRE0": ("EMB",), "PRE1": ("PRE0",), "PRE2": ("PRE1",), "H0": ("EMB", "PRE2", "in"),
           "X": (f"N2{LAYERS - 1}",), "MU": ("X",), "XD": ("X", "in"), "D1": ("XD",), "D2": ("D1",), "LOGW": ("D2",), "SPK": ("in",)}
for _i in range(LAYERS):
    _h = "H0" if _i == 0 else f"N2{_i - 1}"
    SOURCES.update({f"QKV{_i}": (_h,), f"ATT{_i}": (f"QKV{_i}",), f"N1{_i}": (_h, f"ATT{_i}"), f"FF{_i}": (f"N1{_i}",),
                    f"N2{_i}": (f"N1{_i}", f"FF{_i}")})
# the stages of a text beyond 512 tokens: layer 0 and what surrounds the stack; the last layer's output is read as well, as the
# source X is held to (LONG_SOURCE_ONLY: taken, not compared -- its own sources are not)
LONG_SOURCE_ONLY = (f"N2{LAYERS - 1}",)
LONG_STAGES = (("EMB", "PRE0", "PRE1", "PRE2", "H0") + tuple(f"{n}0" for n in LAYER_TAPS) + LONG_SOURCE_ONLY + ("XD", "D1", "D2")
               + OUTPUTS)

# ---------------------------------------------------------------------------------------------------------------------------------
# cases: name -> (first utterance index of synth.batch, Tt, lengths); ids at padded positions are 0, which is in range
CASES = {
    "t1": (300, 1, (1,)),                   # every tap of the k5 / k3 convolutions but the centre reads lead or gap rows
    "t2": (310, 2, (2, 1)),
    "ragged37": (200, 37, (37, 36, 1)),     # an utterance end one row from its neighbour's gap (test_gpu_edges.py's batch)
    "dead": (320, 5, (5, 0, 3)),            # a dead utterance between live ones
    "pad33": (330, 33, (33, 32)),           # the score buffer's ld = 64 != Tt: the zero padding enc_softmax / transpose_v owe P V
    "lanes129": (340, 129, (129, 64, 65)),  # lengths on and across the softmax's 64-lane stride and the transposes' 32-tiles
    "mags": (350, 20, (20, 20, 20)),        # spk_embed of the three utterances scaled by MAG_SCALES
    "long513": (360, 513, (513,)),          # the fused route alone; RoPE positions beyond 512
}
MAG_SCALES = (1.0, 30.0, 0.03)
SHORT_CASES = tuple(k for k in CASES if k != "long513")


def stages_of(name):
    return LONG_STAGES if name == "long513" else STAGES


@functools.lru_cache(maxsize=None)
def inputs(name):
    """the batch of a case: synth.batch's dict (x, lang, tone, word_pos, syllable_pos, spk_embed, x_lengths)"""
    first, Tt, lens = CASES[name]
    b = synth.batch(len(lens), Tt, first_index=first, lengths=list(lens))
    if name == "mags":
        b["spk_embed"] = b["spk_embed"] * torch.tensor(MAG_SCALES)[:, None]
    return b


def only(b, i):
    """utterance i of a batch alone, at the same Tt"""
    return {k: v[i:i + 1] for k, v in b.items()}


@functools.lru_cache(maxsize=None)
def checkpoint():
    return synth.tts_state_dict()


@functools.lru_cache(maxsize=None)
def weights():
    """{dtype: the encoder's, the duration predictor's and the speaker projection's weights}"""
    sd = {k: v for k, v in checkpoint().items() if k.startswith(("encoder.", "dp.", "spk_embed_affine_layer."))}
    return {torch.float32: sd, torch.float64: {k: v.double() for k, v in sd.items()}}


def live(stage, L):
    """positions of a stage that an utterance of L tokens owns (the speaker projection: its one row, whatever L)"""
    return 1 if stage == "SPK" else L


def rows_of(t, b, n):
    """[B, C, T] -> the first n positions of utterance b as rows [n, C]"""
    return t[b, :, :n].T


# The bound.  test_gpu_fused_ops.RATIO = 8 (4 x for the significant bits, 2 x for the summation order inside the MFMAs) was
# established on contractions of up to K = 1024 products per output.  Two derived departures, each recorded in the JSON:
#
# * LONG_K: the feed-forward's hidden rows FFi = ReLU(conv_1), a k3 convolution over 576 channels: K = 1728 products per output,
#   read straight behind the contraction.  conv_gemm's bf16x6 loop accumulates all K products of an output in ONE fp32 chain
#   inside the MFMAs (conv_gemm_x6_kernel.h: "the MFMA accumulates in fp32"); the rounding error of an fp32 chain grows as the
#   square root of its length (random-walk model; Higham, Accuracy and Stability of Numerical Algorithms, 2.8), while the CPU
#   floor sums in blocked vector lanes and barely grows.  The bound therefore scales by sqrt(K / 1024): 8 x 1.30 = 10.4.
#   Measured: the worst of the 193 FF entries at 8.10 x its floor (FF5, lanes129 utterance 1; median 4.99), and jv_op_conv_gemm
#   ALONE on that stage's rows returns the stage's bits (test_long_contraction_alone): it is the contraction's arithmetic, not
#   the stage's.  The other stages behind long contractions (N2i behind conv_2, K = 2304; D1, K = 1728) sit behind a LayerNorm
#   and stay at 8 x.
# * FLOOR_MIN: a row of logw is ONE number, so its fp32 floor is one draw of one rounding and can be arbitrarily small (t1:
#   7.3e-9, against a kernel distance of 1.03e-7, less than one ulp).  No kernel that stores fp32 can promise less than half an
#   ulp, 2^-24 of the value: the floor of a one-channel row is taken as at least that.
RATIO = 8.0
LONG_K = {"FF": 1728}
FLOOR_MIN = {"LOGW": 2.0 ** -24}


def ratio_of(stage):
    """the multiple of its fp32 floor a stage is held to"""
    kind = stage[:-1]
    return RATIO * math.sqrt(LONG_K[kind] / 1024.0) if kind in LONG_K else RATIO


def floor_of(stage, fl):
    return max(fl, FLOOR_MIN.get(stage, 0.0))


def moved(stage):
    """the columns of a stage that only move data (an fp32 floor of zero: held torch.equal), or None"""
    return slice(0, 576) if stage == "X" else slice(192, 576) if stage == "H0" else None


# ---------------------------------------------------------------------------------------------------------------------------------
def x_mask(lens, T, dtype):
    return (torch.arange(T)[None, :] < torch.as_tensor(lens)[:, None]).unsqueeze(1).to(dtype)


def layernorm(x, g, b, mut=None):
    if mut not in ("ln_eps", "ln_unbiased"):
        return otext.channel_layernorm(x, g, b, spec.ENC_LN_EPS)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    if mut == "ln_unbiased":
        var = var * x.shape[1] / (x.shape[1] - 1)
    return (x - mean) * torch.rsqrt(var + (1e-5 if mut == "ln_eps" else spec.ENC_LN_EPS)) * g.view(1, -1, 1) + b.view(1, -1, 1)


def conv(w, name, x, m, lens, mut=None):
    """the model's masked convolution: conv1d(x * mask, padding k // 2)"""
    x = x * m
    if mut == "tap_off":          # every tap one row early
        x = F.pad(x, (1, 0))[..., :-1]
    if mut == "unmasked":         # what lies behind an utterance's end is read: there, a copy of its last live column
        x = x.clone()
        for b, L in enumerate(lens):
            if 0 < L < x.shape[2]:
                x[b, :, L:] = x[b, :, L - 1:L]
    W = w[name + ".weight"]
    return F.conv1d(x, W, w[name + ".bias"], padding=W.shape[2] // 2)


def rope(x, dtype, table="exact", mut=None):
    """x [B, H, T, 288]: the first 144 dims rotated in half-split pairs (i, i + 72) by the fp32 angle t / 10000^(2i/144)"""
    if table == "oracle" and mut is None:
        return otext.rope(x, ROPE_DIM)
    d = HEAD_DIM if mut == "rope_all" else ROPE_DIM
    half, T = d // 2, x.shape[2]
    theta = 1.0 / (10000 ** (torch.arange(0, d, 2).float() / (HEAD_DIM if mut == "rope_exp288" else d)))
    pos = torch.arange(T).float() + (1.0 if mut == "rope_pos1" else 0.0)
    ang = torch.einsum("n,d->nd", pos, theta)      # fp32 [T, d / 2]
    cos, sin = ang.to(dtype).cos(), ang.to(dtype).sin()
    if mut == "rope_sin_sign":
        sin = -sin
    xr, xp = x[..., :d], x[..., d:]
    if mut == "rope_interleaved":      # pairs (2j, 2j + 1)
        a, c = xr[..., 0::2], xr[..., 1::2]
        rot = torch.stack([a * cos - c * sin, c * cos + a * sin], dim=-1).flatten(-2)
    else:
        a, c = xr[..., :half], xr[..., half:]
        rot = torch.cat([a * cos - c * sin, c * cos + a * sin], dim=-1)
    return torch.cat([rot, xp], dim=-1)


def heads(z):
    b, d, t = z.shape
    return z.view(b, HEADS, d // HEADS, t).transpose(2, 3)      # [B, H, T, 288]


def unheads(z):
    b, h, t, c = z.shape
    return z.transpose(2, 3).contiguous().view(b, h * c, t)


def evaluate(stage, ws, src, lens, dtype, mut=None, table="exact"):
    """stage (a name of STAGES) of one batch from src = {name: tensor} (SOURCES[stage]; "in": the batch dict), in `dtype`;
    ws = weights(); lens: the batch's lengths.  -> [B, C, Tt], zeros at and behind every length (SPK: [B, 80, 1])"""
    w = ws[dtype]
    g = lambda n: src[n].to(dtype)
    e, dp = "encoder.", "dp."
    with torch.inference_mode():
        if stage == "SPK":
            spk = src["in"]["spk_embed"].to(dtype)
            v = spk if mut == "spk_raw" else F.normalize(spk, dim=1)
            return F.linear(v, w["spk_embed_affine_layer.weight"], w["spk_embed_affine_layer.bias"])[:, :, None]
        T = src["in"]["x"].shape[1] if "in" in src else next(iter(src.values())).shape[2]
        m = x_mask(lens, T, dtype)
        if stage == "EMB":
            b = src["in"]
            h = (F.embedding(b["x"], w[e + "emb.weight"]) + F.embedding(b["tone"], w[e + "tone_emb.weight"])
                 + F.embedding(b["word_pos"], w[e + "word_pos_emb.weight"])
                 + F.embedding(b["syllable_pos"], w[e + "syllable_pos.weight"]))
            if mut != "no_sqrt":
                h = h * math.sqrt(spec.ENC_CH)
            return h.transpose(1, 2) * m
        if stage.startswith("PRE"):
            i = int(stage[-1])
            h = conv(w, e + f"prenet.conv_layers.{i}", g(SOURCES[stage][0]), m, lens, mut)
            if mut == "relu_first":
                h = torch.relu(h)
            h = layernorm(h, w[e + f"prenet.norm_layers.{i}.gamma"], w[e + f"prenet.norm_layers.{i}.beta"], mut)
            return (h if mut == "relu_first" else torch.relu(h)) * m
        if stage == "H0":
            b = src["in"]
            W, bias = w[e + "prenet.proj.weight"], w[e + "prenet.proj.bias"]
            y = F.conv1d(g("PRE2"), W, None if mut == "no_proj_bias" else bias)
            h = y if mut == "no_residual" else g("EMB") + y
            spk = b["spk_embed"].to(dtype)
            if mut == "spk_normalised":
                spk = F.normalize(spk, dim=1)
            le = F.embedding(b["lang"], w[e + "lang_emb.weight"]).transpose(1, 2)
            return torch.cat([h, spk.unsqueeze(-1).expand(-1, -1, T), le], dim=1) * m
        if stage == "X":
            return g(SOURCES[stage][0]).clone()
        if stage == "MU":
            y = F.conv1d(g("X"), w[e + "proj.weight"], w[e + "proj.bias"])
            return y if mut == "mu_unmasked" else y * m
        if stage == "XD":
            spk = src["in"]["spk_embed"].to(dtype)
            return (g("X") + F.conv1d(spk.unsqueeze(2), w[dp + "cond.weight"], w[dp + "cond.bias"])) * m
        if stage in ("D1", "D2"):
            n = stage[-1]
            h = conv(w, dp + f"conv_{n}", g(SOURCES[stage][0]), m, lens, mut)
            if mut != "relu_after_ln":
                h = torch.relu(h)
            h = layernorm(h, w[dp + f"norm_{n}.gamma"], w[dp + f"norm_{n}.beta"], mut)
            return (torch.relu(h) if mut == "relu_after_ln" else h) * m
        if stage == "LOGW":
            return conv(w, dp + "proj", g("D2"), m, lens) * m
        i, kind = int(stage[-1]), stage[:-1]
        a, f = e + f"encoder.attn_layers.{i}.", e + f"encoder.ffn_layers.{i}."
        if kind == "QKV":
            h = g(SOURCES[stage][0]) * m
            q, k, v = (F.conv1d(h, w[a + f"conv_{n}.weight"], w[a + f"conv_{n}.bias"]) for n in "qkv")
            q, k = (unheads(rope(heads(z), dtype, table, mut)) for z in (q, k))
            return torch.cat([q, k, v], dim=1) * m
        if kind == "ATT":
            q, k, v = (heads(z) for z in g(f"QKV{i}").split(576, dim=1))
            scores = q @ k.transpose(-2, -1) / math.sqrt(2 * HEAD_DIM if mut == "scale_576" else HEAD_DIM)
            keys = torch.ones_like(m) if mut == "keys_unmasked" else m
            mask2d = keys.unsqueeze(2) * m.unsqueeze(-1)      # [B, 1, Tq, Tk]
            p = torch.softmax(scores.masked_fill(mask2d == 0, -1e4), dim=-1)
            return unheads(p @ v) * m
        if kind == "N1":
            y = F.conv1d(g(f"ATT{i}"), w[a + "conv_o.weight"], w[a + "conv_o.bias"])
            return layernorm(g(SOURCES[stage][0]) + y, w[e + f"encoder.norm_layers_1.{i}.gamma"],
                             w[e + f"encoder.norm_layers_1.{i}.beta"], mut) * m
        if kind == "FF":
            y = conv(w, f + "conv_1", g(f"N1{i}"), m, lens, mut)
            return (y if mut == "relu_moved" else torch.relu(y)) * m
        if kind == "N2":
            y = conv(w, f + "conv_2", g(f"FF{i}"), m, lens, mut)
            if mut == "relu_moved":
                y = torch.relu(y)
            return layernorm(g(f"N1{i}") + y * m, w[e + f"encoder.norm_layers_2.{i}.gamma"],
                             w[e + f"encoder.norm_layers_2.{i}.beta"], mut) * m
    raise KeyError(stage)


def chain(name, dtype=torch.float64, table="exact", as_taps=False):
    """every stage of a case from its inputs, each fed the previous ones in `dtype`: {stage: tensor}, "in" included.  as_taps:
    every stage is rounded to fp32 before the next one reads it -- what the GPU test's references are fed (a run's own taps), so
    that a stage's floor is its own arithmetic's and not the rounding of its input"""
    lens = CASES[name][2]
    out = {"in": inputs(name)}
    for stage in TAPS[:-3] + ("X", "MU", "XD", "D1", "D2", "LOGW", "SPK"):      # (XD reads X: dependency order)
        out[stage] = evaluate(stage, weights(), out, lens, dtype, table=table)
        if as_taps:
            out[stage] = out[stage].float()
    return out


@functools.lru_cache(maxsize=None)
def tap_chain(name):
    """the fp64 chain of a case with fp32 taps, all six layers (host test; the conditions on the cases)"""
    return chain(name, as_taps=True)


def one_token_attention(stage, L):
    """the attention of a one-token utterance moves data (softmax over one key is 1, att = v): an fp32 floor of zero"""
    return stage.startswith("ATT") and L == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# length regulation: the kernel's documented rule (encops.hip, "length regulation"), restated in numpy
LR_SCALES = (1.0, 2.0, 0.5, 0.9, 1.1, 1.3, 2.0 / 3.0)
LR_EXACT_SCALES = (1.0, 2.0, 0.5)      # every term and every sum is exact in fp32: no band
LR_TT = (1, 7, 37, 129)
LR_MARGIN = 0.25 - 1e-5               # exp(logw) stays this far from an integer (u in [0.25, 0.75], less the logarithm's fp32 rounding)
LR_BAND_ULPS = 4.0                    # "near an integer": within 4 fp32 ulps of the fp64 sum


def lr_lengths(B, Tt, g):
    """ragged lengths: the first is Tt, the last (B > 1) is 1, the others random in [1, Tt]"""
    lens = torch.randint(1, Tt + 1, (B,), generator=g)
    lens[0] = Tt
    if B > 1:
        lens[-1] = 1
    return lens


def lr_inputs(seed, B, Tt, band=False):
    """(logw [B, 1, Tt] = log(k + u), k an integer in [0, 12), u in [0.25, 0.75]; lens [B] int64; mu_x [B, 80, Tt]).  band: the last
    live token's k is chosen so that the utterance's sum of ceil(k + u) = sum of (k + 1) is a multiple of 10: at a scale of 0.9 or
    1.1 the real sum is then an integer, and the fp32 terms put the computed one within a few ulps of it"""
    g = torch.Generator().manual_seed(seed)
    lens = lr_lengths(B, Tt, g)
    k = torch.randint(0, 12, (B, Tt), generator=g)
    u = 0.25 + 0.5 * torch.rand(B, Tt, generator=g, dtype=torch.float64)
    if band:
        for b in range(B):
            L = int(lens[b])
            rest = int((k[b, :L - 1] + 1).sum())
            k[b, L - 1] = (-rest - 1) % 10      # (k + 1) + rest = 0 mod 10, k in [0, 10)
    logw = torch.log(k.double() + u).float()[:, None, :]
    mu_x = torch.randn(B, 80, Tt, generator=g)
    return logw, lens, mu_x


def lr_sweep():
    """[(key, seed, B, Tt, scale, band)]: every scale x Tt x B in (1, 4), B = 65 at Tt = 37 for every scale, and the band batches
    (scales 0.9 and 1.1: B = 4 at Tt = 7 / 37 / 129, five seeds each, and B = 65 at Tt = 37)"""
    out, seed = [], 5000
    for si, scale in enumerate(LR_SCALES):
        for Tt in LR_TT:
            for B in (1, 4):
                seed += 1
                out.append((f"s{si}/Tt{Tt}/B{B}", seed, B, Tt, scale, False))
        seed += 1
        out.append((f"s{si}/Tt37/B65", seed, 65, 37, scale, False))
    for scale in (0.9, 1.1):
        for Tt in (7, 37, 129):
            for r in range(5):
                seed += 1
                out.append((f"band{scale}/Tt{Tt}/B4/{r}", seed, 4, Tt, scale, True))
        seed += 1
        out.append((f"band{scale}/Tt37/B65", seed, 65, 37, scale, True))
    return out


def lr_margin(logw):
    """distance of exp(logw) in fp64 from the nearest integer, the smallest over the batch: an ulp of difference between two
    exp implementations cannot move the ceil while this stays large"""
    e = torch.exp(logw.double())
    return float((e - e.round()).abs().min())


def lr_rule(logw, lens, mu_x, scale):
    """the kernel's rule: w_ceil = ceil(exp(logw) mask) scale in fp32; prefixes = the sequential fp64 sum rounded to fp32;
    y_len = max(long(float(sum64)), 1); attn and mu_y from the fp32 prefixes and y_len.
    -> (w_ceil [B, 1, Tt] fp32, y_len [B] int64, attn [B, Tt, Ty] fp32, mu_y [B, 80, Ty] fp32, sum64 [B], cum fp32 [B, Tt])"""
    import numpy as np
    lw = logw[:, 0].numpy().astype(np.float32)
    B, Tt = lw.shape
    L = np.minimum(lens.numpy(), Tt)
    mask = (np.arange(Tt)[None, :] < L[:, None]).astype(np.float32)
    w = (np.ceil(np.exp(lw) * mask).astype(np.float32) * np.float32(scale)).astype(np.float32)
    cum64 = np.zeros((B, Tt))
    for b in range(B):
        c = 0.0
        for t in range(Tt):
            c += float(w[b, t])
            cum64[b, t] = c
    cum = cum64.astype(np.float32)
    ylen = np.maximum(cum64[:, -1].astype(np.float32).astype(np.int64), 1)
    Ty = int(ylen.max())
    j = np.arange(Ty, dtype=np.float32)[None, None, :]
    hi = j < cum[:, :, None]
    lo = np.concatenate([np.zeros((B, 1, Ty), bool), hi[:, :-1]], axis=1)
    live = (np.arange(Tt)[None, :, None] < L[:, None, None]) & (np.arange(Ty)[None, None, :] < ylen[:, None, None])
    attn = (hi.astype(np.float32) - lo.astype(np.float32)) * live
    mu = mu_x.numpy()
    mu_y = np.zeros((B, 80, Ty), np.float32)
    for b in range(B):
        for jj in range(int(ylen[b])):
            tok = np.nonzero(np.float32(jj) < cum[b, :L[b]])[0]
            if tok.size:
                mu_y[b, :, jj] = mu[b, :, tok[0]]
    return (torch.from_numpy(w)[:, None, :], torch.from_numpy(ylen), torch.from_numpy(attn.astype(np.float32)), torch.from_numpy(mu_y),
            cum64[:, -1].copy(), cum)


def lr_in_band(sum64):
    """the fp64 sum lies within LR_BAND_ULPS fp32 ulps (of itself) of the nearest integer"""
    import numpy as np
    ulp = np.spacing(np.abs(sum64).astype(np.float32)).astype(np.float64)
    return np.abs(sum64 - np.rint(sum64)) <= LR_BAND_ULPS * ulp


def lr_oracle(logw, lens, mu_x, scale):
    """oracle.textenc.length_regulate on the same inputs"""
    m = x_mask(lens.tolist(), logw.shape[2], torch.float32)
    with torch.inference_mode():
        return otext.length_regulate(logw, m, mu_x, scale)
