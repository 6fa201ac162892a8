"""One plain reference per stage of the CFM estimator's trunk (estimator.hip Est::run), shared by test_gpu_est_stages.py (the stages
of jv_flow_estimator_tap against them) and test_est_stage_refs_host.py (the references against oracle.flow.estimator, and what
mistakes they catch).  A plain module, not a conftest; it loads no library.

Plain torch in `dtype`: fp64 is the reference, fp32 on the CPU the floor.  Every function maps the PREVIOUS stages' tensors, in the
layout a tap returns, to its stage, masked the same way; `mut` is one deliberate mistake.  Tap layout: the time taps are [n, C] (one
row per sample in the "entry" mode, ONE row in the "step" mode), every other tap [S, C, T] channels first over the S samples of the
evaluation, exact zeros at and behind a sample's clamped length.  "entry": the S = B2 samples are the caller's.  "step": S = 2 B,
sample B + b is the unconditional twin of utterance b -- x of the utterance, zeros for mu / spks / cond.  The convolutions, the
conv + LayerNorm + Mish block and the transformer block are oracle.flow's own functions wherever the stage IS that operation; the
local forms below exist for the mistakes only and are held to the oracle's in the host file.

The sinusoid.  The model computes the angle (1000 t) f_j in fp32 (decoder.py:21-30) and time_sinusoid_kernel mirrors that, so the
fp32 angle is part of the OPERATION in any dtype: the fp64 reference of TSIN takes sin / cos in fp64 OF THE FP32 ANGLE, and the floor
is torch's fp32 sin / cos of it.  f is the CORRECTLY ROUNDED table: fp64 exp of the fp32 product j c, rounded once (freq_table).
table="oracle" is what oracle.flow.time_embedding computes when it is handed t in fp64 -- this build's torch.exp in fp32, the angle
in fp64 -- so that the composition test can hold the chain of these formulas to the oracle at 1e-10."""
import functools
import math

import torch
import torch.nn.functional as F

from jyutvoice_amd import synth
from oracle import flow as oflow

PRE = "decoder.estimator."
NRES, NBLK, HALF, HEADS = 14, 4, 160, 8
RATIO = 8.0
# a stage read behind a contraction longer than the 1024 products up to which 8 x was established takes 8 x sqrt(K / 1024)
# (test_gpu_est_stages.py::test_long_contraction_alone grounds each entry)
LONG_K = {"RES13": 1536}
TIME_TAPS = ("TSIN", "T1", "TMISH", "TEMB")
TIME_CHANNELS = {"TSIN": 2 * HALF, "T1": 1024, "TMISH": 1024, "TEMB": NRES * 256}


def stage_taps(i):
    return (f"RES{i}",) + tuple(f"BLK{i}_{j}" for j in range(NBLK))


TAPS = (TIME_TAPS + ("XIN",) + stage_taps(0) + ("DOWN",) + tuple(t for i in range(1, NRES) for t in stage_taps(i))
        + ("UPC", "FIN", "D"))      # execution order: the ids 0 .. 78


def ratio_of(stage):
    return RATIO * math.sqrt(LONG_K[stage] / 1024.0) if stage in LONG_K else RATIO


def channels_of(stage):
    return TIME_CHANNELS.get(stage, 320 if stage == "XIN" else 80 if stage == "D" else 256)


def stage_of(tap):
    """(kind, stage index, block index) of RESi / BLKi_j, else (tap, None, None)"""
    if tap.startswith("RES"):
        return "RES", int(tap[3:]), None
    if tap.startswith("BLK"):
        i, j = tap[3:].split("_")
        return "BLK", int(i), int(j)
    return tap, None, None


def stage_prefix(i):
    return PRE + ("down_blocks.0." if i == 0 else "up_blocks.0." if i == NRES - 1 else f"mid_blocks.{i - 1}.")


def sources_of(tap):
    """what a stage reads: earlier stages, or "in" (the inputs of the batch)"""
    kind, i, j = stage_of(tap)
    if kind == "RES":
        return (("XIN",) if i == 0 else ("DOWN",) if i == 1 else ("BLK12_3", "BLK0_3") if i == NRES - 1 else (f"BLK{i - 1}_3",)) + ("TEMB",)
    if kind == "BLK":
        return (f"RES{i}",) if j == 0 else (f"BLK{i}_{j - 1}",)
    return {"TSIN": ("in",), "T1": ("TSIN",), "TMISH": ("T1",), "TEMB": ("TMISH",), "XIN": ("in",), "DOWN": ("BLK0_3",),
            "UPC": (f"BLK{NRES - 1}_3",), "FIN": ("UPC",), "D": ("FIN",)}[tap]


def moves_data(tap):
    return tap == "XIN"


# ---------------------------------------------------------------------------------------------------------------------------------
# cases: the smallest shapes at which the wiring can go wrong (test_gpu_est_stages.py lists which route runs which)
CASES = {
    "t1": dict(seed=701, T=1, lens=(1,)),                     # every causal tap but the last reads guard rows
    "t2": dict(seed=702, T=2, lens=(2, 1)),
    "ragged37": dict(seed=703, T=37, lens=(37, 36, 1)),       # an end one row from a neighbour's gap; a one-frame utterance
    "dead": dict(seed=704, T=5, lens=(5, 0, 3)),              # a dead utterance between live ones
    # S = 78 rows per sample: sample 1 starts at row 82, inside a 32-row and an 80-row tile; sample 2 at row 160, on a workgroup seam
    # of the tile heights 2 and 5 (32 and 80 rows); sample 1 ends one row short of its gap
    "seam": dict(seed=705, T=74, lens=(74, 73, 74)),
    "mags": dict(seed=706, T=19, lens=(19, 19, 12), scale=(1.0, 30.0, 0.03)),      # the per-utterance amax slots
    "chunk": dict(seed=707, T=37, lens=(37, 33, 17), chunk=16),      # streaming: chunk lines at 16 and 32
    # the smallest M above 2048 in the entry's uniform rows: 4 + 8 x 264 = 2116 (the tile kernels without split-K)
    "big260": dict(seed=708, T=260, lens=(260, 259, 131, 1, 260, 77, 0, 200)),
}
T_STEP = 0.9045      # the step mode's one timestep (a cosine-schedule value); the entry mode takes a distinct t per sample


@functools.lru_cache(maxsize=None)
def inputs(name):
    """the batch as the entries take it: x, mu, cond [B, 80, T], spks [B, 80], lens int32 [B], t [B] (entry) / T_STEP (step)"""
    c = CASES[name]
    B, T = len(c["lens"]), c["T"]
    g = torch.Generator().manual_seed(c["seed"])
    x, mu, cond = (torch.randn(B, 80, T, generator=g) for _ in range(3))
    spks = torch.randn(B, 80, generator=g)
    t = torch.rand(B, generator=g)
    t[0] = 0.3
    for b, s in enumerate(c.get("scale", ())):
        x[b] *= s
        mu[b] *= s
    return dict(x=x, mu=mu, cond=cond, spks=spks, lens=torch.tensor(c["lens"], dtype=torch.int32), t=t, B=B, T=T,
                chunk=c.get("chunk", 0))


def only(inp, b):
    """utterance b alone at the same width"""
    return dict(inp, x=inp["x"][b:b + 1], mu=inp["mu"][b:b + 1], cond=inp["cond"][b:b + 1], spks=inp["spks"][b:b + 1],
                lens=inp["lens"][b:b + 1], t=inp["t"][b:b + 1], B=1)


def step_as_entry(inp):
    """the 2 B samples the step mode lays out, handed to the entry mode with the step's t for every sample: where the two modes
    coincide"""
    x, mu, spks, cond, _ = samples(inp, "step")
    return dict(inp, x=x, mu=mu, cond=cond, spks=spks, lens=torch.cat([inp["lens"], inp["lens"]]), t=torch.full((2 * inp["B"],), T_STEP),
                B=2 * inp["B"])


def samples(inp, mode, mut=None):
    """the S samples of the evaluation: (x, mu, spks, cond, t [n]); step: the B utterances, then their twins"""
    x, mu, spks, cond = inp["x"], inp["mu"], inp["spks"], inp["cond"]
    if mode == "entry":
        return x, mu, spks, cond, inp["t"]
    z = torch.zeros_like(mu)
    twin_mu = mu if mut == "twin_mu" else z
    return (torch.cat([x, x]), torch.cat([mu, twin_mu]), torch.cat([spks, torch.zeros_like(spks)]), torch.cat([cond, z]),
            torch.tensor([T_STEP]))


def geometry(inp, mode):
    L = [min(max(int(v), 0), inp["T"]) for v in inp["lens"]]
    if mode == "step":
        L = L + L
    return dict(mode=mode, S=len(L), T=inp["T"], L=L, n=1 if mode == "step" else len(L), chunk=inp["chunk"])


def shape_of(tap, geo):
    return (geo["n"], channels_of(tap)) if tap in TIME_TAPS else (geo["S"], channels_of(tap), geo["T"])


def rows_of(t, b, n):
    """[n, C]: the first n positions of sample b of a row tap"""
    return t[b, :, :n].transpose(0, 1)


@functools.lru_cache(maxsize=None)
def weights():
    sd = {k: v for k, v in synth.tts_state_dict().items() if k.startswith(PRE)}
    return {torch.float32: sd, torch.float64: {k: v.double() for k, v in sd.items()}}


# ---------------------------------------------------------------------------------------------------------------------------------
def freq_products():
    """the fp32 products j c, c = -(ln 10000) / 159 rounded to fp32, as oracle.flow.time_embedding and the kernel form them"""
    return torch.arange(HALF).float() * -(math.log(10000) / (HALF - 1))


def freq_table(kind="exact"):
    """f [160] fp32.  exact: correctly rounded (fp64 exp of the fp32 product, rounded once); torch: this build's fp32 torch.exp;
    ulp: the exact table moved up one ulp in every entry; over160: the exponent over 160 instead of 159"""
    p = freq_products()
    if kind == "torch":
        return torch.exp(p)
    if kind == "over160":
        p = torch.arange(HALF).float() * -(math.log(10000) / HALF)
    f = torch.exp(p.double()).float()
    if kind == "ulp":
        f = torch.nextafter(f, torch.full_like(f, 2.0))
    return f


def mask_of(geo, dtype):
    return (torch.arange(geo["T"])[None] < torch.tensor(geo["L"])[:, None]).unsqueeze(1).to(dtype)      # [S, 1, T]


def allowed_keys(geo, mut=None):
    """[S, 1, T or 1, T] bool: which keys a query sees -- the key mask, and in streaming the chunk rule of oracle.flow.estimator"""
    T = geo["T"]
    ok = mask_of(geo, torch.float32).bool().unsqueeze(1)
    if mut == "keys_unmasked":
        ok = torch.ones_like(ok)
    if geo["chunk"]:
        i, c = torch.arange(T), geo["chunk"]
        line = ((i + 1) // c + 1) * c if mut == "chunk_off" else (i // c + 1) * c
        ok = ok & (i[None, :] < line[:, None])[None, None]
    return ok


def _cblock(sd, pre, x, mask, mut=None, prev_tail=None):
    """oracle.flow.causal_block with room for a mistake"""
    eps = {"ln_eps": 1e-6, "ln_eps_big": 1e-1}.get(mut, 1e-5)
    w, b = sd[pre + "block.0.weight"], sd[pre + "block.0.bias"]
    xm = x * mask
    if mut == "tap_off":
        h = F.conv1d(F.pad(xm, (1, 1)), w, b)      # rows t-1 .. t+1
    elif mut == "halo":      # the left context of sample b is what sample b - 1 holds in its last two frames, not zeros
        left = torch.cat([torch.zeros_like(x[:1, :, :2]), x[:-1, :, -2:]]) if x.shape[2] >= 2 else torch.zeros_like(x[:, :, :0])
        h = F.conv1d(F.pad(torch.cat([left, xm], dim=2), (2 - left.shape[2], 0)), w, b)
    else:
        h = oflow.causal_conv(xm, w, b)
    h = F.layer_norm(h.transpose(1, 2), (h.shape[1],), sd[pre + "block.2.weight"], sd[pre + "block.2.bias"], eps).transpose(1, 2)
    return (F.silu(h) if mut == "mish_silu" else F.mish(h)) * mask


def _tblock(sd, pre, h, ok, mut=None):
    """oracle.flow.transformer_block with room for a mistake; ok: allowed_keys"""
    S, T, C = h.shape
    eps = {"ln_eps": 1e-6, "ln_eps_big": 1e-1}.get(mut, 1e-5)
    n = F.layer_norm(h, (C,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], eps)
    q, k, v = (F.linear(n, sd[pre + f"attn1.to_{z}.weight"]) for z in "qkv")
    hd = q.shape[-1] // HEADS
    sp = lambda z: z.view(S, T, HEADS, hd).transpose(1, 2)
    bias = (1.0 - ok.to(h.dtype)) * -1.0e10
    s = sp(q) @ sp(k).transpose(-2, -1) / math.sqrt(512 if mut == "scale_512" else hd) + bias
    o = (torch.softmax(s, dim=-1) @ sp(v)).transpose(1, 2).reshape(S, T, HEADS * hd)
    h = h + F.linear(o, sd[pre + "attn1.to_out.0.weight"], sd[pre + "attn1.to_out.0.bias"])
    n = F.layer_norm(h, (C,), sd[pre + "norm3.weight"], sd[pre + "norm3.bias"], eps)
    f = F.gelu(F.linear(n, sd[pre + "ff.net.0.proj.weight"], sd[pre + "ff.net.0.proj.bias"]), approximate="tanh" if mut == "gelu_tanh" else "none")
    return h + F.linear(f, sd[pre + "ff.net.2.weight"], sd[pre + "ff.net.2.bias"])


def _resnet(sd, pre, x, mask, temb, mut=None):
    """the resnet of one stage on its slice of TEMB ([n, 256]; one row: the same for every sample)"""
    block = (lambda p, z: oflow.causal_block(sd, p, z, mask)) if mut is None else (lambda p, z: _cblock(sd, p, z, mask, mut))
    e = temb.expand(x.shape[0], -1).unsqueeze(-1)
    h = block(pre + "block1.", x)
    if mut != "temb_late":
        h = h + e
    h = block(pre + "block2.", h)
    if mut == "temb_late":
        h = h + e * mask
    return h + F.conv1d(x if mut == "res_unmasked" else x * mask, sd[pre + "res_conv.weight"], sd[pre + "res_conv.bias"])


def evaluate(tap, ws, src, geo, dtype, mut=None, table="exact"):
    """stage `tap` in `dtype` from its sources (src: {stage: tensor in the tap layout}, "in": the batch), masked as a tap is"""
    sd = ws[dtype]
    kind, i, j = stage_of(tap)
    get = lambda k: src[k].to(dtype)
    if tap == "TSIN":
        t = samples(src["in"], geo["mode"])[4]
        f = freq_table({"freq_ulp": "ulp", "over160": "over160"}.get(mut, "torch" if table == "oracle" else "exact"))
        scale = 1.0 if mut == "no_1000" else 1000.0
        if table == "oracle":
            a = (scale * t.double()).unsqueeze(1) * f.double().unsqueeze(0)
        else:
            a = ((scale * t.float()).unsqueeze(1) * f.unsqueeze(0)).to(dtype)      # the fp32 angle, whatever the dtype
        return torch.cat([a.cos(), a.sin()] if mut == "sincos_swap" else [a.sin(), a.cos()], dim=-1).to(dtype)
    if tap == "T1":
        return F.silu(F.linear(get("TSIN"), sd[PRE + "time_mlp.linear_1.weight"], sd[PRE + "time_mlp.linear_1.bias"]))
    if tap == "TMISH":
        e = F.linear(get("T1"), sd[PRE + "time_mlp.linear_2.weight"], sd[PRE + "time_mlp.linear_2.bias"])
        return F.silu(e) if mut == "temb_silu" else e if mut == "temb_no_mish" else F.mish(e)
    if tap == "TEMB":
        return torch.cat([F.linear(get("TMISH"), sd[stage_prefix(s) + "0.mlp.1.weight"], sd[stage_prefix(s) + "0.mlp.1.bias"])
                          for s in range(NRES)], dim=-1)
    mask = mask_of(geo, dtype)
    if tap == "XIN":
        x, mu, spks, cond, _ = samples(src["in"], geo["mode"], mut)
        return torch.cat([x, mu, spks.unsqueeze(-1).expand(-1, -1, geo["T"]), cond], dim=1).to(dtype) * mask
    if kind == "RES":
        names = sources_of(tap)[:-1]
        if mut == "cat_swap":
            names = names[::-1]
        x = torch.cat([get(k) for k in names], dim=1)
        s = i + {"temb_prev": -1, "temb_next": 1}.get(mut, 0)
        temb = get("TEMB")[:, 256 * s:256 * (s + 1)]
        return _resnet(sd, stage_prefix(i) + "0.", x, mask, temb, mut) * mask
    if kind == "BLK":
        h = get(sources_of(tap)[0]).transpose(1, 2)
        pre = stage_prefix(i) + f"1.{j}."
        if mut is None:
            ok = allowed_keys(geo)
            out = oflow.transformer_block(sd, pre, h, (1.0 - ok.to(dtype)) * -1.0e10)
        else:
            out = _tblock(sd, pre, h, allowed_keys(geo, mut), mut)
        return out.transpose(1, 2) * mask
    if tap in ("DOWN", "UPC"):
        pre = stage_prefix(0 if tap == "DOWN" else NRES - 1)
        w, b = sd[pre + "2.weight"], sd[pre + "2.bias"]
        x = get(sources_of(tap)[0])
        if mut == "tap_off":
            return F.conv1d(F.pad(x * mask, (1, 1)), w, b) * mask
        return oflow.causal_conv(x if mut == "in_unmasked" else x * mask, w, b) * mask
    if tap == "FIN":
        x = get("UPC")
        return oflow.causal_block(sd, PRE + "final_block.", x, mask) if mut is None else _cblock(sd, PRE + "final_block.", x, mask, mut)
    assert tap == "D", tap
    x = get("FIN")
    return F.conv1d(x if mut == "in_unmasked" else x * mask, sd[PRE + "final_proj.weight"], sd[PRE + "final_proj.bias"]) * mask


def chain(inp, geo, dtype=torch.float64, table="exact", taps=TAPS):
    """every stage from the inputs alone, each fed the chain's own previous stages"""
    out = {"in": inp}
    with torch.inference_mode():
        for tap in taps:
            out[tap] = evaluate(tap, weights(), out, geo, dtype, table=table)
    return out


@functools.lru_cache(maxsize=None)
def tap_chain(name, mode):
    """the fp64 chain of a case rounded to fp32 stage by stage: stand-ins for the taps a GPU run returns"""
    inp = inputs(name)
    return {k: (v if k == "in" else v.float()) for k, v in chain(inp, geometry(inp, mode)).items()}
