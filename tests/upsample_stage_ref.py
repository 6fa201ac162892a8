"""One plain reference per stage of the up-sampling conformer encoder (prompt.hip encoder_stages), shared by
test_gpu_upsample_stages.py (the stages of jv_upsample_encoder_tap against them) and test_upsample_stage_refs_host.py (the references
against oracle.prompt and the G15 fixture, and what mistakes they catch).  A plain module, not a conftest; it loads no library.

Plain torch in `dtype`: fp64 is the reference, fp32 on the CPU the floor.  Every function maps the PREVIOUS stages' tensors, in the
layout a tap returns, to its stage, masked the same way; `mut` is one deliberate mistake.  Tap layout, with W = P + N the width of
the whole sequence and L_b the encoded length of utterance b (its tokens less its look-ahead context): row stages are [B, C, W] at
token rate and [B, C, 2 W] at mel rate, channels first, exact zeros at and behind L_b / 2 L_b (E0 alone also shows the ctx_b context
rows conv1 reads); the position tables and linear_pos of them are [2T - 1, 512] with T the encoded WIDTH (W; in the partial mode
W - 3) times the rate.  Convolutions are F.conv1d on per-utterance slices with the utterance's own zero or context padding, the
attention is the masked-softmax expression of oracle/prompt.py with its rel_shift, on the 2n - 1 table rows an utterance of n rows
reaches.

The position tables.  The model computes the angle r * div_i in fp32 (embedding.py:239-246; `div` is the fp32 tensor the loader
passes, flow/encoder.py div_term) and rel_pos_table_kernel mirrors that, so the fp32 angle is part of the OPERATION in any dtype:
the fp64 reference of PE1 / PE2 takes sin / cos in fp64 OF THE FP32 ANGLE (table="exact", the default) and the floor is torch's
fp32 sin / cos of it.  An angle computed in fp64 would differ by up to 2^-24 |r| div_0 -- 3.6e-5 rad at |r| = 599 -- and the floor
would then measure that rounding and not the kernel.  oracle.prompt in fp64 multiplies by the fp32-ROUNDED sin / cos: table="oracle"
does that, so that the composition test can hold the chain of these formulas to the oracle at 1e-10."""
import functools
import math

import torch
import torch.nn.functional as F

from jyutvoice_amd import spec, synth
from oracle import prompt as oprompt

D, HEADS, DK, FFN, N_OUT = 512, 8, 64, 2048, 80
BLOCKS, UP_BLOCKS = 6, 4
LOOKAHEAD, CHUNK = 3, oprompt.STATIC_CHUNK
BLOCK_TAPS = ("LN1", "QKV", "POS", "ATT", "X1", "LN2", "FF", "X2")
FRONT1, FRONT2 = ("EMB", "EL", "E0", "PE1", "C1", "LA"), ("REP", "UP", "UL", "U0", "PE2")
TAPS = (FRONT1 + tuple(f"{n}_{i}" for i in range(BLOCKS) for n in BLOCK_TAPS) + FRONT2
        + tuple(f"{n}_u{i}" for i in range(UP_BLOCKS) for n in BLOCK_TAPS) + ("AN", "H"))      # execution order: the ids 0 .. 92
BLOCK_CHANNELS = {"LN1": D, "QKV": 3 * D, "POS": D, "ATT": D, "X1": D, "LN2": D, "FF": FFN, "X2": D}


def kind_of(stage):
    return stage.partition("_")[0]


def block_of(stage):
    """(kind, weight prefix, the block's input stage, its table, rate) of a per-block stage, else None"""
    kind, _, idx = stage.partition("_")
    if not idx:
        return None
    if idx[0] == "u":
        i = int(idx[1:])
        return kind, f"encoder.up_encoders.{i}.", "U0" if i == 0 else f"X2_u{i - 1}", "PE2", 2
    i = int(idx)
    return kind, f"encoder.encoders.{i}.", "LA" if i == 0 else f"X2_{i - 1}", "PE1", 1


def rate_of(stage):
    blk = block_of(stage)
    return blk[4] if blk else 1 if stage in FRONT1 else 2


def channels_of(stage):
    return N_OUT if stage == "H" else BLOCK_CHANNELS[kind_of(stage)] if block_of(stage) else D


def is_table(stage):
    return kind_of(stage) in ("PE1", "PE2", "POS")


def sources_of(stage):
    """what a stage reads: earlier stages, or "in" (the ids and lengths of the batch)"""
    blk = block_of(stage)
    if blk:
        kind, _, x, pe, _ = blk
        sfx = stage[len(kind):]
        return {"LN1": (x,), "QKV": ("LN1" + sfx,), "POS": (pe,), "ATT": ("QKV" + sfx, "POS" + sfx), "X1": (x, "ATT" + sfx),
                "LN2": ("X1" + sfx,), "FF": ("LN2" + sfx,), "X2": ("X1" + sfx, "FF" + sfx)}[kind]
    return {"EMB": ("in",), "EL": ("EMB",), "E0": ("EL", "in"), "PE1": (), "C1": ("E0",), "LA": ("C1", "E0"),
            "REP": (f"X2_{BLOCKS - 1}",), "UP": ("REP",), "UL": ("UP",), "U0": ("UL",), "PE2": (),
            "AN": (f"X2_u{UP_BLOCKS - 1}",), "H": ("AN",)}[stage]


# long300: both tables, the fronts, block 0 of each stage, after_norm and the output are compared; the last block of each stage
# is taken as the source REP / AN are held to (SOURCE_ONLY: tapped, not compared -- their own sources are not).  Every other case
# runs all ten blocks
def _blocks(*sfx):
    return tuple(f"{n}_{i}" for i in sfx for n in BLOCK_TAPS)


LONG_STAGES = (FRONT1 + _blocks("0") + (f"X2_{BLOCKS - 1}",) + FRONT2 + _blocks("u0") + (f"X2_u{UP_BLOCKS - 1}",) + ("AN", "H"))
REDUCED = {"long300": LONG_STAGES}
SOURCE_ONLY = {"long300": (f"X2_{BLOCKS - 1}", f"X2_u{UP_BLOCKS - 1}")}

# ---------------------------------------------------------------------------------------------------------------------------------
# cases: the smallest token counts at which these kernels can go wrong.  runs: (mode, streaming) -- "prompt" (jv_prompt_encoder_fwd:
# the three-GEMM attention), "flow" (relattn.hip's one launch), "partial" (a scalar context of 3 tokens), "ctx" (one per utterance)
CASES = {
    # every look-ahead and up-conv tap but one reads guard or gap rows; two keys in stage 2
    "t1": dict(first=500, P=0, N=1, tlens=(1,), runs=(("prompt", False), ("flow", False))),
    # two sources; an utterance end one row from its neighbour's gap; a 1-token utterance; garbage ids behind the lengths
    "split37": dict(first=510, P=12, N=25, plens=(12, 0, 1), tlens=(25, 25, 0), garbage=True, runs=(("flow", False), ("flow", True))),
    "dead": dict(first=520, P=0, N=5, tlens=(5, 0, 3), runs=(("prompt", False), ("flow", False))),      # a dead utterance between live ones
    "chunk26": dict(first=530, P=0, N=26, tlens=(26,), runs=(("flow", True),)),      # the second chunk: one token row, two mel rows
    "chunk51": dict(first=540, P=0, N=51, tlens=(51, 50, 26), runs=(("flow", True), ("prompt", False))),      # on and across both chunks
    # 130 mel-rate rows: relattn's second 128-query workgroup, the 64-lane softmax stride, ld = 96 / 160 of the three-GEMM buffers
    "lanes65": dict(first=550, P=0, N=65, tlens=(65, 64, 33), runs=(("prompt", False), ("flow", False))),
    # L = 27 crosses the chunk line; context rows visible to C1 only
    "part30": dict(first=560, P=8, N=22, plens=(8,), tlens=(22,), ctx=(3,), runs=(("partial", False), ("partial", True))),
    "part4": dict(first=570, P=0, N=4, tlens=(4,), ctx=(3,), runs=(("partial", False),)),      # one encoded token
    # a context at full width, none, and a one-encoded-token utterance in one batch
    "ctxmix": dict(first=580, P=0, N=30, tlens=(30, 30, 4), ctx=(3, 0, 3), runs=(("ctx", False), ("ctx", True))),
    "long300": dict(first=590, P=0, N=300, tlens=(300,), runs=(("flow", False), ("flow", True), ("prompt", False))),      # |r| up to 599
}
SHORT_CASES = tuple(k for k in CASES if k != "long300")
RUNS = tuple((c, m, s) for c, v in CASES.items() for m, s in v["runs"])
GARBAGE_IDS = (10 ** 12, -7)      # behind a length: out of range on either side, never read


def stages_of(name):
    return REDUCED.get(name, TAPS)


def compared(name):
    return tuple(s for s in stages_of(name) if s not in SOURCE_ONLY.get(name, ()))


def make_inputs(ptok, plen, tok, tlen, ctx=None):
    """the batch as the entries take it, and per utterance the ids of its sequence [prompt | tokens] on the host"""
    B, N = tok.shape
    P = 0 if ptok is None else ptok.shape[1]
    pl = [0] * B if P == 0 else [min(max(int(v), 0), P) for v in plen]
    tl = [min(max(int(v), 0), N) for v in tlen]
    ids = [torch.cat([ptok[b, :pl[b]] if P else tok[b, :0], tok[b, :tl[b]]]) for b in range(B)]
    return dict(ptok=ptok, plen=plen, tok=tok, tlen=tlen, ctx=list(ctx) if ctx is not None else [0] * B, ids=ids, B=B, P=P, N=N)


@functools.lru_cache(maxsize=None)
def inputs(name):
    c = CASES[name]
    B = len(c["tlens"])
    tok, tlen = synth.prompt_tokens(B, c["N"], lengths=list(c["tlens"]), first_index=c["first"])
    ptok = plen = None
    if c["P"]:
        ptok, plen = synth.prompt_tokens(B, c["P"], lengths=list(c["plens"]), first_index=c["first"] + 50)
    if c.get("garbage"):
        for t, ln in ((tok, tlen), (ptok, plen)):
            for b in range(B):
                t[b, int(ln[b]):] = GARBAGE_IDS[b % 2]
    return make_inputs(ptok, plen, tok, tlen, c.get("ctx"))


def only(inp, i):
    """utterance i of a batch alone, at the same widths"""
    sl = lambda t: None if t is None else t[i:i + 1]
    return make_inputs(sl(inp["ptok"]), sl(inp["plen"]), sl(inp["tok"]), sl(inp["tlen"]), inp["ctx"][i:i + 1])


def geometry(inp, mode, streaming):
    """W: the width of the whole sequence; T: the encoded width; L: encoded lengths; ctx: context rows behind them (conv1's alone)"""
    W = inp["P"] + inp["N"]
    ctx = [0] * inp["B"] if mode in ("prompt", "flow") else list(inp["ctx"])
    assert mode != "partial" or (inp["B"] == 1 and ctx == [LOOKAHEAD])
    L = [max(len(ids) - c, 0) for ids, c in zip(inp["ids"], ctx)]
    return dict(B=inp["B"], W=W, T=W - LOOKAHEAD if mode == "partial" else W, L=L, ctx=ctx, streaming=bool(streaming), mode=mode)


def live(stage, geo, b):
    """positions of a row stage that utterance b owns"""
    return rate_of(stage) * geo["L"][b] + (geo["ctx"][b] if stage == "E0" else 0)


def shape_of(stage, geo):
    if is_table(stage):
        return (2 * rate_of(stage) * geo["T"] - 1, D)
    return (geo["B"], channels_of(stage), rate_of(stage) * geo["W"])


def rows_of(t, b, n):
    """[B, C, T] -> the first n positions of utterance b as rows [n, C]"""
    return t[b, :, :n].T


@functools.lru_cache(maxsize=None)
def checkpoint():
    return synth.prompt_state_dict()


@functools.lru_cache(maxsize=None)
def div_term():
    from jyutvoice_amd.flow.encoder import div_term as dt
    return dt()


@functools.lru_cache(maxsize=None)
def weights():
    sd = checkpoint()
    return {torch.float32: sd, torch.float64: {k: v.double() for k, v in sd.items()}}


# The bound.  test_gpu_fused_ops.RATIO = 8 (4 x for the significant bits, 2 x for the summation order inside the MFMAs) was
# established on contractions of up to K = 1024 products per output.  Stages read straight behind a longer contraction take the
# project's existing rule (textenc_stage_ref.LONG_K): conv_gemm accumulates all K products of an output in ONE fp32 chain inside the
# MFMAs, whose rounding error grows as sqrt(K) (random-walk model; Higham, Accuracy and Stability of Numerical Algorithms, 2.8),
# while the CPU floor sums in blocked vector lanes and barely grows: RATIO x sqrt(K / 1024).  Here C1 (k4 over 512 channels,
# K = 2048: 11.3 x), UP (k5, K = 2560: 12.6 x) and X2 (w_2 over the 2048 hidden channels: 11.3 x) -- each only because
# test_long_contraction_alone shows jv_op_conv_gemm ALONE on the run's own source tap to return the stage's bits.
RATIO = 8.0
LONG_K = {"C1": 4 * D, "UP": 5 * D, "X2": FFN}


def ratio_of(stage):
    k = LONG_K.get(kind_of(stage))
    return RATIO * math.sqrt(k / 1024.0) if k else RATIO


def moves_data(stage, geo, b=None):
    """stages that only move data have an fp32 floor of zero and are held torch.equal: the embedding lookup, nearest x 2, the
    token-rate attention of a one-token utterance (softmax over one key is 1: att = v), and the one-row table of T = 1 (sin 0, cos 0)"""
    if stage in ("EMB", "REP"):
        return True
    if stage == "PE1":
        return geo["T"] == 1
    return kind_of(stage) == "ATT" and rate_of(stage) == 1 and b is not None and geo["L"][b] == 1


# ---------------------------------------------------------------------------------------------------------------------------------
def layernorm(x, g, b, mut=None):
    """rows [n, 512]"""
    if mut not in ("ln_eps", "ln_eps_big", "ln_unbiased"):
        return F.layer_norm(x, (x.shape[-1],), g, b, 1e-5)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    if mut == "ln_unbiased":
        var = var * x.shape[-1] / (x.shape[-1] - 1)
    return (x - mean) * torch.rsqrt(var + {"ln_eps": 1e-4, "ln_eps_big": 1e-1}.get(mut, 1e-5)) * g + b


def pos_table(T, dtype, table="exact", mut=None):
    """[2T - 1, 512]: row m holds relative position r = T - 1 - m, sin at even and cos at odd columns of the fp32 angle r * div_i"""
    if table == "oracle" and mut is None:
        return oprompt.rel_pos_emb(T, D)[0].to(dtype)
    r = torch.arange(T - 1, -T, -1, dtype=torch.float32)
    if mut == "table_half":      # built for T / 2 (the token-rate table at mel rate): every position off by T / 2
        r = r - float(T // 2)
    div = div_term()
    ang = (r.double()[:, None] * div.double()[None, :]) if mut == "angle_fp64" else r[:, None] * div[None, :]
    s, c = ang.to(dtype).sin(), ang.to(dtype).cos()
    if mut == "angle_fp64":      # (the exact angle's correctly rounded sin / cos: what a "more accurate" kernel would store)
        s, c = ang.sin().to(dtype), ang.cos().to(dtype)
    if mut == "sincos_swap":
        s, c = c, s
    return torch.stack([s, c], dim=-1).reshape(2 * T - 1, D)


def attention(qkv, pos, u, v, T, chunk, mut=None, keys=None):
    """one utterance: qkv rows [n, 1536], pos = linear_pos(table) [2T - 1, 512], u / v [8, 64] -> [n, 512] ahead of linear_out.
    keys: live keys (n); chunk > 0: query i sees keys j < (i // chunk + 1) * chunk"""
    n = qkv.shape[0]
    keys = n if keys is None else keys
    q, k, val = (z.reshape(n, HEADS, DK).transpose(0, 1) for z in qkv.split(D, dim=1))      # [8, n, 64]
    p = pos[T - n:T + n - 1]      # the 2n - 1 positions n - 1 .. -(n - 1)
    if mut == "rel_shift_off":
        p = torch.roll(p, -1, dims=0)
    p = p.reshape(2 * n - 1, HEADS, DK).transpose(0, 1)
    if mut == "uv_swap":
        u, v = v, u
    ac = (q + u[:, None, :]) @ k.transpose(-2, -1)
    bd = oprompt.rel_shift(((q + v[:, None, :]) @ p.transpose(-2, -1))[None])[0]
    scores = (ac + bd) / math.sqrt(D if mut == "scale_512" else DK)
    i, j = torch.arange(n)[:, None], torch.arange(n)[None, :]
    alive = (j < keys).expand(n, n)
    if chunk > 0:
        alive = alive & (j < (chunk if mut == "chunk_line" else (i // chunk + 1) * chunk))
    dead = ~alive[None]
    attn = torch.softmax(scores.masked_fill(dead, -float("inf")), dim=-1).masked_fill(dead, 0.0)
    return (attn @ val).transpose(0, 1).reshape(n, D)


def evaluate(stage, ws, src, geo, dtype, mut=None, table="exact"):
    """stage (a name of TAPS) of one batch from src = {name: tensor} (sources_of(stage); "in": make_inputs' dict) in `dtype`;
    ws = weights(); geo = geometry(...).  -> the tap's layout, zeros at and behind every live length"""
    w = ws[dtype]
    g = lambda n: src[n].to(dtype)
    e = "encoder."
    lin = lambda pre, x: F.linear(x, w[pre + ".weight"], w.get(pre + ".bias"))
    rate = rate_of(stage)

    def per_utt(fn):
        """fn(b, n) -> rows [n, C] of utterance b's n = rate L_b live positions (E0: its context rows behind them)"""
        out = torch.zeros(shape_of(stage, geo), dtype=dtype)
        for b, L in enumerate(geo["L"]):
            if L > 0:
                r = fn(b, rate * L)
                out[b, :, :r.shape[0]] = r.T
        return out

    def per_row(fn, *names):
        """a stage that maps rows to rows: fn(the sources' live rows of every utterance, stacked) in one evaluation"""
        live_b = [(b, rate * L) for b, L in enumerate(geo["L"]) if L > 0]
        out = torch.zeros(shape_of(stage, geo), dtype=dtype)
        if live_b:
            srcs = [g(n) for n in names]
            r = fn(*(torch.cat([rows_of(x, b, n) for b, n in live_b]) for x in srcs))
            for (b, n), rows in zip(live_b, r.split([n for _, n in live_b])):
                out[b, :, :n] = rows.T
        return out

    def embed_norm(pre, x):
        y = layernorm(x, w[pre + "out.1.weight"], w[pre + "out.1.bias"], mut)
        return y if mut == "no_sqrt" else y * math.sqrt(D)

    with torch.inference_mode():
        if stage in ("PE1", "PE2"):
            return pos_table(rate * geo["T"], dtype, table, mut)
        blk = block_of(stage)
        if blk:
            kind, pre, x_in, _, _ = blk
            sfx = stage[len(kind):]
            a, f = pre + "self_attn.", pre + "feed_forward."
            if kind == "POS":
                return F.linear(g(sources_of(stage)[0]), w[a + "linear_pos.weight"])
            if kind == "LN1":
                return per_row(lambda x: layernorm(x, w[pre + "norm_mha.weight"], w[pre + "norm_mha.bias"], mut), x_in)
            if kind == "QKV":
                return per_row(lambda x: torch.cat([lin(a + "linear_" + c, x) for c in "qkv"], dim=1), "LN1" + sfx)
            if kind == "ATT":
                chunk = 0 if not geo["streaming"] else CHUNK if (rate == 1 or mut == "chunk_25") else 2 * CHUNK
                pos = g("POS" + sfx)
                return per_utt(lambda b, n: attention(rows_of(g("QKV" + sfx), b, n), pos, w[a + "pos_bias_u"], w[a + "pos_bias_v"],
                                                      rate * geo["T"], chunk, mut, geo["L"][b] if mut == "keys_L" else None))
            if kind == "X1":
                return per_row(lambda att, x: lin(a + "linear_out", att) + (0.0 if mut == "no_residual" else x), "ATT" + sfx, x_in)
            if kind == "LN2":
                return per_row(lambda x: layernorm(x, w[pre + "norm_ff.weight"], w[pre + "norm_ff.bias"], mut), "X1" + sfx)
            if kind == "FF":
                act = torch.sigmoid if mut == "silu_sigmoid" else F.silu
                return per_row(lambda x: act(lin(f + "w_1", x)), "LN2" + sfx)
            if kind == "X2":
                return per_row(lambda ff, x: lin(f + "w_2", ff) + (0.0 if mut == "no_residual" else x), "FF" + sfx, "X1" + sfx)
        ids = src["in"]["ids"] if "in" in src else None
        emb = lambda t: F.embedding(t.clamp(0, spec.PROMPT_VOCAB - 1), w["input_embedding.weight"])
        if stage == "EMB":
            return per_utt(lambda b, n: emb(ids[b][:n]))
        if stage == "EL":
            return per_row(lambda x: lin(e + "embed.out.0", x), "EMB")
        if stage == "E0":      # the context rows are embedded like the others, row-wise (upsample_encoder.py:446-453)
            def e0(b, n):
                x, c = rows_of(g("EL"), b, n), geo["ctx"][b]
                if c:
                    x = torch.cat([x, lin(e + "embed.out.0", emb(ids[b][n:n + c]))])
                return embed_norm(e + "embed.", x)
            return per_utt(e0)
        if stage == "C1":      # conv k4 over t .. t + 3: behind the last encoded row the context rows, then zeros; LeakyReLU is LA's
            def c1(b, n):
                c = 0 if mut == "c1_zero_ctx" else geo["ctx"][b]
                x = g("E0")[b:b + 1, :, :n + c]
                x = F.pad(x, (1, LOOKAHEAD - 1)) if mut == "tap_off" else F.pad(x, (0, LOOKAHEAD))
                y = F.conv1d(x, w[e + "pre_lookahead_layer.conv1.weight"], w[e + "pre_lookahead_layer.conv1.bias"])
                return y[0, :, :n].T
            return per_utt(c1)
        if stage == "LA":      # causal conv k3 over t - 2 .. t of LeakyReLU(conv1), + the embedding
            def la(b, n):
                m = n + geo["ctx"][b] if mut == "c2_ctx" else n      # c2_ctx: conv2 and its residual take the context rows for live ones
                h = F.leaky_relu(g("C1")[b:b + 1, :, :m], 0.1 if mut == "lrelu_slope" else 0.01)
                h = F.pad(h, (3, 0))[..., :-1] if mut == "tap_off" else F.pad(h, (2, 0))
                y = F.conv1d(h, w[e + "pre_lookahead_layer.conv2.weight"], w[e + "pre_lookahead_layer.conv2.bias"])[0].T
                return y if mut == "no_residual" else y + rows_of(g("E0"), b, m)
            return per_utt(la)
        if stage == "REP":
            def rep(b, n):
                x = rows_of(g(sources_of(stage)[0]), b, n // 2)
                if mut == "rep_round":      # (v + 1) >> 1 in place of v >> 1
                    return x[((torch.arange(n) + 1) // 2).clamp_max(n // 2 - 1)]
                return x.repeat_interleave(2, dim=0)
            return per_utt(rep)
        if stage == "UP":      # conv k5 over u - 4 .. u, zeros ahead of the utterance's start
            def up(b, n):
                x = g("REP")[b:b + 1, :, :n]
                if mut == "up_cross":      # what lies ahead of the start is read: there, a copy of the first live column
                    x = torch.cat([x[..., :1].expand(-1, -1, 4), x], dim=-1)
                else:
                    x = F.pad(x, (5, 0))[..., :-1] if mut == "tap_off" else F.pad(x, (4, 0))
                return F.conv1d(x, w[e + "up_layer.conv.weight"], w[e + "up_layer.conv.bias"])[0].T
            return per_utt(up)
        if stage == "UL":
            return per_row(lambda x: lin(e + "up_embed.out.0", x), "UP")
        if stage == "U0":
            return per_row(lambda x: embed_norm(e + "up_embed.", x), "UL")
        if stage == "AN":
            return per_row(lambda x: layernorm(x, w[e + "after_norm.weight"], w[e + "after_norm.bias"], mut), sources_of(stage)[0])
        if stage == "H":
            return per_row(lambda x: lin("encoder_proj", x), "AN")
    raise KeyError(stage)


def chain(inp, geo, dtype=torch.float64, table="exact", as_taps=False):
    """every stage of a batch from its inputs, each fed the previous ones in `dtype`: {stage: tensor}, "in" included.  as_taps:
    every stage is rounded to fp32 before the next one reads it -- what the GPU test's references are fed (a run's own taps), so
    that a stage's floor is its own arithmetic's and not the rounding of its input"""
    out = {"in": inp}
    for stage in TAPS:
        out[stage] = evaluate(stage, weights(), out, geo, dtype, table=table)
        if as_taps:
            out[stage] = out[stage].float()
    return out


@functools.lru_cache(maxsize=None)
def tap_chain(name, mode, streaming):
    """the fp64 chain of a run with fp32 taps, every block (host test; the conditions on the cases)"""
    inp = inputs(name)
    return chain(inp, geometry(inp, mode, streaming), as_taps=True)
