"""GPU: the four fused row-owning launches -- rowblock_kernel, rowffn_kernel, rowres_kernel, hiftpair_kernel -- and rowgemm's
q | k | v epilogue, each called through its operator hook (jv_op_rowblock, jv_op_rowres, jv_op_hiftpair, jv_op_rowgemm_qkv) and
held to a plain fp64 PyTorch evaluation of the formulas in the kernel headers, at a few hundred rows: three utterances whose
boundaries and masked tails fall inside tiles and on tile seams, three or more workgroups with a ragged last one at every tile
height, and one row count that is an exact multiple of the tile.

The bound is measured, not chosen: every case evaluates the same chain in fp32 torch on the CPU; its worst row (each row against
its OWN magnitude: row_err) is the floor, and the kernel's worst row may be RATIO = 8 times that -- 4 x for fp16x3's 22 significant
bits against fp32's 24, 2 x for the summation order inside the MFMAs.  Kernel distance, floor and ratio of every case go to
parity_fused_ops.json in the output directory (parity_util.Recorder).  tests/test_fused_refs_host.py applies plausible mistakes
to these references, without a GPU, and checks that each lands outside that bound on these inputs.

The references and inputs live in this file (ref_*, *_inputs) and use no library code."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import parity_util as pu

pytestmark = pytest.mark.gpu

RATIO = 8.0
LENS, L = (61, 37, 50), 61          # three utterances in the flow geometry: G = 4 leading rows, 4 gap rows behind each
G, GAP = 4, 4
record = pu.Recorder("parity_fused_ops.json", {
    "what": "worst row of |kernel - fp64| / max |fp64 row| (kernel), of the same chain in fp32 torch on the CPU (floor), and their ratio",
    "bound": "kernel <= 8 x floor", "lens": list(LENS)})


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry
def geometry(lens=LENS, T=L, compact=False, total=None, lead=G, gap=GAP):
    """rows of a batch: `lead` rows, then per utterance T + gap rows (uniform: every utterance padded to T) or len + gap rows
    (compact), then masked rows up to `total`.  -> dict(M, mask uint8 [M], slot int32 [M], start, lens, S)"""
    starts, r = [], lead
    for n in lens:
        starts.append(r)
        r += (n if compact else T) + gap
    M = max(r, total or 0)
    mask = torch.zeros(M, dtype=torch.uint8)
    slot = torch.zeros(M, dtype=torch.int32)
    for b, (s, n) in enumerate(zip(starts, lens)):
        mask[s:s + n] = 1
        slot[s:] = b
    return {"M": M, "mask": mask, "slot": slot, "start": starts, "lens": list(lens), "S": T + gap, "compact": compact, "lead": lead}


def utt_rows(geo, b):
    return slice(geo["start"][b], geo["start"][b] + geo["lens"][b])


def flow_geometry(layout, tile):
    """the three layouts of the trunk kernels' cases; `tile`: output rows per workgroup (16 RT, or 16 RT - 2 for rowres)"""
    if layout == "exact":      # the uniform layout, with masked rows behind it up to a whole number of tiles
        rows = geometry()["M"]
        return geometry(total=-(-rows // tile) * tile)
    return geometry(compact=layout == "compact")


def pad_rows(t, rows, fill=float("nan")):
    out = torch.full((rows,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    out[:t.shape[0]] = t
    return out


def dirty(t, mask, value=float("nan")):
    """rows with mask == 0 replaced by `value`: what a masked row holds must not matter"""
    out = t.clone()
    out[mask == 0] = value
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# error measure
def row_err(got, want, scale):
    """worst row of |got - want| against that ROW's own scale (tests/test_gpu_ops.py)"""
    e = (got.double().cpu() - want).abs().amax(dim=1)
    return float((e / scale.clamp_min(1e-30)).max())


def distances(got, ref64, ref32, sel):
    """(kernel distance, fp32 floor) over the rows `sel` (a bool [rows] or slice), each row against the magnitude of its fp64 row"""
    scale, got = ref64.abs().amax(dim=1), got.double().cpu()
    return row_err(got[sel], ref64[sel], scale[sel]), row_err(ref32[sel], ref64[sel], scale[sel])


def hold(key, got, ref64, ref32, sel):
    kd, fl = distances(got, ref64, ref32, sel)
    record(key, kernel=kd, floor=fl, ratio=kd / fl)
    assert fl > 0.0 and math.isfinite(kd), (key, kd, fl)
    assert kd <= RATIO * fl, (key, kd, fl, kd / fl)
    return kd


# ---------------------------------------------------------------------------------------------------------------------------------
# references: plain torch in `dtype` (fp64: the reference; fp32: the floor); `mut`: one deliberate mistake (test_fused_refs_host.py)
def layer_norm(x, g, b, eps=1e-5):
    return F.layer_norm(x, (x.shape[1],), g, b, eps)


def gelu_tanh(x):
    return F.gelu(x, approximate="tanh")


def conv_rows(x, Wp, ntaps, row0, dil):
    """out[m] = sum_j x[m + row0 + j dil] @ Wp[:, j C : (j + 1) C]^T, rows outside the buffer read as zero (tap-major weights)"""
    rows, C = x.shape
    out = torch.zeros(rows, Wp.shape[0], dtype=x.dtype)
    for j in range(ntaps):
        off = row0 + j * dil
        src = torch.zeros_like(x)
        lo, hi = max(0, -off), min(rows, rows - off)
        if hi > lo:
            src[lo:hi] = x[lo + off:hi + off]
        out += src @ Wp[:, j * C:(j + 1) * C].T
    return out


def cast(p, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in p.items()}


def ref_rowblock(p, dtype=torch.float64, mut=None):
    """rowblock_kernel.h: h += to_out(att) + bo; x = LayerNorm3(h); out = h + ff.net.2(gelu(ff.net.0(x))); x' = LayerNorm1(out);
    q | k | v = Wq x'.  Every row by itself."""
    c = cast(p, dtype)
    eps = 1e-6 if mut == "ln_eps" else 1e-5
    act = gelu_tanh if mut == "gelu_tanh" else F.gelu
    h = c["h"] + c["att"] @ c["Wo"].T + (0 if mut == "drop_bo" else c["bo"])
    x = layer_norm(h, c["ln3_g"], c["ln3_b"], eps)
    hid = act(x @ c["W1"].T + (0 if mut == "drop_b1" else c["b1"]))
    out = h + hid @ c["W2"].T + (0 if mut == "drop_b2" else c["b2"])
    ln = layer_norm(out, c["ln1_g"], c["ln1_b"], eps)
    qkv = ln @ c["Wq"].T
    q, k, v = qkv[:, :512], qkv[:, 512:1024], qkv[:, 1024:]
    if mut == "kv_scales_swapped":      # the planes carry k * k_scale and v * v_scale; read back with the scales exchanged
        k, v = k * (p["v_scale"] / p["k_scale"]), v * (p["k_scale"] / p["v_scale"])
    return {"h": h, "out": out, "ln": ln, "q": q, "k": k, "v": v}


def ref_rowffn(p, dtype=torch.float64, mut=None):
    """rowffn_kernel: out = res + ff.net.2(gelu(ff.net.0(x))) from the LayerNorm3 output x; x' = LayerNorm1(out)"""
    c = cast(p, dtype)
    act = gelu_tanh if mut == "gelu_tanh" else F.gelu
    hid = act(c["x"] @ c["W1"].T + (0 if mut == "drop_b1" else c["b1"]))
    out = c["h"] + hid @ c["W2"].T + (0 if mut == "drop_b2" else c["b2"])
    return {"out": out, "ln": layer_norm(out, c["ln1_g"], c["ln1_b"], 1e-6 if mut == "ln_eps" else 1e-5)}


def ref_rowres(p, dtype=torch.float64, mut=None):
    """rowres_kernel.h: h2 = Mish(LayerNorm1(conv3_causal(x mask) + b1)) mask + temb; out = Mish(LayerNorm2(conv3_causal(h2 mask) + b2))
    mask + res_conv(x mask); x' = LayerNorm1_next(out); q | k | v = Wq x'.  Causal: tap j reads row m - 2 + j."""
    c = cast(p, dtype)
    m = p["mask"].to(dtype)[:, None]
    eps = 1e-6 if mut == "ln_eps" else 1e-5
    act = F.silu if mut == "mish_silu" else F.mish
    row0 = -1 if mut == "tap_shift" else -2
    xm = torch.where(m != 0, c["x"], torch.zeros((), dtype=dtype))
    c1 = conv_rows(xm, c["W1"], 3, row0, 1) + (0 if mut == "drop_b1" else c["b1"])
    if mut == "mask_before_ln":        # block1's mask moved ahead of LayerNorm -> Mish: a masked h2 row then reads as Mish(ln1_b) + temb
        h2m = act(layer_norm(c1 * m, c["ln1_g"], c["ln1_b"], eps)) + c["temb"]
    elif mut == "temb_before_mish":    # the time embedding added ahead of Mish and the mask instead of behind them
        h2m = act(layer_norm(c1, c["ln1_g"], c["ln1_b"], eps) + c["temb"]) * m
    else:
        h2 = act(layer_norm(c1, c["ln1_g"], c["ln1_b"], eps)) * m + c["temb"]
        h2m = h2 * m
    c2 = conv_rows(h2m, c["W2"], 3, row0, 1) + (0 if mut == "drop_b2" else c["b2"])
    xr = c["x"] if mut == "res_unmasked_x" else xm
    res = xr @ c["Wr"].T + (0 if mut == "drop_br" else c["br"])
    out = act(layer_norm(c2, c["ln2_g"], c["ln2_b"], eps)) * m + res
    ln = layer_norm(out, c["lnf_g"], c["lnf_b"], eps)
    qkv = ln @ c["Wq"].T
    q, k, v = qkv[:, :512], qkv[:, 512:1024], qkv[:, 1024:]
    if mut == "kv_scales_swapped":
        k, v = k * (p["v_scale"] / p["k_scale"]), v * (p["k_scale"] / p["v_scale"])
    return {"out": out, "ln": ln, "q": q, "k": k, "v": v}


def snake(x, alpha):
    return x + torch.sin(x * alpha) ** 2 / (alpha + 1e-9)


def ref_hiftpair(p, dtype=torch.float64, mut=None):
    """hiftpair_kernel.h: y = (Conv1d_k,dil(Snake1(A mask)) + b1) mask; out = ((Conv1d_k(Snake2(y)) + b2) + A + res2) out_scale + prev,
    "same" padding on both; rows with mask == 0 read as zero as A and as the intermediate"""
    c = cast(p, dtype)
    k, dil = p["k"], p["dil"]
    m = p["mask"].to(dtype)[:, None]
    a = torch.where(m != 0, c["A"], torch.zeros((), dtype=dtype))
    shift = 1 if mut == "tap_shift" else 0
    y = conv_rows(snake(a, c["alpha1"]), c["W1"], k, -(dil * (k - 1) // 2) + shift, dil)
    if mut == "mask_before_bias":      # the intermediate's mask applied to the accumulators, ahead of the bias: a masked row reads as Snake2(b1)
        y = y * m + c["b1"]
    else:
        y = (y + (0 if mut == "drop_b1" else c["b1"])) * m
    d2 = dil if mut == "conv2_dilation" else 1
    z = conv_rows(snake(y, c["alpha1"] if mut == "snake2_alpha1" else c["alpha2"]), c["W2"], k, -(d2 * (k - 1) // 2), d2)
    z = z + (0 if mut == "drop_b2" else c["b2"])
    if mut == "res_after_scale":
        out = z * p["out_scale"] + a + c["res2"]
    else:
        out = ((z + a) + c["res2"]) * p["out_scale"]
    return {"out": out + c["prev"]}


def ref_hiftconv(p, dtype=torch.float64):
    """hiftconv_kernel.h: out = ((Conv1d_k,dil(Snake(A mask)) + b) + res1 + res2) out_scale + prev, "same" padding"""
    c = cast(p, dtype)
    k, dil = p["k"], p["dil"]
    a = torch.where(p["mask"][:, None] != 0, c["A"], torch.zeros((), dtype=dtype))
    y = conv_rows(snake(a, c["alpha1"]), c["W1"], k, -(dil * (k - 1) // 2), dil) + c["b1"]
    return {"out": ((y + c["res1"]) + c["res2"]) * p["out_scale"] + c["prev"]}


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs that discriminate: LayerNorm gains over [0.5, 2.5] with offsets, biases everywhere, weight rows of very different scale,
# residual rows over six decades, a time embedding of order 1, Snake alphas down to 0.05, utterances of scale 1e-3 / 1 / 30
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _weight(g, N, K, spread=1.0):
    return torch.randn(N, K, generator=g) / math.sqrt(K) * torch.exp(spread * torch.randn(N, 1, generator=g))


def _ln(g, n=256):
    return 0.5 + 2.0 * torch.rand(n, generator=g), 0.3 * torch.randn(n, generator=g)


def _ln_bound(gain, offset):
    return 16.0 * float(gain.abs().max()) + float(offset.abs().max())      # |LayerNorm_256(x) g + b| <= sqrt(255) max|g| + max|b|


def _l1(W):
    return float(W.abs().sum(dim=1).max())


def _h3_scale(bound):
    """registry.hip h3_scale_for_bound: the largest power of two s with bound s <= 60000 (|e| <= 24)"""
    s = 2.0 ** min(max(math.floor(math.log2(60000.0 / bound)), -24), 24)
    while bound * s > 60000.0:
        s *= 0.5
    return s


def _qkv_weight(g):
    """to_q | to_k | to_v; v's rows 8 x larger than k's, so that the two plane scales differ (a swap of them must show)"""
    Wq = _weight(g, 1536, 256, 0.5)
    Wq[1024:] *= 8.0
    return Wq


def _qkv_bounds(p, ln_bound):
    p["k_bound"], p["v_bound"] = _l1(p["Wq"][512:1024]) * ln_bound, _l1(p["Wq"][1024:]) * ln_bound
    p["k_scale"], p["v_scale"] = _h3_scale(p["k_bound"]), _h3_scale(p["v_bound"])
    assert p["k_scale"] != p["v_scale"]


@functools.lru_cache(maxsize=None)
def rowblock_inputs(M, seed=1):
    g = _gen(seed)
    # residual rows over six decades; the attention rows of the small ones are small too and to_out's / ff.net.2's biases and
    # ff.net.2 itself are of order 0.05, so that some rows of h and of out have a variance near 1e-3: that is where a LayerNorm
    # eps of 1e-6 instead of 1e-5 shows (test_fused_refs_host.py)
    decade = (10.0 ** (torch.arange(M) % 7 - 3).float())[:, None]
    p = {"att": torch.randn(M, 512, generator=g) * torch.exp(torch.randn(M, 1, generator=g)) * (10.0 * decade).clamp(max=1.0),
         "h": torch.randn(M, 256, generator=g) * decade}
    p["Wo"], p["bo"] = _weight(g, 256, 512), 0.05 * torch.randn(256, generator=g)
    p["ln3_g"], p["ln3_b"] = _ln(g)
    p["W1"], p["b1"] = _weight(g, 1024, 256, 0.5), 0.5 * torch.randn(1024, generator=g)
    p["W2"], p["b2"] = 0.05 * _weight(g, 256, 1024, 0.5), 0.05 * torch.randn(256, generator=g)
    p["ln1_g"], p["ln1_b"] = _ln(g)
    p["Wq"] = _qkv_weight(g)
    # the bounds behind the plane scales, as registry.hip proves them: LayerNorm outputs, |gelu(x)| <= |x|, row L1 norms
    b3, b1 = _ln_bound(p["ln3_g"], p["ln3_b"]), _ln_bound(p["ln1_g"], p["ln1_b"])
    p["bounds"] = {"att": float(p["att"].abs().max()), "ln3": b3, "hid": _l1(p["W1"]) * b3 + float(p["b1"].abs().max()), "ln1": b1}
    _qkv_bounds(p, b1)
    p["bounds"].update(k=p["k_bound"], v=p["v_bound"])
    return p


@functools.lru_cache(maxsize=None)
def rowffn_inputs(M, seed=2):
    p = dict(rowblock_inputs(M, seed))
    g = _gen(seed + 100)
    p["x"] = torch.randn(M, 256, generator=g) * p["ln3_g"] + p["ln3_b"]      # LayerNorm-like rows, inside the proven bound
    return p


@functools.lru_cache(maxsize=None)
def rowres_inputs(layout, tile, cin, seed=3):
    geo = flow_geometry(layout, tile)
    M = geo["M"]
    g = _gen(seed + cin)
    utt_scale = torch.tensor([1.0, 30.0, 0.01])      # the utterances' own magnitudes: a wrong slot overflows or loses the small one
    p = {"mask": geo["mask"], "geo": geo, "x": torch.randn(M, cin, generator=g) * utt_scale[geo["slot"].long()][:, None]}
    p["W1"], p["b1"] = _weight(g, 256, 3 * cin), 0.5 * torch.randn(256, generator=g)
    p["ln1_g"], p["ln1_b"] = _ln(g)
    p["Wr"], p["br"] = _weight(g, 256, cin), torch.randn(256, generator=g)
    p["temb"] = torch.randn(256, generator=g)
    p["W2"], p["b2"] = _weight(g, 256, 768), 0.5 * torch.randn(256, generator=g)
    p["ln2_g"], p["ln2_b"] = _ln(g)
    p["lnf_g"], p["lnf_b"] = _ln(g)
    p["Wq"] = _qkv_weight(g)
    p["lnf_bound"] = _ln_bound(p["lnf_g"], p["lnf_b"])
    _qkv_bounds(p, p["lnf_bound"])
    p["amax_in"] = torch.stack([p["x"][utt_rows(geo, b)].abs().max() for b in range(len(geo["lens"]))])
    return p


def hift_rows(k):
    return 2 * (160 - (k - 1)) + 37


@functools.lru_cache(maxsize=None)
def hiftpair_inputs(C, k, dil, seed=4, lead=16):
    """about 2 (160 - (k - 1)) + 37 rows: three workgroups, the last one ragged; three utterances with 32-row gaps and ragged tails"""
    total = hift_rows(k)
    T = (total - lead) // 3 - 32
    geo = geometry(lens=(T, T - 13, T - 29), T=T, total=total, lead=lead, gap=32)
    M = geo["M"]
    g = _gen(seed + 1000 * C + 10 * k + dil)
    utt_scale = torch.tensor([1e-3, 1.0, 30.0])
    p = {"mask": geo["mask"], "geo": geo, "k": k, "dil": dil, "out_scale": 1.0 / 3.0,
         "A": torch.randn(M, C, generator=g) * utt_scale[geo["slot"].long()][:, None]}
    for i in "12":
        p["W" + i], p["b" + i] = _weight(g, C, k * C, 0.5), 0.1 * torch.randn(C, generator=g)
        p["alpha" + i] = 0.05 * 40.0 ** torch.rand(C, generator=g)      # log-uniform over [0.05, 2]
        p["alpha" + i][0] = 0.05
    p["res2"] = torch.randn(M, C, generator=g) * utt_scale[geo["slot"].long()][:, None]
    p["prev"] = torch.randn(M, C, generator=g) * utt_scale[geo["slot"].long()][:, None]
    p["amax_in"] = torch.stack([p["A"][utt_rows(geo, b)].abs().max() for b in range(3)])
    return p


@functools.lru_cache(maxsize=None)
def hiftconv_inputs(C, k, dil, seed=5):
    """hiftpair_inputs' rows, utterances and first convolution with a first residual, behind 8 leading rows: an utterance's first
    row is then never a multiple of 16 (the stride is 115 / 112 / 109 rows at k = 3 / 7 / 11; behind 16 rows, k = 3 has 16 + 112 b)"""
    p = dict(hiftpair_inputs(C, k, dil, seed, lead=8))
    geo = p["geo"]
    p["res1"] = torch.randn(geo["M"], C, generator=_gen(seed + 7)) * torch.tensor([1e-3, 1.0, 30.0])[geo["slot"].long()][:, None]
    return p


@functools.lru_cache(maxsize=None)
def refs(kind, *key):
    """(inputs, fp64 reference, fp32 floor chain) of a case, computed once and shared"""
    p = {"rowblock": rowblock_inputs, "rowffn": rowffn_inputs, "rowres": rowres_inputs, "hiftpair": hiftpair_inputs,
         "hiftconv": hiftconv_inputs}[kind](*key)
    f = {"rowblock": ref_rowblock, "rowffn": ref_rowffn, "rowres": ref_rowres, "hiftpair": ref_hiftpair, "hiftconv": ref_hiftconv}[kind]
    return p, f(p), f(p, torch.float32)


def to_dev(p, dev, names):
    return {k: p[k].to(dev) for k in names}


def stream_noise(dev):
    return torch.empty(64 << 20, device=dev)


# ---------------------------------------------------------------------------------------------------------------------------------
# rowgemm's q | k | v epilogue
@pytest.mark.parametrize("rt", [2, 5])
def test_rowgemm_qkv_splits(dev, rt):
    """RG_QKV at nsplit 1, 2, 3, 6 and tile heights 2 and 5: identical bits across the column splits, fp64 parity of q, k and v,
    rows past M untouched"""
    from jyutvoice_amd.engine import op_rowgemm_qkv
    M = 199
    p = rowblock_inputs(M)
    g = _gen(50 + rt)
    A = torch.randn(M + 9, 256, generator=g) * p["ln1_g"] + p["ln1_b"]
    ref64, ref32 = A.double() @ p["Wq"].double().T, A @ p["Wq"].T
    first = None
    for nsplit in (1, 2, 3, 6):
        q, k, v, kv2 = op_rowgemm_qkv(A.to(dev), p["Wq"].to(dev), p["bounds"]["ln1"], p["k_bound"], p["v_bound"], M=M, nsplit=nsplit, rt=rt)
        if first is None:
            first = (q, kv2)
            rows = slice(0, M)
            hold(f"rowgemm_qkv/rt{rt}/q", q, ref64[:, :512], ref32[:, :512], rows)
            hold(f"rowgemm_qkv/rt{rt}/k", k, ref64[:, 512:1024], ref32[:, 512:1024], rows)
            hold(f"rowgemm_qkv/rt{rt}/v", v, ref64[:, 1024:], ref32[:, 1024:], rows)
            assert torch.isnan(q[M:]).all() and torch.isnan(kv2[:, M:]).all()
        else:
            assert torch.equal(q[:M], first[0][:M]) and torch.equal(kv2[:, :M], first[1][:, :M]), nsplit


# ---------------------------------------------------------------------------------------------------------------------------------
# rowblock / rowffn
BLOCK_W = ("Wo", "bo", "ln3_g", "ln3_b", "W1", "b1", "W2", "b2", "ln1_g", "ln1_b", "Wq")


def block_case(layout, rt):
    geo = flow_geometry(layout, 16 * rt)
    rows = -(-geo["M"] // (16 * rt)) * 16 * rt      # the row buffers hold whole tiles; rows past M hold NaN
    return geo, rows


def run_block(dev, p, geo, rows, mode, fused=1, out_ld=None, nan=True, scale_utt=None, key="att", att_bound_mul=1.0):
    """one call of the hook on the case's rows.  nan: masked rows and the rows past M hold NaN; scale_utt: that utterance's
    inputs x 1000 (att_bound_mul: the attention bound is one scale for the whole batch, so both runs of such a pair take the
    larger one)"""
    from jyutvoice_amd.engine import op_rowblock
    a, h = p[key].clone(), p["h"].clone()
    if scale_utt is not None:
        a[utt_rows(geo, scale_utt)] *= 1000.0
        h[utt_rows(geo, scale_utt)] *= 1000.0
    if nan:
        a, h = dirty(a, geo["mask"]), dirty(h, geo["mask"])
    bounds = dict(p["bounds"], att=att_bound_mul * p["bounds"]["att"])
    w = to_dev(p, dev, BLOCK_W)
    return op_rowblock(pad_rows(a, rows).to(dev), pad_rows(h, rows).to(dev), geo["M"], w, bounds, mode=mode, fused=fused, out_ld=out_ld,
                       row_slot=pad_rows(geo["slot"], rows, 0).to(dev), row_mask=pad_rows(geo["mask"], rows, 0).to(dev),
                       nslots=len(geo["lens"]))


def live(geo):
    return geo["mask"].bool()


def tracked(t, geo):
    """the largest stored magnitude over the unmasked rows of each utterance's slot"""
    t = t.cpu()
    return torch.stack([t[utt_rows(geo, b)].abs().max() for b in range(len(geo["lens"]))])


def same_bits(a, b, sel, names):
    for n in names:
        if a[n] is None:
            continue
        # bit patterns, not values: "the same bits" includes the NaN the untouched columns of a strided output buffer still hold
        x, y = (t.cpu().view(torch.int16 if t.dtype == torch.float16 else torch.int32) for t in (a[n], b[n]))
        if x.dim() == 1:      # tracked maxima, one per utterance
            assert torch.equal(x, y), n
        elif x.dim() == 3:      # planes [2][rows][C]
            assert torch.equal(x[:, :sel.shape[0]][:, sel], y[:, :sel.shape[0]][:, sel]), n
        else:
            assert torch.equal(x[:sel.shape[0]][sel], y[:sel.shape[0]][sel]), n


OUTS = ("h", "out", "ln_planes", "q", "kv2")


@pytest.mark.parametrize("layout", ["uniform", "compact", "exact"])
@pytest.mark.parametrize("rt", [2, 3, 4, 5])
def test_rowblock_fp64(dev, monkeypatch, rt, layout):
    """every stored output of the fused block against fp64, in each of its modes: (a) a separate output buffer of stride 512 --
    h after phase A and out; (b) LayerNorm1 planes to HBM; (c) q | k | v.  Masked rows and the rows past M hold NaN; the tracked
    maxima are exactly the largest stored magnitudes of each utterance's unmasked rows; fused equals the separate launchers bit
    for bit (rowblock_kernel.h)."""
    monkeypatch.setenv("JV_ROWGEMM_RT", str(rt))
    monkeypatch.delenv("JV_FF_STAGGER", raising=False)
    geo, rows = block_case(layout, rt)
    M, sel = geo["M"], live(geo)
    p, r64, r32 = refs("rowblock", M)
    tag = f"rowblock/rt{rt}/{layout}"
    # (a) a stage's last block: out is the concat buffer
    a = run_block(dev, p, geo, rows, "plain", out_ld=512)
    hold(tag + "/a/h", a["h"][:M], r64["h"], r32["h"], sel)
    hold(tag + "/a/out", a["out"][:M, :256], r64["out"], r32["out"], sel)
    assert torch.isnan(a["out"][:, 256:]).all() and torch.isnan(a["out"][M:]).all()      # nothing beside or behind the rows is written
    assert torch.equal(a["amax_h"].cpu(), tracked(a["h"], geo))
    assert torch.equal(a["amax_out"].cpu(), tracked(a["out"][:, :256], geo))
    same_bits(a, run_block(dev, p, geo, rows, "plain", out_ld=512, nan=False), sel, OUTS)      # what a masked row holds does not matter
    same_bits(a, run_block(dev, p, geo, rows, "plain", fused=0, out_ld=512), sel, OUTS + ("amax_h", "amax_out"))
    # (b) in place, LayerNorm1 planes to HBM
    b = run_block(dev, p, geo, rows, "ln")
    hold(tag + "/b/out", b["out"][:M], r64["out"], r32["out"], sel)
    hold(tag + "/b/ln", b["ln"][:M], r64["ln"], r32["ln"], sel)
    assert torch.isnan(b["ln_planes"][:, M:]).all()
    assert torch.equal(b["out"][:M].cpu()[sel], a["out"][:M, :256].cpu()[sel])
    same_bits(b, run_block(dev, p, geo, rows, "ln", fused=0), sel, OUTS + ("amax_h", "amax_out"))
    # (c) with the next block's q | k | v
    c = run_block(dev, p, geo, rows, "qkv")
    hold(tag + "/c/out", c["out"][:M], r64["out"], r32["out"], sel)
    for n in "qkv":
        hold(f"{tag}/c/{n}", c[n][:M], r64[n], r32[n], sel)
    assert torch.isnan(c["q"][M:]).all() and torch.isnan(c["kv2"][:, M:]).all()
    assert torch.equal(c["amax_out"].cpu(), tracked(c["out"], geo))
    same_bits(c, run_block(dev, p, geo, rows, "qkv", fused=0), sel, OUTS + ("amax_h", "amax_out"))
    same_bits(c, run_block(dev, p, geo, rows, "qkv", fused=-1), sel, OUTS + ("amax_h", "amax_out"))


@pytest.mark.parametrize("layout", ["uniform", "compact", "exact"])
@pytest.mark.parametrize("rt", [2, 3, 4, 5])
def test_rowffn_fp64(dev, monkeypatch, rt, layout):
    """(d) the feed-forward pair alone (rowffn_kernel): LayerNorm planes in, residual, LayerNorm planes out; against fp64, and bit
    for bit against rowgemm<gelu> + rowgemm<res,ln>"""
    monkeypatch.setenv("JV_ROWGEMM_RT", str(rt))
    geo, rows = block_case(layout, rt)
    M, sel = geo["M"], live(geo)
    p, r64, r32 = refs("rowffn", M)
    d = run_block(dev, p, geo, rows, "ffn", key="x")
    hold(f"rowffn/rt{rt}/{layout}/out", d["out"][:M], r64["out"], r32["out"], sel)
    hold(f"rowffn/rt{rt}/{layout}/ln", d["ln"][:M], r64["ln"], r32["ln"], sel)
    assert torch.equal(d["amax_out"].cpu(), tracked(d["out"], geo))
    assert torch.isnan(d["ln_planes"][:, M:]).all()
    same_bits(d, run_block(dev, p, geo, rows, "ffn", key="x", nan=False), sel, OUTS)
    same_bits(d, run_block(dev, p, geo, rows, "ffn", key="x", fused=-1), sel, OUTS + ("amax_out",))


@pytest.mark.parametrize("rt", [2, 5])
def test_rowblock_stagger_equals_lockstep(dev, monkeypatch, rt):
    """JV_FF_STAGGER=1 (waves 0..3 half a hidden chunk ahead of waves 4..7) gives the bits of the lockstep schedule"""
    monkeypatch.setenv("JV_ROWGEMM_RT", str(rt))
    geo, rows = block_case("uniform", rt)
    p, _, _ = refs("rowblock", geo["M"])
    for mode in ("plain", "qkv"):
        monkeypatch.delenv("JV_FF_STAGGER", raising=False)
        lock = run_block(dev, p, geo, rows, mode)
        monkeypatch.setenv("JV_FF_STAGGER", "1")
        stag = run_block(dev, p, geo, rows, mode)
        same_bits(lock, stag, live(geo), OUTS + ("amax_h", "amax_out"))


@pytest.mark.parametrize("layout", ["uniform", "compact"])
def test_rowblock_utterances_independent(dev, monkeypatch, layout):
    """one utterance's inputs x 1000: the other utterances' rows and tracked maxima keep their bits (the slot table in both
    geometries)"""
    monkeypatch.setenv("JV_ROWGEMM_RT", "3")
    geo, rows = block_case(layout, 3)
    p, _, _ = refs("rowblock", geo["M"])
    base = run_block(dev, p, geo, rows, "qkv", att_bound_mul=1000.0)
    big = run_block(dev, p, geo, rows, "qkv", att_bound_mul=1000.0, scale_utt=1)
    others = live(geo) & (geo["slot"] != 1)
    same_bits(base, big, others, OUTS)
    for n in ("amax_h", "amax_out"):
        assert torch.equal(base[n][[0, 2]], big[n][[0, 2]]) and float(big[n][1]) > 100.0 * float(base[n][1]), n


def test_rowblock_race_screen(dev, monkeypatch):
    """the fused launch and rowffn, ten times each beside a streaming writer: identical bits (the DMA ring and the register double
    buffer are ordered by counted waits alone)"""
    monkeypatch.setenv("JV_ROWGEMM_RT", "5")
    geo, rows = block_case("uniform", 5)
    p, _, _ = refs("rowblock", geo["M"])
    pf, _, _ = refs("rowffn", geo["M"])
    first, first_f = run_block(dev, p, geo, rows, "qkv"), run_block(dev, pf, geo, rows, "ffn", key="x")
    noise = stream_noise(dev)
    for i in range(10):
        noise.normal_()
        same_bits(first, run_block(dev, p, geo, rows, "qkv"), live(geo), OUTS)
        same_bits(first_f, run_block(dev, pf, geo, rows, "ffn", key="x"), live(geo), OUTS)


# ---------------------------------------------------------------------------------------------------------------------------------
# rowres
RES_W = ("W1", "b1", "ln1_g", "ln1_b", "Wr", "br", "temb", "W2", "b2", "ln2_g", "ln2_b")
GUARD = 8      # rows behind M in the buffers: NaN, masked


def run_res(dev, p, what="qkv", table=None, nan=True, scale_utt=None, out=None):
    """one call of jv_op_rowres.  what: "plain" / "ln" (planes to HBM) / "qkv"; table: address the bounds through the row ->
    utterance table (default: the layout's own addressing -- arithmetic in the uniform geometry, the table in the compact one)"""
    from jyutvoice_amd.engine import op_rowres
    geo = p["geo"]
    M, rows = geo["M"], geo["M"] + GUARD
    x, amax = p["x"].clone(), p["amax_in"].clone()
    if scale_utt is not None:
        x[utt_rows(geo, scale_utt)] *= 1000.0
        amax[scale_utt] *= 1000.0
    if nan:
        x = dirty(x, geo["mask"])
    use_table = geo["compact"] if table is None else table
    slots = pad_rows(geo["slot"], rows, 0).to(dev) if use_table else (geo["lead"], geo["S"], len(geo["lens"]))
    amax_out = torch.zeros(len(geo["lens"]), device=dev)
    r = op_rowres(pad_rows(x, rows).to(dev), M, pad_rows(geo["mask"], rows, 0).to(dev), amax.to(dev), slots, to_dev(p, dev, RES_W),
                  lnf=None if what == "plain" else (p["lnf_g"].to(dev), p["lnf_b"].to(dev)), lnf_bound=p["lnf_bound"],
                  Wq=p["Wq"].to(dev) if what == "qkv" else None, k_bound=p["k_bound"], v_bound=p["v_bound"], amax_out=amax_out, out=out)
    r["amax_out"] = amax_out
    return r


RES_OUTS = ("out", "lnf_planes", "q", "kv2")


@pytest.mark.parametrize("cin", [256, 512])
@pytest.mark.parametrize("layout", ["uniform", "compact", "exact"])
@pytest.mark.parametrize("rt", [2, 3, 4, 5])
def test_rowres_fp64(dev, monkeypatch, rt, layout, cin):
    """the whole resnet in one launch against fp64: out on every row below M (a masked row stores res_conv's bias: zero before the
    residual), the following LayerNorm1 planes, q | k | v; per-utterance input scales 1 / 30 / 0.01 through both slot addressings;
    masked rows and guard rows hold NaN; the tracked maximum is exact; the q | k | v phase equals rowgemm<qkv> on the planes the
    launch wrote, bit for bit (rowres_kernel.h)."""
    from jyutvoice_amd.engine import op_rowgemm_qkv
    monkeypatch.setenv("JV_ROWGEMM_RT", str(rt))
    p, r64, r32 = refs("rowres", layout, 16 * rt - 2, cin)
    geo = p["geo"]
    M, sel, every = geo["M"], live(geo), slice(0, geo["M"])
    tag = f"rowres/rt{rt}/{layout}/c{cin}"
    ln = run_res(dev, p, "ln")
    hold(tag + "/out", ln["out"][:M], r64["out"], r32["out"], every)
    hold(tag + "/lnf", ln["lnf"][:M], r64["ln"], r32["ln"], sel)
    assert torch.isnan(ln["out"][M:]).all() and torch.isnan(ln["lnf_planes"][:, M:]).all()
    assert torch.equal(ln["amax_out"].cpu(), tracked(ln["out"], geo))
    qkv = run_res(dev, p, "qkv")
    assert torch.equal(qkv["out"][:M], ln["out"][:M])
    for n in "qkv":
        hold(f"{tag}/{n}", qkv[n][:M], r64[n], r32[n], sel)
    assert torch.isnan(qkv["q"][M:]).all() and torch.isnan(qkv["kv2"][:, M:]).all()
    # what a masked row holds does not matter; the other addressing of the same slots gives the same bits
    clean = run_res(dev, p, "qkv", nan=False)
    same_bits(qkv, clean, torch.ones(M, dtype=torch.bool), RES_OUTS + ("amax_out",))
    if layout != "compact":      # (the compact layout has no arithmetic addressing)
        same_bits(qkv, run_res(dev, p, "qkv", table=True), torch.ones(M, dtype=torch.bool), RES_OUTS + ("amax_out",))
    # phase C against the stand-alone q | k | v launch on the LayerNorm1 planes this kernel wrote
    q2, _, _, kv2 = op_rowgemm_qkv(None, p["Wq"].to(dev), p["lnf_bound"], p["k_bound"], p["v_bound"], M=M, planes=ln["lnf_planes"])
    assert torch.equal(q2[:M], qkv["q"][:M]) and torch.equal(kv2[:, :M], qkv["kv2"][:, :M])


@pytest.mark.parametrize("layout", ["uniform", "compact"])
def test_rowres_utterances_independent(dev, monkeypatch, layout):
    """one utterance's rows and bound x 1000: the other utterances keep their bits, through the arithmetic slots and the table"""
    monkeypatch.setenv("JV_ROWGEMM_RT", "3")
    p, _, _ = refs("rowres", layout, 46, 256)
    geo = p["geo"]
    others = live(geo) & (geo["slot"] != 1)
    for table in ([True] if layout == "compact" else [False, True]):
        base, big = run_res(dev, p, "qkv", table=table), run_res(dev, p, "qkv", table=table, scale_utt=1)
        same_bits(base, big, others, RES_OUTS)
        assert torch.equal(base["amax_out"][[0, 2]], big["amax_out"][[0, 2]])


@pytest.mark.parametrize("cin", [256, 512])
def test_rowres_against_two_rowconv_launches(dev, monkeypatch, cin):
    """fused against unfused: not bit-equal -- the fused kernel scales h2 from a bound, the unfused pair from a measurement -- so both
    are held to the same fp64 bound and their distance is reported"""
    from jyutvoice_amd.engine import op_rowconv, op_rowgemm
    monkeypatch.setenv("JV_ROWGEMM_RT", "4")
    p, r64, r32 = refs("rowres", "uniform", 62, cin)
    geo = p["geo"]
    M, mask = geo["M"], geo["mask"].to(dev)
    fused = run_res(dev, p, "plain")["out"][:M]
    w = to_dev(p, dev, RES_W)
    x = (p["x"] * geo["mask"][:, None]).to(dev)
    slot = torch.zeros(1, device=dev)
    h2 = op_rowconv(x, w["W1"], w["b1"], ln=(w["ln1_g"], w["ln1_b"]), act="mish", rowmask=mask, rowvec=w["temb"], amax_out=slot)
    res = op_rowgemm(x, w["Wr"], w["br"], a_bound=float(x.abs().max()))
    unfused = op_rowconv(h2, w["W2"], w["b2"], ln=(w["ln2_g"], w["ln2_b"]), act="mish", rowmask=mask, res=res, amax_in=slot)
    every = slice(0, M)
    hold(f"rowres_vs_rowconv/c{cin}/fused", fused, r64["out"], r32["out"], every)
    hold(f"rowres_vs_rowconv/c{cin}/unfused", unfused, r64["out"], r32["out"], every)
    record(f"rowres_vs_rowconv/c{cin}/distance", fused_unfused=row_err(fused, unfused.double().cpu(), r64["out"].abs().amax(dim=1)))


def test_rowres_rejects_in_place(dev, monkeypatch):
    """out == x: rejected on the host (a workgroup reads its neighbours' rows of x as halo), nothing is launched"""
    from jyutvoice_amd._lib import JvError
    monkeypatch.setenv("JV_ROWGEMM_RT", "3")
    p, _, _ = refs("rowres", "uniform", 46, 256)
    rows = p["geo"]["M"] + GUARD
    x = pad_rows(p["x"] * p["geo"]["mask"][:, None], rows, 0.0).to(dev)
    keep = x.clone()
    with pytest.raises(JvError, match="alias"):
        from jyutvoice_amd.engine import op_rowres
        op_rowres(x, p["geo"]["M"], pad_rows(p["geo"]["mask"], rows, 0).to(dev), p["amax_in"].to(dev),
                  (G, p["geo"]["S"], 3), to_dev(p, dev, RES_W), out=x)
    assert torch.equal(x, keep)


def test_rowres_race_screen(dev, monkeypatch):
    monkeypatch.setenv("JV_ROWGEMM_RT", "5")
    p, _, _ = refs("rowres", "uniform", 78, 512)
    every = torch.ones(p["geo"]["M"], dtype=torch.bool)
    first = run_res(dev, p, "qkv")
    noise = stream_noise(dev)
    for i in range(10):
        noise.normal_()
        same_bits(first, run_res(dev, p, "qkv"), every, RES_OUTS)


# ---------------------------------------------------------------------------------------------------------------------------------
# hiftpair
PAIR_CASES = [(C, k, dil) for C in (64, 128) for k in (3, 7, 11) for dil in (1, 3, 5) if (k - 1) * dil <= 56]
PAIR_W = ("W1", "b1", "alpha1", "W2", "b2", "alpha2")


def run_pair(dev, p, table=False, nan=True, scale_utt=None, full=True):
    """one call of jv_op_hiftpair; full: with res2, out_scale = 1/3 and accumulation onto prev"""
    from jyutvoice_amd.engine import op_hiftpair
    geo = p["geo"]
    A, amax = p["A"].clone(), p["amax_in"].clone()
    if scale_utt is not None:
        A[utt_rows(geo, scale_utt)] *= 1000.0
        amax[scale_utt] *= 1000.0
    if nan:
        A = dirty(A, geo["mask"])
    w = to_dev(p, dev, PAIR_W)
    slots = geo["slot"].to(dev) if table else (geo["lead"], geo["S"], 3)
    amax_out = torch.zeros(3, device=dev)
    out = op_hiftpair(A.to(dev), w["W1"], w["b1"], w["alpha1"], w["W2"], w["b2"], w["alpha2"], p["k"], p["dil"], amax.to(dev), slots,
                      rowmask=geo["mask"].to(dev), res2=p["res2"].to(dev) if full else None, out_scale=p["out_scale"] if full else 1.0,
                      prev=p["prev"].to(dev) if full else None, amax_out=amax_out)
    return {"out": out, "amax_out": amax_out}


@pytest.mark.parametrize("C,k,dil", PAIR_CASES)
def test_hiftpair_fp64(dev, C, k, dil):
    """a ResBlock's convolution pair in one launch against fp64, with res2, out_scale = 1/3 and accumulation: three workgroups
    (2 (160 - (k - 1)) + 37 rows), utterances of scale 1e-3 / 1 / 30 with their own measured bounds through both slot addressings,
    Snake alphas down to 0.05, masked rows holding NaN, the tracked maximum exact"""
    p, r64, r32 = refs("hiftpair", C, k, dil)
    geo = p["geo"]
    sel = live(geo)
    got = run_pair(dev, p)
    hold(f"hiftpair/C{C}/k{k}/d{dil}", got["out"], r64["out"], r32["out"], sel)
    assert torch.equal(got["amax_out"].cpu(), tracked(got["out"], geo))
    same_bits(got, run_pair(dev, p, nan=False), sel, ("out", "amax_out"))
    same_bits(got, run_pair(dev, p, table=True), sel, ("out", "amax_out"))


@pytest.mark.parametrize("C,k,dil", [(64, 3, 1), (128, 7, 3), (64, 11, 5)])
def test_hiftpair_against_two_hiftconv_launches(dev, C, k, dil):
    """fused against unfused: the pair scales its intermediate from a bound, the two launches from a measurement: both inside the
    same fp64 bound, their distance reported"""
    from jyutvoice_amd.engine import op_hiftconv
    p, r64, r32 = refs("hiftpair", C, k, dil)
    geo = p["geo"]
    sel, mask = live(geo), geo["mask"].to(dev)
    fused = run_pair(dev, p, nan=False)["out"]
    w = to_dev(p, dev, PAIR_W)
    A = (p["A"] * geo["mask"][:, None]).to(dev)
    tmp = op_hiftconv(A, w["W1"], w["b1"], w["alpha1"], k, dil, rowmask=mask)
    unfused = op_hiftconv(tmp, w["W2"], w["b2"], w["alpha2"], k, 1, rowmask=mask, res1=A, res2=p["res2"].to(dev),
                          out_scale=p["out_scale"], prev=p["prev"].to(dev))
    tag = f"hiftpair_vs_hiftconv/C{C}/k{k}/d{dil}"
    hold(tag + "/fused", fused, r64["out"], r32["out"], sel)
    hold(tag + "/unfused", unfused, r64["out"], r32["out"], sel)
    record(tag + "/distance", fused_unfused=row_err(fused.cpu()[sel], unfused.double().cpu()[sel], r64["out"].abs().amax(dim=1)[sel]))


def test_hiftpair_utterances_independent(dev):
    p, _, _ = refs("hiftpair", 64, 7, 3)
    geo = p["geo"]
    others = live(geo) & (geo["slot"] != 1)
    for table in (False, True):
        base, big = run_pair(dev, p, table=table), run_pair(dev, p, table=table, scale_utt=1)
        same_bits(base, big, others, ("out",))
        assert torch.equal(base["amax_out"][[0, 2]], big["amax_out"][[0, 2]])


def test_hiftpair_race_screen(dev):
    p, _, _ = refs("hiftpair", 128, 11, 5)
    first = run_pair(dev, p)
    noise = stream_noise(dev)
    for i in range(10):
        noise.normal_()
        same_bits(first, run_pair(dev, p), live(p["geo"]), ("out",))


# ---------------------------------------------------------------------------------------------------------------------------------
# hiftconv: the utterance slots (one slot: tests/test_gpu_ops.py::test_hiftconv)
def run_conv(dev, p, table=False, scale_utt=None):
    """one call of jv_op_hiftconv with both residuals, out_scale = 1/3 and accumulation onto prev; masked rows of A hold NaN"""
    from jyutvoice_amd.engine import op_hiftconv
    geo = p["geo"]
    A, amax = p["A"].clone(), p["amax_in"].clone()
    if scale_utt is not None:
        A[utt_rows(geo, scale_utt)] *= 1000.0
        amax[scale_utt] *= 1000.0
    w = to_dev(p, dev, ("W1", "b1", "alpha1", "res1", "res2", "prev"))
    amax_out = torch.zeros(3, device=dev)
    out = op_hiftconv(dirty(A, geo["mask"]).to(dev), w["W1"], w["b1"], w["alpha1"], p["k"], p["dil"], rowmask=geo["mask"].to(dev),
                      res1=w["res1"], res2=w["res2"], out_scale=p["out_scale"], prev=w["prev"], amax_out=amax_out, amax_in=amax.to(dev),
                      slots=geo["slot"].to(dev) if table else (geo["lead"], geo["S"], 3))
    return {"out": out, "amax_out": amax_out}


@pytest.mark.parametrize("C,k,dil", [(256, 3, 1), (256, 11, 5), (128, 7, 3), (64, 11, 1)])
def test_hiftconv_utterance_slots(dev, C, k, dil):
    """hiftconv_kernel with per-utterance slots against fp64: three to five workgroups (hift_rows(k) rows, 80 or 160 each), three
    utterances of scale 1e-3 / 1 / 30 with their own measured bounds through both slot addressings, 16-row tiles that hold rows of
    two utterances (the per-lane branch of the tracked maximum), both residuals, out_scale = 1/3, accumulation, masked rows
    holding NaN, the tracked maximum exact per utterance, utterances independent of one another"""
    p, r64, r32 = refs("hiftconv", C, k, dil)
    geo = p["geo"]
    sel, slot = live(geo), geo["slot"]
    # workgroups and their row tiles start at multiples of 16: a tile straddles when an utterance's first row is no multiple of 16
    assert all(s % 16 for s in geo["start"][1:])
    assert sum(1 for t in range(0, geo["M"] - 15, 16) if slot[t] != slot[t + 15]) >= 2
    got = run_conv(dev, p)
    hold(f"hiftconv_slots/C{C}/k{k}/d{dil}", got["out"], r64["out"], r32["out"], sel)
    assert torch.equal(got["amax_out"].cpu(), tracked(got["out"], geo))
    same_bits(got, run_conv(dev, p, table=True), sel, ("out", "amax_out"))
    big = run_conv(dev, p, scale_utt=1)
    same_bits(got, big, sel & (slot != 1), ("out",))
    assert torch.equal(got["amax_out"][[0, 2]], big["amax_out"][[0, 2]])
