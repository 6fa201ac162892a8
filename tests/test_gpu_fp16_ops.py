"""GPU: the one-product form (NP = 1, `jv_op_set_products(1)`) of every fp16x3 kernel family, through the operator hooks.

Each hook's result must match an fp64 evaluation of the same chain in which every operand of a covered contraction is first rounded as
the hi plane of the fp16x3 split holds it -- fp16 under the kernel's power-of-two scale (tests/fp16_ref.py round_h: 11 significant
bits, round to nearest even, fp16's subnormal grid below 2^-14 of the scaled range) -- weights under their per-row scales, P of the
attention kernels as the kernel keeps it (p 2^10 relative to the running maximum of its 32-key tiles, attn_lazy_max), Q with its
prescale.  The bound is test_gpu_fused_ops.py's, unchanged: the kernel's worst row within 8 x the floor, the floor being the distance
of the fp32 torch evaluation of the same rounded chain from its fp64 evaluation.

That the mode took effect: the three-product result on the same inputs must lie OUTSIDE that bound of the rounded reference.  This
holds by a wide factor for an output that follows ONE covered contraction of the case's own fp32 inputs (rows with LayerNorm-like
statistics: the dropped bits are 2^-12 of every product against 2^-24).  Behind a second contraction the floor is no longer the
accumulation order alone: an intermediate that the fp32 chain computes 1e-7 away from the fp64 chain falls on the other side of a
rounding step now and then (about one element in 2^13), and one such element moves an output by 2^-11 of one product -- the fp32
chain, the fp64 chain and the kernel each have their own.  Measured on the CPU (`separation` below, recorded with every case): 1400
for the fused block's h, 23 for its out, 3 - 4 for the q | k | v behind three contractions.  So every output is held to the parity
bound, and the three-product check in that form is asserted where the CPU separation of the case is at least 4 x the bound
(SEPARATES), which every case's first output is (asserted).

In EVERY case, whatever its separation, two relations tell one product from three (`check`):
  * the three-product result is at least TWICE as far from the rounded chain as the one-product result.  One product differs from the
    rounded chain by accumulation order and by the rare element that rounds the other way; three products differ by the rounding of
    every operand element.  A kernel that dropped the lo terms of only one of a chain's contractions (QK^T but not PV, say) keeps the
    other's share of that rounding and misses the factor;
  * the one-product result lies outside 8 x the distance of the three-product result from the UNROUNDED fp64 chain: the mode is not
    the fp32-accurate arithmetic.

Inputs, geometries and helpers are test_gpu_fused_ops.py's (imported).  Distances go to parity_fp16_ops.json in the output directory
(merged into profiles/parity_fp16.json)."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

import fp16_ref as fr
import parity_util as pu
import test_gpu_fused_ops as fo
from test_gpu_fused_ops import dev      # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

RATIO = fo.RATIO
SEPARATES = 4.0 * RATIO
TWICE = 2.0
record = pu.Recorder("parity_fp16_ops.json", {
    "what": "worst row of |kernel - fp64 of the fp16-rounded chain| / max |row|: one product (kernel), three products on the same inputs "
            "(three), the fp32 torch evaluation of the rounded chain (floor); separation = the unrounded fp64 chain's distance / floor",
    "bound": "kernel <= 8 x floor; three > 8 x floor where separation >= 32"})


@contextlib.contextmanager
def products(n):
    from jyutvoice_amd.engine import op_set_products
    op_set_products(n)
    try:
        yield
    finally:
        op_set_products(3)


def both(fn):
    """fn() with one product, then with three (the default, restored whatever happens)"""
    with products(1):
        one = fn()
    return one, fn()


def Rb(x, bound):
    return fr.round_h(x, fo._h3_scale(bound))


def Rw(W):
    return fr.round_h(W, fr.weight_scale(W).to(W.dtype))


def check(key, one, three, r64, r32, plain64, sel, first=False):
    """one product within the bound of the rounded chain r64 / r32; three products outside it where the inputs separate the two"""
    kd, fl = fo.distances(one, r64, r32, sel)
    k3, _ = fo.distances(three, r64, r32, sel)
    sep, _ = fo.distances(plain64, r64, r32, sel)
    record(key, kernel=kd, three=k3, floor=fl, ratio=kd / fl, separation=sep / fl)
    assert fl > 0.0 and math.isfinite(kd), (key, kd, fl)
    assert kd <= RATIO * fl, (key, kd, fl, kd / fl)
    if first:
        assert sep >= SEPARATES * fl, (key, sep / fl)
    if sep >= SEPARATES * fl:
        assert k3 > RATIO * fl, (key, k3, fl)
    assert k3 > TWICE * kd, (key, k3, kd)
    u1, _ = fo.distances(one, plain64, r32, sel)
    u3, _ = fo.distances(three, plain64, r32, sel)
    assert u1 > RATIO * u3, (key, u1, u3)


# ---------------------------------------------------------------------------------------------------------------------------------
# one contraction: the tile route (conv_gemm_h3: jv_op_linear_h3, jv_op_conv_h3_measured) and rowgemm's epilogues
def ln_rows(M, seed, K=256):
    p = fo.rowblock_inputs(199)
    g = fo._gen(seed)
    return p, torch.randn(M, K, generator=g) * p["ln1_g"][:K] + p["ln1_b"][:K]      # LayerNorm-like rows, inside the proven bound


@pytest.mark.parametrize("presplit", [0, 1])
@pytest.mark.parametrize("tile", ["0", "2"])
def test_linear_h3(dev, monkeypatch, tile, presplit):
    """conv_gemm_h3 on two tile shapes, A split in the kernel and fetched as planes (LDS-DMA): 333 rows, ragged last tiles"""
    from jyutvoice_amd.engine import op_linear_h3
    monkeypatch.setenv("JV_TILE", tile)
    p, A = ln_rows(333, 70)
    W, b, bound = p["W1"], p["b1"], p["bounds"]["ln1"]
    one, three = both(lambda: op_linear_h3(A.to(dev), W.to(dev), b.to(dev), a_bound=bound, presplit=presplit))
    ref = lambda dt, r=True: (Rb(A.to(dt), bound) if r else A.to(dt)) @ (Rw(W.to(dt)) if r else W.to(dt)).T + b.to(dt)
    check(f"linear_h3/tile{tile}/presplit{presplit}", one, three, ref(torch.float64), ref(torch.float32), ref(torch.float64, False),
          slice(0, 333), first=True)


def test_conv_h3_measured(dev):
    """the tile route with a measured bound and three taps (the estimator's trunk convolutions at short M)"""
    from jyutvoice_amd.engine import op_conv_h3_measured
    p = fo.rowres_inputs("uniform", 46, 256)
    x = p["x"] * p["mask"][:, None]
    amax = x.abs().max().reshape(1)
    M = x.shape[0]
    one, three = both(lambda: op_conv_h3_measured(x.to(dev), p["W1"].to(dev), p["b1"].to(dev), ntaps=3, tap_row0=-2, amax_in=amax.to(dev)))
    ref = lambda dt, r=True: fo.conv_rows(Rb(x.to(dt), float(amax)) if r else x.to(dt), Rw(p["W1"].to(dt)) if r else p["W1"].to(dt), 3, -2, 1) + p["b1"].to(dt)
    check("conv_h3_measured", one, three, ref(torch.float64), ref(torch.float32), ref(torch.float64, False), fo.live(p["geo"]), first=True)


@pytest.mark.parametrize("rt", [2, 3, 4, 5])
def test_rowgemm(dev, monkeypatch, rt):
    """rowgemm_wd / rowgemm_wa (and, K = 96, the LDS form rowgemm_kernel) at every tile height: plain, GELU -> planes, q | k | v"""
    from jyutvoice_amd.engine import op_rowgemm, op_rowgemm_qkv
    monkeypatch.setenv("JV_ROWGEMM_RT", str(rt))
    M = 199
    p, A = ln_rows(M, 80 + rt)
    bound, rows = p["bounds"]["ln1"], slice(0, M)
    W, b = p["W1"], p["b1"]
    lin = lambda dt, r, A_, W_: (Rb(A_.to(dt), bound) if r else A_.to(dt)) @ (Rw(W_.to(dt)) if r else W_.to(dt)).T
    for epi, post in (("plain", lambda z: z), ("gelu", F.gelu)):
        one, three = both(lambda: op_rowgemm(A.to(dev), W.to(dev), b.to(dev), epi=epi, a_bound=bound, out2_scale=64.0))
        ref = lambda dt, r=True: post(lin(dt, r, A, W) + b.to(dt))
        check(f"rowgemm/rt{rt}/{epi}", one, three, ref(torch.float64), ref(torch.float32), ref(torch.float64, False), rows, first=True)
    A96, W96 = A[:, :96].contiguous(), W[:256, :96].contiguous()      # K % 64 != 0: weights through LDS (rowgemm_kernel)
    one, three = both(lambda: op_rowgemm(A96.to(dev), W96.to(dev), None, epi="plain", a_bound=bound))
    ref = lambda dt, r=True: lin(dt, r, A96, W96)
    check(f"rowgemm/rt{rt}/lds", one, three, ref(torch.float64), ref(torch.float32), ref(torch.float64, False), rows, first=True)
    Ap = torch.cat([A, torch.zeros(9, 256)])
    for nsplit in (1, 3):
        one, three = both(lambda: op_rowgemm_qkv(Ap.to(dev), p["Wq"].to(dev), bound, p["k_bound"], p["v_bound"], M=M, nsplit=nsplit, rt=rt))
        ref = lambda dt, r=True: lin(dt, r, A, p["Wq"])
        r64, r32, u64 = ref(torch.float64), ref(torch.float32), ref(torch.float64, False)
        for i, n in enumerate("qkv"):
            cols = slice(512 * i, 512 * (i + 1))
            check(f"rowgemm_qkv/rt{rt}/split{nsplit}/{n}", one[i][:M], three[i][:M], r64[:, cols], r32[:, cols], u64[:, cols], rows, first=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused block and the feed-forward pair (rowblock_kernel, rowffn_kernel): modes 0 - 3, fused
def ref_rowblock_h(p, dtype=torch.float64, rounded=True):
    """fo.ref_rowblock with the operands of its four contractions as the planes hold them"""
    c, b = fo.cast(p, dtype), p["bounds"]
    R = Rb if rounded else (lambda x, bound: x)
    W = Rw if rounded else (lambda w: w)
    h = c["h"] + R(c["att"], b["att"]) @ W(c["Wo"]).T + c["bo"]
    x = fo.layer_norm(h, c["ln3_g"], c["ln3_b"])
    hid = F.gelu(R(x, b["ln3"]) @ W(c["W1"]).T + c["b1"])
    out = h + R(hid, b["hid"]) @ W(c["W2"]).T + c["b2"]
    ln = fo.layer_norm(out, c["ln1_g"], c["ln1_b"])
    qkv = R(ln, b["ln1"]) @ W(c["Wq"]).T
    return {"h": h, "out": out, "ln": ln, "q": qkv[:, :512], "k": qkv[:, 512:1024], "v": qkv[:, 1024:]}


def ref_rowffn_h(p, dtype=torch.float64, rounded=True):
    c, b = fo.cast(p, dtype), p["bounds"]
    R = Rb if rounded else (lambda x, bound: x)
    W = Rw if rounded else (lambda w: w)
    hid = F.gelu(R(c["x"], b["ln3"]) @ W(c["W1"]).T + c["b1"])
    out = c["h"] + R(hid, b["hid"]) @ W(c["W2"]).T + c["b2"]
    return {"out": out, "ln": fo.layer_norm(out, c["ln1_g"], c["ln1_b"])}


@pytest.mark.parametrize("rt,layout", [(2, "uniform"), (3, "compact"), (4, "exact"), (5, "uniform")])
def test_rowblock_and_rowffn(dev, monkeypatch, rt, layout):
    monkeypatch.setenv("JV_ROWGEMM_RT", str(rt))
    monkeypatch.delenv("JV_FF_STAGGER", raising=False)
    geo, rows = fo.block_case(layout, rt)
    M, sel = geo["M"], fo.live(geo)
    p = fo.rowblock_inputs(M)
    r64, r32, u64 = ref_rowblock_h(p), ref_rowblock_h(p, torch.float32), ref_rowblock_h(p, rounded=False)
    tag = f"rowblock/rt{rt}/{layout}"
    # (h after phase A is visible only where out is a separate buffer: the stage's last block, stride 512)
    for mode, ld, outs in (("plain", 512, ("h", "out")), ("ln", None, ("out", "ln")), ("qkv", None, ("out", "q", "k", "v"))):
        one, three = both(lambda: fo.run_block(dev, p, geo, rows, mode, out_ld=ld))
        for n in outs:
            check(f"{tag}/{mode}/{n}", one[n][:M, :256 if n == "out" else None], three[n][:M, :256 if n == "out" else None], r64[n], r32[n],
                  u64[n], sel, first=n == "h")
    pf = fo.rowffn_inputs(M)
    f64, f32, fu = ref_rowffn_h(pf), ref_rowffn_h(pf, torch.float32), ref_rowffn_h(pf, rounded=False)
    one, three = both(lambda: fo.run_block(dev, pf, geo, rows, "ffn", key="x"))
    for n in ("out", "ln"):
        check(f"rowffn/rt{rt}/{layout}/{n}", one[n][:M], three[n][:M], f64[n], f32[n], fu[n], sel)
    assert not torch.equal(one["out"][:M].cpu()[sel], three["out"][:M].cpu()[sel])
    # the separate launchers on one product (rowgemm<res,ln>, rowffn, rowgemm<qkv>; rowgemm<gelu> + rowgemm<res[,ln]>: what the
    # estimator runs with JV_NO_BLOCK_FUSE / JV_NO_FFN_FUSE or without fragment-order weights) give the fused launch's bits
    with products(1):
        fused = fo.run_block(dev, p, geo, rows, "qkv")
        for unfused in (0, -1):
            fo.same_bits(fused, fo.run_block(dev, p, geo, rows, "qkv", fused=unfused), sel, fo.OUTS + ("amax_h", "amax_out"))
        plain = fo.run_block(dev, p, geo, rows, "plain", out_ld=512)
        fo.same_bits(plain, fo.run_block(dev, p, geo, rows, "plain", fused=-1, out_ld=512), sel, fo.OUTS + ("amax_h", "amax_out"))
        ffn = fo.run_block(dev, pf, geo, rows, "ffn", key="x")
        fo.same_bits(ffn, fo.run_block(dev, pf, geo, rows, "ffn", key="x", fused=-1), sel, fo.OUTS + ("amax_out",))


# ---------------------------------------------------------------------------------------------------------------------------------
# the row-owning convolution and the whole resnet (rowconv_kernel / rowconv_wd_kernel, rowres_kernel: all three products)
def row_scale(p):
    """the power of two each row of x is staged with: its utterance's measured bound (h3_scale_dev)"""
    return torch.tensor([fo._h3_scale(float(a)) for a in p["amax_in"]], dtype=torch.float64)[p["geo"]["slot"].long()][:, None]


def ref_rowres_h(p, dtype=torch.float64, rounded=True):
    """fo.ref_rowres with x under its utterance's scale, h2 under the scale of max(sqrt(255) max|ln1_g| + max|ln1_b|, 0.31) + max|temb|
    (rowres_kernel.h), the LayerNorm1 planes under lnf_bound's"""
    c = fo.cast(p, dtype)
    m = p["mask"].to(dtype)[:, None]
    W = Rw if rounded else (lambda w: w)
    xm = torch.where(m != 0, c["x"], torch.zeros((), dtype=dtype))
    xr = fr.round_h(xm, row_scale(p)) if rounded else xm
    h2b = max(math.sqrt(255.0) * float(p["ln1_g"].abs().max()) + float(p["ln1_b"].abs().max()), 0.31) + float(p["temb"].abs().max())
    c1 = fo.conv_rows(xr, W(c["W1"]), 3, -2, 1) + c["b1"]
    h2m = (F.mish(fo.layer_norm(c1, c["ln1_g"], c["ln1_b"])) * m + c["temb"]) * m
    c2 = fo.conv_rows(Rb(h2m, h2b) if rounded else h2m, W(c["W2"]), 3, -2, 1) + c["b2"]
    out = F.mish(fo.layer_norm(c2, c["ln2_g"], c["ln2_b"])) * m + (xr @ W(c["Wr"]).T + c["br"])
    ln = fo.layer_norm(out, c["lnf_g"], c["lnf_b"])
    qkv = (Rb(ln, p["lnf_bound"]) if rounded else ln) @ W(c["Wq"]).T
    return {"out": out, "ln": ln, "q": qkv[:, :512], "k": qkv[:, 512:1024], "v": qkv[:, 1024:]}


@pytest.mark.parametrize("rt,layout,cin", [(2, "uniform", 256), (3, "compact", 512), (4, "exact", 256), (5, "uniform", 512)])
def test_rowres(dev, monkeypatch, rt, layout, cin):
    monkeypatch.setenv("JV_ROWGEMM_RT", str(rt))
    p = fo.rowres_inputs(layout, 16 * rt - 2, cin)
    geo = p["geo"]
    M, sel, every = geo["M"], fo.live(geo), slice(0, geo["M"])
    r64, r32, u64 = ref_rowres_h(p), ref_rowres_h(p, torch.float32), ref_rowres_h(p, rounded=False)
    tag = f"rowres/rt{rt}/{layout}/c{cin}"
    one, three = both(lambda: fo.run_res(dev, p, "ln"))
    check(tag + "/out", one["out"][:M], three["out"][:M], r64["out"], r32["out"], u64["out"], every)
    check(tag + "/lnf", one["lnf"][:M], three["lnf"][:M], r64["ln"], r32["ln"], u64["ln"], sel)
    assert not torch.equal(one["out"][:M].cpu()[sel], three["out"][:M].cpu()[sel])
    one, three = both(lambda: fo.run_res(dev, p, "qkv"))
    for n in "qkv":
        check(f"{tag}/{n}", one[n][:M], three[n][:M], r64[n], r32[n], u64[n], sel)
    plain, _ = both(lambda: fo.run_res(dev, p, "plain"))
    assert torch.equal(plain["out"][:M], one["out"][:M])


@pytest.mark.parametrize("cin", [256, 96])
def test_rowconv(dev, monkeypatch, cin):
    """rowconv_wd_kernel (cin = 256: weights straight into registers) and rowconv_kernel (cin = 96: an odd number of 32-channel
    chunks, weights through LDS): block1's launch -- LayerNorm, Mish, mask, time embedding -- on one measured slot"""
    from jyutvoice_amd.engine import op_rowconv
    monkeypatch.setenv("JV_ROWGEMM_RT", "3")
    p = fo.rowres_inputs("uniform", 46, 256)
    geo = p["geo"]
    x = (p["x"] * p["mask"][:, None])[:, :cin].contiguous()
    W1 = p["W1"].view(256, 3, 256)[:, :, :cin].reshape(256, 3 * cin).contiguous()
    amax = x.abs().max().reshape(1)
    w = fo.to_dev(p, dev, fo.RES_W)
    one, three = both(lambda: op_rowconv(x.to(dev), W1.to(dev), w["b1"], ln=(w["ln1_g"], w["ln1_b"]), act="mish", rowmask=geo["mask"].to(dev),
                                        rowvec=w["temb"], amax_in=amax.to(dev)))

    def ref(dt, r=True):
        c = fo.cast(p, dt)
        m = p["mask"].to(dt)[:, None]
        c1 = fo.conv_rows(Rb(x.to(dt), float(amax)) if r else x.to(dt), Rw(W1.to(dt)) if r else W1.to(dt), 3, -2, 1) + c["b1"]
        return F.mish(fo.layer_norm(c1, c["ln1_g"], c["ln1_b"])) * m + c["temb"]

    check(f"rowconv/c{cin}", one, three, ref(torch.float64), ref(torch.float32), ref(torch.float64, False), fo.live(geo), first=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# attention: attention64_planes (chunk 0 and 50) and the tile route's attention64 (jv_op_attention_h3)
def ref_attention_h(qkv, B, G, S, L, lens, bounds, chunk, lazy, dtype=torch.float64, rounded=True):
    """softmax(q k^T / 8) v per head as the kernels run it: Q * log2(e) / 8 * q_scale, K * k_scale, V * v_scale rounded to fp16; 32-key
    tiles with a running maximum that moves when a tile's maximum exceeds it by more than `lazy` (attn_lazy_max: 4 in attention_pl.hip,
    0 in attention.hip); P = 2^(score - maximum + 10) rounded to fp16 for the PV product, unrounded in the normaliser"""
    qs, ks, vs = fo._h3_scale(bounds[0] * 0.1803369), fo._h3_scale(bounds[1]), fo._h3_scale(bounds[2])
    R = (lambda x: fr.round_h(x, 1.0)) if rounded else (lambda x: x)
    c = float(torch.tensor(0.125, dtype=torch.float32) * torch.tensor(1.44269504088896340736, dtype=torch.float32) * qs)
    out = torch.zeros(qkv.shape[0], 512, dtype=dtype)
    for b in range(B):
        blk = qkv[G + b * S: G + b * S + L].to(dtype)
        q, k, v = (blk[:, i * 512:(i + 1) * 512].view(L, 8, 64).transpose(0, 1) for i in range(3))
        s = (R(q * c) @ R(k * ks).transpose(1, 2)) / (qs * ks)      # base-2 units
        i = torch.arange(L)
        kend = torch.full((L,), lens[b]) if not chunk else torch.minimum(torch.tensor(lens[b]), (i // chunk + 1) * chunk)
        s = s.masked_fill(~(i[None, :] < kend[:, None])[None], float("-inf"))
        vh = R(v * vs)
        m_run = torch.full((8, L), float("-inf"), dtype=dtype)
        l_run = torch.zeros(8, L, dtype=dtype)
        o = torch.zeros(8, L, 64, dtype=dtype)
        for k0 in range(0, int(kend.max()), 32):
            st = s[:, :, k0:k0 + 32]
            mt = st.amax(dim=-1)
            m_new = torch.where(mt > m_run + lazy, mt, m_run)
            alpha = torch.where(m_new == m_run, torch.ones_like(m_new), torch.exp2(m_run - m_new))
            pt = torch.exp2(st - m_new[..., None] + 10.0)
            pt = torch.where(torch.isfinite(st), pt, torch.zeros_like(pt))
            l_run = l_run * alpha + pt.sum(dim=-1)
            o = o * alpha[..., None] + R(pt) @ vh[:, k0:k0 + 32]
            m_run = m_new
        out[G + b * S: G + b * S + L] = (o / l_run[..., None] / vs).transpose(0, 1).reshape(L, 512)
    return out


@pytest.mark.parametrize("B,L,lens", [(2, 300, [300, 217]), (3, 70, [70, 1, 33]), (2, 129, [129, 64])])
def test_attention(dev, B, L, lens):
    """the shapes of test_gpu_ops.py::test_attention_planes that take 8, 2 and 4 waves; ragged key masks; chunk mask 50"""
    from jyutvoice_amd.engine import op_attention_h3, op_attention_planes
    g = torch.Generator().manual_seed(B * 1000 + L + 9)
    G, gap = 4, 4
    S = L + gap
    qkv = torch.randn(G + B * S + 8, 1536, generator=g)
    qkv[:, 512:1024] *= 3.0
    lens_t = torch.tensor(lens, dtype=torch.int32)
    bounds = tuple(4.0 * float(qkv[:, o:o + 512].abs().max()) for o in (0, 512, 1024))
    sel = torch.zeros(qkv.shape[0], dtype=torch.bool)
    for b in range(B):
        sel[G + b * S: G + b * S + L] = True
    runs = [(f"attention_planes/chunk{chunk}", 4.0, chunk,
             lambda chunk=chunk: op_attention_planes(qkv.to(dev), lens_t.to(dev), B, G, S, L, bounds, chunk=chunk)) for chunk in (0, 50)]
    runs.append(("attention_h3", 0.0, 0, lambda: op_attention_h3(qkv.to(dev), lens_t.to(dev), B, G, S, L, bounds)))
    for name, lazy, chunk, fn in runs:
        one, three = both(fn)
        r64 = ref_attention_h(qkv, B, G, S, L, lens, bounds, chunk, lazy)
        r32 = ref_attention_h(qkv, B, G, S, L, lens, bounds, chunk, lazy, torch.float32)
        u64 = ref_attention_h(qkv, B, G, S, L, lens, bounds, chunk, lazy, rounded=False)
        check(f"{name}/B{B}L{L}", one, three, r64, r32, u64, sel)
        assert not torch.equal(one.cpu()[sel], three.cpu()[sel])
