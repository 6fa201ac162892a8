"""GPU: the estimator's split-K route -- conv_gemm_x6_kernel with ksplit > 1 into partial sums, then splitk_reduce_kernel: the sum in
fixed order, bias, LayerNorm -> Mish -> mask, the time embedding through row_sample, the residual (read from the buffer it then
overwrites), the per-utterance tracked maximum and the LayerNorm of the stored row for the next GEMM -- through jv_op_splitk, which
calls the launcher the estimator calls (conv_splitk, rowops.hip), held to a plain fp64 PyTorch evaluation of the same formulas.

Every evaluation of 2048 rows or fewer takes this route (est_route); test_route_pin checks that with the in-library profiler, so that
the hook does not test a path production left.

The bound is test_gpu_fused_ops.py's, unchanged and argued there: the worst row of |kernel - fp64| over that row's own magnitude may be
RATIO = 8 times the same figure of the fp32 torch evaluation on the CPU, and that floor must be > 0.  `out` is compared on EVERY row
below M (a masked row stores exactly rowvec + res), the second LayerNorm on the live rows.  Kernel distance, floor and ratio of every
case go to parity_splitk_ops.json (parity_util.Recorder).  tests/test_splitk_refs_host.py applies plausible mistakes to ref_splitk,
without a GPU, and checks that each lands outside that bound on these inputs.

The references and inputs live in this file (ref_splitk, case) and use no library code; geometry, dirty, distances, hold and RATIO are
test_gpu_fused_ops.py's."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import fp16_ref as fr
import parity_util as pu
import test_gpu_fp16_ops as f16      # check / both / products (a module object: none of its tests is collected here)
import test_gpu_fused_ops as fo
from test_gpu_fused_ops import dev      # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

RATIO = fo.RATIO
GUARD = 8                               # rows behind M in every buffer: NaN, masked, never touched
KSPLIT = 8                              # flow_ws.h PARTIAL_SPLITS
UTT = (1.0, 30.0, 1e-3)                 # the utterances' own magnitudes: a wrong amax slot overflows fp16 or loses the small one
record = pu.Recorder("parity_splitk_ops.json", {
    "what": "worst row of |kernel - fp64| / max |fp64 row| (kernel), of the same chain in fp32 torch on the CPU (floor), and their ratio",
    "bound": "kernel <= 8 x floor", "lens": list(fo.LENS)})


def hold(key, got, ref64, ref32, sel):
    """fo.hold, recorded in this file's JSON"""
    kd, fl = fo.distances(got, ref64, ref32, sel)
    record(key, kernel=kd, floor=fl, ratio=kd / fl)
    assert fl > 0.0 and math.isfinite(kd), (key, kd, fl)
    assert kd <= RATIO * fl, (key, kd, fl, kd / fl)
    return kd


# ---------------------------------------------------------------------------------------------------------------------------------
# row geometries (flow geometry: 4 lead rows, 4 gap rows behind each utterance)
GEOS = {
    "utt3": lambda: fo.geometry(),                                              # 199 rows: the last 64-row tile has 7
    "pad256": lambda: fo.geometry(total=256),                                   # the same, masked rows up to a multiple of every tile height
    "one": lambda: fo.geometry(lens=(1,), T=1),                                 # one utterance of one frame: 9 rows
    "edge2048": lambda: fo.geometry(lens=(676, 600, 650), T=676, total=2048),   # M = PARTIAL_ROWS: the largest split_stride
    "utt0": lambda: fo.geometry(lens=fo.LENS[:1], T=fo.L),                      # utterance 0 of utt3 alone (its first 69 rows)
}
FLOW_GEOS = ("utt3", "pad256", "one")


@functools.lru_cache(maxsize=None)
def geo_of(name):
    return GEOS[name]()


def share_chunks(cin, ksplit=KSPLIT):
    """conv_gemm_x6_kernel.h: workgroup z of min(ksplit, cin / 32) contracts the 32-channel chunks [z nch / ksplit, (z + 1) nch / ksplit)"""
    nch = cin // 32
    ks = min(ksplit, nch)
    return [(z * nch // ks, (z + 1) * nch // ks) for z in range(ks)]


# ---------------------------------------------------------------------------------------------------------------------------------
# reference: plain torch in `dtype` (fp64: the reference; fp32: the floor); `mut`: one deliberate mistake (test_splitk_refs_host.py);
# rounded: the operands of the contraction as the hi planes of the fp16x3 split hold them (the one-product form, test_np1)
def row_scale(p, shift=0):
    """mode 1: the power of two each row of A is staged with -- its utterance's measured bound (h3_scale_dev); shift: utterance b
    takes utterance b - shift's bound instead (the amax_wrong_slot mutant)"""
    nb = len(p["amax_in"])
    sc = torch.tensor([fo._h3_scale(float(p["amax_in"][(b - shift) % nb])) for b in range(nb)], dtype=torch.float64)
    return sc[p["geo"]["slot"].long()][:, None]


def two_planes(x, scale):
    """x as the fp16x3 split holds it under `scale`: h = fp16(x s), l = fp16(x s - h), both on fp16's grid (overflow: inf)"""
    h = fr.round_h(x, scale)
    return h + fr.round_h(x - h, scale)


def ref_splitk(p, dtype=torch.float64, mut=None, rounded=False):
    """out = act(LayerNorm(conv(A mask) + bias)) mask + rowvec[slot] + res; out2 = LayerNorm2(out) -- each stage where the case has it;
    tap j reads row m + row0 + j; rows with mask == 0 read as zero and store rowvec + res"""
    c = fo.cast(p, dtype)
    M, cin, ntaps = p["A"].shape[0], p["A"].shape[1], p["ntaps"]
    zero = torch.zeros((), dtype=dtype)
    m = (torch.ones(M) if p["mask"] is None else p["mask"]).to(dtype)[:, None]
    x, W = torch.where(m != 0, c["A"], zero), c["W"]
    if mut in ("drop_chunk", "double_chunk"):      # the second chunk of the first two-chunk share: left out / contracted twice
        lo = next(lo for lo, hi in share_chunks(cin) if hi - lo == 2) + 1
        W = W.clone()
        for j in range(ntaps):
            W[:, j * cin + 32 * lo: j * cin + 32 * lo + 32] *= 0.0 if mut == "drop_chunk" else 2.0
    if mut == "amax_wrong_slot":
        x = two_planes(x, row_scale(p, shift=1))
    if rounded:
        x = fr.round_h(x, row_scale(p) if p["mode"] == 1 else fo._h3_scale(p["a_bound"]))
        W = f16.Rw(W)
    v = fo.conv_rows(x, W, ntaps, -1 if mut == "tap_shift" else p["row0"], 1) + (0 if mut == "drop_bias" else c["bias"])
    act = {"none": lambda z: z, "mish": F.silu if mut == "mish_silu" else F.mish}[p["act"]]
    ln = (lambda z: fo.layer_norm(z, c["ln_g"], c["ln_b"], 1e-6 if mut == "ln_eps" else 1e-5)) if p["ln_g"] is not None else (lambda z: z)
    temb = c["rowvec"][p["geo"]["slot"].long() if p["rowvec_ld"] else torch.zeros(M, dtype=torch.long)] if p["rowvec"] is not None else None
    if mut == "mask_before_ln":        # the mask moved ahead of LayerNorm -> Mish: a masked row then stores Mish(ln_b) + rowvec + res
        v = act(ln(v * m))
    elif mut == "temb_before_mish" and temb is not None:      # the time embedding added ahead of Mish and the mask
        v = torch.where(m != 0, act(ln(v) + temb), zero)
        temb = None
    else:
        v = torch.where(m != 0, act(ln(v)), zero)
    if temb is not None:
        v = v + temb
    pre_res = v
    if p["res"] is not None and mut != "res_dropped":
        v = v + c["res"]
    r = {"out": v}
    if p["ln2_g"] is not None:
        r["out2"] = fo.layer_norm(pre_res if mut == "ln2_before_res" else v, c["ln2_g"], c["ln2_b"], 1e-6 if mut == "ln2_eps" else 1e-5)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs that discriminate (test_splitk_refs_host.py): LayerNorm gains over [0.5, 2.5] with offsets, every bias non-zero, residual rows
# over several decades, utterances of magnitude 1 / 30 / 1e-3 with their own measured bounds.  The convolutions' bias is of order 0.02,
# so that the rows of the 1e-3 utterance reach LayerNorm with a variance near 4e-4: that is where an eps of 1e-6 instead of 1e-5 shows;
# to_out's and ff.net.2's inputs are rowblock_inputs' (some stored rows have a variance near 1e-3: the second LayerNorm's eps)
def _blank(geo, A, W, bias, ntaps=1, row0=0, mode=2):
    return {"geo": geo, "mask": geo["mask"], "A": A, "W": W, "bias": bias, "ntaps": ntaps, "row0": row0, "mode": mode, "act": "none",
            "ln_g": None, "ln_b": None, "rowvec": None, "rowvec_ld": 0, "res": None, "ln2_g": None, "ln2_b": None, "in_place": False,
            "amax_in": None, "a_bound": 0.0}


def _utt_rows(g, geo, C):
    nb = len(geo["lens"])
    return torch.randn(geo["M"], C, generator=g) * torch.tensor(UTT[:nb])[geo["slot"].long()][:, None]


def _decades(g, M, C=256):
    return torch.randn(M, C, generator=g) * (10.0 ** (torch.arange(M) % 7 - 3).float())[:, None]


def _measured(p):
    geo = p["geo"]
    p["amax_in"] = torch.stack([p["A"][fo.utt_rows(geo, b)].abs().max() for b in range(len(geo["lens"]))])


@functools.lru_cache(maxsize=None)
def case(kind, geo_name="utt3", opt=None):
    """the inputs of a case (shared, never modified).  kind / opt:
    conv3_first (opt "shared" / "per_utt"): Cin = 320, three taps, bf16x6, uneven shares 1,1,1,2,1,1,1,2; bias -> LayerNorm -> Mish ->
        mask -> + time embedding (one vector for all rows, rowvec_ld = 0, or one per utterance through row_sample)
    conv3_trunk (opt (cin, res)): fp16x3 from the measured bounds; bias -> LayerNorm -> Mish -> mask (-> + res) -> LayerNorm2
    to_out: K = 512, proven bound, res = the output buffer itself, LayerNorm2
    ff2 (opt ldo): K = 1024, proven bound, res = h, out a buffer of its own (256: with LayerNorm2; 512: the concat buffer's right half)
    clamp (opt cin): one tap, Cin = 64 / 96 / 160: ksplit = 2 / 3 / 5 shares of one chunk; no mask, no tail but the bias"""
    geo = geo_of(geo_name)
    M = geo["M"]
    g = fo._gen(900 + sum(map(ord, kind + geo_name + repr(opt))))
    if kind == "conv3_first":
        p = _blank(geo, _utt_rows(g, geo, 320), fo._weight(g, 256, 960), 0.02 * torch.randn(256, generator=g), 3, -2, mode=0)
        p["ln_g"], p["ln_b"] = fo._ln(g)
        p["act"] = "mish"
        nvec = len(geo["lens"]) if opt == "per_utt" else 1
        p["rowvec"], p["rowvec_ld"] = torch.randn(nvec, 256, generator=g), 256 if opt == "per_utt" else 0
    elif kind == "conv3_trunk":
        cin, res = opt
        p = _blank(geo, _utt_rows(g, geo, cin), fo._weight(g, 256, 3 * cin), 0.02 * torch.randn(256, generator=g), 3, -2, mode=1)
        p["ln_g"], p["ln_b"] = fo._ln(g)
        p["act"] = "mish"
        p["res"] = _decades(g, M) if res else None
        p["ln2_g"], p["ln2_b"] = fo._ln(g)
        _measured(p)
    elif kind == "to_out":
        b = fo.rowblock_inputs(M)
        p = _blank(geo, b["att"], b["Wo"], b["bo"])
        p["res"], p["in_place"], p["ln2_g"], p["ln2_b"], p["a_bound"] = b["h"], True, b["ln3_g"], b["ln3_b"], b["bounds"]["att"]
    elif kind == "ff2":
        b = fo.rowblock_inputs(M)
        hid = F.gelu(1.5 * torch.randn(M, 1024, generator=g)) * (10.0 * 10.0 ** (torch.arange(M) % 7 - 3).float()).clamp(max=1.0)[:, None]
        p = _blank(geo, hid, b["W2"], b["b2"])
        p["res"], p["a_bound"], p["ldo"] = b["h"], float(hid.abs().max()), opt
        if opt == 256:
            p["ln2_g"], p["ln2_b"] = b["ln1_g"], b["ln1_b"]
    elif kind == "clamp":
        b = fo.rowblock_inputs(199)
        A = torch.randn(M, opt, generator=g) * b["ln1_g"][:opt] + b["ln1_b"][:opt]
        p = _blank(geo, A, fo._weight(g, 256, opt), 0.5 * torch.randn(256, generator=g))
        p["mask"], p["a_bound"] = None, float(A.abs().max())
    else:
        raise KeyError(kind)
    return p


@functools.lru_cache(maxsize=None)
def refs(kind, geo_name="utt3", opt=None):
    """(inputs, fp64 reference, fp32 floor chain) of a case, computed once and shared"""
    p = case(kind, geo_name, opt)
    return p, ref_splitk(p), ref_splitk(p, torch.float32)


# every case the host test applies its mutants to and the parity tests run: (kind, geometry, opt)
CONV_FIRST = [("conv3_first", g, o) for g in FLOW_GEOS for o in ("shared", "per_utt")]
CONV_TRUNK = [("conv3_trunk", g, (cin, res)) for g in FLOW_GEOS for cin in (256, 512) for res in (False, True)]
TO_OUT = [("to_out", g, None) for g in FLOW_GEOS]
FF2 = [("ff2", g, ldo) for g in FLOW_GEOS for ldo in (256, 512)] + [("ff2", "edge2048", 256)]
CLAMP = [("clamp", "utt3", cin) for cin in (64, 96, 160)]


def case_id(key):
    kind, geo_name, opt = key
    return "-".join(str(x) for x in (kind, geo_name) + (tuple(opt) if isinstance(opt, tuple) else (opt,)) if x is not None)


# ---------------------------------------------------------------------------------------------------------------------------------
# one launch through the hook
def run(dev, p, nan=True, ksplit_max=KSPLIT, A=None, rows_of=None, fill=float("nan")):
    """jv_op_splitk on the case's rows, M + GUARD rows in every buffer.  nan: the masked rows of A and the rows past M hold NaN (so
    do the masked rows of nothing else: res and rowvec reach the stored row).  A: other values for the operand (same shape);
    rows_of: run the first rows of the case under this smaller geometry (test_batch_independence); fill: what the output buffer holds.
    -> out [rows, 256] (the written columns), out2, amax_out, full (the whole output buffer)"""
    from jyutvoice_amd.engine import op_splitk
    geo = p["geo"] if rows_of is None else rows_of
    M, rows, nb = geo["M"], geo["M"] + GUARD, len(geo["lens"])
    cut = lambda t: None if t is None else fo.pad_rows(t[:M], rows)
    mask = None if p["mask"] is None else geo["mask"]
    a = (p["A"] if A is None else A)[:M]
    if nan and mask is not None:
        a = fo.dirty(a, mask)
    d = lambda t: None if t is None else t.to(dev)
    amax_out = torch.zeros(nb, device=dev)
    ldo = p.get("ldo", 256)
    full = torch.full((rows, ldo), fill, device=dev)
    res = cut(p["res"])
    if p["in_place"]:
        full[:] = res.to(dev)
    out = full[:, ldo - 256:]
    ln2 = None if p["ln2_g"] is None else (d(p["ln2_g"]), d(p["ln2_b"]))
    _, out2 = op_splitk(d(fo.pad_rows(a, rows)), d(p["W"]), d(p["bias"]), M=M, ntaps=p["ntaps"], tap_row0=p["row0"],
                        ln=None if p["ln_g"] is None else (d(p["ln_g"]), d(p["ln_b"])), act=p["act"],
                        rowmask=None if mask is None else d(fo.pad_rows(mask, rows, 0)), rowvec=d(p["rowvec"]),
                        row_sample=d(fo.pad_rows(geo["slot"], rows, 0)), rowvec_ld=p["rowvec_ld"],
                        res=out if p["in_place"] else d(res), out=out, ln2=ln2, ksplit_max=ksplit_max, mode=p["mode"],
                        amax_in=None if p["amax_in"] is None else d(p["amax_in"][:nb]), a_bound=p["a_bound"],
                        slots=(geo["lead"], geo["S"], nb), amax_out=amax_out)
    return {"out": out, "out2": out2, "amax_out": amax_out, "full": full}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b, names=("out", "out2", "amax_out")):
    for n in names:
        if a[n] is not None:
            assert torch.equal(bits(a[n]), bits(b[n])), n


def exact_checks(p, got):
    """what must hold bit for bit in every launch: rows at or beyond M untouched, masked rows store exactly rowvec + res (the
    activation branch is zero), and amax_out[slot] is the largest stored magnitude over that slot's unmasked rows"""
    geo = p["geo"]
    M, out = geo["M"], got["out"].cpu()
    assert torch.isnan(got["full"][M:]).all()
    if got["out2"] is not None:
        assert torch.isnan(got["out2"][M:]).all()
    if p["mask"] is None:      # no tracking mask: every row below M counts, in its row_sample slot
        assert torch.equal(got["amax_out"].cpu(), torch.stack([out[:M][geo["slot"] == b].abs().max() for b in range(len(geo["lens"]))]))
        return
    want = torch.zeros(M, 256)
    if p["rowvec"] is not None:
        want = want + p["rowvec"][geo["slot"].long() if p["rowvec_ld"] else torch.zeros(M, dtype=torch.long)]
    if p["res"] is not None:
        want = want + p["res"]
    dead = geo["mask"] == 0
    assert torch.equal(out[:M][dead], want[dead])
    assert torch.equal(got["amax_out"].cpu(), fo.tracked(out[:M], geo))


def parity(dev, key, nan=True):
    p, r64, r32 = refs(*key)
    geo = p["geo"]
    M = geo["M"]
    got = run(dev, p, nan=nan)
    tag = case_id(key)
    hold(tag + "/out", got["out"][:M], r64["out"], r32["out"], slice(0, M))
    if "out2" in r64:
        hold(tag + "/out2", got["out2"][:M], r64["out2"], r32["out2"], fo.live(geo))
    exact_checks(p, got)
    return p, got


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 parity of the cases
@pytest.mark.parametrize("key", CONV_FIRST, ids=case_id)
def test_conv3_first(dev, key):
    """the first resnet's block1: Cin = 320 over eight workgroups with shares 1,1,1,2,1,1,1,2 (bf16x6), bias -> LayerNorm -> Mish ->
    mask -> + time embedding, shared (rowvec_ld = 0) or per utterance (row_sample); amax_out per utterance; masked rows of A hold NaN,
    the two a causal window reads ahead of an utterance's first frame among them"""
    assert [hi - lo for lo, hi in share_chunks(320)] == [1, 1, 1, 2, 1, 1, 1, 2]
    p, got = parity(dev, key)
    same_bits(got, run(dev, p, nan=False))      # what a masked row of A holds does not matter


@pytest.mark.parametrize("key", CONV_TRUNK, ids=case_id)
def test_conv3_trunk(dev, key):
    """the other k = 3 convolutions: Cin = 256 / 512, fp16x3 scaled per utterance from measured bounds (utterances x 1, x 30, x 1e-3),
    with and without the residual, LayerNorm of the stored row -> out2"""
    p, got = parity(dev, key)
    same_bits(got, run(dev, p, nan=False))


@pytest.mark.parametrize("key", TO_OUT, ids=case_id)
def test_to_out(dev, key):
    """to_out: K = 512, proven bound, the residual read from the buffer the launch then overwrites, LayerNorm3 -> out2"""
    p, got = parity(dev, key)
    assert p["in_place"]


@pytest.mark.parametrize("key", FF2, ids=case_id)
def test_ff2(dev, key):
    """ff.net.2: K = 1024, proven bound; ldo = 256 with the next LayerNorm1 -> out2, ldo = 512 writing columns 256..511 of the concat
    buffer, whose columns 0..255 keep their sentinel bit for bit; one case at M = 2048 = PARTIAL_ROWS"""
    p, got = parity(dev, key)
    if p.get("ldo") == 512:
        assert torch.isnan(got["full"][:, :256]).all()      # (run() fills the buffer with NaN)
        again = run(dev, p, fill=12345.678)                   # ... and with a finite sentinel: the same bits beside an untouched left half
        M = p["geo"]["M"]
        assert torch.equal(bits(got["out"][:M]), bits(again["out"][:M])) and torch.equal(bits(got["amax_out"]), bits(again["amax_out"]))
        assert torch.equal(bits(again["full"][M:]), bits(torch.full_like(again["full"][M:], 12345.678)))
        assert torch.equal(bits(again["full"][:, :256]), bits(torch.full_like(again["full"][:, :256], 12345.678)))


@pytest.mark.parametrize("key", CLAMP, ids=case_id)
def test_ksplit_clamp(dev, key):
    """Cin = 64, 96, 160 with one tap: min(ksplit, Cin >> 5) = 2, 3, 5 shares of one chunk each; no mask (the reduce tail's plain
    branch): every row below M is tracked, in its row_sample slot"""
    assert [len(share_chunks(key[2])), {hi - lo for lo, hi in share_chunks(key[2])}] == [key[2] // 32, {1}]
    parity(dev, key)


def test_stale_partials(dev):
    """an ff.net.2 launch leaves 8 x M x 256 partials in the hook's scratch; the Cin = 96 launch behind it writes three and its reduce
    may read those three only: inside the bound, and the same bits whatever the launch before it left behind"""
    big, small = case("ff2", "utt3", 256), ("clamp", "utt3", 96)
    p, r64, r32 = refs(*small)
    M = p["geo"]["M"]
    run(dev, big)
    first = run(dev, p)
    hold("stale_partials/out", first["out"][:M], r64["out"], r32["out"], slice(0, M))
    run(dev, big, A=-3.0 * big["A"])
    same_bits(first, run(dev, p))


@pytest.mark.parametrize("tile", ["0", "1", "2"])
def test_tile_variants(dev, monkeypatch, tile):
    """to_out under JV_TILE = 0 (128 x 128), 1 (64 x 128), 2 (64 x 64): each holds the bound -- the partial layout does not depend on
    the tile shape"""
    monkeypatch.setenv("JV_TILE", tile)
    key = ("to_out", "utt3", None)
    p, r64, r32 = refs(*key)
    M = p["geo"]["M"]
    got = {}
    report = pu.profiled(lambda: got.update(run(dev, p)))
    shape = {"0": "128x128", "1": "64x128", "2": "64x64"}[tile]      # the contraction did run on the forced tile, split, and was reduced once
    assert [k for k in report if k.startswith("conv_gemm_")] == [f"conv_gemm_h3<{shape}>"] and report["splitk_reduce"]["launches"] == 1, sorted(report)
    hold(f"tile_variants/tile{tile}/out", got["out"][:M], r64["out"], r32["out"], slice(0, M))
    hold(f"tile_variants/tile{tile}/out2", got["out2"][:M], r64["out2"], r32["out2"], fo.live(p["geo"]))
    exact_checks(p, got)


@pytest.mark.parametrize("key", [("conv3_trunk", "utt3", (256, True)), ("to_out", "utt3", None)], ids=case_id)
def test_np1(dev, key):
    """the one-product form (jv_op_set_products(1)) on the split-K route, held to test_gpu_fp16_ops.check against the chain whose
    operands are rounded as the hi planes hold them; both of its relations to the three-product result must hold"""
    p = case(*key)
    geo = p["geo"]
    M = geo["M"]
    one, three = f16.both(lambda: run(dev, p))
    r64, r32, u64 = ref_splitk(p, rounded=True), ref_splitk(p, torch.float32, rounded=True), refs(*key)[1]
    for n, rows in (("out", slice(0, M)), ("out2", fo.live(geo))):      # (check() records all its figures in parity_fp16_ops.json)
        kd, fl = fo.distances(one[n][:M], r64[n], r32[n], rows)
        record(f"np1/{case_id(key)}/{n}", kernel=kd, floor=fl, ratio=kd / fl)
    f16.check(f"splitk_np1/{case_id(key)}/out", one["out"][:M], three["out"][:M], r64["out"], r32["out"], u64["out"], slice(0, M),
              first=key[0] == "to_out")
    f16.check(f"splitk_np1/{case_id(key)}/out2", one["out2"][:M], three["out2"][:M], r64["out2"], r32["out2"], u64["out2"], fo.live(geo))
    assert not torch.equal(one["out"][:M].cpu()[fo.live(geo)], three["out"][:M].cpu()[fo.live(geo)])


# ---------------------------------------------------------------------------------------------------------------------------------
# exact properties
@pytest.mark.parametrize("key", [("conv3_trunk", "utt3", (256, True)), ("conv3_trunk", "utt3", (512, False)), ("to_out", "utt3", None)],
                         ids=case_id)
def test_batch_independence(dev, key):
    """utterance 0's rows from a launch over utterance 0 alone equal its rows from the three-utterance launch, bit for bit, in modes
    1 and 2: the split depends on K alone and the scales are per utterance (est_route: a row's bits do not depend on M)"""
    p = case(*key)
    whole, alone = run(dev, p), run(dev, p, rows_of=geo_of("utt0"))
    rows = fo.utt_rows(p["geo"], 0)
    assert geo_of("utt0")["start"][0] == p["geo"]["start"][0] and geo_of("utt0")["M"] < p["geo"]["M"]
    for n in ("out", "out2"):
        assert torch.equal(bits(whole[n][rows]), bits(alone[n][rows])), n
    assert torch.equal(bits(whole["amax_out"][:1]), bits(alone["amax_out"]))


def test_race_screen(dev):
    """twenty repeats of conv3_first and ff2 beside a streaming writer: identical bits (the partials are summed in fixed order)"""
    pa, pb = case("conv3_first", "utt3", "per_utt"), case("ff2", "utt3", 256)
    first_a, first_b = run(dev, pa), run(dev, pb)
    noise = fo.stream_noise(dev)
    for i in range(20):
        noise.normal_()
        same_bits(first_a, run(dev, pa))
        same_bits(first_b, run(dev, pb))


def test_rejects_other_widths(dev):
    """N != 256: JV_ERR_ARG, nothing launched"""
    from jyutvoice_amd._lib import JvError
    from jyutvoice_amd.engine import op_splitk
    out = torch.full((64, 256), 7.0, device=dev)
    with pytest.raises(JvError, match="256"):
        op_splitk(torch.zeros(64, 64, device=dev), torch.zeros(128, 64, device=dev), out=out, mode=2, a_bound=1.0)
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# the route pin: production takes this path at short M and leaves it where the batch fills the chip
def test_route_pin(tts_sd, noise):
    """One profiled estimator evaluation at B = 1, T = 64 (the CFG pair: 4 + 2 x 68 = 140 rows) reports as many splitk_reduce launches
    as estimator.hip has split call sites:
      conv3():  2 per resnet (block1, block2; res_conv is a 1 x 1 conv() and never splits) x 14 resnets (down, 12 mid, up)   = 28
                + trunk_conv() x 3 (down_conv, up_conv, final_conv)                                                          =  3
      block_tiles() with sk_blocks: to_out and ff.net.2, 2 per block x 4 blocks x 14 stages                                  = 112
    = 143; and one evaluation whose rows put it in the row-owning regime (rowgemm_tile(rows) > 0) reports none."""
    from jyutvoice_amd.engine import JV_MODEL_TTS, Engine
    T = 64
    eng = Engine("cuda:0", max_batch=32, max_frames=128, max_tokens=32)
    try:
        eng.load_state_dict(JV_MODEL_TTS, tts_sd)
        eng.load_noise(noise)

        def evaluate(n):
            g = torch.Generator().manual_seed(n)
            x, mu, spks = torch.randn(n, 80, T, generator=g), torch.randn(n, 80, T, generator=g), torch.randn(n, 80, generator=g)
            eng.flow_estimator(x.cuda(), torch.full((n,), T, dtype=torch.int32), mu.cuda(), torch.full((n,), 0.35).cuda(), spks.cuda(),
                               torch.zeros(n, 80, T).cuda())
            torch.cuda.synchronize()

        short = pu.profiled(lambda: evaluate(2))
        assert pu.rowgemm_tile(4 + 2 * (T + 4)) == 0
        assert short["splitk_reduce"]["launches"] == 2 * 14 + 3 + 2 * 4 * 14, short.get("splitk_reduce")
        n = 32
        assert pu.rowgemm_tile(4 + n * (T + 4)) > 0
        full = pu.profiled(lambda: evaluate(n))
        assert "splitk_reduce" not in full, full.get("splitk_reduce")
    finally:
        if hasattr(eng, "close"):
            eng.close()
