"""GPU: the evaluation forward() -- log prior, monotonic alignment search, the three losses (csrc/align.hip) -- against the restated
search (tests/mas_ref.py, bit for bit), fp64 on the CPU, and the CPU oracle for the encoder and the estimator."""
import functools
import math
import random

import numpy as np
import pytest
import torch

import mas_ref

pytestmark = pytest.mark.gpu

# The search: 256 threads, lanes own tokens tid + 256 k with k < NK, and the launcher picks NK = 1, 2, 4 or 8 from the PADDED token
# dimension Tx of the call (Tx <= 256, 512, 1024, 2048), so each t_x below gets a batch of its own, padded to exactly Tx = t_x:
# the small shapes run the instantiation a caller of that size gets (NK = 1 up to 256 tokens, 2 at 257 and 300), and 511 .. 513 /
# 1023 .. 1025 put a batch on either side of the 2 -> 4 and 4 -> 8 thresholds (512 and 1024: the last Tx of NK = 2 and NK = 4).
# Decision bits are 64-bit ballot words: 63 / 64 / 65 cross the first word and the wave, 255 / 256 / 257 the workgroup.
TX_MAIN = [1, 2, 63, 64, 65, 255, 256, 257, 300]
TX_WIDE = [511, 512, 513, 1023, 1024, 1025]


def batch_shapes(t_x):
    """a ragged batch whose longest utterance has t_x tokens: the forced diagonal, one spare frame, the ordinary case (for the
    wide ones a band of 38 cells per column, which keeps the double loops of the restatement quick), and a shorter utterance"""
    t_ys = [t_x, t_x + 1, 2 * t_x + 3] if t_x <= 300 else [t_x, t_x + 1, t_x + 37]
    half = max(1, t_x // 2)
    return [(t_x, t_y) for t_y in t_ys] + [(half, t_x if t_x <= 300 else half + 37)]


def make_scores(kind, shapes, seed):
    """ragged batch padded to a common [B, Tx, Ty] with NaN behind the lengths"""
    rng = np.random.default_rng(seed)
    Tx, Ty = max(s[0] for s in shapes), max(s[1] for s in shapes)
    v = np.full((len(shapes), Tx, Ty), np.nan, dtype=np.float32)
    for b, (t_x, t_y) in enumerate(shapes):
        v[b, :t_x, :t_y] = rng.normal(-150.0, 20.0, (t_x, t_y)) if kind == "gauss" else rng.integers(-3, 1, (t_x, t_y))
    return v


@functools.lru_cache(maxsize=None)
def search_case(kind, t_x):
    """(scores, t_xs, t_ys, paths, frame_index, durations): the restatement, computed once per batch"""
    shapes = batch_shapes(t_x)
    v = make_scores(kind, shapes, 1000 * (kind == "ties") + t_x)
    t_xs, t_ys = [s[0] for s in shapes], [s[1] for s in shapes]
    assert v.shape[1] == t_x
    return (v, t_xs, t_ys) + mas_ref.maximum_path(v, t_xs, t_ys)


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from jyutvoice_amd.engine import Engine
    e = Engine("cuda:0", max_batch=4, max_frames=1088, max_tokens=1056)
    yield e
    e.close()


def assert_search_equal(got, want):
    attn, fi, dur = got
    paths, fi_ref, dur_ref = want
    assert attn.dtype == torch.float32 and fi.dtype == torch.int32 and dur.dtype == torch.int32
    assert np.array_equal(fi.cpu().numpy(), fi_ref)
    assert np.array_equal(dur.cpu().numpy(), dur_ref)
    assert np.array_equal(attn.cpu().numpy(), paths.astype(np.float32))


# ---- 1. the search, exact -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gauss", "ties"])
@pytest.mark.parametrize("t_x", TX_MAIN + TX_WIDE)
def test_search_bit_exact(eng, kind, t_x):
    v, t_xs, t_ys, paths, fi, dur = search_case(kind, t_x)
    got = eng.maximum_path(torch.from_numpy(v), torch.tensor(t_xs), torch.tensor(t_ys))
    assert_search_equal(got, (paths, fi, dur))
    for b, (nx, ny) in enumerate(zip(t_xs, t_ys)):
        mas_ref.check_path(got[0][b].cpu().numpy(), nx, ny)


# ---- 2. the prior, accuracy -------------------------------------------------------------------------------------------------------
def prior_fp64(mu_x, h):
    """the header's expression in fp64: [B, Tx, Ty]"""
    d = h.double().unsqueeze(1) - mu_x.double().transpose(1, 2).unsqueeze(2)      # [B, Tx, Ty, 80]
    return -0.5 * d.pow(2).sum(-1) - 0.5 * math.log(2 * math.pi) * 80


def prior_reference_fp32(mu_x, decoder_h):
    """jyutvoice_tts.py:306-314 restated with torch on the CPU, fp32: three matmuls with factor = -0.5"""
    const = -0.5 * math.log(2 * math.pi) * 80
    factor = -0.5 * torch.ones(mu_x.shape, dtype=mu_x.dtype)
    h = decoder_h.transpose(1, 2)
    h_square = torch.matmul(factor.transpose(1, 2), h ** 2)
    h_mu_double = torch.matmul(2.0 * (factor * mu_x).transpose(1, 2), h)
    mu_square = torch.sum(factor * (mu_x ** 2), 1).unsqueeze(-1)
    return h_square - h_mu_double + mu_square + const


def inside(x_lens, y_lens, Tx, Ty):
    return (torch.arange(Tx)[None, :, None] < torch.tensor(x_lens)[:, None, None]) & \
           (torch.arange(Ty)[None, None, :] < torch.tensor(y_lens)[:, None, None])


def prior_bound(mu_x, h, m):
    """twice the max-abs error of the reference's own fp32 expression against fp64 on the same inputs (another, equally valid fp32
    summation order may land on the other side)"""
    want = prior_fp64(mu_x, h)
    return 2.0 * float((prior_reference_fp32(mu_x, h).double() - want)[m].abs().max()), want


@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_log_prior_accuracy(eng, scale):
    g = torch.Generator().manual_seed(int(10 * scale))
    B, Tx, Ty, x_lens, y_lens = 2, 37, 91, [37, 20], [91, 50]
    mu_x = torch.randn(B, 80, Tx, generator=g) * scale
    h = torch.randn(B, Ty, 80, generator=g) * scale
    m = inside(x_lens, y_lens, Tx, Ty)
    bound, want = prior_bound(mu_x, h, m)
    got = eng.log_prior(mu_x, h, torch.tensor(x_lens), torch.tensor(y_lens)).cpu()
    err = float((got.double() - want)[m].abs().max())
    print(f"log_prior scale {scale}: GPU max-abs error {err:.3e}, bound (2 x the reference's own) {bound:.3e}")
    assert err <= bound
    assert float(got[~m].abs().max()) == 0.0
    # the fused entry writes the same prior and searches it
    attn, fi, dur, lp = eng.align(mu_x, h, torch.tensor(x_lens), torch.tensor(y_lens), want_log_prior=True)
    assert torch.equal(lp.cpu(), got)
    paths, fi_ref, dur_ref = mas_ref.maximum_path(got.numpy(), x_lens, y_lens)
    assert_search_equal((attn, fi, dur), (paths, fi_ref, dur_ref))


# ---- 3. the mirror's own interface -----------------------------------------------------------------------------------------------
def test_maximum_path_interface():
    from jyutvoice_amd.utils.monotonic_align import maximum_path
    v, t_xs, t_ys, paths, _, _ = search_case("gauss", 257)
    B, Tx, Ty = v.shape
    mask = inside(t_xs, t_ys, Tx, Ty)
    value = torch.from_numpy(v).double().cuda()      # (every score is an fp32 number: the conversion inside is exact)
    out = maximum_path(value, mask.cuda().double())
    assert out.dtype == torch.float64 and out.device == value.device
    assert np.array_equal(out.cpu().numpy(), paths.astype(np.float64))
    out = maximum_path(torch.from_numpy(v[:2]), mask[:2].float())
    assert out.dtype == torch.float32 and out.device.type == "cpu"
    assert np.array_equal(out.numpy(), paths[:2].astype(np.float32))


# ---- 4. forward(), chained ---------------------------------------------------------------------------------------------------------
X_LENS, Y_LENS, TT, TY = [12, 20, 31], [40, 75, 120], 31, 120


@pytest.fixture(scope="module")
def tts(tts_sd):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    import jyutvoice_amd
    model, _ = jyutvoice_amd.build_default("cuda:0")
    model.load_state_dict(tts_sd)
    return model


@pytest.fixture(scope="module")
def fwd_inputs():
    from jyutvoice_amd import synth
    b = synth.batch(3, TT, first_index=40, lengths=X_LENS)
    g = torch.Generator().manual_seed(2024)
    y = torch.randn(3, 80, TY, generator=g)
    decoder_h = torch.randn(3, TY, 80, generator=g)
    args = (b["x"], b["x_lengths"], y, torch.tensor(Y_LENS), b["lang"], b["tone"], b["word_pos"], b["syllable_pos"], b["spk_embed"],
            decoder_h)
    kw = dict(t=torch.tensor([0.1, 0.5, 0.9]), z=torch.randn(3, 80, TY, generator=g), cfg_mask=torch.tensor([True, False, True]),
              cond_index=[10, 5, 0])
    return b, args, kw


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def test_forward_chained(tts, tts_sd, fwd_inputs):
    from oracle import flow as oflow
    from oracle import textenc as otext
    b, args, kw = fwd_inputs
    y, decoder_h = args[2], args[9]
    dur_loss, prior_loss, diff_loss, attn, parts = tts(*args, **kw, return_parts=True)
    assert dur_loss.dim() == 0 and prior_loss.dim() == 0 and diff_loss.dim() == 0 and dur_loss.device.type == "cuda"
    assert tuple(attn.shape) == (3, TT, TY)
    m = inside(X_LENS, Y_LENS, TT, TY)
    xm = (torch.arange(TT)[None] < torch.tensor(X_LENS)[:, None]).double()
    ym = (torch.arange(TY)[None] < torch.tensor(Y_LENS)[:, None]).double()

    # the prior: test 2's bound measured on these inputs, plus what the encoder's own tolerance (3e-4 on mu_x, tests/test_gpu_edges.py)
    # can move a cell by: |d log_prior| <= sum_c |h - mu_x| * 3e-4 + 0.5 * 80 * (3e-4)^2
    _, mu_o, _ = otext.text_encoder(tts_sd, b["x"], b["x_lengths"], b["lang"], b["tone"], b["word_pos"], b["syllable_pos"], b["spk_embed"])
    bound, want = prior_bound(mu_o, decoder_h, m)
    l1 = (decoder_h.double().unsqueeze(1) - mu_o.double().transpose(1, 2).unsqueeze(2)).abs().sum(-1)
    enc_tol = 3e-4
    bound += float(l1[m].max()) * enc_tol + 0.5 * 80 * enc_tol ** 2
    lp = parts["log_prior"].cpu()
    err = float((lp.double() - want)[m].abs().max())
    print(f"forward log_prior: max-abs error {err:.3e} against fp64 from the oracle's mu_x, bound {bound:.3e}")
    assert err <= bound and float(lp[~m].abs().max()) == 0.0

    # the search on the GPU's own prior: exact
    paths, fi_ref, dur_ref = mas_ref.maximum_path(lp.numpy(), X_LENS, Y_LENS)
    assert_search_equal((attn, parts["frame_index"], parts["durations"]), (paths, fi_ref, dur_ref))

    # duration and prior loss in fp64 from the GPU's attn, logw and mu_x
    a64, logw, mu_x = attn.cpu().double(), parts["logw"].cpu().double(), parts["mu_x"].cpu().double()
    logw_ = torch.log(1e-8 + a64.sum(-1)) * xm
    dur_ref64 = float(((logw[:, 0] - logw_) ** 2).sum() / sum(X_LENS))
    mu_y64 = torch.matmul(a64.transpose(1, 2), mu_x.transpose(1, 2)).transpose(1, 2)
    prior_ref64 = float((0.5 * ((decoder_h.double().transpose(1, 2) - mu_y64) ** 2 + math.log(2 * math.pi)) * ym[:, None]).sum()
                        / (sum(Y_LENS) * 80))
    print(f"dur_loss {float(dur_loss):.7f} (fp64 {dur_ref64:.7f}), prior_loss {float(prior_loss):.7f} (fp64 {prior_ref64:.7f})")
    assert rel(dur_loss, dur_ref64) <= 1e-5 and rel(prior_loss, prior_ref64) <= 1e-5
    assert torch.equal(parts["mu_y"].cpu().double(), mu_y64)      # a gather: the one-hot matmul exactly

    # the estimator's inputs: the reference's fp32 expressions on the CPU (flow_matching.py:319-334, jyutvoice_tts.py:325-330)
    t = 1 - torch.cos(kw["t"] * 0.5 * torch.pi)
    assert float((parts["t"].cpu() - t).abs().max()) <= 1e-6
    t = parts["t"].cpu()
    tb, z, cm = t.view(-1, 1, 1), kw["z"], kw["cfg_mask"].float()
    y_t = (1 - (1 - 1e-6) * tb) * z + tb * y
    u = y - (1 - 1e-6) * z
    cond = torch.zeros_like(y)
    for i, k in enumerate(kw["cond_index"]):
        cond[i, :, :k] = y[i, :, :k]
    cond = cond * cm.view(-1, 1, 1)
    mu_m = parts["mu_y"].cpu() * cm.view(-1, 1, 1)
    for name, want_t in (("y_t", y_t), ("u", u), ("cond", cond), ("mu_masked", mu_m)):
        e = float((parts[name].cpu() - want_t).abs().max())
        print(f"{name}: max-abs difference from the CPU formula {e:.3e}")
        assert e <= 1e-6, name
    # the speaker projection (jyutvoice_tts.py:288-289) from the state dict, at the encoder tolerance of tests/test_gpu_edges.py,
    # then its masking, which is one exact product per element
    c_ref = torch.nn.functional.linear(torch.nn.functional.normalize(b["spk_embed"], dim=1), tts_sd["spk_embed_affine_layer.weight"],
                                       tts_sd["spk_embed_affine_layer.bias"])
    e = float((parts["spks"].cpu() - c_ref).abs().max())
    print(f"spks: max-abs difference from normalize + affine on the CPU {e:.3e}")
    assert e <= 3e-4
    e = float((parts["spks_masked"].cpu() - parts["spks"].cpu() * cm.view(-1, 1)).abs().max())
    print(f"spks_masked: max-abs difference from spks * cfg_mask {e:.3e}")
    assert e <= 1e-6
    assert float(parts["spks_masked"][1].abs().max()) == 0.0 and float(parts["spks_masked"][0].abs().max()) > 0.0
    assert float(parts["cond"][2].abs().max()) == 0.0 and float(parts["cond"][0, :, 10:].abs().max()) == 0.0

    # the estimator evaluation on the GPU's own inputs, at test_estimator_vs_oracle_fresh's tolerance
    want_pred = oflow.estimator(tts_sd, parts["y_t"].cpu(), ym[:, None].float(), parts["mu_masked"].cpu(), t, parts["spks_masked"].cpu(),
                                parts["cond"].cpu())
    e = float((parts["pred"].cpu() - want_pred).abs().max())
    print(f"pred: max-abs difference from the oracle estimator {e:.3e}")
    assert e <= 2e-4

    # the flow-matching loss in fp64 from the GPU's own pred and u
    d = (parts["pred"].cpu().double() - parts["u"].cpu().double()) * ym[:, None]
    diff_ref64 = float((d ** 2).sum() / (sum(Y_LENS) * 80))
    print(f"diff_loss {float(diff_loss):.7f} (fp64 {diff_ref64:.7f})")
    assert rel(diff_loss, diff_ref64) <= 1e-5


# ---- 5. errors and determinism -----------------------------------------------------------------------------------------------------
def test_errors_name_the_utterance(tts, eng, fwd_inputs):
    from jyutvoice_amd._lib import JvError
    _, args, kw = fwd_inputs
    args = list(args)
    bad = list(args)
    bad[3] = torch.tensor([40, 19, 120])      # utterance 1: 19 frames for 20 tokens
    with pytest.raises(ValueError, match="utterance 1"):
        tts(*bad, **kw)
    bad = list(args)
    bad[1] = torch.tensor([12, 20, 0])
    with pytest.raises(ValueError, match="utterance 2"):
        tts(*bad, **kw)
    bad = list(args)
    bad[9] = args[9][:, :TY - 1]
    with pytest.raises(ValueError, match="decoder_h"):
        tts(*bad, **kw)
    # the library's own check, before anything is launched
    mu_x, h = torch.randn(3, 80, 8), torch.randn(3, 20, 80)
    with pytest.raises(JvError, match="utterance 1"):
        eng.align(mu_x, h, torch.tensor([8, 8, 8]), torch.tensor([20, 7, 20]))
    with pytest.raises(JvError, match="utterance 2"):
        eng.align(mu_x, h, torch.tensor([8, 8, 0]), torch.tensor([20, 20, 20]))
    with pytest.raises(JvError, match="utterance 0"):
        eng.maximum_path(torch.randn(3, 8, 20), torch.tensor([9, 8, 8]), torch.tensor([20, 20, 20]))
    with pytest.raises(JvError, match="capacity"):
        eng.maximum_path(torch.randn(1, 8, 1100), torch.tensor([8]), torch.tensor([20]))
    attn, fi, dur, _ = eng.align(mu_x, h, torch.tensor([8, 5, 1]), torch.tensor([20, 5, 20]))
    for b, (t_x, t_y) in enumerate([(8, 20), (5, 5), (1, 20)]):
        mas_ref.check_path(attn[b].cpu().numpy(), t_x, t_y)
    out = tts(*args, **kw)      # a valid call after the rejected ones
    assert all(bool(torch.isfinite(v).all()) for v in out)


def test_determinism_and_batch_equals_singles(tts, fwd_inputs):
    _, args, kw = fwd_inputs
    first = tts(*args, **kw, return_parts=True)
    again = tts(*args, **kw, return_parts=True)
    for a, c in zip(first[:4], again[:4]):
        assert torch.equal(a, c)
    assert torch.equal(first[4]["pred"], again[4]["pred"]) and torch.equal(first[4]["log_prior"], again[4]["log_prior"])

    # a batch is its utterances run singly: attn exactly; a loss is a quotient of fixed-order fp32 sums, so the batch's equals
    # the singles' recombined by their denominators up to the rounding of the regrouped partial sums -- 1e-6, relative
    num = [0.0, 0.0, 0.0]
    for b in range(3):
        nx, ny = X_LENS[b], Y_LENS[b]
        one = [v[b:b + 1] for v in args]
        one[0], one[4], one[5], one[6], one[7] = (one[i][:, :nx] for i in (0, 4, 5, 6, 7))
        one[2], one[9] = one[2][:, :, :ny], one[9][:, :ny]
        kw1 = dict(t=kw["t"][b:b + 1], z=kw["z"][b:b + 1, :, :ny], cfg_mask=kw["cfg_mask"][b:b + 1], cond_index=kw["cond_index"][b:b + 1])
        d, p, f, attn1 = tts(*one, **kw1)
        assert torch.equal(attn1[0], first[3][b, :nx, :ny])
        assert float(first[3][b, nx:].abs().max() if nx < TT else 0.0) == 0.0 and float(first[3][b, :, ny:].abs().sum()) == 0.0
        num[0] += float(d.double()) * nx
        num[1] += float(p.double()) * ny
        num[2] += float(f.double()) * ny
    for name, got, want in (("dur_loss", first[0], num[0] / sum(X_LENS)), ("prior_loss", first[1], num[1] / sum(Y_LENS)),
                            ("diff_loss", first[2], num[2] / sum(Y_LENS))):
        print(f"{name}: batch {float(got):.8f}, singles recombined {want:.8f}, relative difference {rel(got, want):.2e}")
        assert rel(got, want) <= 1e-6, name


def test_seeded_draws_repeat(tts, fwd_inputs):
    _, args, _ = fwd_inputs
    outs = []
    for _ in range(2):
        random.seed(7)
        g = torch.Generator(device="cuda").manual_seed(7)
        outs.append(tts(*args, generator=g))
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    random.seed(8)
    other = tts(*args, generator=torch.Generator(device="cuda").manual_seed(8))
    assert not torch.equal(other[2], outs[0][2])      # another seed, another noise: the flow-matching loss moves
