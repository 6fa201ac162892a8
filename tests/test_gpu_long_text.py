"""GPU: texts beyond 512 tokens through the context -- jv_encoder_fwd on the one-launch attention of encattn.hip, the mode switch
jv_encoder_set_attention, the workspace that no longer holds a [max_tokens, max_tokens] score buffer, synthesise() and forward().

Before encattn.hip every long case here ended in JvError ("the 512-token attention limit")."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ENC_TOL = 3e-4      # the bound tests/test_gpu_edges.py::test_encoder_tiny_and_ragged holds the encoder to


def md(a, b):
    return float((a.float().cpu() - b.float().cpu()).abs().max())


@pytest.fixture(scope="module")
def eng(tts_sd):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from jyutvoice_amd.engine import JV_MODEL_TTS, Engine
    e = Engine("cuda:0", max_batch=3, max_frames=64, max_tokens=1024)
    e.load_state_dict(JV_MODEL_TTS, tts_sd)
    yield e
    e.close()


_cases = {}


def case(tts_sd, Tt, lens):
    """(batch, the oracle's (h, mu_x, logw)), computed once per shape"""
    key = (Tt, tuple(lens))
    if key not in _cases:
        from jyutvoice_amd import synth
        from oracle import textenc as otext
        b = synth.batch(len(lens), Tt, first_index=200, lengths=lens)
        with torch.inference_mode():
            x_o, mu_o, mask_o = otext.text_encoder(tts_sd, b["x"], b["x_lengths"], b["lang"], b["tone"], b["word_pos"],
                                                   b["syllable_pos"], b["spk_embed"])
            logw_o = otext.duration_predictor(tts_sd, x_o, mask_o, b["spk_embed"])
        _cases[key] = (b, (x_o, mu_o, logw_o))
    return _cases[key]


def encode(eng, b, mode):
    eng.set_encoder_attention(mode)
    try:
        h, mu_x, logw, _ = eng.encoder(b["x"], b["x_lengths"], b["lang"], b["tone"], b["word_pos"], b["syllable_pos"], b["spk_embed"])
        return h.cpu(), mu_x.cpu(), logw.cpu()
    finally:
        eng.set_encoder_attention("auto")


@pytest.mark.parametrize("Tt,lens", [(513, [513]), (600, [600, 512, 1]), (1024, [1024, 700])])
def test_encoder_parity_above_512(eng, tts_sd, Tt, lens):
    b, want = case(tts_sd, Tt, lens)
    got = encode(eng, b, "auto")
    errs = [md(g, w) for g, w in zip(got, want)]
    print(f"encoder Tt={Tt} lens={lens}: h {errs[0]:.3e}  mu_x {errs[1]:.3e}  logw {errs[2]:.3e}")
    assert all(torch.isfinite(g).all() for g in got)
    assert max(errs) <= ENC_TOL


SHORT = [(37, [37, 36, 1]), (512, [512, 300])]


@pytest.mark.parametrize("Tt,lens", SHORT)
def test_fused_against_auto_at_short_lengths(eng, tts_sd, Tt, lens):
    """each output's error against the oracle: fused at most twice AUTO's (the four-launch route's), or 1e-6"""
    b, want = case(tts_sd, Tt, lens)
    auto, fused = encode(eng, b, "auto"), encode(eng, b, "fused")
    for name, a, f, w in zip(("h", "mu_x", "logw"), auto, fused, want):
        e_a, e_f = md(a, w), md(f, w)
        print(f"encoder Tt={Tt} lens={lens} {name}: fused {e_f:.3e}  auto {e_a:.3e}")
        assert e_f <= max(2 * e_a, 1e-6), name


@pytest.mark.parametrize("Tt,lens", SHORT)
def test_auto_is_the_gemm_route_up_to_512(eng, tts_sd, Tt, lens):
    b, _ = case(tts_sd, Tt, lens)
    auto, gemm = encode(eng, b, "auto"), encode(eng, b, "gemm")
    for a, g in zip(auto, gemm):
        assert torch.equal(a, g)


def test_mode_errors(eng, tts_sd):
    from jyutvoice_amd._lib import JvError
    b, _ = case(tts_sd, 513, [513])
    with pytest.raises(JvError, match="512-token attention limit"):
        encode(eng, b, "gemm")
    eng.set_encoder_attention("fused")
    try:
        with pytest.raises(ValueError):
            eng.set_encoder_attention("flash")
        assert eng.encoder_attention == "fused"
        assert eng.lib.jv_encoder_set_attention(eng._h, 7) != 0        # the library refuses too, and keeps the mode:
        short, _ = case(tts_sd, 37, [37, 36, 1])
        h = eng.encoder(short["x"], short["x_lengths"], short["lang"], short["tone"], short["word_pos"], short["syllable_pos"],
                        short["spk_embed"])[0].cpu()
    finally:
        eng.set_encoder_attention("auto")
    assert torch.equal(h, encode(eng, short, "fused")[0])


def test_workspace_is_linear_in_max_tokens():
    """a context for 8192 tokens beside one for 512: the score buffer alone, [1, 2, 8192, 8192] floats, would be 537 MB"""
    from jyutvoice_amd.engine import Engine
    torch.cuda.synchronize()

    def used_by(max_tokens):
        free0, _ = torch.cuda.mem_get_info()
        e = Engine("cuda:0", max_batch=1, max_frames=64, max_tokens=max_tokens)
        free1, _ = torch.cuda.mem_get_info()
        e.close()
        return free0 - free1

    small, large = used_by(512), used_by(8192)
    print(f"workspace: max_tokens 512 -> {small / 2 ** 20:.1f} MiB, 8192 -> {large / 2 ** 20:.1f} MiB, growth {(large - small) / 2 ** 20:.1f} MiB")
    assert large - small < 2 * 8192 * 8192 * 4


@pytest.fixture(scope="module")
def tts(tts_sd):
    import jyutvoice_amd
    model, _ = jyutvoice_amd.build_default("cuda:0")
    model.load_state_dict(tts_sd)
    return model


KEYS = ("x", "x_lengths", "lang", "tone", "word_pos", "syllable_pos", "spk_embed")
LONG_INDEX = 304      # synth.utterance(304, 520): 756 frames, and no duration within 1e-3 of an integer (asserted below)


def test_synthesise_520_tokens(tts, tts_sd, noise):
    from jyutvoice_amd import synth
    from oracle import tts as otts
    u = synth.batch(1, 520, first_index=LONG_INDEX)
    with torch.inference_mode():
        want = otts.synthesise(tts_sd, noise, *[u[k] for k in KEYS], None, n_timesteps=2)
    # durations are a ceiling: a token whose exp(logw) * length_scale sat on an integer could flip on an error of any size
    w = torch.exp(want["logw"])[0, 0].double()
    assert float((w - w.round()).abs().min()) >= 1e-3
    res = tts.synthesise(*[u[k] for k in KEYS], None, n_timesteps=2)
    assert torch.equal(res["mel_lengths"].cpu(), want["mel_lengths"])
    assert torch.equal(res["attn"].cpu(), want["attn"])                       # the path: every token's duration
    e = md(res["mel"], want["mel"])
    print(f"synthesise 520 tokens -> {int(want['mel_lengths'][0])} frames: mel against the oracle {e:.3e}")
    assert e <= 1e-3


def test_forward_520_tokens_600_frames(tts):
    """the alignment search's instantiations beyond 512 tokens (align.hip) are reachable through forward() now"""
    from jyutvoice_amd import synth
    Tt, Ty = 520, 600
    u = synth.batch(1, Tt, first_index=7)
    g = torch.Generator().manual_seed(99)
    y, decoder_h, z = torch.randn(1, 80, Ty, generator=g), torch.randn(1, Ty, 80, generator=g), torch.randn(1, 80, Ty, generator=g)
    dur_loss, prior_loss, diff_loss, attn = tts(u["x"], u["x_lengths"], y, torch.tensor([Ty]), u["lang"], u["tone"], u["word_pos"],
                                                u["syllable_pos"], u["spk_embed"], decoder_h, t=torch.tensor([0.3]), z=z,
                                                cfg_mask=torch.tensor([True]), cond_index=[0])
    for v in (dur_loss, prior_loss, diff_loss):
        assert torch.isfinite(v).all()
    attn = attn.cpu()
    assert tuple(attn.shape) == (1, Tt, Ty)
    assert torch.equal(attn[0].sum(0), torch.ones(Ty))                        # exactly one token per frame
    assert float(attn.min()) == 0.0 and float(attn.max()) == 1.0
    tok = attn[0].argmax(0)
    assert bool((tok[1:] >= tok[:-1]).all()) and int(tok[0]) == 0 and int(tok[-1]) == Tt - 1
