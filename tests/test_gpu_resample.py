"""GPU: jv_resample (resample.hip) -- `torchaudio.functional.resample` with its defaults (infer.py:368-382) for a ragged batch in one
launch -- against the fp64 restatement of tests/resample_ref.py, up through `extract_speech_feat_batch(sample_rates=...)` and the CLI.

The bound is derived, not measured: every output sample satisfies

    |y_gpu - y_fp64| <= (K + 3) 2^-24 sum_k |tab[p][k]| |x[i o + k - width]|

-- K fused multiply-adds of relative error 2^-24 each, the table's one rounding to fp32, and headroom (resample_ref.bound).
test_resample_host.py shows what lands outside it.  Kernel distance, bound and ratio per case go to parity_resample.json in the
output directory."""
import json
import struct

import numpy as np
import pytest
import torch

import resample_ref as ref
from parity_util import Recorder

pytestmark = pytest.mark.gpu

# beyond the eight pairs: the two sizes at which the launcher takes another path -- 192000 -> 8000 (o = 24, n = 1, K = 316): the
# span of 1024 output samples does not fit the LDS budget and the tile is halved; 48000 -> 48 (o = 1000, n = 1, K = 13122): not
# even one tile's span fits, taps are read from global memory
OTHER_PATHS = [(192000, 8000), (48000, 48)]

REC = Recorder("parity_resample.json", {
    "what": "jv_resample against the fp64 restatement (tests/resample_ref.py), per rate pair and case",
    "bound": "(K + 3) 2^-24 sum_k |tab[p][k]| |x[i o + k - width]| per output sample: derived, not measured",
    "columns": "distance = max over samples of |y_gpu - y_fp64|, bound = max over samples of the bound, ratio = max over samples of "
               "distance / bound (asserted <= 1 sample by sample); ends / tiny: the recording of the batch with the largest ratio"})


@pytest.fixture(scope="module")
def eng():
    from jyutvoice_amd.runtime import get_runtime
    return get_runtime("cuda:0").ensure(1, 64, 1)


def pair_id(p):
    return f"{p[0]}-{p[1]}"


def check_recording(got, x, orig, new):
    """one recording's output samples against the definition: (max distance, max bound, max ratio); asserts the bound"""
    want, bnd = ref.resample64(x, orig, new), ref.bound(x, orig, new)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0, 0.0, 0.0
    assert np.isfinite(got).all()
    dist = np.abs(got.astype(np.float64) - want)
    assert (dist <= bnd).all(), (orig, new, float(dist.max()), int(np.argmax(dist - bnd)))
    ratio = np.divide(dist, bnd, out=np.zeros_like(dist), where=bnd > 0)
    return float(dist.max()), float(bnd.max()), float(ratio.max())


_ends = {}


def ends_batch(eng, orig, new):
    """B = 40 recordings of 6001 .. 6040 samples in one call, NaN behind every length (computed once per pair, shared)"""
    if (orig, new) not in _ends:
        x = ref.signal(ref.pair_seed(orig, new) + 1, ref.ENDS_B * ref.ENDS_N).reshape(ref.ENDS_B, ref.ENDS_N)
        lens = np.arange(ref.ENDS_N - ref.ENDS_B + 1, ref.ENDS_N + 1)
        buf = torch.from_numpy(x).clone()
        for b, n in enumerate(lens):
            buf[b, n:] = float("nan")
        out, out_lens = eng.resample(buf, orig, new, torch.from_numpy(lens))
        _ends[(orig, new)] = (x, lens, buf, out.cpu(), out_lens.cpu())
    return _ends[(orig, new)]


# ---- the bound, at the shapes where it can go wrong ---------------------------------------------------------------------------
@pytest.mark.parametrize("pair", ref.PAIRS + OTHER_PATHS, ids=pair_id)
def test_tile_seams(eng, pair):
    """one recording of 20 011 samples, EVERY output sample checked: whatever the tile size, its seams are inside"""
    orig, new = pair
    x = ref.signal(ref.pair_seed(orig, new), ref.SEAM_SAMPLES)
    out = eng.resample(torch.from_numpy(x)[None], orig, new)
    assert out.shape == (1, ref.out_length(x.size, orig, new))
    d, b, r = check_recording(out[0].cpu().numpy(), x, orig, new)
    REC(f"{orig}->{new} seams", distance=d, bound=b, ratio=r)


@pytest.mark.parametrize("pair", ref.PAIRS, ids=pair_id)
def test_recording_ends(eng, pair):
    """40 recordings whose ends fall on 40 consecutive offsets, NaN behind each: every sample inside the bound, exact zeros behind
    out_lens, out_lens exact"""
    orig, new = pair
    x, lens, _, out, out_lens = ends_batch(eng, orig, new)
    assert out.shape == (ref.ENDS_B, ref.out_length(ref.ENDS_N, orig, new))
    assert out_lens.dtype == torch.int32 and out_lens.tolist() == [ref.out_length(int(n), orig, new) for n in lens]
    worst = (0.0, 0.0, 0.0)
    for b, n in enumerate(lens):
        L = int(out_lens[b])
        worst = max(worst, check_recording(out[b, :L].numpy(), x[b, :n], orig, new), key=lambda t: t[2])
        assert torch.equal(out[b, L:], torch.zeros(out.shape[1] - L))
    REC(f"{orig}->{new} ends", distance=worst[0], bound=worst[1], ratio=worst[2])


@pytest.mark.parametrize("pair", ref.PAIRS, ids=pair_id)
def test_tiny_recordings(eng, pair):
    """lengths around every constant of the filter, 0 included, in one batch of n_in = K + 1, NaN behind"""
    orig, new = pair
    o, n, width, K, _ = ref.geometry(orig, new)
    lens = [0, 1, 2, width - 1, width, width + 1, o - 1, o, o + 1, K - 1, K, K + 1]
    x = ref.signal(ref.pair_seed(orig, new) + 2, len(lens) * (K + 1)).reshape(len(lens), K + 1)
    buf = torch.from_numpy(x).clone()
    for b, L in enumerate(lens):
        buf[b, L:] = float("nan")
    out, out_lens = eng.resample(buf, orig, new, torch.tensor(lens))
    out, out_lens = out.cpu(), out_lens.cpu()
    assert out_lens.tolist() == [ref.out_length(L, orig, new) for L in lens]
    worst = (0.0, 0.0, 0.0)
    for b, L in enumerate(lens):
        Lo = int(out_lens[b])
        worst = max(worst, check_recording(out[b, :Lo].numpy(), x[b, :L], orig, new), key=lambda t: t[2])
        assert torch.equal(out[b, Lo:], torch.zeros(out.shape[1] - Lo))
    REC(f"{orig}->{new} tiny", distance=worst[0], bound=worst[1], ratio=worst[2])


# ---- bit-equality: a sample's sum does not depend on where it lies -----------------------------------------------------------------
@pytest.mark.parametrize("pair", ref.PAIRS, ids=pair_id)
def test_row_of_a_batch_equals_the_recording_alone(eng, pair):
    orig, new = pair
    x, lens, buf, out, out_lens = ends_batch(eng, orig, new)
    for b in (0, 17, 39):
        alone = eng.resample(buf[b:b + 1, :int(lens[b])], orig, new).cpu()
        assert alone.shape[1] == int(out_lens[b])
        assert torch.equal(alone[0], out[b, :alone.shape[1]])


@pytest.mark.parametrize("pair", ref.PAIRS, ids=pair_id)
def test_lengths_are_clamped_and_none_is_full(eng, pair):
    orig, new = pair
    n_in = 3001
    x = torch.from_numpy(ref.signal(ref.pair_seed(orig, new) + 3, 4 * n_in).reshape(4, n_in))
    full = eng.resample(x, orig, new).cpu()
    out, out_lens = eng.resample(x, orig, new, torch.tensor([n_in] * 4))
    assert torch.equal(out.cpu(), full) and out_lens.tolist() == [full.shape[1]] * 4
    want, want_lens = eng.resample(x, orig, new, torch.tensor([0, n_in, 1500, n_in]))
    got, got_lens = eng.resample(x, orig, new, torch.tensor([-5, n_in + 7, 1500, 2 ** 31 - 1]))
    assert torch.equal(got, want) and torch.equal(got_lens, want_lens)
    assert got_lens.tolist() == [0, full.shape[1], ref.out_length(1500, orig, new), full.shape[1]]
    assert torch.equal(got[1].cpu(), full[1]) and float(got[0].abs().sum()) == 0.0


def test_table_cache_and_reserve_do_not_change_bits(eng):
    """pair A, then B, then A again; more distinct pairs than the cache holds, then A again; A before and after a jv_reserve growth"""
    from jyutvoice_amd.runtime import get_runtime
    x = torch.from_numpy(ref.signal(77, 2 * 5003).reshape(2, 5003))
    a1 = eng.resample(x, 44100, 24000)
    b1 = eng.resample(x, 16000, 24000)
    assert torch.equal(eng.resample(x, 44100, 24000), a1)
    assert torch.equal(eng.resample(x, 88200, 48000), a1)      # the same reduced pair: the same table
    for new in (8000, 11025, 12000, 16000, 22050, 32000, 44100, 48000, 96000):      # nine more tables: the oldest ones go
        eng.resample(x[:, :500], 24000, new)
    assert torch.equal(eng.resample(x, 44100, 24000), a1) and torch.equal(eng.resample(x, 16000, 24000), b1)
    rt = get_runtime("cuda:0")
    caps = rt.caps
    grown = rt.ensure(caps[0] + 1, caps[1] + 64, caps[2])
    assert grown is eng and rt.caps != caps
    assert torch.equal(eng.resample(x, 44100, 24000), a1)


def test_equal_rates_return_the_input_inside_the_lengths(eng):
    x = torch.from_numpy(ref.signal(78, 3 * 2500).reshape(3, 2500))
    assert torch.equal(eng.resample(x, 24000, 24000).cpu(), x)
    buf = x.clone()
    lens = [2500, 1, 1234]
    for b, L in enumerate(lens):
        buf[b, L:] = float("nan")
    out, out_lens = eng.resample(buf, 16000, 16000, torch.tensor(lens))
    assert out_lens.tolist() == lens and out.shape == x.shape
    for b, L in enumerate(lens):
        assert torch.equal(out[b, :L].cpu(), x[b, :L]) and torch.equal(out[b, L:].cpu(), torch.zeros(2500 - L))


# ---- errors --------------------------------------------------------------------------------------------------------------------
def test_errors_come_before_the_launch_and_leave_the_context_usable(eng):
    from jyutvoice_amd._lib import JvError
    from jyutvoice_amd.engine import _ptr, _stream
    x = torch.from_numpy(ref.signal(79, 4000)[None]).cuda()
    good = eng.resample(x, 44100, 24000)
    for orig, new in ((0, 24000), (24000, 0), (-44100, 24000), (24000, -1)):
        with pytest.raises(JvError) as e:
            eng.resample(x, orig, new)
        assert e.value.code == 1
    with pytest.raises(JvError, match=r"o = 44101, n = 24000.*1048576") as e:
        eng.resample(x, 44101, 24000)
    assert e.value.code == 1
    need = ref.out_length(4000, 44100, 24000)
    short = torch.full((1, need - 1), 7.0, device="cuda")
    rc = eng.lib.jv_resample(eng._h, _ptr(x), None, 1, 4000, 44100, 24000, _ptr(short), need - 1, None, _stream(eng.device))
    assert rc == 4 and b"n_out" in eng.lib.jv_last_error()
    assert float(short.min()) == 7.0 == float(short.max())      # nothing was launched
    assert torch.equal(eng.resample(x, 44100, 24000), good)
    wide = torch.full((1, need + 9), 7.0, device="cuda")      # a wider output: zeros behind the signal
    assert eng.lib.jv_resample(eng._h, _ptr(x), None, 1, 4000, 44100, 24000, _ptr(wide), need + 9, None, _stream(eng.device)) == 0
    assert torch.equal(wide[:, :need], good) and float(wide[:, need:].abs().sum()) == 0.0


# ---- composition ----------------------------------------------------------------------------------------------------------------
def test_batch_extraction_at_mixed_rates_equals_resample_then_extract():
    """four recordings at 16 000, 44 100, 24 000 and 48 000 Hz through extract_speech_feat_batch(sample_rates=...): per recording the
    bits of `resample` alone followed by `extract_speech_feat`; the 24 kHz member is today's extract_speech_feat of the raw recording"""
    from jyutvoice_amd.utils.audio import extract_speech_feat, extract_speech_feat_batch, resample
    rates, seconds = [16000, 44100, 24000, 48000], [0.9, 0.63, 0.5, 0.71]
    gen = torch.Generator().manual_seed(21)
    wavs = [(torch.randn(1, int(s * r), generator=gen) * 0.2).clamp(-1, 1) for r, s in zip(rates, seconds)]
    feat, feat_len = extract_speech_feat_batch(wavs, sample_rates=rates)
    assert feat_len.dtype == torch.int32 and feat.shape[0] == 4 and feat.shape[2] == 80
    for b, (w, r) in enumerate(zip(wavs, rates)):
        w24 = resample(w, r, 24000)
        assert w24.shape == (1, ref.out_length(w.shape[1], r, 24000))
        one, n = extract_speech_feat(w24)
        T = int(n[0])
        assert int(feat_len[b]) == T == 1 + (w24.shape[1] - 480) // 480
        assert torch.equal(feat[b, :T], one[0]), b
        assert float(feat[b, T:].abs().sum()) == 0.0
    raw, n = extract_speech_feat(wavs[2])
    assert torch.equal(feat[2, :int(n[0])], raw[0])
    flat = resample(wavs[0][0], 16000, 24000)      # 1-D in, 1-D out
    assert flat.dim() == 1 and torch.equal(flat, resample(wavs[0], 16000, 24000)[0])


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory, prompt_sd):
    from jyutvoice_amd import synth
    from jyutvoice_amd.flow.encoder import extract_flow_weights
    d = tmp_path_factory.mktemp("resample_cli")
    torch.save(extract_flow_weights(dict(prompt_sd))[0], d / "flow_encoder.pt")
    torch.save({"state_dict": synth.tts_state_dict()}, d / "tts.ckpt")
    torch.save(synth.hift_state_dict(), d / "hift.pt")
    return d, ["--tts_checkpoint", str(d / "tts.ckpt"), "--hift", str(d / "hift.pt"), "--flow_encoder", str(d / "flow_encoder.pt"),
               "--n_timesteps", "2", "--seed", "7"]


def requests(d, recordings):
    """one cloning request per (key, file): 8 / 10 / 12 text tokens, 20 prompt tokens each"""
    from jyutvoice_amd import synth
    utts = []
    for b, (key, name) in enumerate(recordings):
        u = synth.batch(1, 8 + 2 * b, first_index=b)
        tok, _ = synth.prompt_tokens(1, 20, first_index=b)
        obj = {k: u[k][0].tolist() for k in ("x", "lang", "tone", "word_pos", "syllable_pos")}
        obj["interspersed"] = False
        obj.update({"spk_embed": u["spk_embed"][0].tolist(), "prompt_token": tok[0].tolist(), key: str(d / name)})
        utts.append(obj)
    return utts


def read_wav16(path):
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and data[8:16] == b"WAVEfmt " and data[36:40] == b"data"
    code, channels, rate, _, _, bits = struct.unpack("<HHIIHH", data[20:36])
    assert (code, channels, bits) == (1, 1, 16)
    return rate, torch.frombuffer(bytearray(data[44:]), dtype=torch.int16)


def test_cli_prompts_at_any_rate_and_output_rate(checkpoints):
    """the list route with prompt_wav files at 16 kHz (8-bit), 44.1 kHz (24-bit stereo) and 48 kHz (float32): with --sample_rate 16000
    the files say 16 000 Hz, hold ceil(2 frames 480 / 3) samples and are not silent; frames from the same list at 24 kHz"""
    import infer
    d, common = checkpoints
    rng = np.random.default_rng(5)
    ref.write_wav(d / "a.wav", rng.normal(0, 0.1, 16000).clip(-1, 1), 16000, 8)
    ref.write_wav(d / "b.wav", rng.normal(0, 0.1, (44100, 2)).clip(-1, 1), 44100, 24)
    ref.write_wav(d / "c.wav", rng.normal(0, 0.1, 40000).clip(-1, 1), 48000, 32, code=3)
    json.dump(requests(d, [("prompt_wav", "a.wav"), ("prompt_wav", "b.wav"), ("prompt_wav", "c.wav")]), open(d / "any.json", "w"))
    infer.main(["--output", str(d / "r24.wav"), "--tokens", str(d / "any.json")] + common)
    infer.main(["--output", str(d / "r16.wav"), "--tokens", str(d / "any.json"), "--sample_rate", "16000"] + common)
    for b in range(3):
        rate24, pcm24 = read_wav16(d / f"r24_{b:03d}.wav")
        rate16, pcm16 = read_wav16(d / f"r16_{b:03d}.wav")
        assert rate24 == 24000 and pcm24.numel() % 480 == 0 and pcm24.numel() > 0
        frames = pcm24.numel() // 480
        assert rate16 == 16000 and pcm16.numel() == -(-2 * frames * 480 // 3)
        assert int(pcm16.int().abs().max()) > 100 and int(pcm24.int().abs().max()) > 100      # (not silence)


def test_cli_24k_recordings_unchanged_and_single_request(checkpoints):
    """16-bit 24 kHz recordings: the list by `prompt_wav` writes the samples the untouched `prompt_wav_24k` route writes (at 24 kHz
    jv_resample is a copy); a single request with `prompt_wav` at 44.1 kHz and --sample_rate 8000 says 8 000 Hz at a third of the length"""
    import infer
    d, common = checkpoints
    rng = np.random.default_rng(6)
    for name, n in (("p.wav", 26000), ("q.wav", 19000)):
        ref.write_wav(d / name, rng.normal(0, 0.1, n).clip(-1, 1), 24000, 16)
    for key in ("prompt_wav_24k", "prompt_wav"):
        json.dump(requests(d, [(key, "p.wav"), (key, "q.wav")]), open(d / f"{key}.json", "w"))
        infer.main(["--output", str(d / f"{key}.wav"), "--tokens", str(d / f"{key}.json")] + common)
    for b in range(2):
        old, new = read_wav16(d / f"prompt_wav_24k_{b:03d}.wav"), read_wav16(d / f"prompt_wav_{b:03d}.wav")
        assert old[0] == new[0] == 24000 and torch.equal(old[1], new[1]) and int(old[1].int().abs().max()) > 100
    ref.write_wav(d / "s.wav", rng.normal(0, 0.1, 33000).clip(-1, 1), 44100, 16)
    json.dump(requests(d, [("prompt_wav", "s.wav")])[0], open(d / "single.json", "w"))
    infer.main(["--output", str(d / "s24.wav"), "--tokens", str(d / "single.json")] + common)
    infer.main(["--output", str(d / "s8.wav"), "--tokens", str(d / "single.json"), "--sample_rate", "8000"] + common)
    (r24, p24), (r8, p8) = read_wav16(d / "s24.wav"), read_wav16(d / "s8.wav")
    assert r24 == 24000 and r8 == 8000 and p24.numel() % 480 == 0 and p8.numel() == -(-p24.numel() // 3)
    assert int(p8.int().abs().max()) > 100
