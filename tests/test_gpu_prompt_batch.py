"""GPU: the voice-cloning BATCH -- `synthesise(..., batched=True, prompt_lengths=p)`, every utterance with a prompt of its own
length (jv_cfm_solve_prompted), the ragged prompt mel (jv_mel_spectrogram_ragged) and the CLI's list route.

The definition everything is checked against: the batch-1 reference (jyutvoice_tts.py:213-244) looped over the utterances,
utterance b called with prompt_feat[b:b+1, :p_b] and prompt_h[b:b+1, :p_b]; p_b = 0 is the unprompted call.
Tolerances are the ones the suite already uses for the same paths (named at each assertion)."""
import json
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("x", "x_lengths", "lang", "tone", "word_pos", "syllable_pos", "spk_embed")
# test_compact_geometry_equals_uniform's 12-utterance batch (with fixed_duration=1.5 it takes the compact geometry)
LENGTHS12 = [150, 61, 97, 133, 60, 149, 88, 120, 75, 142, 101, 66]
PROMPT_TOKENS12 = [15, 33, 0, 22, 40, 8, 27, 12, 36, 5, 19, 30]


def md(a, b):
    return float((a.detach().cpu().float() - b.detach().cpu().float()).abs().max())


@pytest.fixture(scope="module")
def fenc(prompt_sd):
    from jyutvoice_amd.flow.encoder import FlowEncoder
    m = FlowEncoder(vocab_size=6561, input_size=512, output_size=80, device="cuda:0")
    m.load_state_dict(prompt_sd)
    return m


def new_tts(sd):
    import jyutvoice_amd
    tts, _ = jyutvoice_amd.build_default("cuda:0")
    tts.load_state_dict(sd)
    return tts


def make_prompts(fenc, prompt_tokens, seed=3, P_feat=None, P_h=None, fill=0.0):
    """prompts of prompt_tokens[b] speech tokens (0 = none) -> (tok, prompt_feat [B,P,80], prompt_h [B,P',80], prompt_lengths);
    the ones that exist go through the prompt encoder as one ragged token batch, a prompt-less utterance gets a row of
    padding in both tensors.  `fill` is what lies behind p_b (NaN: must not be read)."""
    from jyutvoice_amd import synth
    B = len(prompt_tokens)
    have = [b for b, n in enumerate(prompt_tokens) if n > 0]
    p = [2 * n for n in prompt_tokens]
    tok, lens = synth.prompt_tokens(len(have), max(prompt_tokens), lengths=[prompt_tokens[b] for b in have], first_index=1)
    h, _ = fenc(tok, lens)
    P_feat, P_h = P_feat or max(p), P_h or max(p)
    prompt_h = torch.full((B, P_h, 80), fill)
    prompt_feat = torch.full((B, P_feat, 80), fill)
    g = torch.Generator().manual_seed(seed)
    for b in range(B):
        f = torch.randn(p[b], 80, generator=g)      # (drawn for every b so that the values do not depend on P)
        prompt_feat[b, :p[b]] = f
    for i, b in enumerate(have):
        prompt_h[b, :p[b]] = h[i, :p[b]].cpu()
    return (tok, lens, have), prompt_feat, prompt_h, torch.tensor(p, dtype=torch.int64)


def run(tts, batch, prompt_feat, prompt_h, prompt_lengths, n_timesteps, sl=slice(None)):
    args = [batch[k][sl] for k in KEYS]      # (a sub-batch keeps the batch's padded token width: x_lengths masks the padding)
    return tts.synthesise(*args, prompt_feat[sl], prompt_h=prompt_h[sl], n_timesteps=n_timesteps, batched=True,
                          prompt_lengths=prompt_lengths[sl])


def single(batch, b):
    """utterance b of a padded batch as the B = 1 call takes it"""
    L = int(batch["x_lengths"][b])
    return [batch[k][b:b + 1] if k in ("x_lengths", "spk_embed") else batch[k][b:b + 1, :L] for k in KEYS]


CASE1_TOKENS, CASE1_PROMPTS = [24, 40, 31, 24], [15, 33, 0, 22]


def test_definition_against_oracle(fenc, prompt_sd, tts_sd, noise):
    """1. B = 4, tokens 24 / 40 / 31 / 24, prompts of 30 / 66 / 0 / 44 frames, n = 4, against a loop of the B = 1 oracle with each
    utterance's own slices (the oracle's own prompt encoder, as test_prompted_synthesis_uses_prompt_h; p_b = 0: no prompt).
    1e-3 max-abs is that test's bound for the same path."""
    from jyutvoice_amd import synth
    from oracle import prompt as oprompt
    from oracle import tts as otts
    tts = new_tts(tts_sd)
    batch = synth.batch(4, 40, lengths=CASE1_TOKENS)
    (tok, lens, have), prompt_feat, prompt_h, p = make_prompts(fenc, CASE1_PROMPTS)
    assert p.tolist() == [30, 66, 0, 44] and prompt_feat.shape == prompt_h.shape == (4, 66, 80)
    res = run(tts, batch, prompt_feat, prompt_h, p, 4)
    mel, lengths = res["mel"].cpu(), res["mel_lengths"].cpu()
    assert res["decoder_outputs"] is res["mel"]
    want = []
    for b in range(4):
        one = single(batch, b)
        if p[b] == 0:
            w = otts.synthesise(tts_sd, noise, *one, n_timesteps=4)
        else:
            i = have.index(b)
            ph_o, _ = oprompt.flow_encoder(prompt_sd, tok[i:i + 1, :int(lens[i])], lens[i:i + 1])
            w = otts.synthesise(tts_sd, noise, *one, prompt_feat[b:b + 1, :p[b]], prompt_h=ph_o, n_timesteps=4)
        want.append(w)
    y = [int(w["mel_lengths"][0]) for w in want]
    assert lengths.tolist() == y
    assert mel.shape == (4, 80, max(y))
    for b in range(4):
        assert want[b]["mel"].shape == (1, 80, y[b])
        err = md(mel[b, :, :y[b]], want[b]["mel"][0])
        print(f"utterance {b}: p = {int(p[b])}, y = {y[b]}, max-abs vs oracle {err:.3e}")
        assert err <= 1e-3, (b, err)
        assert float(mel[b, :, y[b]:].abs().sum()) == 0.0, b
    assert res["encoder_outputs"].shape == (4, 80, max(y)) and res["attn"].shape == (4, 1, 40, max(y))


def test_equal_prompts_same_bits_as_shared_length_path(fenc):
    """2. all p_b equal (30 frames): bit-identical to today's synthesise(batched=True) with the same prompt_feat / prompt_h and no
    prompt_lengths -- for a batch that stays in the uniform geometry (equal token counts) and one that takes the compact one"""
    from jyutvoice_amd import synth
    tts = new_tts(synth.tts_state_dict(fixed_duration=1.5))
    for batch, B in ((synth.batch(4, 24), 4), (synth.batch(12, 150, first_index=5, lengths=LENGTHS12), 12)):
        _, prompt_feat, prompt_h, p = make_prompts(fenc, [15] * B)
        assert p.tolist() == [30] * B
        new = run(tts, batch, prompt_feat, prompt_h, p, 2)
        old = tts.synthesise(*[batch[k] for k in KEYS], prompt_feat, prompt_h=prompt_h, n_timesteps=2, batched=True)
        assert torch.equal(new["mel_lengths"], old["mel_lengths"])
        assert new["mel"].shape == old["mel"].shape and torch.isfinite(new["mel"]).all()
        assert torch.equal(new["mel"], old["mel"]), (B, md(new["mel"], old["mel"]))


def test_batch_equals_singles_and_halves(fenc):
    """3. a ragged-prompt batch of 12 against the library's own B = 1 prompted calls (the shared-length path that exists, given
    each utterance's slices; no prompt for p_b = 0) and against the same batch run as 6 + 6: <= 2e-5, the cross-regime bound of
    test_gpu_dist.py / test_gpu_flow.py (B = 1 runs split-K)"""
    from jyutvoice_amd import synth
    tts = new_tts(synth.tts_state_dict(fixed_duration=1.5))
    batch = synth.batch(12, 150, first_index=5, lengths=LENGTHS12)
    _, prompt_feat, prompt_h, p = make_prompts(fenc, PROMPT_TOKENS12)
    full = run(tts, batch, prompt_feat, prompt_h, p, 2)
    mel, y = full["mel"].cpu(), full["mel_lengths"].cpu().tolist()
    halves = [run(tts, batch, prompt_feat, prompt_h, p, 2, slice(0, 6)), run(tts, batch, prompt_feat, prompt_h, p, 2, slice(6, 12))]
    for i, h in enumerate(halves):
        assert h["mel_lengths"].cpu().tolist() == y[6 * i:6 * i + 6]
        for j in range(6):
            b = 6 * i + j
            err = md(h["mel"][j, :, :y[b]], mel[b, :, :y[b]])
            print(f"utterance {b}: batch of 12 vs batch of 6: {err:.3e}")
            assert err <= 2e-5, (b, err)
    for b in range(12):
        one = single(batch, b)
        if p[b] == 0:
            solo = tts.synthesise(*one, None, n_timesteps=2)
        else:
            solo = tts.synthesise(*one, prompt_feat[b:b + 1, :p[b]], prompt_h=prompt_h[b:b + 1, :p[b]], n_timesteps=2)
        assert solo["mel"].shape == (1, 80, y[b])
        err = md(solo["mel"][0], mel[b, :, :y[b]])
        print(f"utterance {b}: p = {int(p[b])}, y = {y[b]}: batch of 12 vs B = 1: {err:.3e}")
        assert err <= 2e-5, (b, err)
        assert float(mel[b, :, y[b]:].abs().sum()) == 0.0


def test_padding_is_not_read(fenc, tts_sd):
    """4. case 1 with NaN behind p_b in both tensors and P != P': the same bits as case 1"""
    from jyutvoice_amd import synth
    tts = new_tts(tts_sd)
    batch = synth.batch(4, 40, lengths=CASE1_TOKENS)
    _, prompt_feat, prompt_h, p = make_prompts(fenc, CASE1_PROMPTS)
    clean = run(tts, batch, prompt_feat, prompt_h, p, 4)["mel"].cpu()
    _, feat_nan, h_nan, p2 = make_prompts(fenc, CASE1_PROMPTS, P_feat=71, P_h=90, fill=float("nan"))
    assert torch.equal(p, p2) and feat_nan.shape == (4, 71, 80) and h_nan.shape == (4, 90, 80)
    assert torch.isnan(feat_nan[2]).all() and torch.isnan(h_nan[0, 30:]).all()
    for b in range(4):
        assert torch.equal(feat_nan[b, :p[b]], prompt_feat[b, :p[b]]) and torch.equal(h_nan[b, :p[b]], prompt_h[b, :p[b]])
    dirty = run(tts, batch, feat_nan, h_nan, p, 4)["mel"].cpu()
    assert torch.isfinite(dirty).all()
    assert torch.equal(dirty, clean), md(dirty, clean)


def test_prompted_compact_geometry_equals_uniform(fenc, monkeypatch):
    """5. a prompted ragged batch in the compact geometry and with JV_NO_COMPACT=1 (the switch
    test_compact_geometry_equals_uniform uses): equal bit for bit"""
    from jyutvoice_amd import synth
    sd = synth.tts_state_dict(fixed_duration=1.5)
    batch = synth.batch(12, 150, first_index=5, lengths=LENGTHS12)
    _, prompt_feat, prompt_h, p = make_prompts(fenc, PROMPT_TOKENS12)

    def go():
        r = run(new_tts(sd), batch, prompt_feat, prompt_h, p, 2)
        return r["mel"].cpu(), r["mel_lengths"].cpu()

    compact, lc = go()
    monkeypatch.setenv("JV_NO_COMPACT", "1")
    uniform, lu = go()
    assert torch.isfinite(compact).all() and torch.equal(lc, lu)
    assert torch.equal(compact, uniform), md(compact, uniform)


def test_errors_are_raised_on_the_host_and_leave_the_context_usable(fenc, tts_sd):
    """6. bad prompt_lengths / streaming are rejected before any launch; a correct call afterwards passes"""
    from jyutvoice_amd import synth
    from jyutvoice_amd._lib import JvError
    from jyutvoice_amd.runtime import get_runtime
    tts = new_tts(tts_sd)
    batch = synth.batch(4, 40, lengths=CASE1_TOKENS)
    _, prompt_feat, prompt_h, p = make_prompts(fenc, CASE1_PROMPTS, P_feat=70, P_h=66)
    good = run(tts, batch, prompt_feat, prompt_h, p, 2)["mel"].cpu()

    def bad(lengths, exc, match, **kw):
        with pytest.raises(exc, match=match):
            tts.synthesise(*[batch[k] for k in KEYS], prompt_feat, prompt_h=prompt_h, n_timesteps=2, batched=True,
                           prompt_lengths=lengths, **kw)

    bad(torch.tensor([30, 67, 0, 44]), ValueError, "utterance 1")            # > min(P, P') = 66 although P = 70
    bad(torch.tensor([30, 66, -1, 44]), ValueError, "utterance 2")
    bad(torch.tensor([30, 66, 0]), ValueError, "shape")
    bad(torch.tensor([[30, 66, 0, 44]]), ValueError, "shape")
    bad(torch.tensor([30.0, 66.0, 0.0, 44.0]), ValueError, "int")
    bad([30, 66, 0, 44], ValueError, "tensor")
    bad(p, NotImplementedError, "streaming", streaming=True)
    with pytest.raises(ValueError, match="prompt_feat"):
        tts.synthesise(*[batch[k] for k in KEYS], None, prompt_h=prompt_h, n_timesteps=2, batched=True, prompt_lengths=p)
    # the library validates for itself (a caller of the C ABI has no Python in front of it): the utterance is named
    eng = get_runtime("cuda:0").ensure(4, 256, 40)
    mu_y = torch.zeros(4, 80, 50, device="cuda:0")
    spks = torch.zeros(4, 80, device="cuda:0")
    y = torch.tensor([50, 40, 30, 20])
    with pytest.raises(JvError, match="utterance 1"):
        eng.cfm_solve_prompted(mu_y, y, prompt_h, prompt_feat, torch.tensor([30, 67, 0, 44]), spks, 2)
    with pytest.raises(JvError, match="utterance 3"):
        eng.cfm_solve_prompted(mu_y, torch.tensor([50, 40, 30, 51]), prompt_h, prompt_feat, p, spks, 2)
    again = run(tts, batch, prompt_feat, prompt_h, p, 2)["mel"].cpu()
    assert torch.equal(again, good)


def test_ragged_mel_equals_singles():
    """7. three recordings of 1.0 / 2.37 / 0.5 s in one [3, n] buffer, NaN behind each: per recording bit-identical to the
    single call on its own samples and <= 2e-4 from the oracle (test_prompt_mel_golden's bound for its batch case); zero
    behind T_b"""
    from jyutvoice_amd._lib import JvError
    from jyutvoice_amd.runtime import get_runtime
    from jyutvoice_amd.utils.audio import extract_speech_feat, extract_speech_feat_batch, mel_spectrogram
    from oracle import audio as oaudio
    ns = [24000, int(2.37 * 24000), 12000]
    gen = torch.Generator().manual_seed(11)
    wavs = [(torch.randn(1, n, generator=gen) * 0.2).clamp(-1, 1) for n in ns]
    buf = torch.full((3, max(ns)), float("nan"))
    for b, w in enumerate(wavs):
        buf[b, :ns[b]] = w[0]
    singles = [mel_spectrogram(w) for w in wavs]          # (also loads the mel filterbank into the context)
    eng = get_runtime("cuda:0").ensure(1, 64, 1)
    mel, mel_lens = eng.mel_spectrogram(buf, torch.tensor(ns))
    T = [1 + (n - 480) // 480 for n in ns]
    assert T == [50, 118, 25]
    assert mel_lens.dtype == torch.int32 and mel_lens.cpu().tolist() == T and mel.shape == (3, 80, max(T))
    basis = oaudio.mel_basis_slaney()
    for b in range(3):
        assert singles[b].shape == (1, 80, T[b])
        assert torch.equal(mel[b, :, :T[b]], singles[b][0]), (b, md(mel[b, :, :T[b]], singles[b][0]))
        err = md(mel[b, :, :T[b]], oaudio.mel_spectrogram(wavs[b], basis)[0])
        print(f"recording {b}: {ns[b]} samples, {T[b]} frames, max-abs vs oracle {err:.3e}")
        assert err <= 2e-4, (b, err)
        assert float(mel[b, :, T[b]:].abs().sum()) == 0.0
    feat, n = extract_speech_feat_batch(wavs)
    assert feat.shape == (3, max(T), 80) and n.cpu().tolist() == T
    assert torch.equal(feat[1, :T[1]], extract_speech_feat(wavs[1])[0][0])
    with pytest.raises(JvError, match="recording 2"):
        eng.mel_spectrogram(buf, torch.tensor([24000, 30000, 720]))
    with pytest.raises(JvError, match="recording 0"):
        eng.mel_spectrogram(buf, torch.tensor([max(ns) + 1, 30000, 12000]))
    mel2, _ = eng.mel_spectrogram(buf, torch.tensor(ns))
    assert torch.equal(mel2, mel)


def _write_wav16(path, wav):
    pcm = (wav.flatten().clamp(-1, 1) * 32767.0).round().to(torch.int16).numpy().tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(pcm)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, 24000, 48000, 2, 16) +
                b"data" + struct.pack("<I", len(pcm)))
        f.write(pcm)


def _read_pcm(path):
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and data[36:40] == b"data"
    return torch.frombuffer(bytearray(data[44:]), dtype=torch.int16)


def test_cli_list_of_cloning_requests(tmp_path, prompt_sd, capsys):
    """8. infer.py --tokens list.json: three utterances, each with its own prompt recording of its own duration, as one batch.
    Three wavs of y_b x 480 samples.  Utterance 1's recording (2.0 s = 100 frames) is shorter than its 2 x 60 prompt-token
    frames: the CLI trims both to 100 and says so.

    The first wav against the same CLI on a one-element list holding that utterance, same --seed: SAMPLE-IDENTICAL (measured on
    the MI355X: 0 LSB difference over all samples).  Why it can be: the vocoder's seeded noise is a function of (seed, call,
    utterance index, sample) and utterance 0's phase draw is the first row of the batch's draw, so neither depends on the
    batch around utterance 0; and at this size (3 utterances of < 200 frames) the batch and the single request run the same
    short-M kernels, inside which an utterance's result does not depend on what else is in the batch.  A
    batch large enough to change the kernel regime against its B = 1 run differs from it in the mel's last bits (<= 2e-5, test 3)."""
    import infer
    from jyutvoice_amd import synth
    from jyutvoice_amd.flow.encoder import extract_flow_weights
    tts_sd = synth.tts_state_dict()
    flow_pt = dict(prompt_sd)
    enc_part, _ = extract_flow_weights(flow_pt)
    torch.save(enc_part, tmp_path / "flow_encoder.pt")
    torch.save({"state_dict": tts_sd}, tmp_path / "tts.ckpt")
    torch.save(synth.hift_state_dict(), tmp_path / "hift.pt")
    gen = torch.Generator().manual_seed(5)
    durations, ptoks, ntok = [1.2, 2.0, 0.9], [30, 60, 20], [12, 15, 8]      # 60 / 100 / 45 mel frames vs 60 / 120 / 40 from tokens
    utts = []
    for b in range(3):
        wav = (torch.randn(int(durations[b] * 24000), generator=gen) * 0.1).clamp(-1, 1)
        _write_wav16(tmp_path / f"ref{b}.wav", wav)
        u = synth.batch(1, ntok[b], first_index=b)
        tok, _ = synth.prompt_tokens(1, ptoks[b], first_index=b)
        obj = {k: u[k][0].tolist() for k in ("x", "lang", "tone", "word_pos", "syllable_pos")}
        obj["interspersed"] = False      # raw id lists: the CLI puts the blanks in (2 n + 1 tokens)
        obj.update(spk_embed=u["spk_embed"][0].tolist(), prompt_token=tok[0].tolist(), prompt_wav_24k=str(tmp_path / f"ref{b}.wav"))
        utts.append(obj)
    json.dump(utts, open(tmp_path / "list.json", "w"))
    json.dump(utts[:1], open(tmp_path / "one.json", "w"))
    common = ["--tts_checkpoint", str(tmp_path / "tts.ckpt"), "--hift", str(tmp_path / "hift.pt"), "--flow_encoder",
              str(tmp_path / "flow_encoder.pt"), "--n_timesteps", "2", "--seed", "7"]
    infer.main(["--output", str(tmp_path / "out.wav"), "--tokens", str(tmp_path / "list.json")] + common)
    said = capsys.readouterr().out
    assert "utterance 1: prompt_h has 120 frames, the prompt mel 100: both trimmed to 100" in said
    assert "utterance 2: prompt_h has 40 frames, the prompt mel 45: both trimmed to 40" in said
    assert "utterance 0:" not in said
    infer.main(["--output", str(tmp_path / "solo.wav"), "--tokens", str(tmp_path / "one.json")] + common)
    # y_b from the library itself: the same three utterances, unprompted lengths do not depend on the prompt
    tts = new_tts(tts_sd)
    from jyutvoice_amd.utils.text import load_tokens_json
    ids = [load_tokens_json(u) for u in utts]
    xl = torch.cat([i["x_lengths"] for i in ids])
    assert xl.tolist() == [25, 31, 17]
    batch = {k: torch.zeros(3, 31, dtype=torch.int64) for k in KEYS[:1] + KEYS[2:6]}
    for b, i in enumerate(ids):
        for k in batch:
            batch[k][b, :int(xl[b])] = i[k][0]
    spk = torch.tensor([u["spk_embed"] for u in utts])
    y = tts.synthesise(batch["x"], xl, batch["lang"], batch["tone"], batch["word_pos"], batch["syllable_pos"], spk, None,
                       n_timesteps=2, length_scale=0.9, batched=True)["mel_lengths"].cpu().tolist()
    pcm = [_read_pcm(tmp_path / f"out_{b:03d}.wav") for b in range(3)]
    assert [t.numel() for t in pcm] == [480 * n for n in y]
    assert not (tmp_path / "out.wav").exists() and not (tmp_path / "out_003.wav").exists()
    solo = _read_pcm(tmp_path / "solo_000.wav")
    assert solo.numel() == pcm[0].numel()
    diff = int((solo.int() - pcm[0].int()).abs().max())
    print(f"utterance 0, batch of 3 vs one-element list: max |PCM difference| = {diff} LSB, identical samples: "
          f"{float((solo == pcm[0]).float().mean()):.4f}")
    assert diff == 0
    assert int(pcm[0].int().abs().max()) > 100      # (not silence)
