"""GPU: concurrent streaming sessions -- jv_flow_encoder_fwd_ctx / jv_flow_token2mel_ctx (a look-ahead context per utterance),
jv_hift_source_cont_rows (a source signal per row), jv_slab_copy, `HiFTStreamBatch` and `Token2WavServer`.

What is bit-exact is asserted with torch.equal: a row of the source continuation against jv_hift_source_cont at B = 1, a slab copy
against the slicing it replaces, NaN / garbage behind a length against the clean run, the assembled source of a served session against
jv_hift_source_seeded on its own f0 record.  What runs the same arithmetic in another batch geometry takes the bounds the project
already holds that property to: 2e-5 for the mel of a batch row against its single-utterance run (test_gpu_prompt_batch.py,
test_gpu_stream.py), 5e-5 for the encoder against the imported reference modules (G16, recorded as G15 was), 8 x 4.7e-5 Hz for an f0
record (test_gpu_stream.py), and for waveforms rms <= min(8 x floor, 5e-5) against the fp64 oracle's decode of the session's own
(mel, source), floor = rms(fp32 oracle - fp64 oracle), clamped share <= 1 %.  Figures go to parity_stream_batch.json (JV_OUT)."""
import os

import pytest
import torch

import parity_util as pu
import stream_batch_cases as sb
import stream_ref as sr
import token2mel_cases as tc
from conftest import load_golden

pytestmark = pytest.mark.gpu

RATIO, OUTER, MEL_BOUND, ENC_BOUND, F0_BOUND = 8.0, 5e-5, 2e-5, 5e-5, 8 * 4.7e-5
record = pu.Recorder("parity_stream_batch.json",
                     {"mel bound": "a batch row against inference_partial / inference at B = 1, and a served session's mel pieces against its "
                                   "Token2WavStream's: 2e-5",
                      "encoder bound": "jv_flow_encoder_fwd_ctx rows against G16 (imported reference modules at B = 1): 5e-5",
                      "f0 bound": "served f0 record against the Token2WavStream's: 8 x 4.7e-5 Hz",
                      "waveform bound": "rms(served wav - fp64 oracle on the session's mel and source) <= 8 x floor and <= 5e-5; floor = "
                                        "rms(fp32 oracle - fp64 oracle); clamped share of the fp64 reference <= 1 %"})


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    torch.set_num_threads(min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def hift(hift_sd):
    import jyutvoice_amd
    h = jyutvoice_amd.build_default("cuda:0")[1]
    h.load_state_dict(hift_sd)
    return h


@pytest.fixture(scope="module")
def eng(hift):
    return hift._engine(3, 192)


@pytest.fixture(scope="module")
def flow(prompt_sd, tts_sd):
    from jyutvoice_amd.flow.flow import CausalMaskedDiffWithXvec
    from jyutvoice_amd.runtime import Runtime
    m = CausalMaskedDiffWithXvec(vocab_size=6561, input_frame_rate=25, runtime=Runtime("cuda:0"))
    m.load_state_dict(tc.flow_sd(prompt_sd, tts_sd))
    return m


# ---- 1. a look-ahead context per utterance ---------------------------------------------------------------------------------------------
def mixed_batch(poison=False):
    """the fourth step of the timeline as one padded batch: a (53 tokens, final: ctx 0), b (10 + 68, ctx 3), c (7 + 21, ctx 3).
    poison: garbage ids behind every token length, NaN behind every prompt_feat length and in the pad columns"""
    rows = [(name, solve, ctx) for name, solve, ctx, _, _ in sb.ROWS[3]]
    P = max(sb.SESSIONS[n][0] for n, _, _ in rows)
    F = max(sb.SESSIONS[n][1] for n, _, _ in rows)
    N = max(solve - sb.SESSIONS[n][0] for n, solve, _ in rows)
    tok = torch.full((3, N), -7 if poison else 0, dtype=torch.int64)
    ptok = torch.full((3, P), 6560 if poison else 0, dtype=torch.int64)
    feat = torch.full((3, F, 80), float("nan") if poison else 0.0)
    emb = torch.zeros(3, 192)
    for b, (name, solve, ctx) in enumerate(rows):
        p, f = sb.SESSIONS[name][:2]
        t, pt, ft, e = sb.inputs(name)
        tok[b, :solve - p], ptok[b, :p], feat[b, :f], emb[b] = t[0, :solve - p], pt[0], ft[0], e[0]
    lens = (torch.tensor([solve - sb.SESSIONS[n][0] for n, solve, _ in rows]), torch.tensor([sb.SESSIONS[n][0] for n, _, _ in rows]),
            torch.tensor([sb.SESSIONS[n][1] for n, _, _ in rows]))
    return rows, tok, ptok, feat, emb, lens, [c for _, _, c in rows]


@pytest.fixture(scope="module")
def mixed_mel(flow):
    """the mixed batch through inference_partial_batch: computed once, shared, not modified"""
    rows, tok, ptok, feat, emb, (n, p, f), ctx = mixed_batch()
    mel, lens = flow.inference_partial_batch(tok, n, ptok, p, feat, f, emb, ctx, streaming=True, n_timesteps=sb.N_TIMESTEPS)
    return mel, lens


def test_ctx_batch_rows_against_single_utterance_runs(flow, mixed_mel):
    """row b of the batch = inference_partial (ctx 3) or inference(finalize=True) (ctx 0) on utterance b alone, to 2e-5; zeros behind"""
    rows = mixed_batch()[0]
    mel, lens = mixed_mel
    want_lens = [2 * (solve - ctx) - sb.SESSIONS[n][1] for n, solve, ctx in rows]
    assert lens.tolist() == want_lens == [106, 130, 36] and mel.shape == (3, 80, 130) and mel.dtype == torch.float32
    failures = []
    for b, (name, solve, ctx) in enumerate(rows):
        P, F = sb.SESSIONS[name][:2]
        tok, ptok, feat, emb = sb.inputs(name)
        args = (tok[:, :solve - P], torch.tensor([solve - P]), ptok if P else None, torch.tensor([P]), feat if F else None,
                torch.tensor([F]), emb, True)
        if ctx:
            one, _ = flow.inference_partial(*args, n_timesteps=sb.N_TIMESTEPS)
        else:
            one, _ = flow.inference(*args, True, n_timesteps=sb.N_TIMESTEPS)
        y = want_lens[b]
        assert one.shape == (1, 80, y)
        e = pu.md(mel[b:b + 1, :, :y], one)
        record(f"ctx batch row {name} (ctx {ctx})", mel_vs_single=e, exact=float(e == 0.0))
        if e > MEL_BOUND:
            failures.append((name, e))
        if y < mel.shape[2]:
            assert float(mel[b, :, y:].abs().max()) == 0.0
    assert not failures, failures


def test_ctx_batch_reads_nothing_behind_a_length(flow, mixed_mel):
    """garbage token ids behind every token length, NaN behind every prompt_feat length and in the pad columns: the same bits"""
    _, tok, ptok, feat, emb, (n, p, f), ctx = mixed_batch(poison=True)
    mel, lens = flow.inference_partial_batch(tok, n, ptok, p, feat, f, emb, ctx, streaming=True, n_timesteps=sb.N_TIMESTEPS)
    assert torch.isfinite(mel).all()
    assert torch.equal(mel, mixed_mel[0]) and torch.equal(lens, mixed_mel[1])


def test_ctx_encoder_against_reference(flow):
    """jv_flow_encoder_fwd_ctx on the mixed batch against the imported reference modules at B = 1 (G16): 5e-5, zeros behind 2 L_b"""
    from jyutvoice_amd._lib import JvError
    g = load_golden("G16_flow_ctx_batch")
    rows, tok, ptok, _, _, (n, p, _), ctx = mixed_batch()
    e = flow._rt().ensure(3, 256, 1)
    h, hl = e.flow_encoder_ctx(ptok, p, tok, n, torch.tensor(ctx, dtype=torch.int32), streaming=True)
    assert h.shape == (3, 2 * (ptok.shape[1] + tok.shape[1]), 80) and hl.tolist() == [106, 150, 50]
    failures = []
    for b, (name, solve, c) in enumerate(rows):
        P = sb.SESSIONS[name][0]
        ids = torch.cat([ptok[b, :P], tok[b, :solve - P]])
        assert torch.equal(ids, g["ids_" + name][0])      # (the fixture was recorded on these ids)
        L2 = 2 * (solve - c)
        err = pu.md(h[b:b + 1, :L2], g["h_" + name])
        record(f"G16 {name} (ctx {c})", encoder=err)
        if err > ENC_BOUND:
            failures.append((name, err))
        assert float(h[b, L2:].abs().max()) == 0.0
    assert not failures, failures
    # the context is read: the same rows with ctx = 0 on the shortened sequences land elsewhere
    hz, _ = e.flow_encoder_ctx(ptok, p, tok, n - torch.tensor(ctx), torch.zeros(3, dtype=torch.int32), streaming=True)
    assert pu.md(hz[1:2, :150], g["h_b"]) > 1e-2 and pu.md(hz[0:1, :106], g["h_a"]) <= ENC_BOUND
    # the library's own check, before anything is launched on the lengths
    with pytest.raises(JvError, match="utterance 1: context 2"):
        e.flow_encoder_ctx(ptok, p, tok, n, torch.tensor([0, 2, 3], dtype=torch.int32), streaming=True)
    with pytest.raises(JvError, match="utterance 2: 3 tokens with a context of 3"):
        e.flow_encoder_ctx(None, None, tok, torch.tensor([5, 5, 3]), torch.tensor([3, 0, 3], dtype=torch.int32), streaming=True)
    with pytest.raises(JvError, match="utterance 0: context -3"):
        e.flow_token2mel_ctx(None, None, tok, n, torch.tensor([-3, 0, 3], dtype=torch.int32), None, torch.zeros(3, dtype=torch.int32),
                             torch.zeros(3, 192), streaming=True, n_timesteps=2)


# ---- 2. a source signal per row --------------------------------------------------------------------------------------------------------
def i64(v):
    v &= 2 ** 64 - 1
    return v - 2 ** 64 if v >= 2 ** 63 else v


def i32(v):
    v &= 2 ** 32 - 1
    return v - 2 ** 32 if v >= 2 ** 31 else v


def test_source_rows_equal_single_row_continuations(eng):
    """three rows with their own (seed, call, sample0, frames): (11, 0, 25) frames at samples 0, 480 x 37, 480 x 111, one seed with its
    top bit set, one call of 2^32 - 1; unvoiced frames and a near-zero one (the frame scan's sequential path) in rows 0 and 2"""
    f0c, phc = sr.f0_case()
    g = torch.Generator().manual_seed(93)
    f0 = torch.stack([f0c[0, 5:30], f0c[1, :25], f0c[1, 12:37]]).cuda()
    phase = torch.cat([phc, (torch.rand(1, 9, generator=g) * 2 - 1) * 3.14159]).cuda()
    seeds, calls = [0x1234567890ABCDEF, 5, 0xF234567890ABCDEF], [7, 0, 0xFFFFFFFF]
    frames0, lens = [0, 37, 111], [11, 0, 25]
    before = (80.0 + 200.0 * torch.rand(111, generator=g)).cuda()
    cum0, want_s, want_cum = [], [], []
    for b in range(3):
        cum = torch.zeros(1, 9, dtype=torch.float64, device="cuda")
        if frames0[b]:      # the sums a signal has after its first frames0[b] frames
            eng.hift_source_cont(before[None, :frames0[b]], phase[b:b + 1], seeds[b], calls[b], 0, cum)
        cum0.append(cum.clone())
        if lens[b]:
            want_s.append(eng.hift_source_cont(f0[b:b + 1, :lens[b]], phase[b:b + 1], seeds[b], calls[b], 480 * frames0[b], cum))
        else:
            want_s.append(None)
        want_cum.append(cum)

    def run(order):
        cum = torch.cat([cum0[b] for b in order])
        out = torch.full((3, 1, 480 * 25), 7.0, device="cuda")
        s = eng.hift_source_cont_rows(f0[order], phase[order], torch.tensor([i64(seeds[b]) for b in order]).cuda(),
                                      torch.tensor([i32(calls[b]) for b in order], dtype=torch.int32).cuda(),
                                      torch.tensor([480 * frames0[b] for b in order]).cuda(),
                                      torch.tensor([lens[b] for b in order], dtype=torch.int32).cuda(), cum, out=out)
        assert s is out
        return s, cum

    for order in ([0, 1, 2], [2, 1, 0]):      # whichever slot a row sits in
        s, cum = run(order)
        for slot, b in enumerate(order):
            if lens[b] == 0:      # not touched: neither the samples nor the sums
                assert float((s[slot] - 7.0).abs().max()) == 0.0 and torch.equal(cum[slot:slot + 1], cum0[b])
                continue
            n = 480 * lens[b]
            assert torch.equal(s[slot:slot + 1, :, :n], want_s[b]), (order, b, pu.md(s[slot:slot + 1, :, :n], want_s[b]))
            if lens[b] < 25:
                assert float(s[slot, :, n:].abs().max()) == 0.0
            assert torch.equal(cum[slot:slot + 1], want_cum[b]), (order, b)
            assert not torch.equal(cum[slot:slot + 1], cum0[b])
    with pytest.raises(ValueError, match="seeds must be a contiguous torch.int64"):
        eng.hift_source_cont_rows(f0, phase, torch.zeros(3).cuda(), torch.zeros(3, dtype=torch.int32).cuda(), torch.zeros(3, dtype=torch.int64).cuda(),
                                  torch.zeros(3, dtype=torch.int32).cuda(), torch.zeros(3, 9, dtype=torch.float64).cuda())


# ---- 3. slab copy ------------------------------------------------------------------------------------------------------------------------
OFFS, LENS = (0, 1, 3, 481), (0, 1, 959)


def slab_desc(rows):
    return torch.tensor(rows, dtype=torch.int32).cuda()


@pytest.mark.parametrize("C,shift", [(5, 0), (1, 0), (5, 1)])
def test_slab_copy_equals_slicing(eng, C, shift):
    """gather (into column 0, zero-filled to the span), append (at a column offset) and crop (both offsets) at column offsets 0, 1, 3,
    481 and lengths 0, 1, 959; shift = 1: both buffers start 4 bytes off a 16-byte boundary (every access a dword)"""
    g = torch.Generator().manual_seed(481)
    W, span = 1500, 960
    combos = [(o, n) for o in OFFS for n in LENS]

    def buf(rows, fill=None):
        flat = torch.randn(rows * C * W + 4, generator=g).cuda() if fill is None else torch.full((rows * C * W + 4,), fill, device="cuda")
        return flat[shift:shift + rows * C * W].view(rows, C, W)

    src = buf(3)
    assert src.data_ptr() % 16 == 4 * shift and src.is_contiguous()
    # gather: src[r % 3, :, o:o + n] -> dst[i, :, :n], zeros up to the span, nothing behind it
    dst = buf(len(combos), fill=9.0)
    eng.slab_copy(src, dst, slab_desc([(i % 3, o, i, 0, n) for i, (o, n) in enumerate(combos)]), span, zero_fill=True)
    for i, (o, n) in enumerate(combos):
        want = torch.full((C, W), 9.0, device="cuda")
        want[:, :span] = 0.0
        want[:, :n] = src[i % 3, :, o:o + n]
        assert torch.equal(dst[i], want), ("gather", o, n)
    # append: src[r, :, :n] -> dst[i, :, o:o + n], nothing else
    dst = buf(len(combos), fill=9.0)
    eng.slab_copy(src, dst, slab_desc([(i % 3, 0, i, o, n) for i, (o, n) in enumerate(combos)]), span)
    for i, (o, n) in enumerate(combos):
        want = torch.full((C, W), 9.0, device="cuda")
        want[:, o:o + n] = src[i % 3, :, :n]
        assert torch.equal(dst[i], want), ("append", o, n)
    # crop: src[r, :, o:o + n] -> dst[i, :, o2:o2 + n] with the other offsets, zero-filled up to the span or the buffer's end
    dst = buf(len(combos), fill=9.0)
    pairs = [(o, OFFS[::-1][OFFS.index(o)], n) for o, n in combos]
    wide = 1100      # (481 + 1100 > 1500: the fill is cut at the destination's width)
    eng.slab_copy(src, dst, slab_desc([(i % 3, o, i, o2, n) for i, (o, o2, n) in enumerate(pairs)]), wide, zero_fill=True)
    for i, (o, o2, n) in enumerate(pairs):
        want = torch.full((C, W), 9.0, device="cuda")
        want[:, o2:o2 + wide] = 0.0
        want[:, o2:o2 + n] = src[i % 3, :, o:o + n]
        assert torch.equal(dst[i], want), ("crop", o, o2, n)
    # descriptors that do not fit move nothing: rows and columns outside either buffer, n < 0, n above the span
    dst = buf(2, fill=9.0)
    eng.slab_copy(src, dst, slab_desc([(3, 0, 0, 0, 4), (0, 0, 2, 0, 4), (0, W - 3, 0, 0, 4), (0, 0, 1, W - 3, 4), (0, 0, 0, 0, -1),
                                       (0, 0, 1, 0, 9), (-1, 0, 0, 0, 4), (0, -1, 0, 0, 4)]), 8, zero_fill=True)
    assert float((dst - 9.0).abs().max()) == 0.0
    if C == 1:      # the 2-D form
        d2 = torch.full((2, 700), 9.0, device="cuda")
        eng.slab_copy(src[:, 0], d2, slab_desc([(2, 481, 1, 3, 600)]), 600)
        assert torch.equal(d2[1, 3:603], src[2, 0, 481:1081]) and float((d2[0] - 9.0).abs().max()) == 0.0 and float(d2[1, 603:].min()) == 9.0
        with pytest.raises(ValueError, match="src has 1 channels, dst 5"):
            eng.slab_copy(src, torch.zeros(1, 5, 8, device="cuda"), slab_desc([(0, 0, 0, 0, 1)]), 1)


# ---- 4. the server against B = 1 sessions ---------------------------------------------------------------------------------------------
def new_server(flow, hift, sessions=sb.MAX_SESSIONS):
    from jyutvoice_amd.stream import Token2WavServer
    return Token2WavServer(flow, hift, max_sessions=sessions, max_tokens=sb.MAX_TOKENS, n_timesteps=sb.N_TIMESTEPS,
                           max_prompt_tokens=sb.MAX_PROMPT)


@pytest.fixture(scope="module")
def served(flow, hift):
    """the timeline through one server, the records of every session taken when it finishes (a's slot goes to d): computed once"""
    server = new_server(flow, hift)
    caps = (flow._rt().caps, hift._engine(1, 1).max_frames)
    rec, slots = {}, {}

    def on_step(i, got, sids):
        for name, sid in sids.items():
            session = server._sessions.get(sid)
            if session is not None and session.finished and name not in rec:
                phase, seed, call = server.source_draws(sid)
                rec[name] = dict(mel=server.mel(sid).clone(), source=server.source(sid).clone(), f0=server.f0(sid).clone(),
                                 phase=phase.clone(), seed=seed, call=call)
                slots[name] = session.slot

    wavs, _ = sb.play_server(server, on_step=on_step)
    assert (flow._rt().caps, hift._engine(1, 1).max_frames) == caps      # no step rebuilt a context
    return wavs, rec, slots


@pytest.fixture(scope="module")
def singles(flow, hift):
    """every session alone through a Token2WavStream with the same seed and pushes: computed once"""
    return {name: sb.play_single(flow, hift, name) for name in sb.SESSIONS}


def test_server_slots_and_sample_counts(served, singles):
    wavs, rec, slots = served
    assert sorted(rec) == ["a", "b", "c", "d"]
    assert slots["d"] == slots["a"] and len({slots["a"], slots["b"], slots["c"]}) == 3      # d took the slot a left
    for name, (session, want) in singles.items():
        got = [(i, w.shape[1]) for i, w in wavs[name] if w.shape[1]]
        assert got == [(i, w.shape[1]) for i, w in want], name
        P, F, N, _ = sb.SESSIONS[name]
        frames = 2 * (P + N) - F
        assert sum(n for _, n in got) == 480 * frames and rec[name]["mel"].shape == (1, 80, frames)
        assert rec[name]["source"].shape == (1, 1, 480 * frames) and rec[name]["f0"].shape == (1, frames)
        for _, w in wavs[name]:
            assert w.shape[0] == 1 and w.shape[1] % 480 == 0 and torch.isfinite(w).all()


@pytest.mark.parametrize("name", sorted(sb.SESSIONS))
def test_server_session_against_single_session(served, singles, eng, name):
    """mel pieces to 2e-5, the f0 record to 8 x 4.7e-5 Hz, the source bit for bit the one-shot source of the session's own f0 record"""
    wavs, rec, _ = served
    session, _ = singles[name]
    r = rec[name]
    e_mel = pu.md(r["mel"], session.mel)
    e_f0 = pu.md(r["f0"], session.vocoder.f0)
    e_wav = pu.rms(torch.cat([w for _, w in wavs[name]], dim=1), torch.cat([w for _, w in singles[name][1]], dim=1))
    record(f"server {name}", mel_vs_single=e_mel, f0_vs_single=e_f0, wav_rms_vs_single=e_wav)
    assert (r["seed"], r["call"]) == (session.vocoder._seed, session.vocoder._call) and torch.equal(r["phase"], session.vocoder._phase)
    assert e_mel <= MEL_BOUND, (name, e_mel)
    assert e_f0 <= F0_BOUND, (name, e_f0)
    assert torch.equal(r["source"], eng.hift_source_seeded(r["f0"], r["phase"], r["seed"], r["call"]))


@pytest.mark.parametrize("name", ["c", "d"])
def test_server_waveform_against_oracle(served, hift_sd, name):
    """the served waveform against the fp64 oracle's decode of (the session's mel, its assembled source)"""
    wavs, rec, _ = served
    w32, w64 = pu.hift_folded(hift_sd)
    mel, s = rec[name]["mel"].cpu(), rec[name]["source"].cpu()
    T = mel.shape[2]
    wav = torch.cat([w for _, w in wavs[name]], dim=1).cpu()
    r64, r32 = pu.hift_fp64(w64, mel, s, T), pu.hift_fp32(w32, mel, s, T)
    share, floor, err = pu.clamp_share(r64), pu.rms(r32, r64), pu.rms(wav, r64)
    record(f"server {name} waveform", clamped_share=share, floor=floor, error=err, ratio=err / floor)
    assert share <= pu.CLAMP_CAP, (name, share)
    assert 0.0 < floor < OUTER, (name, floor)
    assert err <= RATIO * floor and err <= OUTER, f"{name}: rms {err:.3e} = {err / floor:.2f} x the oracle's own {floor:.3e}"


def test_server_session_does_not_depend_on_its_neighbours(flow, hift, served, singles):
    """the longest session alone in a server against the same session served beside the others: the bounds of a session against its
    B = 1 run hold between the two"""
    wavs, rec, _ = served
    server = new_server(flow, hift)
    alone, sids = sb.play_server(server, only=("b",))
    sid = sids["b"]
    mel, f0, src = server.mel(sid), server.f0(sid), server.source(sid)
    e_mel, e_f0 = pu.md(mel, rec["b"]["mel"]), pu.md(f0, rec["b"]["f0"])
    record("server b alone vs mixed", mel=e_mel, f0=e_f0, exact=float(e_mel == 0.0))
    assert [(i, w.shape[1]) for i, w in alone["b"]] == [(i, w.shape[1]) for i, w in wavs["b"]]
    assert e_mel <= MEL_BOUND and e_f0 <= F0_BOUND
    phase, seed, call = server.source_draws(sid)
    assert (seed, call) == (rec["b"]["seed"], rec["b"]["call"]) and torch.equal(phase, rec["b"]["phase"])
    assert src.shape == rec["b"]["source"].shape


# ---- 5. capacity -------------------------------------------------------------------------------------------------------------------------
def test_server_capacity(flow, hift):
    """max_sessions + 1 opens raise; a step at full slots with max_tokens reached runs without a context rebuild"""
    from jyutvoice_amd.stream import Token2WavServer
    server = Token2WavServer(flow, hift, max_sessions=2, max_tokens=28, n_timesteps=2, max_prompt_tokens=7)
    caps = (flow._rt().caps, hift._engine(1, 1).max_frames)
    tok, ptok, feat, emb = sb.inputs("c")
    s0 = server.open(ptok, feat, emb, seed=1)
    s1 = server.open(None, None, emb, seed=2)
    with pytest.raises(RuntimeError, match="all 2 sessions are taken"):
        server.open(None, None, emb)
    server.push(s0, tok[0, :28])
    server.push(s1, tok[0, :28])
    with pytest.raises(ValueError, match="28 \\+ 1 tokens exceed the session's max_tokens = 28"):
        server.push(s1, tok[0, :1])
    out = server.step()      # 7 + 28 and 28 tokens: both solve 25 + 3
    assert sorted(out) == [s0, s1] and out[s0].shape == (1, 480 * (36 - 21)) and out[s1].shape == (1, 480 * (50 - 21))
    assert server.step() == {}
    server.close(s0)
    server.close(s1)
    out = server.step()
    assert out[s0].shape == (1, 480 * (70 - 14 - 15)) and out[s1].shape == (1, 480 * (56 - 29))
    assert (flow._rt().caps, hift._engine(1, 1).max_frames) == caps
    # both slots are free again
    server.open(None, None, emb)
    server.open(None, None, emb)
    with pytest.raises(RuntimeError, match="all 2 sessions are taken"):
        server.open(None, None, emb)


# ---- 6. CLI --------------------------------------------------------------------------------------------------------------------------
def test_cli_stream_sessions(tmp_path):
    """infer.py --stream-hop K --stream-sessions S writes the files the per-request session route writes: three requests through two
    slots (the third takes the slot that frees first), the same lengths; the first two, whose draws the two routes take in the same
    order, to the waveform bound between two GPU decodes"""
    import json

    import infer
    from jyutvoice_amd.utils.audio import load_wav
    reqs = []
    for name, n in (("c", 40), ("b", 60), ("d", 30)):
        tok, ptok, feat, emb = sb.inputs(name)
        r = {"speech_token": tok[0, :n].tolist(), "embedding": emb[0].tolist()}
        if ptok.shape[1]:
            r.update(prompt_token=ptok[0].tolist(), prompt_feat=feat[0].tolist())
        reqs.append(r)
    (tmp_path / "list.json").write_text(json.dumps(reqs))
    base = ["--token2wav", str(tmp_path / "list.json"), "--synthetic", "1", "--n_timesteps", "2", "--streaming", "--stream-hop", "25"]
    infer.main(["--output", str(tmp_path / "a.wav")] + base)
    infer.main(["--output", str(tmp_path / "b.wav")] + base + ["--stream-sessions", "2"])
    for b, frames in enumerate([2 * 47 - 14, 2 * 70 - 20, 2 * 30]):
        one, rate = load_wav(str(tmp_path / f"a_{b:03d}.wav"))
        srv, rate2 = load_wav(str(tmp_path / f"b_{b:03d}.wav"))
        assert rate == rate2 == 24000 and one.shape[-1] == srv.shape[-1] == 480 * frames
        assert torch.isfinite(srv).all() and float(srv.abs().max()) > 1e-4
        if b < 2:
            d = pu.rms(one, srv)
            record(f"cli request {b}", server_vs_sessions=d)
            assert d <= OUTER, (b, d)
    with pytest.raises(SystemExit, match="--stream-sessions needs --stream-hop"):
        infer.main(["--output", str(tmp_path / "c.wav"), "--token2wav", str(tmp_path / "list.json"), "--synthetic", "1", "--stream-sessions", "2"])
