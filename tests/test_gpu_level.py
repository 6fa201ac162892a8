"""GPU: the level kernels (level.hip) -- jv_trim_bounds, jv_peak, jv_loudness, jv_level_gain, jv_level_apply -- against the fp64
restatements of tests/level_ref.py, up through `condition_prompt`, the CLI and `SynthServer`.

Trim bounds, peaks, the scaled samples and every length are exact.  The loudness bound is 8 floors, the floor being what a
sequential fp32 direct-form meter (level_ref.lufs32_seq) loses against the fp64 definition on the same input -- measured by that
reference, never by the kernel; test_level_host.py asserts the conditions on the inputs (no trim frame near its threshold, no block
near a gate) and shows what lands outside the bound.  Distance, floor and ratio per case go to parity_level.json."""
import json
import math

import numpy as np
import pytest
import torch

import level_ref as ref
from parity_util import Recorder

pytestmark = pytest.mark.gpu

NAN = float("nan")
ULP = 2.0 ** -23

REC = Recorder("parity_level.json", {
    "what": "jv_loudness against the fp64 restatement (tests/level_ref.py), per case",
    "bound": "8 x the largest floor over the rate's four-level cases; floor = |lufs32_seq - lufs64|, a sequential fp32 direct-form "
             "meter against the definition: measured by the reference, not by the kernel",
    "columns": "distance = |L_gpu - L_fp64| in LU, floor = that case's own floor (0 where the case has none), ratio = distance / "
               "the rate's bound (asserted <= 1)"})


@pytest.fixture(scope="module")
def eng():
    from jyutvoice_amd.runtime import get_runtime
    return get_runtime("cuda:0").ensure(1, 64, 1)


def ragged(xs, extra=5):
    """recordings as one padded batch with NaN behind every length"""
    lens = [len(x) for x in xs]
    buf = torch.full((len(xs), max(lens) + extra), NAN)
    for b, x in enumerate(xs):
        buf[b, : len(x)] = torch.from_numpy(np.asarray(x, dtype=np.float32))
    return buf, torch.tensor(lens, dtype=torch.int32)


def alone(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32))[None]


# ---- trim -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", range(-(-len(ref.TRIM_LEADS) // ref.TRIM_CHUNK)))
def test_trim_every_offset(eng, chunk):
    leads = list(ref.TRIM_LEADS)[chunk * ref.TRIM_CHUNK: (chunk + 1) * ref.TRIM_CHUNK]
    xs = [ref.trim_recording(l) for l in leads]
    buf, lens = ragged(xs)
    start, end = (v.cpu() for v in eng.trim_bounds(buf, lens, ref.TRIM_DB, ref.TRIM_F, ref.TRIM_H))
    for b, x in enumerate(xs):
        want = ref.trim64(x)[:2]
        assert (int(start[b]), int(end[b])) == want, (leads[b], int(start[b]), int(end[b]), want)
        s1, e1 = eng.trim_bounds(alone(x))
        assert (int(s1[0]), int(e1[0])) == want, leads[b]


def test_trim_edges(eng):
    from jyutvoice_amd._lib import JvError
    cases = ref.trim_edge_cases()
    for (F, H) in sorted({(F, H) for _, F, H in cases.values()}):
        names = [k for k, (_, f, h) in cases.items() if (f, h) == (F, H)]
        buf, lens = ragged([cases[k][0] for k in names])
        start, end = (v.cpu() for v in eng.trim_bounds(buf, lens, ref.TRIM_DB, F, H))
        for b, k in enumerate(names):
            want = ref.trim64(cases[k][0], ref.TRIM_DB, F, H)[:2]
            assert (int(start[b]), int(end[b])) == want, (k, int(start[b]), int(end[b]), want)
            if cases[k][0].size:
                s1, e1 = eng.trim_bounds(alone(cases[k][0]), None, ref.TRIM_DB, F, H)
                assert (int(s1[0]), int(e1[0])) == want, k
    # the library's own refusals (the wrapper's checks bypassed), each before anything is launched; the context stays usable
    from jyutvoice_amd.engine import _ptr, _stream
    x = alone(ref.trim_recording(1100)).cuda()
    s, e = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    for top_db, F, H in ((0.0, 440, 220), (-1.0, 440, 220), (math.inf, 440, 220), (NAN, 440, 220), (60.0, 0, 220), (60.0, 8193, 220),
                         (60.0, 440, 0)):
        rc = eng.lib.jv_trim_bounds(eng._h, _ptr(x), None, 1, x.shape[1], top_db, F, H, _ptr(s), _ptr(e), _stream(eng.device))
        assert rc == 1, (top_db, F, H)      # JV_ERR_ARG
    with pytest.raises(ValueError):
        eng.trim_bounds(x, top_db=0)
    got = eng.trim_bounds(x)
    assert (int(got[0][0]), int(got[1][0])) == ref.trim64(ref.trim_recording(1100))[:2]
    assert isinstance(JvError(1, "x"), RuntimeError)


# ---- peak -------------------------------------------------------------------------------------------------------------------------------
def test_peak_exact(eng):
    rng = np.random.default_rng(21)
    xs = [rng.standard_normal(n).astype(np.float32) for n in (1, 63, 4096, 4097, 9000, 20001)] + [np.zeros(0, np.float32)]
    buf, lens = ragged(xs)
    got = eng.peak(buf, lens).cpu()
    for b, x in enumerate(xs):
        assert float(got[b]) == ref.peak(x), b
        if x.size:
            assert float(eng.peak(alone(x))[0]) == ref.peak(x)
    starts = [0, 10, 4000, 4097, 8999, 5, 0]
    ends = [1, 10, 4100, 4000, 9000, 20001, 0]      # empty ranges: start == end and end < start (clamped up to start)
    got = eng.peak(buf, lens, torch.tensor(starts), torch.tensor(ends)).cpu()
    for b, x in enumerate(xs):
        assert float(got[b]) == ref.peak(x, starts[b], max(ends[b], starts[b])), b
    assert float(got[1]) == 0.0 and float(got[3]) == 0.0 and float(got[6]) == 0.0


# ---- loudness ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", ref.RATES)
def test_loudness_gates(eng, fs):
    cases = [ref.gate_case(fs, s) for s in ref.SEEDS]
    bound = ref.rate_bound(fs)
    buf, lens = ragged([c[0] for c in cases])
    got = eng.loudness(buf, fs, lens).cpu()
    for b, (x, L, _, floor) in enumerate(cases):
        dist = abs(float(got[b]) - L)
        REC(f"gates {fs} seed {ref.SEEDS[b]}", distance=dist, floor=floor, ratio=dist / bound)
        assert dist <= bound, (fs, ref.SEEDS[b], float(got[b]), L, dist, bound)
        one = eng.loudness(alone(x), fs).cpu()
        assert one[0].view(torch.int32) == got[b].view(torch.int32), (fs, b)      # the same bits alone


def test_loudness_lengths_and_seams(eng):
    fs, h = 24000, ref.hop(24000)
    bound = ref.rate_bound(fs)
    lens = ref.seam_lengths(fs)
    xs = [ref.one_level(n) for n in lens]
    buf, l = ragged(xs)
    got = eng.loudness(buf, fs, l).cpu()
    assert lens[0] == 4 * h - 1 and float(got[0]) == -math.inf
    for b, n in enumerate(lens[1:], 1):
        L = ref.lufs64(xs[b], fs)[0]
        dist = abs(float(got[b]) - L)
        REC(f"seam {n}", distance=dist, floor=0.0, ratio=dist / bound)
        assert dist <= bound, (n, float(got[b]), L)
        assert eng.loudness(alone(xs[b]), fs).cpu()[0].view(torch.int32) == got[b].view(torch.int32), n
    n = 3 * fs
    quiet = torch.stack([torch.zeros(n), torch.from_numpy(ref.one_level(n, sigma=1e-5))])
    got = eng.loudness(quiet, fs).cpu()
    assert float(got[0]) == -math.inf and float(got[1]) == -math.inf and not torch.isnan(got).any()
    with pytest.raises(ValueError):
        eng.loudness(quiet, 7999)
    from jyutvoice_amd.engine import _ptr, _stream
    q, out = quiet.cuda(), torch.zeros(2, device="cuda")
    for bad in (7999, 192001, 0):
        assert eng.lib.jv_loudness(eng._h, _ptr(q), None, 2, n, bad, _ptr(out), _stream(eng.device)) == 1      # JV_ERR_ARG


def test_loudness_calibration(eng):
    x = ref.sine997()
    L = ref.lufs64(x, 48000)[0]
    got = float(eng.loudness(alone(x), 48000)[0])
    bound = ref.rate_bound(48000)
    REC("calibration 997 Hz", distance=abs(got - L), floor=abs(ref.lufs32_seq(x, 48000) - L), ratio=abs(got - L) / bound)
    assert abs(L - -3.010) <= 1e-3 and abs(got - L) <= bound, (got, L)


# ---- gain and apply ---------------------------------------------------------------------------------------------------------------------
def test_gain_and_apply(eng):
    from jyutvoice_amd._lib import JvError
    fs = 24000
    cases = [ref.gate_case(fs, s) for s in ref.SEEDS[:2]]
    xs = [c[0] for c in cases] + [np.zeros(20000, np.float32), ref.one_level(5000)]      # ... one silent, one too short for a block
    buf, lens = ragged(xs)
    lufs, pk = eng.loudness(buf, fs, lens), eng.peak(buf, lens)
    assert float(lufs[2]) == -math.inf and float(lufs[3]) == -math.inf and float(pk[2]) == 0.0
    tol = math.log(10.0) / 20.0 * ref.rate_bound(fs) + 4 * ULP
    for target, ceiling in ((-23.0, None), (-16.0, 0.9), (-5.0, 0.5), (-40.0, 0.9)):
        gain = eng.level_gain(lufs, pk, target, ceiling).cpu()
        for b, x in enumerate(xs):
            L = ref.lufs64(x, fs)[0] if b < 2 else -math.inf
            want = ref.gain64(L, ref.peak(x), target, ceiling)
            assert abs(float(gain[b]) - want) <= tol * want, (target, ceiling, b, float(gain[b]), want)
        assert float(gain[2]) == 1.0 and float(gain[3]) == 1.0
        if ceiling == 0.5:      # 15 LU up would clip: the ceiling binds, and the scaled peak sits on it
            for b in range(2):
                assert abs(float(gain[b]) - ceiling / ref.peak(xs[b])) <= 4 * ULP * float(gain[b])
    # the prompt rule
    loud = [np.float32(3.0) * xs[0], xs[1], np.zeros(100, np.float32)]
    pbuf, plens = ragged(loud)
    ppk = eng.peak(pbuf, plens)
    g = eng.level_gain(None, ppk, ceiling=0.8).cpu()
    for b, x in enumerate(loud):
        want = ref.gain64(None, ref.peak(x), ceiling=0.8)
        assert abs(float(g[b]) - want) <= 4 * ULP * want, b
    assert float(g[0]) < 1.0 and float(g[1]) == 1.0 and float(g[2]) == 1.0
    # apply: bit for bit what torch computes with the kernel's own gain
    gain = eng.level_gain(lufs, pk, -16.0, 0.9)
    start, end = torch.tensor([0, 1000, 5, 4000], dtype=torch.int32), torch.tensor([30000, 20000, 5, 5000], dtype=torch.int32)
    for s, e in ((None, None), (start, end)):
        for tail in (0, 4800):
            out, out_lens = eng.level_apply(buf, lens, s, e, gain, tail)
            assert out.shape == (4, buf.shape[1] + tail) and not torch.isnan(out).any()
            for b, x in enumerate(xs):
                lo, hi = (0, len(x)) if s is None else (int(s[b]), int(e[b]))
                want = torch.from_numpy(x)[lo:hi].cuda() * gain[b]
                assert int(out_lens[b]) == hi - lo + tail
                assert torch.equal(out[b, : hi - lo], want), (b, tail)
                assert float(out[b, hi - lo:].abs().sum()) == 0.0      # the tail and everything behind it: exact zeros
    plain, plain_lens = eng.level_apply(buf, lens)      # no gain: the samples themselves
    for b, x in enumerate(xs):
        assert torch.equal(plain[b, : len(x)].cpu(), torch.from_numpy(x)) and int(plain_lens[b]) == len(x)
    from jyutvoice_amd.engine import _ptr, _stream
    d, small = buf.cuda(), torch.zeros(4, buf.shape[1] + 9, device="cuda")
    rc = eng.lib.jv_level_apply(eng._h, _ptr(d), None, None, None, None, 4, buf.shape[1], 10, _ptr(small), small.shape[1], None,
                                _stream(eng.device))
    assert rc == 4      # JV_ERR_SHAPE
    with pytest.raises(JvError):
        from jyutvoice_amd._lib import check
        check(rc)
    assert torch.equal(eng.level_apply(buf, lens)[0], plain)


# ---- through the pipeline -----------------------------------------------------------------------------------------------------------------
def test_condition_prompt_feeds_the_batch_features():
    """three recordings at two rates: condition_prompt + extract_speech_feat_batch with the lengths staying on the device equals
    the same extraction of recordings trimmed, scaled and padded on the host by the reference"""
    from jyutvoice_amd.utils.audio import condition_prompt, extract_speech_feat_batch
    rates = [16000, 44100, 16000]
    rng = np.random.default_rng(31)
    recs = []
    for r, lead, body, tail, sigma in ((16000, 3000, 20000, 2500, 0.3), (44100, 5000, 50000, 7000, 0.05), (16000, 1000, 30000, 900, 0.2)):
        x = 1e-5 * rng.standard_normal(lead + body + tail)
        x[lead: lead + body] = sigma * rng.standard_normal(body)
        recs.append(x.astype(np.float32))
    rows, lens = condition_prompt([torch.from_numpy(x) for x in recs], rates)
    assert lens.is_cuda and lens.dtype == torch.int32
    host = []
    for b, (x, r) in enumerate(zip(recs, rates)):
        s, e, ratio = ref.trim64(x)
        assert np.abs(ratio - 1.0).min() >= 1e-3 and 0 < s and e < x.size
        g = torch.tensor(ref.gain64(None, ref.peak(x, s, e), ceiling=0.8), dtype=torch.float32)      # fp64, rounded once
        y = torch.cat([torch.from_numpy(x[s:e]) * g, torch.zeros(round(0.2 * r))])
        assert int(lens[b]) == y.numel() and torch.equal(rows[b][: y.numel()].cpu(), y) and float(rows[b][y.numel():].abs().sum()) == 0.0
        host.append(y)
    assert float(np.abs(recs[0]).max()) > 0.8 > float(np.abs(recs[1]).max())      # one is scaled, one is not
    got, got_len = extract_speech_feat_batch(rows, sample_rates=rates, lengths=lens)
    want, want_len = extract_speech_feat_batch(host, sample_rates=rates)
    assert torch.equal(got_len, want_len) and got.shape[1] >= want.shape[1]      # (the rows keep their untrimmed capacity: more padding)
    for b, T in enumerate(want_len.tolist()):
        assert T > 0 and torch.equal(got[b, :T], want[b, :T]) and float(got[b, T:].abs().sum()) == 0.0, b
    only_tail, l2 = condition_prompt([torch.from_numpy(recs[0])], 16000, top_db=None, peak=None, tail_seconds=0.1)
    assert int(l2[0]) == recs[0].size + 1600 and torch.equal(only_tail[0][: recs[0].size].cpu(), torch.from_numpy(recs[0]))


def utterances(counts):
    from jyutvoice_amd import synth
    out = []
    for b, n in enumerate(counts):
        u = synth.batch(1, n, first_index=b)
        obj = {k: u[k][0].tolist() for k in ("x", "lang", "tone", "word_pos", "syllable_pos")}
        obj.update(interspersed=False, spk_embed=u["spk_embed"][0].tolist())
        out.append(obj)
    return out


def test_cli_loudness_writes_the_normalised_samples(tmp_path, monkeypatch):
    """infer.py --synthetic 1 --tokens list.json --loudness -23: the samples handed to the file writer are `normalize_loudness` of
    the samples the same command hands over without the flag, bit for bit, and the files hold them"""
    import infer
    from jyutvoice_amd.utils.audio import load_wav, normalize_loudness
    json.dump(utterances([20, 24]), open(tmp_path / "list.json", "w"))
    written = {}
    real = infer.write_wav

    def spy(path, wav, sample_rate=24000):
        written[str(path)] = wav.detach().clone()
        real(path, wav, sample_rate)

    monkeypatch.setattr(infer, "write_wav", spy)
    common = ["--synthetic", "1", "--tokens", str(tmp_path / "list.json"), "--n_timesteps", "2", "--seed", "7", "--length_scale", "2.0"]
    infer.main(["--output", str(tmp_path / "a.wav")] + common)
    infer.main(["--output", str(tmp_path / "b.wav"), "--loudness", "-23"] + common)
    finite = 0
    for b in range(2):
        plain, loud = written[str(tmp_path / f"a_{b:03d}.wav")], written[str(tmp_path / f"b_{b:03d}.wav")]
        want, lufs, gain = normalize_loudness(plain, 24000, -23.0)
        assert torch.equal(loud, want), b
        finite += math.isfinite(float(lufs[0])) and float(gain[0]) != 1.0
        pcm, rate = load_wav(str(tmp_path / f"b_{b:03d}.wav"))
        assert rate == 24000 and torch.equal(pcm[0], (loud.cpu().clamp(-1, 1) * 32767.0).round() / 32768.0)
    assert finite >= 1      # (an utterance shorter than 400 ms has no loudness and keeps gain 1: not all of them may be that)


def test_server_normalises_only_who_asked(tts_sd, hift_sd):
    from jyutvoice_amd import synth
    import jyutvoice_amd
    from jyutvoice_amd.serve import SynthServer
    from jyutvoice_amd.utils.audio import normalize_loudness
    tts, hift = jyutvoice_amd.build_default("cuda:0")
    tts.load_state_dict(tts_sd)
    hift.load_state_dict(hift_sd)
    tokens = [24, 16, 20]
    keys = ("x", "x_lengths", "lang", "tone", "word_pos", "syllable_pos", "spk_embed")

    def run(options):
        server = SynthServer(tts, hift, max_sessions=3, max_frames=512, max_tokens=64)
        for b, n in enumerate(tokens):
            u = synth.batch(1, n, first_index=b)
            server.submit(*[u[k] for k in keys], n_timesteps=2, length_scale=2.0, seed=40 + b, **options.get(b, {}))
        return server.drain()

    plain, mixed = run({}), run({0: dict(loudness=-20, peak=0.9)})
    assert all("lufs" not in v for v in plain.values()) and "lufs" in mixed[0] and "lufs" not in mixed[1] and "lufs" not in mixed[2]
    for b in (1, 2):
        assert torch.equal(mixed[b]["wav"], plain[b]["wav"])
    want, lufs, gain = normalize_loudness(plain[0]["wav"], 24000, -20.0, 0.9)
    assert torch.equal(mixed[0]["wav"], want) and mixed[0]["wav"].shape == plain[0]["wav"].shape
    assert mixed[0]["lufs"] == float(lufs[0]) and mixed[0]["gain"] == float(gain[0])
    assert math.isfinite(mixed[0]["lufs"]) and mixed[0]["gain"] != 1.0      # (long enough to have a loudness)
    assert float(mixed[0]["wav"].abs().max()) <= 0.9 * (1 + 4 * ULP)


def spied_writer(monkeypatch):
    import infer
    written, real = {}, infer.write_wav

    def spy(path, wav, sample_rate=24000):
        written[str(path)] = wav.detach().clone()
        real(path, wav, sample_rate)

    monkeypatch.setattr(infer, "write_wav", spy)
    return written


@pytest.mark.parametrize("name", ["inflight", "t2w", "single"])
def test_cli_loudness_on_the_other_routes(tmp_path, monkeypatch, name):
    """--loudness -18 --peak 0.9 on the --inflight, --token2wav and single-request routes: what reaches the file writer is
    `normalize_loudness` of what the same command hands over without the flags, bit for bit"""
    import infer
    from jyutvoice_amd import synth
    from jyutvoice_amd.utils.audio import normalize_loudness
    written = spied_writer(monkeypatch)
    json.dump(utterances([20, 24]), open(tmp_path / "list.json", "w"))
    tok, _ = synth.prompt_tokens(2, 30)
    emb = torch.randn(2, 192, generator=torch.Generator().manual_seed(3))
    json.dump([{"speech_token": tok[b].tolist(), "embedding": emb[b].tolist()} for b in range(2)], open(tmp_path / "t2w.json", "w"))
    routes = {
        "inflight": (["--synthetic", "1", "--tokens", str(tmp_path / "list.json"), "--inflight", "2", "--length_scale", "2.0"], 2),
        "t2w": (["--synthetic", "1", "--token2wav", str(tmp_path / "t2w.json")], 2),
        "single": (["--synthetic", "24", "--length_scale", "2.0"], 0),
    }
    flags, count = routes[name]
    common = flags + ["--n_timesteps", "2", "--seed", "7"]
    infer.main(["--output", str(tmp_path / f"{name}_a.wav")] + common)
    infer.main(["--output", str(tmp_path / f"{name}_b.wav"), "--loudness", "-18", "--peak", "0.9"] + common)
    stems = [f"_{b:03d}" for b in range(count)] or [""]
    changed = 0
    for stem in stems:
        plain, loud = written[str(tmp_path / f"{name}_a{stem}.wav")], written[str(tmp_path / f"{name}_b{stem}.wav")]
        want, lufs, gain = normalize_loudness(plain.reshape(-1), 24000, -18.0, 0.9)
        assert torch.equal(loud.reshape(-1), want), (name, stem)
        assert float(want.abs().max()) <= 0.9 * (1 + 4 * ULP)
        changed += math.isfinite(float(lufs[0])) and float(gain[0]) != 1.0
    assert changed >= 1, name


def test_cli_prompt_flags_equal_a_recording_conditioned_on_the_host(tmp_path, monkeypatch):
    """the list route with a "prompt_wav" and --prompt-trim-db 60 --prompt-peak 0.8 --prompt-tail 0.2 writes what it writes, without
    the flags, for a float32 file holding the recording trimmed, scaled and padded by the reference"""
    import infer
    import resample_ref
    from jyutvoice_amd import synth
    written = spied_writer(monkeypatch)
    rng = np.random.default_rng(41)
    x = 1e-5 * rng.standard_normal(4000 + 30000 + 5000)
    x[4000:34000] = 0.3 * rng.standard_normal(30000)
    x = x.astype(np.float32)
    s, e, ratio = ref.trim64(x)
    assert np.abs(ratio - 1.0).min() >= 1e-3 and 0 < s and e < x.size and ref.peak(x, s, e) > 0.8
    g = np.float32(ref.gain64(None, ref.peak(x, s, e), ceiling=0.8))
    y = np.concatenate([x[s:e] * g, np.zeros(3200, np.float32)])
    resample_ref.write_wav(tmp_path / "raw.wav", x, 16000, 32, code=3)
    resample_ref.write_wav(tmp_path / "host.wav", y, 16000, 32, code=3)
    ptok, _ = synth.prompt_tokens(1, 20)
    for name in ("raw", "host"):
        utt = utterances([12])
        utt[0].update(prompt_token=ptok[0].tolist(), prompt_wav=str(tmp_path / f"{name}.wav"))
        json.dump(utt, open(tmp_path / f"{name}.json", "w"))
    common = ["--synthetic", "1", "--n_timesteps", "2", "--seed", "7"]
    infer.main(["--output", str(tmp_path / "a.wav"), "--tokens", str(tmp_path / "raw.json"), "--prompt-trim-db", "60", "--prompt-peak", "0.8",
                "--prompt-tail", "0.2"] + common)
    infer.main(["--output", str(tmp_path / "b.wav"), "--tokens", str(tmp_path / "host.json")] + common)
    infer.main(["--output", str(tmp_path / "c.wav"), "--tokens", str(tmp_path / "raw.json")] + common)
    a, b, c = (written[str(tmp_path / f"{k}_000.wav")] for k in "abc")
    assert torch.equal(a, b) and float(a.abs().max()) > 1e-4
    assert a.shape != c.shape or not torch.equal(a, c)      # (the flags are not a no-op on this recording)
