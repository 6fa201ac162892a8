"""GPU: in-flight batching -- jv_cfm_pool_admit / _step / _fetch driven as timelines on which requests join and leave between
Euler steps, and `SynthServer` end to end.

The definition everything is checked against: a request served by the pool is that request run alone, jv_cfm_solve_prompted at
B = 1 with its own n_timesteps and temperature (and `hift.inference` of its mel after `manual_seed(seed_r)`).  Bounds are the
suite's: 2e-5 max-abs for a mel against the same request in another batch geometry (MEL_BOUND of test_gpu_stream_batch.py), 1e-3
against the CPU oracle (test_gpu_prompt_batch.py), torch.equal where nothing but placement differs, and for waveforms rms <= min(8 x
floor, 5e-5) against the fp64 oracle's decode of the request's own (mel, source).  Figures go to parity_serve.json (JV_OUT)."""
import os

import pytest
import torch

import parity_util as pu
from jyutvoice_amd.serve import step_rows, step_table

pytestmark = pytest.mark.gpu

MEL_BOUND, ORACLE_BOUND, RATIO, OUTER = 2e-5, 1e-3, 8.0, 5e-5
LENGTHS12 = [150, 61, 97, 133, 60, 149, 88, 120, 75, 142, 101, 66]      # tests/test_gpu_prompt_batch.py
KEYS = ("x", "x_lengths", "lang", "tone", "word_pos", "syllable_pos", "spk_embed")
NAN = float("nan")

record = pu.Recorder("parity_serve.json", {
    "what": "tests/test_gpu_serve.py: requests served by the in-flight pool against the same request run alone",
    "mel bound": "max-abs 2e-5 against jv_cfm_solve_prompted at B = 1 (another batch geometry); 1e-3 against the CPU oracle",
    "waveform bound": "rms(served wav - fp64 oracle on the request's mel and source) <= 8 x floor and <= 5e-5; floor = rms(fp32 oracle "
                      "- fp64 oracle); clamped share of the fp64 reference <= 1 %",
    "exact": "1.0 where the served result was in fact bit-equal to the reference it is compared with"})


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    torch.set_num_threads(min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def models(tts_sd, hift_sd):
    import jyutvoice_amd
    tts, hift = jyutvoice_amd.build_default("cuda:0")
    tts.load_state_dict(tts_sd)
    hift.load_state_dict(hift_sd)
    return tts, hift


@pytest.fixture(scope="module")
def rt(models):
    from jyutvoice_amd.runtime import get_runtime
    r = get_runtime("cuda:0")
    r.ensure(12, 256, 64)
    return r


def make_request(idx, y, p, n, temp=1.0, at=0, scale=1.0):
    g = torch.Generator().manual_seed(4000 + idx)
    return dict(y=y, p=p, n=n, temp=temp, at=at, mu_y=torch.randn(1, 80, y, generator=g) * scale, ph=torch.randn(1, p, 80, generator=g),
                pf=torch.randn(1, p, 80, generator=g), spks=torch.randn(1, 80, generator=g) * 0.5)


def padded(reqs, fill=0.0):
    """the admit call's tensors for a group of requests, `fill` behind every length (NaN: must not be read)"""
    B, Ty, P = len(reqs), max(r["y"] for r in reqs) + 3, max(max(r["p"] for r in reqs), 1) + 2
    mu_y, ph, pf = torch.full((B, 80, Ty), fill), torch.full((B, P, 80), fill), torch.full((B, P + 1, 80), fill)
    for b, r in enumerate(reqs):
        mu_y[b, :, :r["y"]], ph[b, :r["p"]], pf[b, :r["p"]] = r["mu_y"][0], r["ph"][0], r["pf"][0]
    return mu_y, ph, pf, torch.cat([r["spks"] for r in reqs])


def run_timeline(eng, reqs, slots, cap, poison=False):
    """requests join at step r['at'] (first free slot, freed slots go to the back of the line), take n Euler steps each at their
    own (t, dt) and leave -> ({index: mel [80, y]}, rows of every step, {index: slot})"""
    pool = eng.cfm_pool(slots, cap)
    if poison:
        for t in pool.tensors():
            t.fill_(NAN)
    tables = [step_table(r["n"]) for r in reqs]
    free, active, out, rows, slot_of = list(range(slots)), [], {}, [], {}
    step = 0
    while len(out) < len(reqs):
        new = [i for i, r in enumerate(reqs) if r["at"] == step]
        if new:
            grp = [reqs[i] for i in new]
            mu_y, ph, pf, spks = padded(grp, NAN if poison else 0.0)
            got = [free.pop(0) for _ in new]
            eng.cfm_pool_admit(pool, mu_y, [r["y"] for r in grp], ph, pf, [r["p"] for r in grp], spks, got, [r["temp"] for r in grp])
            for i, s in zip(new, got):
                active.append([i, s, 0])
                slot_of[i] = s
        assert active and step < 64
        lens = [reqs[i]["p"] + reqs[i]["y"] for i, _, _ in active]
        eng.cfm_pool_step(pool, [s for _, s, _ in active], lens, [tables[i][0][k] for i, _, k in active],
                          [tables[i][1][k] for i, _, k in active])
        rows.append(step_rows(lens))
        for a in active:
            a[2] += 1
        fin = [a for a in active if a[2] == reqs[a[0]]["n"]]
        if fin:
            ys = [reqs[i]["y"] for i, _, _ in fin]
            mel = eng.cfm_pool_fetch(pool, [s for _, s, _ in fin], [reqs[i]["p"] for i, _, _ in fin], ys, frames=max(ys) + 5).cpu()
            for b, (i, s, _) in enumerate(fin):
                assert float(mel[b, :, ys[b]:].abs().sum()) == 0.0      # zeros behind the request's frames
                out[i] = mel[b, :, :ys[b]]
                if poison:      # what a request leaves in its slot must not reach the next occupant
                    for t in pool.tensors():
                        t[s] = NAN
                free.append(s)
            active = [a for a in active if a not in fin]
        step += 1
    return out, rows, slot_of


def solo(eng, r):
    """the definition: the request alone through jv_cfm_solve_prompted, with the t_span `synthesise` passes"""
    ts = 1 - torch.cos(torch.linspace(0, 1, r["n"] + 1) * 0.5 * torch.pi)
    P = max(r["p"], 1)
    ph, pf = torch.zeros(1, P, 80), torch.zeros(1, P, 80)
    ph[:, :r["p"]], pf[:, :r["p"]] = r["ph"], r["pf"]
    mel = eng.cfm_solve_prompted(r["mu_y"], torch.tensor([r["y"]]), ph, pf, torch.tensor([r["p"]]), r["spks"], r["n"], r["temp"], t_span=ts)
    return mel[0].cpu()


def oracle_mel(tts_sd, noise, r):
    from oracle import flow as oflow
    T = r["p"] + r["y"]
    mu = torch.cat([r["ph"].transpose(1, 2), r["mu_y"]], dim=2)
    cond = torch.cat([r["pf"].transpose(1, 2), torch.zeros(1, 80, r["y"])], dim=2)
    with torch.inference_mode():
        m = oflow.cfm_solve(tts_sd, noise, mu, torch.ones(1, 1, T), r["spks"], cond, r["n"], r["temp"])
    return m[0, :, r["p"]:]


def timeline2():
    """three requests admitted at steps 0 / 1 / 3 with their own n and temperature; a fourth takes the slot the first one frees"""
    return [make_request(0, 44, 30, 3, 1.0, 0), make_request(1, 61, 0, 5, 0.6, 1), make_request(2, 97, 44, 4, 1.3, 3),
            make_request(3, 52, 0, 2, 1.0, 3)]


@pytest.fixture(scope="module")
def solos2(rt):
    return [solo(rt.engine, r) for r in timeline2()]


@pytest.fixture(scope="module")
def clean2(rt):
    return run_timeline(rt.engine, timeline2(), 3, 160)


def check_against(name, got, want, bound=MEL_BOUND):
    e = pu.md(got, want)
    record(name, error=e, exact=float(torch.equal(got, want)))
    assert torch.isfinite(got).all(), name
    assert e <= bound, (name, e)


# ---- 1. lockstep ---------------------------------------------------------------------------------------------------------------------
def test_lockstep_pool_against_closed_batch(rt):
    """three requests admitted together, four pool steps + fetch, against jv_cfm_solve_prompted of the same batch"""
    eng = rt.engine
    reqs = [make_request(i, y, p, 4) for i, (y, p) in enumerate(((44, 30), (61, 0), (97, 44)))]
    out, rows, _ = run_timeline(eng, reqs, 3, 160)
    assert rows == [step_rows([74, 61, 141])] * 4
    mu_y, ph, pf, spks = padded(reqs)
    ts = 1 - torch.cos(torch.linspace(0, 1, 5) * 0.5 * torch.pi)
    batch = eng.cfm_solve_prompted(mu_y, torch.tensor([44, 61, 97]), ph, pf, torch.tensor([30, 0, 44]), spks, 4, t_span=ts).cpu()
    for b, r in enumerate(reqs):
        check_against(f"lockstep request {b}", out[b], batch[b, :, :r["y"]])


# ---- 2. staggered ----------------------------------------------------------------------------------------------------------------------
def test_staggered_requests_against_their_solo_solves(clean2, solos2):
    """catches a broadcast t, a shared dt, a wrong twin: every request has its own n, temperature and arrival"""
    out, rows, slot_of = clean2
    assert slot_of == {0: 0, 1: 1, 2: 2, 3: 0}                     # the fourth request sits where the first one was
    assert rows == [step_rows(l) for l in ([74], [74, 61], [74, 61], [61, 141, 52], [61, 141, 52], [61, 141], [141])]
    for i in range(4):
        check_against(f"staggered request {i} vs solo", out[i], solos2[i])


def test_staggered_requests_against_the_oracle(clean2, tts_sd, noise):
    out, _, _ = clean2
    for i, r in enumerate(timeline2()):
        check_against(f"staggered request {i} vs oracle", out[i], oracle_mel(tts_sd, noise, r), ORACLE_BOUND)


# ---- 3. poison -------------------------------------------------------------------------------------------------------------------------
def test_nothing_behind_a_length_or_in_a_free_slot_is_read(rt, clean2):
    """NaN in every pool row behind a request's length, in all unused and freed slots (maxima and speaker vectors included) and in
    the pad columns of mu_y / the prompts: the same bits as the clean run"""
    dirty, _, _ = run_timeline(rt.engine, timeline2(), 3, 160, poison=True)
    for i in range(4):
        assert torch.isfinite(dirty[i]).all(), i
        assert torch.equal(dirty[i], clean2[0][i]), (i, pu.md(dirty[i], clean2[0][i]))


# ---- 4. slot reuse: a request's scales depend on that request alone --------------------------------------------------------------------
@pytest.mark.parametrize("order", ["quiet_then_loud", "loud_then_quiet"])
def test_slot_reuse_does_not_inherit_maxima(rt, order):
    """two requests of 80 frames follow each other in ONE slot while a bystander stays resident.  A stale larger bound would cost
    the quiet one its low bits; a stale smaller one would overflow the loud one's fp16 planes"""
    eng = rt.engine
    quiet = make_request(10, 80, 0, 3, 1.0 / 16, scale=1.0 / 16)
    loud = make_request(11, 80, 0, 3, 1.0, scale=4.0)
    first, second = (quiet, loud) if order == "quiet_then_loud" else (loud, quiet)
    reqs = [dict(make_request(12, 70, 20, 7), at=0), dict(first, at=0), dict(second, at=3)]
    out, _, slot_of = run_timeline(eng, reqs, 2, 96)
    assert slot_of[1] == slot_of[2] != slot_of[0]
    for i, name in ((1, "first"), (2, "second"), (0, "bystander")):
        want = solo(eng, reqs[i])
        scale = max(1.0, float(want.abs().max()))
        e = pu.md(out[i], want)
        record(f"slot reuse {order}: {name}", error=e, scale=scale, exact=float(torch.equal(out[i], want)))
        assert torch.isfinite(out[i]).all()
        assert e <= MEL_BOUND * scale, (order, name, e, scale)


# ---- 5. the row-owning regime and the split-K seam ----------------------------------------------------------------------------------------
def test_twelve_requests_across_the_2048_row_seam(rt):
    """three requests join per step; the step rows 4 + 2 sum(len + 4) start at 644, pass 2048 while all twelve are resident
    (2584) and fall back: a request changes regime in mid-solve and still meets its solo solve"""
    eng = rt.engine
    reqs = [make_request(20 + i, y, 0, 6, 1.0, i // 3) for i, y in enumerate(LENGTHS12)]
    out, rows, _ = run_timeline(eng, reqs, 12, 160)
    assert rows[0] == 644 and max(rows) == 2584 and rows[3] == 2584
    assert sum(r > 2048 for r in rows) >= 3 and sum(r <= 2048 for r in rows) >= 3 and rows[-1] < 2048
    worst = 0.0
    for i, r in enumerate(reqs):
        e = pu.md(out[i], solo(eng, r))
        worst = max(worst, e)
        record(f"seam request {i}", error=e)
        assert torch.isfinite(out[i]).all()
    assert worst <= MEL_BOUND, worst


# ---- 6. modes ----------------------------------------------------------------------------------------------------------------------------
def test_streaming_mode_uniform_geometry(rt, clean2):
    """under set_streaming(50) the compact geometry is not allowed: the uniform one with unequal lengths"""
    eng = rt.engine
    eng.set_streaming(50)
    try:
        out, _, _ = run_timeline(eng, timeline2(), 3, 160)
        want = [solo(eng, r) for r in timeline2()]
    finally:
        eng.set_streaming(0)
    for i in range(4):
        check_against(f"streaming request {i} vs solo", out[i], want[i])
    assert any(not torch.equal(out[i], clean2[0][i]) for i in range(4))      # (the mode did apply)


def test_fp16_mode(rt, clean2):
    rt.set_precision("fp16")
    try:
        out, _, _ = run_timeline(rt.engine, timeline2(), 3, 160)
        want = [solo(rt.engine, r) for r in timeline2()]
    finally:
        rt.set_precision("fp32")
    for i in range(4):
        check_against(f"fp16 request {i} vs solo", out[i], want[i])
    assert any(not torch.equal(out[i], clean2[0][i]) for i in range(4))


# ---- 7. validation -----------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_name_the_request_and_leave_the_pools_unchanged(rt):
    from jyutvoice_amd._lib import JvError
    eng = rt.engine
    reqs = [make_request(30, 40, 10, 3), make_request(31, 33, 0, 3)]
    pool = eng.cfm_pool(3, 64)
    mu_y, ph, pf, spks = padded(reqs)
    eng.cfm_pool_admit(pool, mu_y, [40, 33], ph, pf, [10, 0], spks, [0, 2], [1.0, 1.0])
    tt, dts = step_table(3)
    eng.cfm_pool_step(pool, [0, 2], [50, 33], [tt[0]] * 2, [dts[0]] * 2)
    before = [t.clone() for t in pool.tensors()]

    def rejected(match, fn, *args):
        with pytest.raises(JvError, match=match):
            fn(pool, *args)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, pool.tensors())), match

    t2, d2 = [tt[1]] * 2, [dts[1]] * 2
    rejected("request 1: slot 3 outside", eng.cfm_pool_step, [0, 3], [50, 33], t2, d2)
    rejected("request 0: slot -1 outside", eng.cfm_pool_step, [-1, 2], [50, 33], t2, d2)
    rejected("request 1: slot 0 is named twice", eng.cfm_pool_step, [0, 0], [50, 33], t2, d2)
    rejected("request 1: 0 frames outside", eng.cfm_pool_step, [0, 2], [50, 0], t2, d2)
    rejected("request 0: 65 frames outside", eng.cfm_pool_step, [0, 2], [65, 33], t2, d2)
    rejected("request 1: t / dt is not a number", eng.cfm_pool_step, [0, 2], [50, 33], [tt[1], NAN], d2)
    rejected("request 1: slot 2 is named twice", eng.cfm_pool_admit, mu_y, [40, 33], ph, pf, [10, 0], spks, [2, 2], [1.0, 1.0])
    rejected("request 0: 44 frames outside", eng.cfm_pool_admit, mu_y, [44, 33], ph, pf, [10, 0], spks, [1, 2], [1.0, 1.0])
    small = eng.cfm_pool(3, 45)
    with pytest.raises(JvError, match="request 0: 10 \\+ 40 frames outside"):
        eng.cfm_pool_admit(small, mu_y, [40, 33], ph, pf, [10, 0], spks, [1, 2], [1.0, 1.0])
    assert float(small.x.abs().sum()) == 0.0
    rejected("request 1: prompt length 99 outside", eng.cfm_pool_admit, mu_y, [40, 33], ph, pf, [10, 99], spks, [1, 2], [1.0, 1.0])
    rejected("request 0: frames \\[60, 60 \\+ 10\\) outside", eng.cfm_pool_fetch, [0], [60], [10])
    # rows beyond the reservation: more requests than the context holds, a request longer than its frames
    many = eng.max_batch + 1
    big = eng.cfm_pool(many, 8)
    with pytest.raises(JvError, match="beyond the reservation"):
        eng.cfm_pool_step(big, list(range(many)), [8] * many, [0.0] * many, [0.1] * many)
    long = eng.cfm_pool(1, eng.max_frames + 64)
    with pytest.raises(JvError, match="request 0: .* exceed the reservation"):
        eng.cfm_pool_step(long, [0], [eng.max_frames + 1], [0.0], [0.1])
    assert float(big.x.abs().sum()) == 0.0 and float(long.x.abs().sum()) == 0.0
    # the context and the pools are as usable as before: the remaining steps give what an undisturbed run gives
    for k in (1, 2):
        eng.cfm_pool_step(pool, [0, 2], [50, 33], [tt[k]] * 2, [dts[k]] * 2)
    got = eng.cfm_pool_fetch(pool, [0, 2], [10, 0], [40, 33]).cpu()
    ref, _, _ = run_timeline(eng, reqs, 3, 64)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1, :, :33], ref[1])


# ---- 8. SynthServer end to end ------------------------------------------------------------------------------------------------------------
SERVE_TOKENS, SERVE_PROMPTS, SERVE_N = [24, 40, 31, 24, 36], [15, 0, 33, 0, 0], [4, 3, 5, 4, 4]
SERVE_SCALE, SERVE_SEEDS = [1.0, 1.0, 1.2, 1.0, 1.2], [11, 12, 13, 14, 15]


@pytest.fixture(scope="module")
def served(models, rt, prompt_sd):
    """five requests submitted one per step into three slots -> (results, the B = 1 arguments of every request)"""
    from jyutvoice_amd import synth
    from jyutvoice_amd.flow.encoder import FlowEncoder
    from jyutvoice_amd.serve import SynthServer
    tts, hift = models
    fenc = FlowEncoder(vocab_size=6561, input_size=512, output_size=80, device="cuda:0")
    fenc.load_state_dict(prompt_sd)
    batch = synth.batch(5, 40, lengths=SERVE_TOKENS)
    have = [b for b, n in enumerate(SERVE_PROMPTS) if n]
    tok, lens = synth.prompt_tokens(len(have), max(SERVE_PROMPTS), lengths=[SERVE_PROMPTS[b] for b in have], first_index=1)
    h, _ = fenc(tok, lens)
    g = torch.Generator().manual_seed(3)
    args = []
    for b in range(5):
        L = SERVE_TOKENS[b]
        one = [batch[k][b:b + 1] if k in ("x_lengths", "spk_embed") else batch[k][b:b + 1, :L] for k in KEYS]
        p = 2 * SERVE_PROMPTS[b]
        feat = torch.randn(1, p, 80, generator=g) if p else None
        ph = h[have.index(b):have.index(b) + 1, :p].cpu() if p else None
        args.append((one, feat, ph))
    server = SynthServer(tts, hift, max_sessions=3, max_frames=512, max_tokens=64)      # (its one reservation)
    caps = rt.caps
    out, rids = {}, []
    for b in range(5):
        one, feat, ph = args[b]
        rids.append(server.submit(*one, prompt_feat=feat, prompt_h=ph, n_timesteps=SERVE_N[b], length_scale=SERVE_SCALE[b],
                                  seed=SERVE_SEEDS[b]))
        out.update(server.step())
    out.update(server.drain())
    assert rt.caps == caps                  # no step rebuilt or grew the context
    assert sorted(out) == rids == list(range(5)) and all("error" not in v for v in out.values())
    return out, args


@pytest.mark.parametrize("b", range(5))
def test_synth_server_request_against_its_definition(models, served, hift_sd, b):
    tts, hift = models
    out, args = served
    one, feat, ph = args[b]
    got = out[b]
    p = 0 if feat is None else feat.shape[1]
    kw = dict(n_timesteps=SERVE_N[b], length_scale=SERVE_SCALE[b], batched=True)
    if p:
        want = tts.synthesise(*one, feat, prompt_h=ph, prompt_lengths=torch.tensor([p]), **kw)
    else:
        want = tts.synthesise(*one, torch.zeros(1, 1, 80), prompt_h=torch.zeros(1, 1, 80), prompt_lengths=torch.tensor([0]), **kw)
    y = int(want["mel_lengths"][0])
    assert got["mel_length"] == y and got["mel"].shape == (1, 80, y) and got["wav"].shape == (1, 480 * y)
    check_against(f"server request {b} mel vs synthesise", got["mel"].cpu(), want["mel"][:, :, :y].cpu())
    hift.manual_seed(SERVE_SEEDS[b])
    wav1, s1 = hift.inference(got["mel"])
    assert torch.equal(got["source"], s1)
    w32, w64 = pu.hift_folded(hift_sd)
    mel, s = got["mel"].cpu(), got["source"].cpu()
    r64, r32 = pu.hift_fp64(w64, mel, s, y), pu.hift_fp32(w32, mel, s, y)
    share, floor, err = pu.clamp_share(r64), pu.rms(r32, r64), pu.rms(got["wav"].cpu(), r64)
    record(f"server request {b} waveform", clamped_share=share, floor=floor, error=err, ratio=err / floor,
           vs_inference=pu.rms(got["wav"], wav1))
    assert share <= pu.CLAMP_CAP, (b, share)
    assert 0.0 < floor < OUTER, (b, floor)
    assert err <= RATIO * floor and err <= OUTER, f"request {b}: rms {err:.3e} = {err / floor:.2f} x the oracle's own {floor:.3e}"


# ---- 9. CLI ------------------------------------------------------------------------------------------------------------------------------
def test_cli_inflight_writes_what_the_list_route_writes(tmp_path):
    """infer.py --synthetic 1 --tokens list.json --inflight 3: four requests (two with a voice prompt) through three slots, one
    arrival per step, write the files the list route writes -- the same lengths, each mel within 2e-5 of the list route's"""
    import json

    import numpy as np

    import infer
    from jyutvoice_amd import synth
    from jyutvoice_amd.utils.audio import load_wav
    g = torch.Generator().manual_seed(9)
    utts = []
    for b, n in enumerate([12, 15, 8, 10]):
        u = synth.batch(1, n, first_index=b)
        obj = {k: u[k][0].tolist() for k in ("x", "lang", "tone", "word_pos", "syllable_pos")}
        obj["interspersed"] = False      # raw id lists: the CLI puts the blanks in
        obj["spk_embed"] = u["spk_embed"][0].tolist()
        if b in (0, 2):
            tok, _ = synth.prompt_tokens(1, 10 + 5 * b, first_index=b)
            obj.update(prompt_token=tok[0].tolist(), prompt_feat=torch.randn(2 * (10 + 5 * b), 80, generator=g).tolist())
        utts.append(obj)
    json.dump(utts, open(tmp_path / "list.json", "w"))
    common = ["--synthetic", "1", "--tokens", str(tmp_path / "list.json"), "--n_timesteps", "3", "--seed", "7"]
    infer.main(["--output", str(tmp_path / "a.wav"), "--dump-mel", str(tmp_path / "a")] + common)
    infer.main(["--output", str(tmp_path / "b.wav"), "--dump-mel", str(tmp_path / "b"), "--inflight", "3"] + common)
    assert sorted(p.name for p in tmp_path.glob("b_*.wav")) == sorted(p.name.replace("a_", "b_") for p in tmp_path.glob("a_*.wav"))
    assert len(list(tmp_path.glob("b_*.wav"))) == 4
    for b in range(4):
        one, rate = load_wav(str(tmp_path / f"a_{b:03d}.wav"))
        srv, rate2 = load_wav(str(tmp_path / f"b_{b:03d}.wav"))
        ma, mb = (torch.from_numpy(np.load(tmp_path / d / f"mel_{b:03d}.npy")) for d in "ab")
        assert rate == rate2 == 24000 and ma.shape == mb.shape and one.shape[-1] == srv.shape[-1] == 480 * ma.shape[1]
        assert torch.isfinite(srv).all() and float(srv.abs().max()) > 1e-4
        check_against(f"cli request {b} mel vs list route", mb, ma)
    with pytest.raises(SystemExit, match="--inflight needs --tokens"):
        infer.main(["--output", str(tmp_path / "c.wav"), "--synthetic", "8", "--inflight", "2"])
