"""GPU: a guidance rate per request in the in-flight pool (jv_cfm_pool_step_g), `SynthServer` with a guidance window, and the
no-twin solve in FP16 mode.

A request served by the pool stays DEFINED as that request run alone: jv_cfm_solve_prompted at B = 1 with its rate set
(jv_flow_set_guidance), met within 2e-5, the bound of any change of batch geometry (tests/test_gpu_serve.py).  Measured figures go to
parity_guidance.json (JV_OUT)."""
import pytest
import torch

import parity_util as pu
from jyutvoice_amd.serve import guidance_rates, step_table
from test_gpu_cfg_share import inputs
from test_gpu_serve import KEYS, MEL_BOUND, make_request, padded

pytestmark = pytest.mark.gpu

record = pu.Recorder("parity_guidance.json", {
    "what": "tests/test_gpu_guidance_serve.py: requests served by the in-flight pool at their own guidance rate against the same "
            "request run alone with that rate set; the no-twin solve (rate 0) in FP16 mode against the fp32 CPU oracle",
    "mel bound": "max-abs 2e-5 against jv_cfm_solve_prompted / synthesise at B = 1 (another batch geometry)",
    "fp16": "no bound asserted (tests/test_gpu_fp16_estimator.py bounds its own shapes against an emulation): finiteness only, the "
            "distance is recorded"})


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


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


def solo(eng, r, rate):
    """the definition: the request alone through jv_cfm_solve_prompted with its rate set"""
    ts = 1 - torch.cos(torch.linspace(0, 1, r["n"] + 1) * 0.5 * torch.pi)
    P = max(r["p"], 1)
    ph, pf = torch.zeros(1, P, 80), torch.zeros(1, P, 80)
    ph[:, :r["p"]], pf[:, :r["p"]] = r["ph"], r["pf"]
    with eng.guidance([rate]):
        mel = eng.cfm_solve_prompted(r["mu_y"], torch.tensor([r["y"]]), ph, pf, torch.tensor([r["p"]]), r["spks"], r["n"], r["temp"],
                                     t_span=ts)
    return mel[0].cpu()


def test_three_requests_at_their_own_rates(rt):
    """rates 0 / 0.7 / 2.0 with n = 2 / 3 / 4, the third prompted, admitted at steps 0, 0 and 1: a broadcast rate, or the rate of
    another request's slot, misses the solo solves by orders of magnitude more than the bound"""
    eng = rt.engine
    reqs = [make_request(60, 44, 0, 2, 1.0, 0), make_request(61, 61, 0, 3, 0.8, 0), make_request(62, 50, 24, 4, 1.0, 1)]
    rates = [0.0, 0.7, 2.0]
    tables = [step_table(r["n"]) for r in reqs]
    pool = eng.cfm_pool(3, 96)
    active, out, step = [], {}, 0
    while len(out) < 3:
        new = [i for i, r in enumerate(reqs) if r["at"] == step]
        if new:
            grp = [reqs[i] for i in new]
            mu_y, ph, pf, spks = padded(grp)
            eng.cfm_pool_admit(pool, mu_y, [r["y"] for r in grp], ph, pf, [r["p"] for r in grp], spks, new, [r["temp"] for r in grp])
            active += [[i, 0] for i in new]      # (request i sits in slot i)
        assert active and step < 8
        eng.cfm_pool_step(pool, [i for i, _ in active], [reqs[i]["p"] + reqs[i]["y"] for i, _ in active],
                          [tables[i][0][k] for i, k in active], [tables[i][1][k] for i, k in active], cfg=[rates[i] for i, _ in active])
        for a in active:
            a[1] += 1
        for i, k in [a for a in active if a[1] == reqs[a[0]]["n"]]:
            out[i] = eng.cfm_pool_fetch(pool, [i], [reqs[i]["p"]], [reqs[i]["y"]]).cpu()[0]
        active = [a for a in active if a[1] < reqs[a[0]]["n"]]
        step += 1
    for i, r in enumerate(reqs):
        want = solo(eng, r, rates[i])
        e = pu.md(out[i], want)
        record(f"pool request {i} at rate {rates[i]} vs solo", error=e, exact=float(torch.equal(out[i], want)))
        assert torch.isfinite(out[i]).all() and e <= MEL_BOUND, (i, e)
    assert pu.md(out[0], solo(eng, reqs[0], 0.7)) > 100 * MEL_BOUND      # (the rate is read: request 0 at 0.7 is another mel)


def test_old_entry_is_the_new_one_at_0_7(rt):
    eng = rt.engine
    reqs = [make_request(70, 40, 10, 3), make_request(71, 33, 0, 3)]
    mu_y, ph, pf, spks = padded(reqs)
    tt, dts = step_table(3)
    got = []
    for cfg in (None, [0.7, 0.7]):
        pool = eng.cfm_pool(3, 64)
        eng.cfm_pool_admit(pool, mu_y, [40, 33], ph, pf, [10, 0], spks, [0, 2], [1.0, 1.0])
        for k in range(3):
            eng.cfm_pool_step(pool, [0, 2], [50, 33], [tt[k]] * 2, [dts[k]] * 2, cfg=cfg)
        got.append([t.clone().cpu() for t in pool.tensors()])
    for a, b in zip(*got):
        assert torch.equal(a, b), pu.md(a, b)
    from jyutvoice_amd._lib import JvError
    pool = eng.cfm_pool(3, 64)
    eng.cfm_pool_admit(pool, mu_y, [40, 33], ph, pf, [10, 0], spks, [0, 2], [1.0, 1.0])
    before = pool.x.clone()
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(JvError, match="request 1: guidance rate .* finite and >= 0"):
            eng.cfm_pool_step(pool, [0, 2], [50, 33], [tt[0]] * 2, [dts[0]] * 2, cfg=[0.7, bad])
    torch.cuda.synchronize()
    assert torch.equal(pool.x, before)      # a rejected call leaves the pools unchanged


def test_synth_server_with_a_guidance_window(models, rt):
    """two requests through a SynthServer, one with cfg_rate = 1.5 in the window t in [0, 0.5), against synthesise(cfg_schedule=...)
    of each alone (the comparison and the bound of test_synth_server_request_against_its_definition)"""
    from jyutvoice_amd import synth
    from jyutvoice_amd.serve import SynthServer
    tts, hift = models
    tokens, ns = [20, 27], [4, 3]
    batch = synth.batch(2, 27, lengths=tokens)
    args = [[batch[k][b:b + 1] if k in ("x_lengths", "spk_embed") else batch[k][b:b + 1, :tokens[b]] for k in KEYS] for b in range(2)]
    kws = [dict(cfg_rate=1.5, cfg_window=(0.0, 0.5)), dict()]
    server = SynthServer(tts, hift, max_sessions=2, max_frames=256, max_tokens=64)
    rids = [server.submit(*args[b], n_timesteps=ns[b], seed=20 + b, **kws[b]) for b in range(2)]
    out = server.drain()
    assert sorted(out) == rids and all("error" not in v for v in out.values())
    sched = guidance_rates(ns[0], 1.5, (0.0, 0.5))
    assert 0.0 in sched and 1.5 in sched
    none = torch.zeros(1, 1, 80)
    for b, schedule in enumerate((sched, None)):
        want = tts.synthesise(*args[b], none, prompt_h=none, prompt_lengths=torch.tensor([0]), n_timesteps=ns[b], batched=True,
                              cfg_schedule=schedule)
        y = int(want["mel_lengths"][0])
        got = out[rids[b]]
        assert got["mel_length"] == y
        e = pu.md(got["mel"].cpu(), want["mel"][:, :, :y].cpu())
        record(f"server request {b} mel vs synthesise(cfg_schedule={schedule})", error=e)
        assert torch.isfinite(got["mel"]).all() and e <= MEL_BOUND, (b, e)
    plain = tts.synthesise(*args[0], none, prompt_h=none, prompt_lengths=torch.tensor([0]), n_timesteps=ns[0], batched=True)
    assert pu.md(out[rids[0]]["mel"].cpu(), plain["mel"][:, :, :out[rids[0]]["mel_length"]].cpu()) > 100 * MEL_BOUND      # (the window is read)


def test_no_twin_solve_in_fp16_mode(rt, tts_sd, noise):
    """the rate-0 case of test_constant_rate_against_the_oracle (B = 2, T = 64, lens [64, 41], n = 3) with set_precision("fp16").
    tests/test_gpu_fp16_estimator.py bounds its own shapes against an emulation and has none for this one: finiteness is asserted,
    the distance to the fp32 CPU oracle is written to parity_guidance.json."""
    from oracle import flow as oflow
    eng = rt.engine
    mu, spks, cond = inputs(2, 64, 511)
    lens = torch.tensor([64, 41], dtype=torch.int32)
    mask = (torch.arange(64)[None] < lens[:, None]).unsqueeze(1).float()
    mu, cond = mu * mask, cond * mask
    rt.set_precision("fp16")
    try:
        with eng.guidance([0.0]):
            mel = rt.engine.cfm_solve(mu, lens, spks, cond, 3).cpu()
    finally:
        rt.set_precision("fp32")
    assert torch.isfinite(mel).all()
    for b, L in enumerate([64, 41]):
        with torch.inference_mode():
            want = oflow.cfm_solve(tts_sd, noise, mu[b:b + 1, :, :L], torch.ones(1, 1, L), spks[b:b + 1], cond[b:b + 1, :, :L], 3, 1.0,
                                   cfg_rate=0.0)[0]
        record(f"fp16 rate 0 utterance {b} vs fp32 oracle", error=pu.md(mel[b, :, :L], want), scale=float(want.abs().max()))
        if L < 64:
            assert float(mel[b, :, L:].abs().max()) == 0.0
