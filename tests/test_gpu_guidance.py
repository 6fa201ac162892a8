"""GPU: the guidance rate of the CFM solve as a context mode (jv_flow_set_guidance), per solve and per Euler step, and the steps
without unconditional twins behind a rate of exactly 0 (flow.hip solve_loop, DESIGN.md 5 "Guidance").

Bounds.  Against the CPU oracle: 3e-4 max(1, (1 + 2 r) / 2.4) -- 3e-4 is what test_cfm_batched_equals_singles allows at r = 0.7,
the update weights the two estimator evaluations by 1 + r and r, so an estimator error is amplified by 1 + 2 r, 2.4 at 0.7.
Between two batch geometries of one solve (twins dropped against kept, a batch row against its B = 1 run, a prompted pack against
the hand-concatenated one): 2e-5, the project's bound for a change of batch geometry.  torch.equal where only the way the rate
0.7 arrives differs.  Taken / not taken is read from the in-library profiler: a step's fused-block launches account for B T frames
without twins, 2 B T with them, (B + 1) T in a shared first step."""
import pytest
import torch

import guidance_ref
import token2mel_cases as tc
from parity_util import md, profiled
from test_gpu_cfg_share import block_frames, inputs

pytestmark = pytest.mark.gpu

GEOMETRY_BOUND = 2e-5


def oracle_bound(r):
    return 3e-4 * max(1.0, (1.0 + 2.0 * r) / 2.4)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def fresh_engine(tts_sd, noise, max_batch, max_frames):
    from jyutvoice_amd.engine import JV_MODEL_TTS, Engine
    e = Engine("cuda:0", max_batch=max_batch, max_frames=max_frames, max_tokens=64)
    e.load_state_dict(JV_MODEL_TTS, tts_sd)
    e.load_noise(noise)
    return e


@pytest.fixture(scope="module")
def eng(tts_sd, noise):
    e = fresh_engine(tts_sd, noise, 12, 256)
    yield e
    e.close()


def arm(monkeypatch, tts_sd, noise, drop, max_batch, max_frames, fn):
    """fn(engine) on a fresh engine with the twins of rate-0 steps dropped (the default) or kept (JV_NO_TWIN_DROP=1): the switch
    is read when a context is created"""
    if drop:
        monkeypatch.delenv("JV_NO_TWIN_DROP", raising=False)
    else:
        monkeypatch.setenv("JV_NO_TWIN_DROP", "1")
    e = fresh_engine(tts_sd, noise, max_batch, max_frames)
    try:
        return fn(e)
    finally:
        e.close()


def span(n, sched="cosine"):
    return guidance_ref.t_span(n, sched)


# ---- 1. the default keeps its bits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(1, 61), (12, 200)], ids=["split_k", "row_owning_shared_twin"])
def test_default_bits(eng, B, T):
    """mode unset against 0.7 set once and 0.7 per step: the same fp32 operations in the same order"""
    mu, spks, cond = inputs(B, T, 500 + B)
    base = eng.cfm_solve(mu, None, spks, cond, 3).cpu()
    try:
        eng.set_guidance([0.7])
        one = eng.cfm_solve(mu, None, spks, cond, 3).cpu()
        eng.set_guidance([0.7] * 3)
        per_step = eng.cfm_solve(mu, None, spks, cond, 3).cpu()
    finally:
        eng.set_guidance(None)
    assert torch.isfinite(base).all()
    assert torch.equal(one, base), md(one, base)
    assert torch.equal(per_step, base), md(per_step, base)
    assert torch.equal(eng.cfm_solve(mu, None, spks, cond, 3).cpu(), base)


# ---- 2. / 3. against the oracle ---------------------------------------------------------------------------------------------------
ORACLE_LENS = [64, 41]


@pytest.fixture(scope="module")
def oracle_inputs():
    mu, spks, cond = inputs(2, 64, 511)
    lens = torch.tensor(ORACLE_LENS, dtype=torch.int32)
    mask = (torch.arange(64)[None] < lens[:, None]).unsqueeze(1).float()
    return mu * mask, spks, cond * mask, lens


def check_vs_reference(mel, want_of, bound, tag):
    for b, L in enumerate(ORACLE_LENS):
        assert torch.isfinite(mel[b]).all()
        if L < mel.shape[2]:
            assert float(mel[b, :, L:].abs().max()) == 0.0, (tag, b)      # frames behind a length are exactly 0
        e = md(mel[b, :, :L], want_of(b, L))
        print(f"{tag}, utterance {b}: {e:.3e} (bound {bound:.3e})")
        assert e <= bound, (tag, b, e, bound)


@pytest.mark.parametrize("r", [0.0, 0.35, 2.0])
def test_constant_rate_against_the_oracle(eng, tts_sd, noise, oracle_inputs, r):
    from oracle import flow as oflow
    mu, spks, cond, lens = oracle_inputs
    with eng.guidance([r]):
        mel = eng.cfm_solve(mu, lens, spks, cond, 3, t_span=span(3)).cpu()

    def want(b, L):
        with torch.inference_mode():
            return oflow.cfm_solve(tts_sd, noise, mu[b:b + 1, :, :L], torch.ones(1, 1, L), spks[b:b + 1], cond[b:b + 1, :, :L], 3, 1.0,
                                   cfg_rate=r)[0]
    check_vs_reference(mel, want, oracle_bound(r), f"constant rate {r}")


@pytest.mark.parametrize("sched", ["cosine", "linear"])
def test_schedule_against_the_restated_solver(eng, tts_sd, noise, oracle_inputs, sched):
    mu, spks, cond, lens = oracle_inputs
    rates = [0.0, 1.5, 0.7, 0.0]
    with eng.guidance(rates):
        mel = eng.cfm_solve(mu, lens, spks, cond, 4, t_span=span(4, sched)).cpu()

    def want(b, L):
        with torch.inference_mode():
            return guidance_ref.cfm_solve(tts_sd, noise, mu[b:b + 1, :, :L], torch.ones(1, 1, L), spks[b:b + 1], cond[b:b + 1, :, :L], 4,
                                          1.0, rates=rates, t_scheduler=sched)[0]
    check_vs_reference(mel, want, oracle_bound(max(rates)), f"schedule {rates} {sched}")


# ---- 4. no-twin steps are taken, and equal keeping the twins ----------------------------------------------------------------------
def solve_arms(monkeypatch, tts_sd, noise, B, T, rates, seed):
    mu, spks, cond = inputs(B, T, seed)
    n = len(rates)

    def run(e):
        e.set_guidance(rates)
        mel = e.cfm_solve(mu, None, spks, cond, n).cpu()
        return mel, profiled(lambda: e.cfm_solve(mu, None, spks, cond, n))
    return {drop: arm(monkeypatch, tts_sd, noise, drop, B, T, run) for drop in (True, False)}


def assert_step_frames(report, steps, want_frames):
    """the fused-block launches of the solve account for sum(want_frames) frames: the same launches in every step"""
    n, frames = block_frames(report)
    assert n % steps == 0, (n, steps)
    want = (n // steps) * sum(want_frames)
    assert abs(frames - want) <= 1e-6 * want, (frames / (n // steps), want_frames, sorted(report))


def test_no_twin_solve_row_owning(monkeypatch, tts_sd, noise):
    """rate 0 at B = 12, T = 200, n = 3: 2 452 rows without twins, 4 900 with, row-owning both ways"""
    B, T = 12, 200
    out = solve_arms(monkeypatch, tts_sd, noise, B, T, [0.0] * 3, 520)
    e = md(out[True][0], out[False][0])
    print(f"no twins vs twins kept, B = {B}, T = {T}: {e:.3e}")
    assert torch.isfinite(out[True][0]).all() and e <= GEOMETRY_BOUND, e
    assert_step_frames(out[True][1], 3, [B * T] * 3)
    assert_step_frames(out[False][1], 3, [(B + 1) * T] + [2 * B * T] * 2)      # (twins kept: the shared first step is taken as ever)


def test_no_twin_solve_split_k(monkeypatch, tts_sd, noise):
    """rate 0 at B = 1, T = 61, n = 3: 69 rows against 134, both on the tile kernels (no fused-block launch to count: the
    profiler's algorithmic flops, proportional to the frames of every launch but the three of the time embedding, halve)"""
    out = solve_arms(monkeypatch, tts_sd, noise, 1, 61, [0.0] * 3, 521)
    e = md(out[True][0], out[False][0])
    print(f"no twins vs twins kept, B = 1, T = 61: {e:.3e}")
    assert torch.isfinite(out[True][0]).all() and e <= GEOMETRY_BOUND, e
    flops = {drop: sum(v["flops"] for v in out[drop][1].values()) for drop in (True, False)}
    assert flops[False] > 0 and abs(flops[True] / flops[False] - 0.5) <= 0.01, flops


def test_guidance_window_switches_geometry_between_steps(monkeypatch, tts_sd, noise):
    """window [0.7, 0.7, 0, 0] at B = 12, T = 200: (B + 1) T frames in the shared first step, 2 B T in the second, B T in the two
    steps without guidance; with the twins kept, 2 B T there as well"""
    B, T = 12, 200
    out = solve_arms(monkeypatch, tts_sd, noise, B, T, [0.7, 0.7, 0.0, 0.0], 522)
    e = md(out[True][0], out[False][0])
    print(f"window, twins dropped vs kept, B = {B}, T = {T}: {e:.3e}")
    assert torch.isfinite(out[True][0]).all() and e <= GEOMETRY_BOUND, e
    assert_step_frames(out[True][1], 4, [(B + 1) * T, 2 * B * T, B * T, B * T])
    assert_step_frames(out[False][1], 4, [(B + 1) * T] + [2 * B * T] * 3)


def test_no_twin_step_before_the_first_step_with_twins(monkeypatch, tts_sd, noise):
    """rates [0, 0.7, 0.7, 0] at B = 12, T = 200: the solve STARTS on B samples, so the first 2 B step finds the conditional slots'
    running maxima advanced and the twin slots' still at 0 -- its writers raise them before any reader derives a scale from them,
    as in the first step of any solve.  No twin exists in step 0, so none is shared: B T, 2 B T, 2 B T, B T frames; with the twins
    kept the shared first step runs as ever"""
    B, T = 12, 200
    out = solve_arms(monkeypatch, tts_sd, noise, B, T, [0.0, 0.7, 0.7, 0.0], 523)
    e = md(out[True][0], out[False][0])
    print(f"no-twin step first, twins dropped vs kept, B = {B}, T = {T}: {e:.3e}")
    assert torch.isfinite(out[True][0]).all() and e <= GEOMETRY_BOUND, e
    assert_step_frames(out[True][1], 4, [B * T, 2 * B * T, 2 * B * T, B * T])
    assert_step_frames(out[False][1], 4, [(B + 1) * T] + [2 * B * T] * 3)


# ---- 5. ragged ----------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_without_twins(eng):
    B, T, lens = 4, 200, [200, 120, 90, 60]
    mu, spks, cond = inputs(B, T, 530)
    lt = torch.tensor(lens, dtype=torch.int32)
    mask = (torch.arange(T)[None] < lt[:, None]).unsqueeze(1).float()
    mu, cond = mu * mask, cond * mask
    with eng.guidance([0.0]):
        mel = eng.cfm_solve(mu, lt, spks, cond, 2).cpu()
        for b, L in enumerate(lens):
            one = eng.cfm_solve(mu[b:b + 1, :, :L].contiguous(), None, spks[b:b + 1], cond[b:b + 1, :, :L].contiguous(), 2).cpu()
            e = md(mel[b, :, :L], one[0])
            print(f"ragged rate 0, utterance {b}: {e:.3e}")
            assert torch.isfinite(mel[b]).all() and e <= GEOMETRY_BOUND, (b, e)
            if L < T:
                assert float(mel[b, :, L:].abs().max()) == 0.0, b


# ---- 6. the other routes ------------------------------------------------------------------------------------------------------------
def test_prompted_solve_reads_the_mode_and_leaves_the_default(eng):
    g = torch.Generator().manual_seed(540)
    p, y = [20, 35], [40, 28]
    mu_y, spks = torch.randn(2, 80, 40, generator=g), torch.randn(2, 80, generator=g)
    ph, pf = torch.randn(2, 35, 80, generator=g), torch.randn(2, 35, 80, generator=g)
    args = (mu_y, torch.tensor(y), ph, pf, torch.tensor(p), spks, 3)
    default = eng.cfm_solve_prompted(*args).cpu()
    with eng.guidance([1.5]):
        mel = eng.cfm_solve_prompted(*args).cpu()
        for b in range(2):
            mu = torch.cat([ph[b:b + 1, :p[b]].transpose(1, 2), mu_y[b:b + 1, :, :y[b]]], dim=2).contiguous()
            cond = torch.cat([pf[b:b + 1, :p[b]].transpose(1, 2), torch.zeros(1, 80, y[b])], dim=2).contiguous()
            one = eng.cfm_solve(mu, None, spks[b:b + 1], cond, 3).cpu()[0, :, p[b]:]
            e = md(mel[b, :, :y[b]], one)
            print(f"prompted r = 1.5, utterance {b}: {e:.3e}")
            assert e <= GEOMETRY_BOUND, (b, e)
    assert not torch.equal(mel, default)                                      # (the mode did apply)
    assert torch.equal(eng.cfm_solve_prompted(*args).cpu(), default)          # ... and 0.7 is back behind the block


def test_token2mel_streaming_without_twins(monkeypatch, prompt_sd, tts_sd):
    """flow.inference(batched=True, streaming=True, cfg_rate=0) on the three short utterances of token2mel_cases: twins dropped
    against kept; the decoder's default rate is back after the call"""
    from jyutvoice_amd.flow.flow import CausalMaskedDiffWithXvec
    from jyutvoice_amd.runtime import Runtime
    sd = tc.flow_sd(prompt_sd, tts_sd)
    c = tc.BATCH
    tok, ptok, feat, emb = tc.batch_inputs()
    call = (tok, torch.tensor(c["n"]), ptok, torch.tensor(c["p"]), feat, torch.tensor(c["f"]), emb, True, True)
    got = {}
    for drop in (True, False):
        if drop:
            monkeypatch.delenv("JV_NO_TWIN_DROP", raising=False)
        else:
            monkeypatch.setenv("JV_NO_TWIN_DROP", "1")
        m = CausalMaskedDiffWithXvec(vocab_size=6561, input_frame_rate=25, runtime=Runtime("cuda:0"))
        m.load_state_dict(sd)
        before = m.inference(*call, batched=True, n_timesteps=tc.N_TIMESTEPS)[0].cpu()
        got[drop] = m.inference(*call, batched=True, n_timesteps=tc.N_TIMESTEPS, cfg_rate=0)[0].cpu()
        after = m.inference(*call, batched=True, n_timesteps=tc.N_TIMESTEPS)[0].cpu()
        assert torch.equal(before, after) and not torch.equal(before, got[drop])
        m._rt().engine.close()
    e = md(got[True], got[False])
    print(f"token2mel streaming rate 0, twins dropped vs kept: {e:.3e}")
    assert torch.isfinite(got[True]).all() and e <= GEOMETRY_BOUND, e


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_mode_and_the_bits(eng):
    from jyutvoice_amd._lib import JvError
    mu, spks, cond = inputs(1, 61, 550)
    base = eng.cfm_solve(mu, None, spks, cond, 3).cpu()
    for bad in ([-0.1], [0.7, float("nan"), 0.7], [float("inf")], [0.7, -1.0]):
        with pytest.raises(JvError, match="finite and >= 0"):
            eng.set_guidance(bad)
    assert torch.equal(eng.cfm_solve(mu, None, spks, cond, 3).cpu(), base)      # a refused mode changes nothing
    try:
        eng.set_guidance([0.7, 0.7])
        with pytest.raises(JvError, match="n_timesteps = 3.*holds 2 rates"):
            eng.cfm_solve(mu, None, spks, cond, 3)
        assert torch.equal(eng.cfm_solve(mu, None, spks, cond, 2).cpu(), eng.cfm_solve(mu, None, spks, cond, 2).cpu())
    finally:
        eng.set_guidance(None)
    assert torch.equal(eng.cfm_solve(mu, None, spks, cond, 3).cpu(), base)
