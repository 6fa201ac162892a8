"""CPU: the host side of per-request / per-step guidance -- the configuration mirror takes any rate >= 0 and the linear scheduler,
`step_table` knows the linear schedule, `guidance_rates` places a window on the steps' t, `SynthServer.submit` validates and keeps
a request's rates and hands them to the pool step (over a stub engine), the restated solver of guidance_ref.py is the oracle's bit
for bit, and the two new C-ABI entries are declared and bound."""
import math

import numpy as np
import pytest
import torch

import guidance_ref
from jyutvoice_amd import _lib, spec
from jyutvoice_amd.flow.flow_matching import CausalConditionalCFM, resolve_guidance, time_span
from jyutvoice_amd.serve import SynthServer, guidance_rates, step_table
from test_serve_host import StubEngine, StubHift, StubTts, request


def cfm(rate, sched="cosine", spk=80):
    return CausalConditionalCFM(240, {"t_scheduler": sched, "inference_cfg_rate": rate, "training_cfg_rate": 0.2}, spk_emb_dim=spk)


# ---- the mirror -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0, 0.35, 0.7, 2.0])
@pytest.mark.parametrize("sched", ["cosine", "linear"])
def test_mirror_accepts_any_rate_and_both_schedulers(rate, sched):
    d = cfm(rate, sched)
    assert d.inference_cfg_rate == float(rate) and d.t_scheduler == sched


def test_mirror_still_refuses_what_the_library_cannot_do():
    for bad in (-0.1, float("nan"), float("inf"), "0.7", None, True):
        with pytest.raises((ValueError, NotImplementedError)):
            cfm(bad)
    with pytest.raises(NotImplementedError):
        cfm(0.7, "sigmoid")
    with pytest.raises(NotImplementedError):
        cfm(0.7, spk=64)


def test_resolve_guidance():
    who = "t()"
    assert resolve_guidance(who, 4, 0.7) is None                       # the library's default: nothing to set
    assert resolve_guidance(who, 4, 0.35) == [0.35]                    # the decoder's configured rate
    assert resolve_guidance(who, 4, 0.35, cfg_rate=0.7) is None        # a per-call rate wins over it
    assert resolve_guidance(who, 4, 0.7, cfg_rate=0) == [0.0]
    assert resolve_guidance(who, 3, 0.7, cfg_rate=2.0, cfg_schedule=[0, 1.5, 0.7]) == [0.0, 1.5, 0.7]      # a schedule wins over both
    assert resolve_guidance(who, 2, 0.7, cfg_schedule=torch.tensor([0.7, 0.7])) == pytest.approx([0.7, 0.7])
    with pytest.raises(ValueError, match="3 rates, n_timesteps = 4"):
        resolve_guidance(who, 4, 0.7, cfg_schedule=[0, 1, 2])
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite number >= 0"):
            resolve_guidance(who, 2, 0.7, cfg_rate=bad)
        with pytest.raises(ValueError, match="finite number >= 0"):
            resolve_guidance(who, 2, 0.7, cfg_schedule=[0.7, bad])


# ---- schedules --------------------------------------------------------------------------------------------------------------------
def linear_recurrence(n):
    """ConditionalCFM.solve_euler's running (t, dt) (flow_matching.py:230, 260-263) over t_span = linspace(0, 1, n + 1), on fp32
    tensors as the reference computes it"""
    ts = torch.linspace(0, 1, n + 1, dtype=torch.float32)
    t, dt = ts[0], ts[1] - ts[0]
    tt, dts = [], []
    for step in range(1, n + 1):
        tt.append(float(t))
        dts.append(float(dt))
        t = t + dt
        if step < n:
            dt = ts[step + 1] - t
    return tt, dts


@pytest.mark.parametrize("n", [1, 2, 3, 4, 10, 32])
def test_step_table_linear_is_the_fp32_recurrence_over_linspace(n):
    tt, dts = step_table(n, "linear")
    assert (tt, dts) == linear_recurrence(n)
    assert (tt, dts) == step_table(n, t_scheduler="linear")
    for v in tt + dts:
        assert float(np.float32(v)) == v
    assert tt[0] == 0.0 and abs(tt[-1] + dts[-1] - 1.0) < 1e-6
    assert step_table(n) == step_table(n, "cosine")                     # the default is the cosine schedule, unchanged
    assert torch.equal(time_span(n, "linear"), torch.linspace(0, 1, n + 1))
    assert torch.equal(time_span(n), 1 - torch.cos(torch.linspace(0, 1, n + 1) * 0.5 * torch.pi))
    with pytest.raises(ValueError, match="t_scheduler"):
        step_table(n, "sigmoid")


# ---- windows ----------------------------------------------------------------------------------------------------------------------
def test_guidance_rates_window_edges():
    tt, _ = step_table(4, "linear")                                      # t = 0, 0.25, 0.5, 0.75
    assert tt == [0.0, 0.25, 0.5, 0.75]
    assert guidance_rates(4, 1.5, None, "linear") == [1.5] * 4
    assert guidance_rates(4, 1.5, (0.25, 0.75), "linear") == [0.0, 1.5, 1.5, 0.0]      # closed at t_lo, open at t_hi
    assert guidance_rates(4, 1.5, (0.0, 0.5), "linear") == [1.5, 1.5, 0.0, 0.0]
    assert guidance_rates(4, 1.5, (0.0, 1.0), "linear") == [1.5] * 4
    assert guidance_rates(4, 1.5, (0.25, math.nextafter(0.25, 1.0)), "linear") == [0.0, 1.5, 0.0, 0.0]
    assert guidance_rates(4, 1.5, (0.5, 0.5), "linear") == [0.0] * 4     # an empty window
    assert guidance_rates(4, 1.5, (0.75, 0.25), "linear") == [0.0] * 4
    assert guidance_rates(4, 0, (0.0, 1.0)) == [0.0] * 4
    # the window is placed on the steps' t as step_table computes it: the cosine schedule's t differ from the linear one's
    tc, _ = step_table(4)
    assert guidance_rates(4, 0.7, (tc[1], tc[3])) == [0.0, 0.7, 0.7, 0.0]
    assert guidance_rates(4, 0.7, (0.25, 0.75)) == [0.7 if 0.25 <= t < 0.75 else 0.0 for t in tc]


def test_guidance_rates_one_step_and_errors():
    assert guidance_rates(1, 2.0) == [2.0]
    assert guidance_rates(1, 2.0, (0.0, 0.1)) == [2.0]                   # the one step is at t = 0
    assert guidance_rates(1, 2.0, (0.1, 1.0)) == [0.0]
    for bad in (-0.5, float("nan"), float("inf"), "1", None):
        with pytest.raises(ValueError, match="rate"):
            guidance_rates(3, bad)
    for bad in ((0.1,), (0.1, float("nan")), "ab", 0.5, (0.1, 0.2, 0.3)):
        with pytest.raises(ValueError, match="window"):
            guidance_rates(3, 0.7, bad)
    with pytest.raises(ValueError):
        guidance_rates(0, 0.7)
    with pytest.raises(ValueError, match="t_scheduler"):
        guidance_rates(3, 0.7, None, "sigmoid")


# ---- the server -------------------------------------------------------------------------------------------------------------------
class GuidanceStub(StubEngine):
    def cfm_pool_step(self, pool, slots, lens, t, dt, cfg=None):
        self.calls.append(("step", list(slots), list(lens), list(t), list(dt), None if cfg is None else list(cfg)))


def test_submit_validates_guidance_and_names_the_request():
    server = SynthServer(StubTts(), StubHift(), max_sessions=2, max_frames=64, max_tokens=16, engine=GuidanceStub())
    good, _ = request(8)
    for kw, text in (({"cfg_rate": -0.1}, "cfg_rate must be a finite number >= 0"),
                     ({"cfg_rate": float("nan")}, "cfg_rate must be a finite number >= 0"),
                     ({"cfg_rate": float("inf")}, "cfg_rate must be a finite number >= 0"),
                     ({"cfg_rate": "0.7"}, "cfg_rate must be a finite number >= 0"),
                     ({"cfg_window": (0.2,)}, "cfg_window must be a pair of finite numbers"),
                     ({"cfg_window": (0.2, float("nan"))}, "cfg_window must be a pair of finite numbers"),
                     ({"cfg_window": 0.5}, "cfg_window must be a pair of finite numbers"),
                     ({"t_scheduler": "sigmoid"}, "t_scheduler must be one of")):
        with pytest.raises(ValueError, match=text) as e:
            server.submit(*good, **kw)
        assert "SynthServer.submit(): request 0" in str(e.value)
    assert server.pending() == 0


def test_server_passes_every_resident_request_its_own_rate_of_its_own_step():
    eng = GuidanceStub()
    server = SynthServer(StubTts(), StubHift(), max_sessions=3, max_frames=128, max_tokens=32, engine=eng)
    specs = [(3, {"cfg_rate": 0.0}), (4, {"cfg_rate": 2.0, "cfg_window": (0.0, 0.5), "t_scheduler": "linear"}), (2, {})]
    for i, (n, kw) in enumerate(specs):
        args, _ = request(8 + i)
        server.submit(*args, n_timesteps=n, **kw)
    server.drain()
    steps = [c for c in eng.calls if c[0] == "step"]
    assert len(steps) == 4
    want = {0: [0.0] * 3, 1: [2.0, 2.0, 0.0, 0.0], 2: [spec.CFG_RATE] * 2}
    tts = {0: step_table(3), 1: step_table(4, "linear"), 2: step_table(2)}
    for k, (_, slots, lens, t, dt, cfg) in enumerate(steps):
        assert cfg is not None and len(cfg) == len(slots)
        for s, tv, dv, r in zip(slots, t, dt, cfg):      # slot i holds request i: all three were admitted in the first step
            assert r == want[s][k] and (tv, dv) == (tts[s][0][k], tts[s][1][k])
    # all resident requests at the default rate: the entry without rates (what the stub of test_serve_host.py implements)
    eng2 = StubEngine()
    server = SynthServer(StubTts(), StubHift(), max_sessions=2, max_frames=64, max_tokens=16, engine=eng2)
    args, _ = request(8)
    server.submit(*args, n_timesteps=2)
    server.submit(*args, n_timesteps=2, cfg_rate=0.7)
    assert sorted(server.drain()) == [0, 1]


# ---- the restated solver ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0.0, 0.35, 0.7, 2.0])
def test_restated_solver_is_the_oracle_for_a_constant_schedule(tts_sd, noise, r):
    from oracle import flow as oflow
    g = torch.Generator().manual_seed(11)
    B, T, n = 2, 12, 2
    mu, spks, cond = torch.randn(B, 80, T, generator=g), torch.randn(B, 80, generator=g), torch.randn(B, 80, T, generator=g) * 0.3
    mask = (torch.arange(T)[None] < torch.tensor([T, 7])[:, None]).unsqueeze(1).float()
    with torch.inference_mode():
        want = oflow.cfm_solve(tts_sd, noise, mu, mask, spks, cond, n, 1.0, cfg_rate=r)
        got = guidance_ref.cfm_solve(tts_sd, noise, mu, mask, spks, cond, n, 1.0, rates=[r] * n)
        assert torch.equal(got, want)
        if r == 0.7:
            assert torch.equal(guidance_ref.cfm_solve(tts_sd, noise, mu, mask, spks, cond, n), want)
        other = guidance_ref.cfm_solve(tts_sd, noise, mu, mask, spks, cond, n, 1.0, rates=[r, r + 0.5])
        assert not torch.equal(other, want)                              # the rate of the second step is read


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_bound():
    lib = _lib.load()
    assert len(_lib.SIGNATURES["jv_flow_set_guidance"][1]) == 3
    assert len(_lib.SIGNATURES["jv_cfm_pool_step_g"][1]) == len(_lib.SIGNATURES["jv_cfm_pool_step"][1]) + 1 == 15
    assert lib.jv_flow_set_guidance(None, None, 0) != 0                 # a null context is an error, not a crash
