"""CPU: the host side of the midpoint / Heun solvers -- the restated loop of solver_ref.py is `guidance_ref.cfm_solve` (and so the
oracle) bit for bit on "euler", `step_table` lays a second-order request out per estimator evaluation, a `SynthServer` over a stub
engine takes a request of a second-order solver through two pool steps per solver step and finishes it after its last stage,
every public entry refuses an unknown solver by naming the choices, and the new C-ABI entries are declared and bound."""
import re

import numpy as np
import pytest
import torch

import guidance_ref
import solver_ref
from jyutvoice_amd import _lib, spec
from jyutvoice_amd.flow.flow_matching import (EVALS, SOLVERS, CausalConditionalCFM, check_solver, decoder_settings,
                                              resolve_solver)
from jyutvoice_amd.serve import MAX_STEPS, SynthServer, step_table
from test_abi import HEADER, declared_symbols
from test_serve_host import StubEngine, StubHift, StubTts, request

STAGES = {"euler": [_lib.STAGE_EULER], "midpoint": [_lib.STAGE_MID1, _lib.STAGE_MID2], "heun": [_lib.STAGE_HEUN1, _lib.STAGE_HEUN2]}


# ---- the restated solver ------------------------------------------------------------------------------------------------------------
def small_inputs():
    g = torch.Generator().manual_seed(12)
    B, T = 2, 12
    mu, spks, cond = torch.randn(B, 80, T, generator=g), torch.randn(B, 80, generator=g), torch.randn(B, 80, T, generator=g) * 0.3
    mask = (torch.arange(T)[None] < torch.tensor([T, 7])[:, None]).unsqueeze(1).float()
    return mu, mask, spks, cond


@pytest.mark.parametrize("sched", ["cosine", "linear"])
def test_restated_euler_is_the_guidance_reference_and_the_oracle(tts_sd, noise, sched):
    from oracle import flow as oflow
    mu, mask, spks, cond = small_inputs()
    rates = [0.0, 1.5]
    with torch.inference_mode():
        got = solver_ref.cfm_solve(tts_sd, noise, mu, mask, spks, cond, 2, 1.0, rates=rates, t_scheduler=sched, solver="euler")
        assert torch.equal(got, guidance_ref.cfm_solve(tts_sd, noise, mu, mask, spks, cond, 2, 1.0, rates=rates, t_scheduler=sched))
        if sched == "cosine":
            assert torch.equal(solver_ref.cfm_solve(tts_sd, noise, mu, mask, spks, cond, 2), oflow.cfm_solve(tts_sd, noise, mu, mask, spks, cond, 2))


@pytest.mark.parametrize("solver", ["midpoint", "heun"])
def test_restated_second_order_evaluates_at_the_tabled_times_and_differs(tts_sd, noise, solver):
    """the loop evaluates the estimator at exactly the times `step_table` lists, twice per step, and is another mel than Euler's"""
    mu, mask, spks, cond = small_inputs()
    times = []
    with torch.inference_mode():
        got = solver_ref.cfm_solve(tts_sd, noise, mu, mask, spks, cond, 2, solver=solver, times=times)
        euler = solver_ref.cfm_solve(tts_sd, noise, mu, mask, spks, cond, 2)
    assert times == step_table(2, "cosine", solver)[0]
    assert torch.isfinite(got).all() and float((got - euler).abs().max()) > 1e-3


# ---- step_table -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", ["cosine", "linear"])
@pytest.mark.parametrize("n", [1, 2, 3, 10, 33])
def test_step_table_per_evaluation(n, sched):
    f32 = np.float32
    tt, dts = step_table(n, sched)
    assert step_table(n, sched, "euler") == (tt, dts) == step_table(n, sched, solver="euler")      # today's rows, exactly
    for solver in ("midpoint", "heun"):
        t2, c2, s2 = step_table(n, sched, solver)
        assert len(t2) == len(c2) == len(s2) == 2 * n
        assert s2 == STAGES[solver] * n
        for v in t2 + c2:
            assert float(f32(v)) == v                                       # fp32 values
        for k in range(n):
            t, dt = f32(tt[k]), f32(dts[k])
            half = f32(f32(0.5) * dt)
            assert t2[2 * k] == tt[k]
            if solver == "midpoint":
                assert t2[2 * k + 1] == float(f32(t + half)) and (c2[2 * k], c2[2 * k + 1]) == (float(half), dts[k])
            else:
                assert t2[2 * k + 1] == float(f32(t + dt)) and (c2[2 * k], c2[2 * k + 1]) == (dts[k], float(half))
                if k + 1 < n:
                    assert t2[2 * k + 1] == tt[k + 1]                       # Heun's second time is the next step's t
        if solver == "heun":
            assert abs(t2[-1] - 1.0) < 1e-6
    for bad in ("rk4", None, 2, "Euler"):
        with pytest.raises(ValueError, match=r"solver must be one of \['euler', 'midpoint', 'heun'\]"):
            step_table(n, sched, bad)


def test_stage_codes_are_the_headers():
    text = open(HEADER).read()
    for name, code in (("EULER", _lib.STAGE_EULER), ("MID1", _lib.STAGE_MID1), ("MID2", _lib.STAGE_MID2), ("HEUN1", _lib.STAGE_HEUN1),
                       ("HEUN2", _lib.STAGE_HEUN2)):
        assert re.search(rf"#define JV_STAGE_{name} {code}\b", text), name
    for name, code in _lib.SOLVERS.items():
        assert re.search(rf"#define JV_SOLVER_{name.upper()} {code}\b", text), name
    assert tuple(_lib.SOLVERS) == SOLVERS and EVALS == {"euler": 1, "midpoint": 2, "heun": 2}


# ---- the server over a stub engine ----------------------------------------------------------------------------------------------------
class StageStub(StubEngine):
    def cfm_pool_step(self, pool, slots, lens, t, dt, cfg=None, stage=None):
        self.calls.append(("step", list(slots), list(lens), list(t), list(dt), None if cfg is None else list(cfg),
                           None if stage is None else list(stage)))


def test_server_takes_every_request_through_the_stages_of_its_own_solver():
    """six requests, mixed solvers, n = 2 / 3, three slots, arrivals staggered by one step: request i takes exactly n_i * evals_i pool
    steps, each at the (t, coefficient, stage) row of its own table and at its step's rate, then leaves"""
    eng = StageStub()
    server = SynthServer(StubTts(), StubHift(), max_sessions=3, max_frames=128, max_tokens=32, engine=eng)
    specs = [("midpoint", 2, {}), ("euler", 3, {}), ("heun", 3, {"cfg_rate": 1.5, "cfg_window": (0.0, 0.5), "t_scheduler": "linear"}),
             ("heun", 2, {}), ("euler", 2, {"cfg_rate": 0.0}), ("midpoint", 3, {"t_scheduler": "linear"})]
    tokens = [8 + i for i in range(len(specs))]
    finished_at, submitted_at, t = {}, {}, 0
    while len(finished_at) < len(specs):
        if t < len(specs):
            solver, n, kw = specs[t]
            args, _ = request(tokens[t])
            submitted_at[server.submit(*args, n_timesteps=n, solver=solver, **kw)] = t
        out = server.step()
        t += 1
        assert t < 60
        for rid in out:
            finished_at[rid] = t
    owner, rows = {}, {rid: [] for rid in range(len(specs))}
    for c in eng.calls:
        if c[0] == "admit":
            for s, y in zip(c[1], c[2]):
                owner[s] = tokens.index(y // 2)
        elif c[0] == "step":
            _, slots, lens, ts, cs, cfg, stage = c
            live_stages = []
            for i, s in enumerate(slots):
                rid = owner[s]
                k = len(rows[rid])
                live_stages.append(STAGES[specs[rid][0]][k % EVALS[specs[rid][0]]])
                rows[rid].append((ts[i], cs[i], None if stage is None else stage[i], None if cfg is None else cfg[i]))
            # every live request on an Euler stage: the entries that existed before take the step
            assert (stage is None) == all(v == _lib.STAGE_EULER for v in live_stages), (live_stages, stage)
            if stage is not None:
                assert stage == live_stages and cfg is not None
    for rid, (solver, n, kw) in enumerate(specs):
        sched = kw.get("t_scheduler", "cosine")
        table = step_table(n, sched, solver)
        assert len(rows[rid]) == n * EVALS[solver] == len(table[0])        # finished after its last stage, not before
        rates = server_rates(n, kw, sched)
        for k, (tv, cv, sv, rv) in enumerate(rows[rid]):
            assert (tv, cv) == (table[0][k], table[1][k])
            assert sv in (None, STAGES[solver][k % EVALS[solver]])
            if rv is not None:
                assert rv == rates[k // EVALS[solver]]                       # a step's rate holds for both of its evaluations
    assert sorted(finished_at) == list(range(len(specs)))


def server_rates(n, kw, sched):
    from jyutvoice_amd.serve import guidance_rates
    return guidance_rates(n, kw.get("cfg_rate", spec.CFG_RATE), kw.get("cfg_window"), sched)


def test_all_euler_server_still_uses_the_old_entry():
    eng = StubEngine()                                                      # (its cfm_pool_step takes neither cfg nor stage)
    server = SynthServer(StubTts(), StubHift(), max_sessions=2, max_frames=64, max_tokens=16, engine=eng)
    args, _ = request(8)
    server.submit(*args, n_timesteps=2)
    server.submit(*args, n_timesteps=3, solver="euler")
    assert sorted(server.drain()) == [0, 1] and server.steps == 3


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
CHOICES = r"solver must be one of \['euler', 'midpoint', 'heun'\]"


def test_unknown_solver_is_refused_everywhere_on_the_host():
    for bad in ("rk4", "", "HEUN", 1, True, 0.5):
        with pytest.raises(ValueError, match=CHOICES):
            check_solver("t()", bad)
        with pytest.raises(ValueError, match=CHOICES):
            resolve_solver("t()", "euler", bad)
    assert resolve_solver("t()", "heun") == "heun" and resolve_solver("t()", "heun", "midpoint") == "midpoint"
    with pytest.raises(ValueError, match=CHOICES):
        resolve_solver("t()", "rk4")                                        # a bad configured name is caught too
    params = {"t_scheduler": "cosine", "inference_cfg_rate": 0.7}
    assert CausalConditionalCFM(240, params, spk_emb_dim=80).solver == "euler"
    assert CausalConditionalCFM(240, dict(params, solver="heun"), spk_emb_dim=80).solver == "heun"
    with pytest.raises(ValueError, match=CHOICES):
        CausalConditionalCFM(240, dict(params, solver="rk4"), spk_emb_dim=80)
    assert decoder_settings(None) == (spec.CFG_RATE, "cosine", "euler")
    assert decoder_settings(CausalConditionalCFM(240, dict(params, solver="midpoint"), spk_emb_dim=80))[2] == "midpoint"


def test_submit_validates_the_solver_and_names_the_request():
    server = SynthServer(StubTts(), StubHift(), max_sessions=2, max_frames=64, max_tokens=16, engine=StageStub())
    good, _ = request(8)
    with pytest.raises(ValueError, match=CHOICES) as e:
        server.submit(*good, solver="rk4")
    assert "SynthServer.submit(): request 0" in str(e.value)
    with pytest.raises(ValueError, match=f"n_timesteps = 513 with the heun solver is 1026 estimator evaluations, the limit is {MAX_STEPS}"):
        server.submit(*good, n_timesteps=513, solver="heun")
    assert server.pending() == 0
    server.submit(*good, n_timesteps=512, solver="midpoint")               # 1024 evaluations: the limit itself
    assert server.pending() == 1


def test_infer_cli_knows_the_solver():
    import argparse

    import infer
    ns = dict(t_scheduler=None, cfg_window=None, cfg_rate=None, n_timesteps=5)
    assert infer.guidance_kw(argparse.Namespace(solver="midpoint", **ns), None) == {"solver": "midpoint"}
    assert infer.guidance_kw(argparse.Namespace(solver=None, **ns), None) == {}      # not given: the decoder's setting holds
    with pytest.raises(SystemExit) as e:                                             # refused by the parser, before any device work
        infer.main(["--synthetic", "40", "--output", "unused.wav", "--solver", "rk4"])
    assert e.value.code == 2


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_bound():
    assert {"jv_flow_set_solver", "jv_cfm_pool_step_s"} <= set(declared_symbols())
    lib = _lib.load()
    assert len(_lib.SIGNATURES["jv_flow_set_solver"][1]) == 2
    assert len(_lib.SIGNATURES["jv_cfm_pool_step_s"][1]) == len(_lib.SIGNATURES["jv_cfm_pool_step_g"][1]) + 3 == 18
    assert lib.jv_flow_set_solver(None, 0) != 0                             # a null context is an error, not a crash
    assert "flow_matching.py:215-265" in open(HEADER).read().split("jv_flow_set_solver:")[1].split("*/")[0]
