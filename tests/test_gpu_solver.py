"""GPU: the midpoint and Heun solvers of the closed CFM solves (jv_flow_set_solver; flow.hip solve_loop, rowops.hip
solver_stage_kernel; DESIGN.md 5 "Solver").

What is shown: each second-order solve IS the recurrence it says it is -- against the loop restated in fp64 (solver_ref.py), in every
route and geometry -- and Euler keeps its bits.  Nothing about quality per evaluation is claimed or tested.

Bounds.  Against the fp64 restated loop: `oracle_bound(max rate)` of test_gpu_guidance.py, unchanged -- what an Euler solve of the
same four evaluations is held to there.  Between two batch geometries of one solve (a batch row against its B = 1 run, compact
against padded, prompted against hand-concatenated, twins dropped against kept, embeddings ahead of the loop against per
evaluation, a streamed prefix against the one-shot mel): 2e-5.  Across the split-K seam: `oracle_bound`, as elsewhere.  torch.equal
where only the way Euler is selected differs.  Measured distances go to solver_parity.json in the output directory (JV_OUT;
committed under profiles/)."""
import pytest
import torch

import parity_util as pu
import solver_ref
import stream_ref as sr
import token2mel_cases as tc
from parity_util import md, profiled
from test_gpu_cfg_share import inputs
from test_gpu_guidance import GEOMETRY_BOUND, ORACLE_LENS, assert_step_frames, fresh_engine, oracle_bound, span

pytestmark = pytest.mark.gpu

record = pu.Recorder("solver_parity.json", {
    "what": "tests/test_gpu_solver.py: jv_cfm_solve under jv_flow_set_solver(midpoint / heun), n = 2 steps = 4 estimator evaluations, "
            "B = 2, T = 64, lengths [64, 41], against the same loop restated in fp64 (tests/solver_ref.py), max-abs per utterance "
            "over its own frames",
    "bound": "3e-4 max(1, (1 + 2 r) / 2.4) with r the largest rate of the solve: tests/test_gpu_guidance.py oracle_bound, unchanged",
    "euler": "the Euler solve of the same four evaluations (n = 4) on the same inputs against its own fp64 loop, for comparison"})


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


@pytest.fixture(scope="module")
def eng(tts_sd, noise):
    e = fresh_engine(tts_sd, noise, 12, 256)
    yield e
    e.close()


# ---- 1. the default keeps its bits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(1, 61), (12, 200)], ids=["split_k", "row_owning_shared_twin"])
def test_default_bits(eng, B, T):
    """mode unset = set_solver("euler") = a solve after a second-order solve has run and the mode was reset"""
    mu, spks, cond = inputs(B, T, 600 + B)
    base = eng.cfm_solve(mu, None, spks, cond, 3).cpu()
    eng.set_solver("euler")
    assert torch.equal(eng.cfm_solve(mu, None, spks, cond, 3).cpu(), base)
    for name in ("midpoint", "heun"):
        with eng.solver(name):
            other = eng.cfm_solve(mu, None, spks, cond, 2).cpu()
        assert torch.isfinite(other).all()
        again = eng.cfm_solve(mu, None, spks, cond, 3).cpu()
        assert torch.equal(again, base), (name, md(again, base))


def test_step_graph_replays_for_euler_only(eng, tts_sd, noise):
    """with step graphs switched on a second-order solve runs eagerly -- the bits of the eager context -- and the captured 2B Euler
    step keeps replaying for Euler solves before and after it (B = 12, T = 200: uniform rows, n > 1)"""
    mu, spks, cond = inputs(12, 200, 605)
    want = {}
    for name, n in (("euler", 3), ("midpoint", 2), ("heun", 2)):
        with eng.solver(name):
            want[name] = eng.cfm_solve(mu, None, spks, cond, n).cpu()
    e = fresh_engine(tts_sd, noise, 12, 200)
    try:
        e.set_step_graph(True)
        for name, n in (("euler", 3), ("euler", 3), ("midpoint", 2), ("euler", 3), ("heun", 2), ("euler", 3)):
            with e.solver(name):
                got = e.cfm_solve(mu, None, spks, cond, n).cpu()
            assert torch.equal(got, want[name]), (name, md(got, want[name]))
    finally:
        e.close()


# ---- 2. against the fp64 restated loop ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_inputs():
    mu, spks, cond = inputs(2, 64, 611)
    lens = torch.tensor(ORACLE_LENS, dtype=torch.int32)
    mask = (torch.arange(64)[None] < lens[:, None]).unsqueeze(1).float()
    return mu * mask, spks, cond * mask, lens


@pytest.fixture(scope="module")
def sd64(tts_sd):
    return {k: v.double() for k, v in tts_sd.items() if k.startswith("decoder.")}


def fp64_loop(sd64, noise, mu, spks, cond, b, L, n, rates, sched, solver):
    with torch.inference_mode():
        return solver_ref.cfm_solve(sd64, noise.double(), mu[b:b + 1, :, :L].double(), torch.ones(1, 1, L, dtype=torch.float64),
                                    spks[b:b + 1].double(), cond[b:b + 1, :, :L].double(), n, 1.0, rates=rates, t_scheduler=sched,
                                    solver=solver)[0]


@pytest.mark.parametrize("sched", ["cosine", "linear"])
@pytest.mark.parametrize("rates", [[0.7, 0.7], [0.0, 1.5]], ids=["rate_0.7", "rates_0_1.5"])
@pytest.mark.parametrize("solver", ["midpoint", "heun"])
def test_second_order_against_the_fp64_restated_loop(eng, sd64, noise, oracle_inputs, solver, rates, sched):
    mu, spks, cond, lens = oracle_inputs
    bound = oracle_bound(max(rates))
    with eng.guidance(rates), eng.solver(solver):
        mel = eng.cfm_solve(mu, lens, spks, cond, 2, t_span=span(2, sched)).cpu()
    tag = f"{solver} {sched} rates {rates}"
    worst = 0.0
    for b, L in enumerate(ORACLE_LENS):
        assert torch.isfinite(mel[b]).all()
        if L < mel.shape[2]:
            assert float(mel[b, :, L:].abs().max()) == 0.0, (tag, b)      # frames behind a length are exactly 0
        e = md(mel[b, :, :L], fp64_loop(sd64, noise, mu, spks, cond, b, L, 2, rates, sched, solver))
        record(tag, **{f"utterance_{b}": e, "bound": bound})
        worst = max(worst, e)
    assert worst <= bound, (tag, worst, bound)


def test_euler_of_equal_evaluations_on_the_same_inputs(eng, sd64, noise, oracle_inputs):
    """the comparison figure: n = 4 Euler steps (four evaluations) on the inputs above, against its own fp64 loop, same bound"""
    mu, spks, cond, lens = oracle_inputs
    mel = eng.cfm_solve(mu, lens, spks, cond, 4, t_span=span(4)).cpu()
    for b, L in enumerate(ORACLE_LENS):
        e = md(mel[b, :, :L], fp64_loop(sd64, noise, mu, spks, cond, b, L, 4, [0.7] * 4, "cosine", "euler"))
        record("euler cosine rate 0.7, n = 4", **{f"utterance_{b}": e, "bound": oracle_bound(0.7)})
        assert e <= oracle_bound(0.7), (b, e)


# ---- 3. the solver really differs ---------------------------------------------------------------------------------------------------
def test_the_three_solvers_give_three_mels(eng):
    mu, spks, cond = inputs(2, 64, 612)
    got = {}
    for name in ("euler", "midpoint", "heun"):
        with eng.solver(name):
            got[name] = eng.cfm_solve(mu, None, spks, cond, 2).cpu()
    for a, b in (("euler", "midpoint"), ("euler", "heun"), ("midpoint", "heun")):
        e = md(got[a], got[b])
        print(f"{a} vs {b}: {e:.3e}")
        assert e > 1e-3, (a, b, e)


# ---- 4. geometry --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["midpoint", "heun"])
def test_batch_row_against_its_own_run(eng, solver):
    B, T = 12, 200
    mu, spks, cond = inputs(B, T, 620)
    with eng.solver(solver):
        mel = eng.cfm_solve(mu, None, spks, cond, 2).cpu()
        for b in (0, 7):
            one = eng.cfm_solve(mu[b:b + 1].contiguous(), None, spks[b:b + 1], cond[b:b + 1].contiguous(), 2).cpu()
            e = md(mel[b], one[0])
            print(f"{solver}, row {b} of B = {B}, T = {T} vs B = 1: {e:.3e}")
            assert torch.isfinite(mel[b]).all() and e <= GEOMETRY_BOUND, (b, e)


RAGGED = {  # lengths, the utterances compared with their B = 1 run, is the compact geometry taken?
    # 1 636 uniform rows: below the 2 048-row seam the tile kernels run, which know the uniform (padded) geometry only
    "four_padded": ([200, 120, 90, 60], (0, 1, 2, 3), False),
    # 4 900 uniform rows against 4 + 2 (2 060 + 48) = 4 220 compact ones (86 %): row-owning, compact
    "twelve_compact": ([200] * 8 + [150, 120, 100, 90], (0, 8, 11), True),
}


@pytest.mark.parametrize("case", sorted(RAGGED))
@pytest.mark.parametrize("solver", ["midpoint", "heun"])
def test_ragged_batch(eng, solver, case):
    lens, compare, compact = RAGGED[case]
    B, T = len(lens), 200
    mu, spks, cond = inputs(B, T, 621)
    lt = torch.tensor(lens, dtype=torch.int32)
    mask = (torch.arange(T)[None] < lt[:, None]).unsqueeze(1).float()
    mu, cond = mu * mask, cond * mask
    with eng.solver(solver):
        mel = eng.cfm_solve(mu, lt, spks, cond, 2).cpu()
        if compact:      # the fused-block launches of all four evaluations account for the real frames (and their twins) only
            assert pu.solve_frames(profiled(lambda: eng.cfm_solve(mu, lt, spks, cond, 2))) == 2 * sum(lens)
        for b, L in enumerate(lens):
            if b not in compare:
                assert torch.isfinite(mel[b]).all() and (L == T or float(mel[b, :, L:].abs().max()) == 0.0), b
                continue
            one = eng.cfm_solve(mu[b:b + 1, :, :L].contiguous(), None, spks[b:b + 1], cond[b:b + 1, :, :L].contiguous(), 2).cpu()
            e = md(mel[b, :, :L], one[0])
            print(f"{solver}, ragged utterance {b}: {e:.3e}")
            assert torch.isfinite(mel[b]).all() and e <= GEOMETRY_BOUND, (b, e)
            if L < T:
                assert float(mel[b, :, L:].abs().max()) == 0.0, b


@pytest.mark.parametrize("solver", ["midpoint", "heun"])
def test_prompted_solve_against_the_hand_concatenated_one(eng, solver):
    g = torch.Generator().manual_seed(622)
    p, y = [20, 35], [40, 28]
    mu_y, spks = torch.randn(2, 80, 40, generator=g), torch.randn(2, 80, generator=g)
    ph, pf = torch.randn(2, 35, 80, generator=g), torch.randn(2, 35, 80, generator=g)
    args = (mu_y, torch.tensor(y), ph, pf, torch.tensor(p), spks, 2)
    default = eng.cfm_solve_prompted(*args).cpu()
    with eng.solver(solver):
        mel = eng.cfm_solve_prompted(*args).cpu()
        for b in range(2):
            mu = torch.cat([ph[b:b + 1, :p[b]].transpose(1, 2), mu_y[b:b + 1, :, :y[b]]], dim=2).contiguous()
            cond = torch.cat([pf[b:b + 1, :p[b]].transpose(1, 2), torch.zeros(1, 80, y[b])], dim=2).contiguous()
            one = eng.cfm_solve(mu, None, spks[b:b + 1], cond, 2).cpu()[0, :, p[b]:]
            e = md(mel[b, :, :y[b]], one)
            print(f"{solver}, prompted utterance {b}: {e:.3e}")
            assert e <= GEOMETRY_BOUND, (b, e)
    assert md(mel, default) > 1e-3                                            # (the mode did apply)
    assert torch.equal(eng.cfm_solve_prompted(*args).cpu(), default)          # ... and Euler is back behind the block


@pytest.mark.parametrize("solver", ["midpoint", "heun"])
def test_split_k_route_against_a_row_owning_batch(eng, solver):
    """B = 1, T = 61 (134 rows: the tile kernels, K split) against the same utterance as row 3 of a ragged B = 12 batch whose rows
    are on the row-owning side of the seam: another arithmetic, held to the oracle bound as elsewhere across it"""
    B, T = 12, 200
    mu, spks, cond = inputs(B, T, 623)
    lens = [200] * B
    lens[3] = 61
    lt = torch.tensor(lens, dtype=torch.int32)
    mask = (torch.arange(T)[None] < lt[:, None]).unsqueeze(1).float()
    mu, cond = mu * mask, cond * mask
    with eng.solver(solver):
        mel = eng.cfm_solve(mu, lt, spks, cond, 2).cpu()
        one = eng.cfm_solve(mu[3:4, :, :61].contiguous(), None, spks[3:4], cond[3:4, :, :61].contiguous(), 2).cpu()
    e = md(mel[3, :, :61], one[0])
    print(f"{solver}, split-K B = 1, T = 61 vs its row in a row-owning batch: {e:.3e}")
    assert torch.isfinite(one).all() and e <= oracle_bound(0.7), e


# ---- 5. twins -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,rates", [("midpoint", [0.0, 0.0]), ("heun", [0.7, 0.0])], ids=["midpoint_0_0", "heun_0.7_0"])
def test_steps_without_twins(monkeypatch, tts_sd, noise, solver, rates):
    """B = 12, T = 200: both evaluations of a rate-0 step run on B T frames, both of a guided step on 2 B T (no twin is shared in a
    second-order solve); with JV_NO_TWIN_DROP=1 all four run on 2 B T and the mel is the same within the geometry bound"""
    B, T = 12, 200
    mu, spks, cond = inputs(B, T, 630)
    out = {}
    for drop in (True, False):
        if drop:
            monkeypatch.delenv("JV_NO_TWIN_DROP", raising=False)
        else:
            monkeypatch.setenv("JV_NO_TWIN_DROP", "1")
        e = fresh_engine(tts_sd, noise, B, T)
        try:
            e.set_guidance(rates)
            e.set_solver(solver)
            out[drop] = (e.cfm_solve(mu, None, spks, cond, 2).cpu(), profiled(lambda: e.cfm_solve(mu, None, spks, cond, 2)))
        finally:
            e.close()
    err = md(out[True][0], out[False][0])
    print(f"{solver} rates {rates}, twins dropped vs kept: {err:.3e}")
    assert torch.isfinite(out[True][0]).all() and err <= GEOMETRY_BOUND, err
    assert_step_frames(out[True][1], 4, [B * T if r == 0.0 else 2 * B * T for r in rates for _ in range(2)])
    assert_step_frames(out[False][1], 4, [2 * B * T] * 4)


# ---- 6. many evaluations ----------------------------------------------------------------------------------------------------------------
def test_more_evaluations_than_precomputed_embeddings(monkeypatch, tts_sd, noise):
    """n = 33 midpoint steps = 66 evaluations > TS_MAX = 64: the embeddings are computed per evaluation, which JV_NO_TEMB_PRE=1
    forces for any n -- the same solve within the geometry bound (the 64-evaluation solve below takes the precomputed rows)"""
    mu, spks, cond = inputs(1, 61, 640)
    got = {}
    for pre in (True, False):
        if pre:
            monkeypatch.delenv("JV_NO_TEMB_PRE", raising=False)
        else:
            monkeypatch.setenv("JV_NO_TEMB_PRE", "1")
        e = fresh_engine(tts_sd, noise, 1, 64)
        try:
            e.set_solver("midpoint")
            got[pre] = (e.cfm_solve(mu, None, spks, cond, 33).cpu(), e.cfm_solve(mu, None, spks, cond, 32).cpu())
        finally:
            e.close()
    for k, n in enumerate((33, 32)):
        err = md(got[True][k], got[False][k])
        print(f"midpoint n = {n}, embeddings by default vs per evaluation: {err:.3e}")
        assert torch.isfinite(got[True][k]).all() and err <= GEOMETRY_BOUND, (n, err)


# ---- 7. token-to-mel ----------------------------------------------------------------------------------------------------------------------
def test_token2mel_streaming_prefix_under_midpoint(prompt_sd, tts_sd):
    """the 77-token session case (stream_ref): inference(streaming=True, solver="midpoint") on all tokens against
    inference_partial on the first L + 3 = 53, frames [0, 2 L - F); the decoder's default solver is back after the calls"""
    from jyutvoice_amd.flow.flow import CausalMaskedDiffWithXvec
    from jyutvoice_amd.runtime import Runtime
    flow = CausalMaskedDiffWithXvec(vocab_size=6561, input_frame_rate=25, runtime=Runtime("cuda:0"))
    flow.load_state_dict(tc.flow_sd(prompt_sd, tts_sd))
    tok, ptok, feat, emb = sr.session_inputs()

    def args(n):
        return tok[:, :n], torch.tensor([n]), ptok, torch.tensor([sr.P]), feat, torch.tensor([sr.F]), emb

    try:
        before = flow.inference(*args(sr.N), True, True, n_timesteps=2)[0].cpu()
        whole = flow.inference(*args(sr.N), True, True, n_timesteps=2, solver="midpoint")[0].cpu()
        L = 50
        k = 2 * L - sr.F
        part = flow.inference_partial(*args(L + 3 - sr.P), True, n_timesteps=2, solver="midpoint")[0].cpu()
        after = flow.inference(*args(sr.N), True, True, n_timesteps=2)[0].cpu()
    finally:
        flow._rt().engine.close()
    assert part.shape == (1, 80, k) and whole.shape[2] > k
    e = md(part, whole[:, :, :k])
    print(f"midpoint, streamed prefix L = {L} vs one-shot: {e:.3e}")
    assert torch.isfinite(whole).all() and e <= GEOMETRY_BOUND, e
    assert torch.equal(before, after) and md(before, whole) > 1e-3
    with pytest.raises(ValueError, match=r"solver must be one of \['euler', 'midpoint', 'heun'\]"):
        flow.inference(*args(sr.N), True, True, n_timesteps=2, solver="rk4")


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_mode_and_the_bits(eng):
    from jyutvoice_amd import _lib
    from jyutvoice_amd._lib import JvError
    mu, spks, cond = inputs(1, 61, 650)
    base = eng.cfm_solve(mu, None, spks, cond, 3).cpu()
    for bad in ("rk4", "", None, 3):
        with pytest.raises(ValueError, match=r"solver must be one of \['euler', 'midpoint', 'heun'\]"):
            eng.set_solver(bad)
    for bad in (-1, 3, 99):
        assert eng.lib.jv_flow_set_solver(eng._h, bad) != 0                  # the library itself refuses an unknown value ...
        assert "JV_SOLVER_EULER, JV_SOLVER_MIDPOINT, JV_SOLVER_HEUN" in eng.lib.jv_last_error().decode()
    assert torch.equal(eng.cfm_solve(mu, None, spks, cond, 3).cpu(), base)      # ... and leaves the mode as it was
    eng.set_solver("heun")
    try:
        assert eng.lib.jv_flow_set_solver(eng._h, 7) != 0
        heun = eng.cfm_solve(mu, None, spks, cond, 2).cpu()
        assert md(heun, base) > 1e-3                                          # (still Heun after the refused call)
        with pytest.raises(JvError, match="n_timesteps = 513 with the Heun solver .* 1026 estimator evaluations, the limit is 1024"):
            eng.cfm_solve(mu, None, spks, cond, 513)
        assert torch.equal(eng.cfm_solve(mu, None, spks, cond, 2).cpu(), heun)
    finally:
        eng.set_solver("euler")
    assert torch.equal(eng.cfm_solve(mu, None, spks, cond, 3).cpu(), base)
    assert _lib.SOLVERS["euler"] == 0
