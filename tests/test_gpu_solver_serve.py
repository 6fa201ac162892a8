"""GPU: a solver per request in the in-flight pool (jv_cfm_pool_step_s) through `SynthServer`.

A served request stays DEFINED as that request run alone at B = 1, `synthesise(..., solver=...)`, met within 2e-5 -- the bound
tests/test_gpu_serve.py uses for the same comparison (another batch geometry).  Six requests of 64 tokens, two of them prompted,
solvers mixed among euler / midpoint / heun, n_timesteps of 2 and 3, one with a guidance window, arrive one per step into four
slots whose pools -- x0 / k1 included -- were filled with NaN beforehand; two slots are taken over from an occupant with another
solver.  Measured distances go to solver_serve_parity.json in the output directory (JV_OUT; committed under profiles/)."""
import pytest
import torch

import parity_util as pu
from jyutvoice_amd.serve import guidance_rates
from test_gpu_serve import KEYS, MEL_BOUND

pytestmark = pytest.mark.gpu

record = pu.Recorder("solver_serve_parity.json", {
    "what": "tests/test_gpu_solver_serve.py: requests served by the in-flight pool under their own solver against the same request "
            "run alone through synthesise(..., solver=...) at B = 1",
    "mel bound": "max-abs 2e-5 (another batch geometry)"})

TOKENS = 64
#          solver      n  prompt tokens  submit() keywords
REQUESTS = [("midpoint", 2, 0, {}),
            ("euler", 3, 12, {}),
            ("heun", 3, 0, {"cfg_rate": 1.5, "cfg_window": (0.0, 0.3)}),
            ("heun", 2, 0, {}),
            ("euler", 2, 0, {}),
            ("midpoint", 3, 20, {})]


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
def served(models, prompt_sd):
    """-> (results by request, the B = 1 arguments of every request, {request: slot})"""
    from jyutvoice_amd import synth
    from jyutvoice_amd.flow.encoder import FlowEncoder
    from jyutvoice_amd.serve import SynthServer
    tts, hift = models
    fenc = FlowEncoder(vocab_size=6561, input_size=512, output_size=80, device="cuda:0")
    fenc.load_state_dict(prompt_sd)
    n = len(REQUESTS)
    batch = synth.batch(n, TOKENS)
    prompts = [r[2] for r in REQUESTS]
    have = [b for b, k in enumerate(prompts) if k]
    tok, lens = synth.prompt_tokens(len(have), max(prompts), lengths=[prompts[b] for b in have], first_index=1)
    h, _ = fenc(tok, lens)
    g = torch.Generator().manual_seed(5)
    args = []
    for b in range(n):
        one = [batch[k][b:b + 1] for k in KEYS]
        p = 2 * prompts[b]
        feat = torch.randn(1, p, 80, generator=g) if p else None
        ph = h[have.index(b):have.index(b) + 1, :p].cpu() if p else None
        args.append((one, feat, ph))
    server = SynthServer(tts, hift, max_sessions=4, max_frames=1024, max_tokens=TOKENS)
    server.pool.ensure_stage_pools()
    for t in server.pool.tensors() + (server.pool.x0, server.pool.k1):      # nothing a request did not write itself may be read
        t.fill_(float("nan"))
    out, slot_of = {}, {}
    for b, (solver, steps, _, kw) in enumerate(REQUESTS):                   # arrivals staggered by one step
        one, feat, ph = args[b]
        rid = server.submit(*one, prompt_feat=feat, prompt_h=ph, n_timesteps=steps, seed=40 + b, solver=solver, **kw)
        assert rid == b
        out.update(server.step())
        slot_of.update({r.rid: s for s, r in server._active.items()})
    out.update(server.drain())
    assert sorted(out) == list(range(n)) and all("error" not in v for v in out.values()), out
    # every request took n * evaluations pool steps; the last one (midpoint, n = 3) arrived at step 5 and left after step 10
    assert server.steps == 11
    return out, args, slot_of


def test_slots_are_taken_over_across_solvers(served):
    _, _, slot_of = served
    assert slot_of[4] == slot_of[0] and REQUESTS[4][0] != REQUESTS[0][0]      # euler behind midpoint
    assert slot_of[5] == slot_of[1] and REQUESTS[5][0] != REQUESTS[1][0]      # midpoint behind euler


@pytest.mark.parametrize("b", range(len(REQUESTS)))
def test_served_request_against_its_definition(models, served, b):
    tts, _ = models
    out, args, _ = served
    solver, steps, ptok, kw = REQUESTS[b]
    one, feat, ph = args[b]
    p = 2 * ptok
    schedule = guidance_rates(steps, kw["cfg_rate"], kw["cfg_window"]) if "cfg_window" in kw else None
    if schedule is not None:
        assert 0.0 in schedule and 1.5 in schedule
    call = dict(n_timesteps=steps, batched=True, solver=solver, cfg_schedule=schedule)
    none = torch.zeros(1, 1, 80)
    if p:
        want = tts.synthesise(*one, feat, prompt_h=ph, prompt_lengths=torch.tensor([p]), **call)
    else:
        want = tts.synthesise(*one, none, prompt_h=none, prompt_lengths=torch.tensor([0]), **call)
    y = int(want["mel_lengths"][0])
    got = out[b]
    assert got["mel_length"] == y and got["mel"].shape == (1, 80, y) and got["wav"].shape == (1, 480 * y)
    e = pu.md(got["mel"].cpu(), want["mel"][:, :, :y].cpu())
    record(f"request {b}: {solver}, n = {steps}, prompt frames {p}{', window' if schedule else ''}", error=e)
    assert torch.isfinite(got["mel"]).all() and torch.isfinite(got["wav"]).all() and e <= MEL_BOUND, (b, e)
    if solver != "euler":      # (the solver is read: the same request on Euler is another mel)
        euler = tts.synthesise(*one, none if not p else feat, prompt_h=none if not p else ph, prompt_lengths=torch.tensor([p]),
                               **dict(call, solver="euler"))
        assert pu.md(got["mel"].cpu(), euler["mel"][:, :, :y].cpu()) > 100 * MEL_BOUND


def test_rejected_stage_names_the_request_and_leaves_the_pools_unchanged(models):
    from jyutvoice_amd import _lib
    from jyutvoice_amd._lib import JvError
    from jyutvoice_amd.runtime import get_runtime
    from jyutvoice_amd.serve import step_table
    from test_gpu_serve import make_request, padded
    eng = get_runtime("cuda:0").ensure(4, 256, TOKENS)
    reqs = [make_request(80, 40, 10, 2), make_request(81, 33, 0, 2)]
    mu_y, ph, pf, spks = padded(reqs)
    pool = eng.cfm_pool(3, 64)
    eng.cfm_pool_admit(pool, mu_y, [40, 33], ph, pf, [10, 0], spks, [0, 2], [1.0, 1.0])
    before = pool.x.clone()
    tt, cs, stages = step_table(2, "cosine", "heun")
    for bad in (2, 5, -1, 16):                                              # (2 alone would save a slope without a base state)
        with pytest.raises(JvError, match=f"jv_cfm_pool_step_s: request 1: stage {bad} is none of"):
            eng.cfm_pool_step(pool, [0, 2], [50, 33], [tt[0]] * 2, [cs[0]] * 2, stage=[stages[0], bad])
    torch.cuda.synchronize()
    assert torch.equal(pool.x, before)
    # the old entries are the new one on STAGE_EULER, bit for bit
    other = eng.cfm_pool(3, 64)
    eng.cfm_pool_admit(other, mu_y, [40, 33], ph, pf, [10, 0], spks, [0, 2], [1.0, 1.0])
    et, ed = step_table(2)
    for k in range(2):
        eng.cfm_pool_step(pool, [0, 2], [50, 33], [et[k]] * 2, [ed[k]] * 2)
        eng.cfm_pool_step(other, [0, 2], [50, 33], [et[k]] * 2, [ed[k]] * 2, stage=[_lib.STAGE_EULER] * 2)
    for a, b in zip(pool.tensors(), other.tensors()):
        assert torch.equal(a, b), pu.md(a, b)
