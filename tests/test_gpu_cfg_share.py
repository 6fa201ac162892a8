"""GPU: one unconditional CFG twin for the first Euler step of an equal-length batch (flow.hip solve_loop).

Every utterance of a solve starts from the same noise prefix, a twin has mu = spks = cond = 0 and t is one scalar, so the B twins
of step 0 are one sample: the step runs on B + 1 samples and every utterance's CFG update reads the twin at slot B.  An utterance's
bits do not depend on the batch, the tile height or the row-owning regime (the project's own contract), so every case compares the
default against JV_NO_CFG_SHARE=1 with torch.equal -- a fresh engine per arm, the switch is read when a context is created.

Taken / not taken is read from the in-library profiler: the fused-block launches of a solve account for (B + 1) T frames in the
first step and 2 B T in the others when the twin is shared, 2 B T in all of them when it is not."""
import pytest
import torch

from parity_util import profiled

pytestmark = pytest.mark.gpu


def inputs(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 80, T, generator=g), torch.randn(B, 80, generator=g), torch.randn(B, 80, T, generator=g) * 0.3


def arm(monkeypatch, tts_sd, noise, shared, max_batch, max_frames, fn):
    """fn(engine) on a fresh engine with the twin shared (the default) or with JV_NO_CFG_SHARE=1"""
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from jyutvoice_amd.engine import JV_MODEL_TTS, Engine
    if shared:
        monkeypatch.delenv("JV_NO_CFG_SHARE", raising=False)
    else:
        monkeypatch.setenv("JV_NO_CFG_SHARE", "1")
    e = Engine("cuda:0", max_batch=max_batch, max_frames=max_frames, max_tokens=64)
    try:
        e.load_state_dict(JV_MODEL_TTS, tts_sd)
        e.load_noise(noise)
        return fn(e)
    finally:
        e.close()


def block_frames(report):
    """(launches, frames summed over them) of a solve's fused transformer-block launches: a launch's flops are 2 frames
    (512 x 256 + 2 x 256 x 1024 MACs, + 256 x 1536 where q | k | v rides along) (rowblock.hip; parity_util.solve_frames)"""
    n, frames = 0, 0.0
    for k, v in report.items():
        if k.startswith("rowblock_h3<"):
            macs = 256.0 * 512 + 2.0 * 256 * 1024 + (256.0 * 1536 if k.endswith(",qkv>") else 0.0)
            n += v["launches"]
            frames += v["flops"] / (2.0 * macs)
    assert n > 0, sorted(report)
    return n, frames


def assert_taken(report, B, T, steps, taken):
    n, frames = block_frames(report)
    assert n % steps == 0, (n, steps)
    want = (n // steps) * (((B + 1) * T + (steps - 1) * 2 * B * T) if taken else steps * 2 * B * T)
    assert abs(frames - want) <= 1e-6 * want, (frames, want, "shared" if taken else "not shared", sorted(report))


def solve_both(monkeypatch, tts_sd, noise, B, T, steps, seed, lens=None, temperature=1.0):
    """{shared: (mels per step count, profiler report of the last one)}"""
    mu, spks, cond = inputs(B, T, seed)
    if lens is not None:
        mask = (torch.arange(T)[None] < lens[:, None]).unsqueeze(1).float()
        mu, cond = mu * mask, cond * mask

    def run(e):
        mels = [e.cfm_solve(mu, lens, spks, cond, n, temperature).cpu() for n in steps]
        rep = profiled(lambda: e.cfm_solve(mu, lens, spks, cond, steps[-1], temperature))
        return mels, rep

    return {s: arm(monkeypatch, tts_sd, noise, s, B, T, run) for s in (True, False)}


def assert_equal(out):
    for a, b in zip(out[True][0], out[False][0]):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), float((a - b).abs().max())


@pytest.mark.parametrize("with_lens", [False, True], ids=["no_lengths", "equal_lengths_passed"])
def test_shared_twin_row_owning_in_both_geometries(monkeypatch, tts_sd, noise, with_lens):
    """B = 12, T = 200: step 0 on 13 samples (2 656 rows), the others on 24 (4 900 rows), both on the row-owning kernels;
    n_timesteps 1 (the shared step alone) and 3.  With no lengths, and with twelve equal lengths passed (what a batched
    synthesise() of equal utterances does: the host learns they are equal from the copy the ragged check brings down anyway)"""
    B, T = 12, 200
    lens = torch.full((B,), T, dtype=torch.int32) if with_lens else None
    out = solve_both(monkeypatch, tts_sd, noise, B, T, (1, 3), 301, lens)
    assert_equal(out)
    assert_taken(out[True][1], B, T, 3, True)
    assert_taken(out[False][1], B, T, 3, False)


def test_shared_twin_other_tiling_in_step_0(monkeypatch, tts_sd, noise):
    """B = 7, T = 300: 2 436 rows in step 0 against 4 260 (q | k | v dealt over 6 against 3 workgroups per 80 rows)"""
    B, T = 7, 300
    out = solve_both(monkeypatch, tts_sd, noise, B, T, (3,), 302)
    assert_equal(out)
    assert_taken(out[True][1], B, T, 3, True)
    assert_taken(out[False][1], B, T, 3, False)


def test_shared_twin_other_tile_height_in_step_0(monkeypatch, tts_sd, noise):
    """B = 16, T = 300: step 0 on 17 samples (5 172 rows, 32-row tiles), step 1 on 32 (9 732 rows, 48-row tiles) -- what the
    headline does with 48- against 80-row tiles"""
    from parity_util import rowgemm_tile
    B, T = 16, 300
    assert (rowgemm_tile(4 + (B + 1) * (T + 4)), rowgemm_tile(4 + 2 * B * (T + 4))) == (2, 3)
    out = solve_both(monkeypatch, tts_sd, noise, B, T, (2,), 307)
    assert_equal(out)
    assert_taken(out[True][1], B, T, 2, True)
    assert_taken(out[False][1], B, T, 2, False)


def test_shared_step_keeps_the_later_steps_resnet_route(monkeypatch, tts_sd, noise):
    """B = 4, T = 1000: the whole-resnet launch fits its rounds at 5 samples (5 024 rows: 168 tiles of 30 rows) and not at 8
    (8 036 rows: 268 > 256).  It alternates the trunk between two buffers, the two-launch form does not, and the running maxima
    are kept per buffer: the shared step takes the two-launch form too (no rowres launch in either arm), and the mels are equal"""
    B, T = 4, 1000
    out = solve_both(monkeypatch, tts_sd, noise, B, T, (2,), 308)
    assert_equal(out)
    for s in (True, False):
        assert not [k for k in out[s][1] if k.startswith("rowres_h3")], sorted(out[s][1])
    assert_taken(out[True][1], B, T, 2, True)
    assert_taken(out[False][1], B, T, 2, False)


def test_not_shared_across_the_split_k_seam(monkeypatch, tts_sd, noise):
    """B = 4, T = 300: 5 samples are 1 524 rows <= 2 048, the split-K regime, whose sums group differently from the row-owning
    kernels' (up to 2e-5, test_ln_fold_matches_separate_norm): the twin is not shared, both arms launch the same"""
    B, T = 4, 300
    out = solve_both(monkeypatch, tts_sd, noise, B, T, (3,), 303)
    assert_equal(out)
    launches = {s: {k: v["launches"] for k, v in out[s][1].items()} for s in (True, False)}
    assert launches[True] == launches[False]
    assert_taken(out[True][1], B, T, 3, False)


def test_not_shared_with_unequal_lengths(monkeypatch, tts_sd, noise):
    """B = 12, T = 200, one utterance a frame shorter: the uniform geometry (the compact one would save 0.04 % of the rows, its
    threshold is 8 %), and the twins are no longer one sample"""
    B, T = 12, 200
    lens = torch.full((B,), T, dtype=torch.int32)
    lens[5] = T - 1
    out = solve_both(monkeypatch, tts_sd, noise, B, T, (3,), 304, lens)
    assert_equal(out)
    assert_taken(out[True][1], B, T, 3, False)
    assert_taken(out[False][1], B, T, 3, False)


AMAX_TEMPERATURE = 1000.0


def test_amax_hand_over(monkeypatch, tts_sd, noise):
    """The running trunk maxima (FlowWs::amax) that step 0 leaves in the shared twin's slot go to the B - 1 slots it stands for:
    the later steps derive their fp16x3 power-of-two scales from them.  B = 12, T = 200, three steps, temperature 1000: the
    twin's input is 1000 x the noise and nothing conditions it, so its residual stream (res_conv is linear in x) is at its
    largest in step 0, before the conditional samples' guidance has moved x.

    This case fails when the broadcast is removed.  Checked once while developing, on a library built without
    amax_share_kernel's launch, against JV_NO_CFG_SHARE=1: max |mel difference| 2.4e-4 at temperature 1000 (1.6e-2 at 1e5,
    1.8e-6 at 0), while the temperatures 1e-4 .. 64 stayed equal even so -- three fp16 planes hold an fp32 value exactly under
    any power-of-two scale, so a slot that misses step 0's maximum only shows where elements far below it lose their low bits;
    hence the large temperature."""
    B, T = 12, 200
    out = solve_both(monkeypatch, tts_sd, noise, B, T, (3,), 305, temperature=AMAX_TEMPERATURE)
    assert_equal(out)
    assert_taken(out[True][1], B, T, 3, True)


def test_shared_twin_under_step_graph(monkeypatch, tts_sd, noise):
    """jv_flow_set_graph on: the shared step runs eagerly, the captured 2B step replays for the others -- the capturing solve,
    a replaying one, two steps (nothing left to replay after the eager pair on a fresh geometry) and one step"""
    B, T = 12, 200
    mu, spks, cond = inputs(B, T, 301)

    def eager(e):
        return {n: e.cfm_solve(mu, None, spks, cond, n, 1.0).cpu() for n in (1, 2, 3)}

    def graphed(e):
        e.set_step_graph(True)
        return [(n, e.cfm_solve(mu, None, spks, cond, n, 1.0).cpu()) for n in (2, 3, 3, 1, 2)]

    want = arm(monkeypatch, tts_sd, noise, False, B, T, eager)
    shared = arm(monkeypatch, tts_sd, noise, True, B, T, eager)
    for n in want:
        assert torch.equal(shared[n], want[n]), n
    for n, mel in arm(monkeypatch, tts_sd, noise, True, B, T, graphed):
        assert torch.equal(mel, want[n]), n


def test_shared_twin_prompted(monkeypatch, tts_sd, noise):
    """cfm_solve_prompted, eight utterances of 60 prompt + 200 generated frames each: 9 samples of 260 frames (2 380 rows)"""
    B, P, Ty = 8, 60, 200
    g = torch.Generator().manual_seed(306)
    mu_y, spks = torch.randn(B, 80, Ty, generator=g), torch.randn(B, 80, generator=g)
    ph, pf = torch.randn(B, P, 80, generator=g), torch.randn(B, P, 80, generator=g)
    yl, pl = torch.full((B,), Ty, dtype=torch.int32), torch.full((B,), P, dtype=torch.int32)

    def run(e):
        mel = e.cfm_solve_prompted(mu_y, yl, ph, pf, pl, spks, 3).cpu()
        return mel, profiled(lambda: e.cfm_solve_prompted(mu_y, yl, ph, pf, pl, spks, 3))

    out = {s: arm(monkeypatch, tts_sd, noise, s, B, P + Ty, run) for s in (True, False)}
    assert torch.isfinite(out[True][0]).all()
    assert torch.equal(out[True][0], out[False][0])
    assert_taken(out[True][1], B, P + Ty, 3, True)
    assert_taken(out[False][1], B, P + Ty, 3, False)


@pytest.mark.parametrize("streaming", [False, True], ids=["full_attention", "streaming"])
def test_shared_twin_token2mel(monkeypatch, prompt_sd, tts_sd, streaming):
    """flow_token2mel, eight utterances of 30 prompt + 100 tokens each (260 frames, 9 samples: 2 380 rows), 40 prompt frames;
    with the estimator's full and its chunk-causal attention"""
    from jyutvoice_amd import synth
    from jyutvoice_amd.flow.flow import CausalMaskedDiffWithXvec
    from jyutvoice_amd.runtime import Runtime
    B, P, N, F = 8, 30, 100, 40
    tok, _ = synth.prompt_tokens(B, N, lengths=[N] * B, first_index=11)
    ptok, _ = synth.prompt_tokens(B, P, lengths=[P] * B, first_index=41)
    g = torch.Generator().manual_seed(309)
    feat, emb = torch.randn(B, F, 80, generator=g), torch.randn(B, 192, generator=g)
    lens = [torch.full((B,), v) for v in (N, P, F)]
    sd = dict(prompt_sd)
    sd.update({k: v for k, v in tts_sd.items() if k.startswith(("decoder.", "spk_embed_affine_layer."))})
    out = {}
    for shared in (True, False):
        if shared:
            monkeypatch.delenv("JV_NO_CFG_SHARE", raising=False)
        else:
            monkeypatch.setenv("JV_NO_CFG_SHARE", "1")
        rt = Runtime("cuda:0")
        try:
            m = CausalMaskedDiffWithXvec(vocab_size=6561, input_frame_rate=25, runtime=rt)
            m.load_state_dict(sd)
            run = lambda: m.inference(tok, lens[0], ptok, lens[1], feat, lens[2], emb, streaming, True, batched=True, n_timesteps=3)[0]
            mel = run().cpu()
            out[shared] = (mel, profiled(run))
        finally:
            rt.engine.close()
    assert torch.isfinite(out[True][0]).all()
    assert torch.equal(out[True][0], out[False][0])
    assert_taken(out[True][1], B, 2 * (P + N), 3, True)
    assert_taken(out[False][1], B, 2 * (P + N), 3, False)
