"""GPU: an utterance's result does not depend on where in the batch it sits.

flow_ws.h's invariant -- per-utterance measured bounds, and a row summed in the same order wherever it lies -- makes this a
zero-tolerance property: B copies of one utterance must come back as B identical results, in every regime the row count
selects (split-K tiles, plain tiles, row-owning kernels at tile heights 2 - 5, q | k | v split 6 / 3 / 2 or fused, one-launch
resnets of 16 rt - 2 rows per workgroup, attn64_s against attn64_pl, compact or not).  test_gpu_regimes.py compares utterance 0
only, the one position where a row-owning kernel's positional faults cannot show: the last, partly empty workgroup, a tile seam
that falls inside the gap or on an utterance's first rows, the twin half of the CFG batch, an offset table entry.  Here every
position is compared with position 0, over batch sizes x frame counts that move the seams, over ragged replicated batches with
odd lengths in the compact geometry (bit-equal to the uniform one, the q | k | v regime asserted), and over the vocoder.

Position 0 itself is anchored to the reference: for every (B, T) of the equal-length sweep, copy 0 against the same model
evaluated in fp64 (oracle.flow.cfm_solve on the decoder weights cast to double).  The bound is measured from the reference in
the test: floor = max |fp32 oracle - fp64 model| on that input, and max |gpu - fp64| <= 4 x floor (twofold headroom over the
only ratio on record: profiles/r04_parity_hostile.json has the GPU at 1.0 - 1.8e-5 where the oracle is 7 - 9e-6).  Floor,
error and ratio per (B, T) go to parity_positions.json in the output directory (JV_OUT; committed as profiles/parity_positions.json)."""
import os

import pytest
import torch

import parity_util as pu

pytestmark = pytest.mark.gpu

BATCHES = (1, 2, 4, 8, 16, 24, 32, 40, 48, 64)      # test_gpu_regimes.py's list
FRAMES = (300, 301, 77, 517)
MAX_ROWS = 64 * 304                                 # what test_gpu_regimes.py allocates (64 utterances of 300 + 4 frames)
N_STEPS = 2
RATIO = 4.0
RAGGED_T, RAGGED_PATTERN = 301, [301, 150, 233]
record = pu.Recorder("parity_positions.json",
                     {"bound": "max |gpu copy 0 - fp64 model| <= 4 x floor, floor = max |fp32 oracle - fp64 model| on the same input",
                      "input": "B copies of one utterance (mu, spks ~ N(0,1), cond = 0), n = 2"})


def batches_for(T):
    return [b for b in BATCHES if b * T <= MAX_ROWS]


def make_engines(sd_tts, sd_hift, noise, max_batch, max_frames):
    """one context per geometry (JV_NO_COMPACT is read when a context is created)"""
    from jyutvoice_amd.engine import JV_MODEL_HIFT, JV_MODEL_TTS, Engine
    made = {}
    saved = os.environ.pop("JV_NO_COMPACT", None)
    try:
        for name in ("compact", "uniform"):
            if name == "uniform":
                os.environ["JV_NO_COMPACT"] = "1"
            e = Engine("cuda:0", max_batch=max_batch, max_frames=max_frames, max_tokens=32)
            if sd_tts is not None:
                e.load_state_dict(JV_MODEL_TTS, sd_tts)
                e.load_noise(noise)
            if sd_hift is not None:
                e.load_state_dict(JV_MODEL_HIFT, sd_hift)
            made[name] = e
    finally:
        os.environ.pop("JV_NO_COMPACT", None)
        if saved is not None:
            os.environ["JV_NO_COMPACT"] = saved
    return made


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def differing(out):
    return [b for b in range(1, out.shape[0]) if not torch.equal(out[b], out[0])]


# ---- equal lengths: every batch size of the regime list x frame counts that move the seams -----------------------------------
@pytest.mark.parametrize("T", FRAMES)
def test_replicated_batch_every_copy_equals_copy_zero(gpu, tts_sd, noise, T):
    from jyutvoice_amd.engine import JV_MODEL_TTS, Engine
    sizes = batches_for(T)
    assert sizes and (T != 517 or max(sizes) == 32)
    g = torch.Generator().manual_seed(7000 + T)
    mu, spks = torch.randn(1, 80, T, generator=g), torch.randn(1, 80, generator=g)
    m32, m64 = pu.cfm_oracles(tts_sd, noise, mu, spks, N_STEPS)      # once per T
    floor = pu.md(m32, m64)
    assert 0.0 < floor < 1e-4, floor
    eng = Engine("cuda:0", max_batch=max(sizes), max_frames=T, max_tokens=32)
    failures = []
    try:
        eng.load_state_dict(JV_MODEL_TTS, tts_sd)
        eng.load_noise(noise)
        for B in sizes:
            mu_b, spks_b = mu.expand(B, 80, T).contiguous().cuda(), spks.expand(B, 80).contiguous().cuda()
            mel = eng.cfm_solve(mu_b, None, spks_b, torch.zeros(B, 80, T, device="cuda"), N_STEPS, 1.0)
            torch.cuda.synchronize()
            mel = mel.cpu()
            assert torch.isfinite(mel).all(), (B, T)
            err = pu.md(mel[:1], m64)
            M = pu.flow_rows([T] * B, T)
            record(f"T={T} B={B}", floor=floor, error=err, ratio=err / floor, rows=float(M), tile_height=float(pu.rowgemm_tile(M)))
            print(f"    rows {M}: {pu.qkv_regime(M)}")
            bad = differing(mel)
            if bad:
                failures.append(f"B={B} T={T}: copies {bad[:8]}{'...' if len(bad) > 8 else ''} differ from copy 0 "
                                f"(max {max(pu.md(mel[b], mel[0]) for b in bad):.3e})")
            if err > RATIO * floor:
                failures.append(f"B={B} T={T}: copy 0 is {err:.3e} from the fp64 model, {err / floor:.2f} x the oracle's own {floor:.3e}")
    finally:
        eng.close()
    assert not failures, failures


# ---- ragged replicated batches in the compact geometry ------------------------------------------------------------------------
@pytest.mark.parametrize("k,regime", [(2, "split6"), (3, "split3"), (5, "fused")])
def test_ragged_replicated_batch_by_length_group_and_geometry(gpu, tts_sd, noise, k, regime):
    """lengths [301, 150, 233] x k (odd ones included: 2 frames per token never produces them) on copies of one input: the copies
    that share a length are identical, and the compact geometry gives the uniform one's bits.  6 / 9 / 15 utterances are 2788 /
    4180 / 6964 compact rows: q | k | v dealt over 6 and 3 workgroups per row tile, and inside the block launch."""
    lens = RAGGED_PATTERN * k
    B, T = len(lens), RAGGED_T
    g = torch.Generator().manual_seed(8000 + k)
    mu = torch.randn(1, 80, T, generator=g).expand(B, 80, T).contiguous().cuda()
    spks = torch.randn(1, 80, generator=g).expand(B, 80).contiguous().cuda()
    cond = torch.zeros(B, 80, T, device="cuda")
    lens_t = torch.tensor(lens, dtype=torch.int32)
    engs = make_engines(tts_sd, None, noise, B, T)
    try:
        def run(name):
            out = engs[name].cfm_solve(mu, lens_t, spks, cond, N_STEPS, 1.0)
            torch.cuda.synchronize()
            return out.cpu()
        rc, ru = pu.profiled(lambda: run("compact")), pu.profiled(lambda: run("uniform"))
        pu.assert_solve_compact(rc, ru, lens, T)
        pu.assert_qkv_regime(rc, pu.flow_rows(lens), regime)
        compact, uniform = run("compact"), run("uniform")
    finally:
        for e in engs.values():
            e.close()
    assert torch.isfinite(compact).all()
    for n in RAGGED_PATTERN:
        idx = [b for b in range(B) if lens[b] == n]
        bad = [b for b in idx[1:] if not torch.equal(compact[b], compact[idx[0]])]
        assert not bad, (f"length {n}: copies {bad} differ from copy {idx[0]}", max(pu.md(compact[b], compact[idx[0]]) for b in bad))
        assert float(compact[idx[0], :, n:].abs().sum()) == 0.0 and float(compact[idx[0], :, :n].abs().max()) > 0.0
    assert torch.equal(compact, uniform), pu.md(compact, uniform)


# ---- the vocoder ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,pattern", [("positions_61", [61, 37, 50]), ("positions_151", [151, 97, 150, 12])])
def test_vocoder_replicated_batch(gpu, hift_sd, case, pattern):
    """8 copies of one (mel, s) on audio the clamp does not hide (parity_util: the quiet recipe; its cap is asserted without a GPU
    in test_vocoder_inputs_host.py): equal lengths, and a repeating length pattern in the compact geometry"""
    B = 8
    mel1, s1, (T,) = pu.quiet_vocoder_inputs(case)
    mel, s = mel1.expand(B, 80, T).contiguous(), s1.expand(B, 1, 480 * T).contiguous()
    lens = (pattern * B)[:B]
    engs = make_engines(None, hift_sd, None, B, T)
    try:
        def run(name, ln):
            out = engs[name].hift_decode(mel, s, None if ln is None else torch.tensor(ln, dtype=torch.int32))
            torch.cuda.synchronize()
            return out.cpu()
        equal = run("compact", None)
        equal_lens = run("compact", [T] * B)
        rc, ru = pu.profiled(lambda: run("compact", lens)), pu.profiled(lambda: run("uniform", lens))
        pu.assert_compact_taken(rc, ru, lens, T, "hiftpair_h3<", "x128,snake>")
        compact, uniform = run("compact", lens), run("uniform", lens)
    finally:
        for e in engs.values():
            e.close()
    assert torch.isfinite(equal).all() and torch.isfinite(compact).all()
    assert pu.clamp_share(equal[0]) <= pu.CLAMP_CAP, pu.clamp_share(equal[0])
    bad = differing(equal)
    assert not bad, (f"equal lengths: copies {bad} differ from copy 0", max(pu.md(equal[b], equal[0]) for b in bad))
    assert torch.equal(equal_lens, equal)      # (lengths given, all T: the same call)
    for n in sorted(set(lens)):
        idx = [b for b in range(B) if lens[b] == n]
        bad = [b for b in idx[1:] if not torch.equal(compact[b], compact[idx[0]])]
        assert not bad, (f"length {n}: copies {bad} differ from copy {idx[0]}", max(pu.md(compact[b], compact[idx[0]]) for b in bad))
        assert float(compact[idx[0], 480 * n:].abs().sum()) == 0.0 and float(compact[idx[0], :480 * n].abs().max()) > 0.0
    assert torch.equal(compact, uniform), pu.md(compact, uniform)
    assert torch.equal(compact[0], equal[0])      # a full-length utterance does not see that its neighbours are shorter
