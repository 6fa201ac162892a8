"""GPU: the length contract of the C ABI (include/jyutvoice_hip.h "Lengths").

Every lens[b] handed to jv_cfm_solve, jv_hift_decode, jv_hift_f0 and jv_flow_estimator_step means min(max(lens[b], 0), T) -- the
reference's sequence_mask(lens, T).  An utterance of effective length 0 comes back as zeros and changes nothing in its
neighbours.  jv_cfm_solve_prompted validates instead: it rejects a length outside its range.

The cases that matter are the ragged batches in the COMPACT row geometry (flow.hip solve_compact, hift.hip hift_decode), where
the rows behind an utterance's last frame are not its own padding but the gap in front of the next utterance: the estimator's
causal convolutions read them as the next utterance's left context, the vocoder's symmetric ones in both directions.  The host
lays the utterances out by the clamped length; row_meta has to mark rows valid by the same rule (rowops.hip).  So every case
here first shows that its batch DID take the compact geometry (the frames the profiler's launches account for: the sum of the
clamped lengths, not B T), and then asserts bits:
  (a) lens[b] = T + 57, on a non-last utterance followed by a shorter one and on the last: the call with lens[b] = T, and the
      uniform geometry (JV_NO_COMPACT=1);
  (b) lens[b] = -3 and 0 in the middle of the batch: compact = uniform, everything finite, that utterance exactly zero, every
      other utterance what it is when the dead utterance's inputs are replaced by other data;
  (c) the entries that only know the uniform geometry, on the same values: the call with clamped lengths;
  (d) jv_cfm_solve_prompted keeps rejecting."""
import os

import pytest
import torch

import parity_util as pu

pytestmark = pytest.mark.gpu

B, T, N_STEPS = 12, 300, 2
LENS = [260, 120, 300, 200, 150, 240, 180, 130, 220, 160, 250, 140]      # M = 4 + 2 B (T + 4) = 7300 rows uniform, 4800 compact
OVER = T + 57
VB, VT = 6, 70
VLENS = [70, 31, 70, 12, 55, 64]


def clamp(lens, t):
    return [min(max(n, 0), t) for n in lens]


@pytest.fixture(scope="module")
def engines(tts_sd, hift_sd, noise):
    """one context per geometry: JV_NO_COMPACT is read when a context is created"""
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from jyutvoice_amd.engine import JV_MODEL_HIFT, JV_MODEL_TTS, Engine
    made = {}
    saved = os.environ.pop("JV_NO_COMPACT", None)
    try:
        for name in ("compact", "uniform"):
            if name == "uniform":
                os.environ["JV_NO_COMPACT"] = "1"
            e = Engine("cuda:0", max_batch=B, max_frames=T + 4, max_tokens=32)
            e.load_state_dict(JV_MODEL_TTS, tts_sd)
            e.load_state_dict(JV_MODEL_HIFT, hift_sd)
            e.load_noise(noise)
            made[name] = e
    finally:
        os.environ.pop("JV_NO_COMPACT", None)
        if saved is not None:
            os.environ["JV_NO_COMPACT"] = saved
    yield made
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def flow_in():
    g = torch.Generator().manual_seed(20577)
    return {"mu": torch.randn(B, 80, T, generator=g).cuda(), "cond": torch.randn(B, 80, T, generator=g).cuda(),
            "spks": torch.randn(B, 80, generator=g).cuda(), "other": torch.randn(3, 80, T + 1, generator=g).cuda()}


def solve(eng, f, lens):
    mel = eng.cfm_solve(f["mu"], torch.tensor(lens, dtype=torch.int32), f["spks"], f["cond"], N_STEPS, 1.0)
    torch.cuda.synchronize()
    return mel.cpu()


def solve_was_compact(engines, f, lens):
    rc = pu.profiled(lambda: solve(engines["compact"], f, lens))
    ru = pu.profiled(lambda: solve(engines["uniform"], f, lens))
    pu.assert_solve_compact(rc, ru, lens, T)


def decode(eng, mel, s, lens):
    wav = eng.hift_decode(mel, s, torch.tensor(lens, dtype=torch.int32))
    torch.cuda.synchronize()
    return wav.cpu()


def decode_was_compact(engines, mel, s, lens):
    rc = pu.profiled(lambda: decode(engines["compact"], mel, s, lens))
    ru = pu.profiled(lambda: decode(engines["uniform"], mel, s, lens))
    # the 128-channel level: 40 rows per mel frame in both geometries
    pu.assert_compact_taken(rc, ru, lens, VT, "hiftpair_h3<", "x128,snake>")


# ---- (a) over-long lengths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [2, B - 1], ids=["before_a_shorter_utterance", "last"])
def test_cfm_solve_overlong_length_is_the_full_length(engines, flow_in, where):
    over, full = list(LENS), list(LENS)
    over[where], full[where] = OVER, T
    assert where == B - 1 or full[where + 1] < T
    solve_was_compact(engines, flow_in, over)
    want = solve(engines["compact"], flow_in, full)
    got = solve(engines["compact"], flow_in, over)
    uni = solve(engines["uniform"], flow_in, over)
    assert torch.isfinite(got).all()
    assert torch.equal(solve(engines["uniform"], flow_in, full), want)          # (the two geometries agree on in-range lengths)
    bad = [b for b in range(B) if not torch.equal(got[b], want[b])]
    assert not bad, (f"utterances {bad} differ from the call with lens[{where}] = T", pu.md(got, want))
    assert torch.equal(got, uni), pu.md(got, uni)
    for b, n in enumerate(full):
        assert float(got[b, :, n:].abs().sum()) == 0.0, b


@pytest.mark.parametrize("where", [2, VB - 1], ids=["before_a_shorter_utterance", "last"])
def test_hift_decode_overlong_length_is_the_full_length(engines, where):
    mel, s, _ = pu.quiet_vocoder_inputs("compact_70")
    over, full = list(VLENS), list(VLENS)
    over[where], full[where] = VT + 57, VT
    assert where == VB - 1 or full[where + 1] < VT
    decode_was_compact(engines, mel, s, over)
    want = decode(engines["compact"], mel, s, full)
    got = decode(engines["compact"], mel, s, over)
    uni = decode(engines["uniform"], mel, s, over)
    assert torch.isfinite(got).all()
    assert torch.equal(decode(engines["uniform"], mel, s, full), want)
    bad = [b for b in range(VB) if not torch.equal(got[b], want[b])]
    assert not bad, (f"utterances {bad} differ from the call with lens[{where}] = T", pu.md(got, want))
    assert torch.equal(got, uni), pu.md(got, uni)
    for b, n in enumerate(full):
        assert float(got[b, 480 * n:].abs().sum()) == 0.0, b


# ---- (b) lengths <= 0 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dead", [-3, 0])
def test_cfm_solve_empty_utterance_is_zero_and_invisible(engines, flow_in, dead):
    at = 5
    lens = list(LENS)
    lens[at] = dead
    solve_was_compact(engines, flow_in, lens)
    got = solve(engines["compact"], flow_in, lens)
    uni = solve(engines["uniform"], flow_in, lens)
    assert torch.isfinite(got).all() and torch.isfinite(uni).all()
    assert torch.equal(got, uni), pu.md(got, uni)
    assert float(got[at].abs().sum()) == 0.0
    for b, n in enumerate(clamp(lens, T)):
        assert float(got[b, :, n:].abs().sum()) == 0.0, b
        assert n == 0 or float(got[b, :, :n].abs().max()) > 0.0, b
    # nothing is read from the dead utterance: other data in its place
    swapped = {k: v.clone() for k, v in flow_in.items()}
    swapped["mu"][at] = flow_in["other"][0, :, :T]
    swapped["cond"][at] = flow_in["other"][1, :, :T]
    swapped["spks"][at] = flow_in["other"][2, :, 0]
    for name in ("compact", "uniform"):
        again = solve(engines[name], swapped, lens)
        assert torch.equal(again, got), (name, [b for b in range(B) if not torch.equal(again[b], got[b])])
    # ... and the contract's clamp: a negative length is the length 0
    zero = list(lens)
    zero[at] = 0
    assert torch.equal(solve(engines["compact"], flow_in, zero), got)


@pytest.mark.parametrize("dead", [-3, 0])
def test_hift_decode_empty_utterance_is_zero_and_invisible(engines, dead):
    mel, s, _ = pu.quiet_vocoder_inputs("compact_70")
    at = 2
    lens = list(VLENS)
    lens[at] = dead
    decode_was_compact(engines, mel, s, lens)
    got = decode(engines["compact"], mel, s, lens)
    uni = decode(engines["uniform"], mel, s, lens)
    assert torch.isfinite(got).all() and torch.isfinite(uni).all()
    assert torch.equal(got, uni), pu.md(got, uni)
    assert float(got[at].abs().sum()) == 0.0
    for b, n in enumerate(clamp(lens, VT)):
        assert float(got[b, 480 * n:].abs().sum()) == 0.0, b
        assert n == 0 or float(got[b, :480 * n].abs().max()) > 0.0, b
    g = torch.Generator().manual_seed(99)
    mel2, s2 = mel.clone(), s.clone()
    mel2[at] = torch.randn(80, VT, generator=g) * 3.0
    s2[at] = torch.tanh(torch.randn(1, 480 * VT, generator=g) * 0.3)
    for name in ("compact", "uniform"):
        again = decode(engines[name], mel2, s2, lens)
        assert torch.equal(again, got), (name, [b for b in range(VB) if not torch.equal(again[b], got[b])])
    zero = list(lens)
    zero[at] = 0
    assert torch.equal(decode(engines["compact"], mel, s, zero), got)


# ---- (c) the uniform-only entries --------------------------------------------------------------------------------------------
WILD = [260, OVER, 300, -3, 150, 0, 180, 1 << 30, 220, 160, -(1 << 30), OVER]


def test_flow_estimator_step_clamps_its_lengths(engines, flow_in):
    g = torch.Generator().manual_seed(31)
    x = torch.randn(B, 80, T, generator=g).cuda()
    t = torch.rand(B, generator=g).cuda()
    eng = engines["compact"]
    run = lambda lens: eng.flow_estimator(x, torch.tensor(lens, dtype=torch.int32), flow_in["mu"], t, flow_in["spks"], flow_in["cond"]).cpu()
    got, want = run(WILD), run(clamp(WILD, T))
    assert torch.isfinite(want).all() and torch.isfinite(got).all()
    assert torch.equal(got, want), pu.md(got, want)
    for b, n in enumerate(clamp(WILD, T)):
        assert float(got[b, :, n:].abs().sum()) == 0.0, b


def test_hift_f0_clamps_its_lengths(engines):
    g = torch.Generator().manual_seed(32)
    mel = torch.randn(B, 80, T, generator=g)
    eng = engines["compact"]
    run = lambda lens: eng.hift_f0(mel, torch.tensor(lens, dtype=torch.int32)).cpu()
    got, want = run(WILD), run(clamp(WILD, T))
    assert torch.isfinite(want).all() and torch.isfinite(got).all()
    assert torch.equal(got, want), pu.md(got, want)


# ---- (d) the prompted entry validates ----------------------------------------------------------------------------------------
def test_cfm_solve_prompted_rejects_out_of_range_lengths(engines):
    from jyutvoice_amd._lib import JvError
    eng = engines["compact"]
    g = torch.Generator().manual_seed(33)
    Bp, Ty, P = 4, 120, 60
    mu_y, spks = torch.randn(Bp, 80, Ty, generator=g).cuda(), torch.randn(Bp, 80, generator=g).cuda()
    ph, pf = torch.randn(Bp, P, 80, generator=g).cuda(), torch.randn(Bp, P, 80, generator=g).cuda()
    y, p = [120, 100, 80, 111], [60, 40, 50, 33]
    call = lambda yl, pl: eng.cfm_solve_prompted(mu_y, torch.tensor(yl), ph, pf, torch.tensor(pl), spks, N_STEPS)
    good = call(y, p).cpu()
    for yl, pl, who in (([120, 100, Ty + 57, 111], p, "utterance 2"), ([120, -3, 80, 111], p, "utterance 1"),
                        (y, [60, 40, 50, P + 1], "utterance 3"), (y, [-1, 40, 50, 33], "utterance 0")):
        with pytest.raises(JvError, match=who):
            call(yl, pl)
    assert torch.equal(call(y, p).cpu(), good)      # the context stays usable
