"""CPU: the streaming session's host logic and the three facts it stands on, checked on the oracle alone.

  * the frame schedule (jyutvoice_amd.stream.frame_schedule) against a restatement written from its description (stream_ref);
  * with streaming=True the frames of an aligned prefix are final: oracle.token2mel on the first L + 3 tokens against the run on all
    of them;
  * HiFT's receptive field: a window with HIFT_DECODE_HALO frames of context reproduces the one-shot decode in fp64 and one with 12
    visibly does not; the F0 predictor needs HIFT_F0_HALO = 5 and not 4;
  * argument errors of HiFTStream / Token2WavStream that are raised before any device call."""
import pytest
import torch

import parity_util as pu
import stream_ref as sr
import token2mel_cases as tc


# ---- the schedule ---------------------------------------------------------------------------------------------------------------
def test_schedule_of_the_session_case():
    """P = 7, F = 14, pushes of 21 / 25 / 25 and a finish at N = 70 (one token left for it)"""
    from jyutvoice_amd.stream import frame_schedule
    got = frame_schedule(7, 14, [21, 25, 24], finish=0)
    assert got == [(28, 0, 36), (53, 36, 86), (0, 86, 86), (77, 86, 140)]
    assert got == sr.schedule_ref(7, 14, [21, 25, 24], 0)
    # the issue's split: three pushes of 21 / 25 / 25 reach 78 tokens = 7 + 71, so with N = 70 the last push has 24
    got = frame_schedule(7, 14, [21, 25], finish=24)
    assert got == [(28, 0, 36), (53, 36, 86), (77, 86, 140)] == sr.schedule_ref(7, 14, [21, 25], 24)


def test_schedule_long_prompt_emits_nothing_until_past_it():
    """P = 30, F = 60: the first aligned length (25 tokens, 50 frames) lies inside the prompt; so does nothing until 2 L > F"""
    from jyutvoice_amd.stream import frame_schedule
    got = frame_schedule(30, 60, [1, 10, 15, 30], finish=5)
    assert got == sr.schedule_ref(30, 60, [1, 10, 15, 30], 5)
    assert got[0] == (0, 0, 0) and got[1] == (0, 0, 0)      # 31, 41 tokens: L = 25, 2 L = 50 <= 60
    assert got[2] == (53, 0, 40)                            # 56 tokens: L = 50
    assert got[3] == (78, 40, 90) and got[4] == (91, 90, 122)
    # F = 2 L exactly: still nothing
    assert frame_schedule(20, 50, [8], finish=None) == [(0, 0, 0)]


@pytest.mark.parametrize("P,F,N", [(7, 14, 70), (0, 0, 53), (3, 10, 27), (26, 51, 30)])
def test_schedule_one_token_at_a_time(P, F, N):
    from jyutvoice_amd.stream import frame_schedule
    for finish in (0, 1):
        pushes = [1] * (N - finish)
        got = frame_schedule(P, F, pushes, finish=finish)
        assert got == sr.schedule_ref(P, F, pushes, finish)
        # every frame exactly once and in order, whatever the split
        pos = 0
        for solved, lo, hi in got:
            assert lo == pos and hi >= lo and (solved > 0) == (hi > lo)
            pos = hi
        assert pos == 2 * (P + N) - F
        # a push solves only when a chunk completes: at most one solve per 25 tokens
        assert sum(1 for s, _, _ in got[:-1] if s) <= (P + N) // 25


def test_schedule_errors():
    from jyutvoice_amd.stream import frame_schedule
    with pytest.raises(ValueError, match="fewer than the 14 prompt frames"):
        frame_schedule(2, 14, [3], finish=0)
    with pytest.raises(ValueError, match="call 1 has -1 tokens"):
        frame_schedule(2, 0, [3, -1])


def test_hift_stream_counts_of_the_gpu_cases():
    """what test_gpu_stream.py expects of the three splits: the lag is 21 frames, a push shorter than either halo emits nothing"""
    assert sr.hift_stream_counts([50, 50, 30]) == ([29, 50, 30], 21)
    assert sr.hift_stream_counts([7, 123]) == ([0, 109], 21)
    counts, rest = sr.hift_stream_counts([1] * 130)
    assert counts[:21] == [0] * 21 and counts[21:] == [1] * 109 and rest == 21
    for lo, hi in sr.KEPT:
        assert sr.window_of(lo, hi, 16, 130) in ((0, 66), (34, 101), (69, 130))


# ---- an aligned prefix is final (oracle alone) -----------------------------------------------------------------------------------
def test_oracle_prefix_frames_are_final(prompt_sd, tts_sd, noise):
    """oracle.token2mel(streaming=True) on the first L + 3 of the 77 tokens against the run on all 77, frames [0, 2 L - F), L = 25 and
    50.  Bound: 2 x the oracle's own fp32 floor (max abs of its fp32 run against its fp64 run on the 77 tokens) -- both runs carry
    that much rounding and nothing else separates them.  The figures are in tests/golden/README_stream.md."""
    from oracle import token2mel as ot2m
    sd = tc.flow_sd(prompt_sd, tts_sd)
    tok, ptok, feat, emb = sr.session_inputs()

    def run(n, dtype=torch.float32):
        mel, _ = ot2m.token2mel(sd, noise, tok[:, :n], torch.tensor([n]), ptok, torch.tensor([sr.P]), feat, torch.tensor([sr.F]), emb, True,
                                n_timesteps=sr.N_TIMESTEPS, dtype=dtype)
        return mel

    with torch.inference_mode():
        full, full64 = run(sr.N), run(sr.N, torch.float64)
        floor = pu.md(full, full64)
        print(f"oracle fp32 vs fp64 on 77 tokens: {floor:.3e}")
        assert 0.0 < floor < 1e-3
        for L in (25, 50):
            part = run(L + 3 - sr.P)
            k = 2 * L - sr.F
            e = pu.md(part[:, :, :k], full[:, :, :k])
            behind = pu.md(part[:, :, k:], full[:, :, k:part.shape[2]])
            print(f"L = {L}: frames [0, {k}) of {L + 3} vs 77 tokens: {e:.3e} (bound {2 * floor:.3e}); frames behind: {behind:.3e}")
            assert e <= 2 * floor, (L, e, floor)
            assert behind > 1e-2, (L, behind)      # the frames behind the aligned prefix do move: the test can see a wrong L


# ---- HiFT's receptive field (oracle alone, fp64) ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def voc(hift_sd):
    mel, s = sr.vocoder_inputs()
    _, w64 = pu.hift_folded(hift_sd)
    from oracle import hift as ohift
    with torch.inference_mode():
        whole = ohift.decode(w64, mel.double(), s.double())
        f0 = ohift.f0_predict(w64, mel.double())
    assert pu.clamp_share(whole) <= pu.CLAMP_CAP
    return mel.double(), s.double(), w64, whole, f0


def test_decode_halo(voc):
    """fp64: 1e-12 is rounding (|wav| < 1, a few thousand additions per sample; the figure measured is 0), 1e-5 is a seam"""
    from jyutvoice_amd import spec
    mel, s, w64, whole, _ = voc
    assert spec.HIFT_DECODE_HALO == 16
    for lo, hi in sr.KEPT:
        good = pu.md(sr.windowed_decode(w64, mel, s, lo, hi, 16), whole[:, 480 * lo:480 * hi])
        short = pu.md(sr.windowed_decode(w64, mel, s, lo, hi, 12), whole[:, 480 * lo:480 * hi])
        print(f"frames [{lo}, {hi}): halo 16 {good:.3e}, halo 12 {short:.3e}")
        assert good <= 1e-12, (lo, hi, good)
        assert short > 1e-5, (lo, hi, short)


def test_f0_halo(voc):
    """fp64, f0 ~ 1e2 Hz: 1e-10 Hz is rounding, and a halo of 4 is off by more than 0.1 Hz"""
    from jyutvoice_amd import spec
    mel, _, w64, _, f0 = voc
    assert spec.HIFT_F0_HALO == 5
    for lo, hi in sr.KEPT:
        good = pu.md(sr.windowed_f0(w64, mel, lo, hi, 5), f0[:, lo:hi])
        short = pu.md(sr.windowed_f0(w64, mel, lo, hi, 4), f0[:, lo:hi])
        print(f"f0 of frames [{lo}, {hi}): halo 5 {good:.3e}, halo 4 {short:.3e}")
        assert good <= 1e-10, (lo, hi, good)
        assert short > 0.1, (lo, hi, short)


# ---- argument errors before the device -----------------------------------------------------------------------------------------------
class _Draws:
    """stands in for a loaded HiFTGenerator: the draws, and nothing that could reach a device"""
    device = torch.device("cpu")

    def _source_draws(self, B):
        return torch.zeros(B, 9), 0, 0

    def _engine(self, B, T):
        raise AssertionError("a device call was reached")


def test_hift_stream_argument_errors():
    import jyutvoice_amd
    from jyutvoice_amd.hifigan.generator import HiFTStream
    with pytest.raises(RuntimeError, match="load_state_dict"):
        jyutvoice_amd.build_default("cuda:0")[1].stream()
    st = HiFTStream(_Draws())
    for bad in (torch.zeros(80, 5), torch.zeros(2, 80, 5), torch.zeros(1, 79, 5), [1.0]):
        with pytest.raises(ValueError, match=r"mel must be \[1, 80, frames\]"):
            st.push(bad)
    wav, s = st.push(torch.zeros(1, 80, 0))      # nothing received: nothing to compute
    assert wav.shape == (1, 0) and s.shape == (1, 1, 0)
    wav, s = st.push(torch.zeros(1, 80, 5))      # five frames: none has a final f0 yet
    assert wav.shape == (1, 0) and st.received == 5 and st.sourced == 0 and st.emitted == 0
    st.finished = True
    with pytest.raises(RuntimeError, match="finish\\(\\) has been called"):
        st.push(torch.zeros(1, 80, 1))
    with pytest.raises(RuntimeError, match="finish\\(\\) has been called"):
        st.finish()


def test_token2wav_stream_argument_errors():
    from jyutvoice_amd.stream import Token2WavStream
    ptok, feat, emb = torch.zeros(1, 7, dtype=torch.int64), torch.zeros(1, 14, 80), torch.zeros(1, 192)
    cases = [((ptok[0], feat, emb, 10), "prompt_token must be an integer"), ((ptok.float(), feat, emb, 10), "prompt_token must be an integer"),
             ((ptok, feat[0], emb, 10), "prompt_feat must be"), ((ptok, torch.zeros(1, 14, 79), emb, 10), "prompt_feat must be"),
             ((ptok, feat, torch.zeros(192), 10), "embedding must be"), ((ptok, feat, emb, 0), "max_tokens must be a positive int"),
             ((ptok, feat, emb, 2.5), "max_tokens must be a positive int")]
    for (a, b, c, cap), word in cases:
        with pytest.raises(ValueError, match=word):
            Token2WavStream(None, None, a, b, c, cap)      # (flow / hift = None: reaching them would be an AttributeError)
    with pytest.raises(ValueError, match="n_timesteps must be positive"):
        Token2WavStream(None, None, ptok, feat, emb, 10, n_timesteps=0)


def test_inference_partial_errors_before_the_device():
    from jyutvoice_amd.flow.flow import CausalMaskedDiffWithXvec
    flow = CausalMaskedDiffWithXvec(vocab_size=6561, input_frame_rate=25)
    emb, one = torch.zeros(1, 192), torch.tensor([1])
    tok = torch.zeros(1, 10, dtype=torch.int64)
    with pytest.raises(ValueError, match="token must be \\[1, N\\]"):
        flow.inference_partial(torch.zeros(2, 10, dtype=torch.int64), one, None, None, None, None, emb, True)
    with pytest.raises(ValueError, match="3 tokens: at least 4 are needed"):
        flow.inference_partial(tok[:, :3], torch.tensor([3]), None, None, None, None, emb, True)
    with pytest.raises(ValueError, match="prompt_feat has 15 frames but the 7 encoded tokens give only 14"):
        flow.inference_partial(tok, torch.tensor([10]), None, None, torch.zeros(1, 15, 80), None, emb, True)
    with pytest.raises(ValueError, match="outside \\[2, 12\\]"):
        flow.inference_partial(tok, torch.tensor([11]), tok[:, :2], torch.tensor([2]), None, None, emb, True)
    with pytest.raises(RuntimeError, match="load_state_dict"):
        flow.inference_partial(tok, torch.tensor([10]), None, None, torch.zeros(1, 14, 80), None, emb, True)
    with pytest.raises(NotImplementedError):      # the reference's own branch keeps raising
        flow.inference(tok, torch.tensor([10]), None, None, None, None, emb, True, False)
