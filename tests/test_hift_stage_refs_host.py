"""CPU: the stage references of tests/hift_stage_ref.py, without a GPU.

(a) They are the model: the fp64 chain of formulas equals oracle.hift.decode's path -- torch.stft, the `stage{i}` and `post` taps,
    torch.istft and the clip -- to 1e-10 relative on every utterance of every case of test_gpu_hift_stages.py.
(b) They can tell: each plausible mistake, applied to ONE stage reference in fp64 and fed the fp64 chain's previous stage, lands
    more than RATIO x the fp32 floor from the true fp64 stage on at least one row of at least one utterance of those cases -- the
    bound test_gpu_hift_stages.py holds the kernels to.  A mistake no case showed would be answered by changing the cases.
(c) The conditions the cases are built on hold on the fp64 reference alone: clipped share <= 1 % everywhere but in `clamp`, `mags`
    spreads the utterances' conv_pre maxima over 8 x or more, `clamp` drives 5 .. 50 % of the log-magnitudes above ln 100, and the
    compact geometry is taken exactly where the GPU file says."""
import pytest
import torch

import hift_stage_ref as hs
import parity_util as pu
import test_gpu_fused_ops as fo      # distances / RATIO (a module object: none of its tests is collected here)

RATIO = fo.RATIO
UTTERANCES = [(name, b) for name, (_, _, lens) in hs.CASES.items() for b, L in enumerate(lens) if L > 0]


@pytest.fixture(scope="module", autouse=True)
def threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


def close(a, b, tol=1e-10):
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("name,b", UTTERANCES)
def test_references_are_the_oracle(name, b):
    from oracle import hift as ohift
    mel, s, lens = hs.inputs(name)
    L, w64 = lens[b], hs.weights(name)[torch.float64]
    got = hs.oracle_chain(name, b)
    taps = {}
    with torch.inference_mode():
        wav = ohift.decode(w64, mel[b:b + 1, :, :L].double(), s[b:b + 1, :, :480 * L].double(), taps)
        st = ohift.stft(s[b, :, :480 * L].double())
    assert close(got["STFT"], st), "STFT"
    for i in range(3):
        assert close(got[f"X{i}"], taps[f"stage{i}"]), f"X{i}"
    assert close(got["POST"], taps["post"]), "POST"
    assert close(got["WAV"], wav), "WAV"
    # the weight-free formulas alone, fed the oracle's own tensors
    assert close(hs.ola(hs.frames(taps["post"], torch.float64), torch.float64), wav), "frames + ola"
    for tap in hs.TAPS + ("WAV",):
        assert got[tap].shape[2 if tap != "WAV" else 1] == hs.live(tap, L), tap


# mistake -> the stage references it is applied to
MUTANTS = [("polyphase_off", "UP0"), ("polyphase_off", "UP1"), ("polyphase_off", "UP2"),
           ("up_pad_plus1", "UP0"), ("up_pad_plus1", "UP1"), ("up_pad_plus1", "UP2"),
           ("reflect_tau1", "UP2"), ("reflect_missing", "UP2"),
           ("sd0_pad8", "SI0"), ("sd1_pad0", "SI1"),
           ("hann_symmetric", "STFT"), ("reflect_nvalid", "STFT"), ("stft_reflect_T", "STFT"), ("imag_sign", "STFT"),
           ("post_lrelu_01", "POST"),
           ("mrf_no_div", "X0"), ("mrf_no_div", "X1"), ("mrf_no_div", "X2"),
           ("no_clamp", "FRAMES"), ("no_sin", "FRAMES"), ("bin8_doubled", "FRAMES"),
           ("envelope_const", "WAV"), ("clip_1", "WAV")]


def compared(name, tap, ref):
    """the waveform of `clamp` is compared only where the reference is below the clip (test_gpu_hift_stages.py)"""
    if name == "clamp" and tap == "WAV":
        return lambda t: t * (ref["WAV_RAW"].abs() < pu.AUDIO_LIMIT)
    return lambda t: t


@pytest.mark.parametrize("mut,tap", MUTANTS)
def test_reference_catches(mut, tap):
    seen = {}
    for name, b in UTTERANCES:
        L, ws, ref = hs.CASES[name][2][b], hs.weights(name), hs.oracle_chain(name, b)
        cut = compared(name, tap, ref)
        r64 = hs.rows_of(tap, cut(ref[tap]))
        r32 = hs.rows_of(tap, cut(hs.evaluate(tap, ws, ref, L, torch.float32).double()))
        bad = hs.rows_of(tap, cut(hs.evaluate(tap, ws, ref, L, torch.float64, mut)))
        md, fl = fo.distances(bad, r64, r32, slice(None))
        assert fl > 0.0, (name, b)
        seen[(name, b)] = (md, RATIO * fl)
        if md > RATIO * fl:
            return
    assert False, (mut, tap, seen)


@pytest.mark.parametrize("name", list(hs.CASES))
def test_case_conditions(name):
    _, T, lens = hs.CASES[name]
    compact, uniform = hs.compact_rows(T, lens)
    assert (len(lens) > 1 and compact * 100 <= uniform * 92) == (name in hs.COMPACT_CASES), (compact, uniform)
    refs = [hs.oracle_chain(name, b) for b, L in enumerate(lens) if L > 0]
    if name == "clamp":
        above = torch.cat([(r["POST"][0, :hs.NB] > hs.LN100).flatten() for r in refs]).double().mean()
        assert 0.05 <= float(above) <= 0.50, float(above)
    else:
        for r in refs:
            assert pu.clamp_share(r["WAV"]) <= pu.CLAMP_CAP, pu.clamp_share(r["WAV"])
    if name == "mags":
        peak = [float(r["PRE"].abs().max()) for r in refs]
        assert max(peak) >= 8.0 * min(peak), peak
