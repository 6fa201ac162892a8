"""GPU parity of the token-to-mel route: jv_flow_encoder_fwd / jv_flow_token2mel and `CausalMaskedDiffWithXvec.inference`
(jyutvoice/flow/flow.py:300-358) against the imported reference's outputs (G13, G14), plus the properties the route promises:
in-kernel concatenation, streaming, batches as loops of B = 1, a flow-only context, no quadratic workspace, the CLI."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import REPO, load_golden

pytestmark = pytest.mark.gpu


def md(a, b):
    return float((a.detach().cpu().float() - b.detach().cpu().float()).abs().max())


def flow_state_dict(prompt_sd, tts_sd):
    sd = dict(prompt_sd)
    sd.update({k: v for k, v in tts_sd.items() if k.startswith(("decoder.", "spk_embed_affine_layer."))})
    return sd


@pytest.fixture(scope="module")
def flow(prompt_sd, tts_sd):
    """the flow on a FRESH runtime that is given nothing but the 1121-key dict: a flow-only context (JV_MODEL_PROMPT + JV_MODEL_FLOW)"""
    from jyutvoice_amd.flow.flow import CausalMaskedDiffWithXvec
    from jyutvoice_amd.runtime import Runtime
    sd = flow_state_dict(prompt_sd, tts_sd)
    assert len(sd) == 1121
    m = CausalMaskedDiffWithXvec(vocab_size=6561, input_frame_rate=25, runtime=Runtime("cuda:0"))
    m.load_state_dict(sd)
    return m


@pytest.fixture(scope="module")
def eng(flow):
    return flow._rt().ensure(3, 256, 1)


@pytest.fixture(scope="module")
def g13():
    return load_golden("G13_flow_encoder")


@pytest.fixture(scope="module")
def g14():
    return load_golden("G14_token2mel")


def test_encoder_against_reference(eng, g13):
    """93 tokens (three chunks of 25, the last one partial), no prompt, both streaming values; and the fused-attention route
    against the three-GEMM route of jv_prompt_encoder_fwd on the same tokens.  5e-5: the bound test_gpu_prompt.py holds the same
    arithmetic to"""
    tok, lens = g13["tok"], torch.tensor([93])
    for tag, streaming in (("full", False), ("stream", True)):
        h, hl = eng.flow_encoder(None, None, tok, lens, streaming=streaming)
        assert h.shape == (1, 186, 80) and hl.tolist() == [186]
        e = md(h, g13["h_" + tag])
        print(f"flow encoder vs G13 ({tag}): {e:.3e}")
        assert e <= 5e-5, tag
    h, _ = eng.flow_encoder(None, None, tok, lens, streaming=False)
    e = md(h, eng.prompt_encoder(tok, lens))
    print(f"flow encoder (fused attention) vs prompt encoder (three GEMMs): {e:.3e}")
    assert e <= 5e-5


def test_concatenation_inside_the_kernel(eng, g13):
    """prompt 33 | tokens 60 as two tensors = the 93 tokens as one, bit for bit; NaN-free garbage ids behind the lengths change
    nothing"""
    tok = g13["tok"]
    for streaming in (False, True):
        one, _ = eng.flow_encoder(None, None, tok, torch.tensor([93]), streaming=streaming)
        two, hl = eng.flow_encoder(tok[:, :33], torch.tensor([33]), tok[:, 33:], torch.tensor([60]), streaming=streaming)
        assert hl.tolist() == [186] and torch.equal(one, two)
    g = torch.Generator().manual_seed(1)
    wide = []
    for fill in (None, "garbage"):
        p = torch.zeros(1, 40, dtype=torch.int64)
        t = torch.zeros(1, 70, dtype=torch.int64)
        if fill:
            p = torch.randint(-(2 ** 40), 2 ** 40, (1, 40), generator=g)
            t = torch.randint(-(2 ** 40), 2 ** 40, (1, 70), generator=g)
        p[:, :33], t[:, :60] = tok[:, :33], tok[:, 33:]
        h, hl = eng.flow_encoder(p, torch.tensor([33]), t, torch.tensor([60]), streaming=True)
        assert h.shape == (1, 220, 80) and hl.tolist() == [186]
        wide.append(h)
    assert torch.equal(wide[0], wide[1])
    assert float(wide[0][:, 186:].abs().max()) == 0.0
    one, _ = eng.flow_encoder(None, None, tok, torch.tensor([93]), streaming=True)
    assert md(wide[0][:, :186], one) <= 2e-5      # same kernels at another row stride


def test_streaming_property(eng, g13):
    """with streaming=True the rows of chunks that ended at least the look-ahead (3 tokens) before the end of the shorter input are
    final: floor((60 - 3) / 25) = 2 chunks = 100 rows of h agree between the first 60 tokens and all 93 (2e-5, the bound of
    test_streaming_two_chunks); without streaming they do not (the reference differs by 5e-2)"""
    tok = g13["tok"]
    got = {}
    for streaming in (True, False):
        h60, _ = eng.flow_encoder(None, None, tok[:, :60], torch.tensor([60]), streaming=streaming)
        h93, _ = eng.flow_encoder(None, None, tok, torch.tensor([93]), streaming=streaming)
        got[streaming] = md(h60[:, :100], h93[:, :100])
    print(f"rows [0, 100) of 60 vs 93 tokens: streaming {got[True]:.3e}  full {got[False]:.3e}")
    assert got[True] <= 2e-5
    assert got[False] > 1e-3


def g14_args(g):
    return (g["token"], torch.tensor([60]), g["prompt_token"], torch.tensor([33]), g["prompt_feat"], torch.tensor([66]), g["embedding"])


def test_inference_against_reference(flow, g14):
    """end to end on the flow-only context: prompt 33 + 60 tokens, prompt_feat 66 frames, both streaming values, against the mel of
    the imported CausalMaskedDiffWithXvec (1e-3: the project's mel tolerance, test_prompted_synthesis_uses_prompt_h)"""
    mels = {}
    for tag, streaming in (("full", False), ("stream", True)):
        mel, none = flow.inference(*g14_args(g14), streaming, True)
        assert none is None and mel.dtype == torch.float32 and mel.shape == (1, 80, 120)
        e = md(mel, g14["mel_" + tag])
        print(f"token2mel vs G14 ({tag}): {e:.3e}")
        assert e <= 1e-3, tag
        mels[tag] = mel
    assert md(mels["full"], mels["stream"]) > 1e-2      # the reference's two modes differ by 0.57
    assert flow.mel_lengths.tolist() == [120]


def test_flow_only_context_and_shared_decoder(flow, g14, prompt_sd, tts_sd):
    """the text side of a flow-only context says what is missing; a runtime that holds a full JyutVoiceTTS gives the same mel bit
    for bit through decoder='shared'"""
    from jyutvoice_amd import spec, synth
    from jyutvoice_amd._lib import JvError
    from jyutvoice_amd.engine import JV_MODEL_TTS
    from jyutvoice_amd.flow.flow import CausalMaskedDiffWithXvec
    from jyutvoice_amd.runtime import Runtime
    e = flow._rt().ensure(1, 64, 32)
    u = synth.batch(1, 8)
    with pytest.raises(JvError) as err:
        e.encoder(u["x"], u["x_lengths"], u["lang"], u["tone"], u["word_pos"], u["syllable_pos"], u["spk_embed"])
    assert err.value.code == 2 and "flow decoder only" in err.value.msg and "encoder.*" in err.value.msg
    with pytest.raises(RuntimeError, match="holds no finalized JyutVoiceTTS"):
        CausalMaskedDiffWithXvec(vocab_size=6561, runtime=Runtime("cuda:0")).load_state_dict(prompt_sd, decoder="shared")
    rt = Runtime("cuda:0")
    rt.set_weights(JV_MODEL_TTS, {k: tts_sd[k] for k in spec.TTS_INVENTORY})      # what JyutVoiceTTS.load_state_dict does
    with pytest.raises(RuntimeError, match="decoder=.shared."):
        CausalMaskedDiffWithXvec(vocab_size=6561, runtime=rt).load_state_dict(flow_state_dict(prompt_sd, tts_sd))
    shared = CausalMaskedDiffWithXvec(vocab_size=6561, runtime=rt)
    shared.load_state_dict(flow_state_dict(prompt_sd, tts_sd), decoder="shared")
    for streaming in (False, True):
        a, _ = flow.inference(*g14_args(g14), streaming, True)
        b, _ = shared.inference(*g14_args(g14), streaming, True)
        assert torch.equal(a, b), streaming
    rt.engine.close()


def test_batch_equals_singles(flow):
    """batched=True with three utterances (tokens 60 / 17 / 40, prompts 33 / 0 / 12, f_b = 66 / 0 / 20) = the three B = 1 calls on
    tensors cut to their own lengths (2e-5: same kernels, other tile occupancy), zeros behind every y_b; NaN in prompt_feat behind
    f_b, garbage ids behind the token lengths and NaN in embedding rows of no utterance change nothing"""
    from jyutvoice_amd import synth
    n, p, f = [60, 17, 40], [33, 0, 12], [66, 0, 20]
    tok, _ = synth.prompt_tokens(3, 60, lengths=n, first_index=21)
    ptok, _ = synth.prompt_tokens(3, 33, lengths=[33, 1, 12], first_index=31)
    g = torch.Generator().manual_seed(6)
    feat = torch.randn(3, 66, 80, generator=g)
    emb_all = torch.randn(5, 192, generator=g)
    emb_all[3:] = float("nan")                     # rows of no utterance
    emb = emb_all[:3]
    lens = (torch.tensor(n), torch.tensor(p), torch.tensor(f))
    for streaming in (False, True):
        mel, _ = flow.inference(tok, lens[0], ptok, lens[1], feat, lens[2], emb, streaming, True, batched=True, n_timesteps=4)
        y = [2 * (p[b] + n[b]) - f[b] for b in range(3)]
        assert mel.shape == (3, 80, max(y)) and flow.mel_lengths.tolist() == y
        for b in range(3):
            assert float(mel[b, :, y[b]:].abs().max()) == 0.0 if y[b] < max(y) else True
            solo, _ = flow.inference(tok[b:b + 1, :n[b]], lens[0][b:b + 1], ptok[b:b + 1, :p[b]], lens[1][b:b + 1], feat[b:b + 1, :f[b]],
                                     lens[2][b:b + 1], emb[b:b + 1], streaming, True, n_timesteps=4)
            assert solo.shape == (1, 80, y[b])
            e = md(solo, mel[b:b + 1, :, :y[b]])
            print(f"batch vs single, utterance {b}, streaming={streaming}: {e:.3e}")
            assert e <= 2e-5, (b, streaming)
        hostile_feat, hostile_tok, hostile_ptok = feat.clone(), tok.clone(), ptok.clone()
        for b in range(3):
            hostile_feat[b, f[b]:] = float("nan")
            hostile_tok[b, n[b]:] = -(2 ** 33) - b
            hostile_ptok[b, p[b]:] = 2 ** 35 + b
        again, _ = flow.inference(hostile_tok, lens[0], hostile_ptok, lens[1], hostile_feat, lens[2], emb, streaming, True, batched=True,
                                  n_timesteps=4)
        assert torch.equal(again, mel), streaming


def test_length_errors_from_the_library(eng):
    """jv_flow_token2mel rejects an f_b outside [0, min(F, T_b)] naming the utterance, before the solve is launched"""
    from jyutvoice_amd._lib import JvError
    tok = torch.zeros(2, 10, dtype=torch.int64)
    feat = torch.zeros(2, 30, 80)
    emb = torch.ones(2, 192)
    for bad, word in (([4, 13], "utterance 1: prompt_feat length 13"), ([-1, 0], "utterance 0: prompt_feat length -1")):
        with pytest.raises(JvError) as err:
            eng.flow_token2mel(None, None, tok, torch.tensor([10, 6]), feat, torch.tensor(bad), emb, n_timesteps=2)
        assert err.value.code == 1 and word in err.value.msg
    mel, ml = eng.flow_token2mel(None, None, tok, torch.tensor([10, 6]), feat, torch.tensor([4, 12]), emb, n_timesteps=2)
    assert ml.tolist() == [16, 0] and float(mel[1].abs().max()) == 0.0 and torch.isfinite(mel).all()


WORKER = r"""
import sys, torch
from jyutvoice_amd import synth
from jyutvoice_amd.engine import JV_MODEL_PROMPT
from jyutvoice_amd.flow.encoder import DIV_TERM_KEY, div_term
from jyutvoice_amd.runtime import Runtime
rt = Runtime("cuda:0")
sd = synth.prompt_state_dict()
sd[DIV_TERM_KEY] = div_term()
rt.set_weights(JV_MODEL_PROMPT, sd)
eng = rt.ensure(2, 2048, 1)
tok, lens = synth.prompt_tokens(2, 1024)
tok, lens = tok.cuda(), lens.cuda()
torch.cuda.synchronize()
free0, _ = torch.cuda.mem_get_info()
h, hl = eng.flow_encoder(None, None, tok, lens, streaming=True)
torch.cuda.synchronize()
free1, _ = torch.cuda.mem_get_info()
assert torch.isfinite(h).all() and hl.tolist() == [2048, 2048]
print("GROWTH_MB", (free0 - free1) / 1e6)
"""


def test_no_quadratic_workspace():
    """a fresh process, B = 2 x 1024 tokens (2048 mel-rate rows): device memory in use grows by less than 400 MB across the call.
    ac + bd of the three-GEMM route alone would be 2 * 8 * 2048 * 6144 * 4 B = 805 MB; the row buffers come to about 120 MB"""
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", WORKER], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    growth = float(r.stdout.split("GROWTH_MB")[1].split()[0])
    print(f"device memory growth across jv_flow_encoder_fwd(B = 2, 1024 tokens): {growth:.1f} MB")
    assert growth < 400.0


def test_cli_token2wav(tmp_path, g14):
    """infer.py --token2wav on a two-request list with synthetic weights: two finite, non-silent wavs of the expected lengths"""
    import infer
    from jyutvoice_amd.utils.audio import load_wav
    g = torch.Generator().manual_seed(2)
    reqs = [{"speech_token": g14["token"][0, :20].tolist(), "embedding": torch.randn(192, generator=g).tolist(),
             "prompt_token": g14["prompt_token"][0, :8].tolist(), "prompt_feat": g14["prompt_feat"][0, :16].tolist()},
            {"speech_token": g14["token"][0, 20:32].tolist(), "embedding": torch.randn(192, generator=g).tolist()}]
    (tmp_path / "list.json").write_text(json.dumps(reqs))
    infer.main(["--output", str(tmp_path / "out.wav"), "--token2wav", str(tmp_path / "list.json"), "--synthetic", "1", "--n_timesteps", "2",
                "--streaming"])
    for b, frames in enumerate([2 * 28 - 16, 2 * 12]):
        wav, rate = load_wav(str(tmp_path / f"out_{b:03d}.wav"))
        assert rate == 24000 and wav.shape[-1] == 480 * frames
        assert torch.isfinite(wav).all() and float(wav.abs().max()) > 1e-4
