"""what does a streaming session cost beside the one-shot route?  One request of 75 prompt tokens (150 prompt frames) and 250
tokens, pushed 25 at a time through jyutvoice_amd.stream.Token2WavStream: time to the first audio, time per push, the session's
total, and the one-shot total (`inference(streaming=True, finalize=True)` + `HiFTGenerator.inference` on all 250 tokens).  The
session solves the aligned prefix again on every push that lengthens it, so its total is expected to exceed the one-shot total:
the ratio is the price of the first audio arriving early.  Synthetic weights.  Every figure is a device-event interval (a push ends
when its audio is on the device) after a warm-up session and a warm-up one-shot pass -- which also capture the solver's step graphs
of every geometry the timed rounds use; median and minimum over the rounds.  One JSON line, also written to
<output directory>/stream_bench.json (JV_OUT, default out/; committed under profiles/).

    python tools/stream_bench.py [--rounds 7] [--prompt 75] [--tokens 250] [--hop 25] [--steps 10]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch

import jyutvoice_amd
from jyutvoice_amd import synth
from jyutvoice_amd.flow.flow import CausalMaskedDiffWithXvec
from jyutvoice_amd.stream import Token2WavStream, frame_schedule


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3)}


def session(flow, hift, ptok, feat, emb, tok, hop, steps):
    """one session -> (ms from its start to the end of every call, samples every call returned); the last call is finish()"""
    marks = [torch.cuda.Event(enable_timing=True)]
    marks[0].record()
    s = Token2WavStream(flow, hift, ptok, feat, emb, max_tokens=tok.shape[1], n_timesteps=steps, seed=0)
    samples = []
    for i in range(0, tok.shape[1], hop):
        samples.append(s.push(tok[0, i:i + hop]).shape[1])
        marks.append(torch.cuda.Event(enable_timing=True))
        marks[-1].record()
    samples.append(s.finish().shape[1])
    marks.append(torch.cuda.Event(enable_timing=True))
    marks[-1].record()
    marks[-1].synchronize()
    return [marks[0].elapsed_time(m) for m in marks[1:]], samples


def oneshot(flow, hift, ptok, feat, emb, tok, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    P, N, F = ptok.shape[1], tok.shape[1], feat.shape[1]
    a.record()
    hift.manual_seed(0)
    mel, _ = flow.inference(tok, torch.tensor([N]), ptok, torch.tensor([P]), feat, torch.tensor([F]), emb, True, True, n_timesteps=steps)
    wav, _ = hift.inference(mel)
    b.record()
    b.synchronize()
    return a.elapsed_time(b), wav.shape[1]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--prompt", type=int, default=75)
    p.add_argument("--tokens", type=int, default=250)
    p.add_argument("--hop", type=int, default=25)
    p.add_argument("--steps", type=int, default=10)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench.py measures on the GPU; none is visible")
    flow = CausalMaskedDiffWithXvec(vocab_size=6561, input_frame_rate=25)
    sd = synth.prompt_state_dict()
    sd.update({k: v for k, v in synth.tts_state_dict().items() if k.startswith(("decoder.", "spk_embed_affine_layer."))})
    flow.load_state_dict(sd)
    hift = jyutvoice_amd.build_default("cuda:0")[1]
    hift.load_state_dict(synth.hift_state_dict())
    tok, _ = synth.prompt_tokens(1, a.tokens, first_index=3)
    ptok, _ = synth.prompt_tokens(1, a.prompt, first_index=4)
    g = torch.Generator().manual_seed(0)
    feat, emb = torch.randn(1, 2 * a.prompt, 80, generator=g), torch.randn(1, 192, generator=g)
    args = (flow, hift, ptok, feat, emb, tok)
    plan = frame_schedule(a.prompt, 2 * a.prompt, [min(a.hop, a.tokens - i) for i in range(0, a.tokens, a.hop)], finish=0)
    for _ in range(2):      # warm-up: every geometry of the timed rounds
        session(*args, a.hop, a.steps)
        oneshot(*args, a.steps)
    torch.cuda.synchronize()
    ends, shots, samples = [], [], None
    for _ in range(a.rounds):      # interleaved: both routes see the same clocks
        e, samples = session(*args, a.hop, a.steps)
        ends.append(e)
        t, n = oneshot(*args, a.steps)
        shots.append(t)
        assert sum(samples) == n == 480 * plan[-1][2], (samples, n, plan[-1])
    first_call = next(i for i, n in enumerate(samples) if n > 0)
    calls = len(ends[0])
    per_call = [stats([e[i] - (e[i - 1] if i else 0.0) for e in ends]) for i in range(calls)]
    total, shot = stats([e[-1] for e in ends]), stats(shots)
    out = {"what": "Token2WavStream (tokens pushed `hop` at a time, the aligned prefix solved again on every push that lengthens it) beside "
                   "the one-shot route on the same request; device events, interleaved rounds after two warm-up rounds, median / min",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "n_timesteps": a.steps, "prompt_tokens": a.prompt,
           "prompt_frames": 2 * a.prompt, "tokens": a.tokens, "hop": a.hop, "audio_s": round(sum(samples) / 24000.0, 3),
           "schedule_tokens_solved_first_frame_end_frame": plan, "samples_per_call": samples,
           "time_to_first_audio": dict(stats([e[first_call] for e in ends]), call=first_call),
           "per_call": per_call, "solving_pushes": stats([e[i] - (e[i - 1] if i else 0.0) for e in ends for i in range(calls - 1) if plan[i][0]]),
           "session_total": total, "oneshot_total": shot, "session_over_oneshot": round(total["median_ms"] / shot["median_ms"], 3)}
    line = json.dumps(out)
    print(line, flush=True)
    d = os.environ.get("JV_OUT") or os.path.join(REPO, "out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "stream_bench.json"), "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
