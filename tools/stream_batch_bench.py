"""what does a step of N concurrent streaming sessions cost in one Token2WavServer, beside N Token2WavStream sessions advanced one
after another?  The request of tools/stream_bench.py -- 75 prompt tokens (150 prompt frames) + 250 tokens, hop 25, ten Euler steps
-- N times over, with a token stream and a seed per session.  A step: every session receives `hop` tokens (the last step closes
them); the server then runs ONE `step()`, the sequential route one `push()` / `finish()` per session.  Every figure is a
device-event interval (a step ends when all its audio is on the device).  The two routes alternate for `--rounds` rounds after two
warm-up rounds (which also capture the solver's step graphs of every geometry); median and minimum over the rounds of the mean
solving step, of every step, and of the whole run.  Synthetic weights.  One JSON line, also written to
<output directory>/stream_batch_bench.json (JV_OUT, default out/; committed under profiles/).

    python tools/stream_batch_bench.py [--rounds 7] [--sessions 1,2,4,8,16] [--prompt 75] [--tokens 250] [--hop 25] [--steps 10]
    python tools/stream_batch_bench.py --count-only N      # no timing: set up, then N sessions through one server once (N = 0: set
                                                           # up only) -- run it under a kernel trace to count a run's launches"""
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
from jyutvoice_amd.stream import Token2WavServer, Token2WavStream, frame_schedule


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3)}


def mark():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def hops_of(tokens, hop):
    return [(i, min(i + hop, tokens)) for i in range(0, tokens, hop)]


def run_server(server, reqs, hop):
    """N sessions through the server -> (ms of every step, samples every step returned in all)"""
    marks, samples = [mark()], []
    sids = [server.open(ptok, feat, emb, seed=k) for k, (tok, ptok, feat, emb) in enumerate(reqs)]
    for lo, hi in hops_of(reqs[0][0].shape[1], hop) + [(None, None)]:
        for sid, (tok, _, _, _) in zip(sids, reqs):
            if lo is None:
                server.close(sid)
            else:
                server.push(sid, tok[0, lo:hi])
        samples.append(sum(w.shape[1] for w in server.step().values()))
        marks.append(mark())
    marks[-1].synchronize()
    return [a.elapsed_time(b) for a, b in zip(marks[:-1], marks[1:])], samples


def run_sequential(flow, hift, reqs, hop, steps):
    """the same calls through one Token2WavStream per session, one after another"""
    marks, samples = [mark()], []
    sessions = [Token2WavStream(flow, hift, ptok, feat, emb, max_tokens=tok.shape[1], n_timesteps=steps, seed=k)
                for k, (tok, ptok, feat, emb) in enumerate(reqs)]
    for lo, hi in hops_of(reqs[0][0].shape[1], hop) + [(None, None)]:
        n = 0
        for s, (tok, _, _, _) in zip(sessions, reqs):
            n += (s.finish() if lo is None else s.push(tok[0, lo:hi])).shape[1]
        samples.append(n)
        marks.append(mark())
    marks[-1].synchronize()
    return [a.elapsed_time(b) for a, b in zip(marks[:-1], marks[1:])], samples


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--sessions", default="1,2,4,8,16")
    p.add_argument("--prompt", type=int, default=75)
    p.add_argument("--tokens", type=int, default=250)
    p.add_argument("--hop", type=int, default=25)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--count-only", type=int, default=None, metavar="N")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_batch_bench.py measures on the GPU; none is visible")
    counts = [int(v) for v in a.sessions.split(",")] if a.count_only is None else [max(a.count_only, 1)]
    flow = CausalMaskedDiffWithXvec(vocab_size=6561, input_frame_rate=25)
    sd = synth.prompt_state_dict()
    sd.update({k: v for k, v in synth.tts_state_dict().items() if k.startswith(("decoder.", "spk_embed_affine_layer."))})
    flow.load_state_dict(sd)
    hift = jyutvoice_amd.build_default("cuda:0")[1]
    hift.load_state_dict(synth.hift_state_dict())
    reqs = []
    for k in range(max(counts)):
        tok, _ = synth.prompt_tokens(1, a.tokens, first_index=3 + 2 * k)
        ptok, _ = synth.prompt_tokens(1, a.prompt, first_index=4 + 2 * k)
        g = torch.Generator().manual_seed(k)
        reqs.append((tok, ptok, torch.randn(1, 2 * a.prompt, 80, generator=g), torch.randn(1, 192, generator=g)))
    plan = frame_schedule(a.prompt, 2 * a.prompt, [hi - lo for lo, hi in hops_of(a.tokens, a.hop)], finish=0)
    solving = [i for i, (solve, _, _) in enumerate(plan) if solve]
    # one reservation for the largest case: the servers and the sessions below never rebuild a context
    servers = {n: Token2WavServer(flow, hift, n, a.tokens, n_timesteps=a.steps, max_prompt_tokens=a.prompt) for n in sorted(counts, reverse=True)}
    torch.cuda.synchronize()
    if a.count_only is not None:
        if a.count_only > 0:
            _, samples = run_server(servers[a.count_only], reqs[:a.count_only], a.hop)
            assert sum(samples) == a.count_only * 480 * plan[-1][2]
        torch.cuda.synchronize()
        print(json.dumps({"count_only": a.count_only, "steps": len(plan), "solving_steps": len(solving)}))
        return
    cases = {}
    for n in counts:
        for _ in range(2):      # warm-up: every geometry of the timed rounds
            run_server(servers[n], reqs[:n], a.hop)
            run_sequential(flow, hift, reqs[:n], a.hop, a.steps)
        torch.cuda.synchronize()
        srv, seq = [], []
        for _ in range(a.rounds):      # alternating: both routes see the same clocks
            t, samples = run_server(servers[n], reqs[:n], a.hop)
            srv.append(t)
            t, samples_seq = run_sequential(flow, hift, reqs[:n], a.hop, a.steps)
            seq.append(t)
            assert samples == samples_seq and sum(samples) == n * 480 * plan[-1][2], (samples, samples_seq)

        def summary(rounds):
            return {"solving_step": stats([sum(r[i] for i in solving) / len(solving) for r in rounds]),
                    "per_step": [stats([r[i] for r in rounds]) for i in range(len(plan))], "run_total": stats([sum(r) for r in rounds])}

        s, q = summary(srv), summary(seq)
        spread = max(v["solving_step"]["median_ms"] - v["solving_step"]["min_ms"] for v in (s, q))
        cases[str(n)] = {"server": s, "sequential": q, "min_to_median_spread_ms": round(spread, 3),
                         "sequential_minus_server_ms": round(q["solving_step"]["median_ms"] - s["solving_step"]["median_ms"], 3),
                         "sequential_over_server": round(q["solving_step"]["median_ms"] / s["solving_step"]["median_ms"], 3)}
        print(f"N = {n}: solving step, server {s['solving_step']} sequential {q['solving_step']}", flush=True)
    out = {"what": "a step of N streaming sessions: one Token2WavServer.step() beside N Token2WavStream pushes one after another; device "
                   "events, alternating rounds after two warm-up rounds, median / min; solving_step = the mean over the steps in which "
                   "the sessions solve",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "n_timesteps": a.steps, "prompt_tokens": a.prompt,
           "prompt_frames": 2 * a.prompt, "tokens": a.tokens, "hop": a.hop, "schedule_tokens_solved_first_frame_end_frame": plan,
           "solving_steps": solving, "sessions": cases}
    print(json.dumps(out), flush=True)
    d = os.environ.get("JV_OUT") or os.path.join(REPO, "out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "stream_batch_bench.json"), "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
