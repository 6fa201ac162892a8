#!/usr/bin/env python
"""In-flight batching, measured (DESIGN.md section 5 "In-flight batching"; writes profiles/serve_bench.json).

A. Price of a pool step.  32 requests x 300 frames, all at the same step: one jv_cfm_pool_step against one step of jv_cfm_solve
   on the same batch (solve time / n).  The pool step pays for the two-launch resnets (no shared time embedding, so no whole-resnet
   launch), the per-sample time embedding, gather / scatter and no shared first-step twin.  Device events, every shape warmed up,
   the two sides alternated for --rounds rounds in one process, medians.
B. What it buys.  --requests requests of 150 tokens (300 frames each) arrive at a fixed interval, at two loads -- saturating (the
   measured batch-32 pass time / 32) and half of it -- and are served two ways in the same run: as closed batches (whatever is
   waiting when the previous batch ends, up to 32, through synthesise(batched=True) + hift.inference) and by a SynthServer with 32
   slots.  Latency from arrival to audio on the device (the host waits for the device after every batch / step), frames per second.

    python tools/serve_bench.py [--out profiles/serve_bench.json] [--rounds 5] [--requests 96]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

KEYS = ("x", "x_lengths", "lang", "tone", "word_pos", "syllable_pos", "spk_embed")
B, T, N_STEPS, TOKENS = 32, 300, 10, 150


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def part_a(eng, rounds):
    from jyutvoice_amd.serve import step_table
    g = torch.Generator().manual_seed(0)
    mu = torch.randn(B, 80, T, generator=g).cuda()
    spks = (torch.randn(B, 80, generator=g) * 0.5).cuda()
    cond = torch.zeros_like(mu)
    pool = eng.cfm_pool(B, T)
    tt, dts = step_table(N_STEPS)
    slots, lens = list(range(B)), [T] * B

    def closed():
        eng.cfm_solve(mu, None, spks, cond, N_STEPS)

    def pooled():
        for k in range(N_STEPS):
            eng.cfm_pool_step(pool, slots, lens, [tt[k]] * B, [dts[k]] * B)

    def admit():
        eng.cfm_pool_admit(pool, mu, lens, None, None, [0] * B, spks, slots, [1.0] * B)

    for _ in range(2):
        closed()
        admit()
        pooled()
    ms_closed, ms_pool, ms_admit = [], [], []
    for _ in range(rounds):
        ms_closed.append(timed(closed) / N_STEPS)
        ms_admit.append(timed(admit))
        ms_pool.append(timed(pooled) / N_STEPS)
    c, p = statistics.median(ms_closed), statistics.median(ms_pool)
    return {"shape": f"{B} requests x {T} frames, {N_STEPS} steps", "rounds": rounds, "closed_solve_ms_per_step": round(c, 3),
            "pool_step_ms": round(p, 3), "ratio_pool_over_closed": round(p / c, 4), "admit_ms": round(statistics.median(ms_admit), 3),
            "closed_all": [round(v, 3) for v in ms_closed], "pool_all": [round(v, 3) for v in ms_pool]}


def percentile(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def summary(lat, frames, span):
    return {"median_latency_ms": round(1e3 * statistics.median(lat), 2), "p95_latency_ms": round(1e3 * percentile(lat, 0.95), 2),
            "frames_per_s": round(frames / span, 1), "makespan_ms": round(1e3 * span, 1)}


def serve_closed(tts, hift, batch, n, interval):
    arrive = [i * interval for i in range(n)]
    lat, frames, nxt = [0.0] * n, 0, 0
    t0 = time.perf_counter()
    while nxt < n:
        while time.perf_counter() - t0 < arrive[nxt]:
            pass
        now = time.perf_counter() - t0
        hi = nxt
        while hi < n and hi - nxt < B and arrive[hi] <= now:
            hi += 1
        res = tts.synthesise(*[batch[k][nxt:hi] for k in KEYS], None, n_timesteps=N_STEPS, batched=True)
        hift.inference(res["mel"], lengths=res["mel_lengths"])
        torch.cuda.synchronize()
        done = time.perf_counter() - t0
        frames += int(res["mel_lengths"].sum())
        for i in range(nxt, hi):
            lat[i] = done - arrive[i]
        nxt = hi
    return summary(lat, frames, time.perf_counter() - t0)


def serve_inflight(server, batch, n, interval):
    arrive = [i * interval for i in range(n)]
    lat, frames, nxt, left = [0.0] * n, 0, 0, n
    rid0 = None
    t0 = time.perf_counter()
    while left:
        now = time.perf_counter() - t0
        while nxt < n and arrive[nxt] <= now:
            rid = server.submit(*[batch[k][nxt:nxt + 1] for k in KEYS], n_timesteps=N_STEPS, seed=nxt)
            rid0 = rid if rid0 is None else rid0
            nxt += 1
        if not server.pending():
            continue
        out = server.step()
        torch.cuda.synchronize()
        done = time.perf_counter() - t0
        for rid, r in out.items():
            lat[rid - rid0] = done - arrive[rid - rid0]
            frames += r["mel_length"]
            left -= 1
    return summary(lat, frames, time.perf_counter() - t0)


def part_b(tts, hift, rounds, n):
    from jyutvoice_amd import synth
    from jyutvoice_amd.serve import SynthServer
    batch = synth.batch(n, TOKENS)
    server = SynthServer(tts, hift, max_sessions=B, max_frames=T + 20, max_tokens=TOKENS)

    def one_pass():
        res = tts.synthesise(*[batch[k][:B] for k in KEYS], None, n_timesteps=N_STEPS, batched=True)
        hift.inference(res["mel"], lengths=res["mel_lengths"])

    one_pass()
    pass_ms = statistics.median(timed(one_pass) for _ in range(3))
    # warm every shape the two policies will meet: partial closed batches, and a full pool
    for k in (1, 8, 16):
        res = tts.synthesise(*[batch[key][:k] for key in KEYS], None, n_timesteps=N_STEPS, batched=True)
        hift.inference(res["mel"], lengths=res["mel_lengths"])
    serve_inflight(server, batch, B + 4, 0.0)
    out = {"requests": n, "tokens": TOKENS, "n_timesteps": N_STEPS, "batch32_pass_ms": round(pass_ms, 2), "rounds": rounds, "loads": {}}
    for name, interval in (("saturating", pass_ms / 1e3 / B), ("half", 2 * pass_ms / 1e3 / B)):
        runs = {"closed_batches": [], "inflight": []}
        for _ in range(rounds):      # the two policies alternate
            runs["closed_batches"].append(serve_closed(tts, hift, batch, n, interval))
            runs["inflight"].append(serve_inflight(server, batch, n, interval))
        med = {pol: {k: round(statistics.median(r[k] for r in rs), 2) for k in rs[0]} for pol, rs in runs.items()}
        out["loads"][name] = dict(med, arrival_interval_ms=round(1e3 * interval, 3))
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "serve_bench.json"))
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--requests", type=int, default=96)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no AMD GPU visible: jyutvoice_amd has no CPU path")
    import jyutvoice_amd
    from jyutvoice_amd import synth
    from jyutvoice_amd.runtime import get_runtime
    tts, hift = jyutvoice_amd.build_default("cuda:0")
    tts.load_state_dict(synth.tts_state_dict(fixed_duration=2.0))      # 150 tokens -> 300 frames, the headline shape
    hift.load_state_dict(synth.hift_state_dict())
    hift.manual_seed(0)
    eng = get_runtime("cuda:0").ensure(B, T + 20, TOKENS)
    doc = {"what": "tools/serve_bench.py: in-flight batching on one MI355X, device events / host clock with a device wait per step",
           "device": torch.cuda.get_device_name(0), "A_pool_step_price": part_a(eng, args.rounds),
           "B_arrivals": part_b(tts, hift, args.rounds, args.requests)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
