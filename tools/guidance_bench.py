#!/usr/bin/env python
"""What do Euler steps without unconditional twins save?  (DESIGN.md section 5 "Guidance"; writes profiles/guidance_bench.json.)

The closed solve (jv_cfm_solve, n = 10 steps) at three shapes -- the benchmark's 32 x 300 frames, 8 x 300 and 1 x 128 -- under four
settings: guidance rate 0.7 (the default path), rate 0 (no twin is laid out), rate 0 with JV_NO_TWIN_DROP=1 (the twins kept: the
A/B arm, on a second context created under that switch), and a window that guides the first half of the steps (0.7 x 5, then 0 x 5:
the solve changes between the 2B- and the B-sample rows where the route rule allows it).  Device events around each solve, every
setting warmed up at every shape, the settings alternated inside each of --rounds rounds in one process; medians and the spread
(min, max) per setting, and the saving against rate 0.7.

    python tools/guidance_bench.py [--out profiles/guidance_bench.json] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

SHAPES = [(32, 300), (8, 300), (1, 128)]
N_STEPS = 10
WINDOW = [0.7] * (N_STEPS // 2) + [0.0] * (N_STEPS - N_STEPS // 2)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def make_engine(sd, noise, keep_twins):
    from jyutvoice_amd.engine import JV_MODEL_TTS, Engine
    was = os.environ.pop("JV_NO_TWIN_DROP", None)
    if keep_twins:
        os.environ["JV_NO_TWIN_DROP"] = "1"      # (read when the context is created)
    try:
        e = Engine("cuda:0", max_batch=max(b for b, _ in SHAPES), max_frames=max(t for _, t in SHAPES), max_tokens=64)
    finally:
        os.environ.pop("JV_NO_TWIN_DROP", None)
        if was is not None:
            os.environ["JV_NO_TWIN_DROP"] = was
    e.load_state_dict(JV_MODEL_TTS, sd)
    e.load_noise(noise)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "guidance_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    from jyutvoice_amd import synth
    sd, noise = synth.tts_state_dict(), synth.rand_noise()
    drop, keep = make_engine(sd, noise, False), make_engine(sd, noise, True)
    settings = [("rate_0.7", drop, None), ("rate_0", drop, [0.0]), ("rate_0_twins_kept", keep, [0.0]), ("window_first_half", drop, WINDOW)]
    result = {"what": "jv_cfm_solve, n = 10 Euler steps, ms per solve (device events)", "rounds": a.rounds, "n_timesteps": N_STEPS,
              "window": WINDOW, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for B, T in SHAPES:
        g = torch.Generator().manual_seed(B)
        mu = torch.randn(B, 80, T, generator=g).cuda()
        spks = (torch.randn(B, 80, generator=g) * 0.5).cuda()
        cond = torch.zeros_like(mu)

        def run(eng, rates):
            with eng.guidance(rates):
                eng.cfm_solve(mu, None, spks, cond, N_STEPS)

        for _ in range(2):
            for _, eng, rates in settings:
                run(eng, rates)
        torch.cuda.synchronize()
        ms = {name: [] for name, _, _ in settings}
        for r in range(a.rounds):
            order = settings if r % 2 == 0 else settings[::-1]      # alternate the order: drift hits every setting alike
            for name, eng, rates in order:
                ms[name].append(timed(lambda: run(eng, rates)))
        base = statistics.median(ms["rate_0.7"])
        shape = {}
        for name, _, _ in settings:
            m = statistics.median(ms[name])
            shape[name] = {"median_ms": round(m, 3), "min_ms": round(min(ms[name]), 3), "max_ms": round(max(ms[name]), 3),
                           "saving_vs_rate_0.7": round(1.0 - m / base, 4), "all_ms": [round(v, 3) for v in ms[name]]}
        result["shapes"][f"{B}x{T}"] = shape
        print(f"{B} x {T}: " + ", ".join(f"{k} {v['median_ms']:.2f} ms ({100 * v['saving_vs_rate_0.7']:+.1f} %)" for k, v in shape.items()),
              flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
