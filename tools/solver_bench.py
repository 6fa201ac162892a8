#!/usr/bin/env python
"""What does an estimator evaluation cost inside a midpoint / Heun solve, against one inside an Euler solve?  (DESIGN.md section 5
"Solver"; writes profiles/solver_bench.json.)

The closed solve (jv_cfm_solve) at three shapes -- the benchmark's 32 x 300 frames, 8 x 300 and 1 x 128 -- spending the same 10
estimator evaluations three ways: Euler n = 10, midpoint n = 5, Heun n = 5.  The comparison is PER EVALUATION (ms per solve / 10)
against the Euler solve of this build at the same geometry, whose launches are the parent commit's (the default path is untouched;
bench.py's line before and after is the check of that).  Two more Euler arms separate what a second-order solve does without:
`euler_no_share` (JV_NO_CFG_SHARE=1 at context creation: 2B samples in the first step too, as every second-order evaluation runs)
and `euler_graph` (jv_flow_set_graph: the captured step, which second-order solves never replay).  So
    midpoint / heun  vs  euler_no_share   = the stage kernel (solver_stage in euler_cfg's place), nothing else differs
    euler_no_share   vs  euler            = the shared first twin a second-order solve does not take
    euler_graph      vs  euler            = the captured step it does not replay
Device events around each solve, every arm warmed up at every shape, the arms alternated inside each of --rounds rounds in one
process; medians and the spread (min, max) per arm.  Nothing here says anything about quality per evaluation.

    python tools/solver_bench.py [--out profiles/solver_bench.json] [--rounds 9]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

SHAPES = [(32, 300), (8, 300), (1, 128)]
EVALS = 10


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def make_engine(sd, noise, no_share=False, graph=False):
    from jyutvoice_amd.engine import JV_MODEL_TTS, Engine
    was = os.environ.pop("JV_NO_CFG_SHARE", None)
    if no_share:
        os.environ["JV_NO_CFG_SHARE"] = "1"      # (read when the context is created)
    try:
        e = Engine("cuda:0", max_batch=max(b for b, _ in SHAPES), max_frames=max(t for _, t in SHAPES), max_tokens=64)
    finally:
        os.environ.pop("JV_NO_CFG_SHARE", None)
        if was is not None:
            os.environ["JV_NO_CFG_SHARE"] = was
    e.load_state_dict(JV_MODEL_TTS, sd)
    e.load_noise(noise)
    e.set_step_graph(graph)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "solver_bench.json"))
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    from jyutvoice_amd import synth
    sd, noise = synth.tts_state_dict(), synth.rand_noise()
    plain, no_share, graph = make_engine(sd, noise), make_engine(sd, noise, no_share=True), make_engine(sd, noise, graph=True)
    arms = [("euler", plain, "euler", EVALS), ("euler_no_share", no_share, "euler", EVALS), ("euler_graph", graph, "euler", EVALS),
            ("midpoint", plain, "midpoint", EVALS // 2), ("heun", plain, "heun", EVALS // 2)]
    result = {"what": "jv_cfm_solve spending 10 estimator evaluations as Euler n = 10 / midpoint n = 5 / Heun n = 5: ms per solve and "
                      "per evaluation (device events), ratios per evaluation against `euler` (the parent commit's launches)",
              "rounds": a.rounds, "evaluations": EVALS, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for B, T in SHAPES:
        g = torch.Generator().manual_seed(B)
        mu = torch.randn(B, 80, T, generator=g).cuda()
        spks = (torch.randn(B, 80, generator=g) * 0.5).cuda()
        cond = torch.zeros_like(mu)

        def run(eng, solver, n):
            with eng.solver(solver):
                eng.cfm_solve(mu, None, spks, cond, n)

        for _ in range(3):
            for _, eng, solver, n in arms:
                run(eng, solver, n)
        torch.cuda.synchronize()
        ms = {name: [] for name, *_ in arms}
        for r in range(a.rounds):
            order = arms if r % 2 == 0 else arms[::-1]      # alternate the order: drift hits every arm alike
            for name, eng, solver, n in order:
                ms[name].append(timed(lambda: run(eng, solver, n)))
        med = {name: statistics.median(v) for name, v in ms.items()}
        shape = {}
        for name, *_ in arms:
            shape[name] = {"median_ms": round(med[name], 3), "min_ms": round(min(ms[name]), 3), "max_ms": round(max(ms[name]), 3),
                           "ms_per_evaluation": round(med[name] / EVALS, 4), "vs_euler": round(med[name] / med["euler"], 4),
                           "all_ms": [round(v, 3) for v in ms[name]]}
        shape["stage_kernel_overhead"] = {k: round(med[k] / med["euler_no_share"] - 1.0, 4) for k in ("midpoint", "heun")}
        shape["no_shared_twin_overhead"] = round(med["euler_no_share"] / med["euler"] - 1.0, 4)
        shape["graph_vs_eager"] = round(med["euler_graph"] / med["euler"] - 1.0, 4)
        result["shapes"][f"{B}x{T}"] = shape
        print(f"{B} x {T}: " + ", ".join(f"{name} {med[name]:.2f} ms ({med[name] / med['euler']:.3f} x)" for name, *_ in arms), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
