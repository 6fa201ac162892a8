"""what does the estimator's FP16 mode (Engine.set_precision("fp16"): one MFMA product per fp16x3 contraction) buy?  Three workloads,
each in fp32 mode and in FP16 mode, alternating in one process:
  * c3: bench.py's C3 pass -- 32 utterances x 150 tokens -> 300 frames, n = 10: text encoder -> CFM solve -> HiFT vocoder
    (synthesise(batched=True) + inference());
  * b1: the same pass for one utterance of 64 tokens;
  * stream8: one row of tools/stream_batch_bench.py -- 8 streaming sessions through one Token2WavServer, 75 prompt tokens and 250 tokens
    each, pushed 25 at a time (its run total).
Every figure is a device-event interval; 2 warm-up rounds of both modes, then 7 rounds alternating fp32 / fp16 (both see the same
clocks); median and minimum.  One extra pass per mode and workload runs under the in-library profiler: the per-kernel table of both
modes, so that each kernel family's one-product time stands beside its three-product time (`families`: launches and ms summed over the
profiler names of a family; the FP16 mode's launches carry `,np1`).  Synthetic weights.  One JSON line, also written to
<output directory>/precision_bench.json (JV_OUT, default out/; committed under profiles/).

    python tools/precision_bench.py [--rounds 7] [--steps 10]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch

import jyutvoice_amd
from jyutvoice_amd import engine as jv_engine
from jyutvoice_amd import synth
from jyutvoice_amd.flow.flow import CausalMaskedDiffWithXvec
from jyutvoice_amd.runtime import Runtime, get_runtime
from jyutvoice_amd.stream import Token2WavServer
from stream_batch_bench import run_server

FAMILIES = ("rowblock_h3", "rowffn_h3", "rowgemm_h3", "rowres_h3", "rowconv_h3", "conv_gemm_h3", "conv_gemm_x6", "attn64_pl", "attn64_s",
            "attn64_h3", "attn64_x6")
MODES = ("fp32", "fp16")


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def families(report):
    out = {}
    for fam in FAMILIES:
        hit = {k: v for k, v in report.items() if k.startswith(fam + "<")}
        if hit:
            out[fam] = {"launches": sum(v["launches"] for v in hit.values()), "ms": round(sum(v["ms"] for v in hit.values()), 3)}
    return out


def measure(name, set_precision, run, rounds, result):
    for _ in range(2):
        for m in MODES:
            set_precision(m)
            run()
    torch.cuda.synchronize()
    times = {m: [] for m in MODES}
    for _ in range(rounds):
        for m in MODES:
            set_precision(m)
            times[m].append(timed(run))
    entry = {m: stats(times[m]) for m in MODES}
    entry["fp32_over_fp16"] = round(entry["fp32"]["median_ms"] / entry["fp16"]["median_ms"], 3)
    for m in MODES:      # one extra pass under the profiler (eager launches, every one bracketed by events: not a timing of the pass)
        set_precision(m)
        jv_engine.profile_enable(True)
        try:
            run()
            torch.cuda.synchronize()
            rep = jv_engine.profile_report()
        finally:
            jv_engine.profile_enable(False)
        entry["kernels_" + m] = {k: {"launches": v["launches"], "ms": round(v["ms"], 3)} for k, v in sorted(rep.items()) if not k.startswith("_")}
        entry["families_" + m] = families(rep)
    set_precision("fp32")
    result[name] = entry
    print(f"{name}: fp32 {entry['fp32']}  fp16 {entry['fp16']}  x{entry['fp32_over_fp16']}", flush=True)
    for fam in FAMILIES:
        a, b = entry["families_fp32"].get(fam), entry["families_fp16"].get(fam)
        if a or b:
            print(f"    {fam:14s} fp32 {a}  fp16 {b}", flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--steps", type=int, default=10)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("precision_bench.py measures on the GPU; none is visible")
    result = {}
    # ---- the full pass, bench.py's C3 and one short utterance
    tts, hift = jyutvoice_amd.build_default("cuda:0")
    tts.load_state_dict(synth.tts_state_dict(fixed_duration=1.5))
    hift.load_state_dict(synth.hift_state_dict())
    rt = get_runtime("cuda:0")
    rt.ensure(32, 300, 150)
    keys = ("x", "x_lengths", "lang", "tone", "word_pos", "syllable_pos", "spk_embed")
    for name, B, Tt in (("c3", 32, 150), ("b1", 1, 64)):
        batch = {k: v.cuda() for k, v in synth.batch(B, Tt).items()}

        def run(batch=batch):
            hift.manual_seed(0)
            res = tts.synthesise(*[batch[k] for k in keys], None, n_timesteps=a.steps, batched=True)
            hift.inference(res["mel"])

        measure(name, rt.set_precision, run, a.rounds, result)
        result[name].update(batch=B, tokens=Tt, n_timesteps=a.steps)
    # ---- eight streaming sessions in one batched step (the flow on a runtime of its own: the TTS holds the decoder's slots above)
    frt = Runtime("cuda:0")
    flow = CausalMaskedDiffWithXvec(vocab_size=6561, input_frame_rate=25, runtime=frt)
    sd = synth.prompt_state_dict()
    sd.update({k: v for k, v in synth.tts_state_dict().items() if k.startswith(("decoder.", "spk_embed_affine_layer."))})
    flow.load_state_dict(sd)
    N, prompt, tokens, hop = 8, 75, 250, 25
    reqs = []
    for k in range(N):
        tok, _ = synth.prompt_tokens(1, tokens, first_index=3 + 2 * k)
        ptok, _ = synth.prompt_tokens(1, prompt, first_index=4 + 2 * k)
        g = torch.Generator().manual_seed(k)
        reqs.append((tok, ptok, torch.randn(1, 2 * prompt, 80, generator=g), torch.randn(1, 192, generator=g)))
    server = Token2WavServer(flow, hift, N, tokens, n_timesteps=a.steps, max_prompt_tokens=prompt)
    measure("stream8", frt.set_precision, lambda: run_server(server, reqs, hop), a.rounds, result)
    result["stream8"].update(sessions=N, prompt_tokens=prompt, tokens=tokens, hop=hop, n_timesteps=a.steps)
    out = {"what": "fp32 mode beside FP16 mode (one MFMA product per fp16x3 contraction of the estimator): whole passes by device events, "
                   "alternating rounds after two warm-up rounds of both, median / min; per-kernel tables from one extra profiled pass per mode",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "workloads": result}
    print(json.dumps({k: {m: v[m] for m in MODES + ("fp32_over_fp16",)} for k, v in result.items()}), flush=True)
    d = os.environ.get("JV_OUT") or os.path.join(REPO, "out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "precision_bench.json"), "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
