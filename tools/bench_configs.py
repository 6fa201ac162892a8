#!/usr/bin/env python3
"""bench.py lines of the other configurations on ONE box (through gpurun, repo root):
    python tools/bench_configs.py [tag]      -> gpurun_out/bench_configs_<tag>.json   (committed as profiles/rNN_bench_configs.json)
Every run is --full --no-cpu-baseline --no-exact-range --no-profile (for `stage_ms`); a failed run is recorded with its stderr tail.

The voice-cloning workload is not a bench.py configuration (bench.py has no prompts) and is timed here:
    python tools/bench_configs.py cloning batch|singles OUT.json   (committed as profiles/cloning_batch_bench.json)
32 requests of 150 text tokens, each with its own prompt of 3 - 10 s (seeded), n = 10: `batch` = ONE
synthesise(batched=True, prompt_lengths=...) call, `singles` = 32 prompted B = 1 calls (the only way to serve them before
prompt_lengths existed; that mode uses nothing newer, so the same file times an older checkout)."""
import json
import subprocess
import sys
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [
    ("c3", "", "the headline (32 utterances x 150 tokens, n = 10), no instrumentation"),
    ("b1", "--batch 1 --tokens 64", "C1's shape on the GPU: one utterance of 64 tokens"),
    ("c2", "--workload c2 --batch 8 --tokens 256", "BASELINE.json configs[1]: the CFM loop alone, 8 x 512 frames"),
    ("c4", "--timesteps 32", "C3 with n = 32"),
    ("b4", "--batch 4", ""), ("b8", "--batch 8", ""), ("b16", "--batch 16", ""), ("b22", "--batch 22", "as many frames as the ragged batch below holds"),
    ("b64", "--batch 64", "two rounds of the row-owning tiles"),
    ("ragged", "--ragged", "32 utterances of 60 .. 150 tokens (seeded), compact geometry; `value` counts valid frames"),
    ("ragged_uniform", "--ragged", "the same padded to the longest (JV_NO_COMPACT=1)"),
]


def cloning(mode, dst, n_req=32, tokens=150, n_timesteps=10, passes=3):
    """valid generated mel frames per second of synthesise() (encoder + duration predictor + CFM solve; prompt_h and the prompt
    mel are inputs prepared before the clock starts), device events around each pass, one warm-up pass first, median pass"""
    sys.path.insert(0, ROOT)
    import torch
    import jyutvoice_amd
    from jyutvoice_amd import synth
    from jyutvoice_amd.flow.encoder import FlowEncoder
    keys = ("x", "x_lengths", "lang", "tone", "word_pos", "syllable_pos", "spk_embed")
    g = torch.Generator().manual_seed(2024)
    ptok = torch.randint(75, 251, (n_req,), generator=g).tolist()      # 3 - 10 s of prompt: 25 tokens = 50 frames per second
    p = [2 * n for n in ptok]
    tts, _ = jyutvoice_amd.build_default("cuda:0")
    tts.load_state_dict(synth.tts_state_dict(fixed_duration=1.5))      # two frames per text token, as bench.py
    fenc = FlowEncoder(device="cuda:0")
    fenc.load_state_dict(synth.prompt_state_dict())
    tok, lens = synth.prompt_tokens(n_req, max(ptok), lengths=ptok)
    prompt_h, _ = fenc(tok, lens)                                       # [B, max p, 80], zero behind p_b
    prompt_feat = torch.randn(n_req, max(p), 80, generator=g).to("cuda:0")
    b = synth.batch(n_req, tokens)
    args = [b[k] for k in keys]

    def one_pass():
        if mode == "batch":
            r = tts.synthesise(*args, prompt_feat, prompt_h=prompt_h, n_timesteps=n_timesteps, batched=True,
                               prompt_lengths=torch.tensor(p))
            return int(r["mel_lengths"].sum()), bool(torch.isfinite(r["mel"]).all())
        frames, ok = 0, True
        for i in range(n_req):
            r = tts.synthesise(*[a[i:i + 1] for a in args], prompt_feat[i:i + 1, :p[i]], prompt_h=prompt_h[i:i + 1, :p[i]],
                               n_timesteps=n_timesteps)
            frames += int(r["mel_lengths"].sum())
            ok = ok and bool(torch.isfinite(r["mel"]).all())
        return frames, ok

    one_pass()
    ms = []
    for _ in range(passes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        frames, ok = one_pass()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = sorted(ms)[len(ms) // 2]
    out = {"workload": f"{n_req} cloning requests, {tokens} text tokens each, prompts of 3 - 10 s (seed 2024), n = {n_timesteps}",
           "mode": mode, "prompt_frames": p, "prompt_frames_sum": sum(p), "valid_generated_frames": frames, "finite": ok,
           "pass_ms": [round(m, 2) for m in ms], "median_ms": round(med, 2), "valid_generated_frames_per_s": round(frames / med * 1e3, 1)}
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "prompt_frames"}))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "cloning":
        if sys.argv[2] not in ("batch", "singles") or len(sys.argv) < 4:
            raise SystemExit("usage: bench_configs.py cloning batch|singles OUT.json")
        return cloning(sys.argv[2], sys.argv[3])
    tag = sys.argv[1] if len(sys.argv) > 1 else "r"
    out = {}
    for key, flags, what in CONFIGS:
        env = dict(os.environ)
        if key == "ragged_uniform":
            env["JV_NO_COMPACT"] = "1"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--no-cpu-baseline", "--no-exact-range", "--no-profile"] + flags.split()
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not lines:
            out[key] = {"flags": flags, "error": (r.stderr or "")[-400:]}
            print(key, "FAILED", flush=True)
            continue
        j = json.loads(lines[-1])
        out[key] = {"flags": flags + (" (JV_NO_COMPACT=1)" if key == "ragged_uniform" else ""), "what": what, "ms_per_step": j["ms_per_step"],
                    "mel_frames_per_s": j["value"], "x_realtime": j["x_realtime"], "stage_ms": {k: v for k, v in (j.get("stage_ms") or {}).items() if k != "measured"},
                    "roofline_path_frac": (j.get("roofline_path") or {}).get("frac")}
        if "ragged" in j.get("config", {}):
            out[key]["ragged"] = j["config"]["ragged"]
        print(key, j["ms_per_step"], j["value"], flush=True)
    dst = os.path.join(ROOT, "gpurun_out", f"bench_configs_{tag}.json")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as fh:
        json.dump({"note": "bench.py lines of one build on one box, back to back; --full --no-cpu-baseline --no-exact-range --no-profile", "configs": out}, fh, indent=1)


if __name__ == "__main__":
    main()
