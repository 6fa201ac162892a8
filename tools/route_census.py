"""Census of the estimator's routes: which kernels a solve launches, how often, and the SHA-256 of the mel it returns --
for every regime of the batch size and every control switch the library keeps.

    python tools/route_census.py --out profiles/route_census.json
    JYUTVOICE_HIP_LIB=jyutvoice_amd/libjyutvoice_hip.<tag>.so python tools/route_census.py --out other.json --compare profiles/route_census.json

Two builds of the library compute the same thing on the same routes iff their two files are identical (`--compare` exits 1
on the first difference): the check a change to the host-side launch path (estimator.hip est_route) has to pass against the
build before it.  The switches are read when a context is created, so every SETTING runs in a fresh child process -- one at
a time, each under its own time limit, and nothing more is started after a child that failed -- and every CASE inside it on
a context of its own.  Launch counts come from the in-library profiler (engine.profile_report()), the hash from a run
without it (the profiler forces the eager path; JV_STEP_GRAPH replays a captured step only without it)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SWITCHES = ["JV_NO_ROWGEMM", "JV_DMA_A", "JV_NO_FFN_FUSE", "JV_NO_BLOCK_FUSE", "JV_NO_QKV_SPLIT", "JV_NO_LN_FOLD", "JV_NO_RES_FOLD",
            "JV_NO_RES_PAIR", "JV_NO_RES_QKV", "JV_NO_TEMB_PRE", "JV_NO_CFG_SHARE", "JV_NO_COMPACT", "JV_FF_STAGGER", "JV_EXACT_RANGE", "JV_STEP_GRAPH",
            "JV_NO_HIFTCONV", "JV_NO_HIFT_PAIR"]
SETTINGS = {"default": {}}
SETTINGS.update({s: {s: "1"} for s in SWITCHES})
SETTINGS["set_exact_range"] = {}      # jv_flow_set_contraction(1) on a context created in the default mode
SETTINGS["set_precision_fp16"] = {}   # jv_flow_set_precision(JV_PRECISION_FP16) on a context created in the default mode
SETTINGS["JV_EST_FP16"] = {"JV_EST_FP16": "1"}
SETTINGS["JV_ROWGEMM_RT=2"] = {"JV_DYNAMIC_ENV": "1", "JV_ROWGEMM_RT": "2"}
SETTINGS["JV_ROWGEMM_RT=5"] = {"JV_DYNAMIC_ENV": "1", "JV_ROWGEMM_RT": "5"}

KEYS = ("x", "x_lengths", "lang", "tone", "word_pos", "syllable_pos", "spk_embed")


def batch_cases():
    from jyutvoice_amd import synth
    return {
        "1x64 (split-K)": synth.batch(1, 64, first_index=9),
        "2x33": synth.batch(2, 33, first_index=5),
        "ragged 4 (q|k|v split x6)": synth.batch(4, 150, first_index=3, lengths=[150, 97, 141, 150]),
        "ragged 8 (q|k|v split x3)": synth.batch(8, 150, first_index=40, lengths=[150 - 11 * i for i in range(8)]),
        "ragged 20x131 (tile height 4, compact)": synth.batch(20, 131, first_index=7, lengths=[131 - 3 * i for i in range(20)]),
        "32x150 (full chip)": synth.batch(32, 150),
        "40x150 (attn64_pl)": synth.batch(40, 150),
    }


def child(setting, out_path):
    import torch
    import jyutvoice_amd
    from jyutvoice_amd import engine, synth
    from jyutvoice_amd.runtime import get_runtime
    sd = synth.tts_state_dict(fixed_duration=1.5)
    result = {}

    def fresh(batch, frames, tokens):
        tts, _ = jyutvoice_amd.build_default("cuda:0")
        tts.load_state_dict(sd)      # (re-loading a finalized model: a new context)
        eng = get_runtime("cuda:0").ensure(batch, frames, tokens)
        if setting == "set_exact_range":
            eng.set_exact_range(True)
        if setting == "set_precision_fp16":
            eng.set_precision("fp16")
        return tts, eng

    def census(name, run):
        mel = run().float().cpu().contiguous()
        engine.profile_enable(True)
        try:
            run()
            rep = engine.profile_report()
        finally:
            engine.profile_enable(False)
        result[name] = {"launches": {k: v["launches"] for k, v in sorted(rep.items())},
                        "mel_sha256": hashlib.sha256(mel.numpy().tobytes()).hexdigest(), "finite": bool(torch.isfinite(mel).all())}
        print(f"[route_census] {setting} | {name}: {sum(v['launches'] for v in rep.values())} launches", flush=True)

    for name, b in batch_cases().items():
        tts, _ = fresh(b["x"].shape[0], 2 * b["x"].shape[1], b["x"].shape[1])
        census(name, lambda: tts.synthesise(*[b[k] for k in KEYS], None, n_timesteps=2, batched=True)["mel"])

    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g).cuda()
    # one estimator call with the caller's own t (the seam's entry point: the time embedding inside the call)
    _, eng = fresh(8, 256, 128)
    x, mu, cond, spk, t = rnd(8, 80, 120), rnd(8, 80, 120), rnd(8, 80, 120), rnd(8, 80), torch.rand(8, generator=g).cuda()
    lens = torch.tensor([120, 120, 99, 64, 120, 120, 99, 64], dtype=torch.int32)
    census("estimator call 8x120", lambda: eng.flow_estimator(x, lens, mu, t, spk, cond))
    # a prompted (voice cloning) solve of four utterances
    _, eng = fresh(8, 256, 128)
    mu_y, ph, pf, spk4 = rnd(4, 80, 120), rnd(4, 60, 80), rnd(4, 60, 80), rnd(4, 80)
    yl, pl = torch.tensor([120, 100, 80, 111], dtype=torch.int32), torch.tensor([60, 40, 50, 33], dtype=torch.int32)
    census("prompted solve 4x(60+120)", lambda: eng.cfm_solve_prompted(mu_y, yl, ph, pf, pl, spk4, 2))
    # a streaming (chunk-causal) solve
    _, eng = fresh(8, 256, 128)
    eng.set_streaming(50)
    mu4, cond4, l4 = rnd(4, 80, 200), rnd(4, 80, 200), torch.tensor([200, 200, 170, 120], dtype=torch.int32)
    census("streaming solve 4x200, chunk 50", lambda: eng.cfm_solve(mu4, l4, spk4, cond4, 2))
    eng.set_streaming(0)
    with open(out_path, "w") as fh:
        json.dump(result, fh)


def first_difference(a, b, path=""):
    if isinstance(a, dict) and isinstance(b, dict):
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                return f"{path}/{k}: only in one file"
            d = first_difference(a[k], b[k], f"{path}/{k}")
            if d:
                return d
        return None
    return None if a == b else f"{path}: {a!r} != {b!r}"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.environ.get("JV_OUT", os.path.join(REPO, "out")), "route_census.json"))
    ap.add_argument("--settings", nargs="*", default=list(SETTINGS), help="subset of: " + ", ".join(SETTINGS))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--compare", help="a census file of another build: exit 1 unless identical")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.out)
    census = {}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for s in args.settings:
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES and k not in ("JV_ROWGEMM_RT", "JV_DYNAMIC_ENV")}
        env.update(SETTINGS[s])
        with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", s, "--out", tmp.name], env=env, timeout=args.timeout)
            if r.returncode != 0:
                print(f"[route_census] setting {s}: child exited with {r.returncode}; stopping", file=sys.stderr)
                return 1
            census[s] = json.load(open(tmp.name))
        with open(args.out, "w") as fh:      # (rewritten after every setting: a later failure keeps what was measured)
            json.dump(census, fh, indent=1, sort_keys=True)
    if args.compare:
        other = json.load(open(args.compare))
        d = first_difference({k: other.get(k) for k in census}, census)
        print(f"[route_census] {'identical to' if not d else 'DIFFERS from'} {args.compare}" + (f": {d}" if d else ""))
        return 1 if d else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
