"""what do the level kernels cost beside the vocoder and the resampler?  32 recordings of 6 s at 24 kHz: `condition_prompt`'s
kernels (jv_trim_bounds, jv_peak, jv_level_gain, jv_level_apply with the 0.2 s tail), jv_loudness and jv_level_apply alone, beside
`hift.inference` of a mel batch of the same duration and jv_resample 24 -> 16 kHz of the same batch.  Device events; after the warm-up
(tables, intermediates, every geometry) the routes alternate round by round so that all see the same clocks; median and minimum
over the rounds.  Once more under the in-library profiler for jv_loudness's four kernels.  Writes profiles/level_bench.json (--out).

    python tools/level_bench.py [--rounds 15] [--batch 32] [--seconds 6] [--out profiles/level_bench.json]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch

import jyutvoice_amd
from jyutvoice_amd import engine, synth
from jyutvoice_amd.runtime import get_runtime

FS = 24000


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=15)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--seconds", type=float, default=6.0)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "level_bench.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("level_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    B, n = a.batch, int(a.seconds * FS)
    frames = n // 480
    hift = jyutvoice_amd.build_default("cuda:0")[1]
    hift.load_state_dict(synth.hift_state_dict())
    eng = get_runtime(dev).ensure(B, frames, 1)
    g = torch.Generator().manual_seed(0)
    wav = torch.randn(B, n, generator=g) * 0.1
    wav[:, : FS // 2] *= 1e-3      # half a second of room tone at either end
    wav[:, -FS // 2:] *= 1e-3
    wav = wav.to(dev)
    lens = torch.full((B,), n, dtype=torch.int32, device=dev)
    mel = torch.randn(B, 80, frames, generator=g).to(dev)
    gain = torch.full((B,), 0.5, device=dev)

    def condition():
        start, end = eng.trim_bounds(wav, lens, 60.0, 440, 220)
        return eng.level_apply(wav, lens, start, end, eng.level_gain(None, eng.peak(wav, lens, start, end), ceiling=0.8), FS // 5)

    routes = {
        "condition_prompt": condition,
        "loudness": lambda: eng.loudness(wav, FS, lens),
        "level_apply": lambda: eng.level_apply(wav, lens, gain=gain),
        "normalize": lambda: eng.level_apply(wav, lens, gain=eng.level_gain(eng.loudness(wav, FS, lens), eng.peak(wav, lens), -23.0, 0.95)),
        "resample_24k_16k": lambda: eng.resample(wav, FS, 16000, lens),
        "hift_inference": lambda: hift.inference(mel),
    }
    for _ in range(3):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(a.rounds):
        for k, fn in routes.items():
            ms[k].append(once(fn))
    engine.profile_enable(True)
    eng.loudness(wav, FS, lens)
    rep = engine.profile_report()
    engine.profile_enable(False)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    out = {
        "what": f"{B} recordings of {a.seconds:g} s at {FS} Hz: the level calls beside hift.inference of {frames} frames each and jv_resample "
                f"{FS} -> 16000 Hz of the same batch; device events, routes alternating per round after 3 warm-up rounds",
        "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
        "median_ms": {k: round(v, 4) for k, v in med.items()}, "min_ms": {k: round(min(v), 4) for k, v in ms.items()},
        "loudness_over_hift": round(med["loudness"] / med["hift_inference"], 5),
        "loudness_over_resample": round(med["loudness"] / med["resample_24k_16k"], 4),
        "condition_over_resample": round(med["condition_prompt"] / med["resample_24k_16k"], 4),
        "loudness_kernels_ms": {k: v["ms"] for k, v in sorted(rep.items()) if k.startswith("loud_")},
        "samples": B * n}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
