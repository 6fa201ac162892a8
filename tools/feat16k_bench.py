"""what do jv_fbank and jv_whisper_log_mel cost beside the resample that feeds them?  B recordings of 10 s at 44 100 Hz -> 16 kHz in one
ragged jv_resample call, then the two features on the resampled batch with the lengths it left on the device; each timed with device
events after warm-up (median of --iters calls) and once more under the in-library profiler (kernel time alone).  One JSON line per
batch size (1 and 32 unless --batch is given).

    python tools/feat16k_bench.py [--iters 20] [--orig 44100] [--batch 1 32] [--seconds 10]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from jyutvoice_amd import engine
from jyutvoice_amd.runtime import get_runtime
from jyutvoice_amd.utils.audio import whisper_filters

NEW = 16000


def timed(fn, iters):
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def kernels(fn):
    engine.profile_enable(True)
    try:
        fn()
        rep = engine.profile_report()
    finally:
        engine.profile_enable(False)
    return {n: v for n, v in sorted(rep.items()) if not n.startswith("_")}


def one(eng, dev, batch, seconds, orig, iters):
    n_in = int(seconds * orig)
    wav = (torch.randn(batch, n_in, generator=torch.Generator().manual_seed(0)) * 0.2).clamp(-1, 1).to(dev)
    lens = torch.full((batch,), n_in, dtype=torch.int32, device=dev)
    w16, l16 = eng.resample(wav, orig, NEW, lens)      # warm-up: builds and uploads the table
    for _ in range(3):
        eng.resample(wav, orig, NEW, lens)
        eng.fbank(w16, l16)
        eng.whisper_log_mel(w16, l16)
    res_ms = timed(lambda: eng.resample(wav, orig, NEW, lens), iters)
    fb_ms = timed(lambda: eng.fbank(w16, l16), iters)
    wh_ms = timed(lambda: eng.whisper_log_mel(w16, l16), iters)
    res_k, fb_k, wh_k = (kernels(f) for f in (lambda: eng.resample(wav, orig, NEW, lens), lambda: eng.fbank(w16, l16),
                                              lambda: eng.whisper_log_mel(w16, l16)))

    def tflops(rep, name):
        k = rep.get(name, {})
        return round(k.get("flops", 0.0) / max(k.get("ms", 0.0), 1e-9) / 1e9, 2)

    return {"what": f"{batch} recordings of {seconds:g} s, {orig} -> {NEW} Hz, then fbank and Whisper log-mel on {w16.shape[1]} samples each",
            "device": torch.cuda.get_device_name(0), "iters": iters,
            "resample_ms": round(res_ms, 4), "fbank_ms": round(fb_ms, 4), "whisper_ms": round(wh_ms, 4),
            "fbank_over_resample": round(fb_ms / res_ms, 3), "whisper_over_resample": round(wh_ms / res_ms, 3),
            "resample_kernels_ms": {n: v["ms"] for n, v in res_k.items()},
            "fbank_kernels_ms": {n: v["ms"] for n, v in fb_k.items()}, "whisper_kernels_ms": {n: v["ms"] for n, v in wh_k.items()},
            "fbank_tflops": tflops(fb_k, "feat16k_fbank"), "whisper_tflops": tflops(wh_k, "feat16k_whisper"),
            "frames": int(eng.lib.jv_fbank_frames(w16.shape[1])) * batch}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--orig", type=int, default=44100)
    p.add_argument("--batch", type=int, nargs="+", default=[1, 32])
    p.add_argument("--seconds", type=float, default=10.0)
    a = p.parse_args()
    dev = torch.device("cuda:0")
    eng = get_runtime(dev).ensure(1, 64, 1)
    eng.load_whisper_filters(whisper_filters())
    for batch in a.batch:
        print(json.dumps(one(eng, dev, batch, a.seconds, a.orig, a.iters)), flush=True)


if __name__ == "__main__":
    main()
