"""what does jv_resample cost beside the mel pass it feeds?  32 recordings of 10 s: 44 100 -> 24 000 Hz in one ragged call, then the
ragged prompt-mel pass (jv_mel_spectrogram_ragged) on the 32 resampled recordings (the target rate is the mel pass's 24 kHz, so
that it is the pass the resampler feeds), both timed with device events after warm-up
(median of --iters calls) and once more under the in-library profiler (kernel time alone, without the mel pass's host-side length
check).  Prints one JSON line.

    python tools/resample_bench.py [--iters 20] [--orig 44100] [--batch 32] [--seconds 10]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from jyutvoice_amd import engine
from jyutvoice_amd.runtime import get_runtime
from jyutvoice_amd.utils.audio import mel_basis

NEW = 24000      # the rate of the mel pass


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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--orig", type=int, default=44100)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--seconds", type=float, default=10.0)
    a = p.parse_args()
    dev = torch.device("cuda:0")
    eng = get_runtime(dev).ensure(1, 64, 1)
    eng.load_mel_basis(mel_basis())
    n_in = int(a.seconds * a.orig)
    wav = (torch.randn(a.batch, n_in, generator=torch.Generator().manual_seed(0)) * 0.2).clamp(-1, 1).to(dev)
    lens = torch.full((a.batch,), n_in, dtype=torch.int32, device=dev)
    mel_in, mel_lens = eng.resample(wav, a.orig, NEW, lens)      # warm-up: builds and uploads the table
    for _ in range(3):
        eng.resample(wav, a.orig, NEW, lens)
        eng.mel_spectrogram(mel_in, mel_lens)
    res_ms = timed(lambda: eng.resample(wav, a.orig, NEW, lens), a.iters)
    mel_ms = timed(lambda: eng.mel_spectrogram(mel_in, mel_lens), a.iters)
    engine.profile_enable(True)
    eng.resample(wav, a.orig, NEW, lens)
    res_rep = engine.profile_report()
    eng.mel_spectrogram(mel_in, mel_lens)
    mel_rep = engine.profile_report()
    engine.profile_enable(False)
    k = res_rep.get("resample", {})
    print(json.dumps({
        "what": f"{a.batch} recordings of {a.seconds:g} s, {a.orig} -> {NEW} Hz, beside the ragged mel pass on {mel_in.shape[1]} samples each",
        "device": torch.cuda.get_device_name(0), "iters": a.iters,
        "resample_ms": round(res_ms, 4), "mel_ragged_ms": round(mel_ms, 4), "resample_over_mel": round(res_ms / mel_ms, 4),
        "resample_kernel_ms": k.get("ms"), "resample_gflops": round(k.get("flops", 0.0) / max(k.get("ms", 0.0), 1e-9) / 1e6, 1),
        "resample_gbytes_per_s": round(k.get("bytes", 0.0) / max(k.get("ms", 0.0), 1e-9) / 1e6, 1),
        "mel_kernels_ms": round(sum(v["ms"] for n, v in mel_rep.items() if not n.startswith("_")), 4),
        "mel_kernels": {n: v["ms"] for n, v in sorted(mel_rep.items()) if not n.startswith("_")},
        "output_samples": int(mel_lens.sum())}))


if __name__ == "__main__":
    main()
