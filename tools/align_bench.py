"""what does the evaluation forward() cost, and where?  B utterances of about --tokens tokens and --frames frames (ragged: lengths between
80 % and 100 % of those), synthetic weights.  Each piece timed with device events after warm-up (median of --iters calls) -- the log
prior, the alignment search, prior + search fused (jv_align), the loss kernels, the ONE estimator evaluation forward() contains, and
the whole forward() -- and once more under the in-library profiler (kernel time alone).  One JSON line per batch size.

    python tools/align_bench.py [--iters 20] [--batch 32] [--tokens 150] [--frames 300]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import jyutvoice_amd
from jyutvoice_amd import engine, synth
from jyutvoice_amd.runtime import get_runtime


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
    return {n: round(v["ms"], 4) for n, v in sorted(rep.items()) if not n.startswith("_")}


def one(tts, dev, batch, tokens, frames, iters):
    g = torch.Generator().manual_seed(0)
    x_lens = torch.randint(int(0.8 * tokens), tokens + 1, (batch,), generator=g)
    y_lens = torch.randint(int(0.8 * frames), frames + 1, (batch,), generator=g)
    x_lens[0], y_lens[0] = tokens, frames
    b = synth.batch(batch, tokens, lengths=x_lens.tolist())
    y = torch.randn(batch, 80, frames, generator=g).to(dev)
    decoder_h = torch.randn(batch, frames, 80, generator=g).to(dev)
    args = [b["x"], x_lens, y, y_lens, b["lang"], b["tone"], b["word_pos"], b["syllable_pos"], b["spk_embed"], decoder_h]
    args = [a.to(dev) if i not in (1, 3) else a for i, a in enumerate(args)]
    kw = dict(t=torch.rand(batch, generator=g).to(dev), z=torch.randn(batch, 80, frames, generator=g).to(dev),
              cfg_mask=torch.ones(batch, device=dev), cond_index=[0] * batch)
    eng = get_runtime(dev).ensure(batch, frames, tokens)
    xl, yl = x_lens.to(dev, torch.int32), y_lens.to(dev, torch.int32)
    _, _, _, _, parts = tts(*args, **kw, return_parts=True)
    mu_x, logw, fi, dur, lp = parts["mu_x"], parts["logw"], parts["frame_index"], parts["durations"], parts["log_prior"]
    pieces = {
        "log_prior_ms": lambda: eng.log_prior(mu_x, decoder_h, xl, yl),
        "search_ms": lambda: eng.maximum_path(lp, xl, yl),
        "align_ms": lambda: eng.align(mu_x, decoder_h, xl, yl),
        "losses_ms": lambda: (eng.align_losses(logw, dur, xl, mu_x, decoder_h, fi, yl),
                              eng.cfm_loss_inputs(y, kw["z"], parts["t"], kw["cfg_mask"], torch.zeros(batch, dtype=torch.int32), parts["mu_y"],
                                                  parts["spks_masked"]),
                              eng.masked_mse(parts["pred"], parts["u"], yl)),
        "estimator_ms": lambda: eng.flow_estimator(parts["y_t"], yl, parts["mu_masked"], parts["t"], parts["spks_masked"], parts["cond"]),
        "forward_ms": lambda: tts(*args, **kw),
    }
    res = {"what": f"forward() on {batch} utterances of {int(0.8 * tokens)}..{tokens} tokens and {int(0.8 * frames)}..{frames} frames; "
                   "the entries with a length check (log_prior, search, align, forward) include their host synchronisation",
           "device": torch.cuda.get_device_name(0), "iters": iters, "tokens": int(x_lens.sum()), "frames": int(y_lens.sum())}
    for name, fn in pieces.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        res[name] = round(timed(fn, iters), 4)
    res["search_over_estimator"] = round(res["search_ms"] / res["estimator_ms"], 3)
    res["kernels_ms"] = {n: v for n, v in kernels(pieces["forward_ms"]).items() if n.startswith("align_")}
    res["search_kernel_us_per_frame"] = round(1e3 * res["kernels_ms"].get("align_search", 0.0) / frames, 3)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--batch", type=int, nargs="+", default=[32])
    p.add_argument("--tokens", type=int, default=150)
    p.add_argument("--frames", type=int, default=300)
    a = p.parse_args()
    dev = torch.device("cuda:0")
    tts, _ = jyutvoice_amd.build_default(dev)
    tts.load_state_dict(synth.tts_state_dict())
    for batch in a.batch:
        print(json.dumps(one(tts, dev, batch, a.tokens, a.frames, a.iters)), flush=True)


if __name__ == "__main__":
    main()
