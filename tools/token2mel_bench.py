"""what does token-to-mel cost, and what does the fused relative-position attention buy?  The flow encoder (jv_flow_encoder_fwd,
relattn.hip: one attention launch per block, no [T, T] buffer) beside the same encoder on the three-GEMM attention
(jv_prompt_encoder_fwd on the same tokens: identical stages, the route with ac / bd / vt), and the whole token-to-mel pass
(CausalMaskedDiffWithXvec.inference: encoder + 10 Euler steps), at B = 32 x 150 tokens (the bench shape's 300 frames) and at
B = 1 x 750 tokens (30 s).  Synthetic weights.  The two encoders are timed in interleaved rounds in ONE process after warm-up,
device events around each call, median and minimum per arm; the ratio is fused / three-GEMM of the medians.  One JSON line.

    python tools/token2mel_bench.py [--rounds 15] [--shapes 32x150 1x750] [--steps 10]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from jyutvoice_amd import synth
from jyutvoice_amd.flow.flow import CausalMaskedDiffWithXvec
from jyutvoice_amd.runtime import Runtime


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4)}


def one(flow, rt, batch, tokens, rounds, steps):
    tok, lens = synth.prompt_tokens(batch, tokens)
    eng = rt.ensure(batch, 2 * tokens, 1)
    dev = eng.device
    tok_d, lens_d = tok.to(dev), lens.to(dev)
    g = torch.Generator().manual_seed(0)
    emb = torch.randn(batch, 192, generator=g).to(dev)
    feat = torch.randn(batch, 60, 80, generator=g).to(dev)
    flen = torch.full((batch,), 60, dtype=torch.int32)
    arms = {
        "encoder_fused": lambda: eng.flow_encoder(None, None, tok_d, lens_d, streaming=False),
        "encoder_three_gemm": lambda: eng.prompt_encoder(tok_d, lens_d),
    }
    whole = lambda: flow.inference(tok_d, lens, None, None, feat, flen, emb, False, True, batched=True, n_timesteps=steps)
    for fn in list(arms.values()) + [whole]:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(rounds):                      # interleaved: both arms see the same clocks and cache state
        for k, fn in arms.items():
            ms[k].append(once(fn))
    res = {"batch": batch, "tokens": tokens, "frames": 2 * tokens}
    for k in arms:
        res[k] = stats(ms[k])
    res["fused_over_three_gemm"] = round(res["encoder_fused"]["median_ms"] / res["encoder_three_gemm"]["median_ms"], 4)
    res["streaming_encoder"] = stats([once(lambda: eng.flow_encoder(None, None, tok_d, lens_d, streaming=True)) for _ in range(rounds)])
    res["token2mel"] = stats([once(whole) for _ in range(max(3, rounds // 3))])
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=15)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--shapes", nargs="+", default=["32x150", "1x750"], help="BxTOKENS")
    a = p.parse_args()
    rt = Runtime("cuda:0")
    flow = CausalMaskedDiffWithXvec(vocab_size=6561, input_frame_rate=25, runtime=rt)
    sd = synth.prompt_state_dict()
    sd.update({k: v for k, v in synth.tts_state_dict().items() if k.startswith(("decoder.", "spk_embed_affine_layer."))})
    flow.load_state_dict(sd)
    out = {"what": "flow encoder on the fused rel-pos attention vs the same encoder on the three-GEMM attention (interleaved rounds, "
                   "device events, median / min), the streaming encoder, and the whole token-to-mel pass",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "n_timesteps": a.steps, "shapes": []}
    for s in a.shapes:
        b, t = (int(v) for v in s.split("x"))
        out["shapes"].append(one(flow, rt, b, t, a.rounds, a.steps))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
