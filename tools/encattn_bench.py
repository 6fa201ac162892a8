"""what does the text encoder's one-launch attention (encattn.hip) cost beside the four-launch route?  Per attention call
(jv_op_enc_attention on a random qkv row buffer; fused = 0 includes that hook's allocation and synchronise, so its figure is an
upper bound of the four launches) and per whole jv_encoder_fwd (synthetic weights, Engine.set_encoder_attention), both routes at
Tt in {128, 256, 512} for B = 1 and B = 32; the fused route alone at Tt in {1024, 2048, 4096}, B = 1, with the fp32-MFMA flop
floor beside each figure: 2 heads x 2 products x 2 * 288 flops per (query, key) at 157.3 TFLOP/s (the f32-input MFMA peak).

Device events; every shape is warmed first, then the routes alternate round by round so that both see the same clocks; median and
minimum over the rounds.  Nothing in the library depends on these numbers.  Writes profiles/encattn_bench.json (--out).

    python tools/encattn_bench.py [--rounds 15] [--out profiles/encattn_bench.json]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch

from jyutvoice_amd import synth
from jyutvoice_amd.engine import JV_MODEL_TTS, Engine, op_enc_attention

G, GAP = 4, 4
PEAK_F32_MFMA = 157.3e12


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def floor_ms(B, T):
    return 1e3 * B * 2 * 2 * 2 * 288 * float(T) * T / PEAK_F32_MFMA


def measure(routes, rounds):
    for _ in range(2):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            ms[k].append(once(fn))
    return {k: {"median_ms": round(sorted(v)[len(v) // 2], 4), "min_ms": round(min(v), 4)} for k, v in ms.items()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=15)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "encattn_bench.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("encattn_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    sd = synth.tts_state_dict()
    g = torch.Generator().manual_seed(0)
    results = []
    shapes = [(B, T, True) for T in (128, 256, 512) for B in (1, 32)] + [(1, T, False) for T in (1024, 2048, 4096)]
    eng, cap = None, (0, 0)
    for B, T, both in shapes:
        if eng is None or B > cap[0] or T > cap[1]:      # one context per capacity class: 32 x 512, then 1 x 4096
            if eng is not None:
                eng.close()
            cap = (32, 512) if both else (1, 4096)
            eng = Engine(dev, max_batch=cap[0], max_frames=64, max_tokens=cap[1])
            eng.load_state_dict(JV_MODEL_TTS, sd)
        S = T + GAP
        qkv = torch.randn(G + B * S, 1728, generator=g).to(dev)
        lens = torch.full((B,), T, dtype=torch.int64, device=dev)
        u = {k: v.to(dev) for k, v in synth.batch(B, T).items() if torch.is_tensor(v)}

        def enc(mode):
            eng.set_encoder_attention(mode)
            eng.encoder(u["x"], u["x_lengths"], u["lang"], u["tone"], u["word_pos"], u["syllable_pos"], u["spk_embed"])

        routes = {"attention_fused": lambda: op_enc_attention(qkv, lens, B, T, G, S, fused=True),
                  "encoder_fused": lambda: enc("fused")}
        if both:
            routes["attention_four_launch_hook"] = lambda: op_enc_attention(qkv, lens, B, T, G, S, fused=False)
            routes["encoder_four_launch"] = lambda: enc("gemm")
        r = measure(routes, a.rounds)
        eng.set_encoder_attention("auto")
        row = {"B": B, "Tt": T, "attention_flop_floor_ms": round(floor_ms(B, T), 5), **r}
        row["attention_fused_share_of_floor"] = round(floor_ms(B, T) / r["attention_fused"]["median_ms"], 4)
        results.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    out = {"what": "text encoder attention: encattn.hip (one launch) beside the four-launch route; per jv_op_enc_attention call (the "
                   "fused = 0 hook allocates and synchronises inside the call: an upper bound of the four launches) and per "
                   "jv_encoder_fwd (6 layers, synthetic weights); device events, routes alternating per round after 2 warm-up rounds; "
                   "floor = attention flops at the 157.3 TFLOP/s f32-input MFMA peak",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
