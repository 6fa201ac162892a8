#!/usr/bin/env python3
"""Generate the mixed-context encoder fixture of the batched streaming tests from the REFERENCE's own modules, utterance by
utterance at B = 1.  Build container only.

    python tests/golden/make_golden_stream_batch.py      # needs the reference tree; writes G16_flow_ctx_batch.npz

The batch is the fourth step of the timeline in tests/stream_batch_cases.py, streaming=True: session a finishes (53 tokens, the
whole sequence: the imported encoder's own forward(), flow.py:319-328), sessions b and c are in mid-stream (10 + 68 and 7 + 21 tokens
of which the last three are look-ahead context only: `make_golden_stream.partial_encoder`, the composition G15 uses).

G16  ids_a [1,53], ids_b [1,78], ids_c [1,28] (prompt tokens | tokens, as the sessions hold them); h_a [1,106,80], h_b [1,150,80],
     h_c [1,50,80].
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg                  # noqa: E402
import make_golden_flow as mgf            # noqa: E402
import make_golden_stream as mgs          # noqa: E402
import stream_batch_cases as sb           # noqa: E402


@torch.inference_mode()
def main():
    torch.manual_seed(20240616)
    flow, _ = mgf.build_flow()
    rows = {name: (solve, ctx) for name, solve, ctx, _, _ in sb.ROWS[3]}
    assert rows == {"a": (53, 0), "b": (78, 3), "c": (28, 3)}
    out = {}
    for name, (solve, ctx) in rows.items():
        tok, ptok, _, _ = sb.inputs(name)
        ids = torch.cat([ptok, tok], dim=1)[:, :solve]
        if ctx:
            h = mgs.partial_encoder(flow, ids, True)
        else:
            h, _ = flow.encoder(flow.input_embedding(torch.clamp(ids, min=0)), torch.tensor([solve]), streaming=True)
            h = flow.encoder_proj(h)
        assert h.shape == (1, 2 * (solve - ctx), 80), h.shape
        out["ids_" + name], out["h_" + name] = ids, h
        print(f"G16 {name}: {solve} tokens, ctx {ctx}: h {tuple(h.shape)} max abs {float(h.abs().max()):.3f}")
    mg.save("G16_flow_ctx_batch", **out)


if __name__ == "__main__":
    main()
