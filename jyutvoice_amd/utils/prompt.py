"""Host-side helper of the voice-cloning batch (`JyutVoiceTTS.synthesise(..., prompt_lengths=...)`): prompts of different
lengths -> the padded tensors and the length vector the batched call takes.  Pure host code."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch


def pad_prompts(feats: Sequence[torch.Tensor], hs: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """feats[b]: prompt mel [p_b, 80] (`extract_speech_feat(...)[0][0]`), hs[b]: prompt encoder output [p_b, 80]
    (`flow_encoder(...)[0][0]`); p_b = 0 (an empty [0, 80] tensor) means "no prompt for this utterance".
    Returns (prompt_feat [B, P, 80], prompt_h [B, P, 80], prompt_lengths [B] int64) with P = max(p_b, 1) and zeros behind p_b.
    One length serves both tensors of an utterance: a pair whose lengths differ is a ValueError naming the index (trim both to
    the shorter first, as infer.py does)."""
    if len(feats) != len(hs):
        raise ValueError(f"pad_prompts: {len(feats)} prompt mels but {len(hs)} prompt encoder outputs")
    if len(feats) == 0:
        raise ValueError("pad_prompts: empty batch")
    lens: List[int] = []
    for b, (f, h) in enumerate(zip(feats, hs)):
        for name, t in (("feats", f), ("hs", h)):
            if t.dim() != 2 or t.shape[1] != 80:
                raise ValueError(f"pad_prompts: {name}[{b}] must be [frames, 80], got {tuple(t.shape)}")
        if f.shape[0] != h.shape[0]:
            raise ValueError(f"pad_prompts: utterance {b}: prompt mel has {f.shape[0]} frames but prompt_h has {h.shape[0]}; "
                             "trim both to the shorter")
        lens.append(int(f.shape[0]))
    P = max(max(lens), 1)
    dev = feats[0].device
    feat = torch.zeros(len(lens), P, 80, dtype=torch.float32, device=dev)
    ph = torch.zeros(len(lens), P, 80, dtype=torch.float32, device=dev)
    for b, (f, h) in enumerate(zip(feats, hs)):
        feat[b, : lens[b]] = f.to(dev, torch.float32)
        ph[b, : lens[b]] = h.to(dev, torch.float32)
    return feat, ph, torch.tensor(lens, dtype=torch.int64)
