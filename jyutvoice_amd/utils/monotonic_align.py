"""`monotonic_align.maximum_path` of the reference (jyutvoice/utils/monotonic_align/__init__.py:7-22) on the GPU.

The reference copies the whole [b, t_x, t_y] score tensor to the host and runs a Cython loop there; this one hands the tensor to
jv_maximum_path where it lies.  Same name, argument order and return: the 0 / 1 path with `value`'s dtype and device, lengths
taken from the mask as the reference takes them (`mask.sum(1)[:, 0]`, `mask.sum(2)[:, 0]`).  The reference multiplies `value` by
the mask first; inside the lengths that changes nothing, and what lies behind them is not read here (it may be NaN).
One limit the reference does not have: t_x (the padded token dimension) may be at most 2048 -- a lane of the search's one
workgroup per utterance owns at most eight tokens; beyond that the call raises (JV_ERR_SHAPE).
A tensor that is not on a GPU is computed on the current one and returned where it came from: there is no CPU path.
"""
from __future__ import annotations

import torch

from ..runtime import get_runtime


def maximum_path(value, mask):
    """value: [b, t_x, t_y] scores; mask: [b, t_x, t_y] (1 inside each utterance) -> path [b, t_x, t_y]"""
    if value.dim() != 3 or tuple(mask.shape) != tuple(value.shape):
        raise ValueError(f"maximum_path: value and mask must both be [b, t_x, t_y], got {tuple(value.shape)} and {tuple(mask.shape)}")
    device, dtype = value.device, value.dtype
    dev = device if device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    B, Tx, Ty = value.shape
    m = mask.to(dev)
    x_lens = m.sum(1)[:, 0].to(torch.int32)
    y_lens = m.sum(2)[:, 0].to(torch.int32)
    eng = get_runtime(dev).ensure(1, Ty, Tx)      # the search's buffers grow on their own: only the two length capacities apply
    attn, _, _ = eng.maximum_path(value.detach().to(dev), x_lens, y_lens)
    return attn.to(device=device, dtype=dtype)
