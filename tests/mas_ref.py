"""Test infrastructure: the monotonic alignment search of the reference (jyutvoice/utils/monotonic_align/core.pyx:11-37) restated
in plain double loops, `value` updated in place in fp32.

Unpinned: the reference ships a prebuilt extension module for CPython 3.11; under the interpreter of this build it does not
load (`undefined symbol: Py_Version`), so there is no recorded fixture of the Cython's own paths and this restatement stands alone,
checked on hand-worked cases (tests/test_mas_host.py).

fp32 without numpy scalars: the scores live in `array('f')` rows.  Storing a Python float there rounds it to fp32 (nearest even),
reading gives that fp32 back exactly, and the double sum of two fp32 numbers rounded once more to fp32 is the fp32 sum (53 >= 2 * 24 + 2
bits: the double rounding is innocuous).  So `row[y] = max(a, b) + row[y]` is the Cython's float statement, bit for bit.
"""
from array import array

import numpy as np

MAX_NEG_VAL = -1e9      # exactly representable in fp32


def maximum_path_each(value, t_x, t_y, max_neg_val=MAX_NEG_VAL):
    """value: float32 [>= t_x, >= t_y], updated in place inside the band (what lies outside [:t_x, :t_y] is never read).
    Returns the path, int32 of value's shape.  Needs 1 <= t_x <= t_y (the Cython reads out of bounds otherwise)."""
    assert value.dtype == np.float32 and value.ndim == 2 and 1 <= t_x <= t_y <= value.shape[1] and t_x <= value.shape[0]
    rows = [array("f", value[x, :t_y].tolist()) for x in range(t_x)]
    for y in range(t_y):
        for x in range(max(0, t_x + y - t_y), min(t_x, y + 1)):
            if x == y:
                v_cur = max_neg_val
            else:
                v_cur = rows[x][y - 1]
            if x == 0:
                v_prev = 0.0 if y == 0 else max_neg_val
            else:
                v_prev = rows[x - 1][y - 1]
            rows[x][y] = (v_prev if v_prev > v_cur else v_cur) + rows[x][y]
    path = np.zeros(value.shape, dtype=np.int32)
    index = t_x - 1
    for y in range(t_y - 1, -1, -1):
        path[index, y] = 1
        if index != 0 and (index == y or rows[index][y - 1] < rows[index - 1][y - 1]):
            index -= 1
    for x in range(t_x):
        value[x, :t_y] = np.frombuffer(rows[x], dtype=np.float32)
    return path


def maximum_path(values, t_xs, t_ys):
    """values: float32 [B, Tx, Ty] (left unchanged); lengths per utterance -> (paths int32 [B, Tx, Ty], frame_index int32 [B, Ty]
    with -1 behind t_y, durations int32 [B, Tx])"""
    values = np.asarray(values)
    B, Tx, Ty = values.shape
    paths = np.zeros((B, Tx, Ty), dtype=np.int32)
    frame_index = np.full((B, Ty), -1, dtype=np.int32)
    for b in range(B):
        t_x, t_y = int(t_xs[b]), int(t_ys[b])
        paths[b] = maximum_path_each(values[b].astype(np.float32, copy=True), t_x, t_y)
        frame_index[b, :t_y] = paths[b, :, :t_y].argmax(axis=0)
    return paths, frame_index, paths.sum(axis=2).astype(np.int32)


def check_path(path, t_x, t_y):
    """every frame has exactly one token, every token at least one frame, the path starts at token 0, ends at t_x - 1 and never
    steps back or skips; nothing is set outside the utterance"""
    p = np.asarray(path)
    assert p[t_x:].sum() == 0 and p[:, t_y:].sum() == 0
    q = p[:t_x, :t_y]
    assert (q.sum(axis=0) == 1).all() and (q.sum(axis=1) >= 1).all()
    idx = q.argmax(axis=0)
    assert idx[0] == 0 and idx[-1] == t_x - 1
    step = np.diff(idx)
    assert ((step == 0) | (step == 1)).all()
