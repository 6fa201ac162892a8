"""Operator parity of the fused relative-position attention (relattn.hip, jv_op_rel_attention fused = 1) and of the three-GEMM
route it replaces (fused = 0) against the fp64 restatement tests/relattn_ref.py.

Tolerance (the issue's rule, measured not guessed): at every case the fused route's max-abs error against fp64 may be at most twice
the three-GEMM route's error on the same inputs in the same run, or 1e-6 where that is larger -- the existing route is the
yardstick, the factor 2 covers the different summation order of an online softmax.  Each case prints its pair."""
import pytest
import torch

import relattn_ref as ref

pytestmark = pytest.mark.gpu

G, GAP = 8, 8      # the prompt encoder's row geometry (prompt.hip P_G, P_GAP)


def make_inputs(B, T, seed):
    """operands of the magnitudes a LayerNorm'd activation gives through the encoder's linears: q, k, v and p of order one, the
    two position biases of order 0.1 (xavier-uniform [8, 64]); rows of no utterance are NaN (they must not be read)"""
    g = torch.Generator().manual_seed(seed)
    S = T + GAP
    rows = G + B * S
    qkv = torch.full((rows, 1536), float("nan"))
    for b in range(B):
        qkv[G + b * S:G + b * S + T] = torch.randn(T, 1536, generator=g)
    p = torch.randn(2 * T - 1, 512, generator=g) * 0.7
    u = (torch.rand(8, 64, generator=g) - 0.5) * 0.4
    v = (torch.rand(8, 64, generator=g) - 0.5) * 0.4
    return qkv, p, u, v, S


def run_pair(qkv, p, u, v, lens, B, T, S, len_mul, chunk):
    from jyutvoice_amd.engine import op_rel_attention
    want = ref.rel_attention(qkv, p, u, v, lens, B, T, G, S, len_mul, chunk)
    dev = [t.cuda() for t in (qkv, p, u, v)]
    lens_d = torch.tensor(lens, dtype=torch.int64)
    got = {f: op_rel_attention(*dev, lens_d, B, T, G, S, len_mul, chunk, fused=bool(f)).cpu().double() for f in (1, 0)}
    own = ~torch.isnan(want[:, 0])
    err = {}
    for f in (1, 0):
        assert torch.isnan(got[f][~own]).all(), "a row of no utterance was written"
        assert torch.isfinite(got[f][own]).all()
        err[f] = float((got[f][own] - want[own]).abs().max())
    return got, want, err


@pytest.mark.parametrize("chunk", [0, 25, 50])
@pytest.mark.parametrize("T", [1, 25, 26, 64, 65, 186, 257, 600])
def test_fused_against_fp64_and_three_gemm(T, chunk):
    qkv, p, u, v, S = make_inputs(1, T, 1000 + T)
    _, _, err = run_pair(qkv, p, u, v, [T], 1, T, S, 1, chunk)
    print(f"rel_attention T={T} chunk={chunk}: fused {err[1]:.3e}  three-GEMM {err[0]:.3e}")
    assert err[1] <= max(2 * err[0], 1e-6)
    assert err[0] <= 1e-5      # the yardstick itself is an fp32-accurate route (outputs of order one)


@pytest.mark.parametrize("chunk", [0, 25, 50])
def test_ragged_batch_zero_rows(chunk):
    """three utterances: length 0, the full T, and one in between (through len_mul = 2, as the encoder's second stage calls it);
    rows at and behind a length are exactly zero on both routes, and NaN behind the lengths changes nothing on the fused one"""
    T = 130      # two 128-query workgroups per (utterance, head), the second one nearly empty
    lens = [0, 65, 41]
    qkv, p, u, v, S = make_inputs(3, T, 77)
    got, want, err = run_pair(qkv, p, u, v, lens, 3, T, S, 2, chunk)
    print(f"rel_attention ragged chunk={chunk}: fused {err[1]:.3e}  three-GEMM {err[0]:.3e}")
    assert err[1] <= max(2 * err[0], 1e-6)
    for b, n in enumerate(lens):
        L = min(2 * n, T)
        r0 = G + b * S
        for f in (1, 0):
            assert float(got[f][r0 + L:r0 + T].abs().max()) == 0.0 if L < T else True, (b, f)
    from jyutvoice_amd.engine import op_rel_attention
    hostile = qkv.clone()
    for b, n in enumerate(lens):
        hostile[G + b * S + min(2 * n, T):G + b * S + T] = float("nan")
    again = op_rel_attention(hostile.cuda(), p.cuda(), u.cuda(), v.cuda(), torch.tensor(lens), 3, T, G, S, 2, chunk, fused=True)
    assert torch.equal(again.cpu().double().nan_to_num(nan=-7.0), got[1].nan_to_num(nan=-7.0))


@pytest.mark.parametrize("chunk", [0, 50])
def test_ragged_batch_long_rows(chunk):
    """T = 300 at len_mul = 1: three workgroups per (utterance, head), ten key tiles.  The full utterance ends 44 queries into
    the workgroup at I0 = 256; the one of 129 rows has one query in its second workgroup and nothing but padding in its third;
    the one of a single row has one query and one key.  Same assertions as test_ragged_batch_zero_rows"""
    from jyutvoice_amd.engine import op_rel_attention
    T = 300
    lens = [300, 129, 1]
    qkv, p, u, v, S = make_inputs(3, T, 78)
    got, want, err = run_pair(qkv, p, u, v, lens, 3, T, S, 1, chunk)
    print(f"rel_attention ragged T=300 chunk={chunk}: fused {err[1]:.3e}  three-GEMM {err[0]:.3e}")
    assert err[1] <= max(2 * err[0], 1e-6)
    for b, L in enumerate(lens):
        r0 = G + b * S
        for f in (1, 0):
            assert float(got[f][r0 + L:r0 + T].abs().max()) == 0.0 if L < T else True, (b, f)
    hostile = qkv.clone()
    for b, L in enumerate(lens):
        hostile[G + b * S + L:G + b * S + T] = float("nan")
    again = op_rel_attention(hostile.cuda(), p.cuda(), u.cuda(), v.cuda(), torch.tensor(lens), 3, T, G, S, 1, chunk, fused=True)
    assert torch.equal(again.cpu().double().nan_to_num(nan=-7.0), got[1].nan_to_num(nan=-7.0))


def test_chunk_mask_is_the_only_difference():
    """a chunk that covers the whole utterance is full attention, bit for bit, on both routes (the three-GEMM route with
    chunk = 0 is the sequence jv_prompt_encoder_fwd runs, whose own golden test is unchanged)"""
    from jyutvoice_amd.engine import op_rel_attention
    T = 65
    qkv, p, u, v, S = make_inputs(2, T, 5)
    dev = [t.cuda() for t in (qkv, p, u, v)]
    lens = torch.tensor([65, 33])
    for fused in (True, False):
        a = op_rel_attention(*dev, lens, 2, T, G, S, 1, 0, fused=fused)
        b = op_rel_attention(*dev, lens, 2, T, G, S, 1, 128, fused=fused)
        assert torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)), fused


def test_online_softmax_rescale_is_forced():
    """a key in the LAST tile that dominates every earlier one: the running maximum jumps there, so the rescale of the accumulated
    output is what the result hangs on (random scores alone rarely move the maximum by much)"""
    T = 96
    qkv, p, u, v, S = make_inputs(1, T, 9)
    qkv[G + 3, :512] *= 4.0                                   # one query with large scores ...
    qkv[G + 90, 512:1024] = qkv[G + 3, :512] * 0.5            # ... and a late key aligned with it
    _, _, err = run_pair(qkv, p, u, v, [T], 1, T, S, 1, 0)
    print(f"rel_attention spike: fused {err[1]:.3e}  three-GEMM {err[0]:.3e}")
    assert err[1] <= max(2 * err[0], 1e-6)


def test_argument_errors():
    from jyutvoice_amd._lib import JvError
    from jyutvoice_amd.engine import op_rel_attention
    qkv, p, u, v, S = make_inputs(1, 8, 1)
    dev = [t.cuda() for t in (qkv, p, u, v)]
    with pytest.raises(JvError):
        op_rel_attention(*dev, torch.tensor([8]), 1, 8, G, 4, 1, 0)          # stride shorter than the utterance
    with pytest.raises(JvError):
        op_rel_attention(*dev, torch.tensor([8]), 1, 8, G, S, 1, -1)
