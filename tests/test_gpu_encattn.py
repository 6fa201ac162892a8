"""Operator parity of the text encoder's one-launch attention (encattn.hip, jv_op_enc_attention fused = 1) and of the four-launch
route it stands beside (fused = 0) against the fp64 restatement tests/encattn_ref.py.

Tolerance (the rule of tests/test_gpu_relattn.py): the fused route's max-abs error against fp64 may be at most twice the yardstick's
error on the same inputs in the same run, or 1e-6 where that is larger; the factor 2 covers the different summation order of an
online softmax.  Up to 512 tokens the yardstick is the four-launch route; above, where that route does not exist, it is the same
expression in fp32 torch on the CPU (the reference's own arithmetic).  Each case prints its pair."""
import pytest
import torch

import encattn_ref as ref

pytestmark = pytest.mark.gpu

G, GAP = 4, 4      # the text encoder's row geometry (encoder.hip E_G, E_GAP)


def make_inputs(B, T, seed):
    """q, k, v of order one (what a LayerNorm'd activation gives through conv_q / conv_k / conv_v); rows of no utterance are NaN
    (they must not be read)"""
    g = torch.Generator().manual_seed(seed)
    S = T + GAP
    qkv = torch.full((ref.n_rows(G, S, B), ref.LDQ), float("nan"))
    for b in range(B):
        qkv[ref.row(G, S, b, 0):ref.row(G, S, b, T)] = torch.randn(T, ref.LDQ, generator=g)
    return qkv, S


def valid_rows(lens, B, T, S, n):
    m = torch.zeros(n, dtype=torch.bool)
    for b in range(B):
        m[ref.row(G, S, b, 0):ref.row(G, S, b, min(int(lens[b]), T))] = True
    return m


def run(qkv, lens, B, T, S, fused):
    from jyutvoice_amd.engine import op_enc_attention
    return op_enc_attention(qkv.cuda(), torch.tensor(lens, dtype=torch.int64), B, T, G, S, fused=fused).cpu()


def errors(qkv, lens, B, T, S):
    """-> (fused output, fused error, yardstick error) over the rows i < L_b; checks what every call owes its row buffer"""
    want = ref.enc_attention(qkv, lens, B, T, G, S)
    own = ~torch.isnan(want[:, 0])
    val = valid_rows(lens, B, T, S, qkv.shape[0])
    got = run(qkv, lens, B, T, S, True)
    assert torch.isnan(got[~own]).all(), "a row of no utterance was written"
    assert torch.isfinite(got[own]).all()
    assert float(got[own & ~val].abs().max()) == 0.0 if bool((own & ~val).any()) else True, "rows at and behind a length are not zero"
    if T <= 512:
        other = run(qkv, lens, B, T, S, False)
        assert torch.isnan(other[~own]).all() and torch.isfinite(other[own]).all()
        name = "four-launch"
    else:
        other = ref.enc_attention(qkv, lens, B, T, G, S, torch.float32)
        name = "fp32 torch"
    e_f = float((got[val].double() - want[val]).abs().max())
    e_y = float((other[val].double() - want[val]).abs().max())
    print(f"enc_attention B={B} T={T} lens={lens}: fused {e_f:.3e}  {name} {e_y:.3e}")
    return got, e_f, e_y


@pytest.mark.parametrize("T", [1, 31, 32, 33, 64, 65, 129, 257, 512])
def test_fused_against_fp64_and_four_launch(T):
    qkv, S = make_inputs(1, T, 2000 + T)
    _, e_f, e_y = errors(qkv, [T], 1, T, S)
    assert e_f <= max(2 * e_y, 1e-6)
    assert e_y <= 1e-5      # the yardstick itself is an fp32-accurate route (outputs of order one)


@pytest.mark.parametrize("T", [513, 545, 1025])
def test_fused_above_512_against_fp64_and_fp32(T):
    qkv, S = make_inputs(1, T, 2000 + T)
    _, e_f, e_y = errors(qkv, [T], 1, T, S)
    assert e_f <= max(2 * e_y, 1e-6)


def test_four_launch_route_refuses_above_512():
    from jyutvoice_amd._lib import JvError
    qkv, S = make_inputs(1, 513, 1)
    with pytest.raises(JvError):
        run(qkv, [513], 1, 513, S, False)


@pytest.mark.parametrize("T", [130, 600])
def test_ragged_batch(T):
    """lengths [T, 1, T // 2 + 1]: a full utterance (T = 130: two query tiles of 64 and two rows of a third), one of a single token
    and one that ends inside a tile.  (1) rows at and behind a length are exactly zero, (2) rows of no utterance stay NaN (both in
    errors()), (3) NaN at and behind the lengths changes no bit, (4) each utterance equals its own B = 1 call with T = L_b"""
    lens = [T, 1, T // 2 + 1]
    qkv, S = make_inputs(3, T, 88 + T)
    got, e_f, e_y = errors(qkv, lens, 3, T, S)
    assert e_f <= max(2 * e_y, 1e-6)
    hostile = qkv.clone()
    for b, L in enumerate(lens):
        hostile[ref.row(G, S, b, L):ref.row(G, S, b, T)] = float("nan")
    again = run(hostile, lens, 3, T, S, True)
    assert torch.equal(again.nan_to_num(nan=-7.0), got.nan_to_num(nan=-7.0))
    for b, L in enumerate(lens):
        S1 = L + GAP
        alone = torch.full((ref.n_rows(G, S1, 1), ref.LDQ), float("nan"))
        alone[G:G + L] = qkv[ref.row(G, S, b, 0):ref.row(G, S, b, L)]
        one = run(alone, [L], 1, L, S1, True)
        assert torch.equal(one[G:G + L], got[ref.row(G, S, b, 0):ref.row(G, S, b, L)]), b


def test_zero_length_reads_nothing():
    T = 40
    qkv, S = make_inputs(2, T, 6)
    qkv[ref.row(G, S, 0, 0):ref.row(G, S, 0, T)] = float("nan")      # the utterance of length 0 is all NaN
    got = run(qkv, [0, T], 2, T, S, True)
    assert float(got[ref.row(G, S, 0, 0):ref.row(G, S, 0, T)].abs().max()) == 0.0
    want = ref.enc_attention(qkv, [0, T], 2, T, G, S)
    r = slice(ref.row(G, S, 1, 0), ref.row(G, S, 1, T))
    assert float((got[r].double() - want[r]).abs().max()) <= 1e-5


def test_dominated_scores(T=96):
    """the running-maximum rescale is where an online softmax goes wrong; three key tiles show it, and at 96 tokens the four-launch
    route is there as the yardstick.  Every key carries 10 w (w a unit vector); query 3 is
    -153 w, so all its scores are -9 (10 + N(0, 1)): near -90, far below the initial maximum of any implementation that starts
    from 0.  Query 5 meets one key in the LAST tile that beats every earlier one by about 60: the maximum jumps there and the
    accumulated output is rescaled by exp(-60)"""
    qkv, S = make_inputs(1, T, 31 + T)
    w = torch.full((288,), 288 ** -0.5)
    for h in range(2):
        qkv[G:G + T, 576 + 288 * h:576 + 288 * (h + 1)] += 10.0 * w
        qkv[G + 3, 288 * h:288 * (h + 1)] = -153.0 * w
        q5 = qkv[G + 5, 288 * h:288 * (h + 1)]
        q5p = q5 - (q5 @ w) * w                                     # (orthogonal to w: query 3 sees -90 at this key too)
        qkv[G + T - 2, 576 + 288 * h:576 + 288 * (h + 1)] = q5p * (60.0 * 288 ** 0.5 / float(q5p @ q5p)) + 10.0 * w
    s3 = (qkv[G:G + T, 576:864] @ qkv[G + 3, :288]) / 288 ** 0.5
    s5 = (qkv[G:G + T, 576:864] @ qkv[G + 5, :288]) / 288 ** 0.5
    assert float(s3.max()) < -50 and float(s5[T - 2] - s5[:T - 2].max()) > 40      # the construction is what it says
    _, e_f, e_y = errors(qkv, [T], 1, T, S)
    assert e_f <= max(2 * e_y, 1e-6)


def test_argument_errors():
    from jyutvoice_amd._lib import JvError
    qkv, S = make_inputs(1, 8, 1)
    for fused in (True, False):
        with pytest.raises(JvError):
            run(qkv, [8], 1, 8, 4, fused)          # stride shorter than the utterance
