"""Shared by test_stream_host.py and test_gpu_stream.py (a plain module, not a conftest; it may import `oracle`): the inputs of the
streaming cases, a CPU restatement of the session's frame schedule written from its description rather than from the product's
code, and windowed decode / f0 through the oracle."""
import math

import torch

T_VOC = 130                                        # frames of the vocoder cases
KEPT = [(0, 50), (50, 85), (85, 130)]              # frames each windowed decode keeps; with a halo of 16: [0,66) [34,101) [69,130)
P, F, N = 7, 14, 70                                # the session case: prompt tokens, prompt frames, tokens
HOPS = [21, 25, 24]                                # pushed, then finish()
N_TIMESTEPS = 4


def window_of(lo, hi, halo, T):
    """the frames a decode has to see so that [lo, hi) come out as in the one-shot decode: `halo` more on each side, except where
    the side is the utterance's true edge"""
    return max(lo - halo, 0), min(hi + halo, T)


def vocoder_inputs(seed=1300, T=T_VOC):
    """the quiet recipe of parity_util: mel = randn [1,80,T], s = tanh(0.05 randn) [1,1,480 T]"""
    g = torch.Generator().manual_seed(seed)
    mel = torch.randn(1, 80, T, generator=g)
    return mel, torch.tanh(torch.randn(1, 1, 480 * T, generator=g) * 0.05)


def windowed_decode(w, mel, s, lo, hi, halo):
    """oracle.hift.decode on the window of [lo, hi), cropped to those frames -> wav [1, 480 (hi - lo)]"""
    from oracle import hift as ohift
    a, b = window_of(lo, hi, halo, mel.shape[2])
    with torch.inference_mode():
        wav = ohift.decode(w, mel[:, :, a:b], s[:, :, 480 * a:480 * b])
    return wav[:, 480 * (lo - a):480 * (hi - a)]


def windowed_f0(w, mel, lo, hi, halo):
    from oracle import hift as ohift
    a, b = window_of(lo, hi, halo, mel.shape[2])
    with torch.inference_mode():
        return ohift.f0_predict(w, mel[:, :, a:b])[:, lo - a:hi - a]


def f0_case():
    """37 frames: voiced, unvoiced (0 and below the threshold of 10 Hz), and one near-zero frame (1e-30 Hz: its increment's last
    bit lies far below the running sum's ulp, which sends the frame scan down its sequential path)"""
    g = torch.Generator().manual_seed(37)
    f0 = 80.0 + 200.0 * torch.rand(2, 37, generator=g)
    f0[0, 3:6] = 0.0
    f0[0, 11] = 1e-30
    f0[0, 12] = 5.0
    f0[0, 30] = 0.0
    f0[1, 0] = 0.0
    f0[1, 20] = 1e-30
    f0[1, 36] = 0.0
    phase = (torch.rand(2, 9, generator=g) * 2 - 1) * math.pi
    return f0, phase


def session_inputs():
    """-> token [1,70], prompt_token [1,7], prompt_feat [1,14,80], embedding [1,192]"""
    from jyutvoice_amd import synth
    tok, _ = synth.prompt_tokens(1, N, first_index=81)
    ptok, _ = synth.prompt_tokens(1, P, first_index=82)
    g = torch.Generator().manual_seed(1570)
    return tok, ptok, torch.randn(1, F, 80, generator=g), torch.randn(1, 192, generator=g)


def schedule_ref(P, F, pushes, finish=0):
    """The session's schedule from its description.  After each push, m tokens are known (prompt included).  The frames that are
    final are those of the whole 25-token chunks among the first m - 3 tokens, two per token, minus the F prompt frames that are
    never emitted; a push emits the final frames not emitted yet and says how many tokens it solved (chunks + the 3 of look-ahead),
    or (0, d, d).  finish (None: absent) adds its tokens and emits everything up to 2 m - F from a solve of all m tokens."""
    out, m, emitted, chunks_solved = [], P, 0, 0
    for n in pushes:
        m += n
        chunks = max(m - 3, 0) // 25
        final_frames = 50 * chunks - F
        if chunks > chunks_solved and final_frames > 0:
            out.append((25 * chunks + 3, emitted, final_frames))
            emitted, chunks_solved = final_frames, chunks
        else:
            out.append((0, emitted, emitted))
    if finish is not None:
        m += finish
        out.append((m, emitted, 2 * m - F))
    return out


def hift_stream_counts(pushes, f0_halo=5, decode_halo=16):
    """frames each HiFTStream.push emits, then what finish() emits: f0 is final 5 frames behind the newest frame, the decode keeps
    what lies 16 frames behind the newest frame with a source"""
    A = E = 0
    out = []
    for t in pushes:
        A += t
        hi = max(A - f0_halo - decode_halo, E)
        out.append(hi - E)
        E = hi
    return out, A - E
