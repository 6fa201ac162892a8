"""Streaming token-to-wav: a session that takes speech tokens as they arrive and returns audio that is final -- the same audio the
one-shot route (`CausalMaskedDiffWithXvec.inference(streaming=True)` + `HiFTGenerator.inference`) gives for the whole sequence, up
to the arithmetic of another launch geometry; nothing is cross-faded.

Why a prefix is final.  With `streaming=True` the flow encoder is chunk-causal in 25-token chunks with a 3-token look-ahead
convolution and a causal up-convolution, the estimator chunk-causal in 50-frame chunks with causal convolutions: the frames of
finished chunks do not move when the sequence grows.  So with m tokens known, L = 25 floor((m - 3) / 25) tokens are an aligned prefix
whose look-ahead is known too, and `inference_partial` on the first L + 3 tokens yields the final frames [0, 2 L - F) of the mel
(F prompt frames are cut).  The prefix is solved again on every push that lengthens it, as CosyVoice2 itself does: at B = 1 a solve
of a few hundred frames sits on the launch-latency floor, so a KV-cached estimator would buy little ("Streaming token-to-wav").  The mel
frames go to a `HiFTStream`, which emits the samples whose halo is complete.

    session = Token2WavStream(flow, hift, prompt_token, prompt_feat, embedding, max_tokens=500)
    for piece in token_source:
        play(session.push(piece))
    play(session.finish())
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from . import spec


def aligned_length(m: int) -> int:
    """tokens of the longest chunk-aligned prefix whose 3-token look-ahead lies inside m tokens"""
    return spec.PROMPT_STATIC_CHUNK * ((m - spec.PROMPT_LOOKAHEAD) // spec.PROMPT_STATIC_CHUNK) if m >= spec.PROMPT_LOOKAHEAD else 0


def next_step(m: int, F: int, L_done: int, done: int, final: bool) -> Tuple[int, int, int]:
    """one step of the schedule.  m: tokens so far, prompt included; F: prompt mel frames; L_done: the aligned length already
    solved; done: mel frames already handed on.  -> (tokens to solve, first frame, end frame): (L + 3, done, 2 L - F) when the
    aligned prefix has grown and reaches past the prompt, (m, done, 2 m - F) for the final solve, (0, done, done) otherwise."""
    if final:
        if m < 1 or spec.PROMPT_UP_STRIDE * m < F:
            raise ValueError(f"finish(): {m} tokens give {spec.PROMPT_UP_STRIDE * m} frames, fewer than the {F} prompt frames")
        return m, done, spec.PROMPT_UP_STRIDE * m - F
    L = aligned_length(m)
    if L > L_done and spec.PROMPT_UP_STRIDE * L > F:
        return L + spec.PROMPT_LOOKAHEAD, done, spec.PROMPT_UP_STRIDE * L - F
    return 0, done, done


def frame_schedule(P: int, F: int, pushes: Sequence[int], finish: Optional[int] = 0) -> List[Tuple[int, int, int]]:
    """the whole schedule of a session, without a device: P prompt tokens, F prompt frames, the token count of every push and of
    finish() (None: no finish) -> one (tokens solved, first frame, end frame) per call; (0, d, d) for a call that emits nothing"""
    m, L_done, done, out = P, 0, 0, []
    for i, n in enumerate(list(pushes) + ([] if finish is None else [finish])):
        if n < 0:
            raise ValueError(f"frame_schedule(): call {i} has {n} tokens")
        m += n
        step = next_step(m, F, L_done, done, finish is not None and i == len(pushes))
        if step[0]:
            L_done, done = step[0] - spec.PROMPT_LOOKAHEAD, step[2]
        out.append(step)
    return out


class Token2WavStream:
    """tokens in pieces -> audio in pieces, B = 1.  `push(tokens [n] or [1, n]) -> wav [1, 480 k]` (k may be 0),
    `finish(tokens=None) -> wav`.  `mel` collects the mel pieces handed to the vocoder ([1, 80, frames so far]), `source` the source
    signal of the audio returned so far ([1, 1, samples so far])."""

    def __init__(self, flow, hift, prompt_token, prompt_feat, embedding, max_tokens: int, n_timesteps: int = 10,
                 seed: Optional[int] = None):
        if prompt_token is None:
            prompt_token = torch.zeros(1, 0, dtype=torch.int64)
        if prompt_feat is None:
            prompt_feat = torch.zeros(1, 0, spec.N_FEATS)
        if prompt_token.dim() != 2 or prompt_token.shape[0] != 1 or prompt_token.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"Token2WavStream: prompt_token must be an integer [1, P] tensor, got {tuple(prompt_token.shape)} "
                             f"{prompt_token.dtype}")
        if prompt_feat.dim() != 3 or prompt_feat.shape[0] != 1 or prompt_feat.shape[2] != spec.N_FEATS:
            raise ValueError(f"Token2WavStream: prompt_feat must be [1, frames, {spec.N_FEATS}], got {tuple(prompt_feat.shape)}")
        if embedding.dim() != 2 or tuple(embedding.shape) != (1, spec.SPK_EMBED_DIM):
            raise ValueError(f"Token2WavStream: embedding must be [1, {spec.SPK_EMBED_DIM}], got {tuple(embedding.shape)}")
        if not isinstance(max_tokens, int) or max_tokens < 1:
            raise ValueError(f"Token2WavStream: max_tokens must be a positive int, got {max_tokens!r}")
        if n_timesteps < 1:
            raise ValueError(f"Token2WavStream: n_timesteps must be positive, got {n_timesteps}")
        self.flow, self.hift, self.n_timesteps, self.max_tokens = flow, hift, n_timesteps, max_tokens
        self.prompt_token, self.prompt_feat, self.embedding = prompt_token.to(torch.int64), prompt_feat, embedding
        self.P, self.F = prompt_token.shape[1], prompt_feat.shape[1]
        self.tokens = torch.zeros(1, 0, dtype=torch.int64)
        self.L_done = self.done = 0
        self.finished = False
        # everything above is host-side; from here on the device is touched.  One reservation: no push rebuilds the context
        frames = spec.PROMPT_UP_STRIDE * (self.P + max_tokens)
        flow._rt().ensure(1, frames, 1)
        if seed is not None:
            hift.manual_seed(seed)
        self.vocoder = hift.stream()
        hift._engine(1, frames)      # (the vocoder's runtime, where it is not the flow's)
        self.mel = torch.zeros(1, spec.N_FEATS, 0, device=hift.device)
        self.source = torch.zeros(1, 1, 0, device=hift.device)

    def _take(self, tokens, who):
        if self.finished:
            raise RuntimeError("Token2WavStream: finish() has been called")
        if tokens is None:
            return
        t = torch.as_tensor(tokens)
        if t.dtype not in (torch.int32, torch.int64) or t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[0] != 1):
            raise ValueError(f"{who}: tokens must be an integer [n] or [1, n] tensor, got {tuple(t.shape)} {t.dtype}")
        t = t.reshape(1, -1).to(device="cpu", dtype=torch.int64)
        if self.tokens.shape[1] + t.shape[1] > self.max_tokens:
            raise ValueError(f"{who}: {self.tokens.shape[1]} + {t.shape[1]} tokens exceed the session's max_tokens = {self.max_tokens}")
        self.tokens = torch.cat([self.tokens, t], dim=1)

    def _args(self, n):
        return (self.tokens[:, :n], torch.tensor([n]), self.prompt_token, torch.tensor([self.P]), self.prompt_feat,
                torch.tensor([self.F]), self.embedding, True)

    @torch.inference_mode()
    def push(self, tokens) -> torch.Tensor:
        self._take(tokens, "push()")
        solve, lo, hi = next_step(self.P + self.tokens.shape[1], self.F, self.L_done, self.done, False)
        if not solve:
            return torch.zeros(1, 0, device=self.hift.device)
        mel, _ = self.flow.inference_partial(*self._args(solve - self.P), n_timesteps=self.n_timesteps)
        return self._feed(mel, solve - spec.PROMPT_LOOKAHEAD, lo, hi, False)

    @torch.inference_mode()
    def finish(self, tokens=None) -> torch.Tensor:
        self._take(tokens, "finish()")
        solve, lo, hi = next_step(self.P + self.tokens.shape[1], self.F, self.L_done, self.done, True)
        mel, _ = self.flow.inference(*self._args(solve - self.P), True, n_timesteps=self.n_timesteps)
        wav = self._feed(mel, solve, lo, hi, True)
        self.finished = True
        return wav

    def _feed(self, mel, L, lo, hi, final):
        piece = mel[:, :, lo:hi]
        self.mel = torch.cat([self.mel, piece], dim=2)
        self.L_done, self.done = L, hi
        wav, s = self.vocoder.finish(piece) if final else self.vocoder.push(piece)
        self.source = torch.cat([self.source, s], dim=2)
        return wav
