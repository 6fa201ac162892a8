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

Several listeners: `Token2WavServer` advances all its sessions in one batched step -- one `inference_partial_batch` solve with a
look-ahead context per row, one `HiFTStreamBatch` advance -- because a push at B = 1 is almost all launch latency, which N sessions
advanced one after another pay N times ("Concurrent sessions").  `batch_plan` is its schedule, host only.
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
                 seed: Optional[int] = None, cfg_rate=None, cfg_schedule=None, t_scheduler=None, solver=None):
        # cfg_rate / cfg_schedule: the guidance rate of every solve of the session / one rate per Euler step, handed to the flow's
        # inference calls; t_scheduler: "cosine" / "linear"; solver: "euler" / "midpoint" / "heun" (None each: the flow decoder's configuration)
        self._cfg = {k: v for k, v in (("cfg_rate", cfg_rate), ("cfg_schedule", cfg_schedule), ("t_scheduler", t_scheduler),
                                       ("solver", solver)) if v is not None}
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
        mel, _ = self.flow.inference_partial(*self._args(solve - self.P), n_timesteps=self.n_timesteps, **self._cfg)
        return self._feed(mel, solve - spec.PROMPT_LOOKAHEAD, lo, hi, False)

    @torch.inference_mode()
    def finish(self, tokens=None) -> torch.Tensor:
        self._take(tokens, "finish()")
        solve, lo, hi = next_step(self.P + self.tokens.shape[1], self.F, self.L_done, self.done, True)
        mel, _ = self.flow.inference(*self._args(solve - self.P), True, n_timesteps=self.n_timesteps, **self._cfg)
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


# ---- concurrent sessions ------------------------------------------------------------------------------------------------------------
def batch_plan(states: Sequence[Tuple[int, int, int, int, int, bool]]) -> List[Tuple[int, int, int, int, int]]:
    """One step of a server from host state alone.  states: per session (P prompt tokens, F prompt frames, tokens pushed so far,
    L_done, done, closing) -- the arguments of `next_step`, which every session is asked in turn.  -> the rows of the step's batch,
    one (index into states, tokens to solve, ctx, first frame, end frame) per session that has a solve due: ctx = 3 for a push
    solve (the last three tokens are look-ahead context), 0 for the final solve of a closing session.  A session with nothing due
    is not in the rows."""
    rows = []
    for i, (P, F, n, L_done, done, closing) in enumerate(states):
        solve, lo, hi = next_step(P + n, F, L_done, done, bool(closing))
        if solve:
            rows.append((i, solve, 0 if closing else spec.PROMPT_LOOKAHEAD, lo, hi))
    return rows


class _Session:
    def __init__(self, slot, P, F):
        self.slot, self.P, self.F = slot, P, F
        self.n = self.L_done = self.done = 0
        self.closing = self.finished = False


class Token2WavServer:
    """Several Token2WavStream sessions advanced together: `step()` solves every session that has a solve due in ONE
    `inference_partial_batch` call (a context of 3 tokens for the rows in mid-stream, 0 for those that finish) and moves all their
    vocoders in ONE `HiFTStreamBatch.advance`, so its launch count does not grow with the number of sessions.

        server = Token2WavServer(flow, hift, max_sessions=8, max_tokens=500)
        sid = server.open(prompt_token, prompt_feat, embedding)
        server.push(sid, tokens)            # host only
        server.close(sid)                   # the next step runs the final solve
        for sid, wav in server.step().items(): play(sid, wav)

    Every session follows `next_step` and its vocoder slot HiFTStream's schedule: a session's audio is what a Token2WavStream with
    the same seed and pushes returns, up to the arithmetic of another batch geometry.  One reservation at construction, for
    `max_sessions` utterances of 2 (max_prompt_tokens + max_tokens) frames: no step rebuilds a context.  `mel(sid)`, `source(sid)`
    and `f0(sid)` are views of a session's records; those of a finished session stay valid until its slot is opened again."""

    def __init__(self, flow, hift, max_sessions: int, max_tokens: int, n_timesteps: int = 10, max_prompt_tokens: int = 150,
                 cfg_rate=None, cfg_schedule=None, t_scheduler=None, solver=None):
        # cfg_rate / cfg_schedule / solver: as for Token2WavStream, for every step of the server (one solve serves all its sessions)
        self._cfg = {k: v for k, v in (("cfg_rate", cfg_rate), ("cfg_schedule", cfg_schedule), ("t_scheduler", t_scheduler),
                                       ("solver", solver)) if v is not None}
        for name, v in (("max_sessions", max_sessions), ("max_tokens", max_tokens)):
            if not isinstance(v, int) or v < 1:
                raise ValueError(f"Token2WavServer: {name} must be a positive int, got {v!r}")
        if not isinstance(max_prompt_tokens, int) or max_prompt_tokens < 0:
            raise ValueError(f"Token2WavServer: max_prompt_tokens must be a non-negative int, got {max_prompt_tokens!r}")
        if n_timesteps < 1:
            raise ValueError(f"Token2WavServer: n_timesteps must be positive, got {n_timesteps}")
        self.flow, self.hift, self.n_timesteps = flow, hift, n_timesteps
        self.max_sessions, self.max_tokens, self.max_prompt_tokens = max_sessions, max_tokens, max_prompt_tokens
        up = spec.PROMPT_UP_STRIDE
        self.frames = up * (max_prompt_tokens + max_tokens)
        # host-side pools, one row per slot: a step's padded batch is an index_select of them
        self._ptok = torch.zeros(max_sessions, max_prompt_tokens, dtype=torch.int64)
        self._feat = torch.zeros(max_sessions, up * max_prompt_tokens, spec.N_FEATS)
        self._emb = torch.zeros(max_sessions, spec.SPK_EMBED_DIM)
        self._tok = torch.zeros(max_sessions, max_tokens, dtype=torch.int64)
        self._sessions = {}
        self._free = list(range(max_sessions))
        self._next_sid = 0
        # everything above is host-side; from here on the device is touched.  One reservation: no step rebuilds a context
        flow._rt().ensure(max_sessions, self.frames, 1)
        self.vocoder = hift.stream_batch(max_sessions, self.frames)

    def _session(self, sid, who):
        s = self._sessions.get(sid)
        if s is None:
            raise RuntimeError(f"Token2WavServer.{who}: unknown session {sid!r}")
        if s.finished:
            raise RuntimeError(f"Token2WavServer.{who}: session {sid} has finished")
        return s

    def open(self, prompt_token, prompt_feat, embedding, seed: Optional[int] = None) -> int:
        if prompt_token is None:
            prompt_token = torch.zeros(1, 0, dtype=torch.int64)
        if prompt_feat is None:
            prompt_feat = torch.zeros(1, 0, spec.N_FEATS)
        if prompt_token.dim() != 2 or prompt_token.shape[0] != 1 or prompt_token.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"Token2WavServer.open(): prompt_token must be an integer [1, P] tensor, got {tuple(prompt_token.shape)} "
                             f"{prompt_token.dtype}")
        if prompt_feat.dim() != 3 or prompt_feat.shape[0] != 1 or prompt_feat.shape[2] != spec.N_FEATS:
            raise ValueError(f"Token2WavServer.open(): prompt_feat must be [1, frames, {spec.N_FEATS}], got {tuple(prompt_feat.shape)}")
        if embedding.dim() != 2 or tuple(embedding.shape) != (1, spec.SPK_EMBED_DIM):
            raise ValueError(f"Token2WavServer.open(): embedding must be [1, {spec.SPK_EMBED_DIM}], got {tuple(embedding.shape)}")
        P, F = prompt_token.shape[1], prompt_feat.shape[1]
        if P > self.max_prompt_tokens or F > self._feat.shape[1]:
            raise ValueError(f"Token2WavServer.open(): a prompt of {P} tokens / {F} frames exceeds max_prompt_tokens = "
                             f"{self.max_prompt_tokens} (and twice as many frames)")
        if not self._free:
            raise RuntimeError(f"Token2WavServer.open(): all {self.max_sessions} sessions are taken")
        slot = self._free.pop(0)
        for old in [k for k, v in self._sessions.items() if v.slot == slot]:      # (the finished session whose records lived here)
            del self._sessions[old]
        self._ptok[slot, :P] = prompt_token[0].to(device="cpu", dtype=torch.int64)
        self._feat[slot, :F] = prompt_feat[0].to(device="cpu", dtype=torch.float32)
        self._emb[slot] = embedding[0].to(device="cpu", dtype=torch.float32)
        if seed is not None:
            self.hift.manual_seed(seed)
        self.vocoder.open(slot)
        sid = self._next_sid
        self._next_sid += 1
        self._sessions[sid] = _Session(slot, P, F)
        return sid

    def push(self, sid: int, tokens) -> None:
        s = self._session(sid, "push()")
        if s.closing:
            raise RuntimeError(f"Token2WavServer.push(): close() has been called for session {sid}")
        t = torch.as_tensor(tokens)
        if t.dtype not in (torch.int32, torch.int64) or t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[0] != 1):
            raise ValueError(f"push(): tokens must be an integer [n] or [1, n] tensor, got {tuple(t.shape)} {t.dtype}")
        t = t.reshape(-1).to(device="cpu", dtype=torch.int64)
        if s.n + t.shape[0] > self.max_tokens:
            raise ValueError(f"push(): {s.n} + {t.shape[0]} tokens exceed the session's max_tokens = {self.max_tokens}")
        self._tok[s.slot, s.n:s.n + t.shape[0]] = t
        s.n += t.shape[0]

    def close(self, sid: int) -> None:
        """no more tokens: the next step runs this session's final solve and returns the rest of its audio"""
        s = self._session(sid, "close()")
        if spec.PROMPT_UP_STRIDE * (s.P + s.n) < max(s.F, 1):
            raise ValueError(f"close(): {s.P + s.n} tokens give {spec.PROMPT_UP_STRIDE * (s.P + s.n)} frames, fewer than the {s.F} "
                             "prompt frames")
        s.closing = True

    def finished(self, sid: int) -> bool:
        """the session's final step has run (or its slot has been given to another session since)"""
        s = self._sessions.get(sid)
        return s is None or s.finished

    def _records(self, sid):
        s = self._sessions.get(sid)
        if s is None:
            raise RuntimeError(f"Token2WavServer: unknown session {sid!r}")
        return self.vocoder.records(s.slot)

    def mel(self, sid: int) -> torch.Tensor:
        """the mel pieces handed to the vocoder so far, [1, 80, frames]"""
        return self._records(sid)[0]

    def source(self, sid: int) -> torch.Tensor:
        """the source signal of the audio returned so far, [1, 1, samples]"""
        return self._records(sid)[1]

    def f0(self, sid: int) -> torch.Tensor:
        """the f0 record, [1, frames with a final f0]"""
        return self._records(sid)[2]

    def source_draws(self, sid: int):
        """(phase [1, 9], seed, call) of the session's source signal"""
        slot = self._sessions[sid].slot
        return (self.vocoder.phase[slot:slot + 1],) + self.vocoder.draws[slot]

    @torch.inference_mode()
    def step(self):
        """advance every session that has a solve due -> {sid: wav [1, 480 k]}; nothing due: nothing is launched"""
        live = [(sid, s) for sid, s in self._sessions.items() if not s.finished]
        plan = batch_plan([(s.P, s.F, s.n, s.L_done, s.done, s.closing) for _, s in live])
        if not plan:
            return {}
        rows = [live[i] + (solve, ctx, lo, hi) for i, solve, ctx, lo, hi in plan]
        slots = torch.tensor([s.slot for _, s, *_ in rows])
        p_len = [min(s.P, solve) for _, s, solve, *_ in rows]      # (a prefix may end inside the prompt)
        n_len = [solve - p for (_, _, solve, *_), p in zip(rows, p_len)]
        f_len = [s.F for _, s, *_ in rows]
        P, N, F = max(p_len), max(n_len), max(f_len)
        mel, _ = self.flow.inference_partial_batch(
            self._tok.index_select(0, slots)[:, :N], torch.tensor(n_len), self._ptok.index_select(0, slots)[:, :P], torch.tensor(p_len),
            self._feat.index_select(0, slots)[:, :F], torch.tensor(f_len), self._emb.index_select(0, slots),
            [ctx for *_, ctx, _, _ in rows], streaming=True, n_timesteps=self.n_timesteps, **self._cfg)
        out = self.vocoder.advance(mel, [(s.slot, r, lo, hi, s.closing) for r, (_, s, _, _, lo, hi) in enumerate(rows)])
        res = {}
        for sid, s, solve, ctx, lo, hi in rows:
            s.L_done, s.done = solve - ctx, hi
            res[sid] = out[s.slot][0]
            if s.closing:
                s.finished = True
                self.vocoder.close(s.slot)
                self._free.append(s.slot)
        return res
