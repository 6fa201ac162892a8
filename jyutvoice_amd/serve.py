"""In-flight ("continuous") batching of text-to-audio: requests join and leave a pool of resident CFM solves between two Euler steps.

`JyutVoiceTTS.synthesise` + `HiFTGenerator.inference` run a closed batch: every utterance enters the solver together, shares one
`n_timesteps` and one `temperature`, and leaves after the last step.  A service in front of it either waits to fill a batch (a
request that arrives just after one started waits a whole pass) or runs small batches at the launch-latency floor.  But between two
steps a solve's state is only x, the running trunk maxima and a step counter, and the estimator takes one t per sample
("In-flight batching"): the utterances of one estimator evaluation need not be at the same step.

    server = SynthServer(tts, hift, max_sessions=32, max_frames=1024, max_tokens=256)
    rid = server.submit(x, x_lengths, lang, tone, word_pos, syllable_pos, spk_embed, n_timesteps=10, seed=7)      # host only
    for rid, out in server.step().items(): play(rid, out["wav"])      # the requests that finished in this step
    server.drain()

A request is DEFINED as that request run alone: its mel is `tts.synthesise(..., n_timesteps=n_r, temperature=tau_r,
length_scale=s_r, batched=True, prompt_lengths=[p_r], cfg_schedule=guidance_rates(n_r, rate_r, window_r, sched_r), t_scheduler=sched_r)`
at B = 1, its audio `hift.inference(mel_r)` at B = 1 after
`hift.manual_seed(seed_r)` -- whatever else is in the pool and whenever the others joined or left.  A request that arrives waits at
most one Euler step, not up to a whole pass.

A request may run its own integrator (`submit(..., solver="midpoint" | "heun")`; DESIGN.md section 5, "Solver"): it then takes two
pool steps per solver step, each at the stage of its own solver, beside requests on Euler or at other stages in the same step
(jv_cfm_pool_step_s), finishes after its last stage, and is that request run alone with `synthesise(..., solver=...)`.

Everything a step decides comes from host state, through `step_table` and `admit_plan` (pure functions, no device).
"""
from __future__ import annotations

import math
from collections import deque
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import spec
from ._lib import STAGE_EULER, STAGE_HEUN1, STAGE_HEUN2, STAGE_MID1, STAGE_MID2
from .flow.flow_matching import EVALS, check_rate, check_scheduler, check_solver, decoder_settings, time_span

FLOW_G, FLOW_GAP = 4, 4      # guard rows ahead of a step's first utterance / between two utterances (csrc/flow_ws.h)
MAX_STEPS = 1024             # the solver's limit on n_timesteps (csrc/flow_ws.h: FlowWs::max_steps)


def step_table(n: int, t_scheduler: str = "cosine", solver: str = "euler"):
    """(t, dt) of the n Euler steps of a request, as fp32 values: the cosine schedule `1 - cos(linspace(0, 1, n + 1) pi / 2)` that
    `synthesise` hands the solver (t_scheduler="linear": `linspace(0, 1, n + 1)` itself) and the reference's running recurrence
    over it (flow_matching.py:230, 260-263, 387-389), in fp32 -- what `solve_schedule` computes for a closed solve of n steps.
    Step k of the request uses (tt[k], dts[k]).

    solver = "midpoint" / "heun": three lists of 2 n entries, one per estimator EVALUATION -- (t, coefficient, stage) as
    jv_cfm_pool_step_s takes them and as `solve_schedule` lays them out for a closed solve of that solver.  Step k, with (t, dt)
    its Euler row, is evaluations 2 k and 2 k + 1:
        midpoint   (t, fp32(0.5 dt), STAGE_MID1),   (fp32(t + fp32(0.5 dt)), dt, STAGE_MID2)
        heun       (t, dt, STAGE_HEUN1),            (fp32(t + dt), fp32(0.5 dt), STAGE_HEUN2)      -- t + dt is the next step's t
    (for "euler" the coefficient is dt and the stage STAGE_EULER throughout: the two lists as ever).  Pure host function."""
    if not isinstance(n, int) or n < 1:
        raise ValueError(f"step_table(): n must be a positive int, got {n!r}")
    check_scheduler("step_table()", t_scheduler)
    if check_solver("step_table()", solver) != "euler":
        tt, dts = step_table(n, t_scheduler)
        mid = solver == "midpoint"
        t2, c2, s2 = [], [], []
        for t, dt in zip(tt, dts):
            t, dt = np.float32(t), np.float32(dt)
            half = np.float32(np.float32(0.5) * dt)
            t2 += [float(t), float(np.float32(t + half) if mid else np.float32(t + dt))]
            c2 += [float(half), float(dt)] if mid else [float(dt), float(half)]
            s2 += [STAGE_MID1, STAGE_MID2] if mid else [STAGE_HEUN1, STAGE_HEUN2]
        return t2, c2, s2
    ts = time_span(n, t_scheduler).numpy().astype(np.float32)
    tt, dts = [], []
    t, dt = ts[0], np.float32(ts[1] - ts[0])
    for s in range(1, n + 1):
        tt.append(float(t))
        dts.append(float(dt))
        t = np.float32(t + dt)
        if s < n:
            dt = np.float32(ts[s + 1] - t)
    return tt, dts


def guidance_rates(n: int, rate: float, window: Optional[Tuple[float, float]] = None, t_scheduler: str = "cosine") -> List[float]:
    """The guidance rate of each of the n Euler steps (flow_matching.py:215-265 with a rate per step): `rate` in a step whose t --
    tt[k] of `step_table(n, t_scheduler)` -- lies in window = (t_lo, t_hi), closed at t_lo and open at t_hi, and 0 outside it (such
    a step runs without unconditional twins in a closed solve).  window = None: `rate` in every step.  Pure host function."""
    who = "guidance_rates()"
    rate = check_rate(who, rate, "rate")
    window = check_window(who, window)
    tt, _ = step_table(n, t_scheduler)
    if window is None:
        return [rate] * n
    return [rate if window[0] <= t < window[1] else 0.0 for t in tt]


def check_window(who: str, window, name: str = "window") -> Optional[Tuple[float, float]]:
    """a guidance window: None, or a pair of finite numbers (t_lo, t_hi)"""
    if window is None:
        return None
    if (not isinstance(window, (tuple, list)) or len(window) != 2 or
            not all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) for v in window)):
        raise ValueError(f"{who}: {name} must be a pair of finite numbers (t_lo, t_hi), got {window!r}")
    return float(window[0]), float(window[1])


def step_rows(lens: Sequence[int]) -> int:
    """rows of one pool step over requests of `lens` frames (each with its CFG twin), in the compact geometry"""
    return FLOW_G + sum(2 * (int(n) + FLOW_GAP) for n in lens)


def admit_plan(waiting: Sequence[int], active: Sequence[int], free_slots: int, row_capacity: int) -> List[int]:
    """Which waiting requests join the next step.  waiting / active: frame counts (prompt + generated) in arrival order / of the
    resident requests.  Strictly first in, first out: the head of the line is admitted while a slot is free and the step's rows,
    FLOW_G + sum 2 (len + FLOW_GAP), stay within row_capacity; the first one that does not fit stops the admission, so nothing
    overtakes it and it is admitted as soon as the pool has room.  -> indices into `waiting`, ascending from 0."""
    rows = step_rows(active)
    out: List[int] = []
    for i, n in enumerate(waiting):
        need = 2 * (int(n) + FLOW_GAP)
        if len(out) >= free_slots or rows + need > row_capacity:
            break
        rows += need
        out.append(i)
    return out


class _Request:
    def __init__(self, rid, args, prompt_feat, prompt_h, n, temperature, length_scale, seed, loudness=None, peak=None, rates=None,
                 t_scheduler="cosine", solver="euler"):
        self.rid, self.args, self.prompt_feat, self.prompt_h = rid, args, prompt_feat, prompt_h
        self.loudness, self.peak = loudness, peak      # target LUFS and peak ceiling of the output, or None
        self.n, self.temperature, self.length_scale, self.seed = n, temperature, length_scale, seed
        self.p = 0 if prompt_feat is None else int(prompt_feat.shape[1])
        # one row per estimator evaluation = per pool step: an Euler step is one, a midpoint / Heun step two (`step_table`)
        self.solver = solver
        if solver == "euler":
            self.tt, self.dts = step_table(n, t_scheduler)
            self.stages = [STAGE_EULER] * n
        else:
            self.tt, self.dts, self.stages = step_table(n, t_scheduler, solver)
        rates = [spec.CFG_RATE] * n if rates is None else rates
        self.rates = [rates[k // EVALS[solver]] for k in range(len(self.tt))]      # a step's rate holds for both of its evaluations
        self.k = 0                 # pool steps (evaluations) taken; the request is finished at len(tt)
        self.slot = None
        self.y = None              # generated frames, once the text encoder has run
        self.mu_y = self.spks = None      # [1, 80, y], [1, 80] on the device, between encoding and admission

    @property
    def frames(self):
        return self.p + self.y


class SynthServer:
    """A pool of `max_sessions` resident solves served step by step.

    `submit(...)` takes one request (the B = 1 tensors `synthesise` takes, its own n_timesteps, temperature, length_scale, voice
    prompt and vocoder seed), validates it on the host and returns its id.  `step()`, in order: runs the text encoder and
    `length_regulate` for the requests at the head of the line (one call per distinct length_scale), admits them first in, first out
    while a slot is free and the step's rows fit (`admit_plan`), packs them into their slots (jv_cfm_pool_admit), runs ONE Euler step
    for all resident requests, each at its own (t, dt) (jv_cfm_pool_step; a request admitted in this step takes its first step in
    it), and for the requests whose last step this was fetches the mel (jv_cfm_pool_fetch), runs the vocoder for all of them together
    -- one `HiFTStreamBatch` slot each, opened after `manual_seed(seed_r)` and advanced once with the whole mel as final, which is
    `hift.inference` of that mel bit for bit in its source signal -- and frees their slots.
    -> {rid: {"wav" [1, 480 y], "mel" [1, 80, y], "mel_length": y, "source" [1, 1, 480 y]}}; a request that cannot be served (more
    frames than max_frames once its durations are known) comes back as {rid: {"error": message}}.
    A request submitted with `loudness` (LUFS; optionally `peak`, a ceiling on |sample|) has its audio brought to that integrated
    loudness (ITU-R BS.1770-4): the requests of a step that ask for it are measured and scaled together after the vocoder
    (jv_loudness, jv_peak, jv_level_gain, jv_level_apply), and their results gain "lufs" (as measured) and "gain" (as applied); each
    gets the bits `normalize_loudness` of its own audio gives, and a request without the option is untouched.

    One reservation at construction for max_sessions utterances of max_frames frames / max_tokens tokens: no step rebuilds a context.
    row_capacity (default: what that reservation holds) bounds the rows of a step.  `engine`: the library context to run on
    (default: the runtime of `tts.device`)."""

    def __init__(self, tts, hift, max_sessions: int = 32, max_frames: int = 1024, max_tokens: int = 256,
                 row_capacity: Optional[int] = None, engine=None):
        for name, v in (("max_sessions", max_sessions), ("max_frames", max_frames), ("max_tokens", max_tokens)):
            if not isinstance(v, int) or v < 1:
                raise ValueError(f"SynthServer: {name} must be a positive int, got {v!r}")
        full = step_rows([max_frames] * max_sessions)
        if row_capacity is None:
            row_capacity = full
        if not isinstance(row_capacity, int) or row_capacity < step_rows([1]) or row_capacity > full:
            raise ValueError(f"SynthServer: row_capacity must be an int in [{step_rows([1])}, {full}], got {row_capacity!r}")
        self.tts, self.hift = tts, hift
        self.max_sessions, self.max_frames, self.max_tokens, self.row_capacity = max_sessions, max_frames, max_tokens, row_capacity
        self.device = torch.device(getattr(tts, "device", "cpu"))
        self._waiting: deque = deque()
        self._active: Dict[int, _Request] = {}      # slot -> request
        self._free = list(range(max_sessions))
        self._failed: Dict[int, dict] = {}
        self._next_rid = 0
        self.steps = 0
        # everything above is host-side; from here on the device is touched
        self._rt = None
        if engine is None:
            from .runtime import get_runtime
            self._rt = get_runtime(self.device)
            engine = self._rt.ensure(max_sessions, max_frames, max_tokens)
        self._engine = engine
        self.pool = engine.cfm_pool(max_sessions, max_frames)
        self.vocoder = hift.stream_batch(max_sessions, max_frames)

    def _eng(self):
        return self._rt.engine if self._rt is not None else self._engine      # (a weight reload makes a new context: the pools stay)

    # ---- host only ------------------------------------------------------------------------------------------------------------------
    def submit(self, x, x_lengths, lang, tone, word_pos, syllable_pos, spk_embed, prompt_feat=None, prompt_h=None, n_timesteps=10,
               temperature=1.0, length_scale=1.0, seed=None, loudness=None, peak=None, cfg_rate=None, cfg_window=None,
               t_scheduler="cosine", solver=None) -> int:
        """solver: the request's integrator, "euler" / "midpoint" / "heun" (None: the decoder's `solver`) -- n_timesteps second-order
        steps take 2 n_timesteps pool steps, and the request is the one `synthesise(..., solver=solver)` runs alone at B = 1.
        cfg_rate: the request's guidance rate (None: the decoder's inference_cfg_rate); cfg_window = (t_lo, t_hi): guidance in
        the steps whose t lies in [t_lo, t_hi) only, rate 0 outside (`guidance_rates`); t_scheduler: "cosine" / "linear" (None: the
        decoder's)."""
        rid = self._next_rid
        who = f"SynthServer.submit(): request {rid}"
        ids = {"x": x, "lang": lang, "tone": tone, "word_pos": word_pos, "syllable_pos": syllable_pos}
        for name, v in ids.items():
            if not isinstance(v, torch.Tensor) or v.dim() != 2 or v.shape[0] != 1 or v.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"{who}: {name} must be an integer [1, tokens] tensor, got "
                                 f"{tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__}")
            if v.shape != x.shape:
                raise ValueError(f"{who}: {name} has shape {tuple(v.shape)}, x {tuple(x.shape)}")
        Tt = x.shape[1]
        if Tt < 1 or Tt > self.max_tokens:
            raise ValueError(f"{who}: {Tt} tokens outside [1, max_tokens = {self.max_tokens}]")
        xl = torch.as_tensor(x_lengths).reshape(-1)
        if xl.numel() != 1 or xl.dtype not in (torch.int32, torch.int64) or not 1 <= int(xl[0]) <= Tt:
            raise ValueError(f"{who}: x_lengths must be one integer in [1, {Tt}]")
        if not isinstance(spk_embed, torch.Tensor) or tuple(spk_embed.shape) != (1, spec.SPK_EMBED_DIM):
            raise ValueError(f"{who}: spk_embed must be [1, {spec.SPK_EMBED_DIM}]")
        if (prompt_feat is None) != (prompt_h is None):
            raise ValueError(f"{who}: prompt_feat and prompt_h come together")
        if prompt_feat is not None:
            for name, v in (("prompt_feat", prompt_feat), ("prompt_h", prompt_h)):
                if not isinstance(v, torch.Tensor) or v.dim() != 3 or v.shape[0] != 1 or v.shape[2] != spec.N_FEATS:
                    raise ValueError(f"{who}: {name} must be [1, frames, {spec.N_FEATS}]")
            if prompt_feat.shape[1] != prompt_h.shape[1]:
                raise ValueError(f"{who}: prompt_feat has {prompt_feat.shape[1]} frames, prompt_h {prompt_h.shape[1]}")
            if prompt_feat.shape[1] == 0:
                prompt_feat = prompt_h = None
        if not isinstance(n_timesteps, int) or isinstance(n_timesteps, bool) or not 1 <= n_timesteps <= MAX_STEPS:
            raise ValueError(f"{who}: n_timesteps must be an int in [1, {MAX_STEPS}], got {n_timesteps!r}")
        temperature, length_scale = float(temperature), float(length_scale)
        if not math.isfinite(temperature):
            raise ValueError(f"{who}: temperature must be finite, got {temperature}")
        if not math.isfinite(length_scale) or length_scale <= 0:
            raise ValueError(f"{who}: length_scale must be positive, got {length_scale}")
        if loudness is not None and not (isinstance(loudness, (int, float)) and math.isfinite(loudness)):
            raise ValueError(f"{who}: loudness must be a finite number of LUFS (or None), got {loudness!r}")
        if peak is not None and not (isinstance(peak, (int, float)) and math.isfinite(peak) and peak > 0):
            raise ValueError(f"{who}: peak must be positive and finite (or None), got {peak!r}")
        if peak is not None and loudness is None:
            raise ValueError(f"{who}: peak limits the gain of loudness: give loudness too")
        conf_rate, conf_sched, conf_solver = decoder_settings(getattr(self.tts, "decoder", None))
        solver = check_solver(who, conf_solver if solver is None else solver)
        if n_timesteps * EVALS[solver] > MAX_STEPS:
            raise ValueError(f"{who}: n_timesteps = {n_timesteps} with the {solver} solver is {n_timesteps * EVALS[solver]} estimator "
                             f"evaluations, the limit is {MAX_STEPS}")
        t_scheduler = check_scheduler(who, conf_sched if t_scheduler is None else t_scheduler)
        cfg_rate = check_rate(who, conf_rate if cfg_rate is None else cfg_rate, "cfg_rate")
        rates = guidance_rates(n_timesteps, cfg_rate, check_window(who, cfg_window, "cfg_window"), t_scheduler)
        p = 0 if prompt_feat is None else prompt_feat.shape[1]
        # every token gets at least one frame unless length_scale shortens it; the prompt alone must leave room for one
        least = p + max(1, int(xl[0]) if length_scale >= 1.0 else 1)
        if least > self.max_frames or step_rows([least]) > self.row_capacity:
            raise ValueError(f"{who}: at least {least} frames ({p} of them prompt) exceed max_frames = {self.max_frames} or the "
                             f"row capacity {self.row_capacity}")
        if seed is None:      # (a host draw, as HiFTGenerator draws it)
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
        args = (x, xl.to(torch.int64), lang, tone, word_pos, syllable_pos, spk_embed)
        self._waiting.append(_Request(rid, args, prompt_feat, prompt_h, n_timesteps, temperature, length_scale, int(seed),
                                      None if loudness is None else float(loudness), None if peak is None else float(peak),
                                      rates, t_scheduler, solver))
        self._next_rid += 1
        return rid

    def pending(self) -> int:
        """requests waiting or resident"""
        return len(self._waiting) + len(self._active)

    # ---- one step -------------------------------------------------------------------------------------------------------------------
    def _encode(self, eng, reqs: List[_Request]):
        """text encoder + length regulation of `reqs` as one batch per distinct length_scale; leaves y, mu_y, spks on each"""
        groups: Dict[float, List[_Request]] = {}
        for r in reqs:
            groups.setdefault(r.length_scale, []).append(r)
        for scale, grp in groups.items():
            Tt = max(r.args[0].shape[1] for r in grp)
            pad = lambda i: torch.cat([torch.nn.functional.pad(r.args[i].to(torch.int64), (0, Tt - r.args[i].shape[1])) for r in grp])
            xl = torch.cat([r.args[1] for r in grp])
            spk = torch.cat([r.args[6].to(torch.float32) for r in grp])
            _, mu_x, logw, c = eng.encoder(pad(0), xl, pad(2), pad(3), pad(4), pad(5), spk)
            _, _, _, mu_y = eng.length_regulate(logw, xl, mu_x, scale, host_lengths=True)
            for b, r in enumerate(grp):
                r.y = int(eng.y_lengths_host[b])
                r.mu_y, r.spks = mu_y[b:b + 1, :, :r.y], c[b:b + 1]

    def _admit(self, eng):
        # the requests that could be admitted now: as many as there are free slots, from the head of the line
        head = [r for r, _ in zip(self._waiting, range(len(self._free)))]
        fresh = [r for r in head if r.y is None]
        if fresh:
            self._encode(eng, fresh)
        for r in [r for r in head if r.frames > self.max_frames or step_rows([r.frames]) > self.row_capacity]:
            self._waiting.remove(r)
            head.remove(r)
            self._failed[r.rid] = {"error": f"request {r.rid}: {r.p} prompt + {r.y} generated frames exceed max_frames = "
                                            f"{self.max_frames} or the row capacity {self.row_capacity}"}
        take = admit_plan([r.frames for r in head], [r.frames for r in self._active.values()], len(self._free), self.row_capacity)
        new = [self._waiting.popleft() for _ in take]
        groups: Dict[float, List[_Request]] = {}
        for r in new:
            r.slot = self._free.pop(0)
            self._active[r.slot] = r
            groups.setdefault(r.length_scale, []).append(r)
        for grp in groups.values():      # (one pack per encoder batch: its mu_y rows share a buffer)
            B, Ty, P = len(grp), max(r.y for r in grp), max(r.p for r in grp)
            dev = grp[0].mu_y.device
            mu_y = torch.zeros(B, spec.N_FEATS, Ty, device=dev)
            spks = torch.cat([r.spks for r in grp])
            ph = pf = None
            if P:
                ph, pf = torch.zeros(B, P, spec.N_FEATS), torch.zeros(B, P, spec.N_FEATS)
            for b, r in enumerate(grp):
                mu_y[b, :, :r.y] = r.mu_y[0]
                if r.p:
                    ph[b, :r.p], pf[b, :r.p] = r.prompt_h[0].to("cpu", torch.float32), r.prompt_feat[0].to("cpu", torch.float32)
                r.mu_y = r.spks = None
            eng.cfm_pool_admit(self.pool, mu_y, [r.y for r in grp], None if ph is None else ph.to(dev), None if pf is None else pf.to(dev),
                               [r.p for r in grp], spks, [r.slot for r in grp], [r.temperature for r in grp])

    @torch.inference_mode()
    def step(self) -> Dict[int, dict]:
        eng = self._eng()
        if self._waiting and self._free:
            self._admit(eng)
        done, self._failed = self._failed, {}
        live = list(self._active.values())
        if not live:
            return done
        cfg = [r.rates[r.k] for r in live]
        # (all at the default rate: the entry without rates, jv_cfm_pool_step, which is the other one with 0.7 for all)
        kw = {} if all(abs(v - spec.CFG_RATE) <= 1e-12 for v in cfg) else {"cfg": cfg}
        stages = [r.stages[r.k] for r in live]
        if any(s != STAGE_EULER for s in stages):      # (all on Euler: the entries above, as before solvers per request existed)
            kw = {"cfg": cfg, "stage": stages}
        eng.cfm_pool_step(self.pool, [r.slot for r in live], [r.frames for r in live], [r.tt[r.k] for r in live],
                          [r.dts[r.k] for r in live], **kw)
        self.steps += 1
        for r in live:
            r.k += 1
        fin = [r for r in live if r.k == len(r.tt)]
        if not fin:
            return done
        mel = eng.cfm_pool_fetch(self.pool, [r.slot for r in fin], [r.p for r in fin], [r.y for r in fin])
        for r in fin:      # a source signal per request: the slot opened after manual_seed(seed_r) is hift.inference's draw
            self.hift.manual_seed(r.seed)
            self.vocoder.open(r.slot)
        out = self.vocoder.advance(mel, [(r.slot, b, 0, r.y, True) for b, r in enumerate(fin)])
        for b, r in enumerate(fin):
            wav, s = out[r.slot]
            done[r.rid] = {"wav": wav, "mel": mel[b:b + 1, :, :r.y], "mel_length": r.y, "source": s.clone()}
            self.vocoder.close(r.slot)
            del self._active[r.slot]
            self._free.append(r.slot)
        self._normalize(eng, [r for r in fin if r.loudness is not None], done)
        return done

    def _normalize(self, eng, reqs: List[_Request], done: Dict[int, dict]):
        """the finished requests that asked for a loudness, as one ragged batch: one measurement, one gain per distinct
        (loudness, peak), one scaling"""
        if not reqs:
            return
        wavs = [done[r.rid]["wav"] for r in reqs]
        lens = torch.tensor([w.shape[1] for w in wavs], dtype=torch.int32)
        buf = torch.zeros(len(reqs), int(lens.max()), device=wavs[0].device)
        for b, w in enumerate(wavs):
            buf[b, : w.shape[1]] = w[0]
        lens = lens.to(buf.device)
        lufs, pk = eng.loudness(buf, spec.SAMPLE_RATE, lens), eng.peak(buf, lens)
        gain = torch.ones(len(reqs), device=buf.device)
        groups: Dict[tuple, List[int]] = {}
        for b, r in enumerate(reqs):
            groups.setdefault((r.loudness, r.peak), []).append(b)
        for (target, ceiling), members in groups.items():
            idx = torch.tensor(members, device=buf.device)
            gain[idx] = eng.level_gain(lufs[idx], None if ceiling is None else pk[idx], target, ceiling)
        out, _ = eng.level_apply(buf, lens, gain=gain)
        for b, (r, l, g) in enumerate(zip(reqs, lufs.tolist(), gain.tolist())):
            done[r.rid].update({"wav": out[b:b + 1, : wavs[b].shape[1]], "lufs": l, "gain": g})

    def drain(self) -> Dict[int, dict]:
        """step() until nothing is waiting or resident -> all results"""
        out: Dict[int, dict] = {}
        while self.pending() or self._failed:
            out.update(self.step())
        return out
