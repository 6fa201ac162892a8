"""Thin host wrapper around one libjyutvoice_hip context.

PyTorch is plumbing only: it owns the device buffers handed to the C ABI (raw `data_ptr()`s) and the
stream they are enqueued on.  Every numerical step of the hot path runs inside the library.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib, spec
from ._lib import JV_MODEL_FLOW, JV_MODEL_HIFT, JV_MODEL_PROMPT, JV_MODEL_TTS, JvError, check


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


class CfmPool:
    """The state of `slots` resident CFM solves (jv_cfm_pool_*), owned by the caller: x / mu / cond [slots, max_frames, 80]
    frame-major, the projected speaker vectors [slots, 80] and the running trunk maxima [slots, 3, 2] (buffer; request, CFG
    twin).  The library keeps nothing about a request between calls, so the pools survive jv_reserve and a new context."""

    def __init__(self, slots: int, max_frames: int, device):
        if not isinstance(slots, int) or slots < 1 or not isinstance(max_frames, int) or max_frames < 1:
            raise ValueError(f"CfmPool: slots and max_frames must be positive ints, got {slots!r}, {max_frames!r}")
        self.slots, self.max_frames = slots, max_frames
        self.x = torch.zeros(slots, max_frames, spec.N_FEATS, device=device)
        self.mu = torch.zeros_like(self.x)
        self.cond = torch.zeros_like(self.x)
        self.spks = torch.zeros(slots, spec.N_FEATS, device=device)
        self.amax = torch.zeros(slots, 3, 2, device=device)
        self.x0 = self.k1 = None      # second-order requests (jv_cfm_pool_step_s): the state a step started from / its first slope

    def ensure_stage_pools(self):
        """x0 / k1, sized like x: allocated when the first request with a second-order solver is admitted"""
        if self.x0 is None:
            self.x0, self.k1 = torch.zeros_like(self.x), torch.zeros_like(self.x)

    def tensors(self):
        return self.x, self.mu, self.cond, self.spks, self.amax


class Engine:
    """One library context = packed weights + workspace for up to `max_batch` utterances of
    `max_frames` mel frames / `max_tokens` tokens, bound to one GPU."""

    def __init__(self, device="cuda:0", max_batch=1, max_frames=2048, max_tokens=512):
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("jyutvoice_amd runs on an AMD GPU only (device must be cuda:N); there is no CPU path")
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible to PyTorch-ROCm; jyutvoice_amd has no CPU path")
        self.max_batch, self.max_frames, self.max_tokens = max_batch, max_frames, max_tokens
        h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        check(self.lib.jv_create(C.byref(h), idx, max_batch, max_frames, max_tokens))
        self._h = h
        self._loaded = {JV_MODEL_TTS: False, JV_MODEL_HIFT: False, JV_MODEL_PROMPT: False, JV_MODEL_FLOW: False}

    def reserve(self, max_batch, max_frames, max_tokens):
        """grow (or shrink) the workspace of the live context; weights stay loaded (jv_reserve)"""
        check(self.lib.jv_reserve(self._h, int(max_batch), int(max_frames), int(max_tokens)))
        self.max_batch, self.max_frames, self.max_tokens = max_batch, max_frames, max_tokens

    def broken(self) -> bool:
        """True once a failed jv_reserve could not restore the previous workspace: the context refuses every call"""
        return not getattr(self, "_h", None) or self.lib.jv_usable(self._h) == 0

    def close(self):
        if getattr(self, "_h", None):
            self.lib.jv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- registry ---------------------------------------------------------------------------------
    def registry(self, model: int) -> Dict[str, tuple]:
        """name -> shape of a model's tensors; JV_MODEL_FLOW: the decoder.* / spk_embed_affine_layer.* slots of JV_MODEL_TTS"""
        out = {}
        owner = JV_MODEL_TTS if model == JV_MODEL_FLOW else model
        for i in range(self.lib.jv_num_tensors(self._h)):
            if self.lib.jv_tensor_model(self._h, i) != owner:
                continue
            if model == JV_MODEL_FLOW and not self.lib.jv_tensor_name(self._h, i).decode().startswith(spec.FLOW_DECODER_PREFIXES):
                continue
            nd = self.lib.jv_tensor_ndim(self._h, i)
            out[self.lib.jv_tensor_name(self._h, i).decode()] = tuple(
                int(self.lib.jv_tensor_dim(self._h, i, d)) for d in range(nd))
        return out

    # ---- weights ----------------------------------------------------------------------------------
    def load_state_dict(self, model: int, sd: Dict[str, torch.Tensor], strict: bool = True):
        """Mirror of nn.Module.load_state_dict for the library's registry: same missing/unexpected-key
        semantics; shapes are checked by the library (RuntimeError on mismatch, like torch)."""
        expected = self.registry(model)
        missing = [k for k in expected if k not in sd]
        unexpected = [k for k in sd if k not in expected]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: Missing key(s): {missing[:8]}{'...' if len(missing) > 8 else ''}; "
                               f"Unexpected key(s): {unexpected[:8]}{'...' if len(unexpected) > 8 else ''}")
        st = _stream(self.device)
        for k in expected:
            if k not in sd:
                continue
            t = _f32(sd[k].detach(), self.device)
            shape = (C.c_int64 * t.dim())(*t.shape)
            try:
                check(self.lib.jv_load_tensor(self._h, k.encode(), _ptr(t), shape, t.dim(), 1, st))
            except JvError as e:
                raise RuntimeError(e.msg) from None
        torch.cuda.synchronize(self.device)
        if not missing:
            check(self.lib.jv_finalize(self._h, model, st))
            self._loaded[model] = True
            if model == JV_MODEL_TTS:
                self._loaded[JV_MODEL_FLOW] = True
        return missing, unexpected

    def load_noise(self, noise: torch.Tensor):
        t = _f32(noise, self.device)
        check(self.lib.jv_load_noise(self._h, _ptr(t), t.numel(), 1, _stream(self.device)))
        torch.cuda.synchronize(self.device)

    # ---- flow ---------------------------------------------------------------------------------------
    def set_streaming(self, chunk_frames: int = spec.EST_STATIC_CHUNK):
        """chunk-causal estimator attention (the reference's streaming=True); 0 = full attention"""
        check(self.lib.jv_flow_set_streaming(self._h, int(chunk_frames)))

    def set_guidance(self, rates=None):
        """the classifier-free-guidance rate of the closed solves on this context (jv_flow_set_guidance; flow_matching.py:215-265).
        None: the default, 0.7 in every Euler step.  A number, or a sequence of one: that rate in every step.  A sequence of n:
        one rate per step of a solve with n_timesteps = n (any other solve raises JvError).  A step whose rate is exactly 0 runs
        without unconditional twins.  A negative or non-finite rate raises JvError and leaves the mode as it was."""
        if rates is None:
            check(self.lib.jv_flow_set_guidance(self._h, None, 0))
            return
        vals = [float(rates)] if isinstance(rates, (int, float)) else [float(r) for r in
                                                                      (rates.tolist() if isinstance(rates, torch.Tensor) else rates)]
        if not vals:
            raise ValueError("set_guidance: an empty schedule; pass None for the default rate")
        check(self.lib.jv_flow_set_guidance(self._h, (C.c_float * len(vals))(*vals), len(vals)))

    @contextlib.contextmanager
    def guidance(self, rates):
        """`with eng.guidance(rates):` -- set_guidance(rates) for the block, the default again behind it (rates = None: nothing)"""
        if rates is None:
            yield
            return
        self.set_guidance(rates)
        try:
            yield
        finally:
            self.set_guidance(None)

    def set_solver(self, name: str = "euler"):
        """the integrator of the closed solves on this context (jv_flow_set_solver): "euler" (default; flow_matching.py:215-265),
        "midpoint" or "heun" -- second-order steps of two estimator evaluations each, `n_timesteps` staying the number of steps.
        An unknown name raises ValueError naming the choices and leaves the mode as it was."""
        if name not in _lib.SOLVERS:
            raise ValueError(f"set_solver: solver must be one of {list(_lib.SOLVERS)}, got {name!r}")
        check(self.lib.jv_flow_set_solver(self._h, _lib.SOLVERS[name]))

    @contextlib.contextmanager
    def solver(self, name):
        """`with eng.solver(name):` -- set_solver(name) for the block, Euler again behind it (name = None or "euler": nothing)"""
        if name is None or name == "euler":
            yield
            return
        self.set_solver(name)
        try:
            yield
        finally:
            self.set_solver("euler")

    def set_step_graph(self, on: bool = True):
        """replay the Euler step of cfm_solve as a captured hipGraph (default off: measured no faster; same results)"""
        check(self.lib.jv_flow_set_graph(self._h, 1 if on else 0))

    def set_exact_range(self, on: bool = True):
        """True: bf16x6 for every contraction; False (default): fp16x3 on the estimator linears whose input range is proven
        at load time (jv_flow_set_contraction)"""
        check(self.lib.jv_flow_set_contraction(self._h, 1 if on else 0))

    PRECISIONS = {"fp32": 0, "fp16": 1}      # JV_PRECISION_FP32 / JV_PRECISION_FP16

    def set_precision(self, precision: str = "fp32"):
        """"fp32" (default): every contraction at fp32 accuracy.  "fp16": the estimator as the reference's fp16 TensorRT plan
        runs it -- each contraction that would run fp16x3 issues its hi x hi product alone (operands rounded to 11 significant
        bits under the same power-of-two scales, fp32 accumulation); layers without a usable bound, the encoders and the
        vocoder are unchanged (jv_flow_set_precision).  Not together with set_exact_range(True)."""
        if precision not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(self.PRECISIONS)}, not {precision!r}")
        check(self.lib.jv_flow_set_precision(self._h, self.PRECISIONS[precision]))

    def contraction_info(self, with_precision: bool = False) -> dict:
        """which of the estimator's transformer layers have a usable load-time bound (fp16x3) and which stay on bf16x6
        (jv_flow_contraction_info); with_precision: also "precision", the mode set_precision() left ("fp32" / "fp16")"""
        out = (C.c_int32 * 5)()
        check(self.lib.jv_flow_contraction_info(self._h, out, 5))
        info = {"blocks": out[0], "blocks_all_h3": out[1], "linears_h3": out[2], "attention_h3": out[3]}
        if with_precision:
            info["precision"] = "fp16" if out[4] else "fp32"
        return info

    def flow_estimator(self, x, mask_lens, mu, t, spks, cond):
        """[B2,80,T] tensors on the device; mask_lens int32 [B2] or None."""
        B2, _, T = x.shape
        x, mu, cond = (_f32(v, self.device) for v in (x, mu, cond))
        t, spks = _f32(t, self.device), _f32(spks, self.device)
        lens = None if mask_lens is None else mask_lens.to(device=self.device, dtype=torch.int32).contiguous()
        out = torch.empty_like(x)
        check(self.lib.jv_flow_estimator_step(self._h, _ptr(x), _ptr(lens), _ptr(mu), _ptr(t), _ptr(spks), _ptr(cond), B2, T,
                                              _ptr(out), _stream(self.device)))
        return out

    def flow_estimator_tap(self, mode, x, mask_lens, mu, t, spks, cond, tap, out=None):
        """jv_flow_estimator_tap: the launches of one estimator evaluation up to and including the stage `tap` (a name of
        _lib.EST_TAPS), that stage's buffer channels first, zeros at and behind every sample's clamped length.  mode "entry":
        flow_estimator's call (x, mu, cond [B2,80,T], t [B2], spks [B2,80]) -> [B2, C, T]; mode "step": one evaluation of a
        cfm_solve step over B utterances and their B unconditional twins (x, mu, cond [B,80,T], t one scalar, spks [B,80]) ->
        [2B, C, T], twin b at sample B + b.  The time taps (_lib.EST_TIME_TAPS) are [B2, C] / [1, C].  (mode or tap as a raw
        id, or `out` given: passed on as they are -- the library rejects what it does not know and a buffer that is too small)"""
        B, _, T = x.shape
        x, mu, cond = (_f32(v, self.device) for v in (x, mu, cond))
        t, spks = _f32(torch.as_tensor(t).reshape(-1), self.device), _f32(spks, self.device)
        lens = None if mask_lens is None else mask_lens.to(device=self.device, dtype=torch.int32).contiguous()
        step = mode in ("step", _lib.EST_MODES["step"])
        tap_id, C_ = _lib.EST_TAPS[tap] if isinstance(tap, str) else (int(tap), 1)
        if out is None:
            out = (torch.empty(1 if step else B, C_, device=self.device) if tap in _lib.EST_TIME_TAPS
                   else torch.empty(2 * B if step else B, C_, T, device=self.device))
        check(self.lib.jv_flow_estimator_tap(self._h, _lib.EST_MODES[mode] if isinstance(mode, str) else int(mode), _ptr(x), _ptr(lens),
                                             _ptr(mu), _ptr(t), _ptr(spks), _ptr(cond), B, T, tap_id, _ptr(out), out.numel(),
                                             _stream(self.device)))
        return out

    def cfm_solve(self, mu, lens, spks, cond, n_timesteps, temperature=1.0, t_span=None):
        B, _, T = mu.shape
        mu, cond, spks = _f32(mu, self.device), _f32(cond, self.device), _f32(spks, self.device)
        lens_d = None if lens is None else lens.to(device=self.device, dtype=torch.int32).contiguous()
        mel = torch.empty_like(mu)
        ts = None
        if t_span is not None:
            ts_host = t_span.detach().to("cpu", torch.float32).contiguous()
            ts = (C.c_float * ts_host.numel())(*ts_host.tolist())
        check(self.lib.jv_cfm_solve(self._h, _ptr(mu), _ptr(lens_d), _ptr(spks), _ptr(cond), B, T, int(n_timesteps),
                                    float(temperature), ts, _ptr(mel), _stream(self.device)))
        return mel

    def cfm_solve_prompted(self, mu_y, y_lens, prompt_h, prompt_feat, prompt_lens, spks, n_timesteps, temperature=1.0,
                           t_span=None):
        """jv_cfm_solve_prompted: mu_y [B,80,Ty], prompt_h [B,Ph,80], prompt_feat [B,Pf,80] (batch, time, channel, as the
        prompt encoder and extract_speech_feat return them), y_lens / prompt_lens [B] -> the generated frames [B,80,Ty],
        utterance b in [:y_lens[b]], zeros behind.  The tensors go to the library as they are: no assembly here."""
        B, _, Ty = mu_y.shape
        mu_y, spks = _f32(mu_y, self.device), _f32(spks, self.device)
        prompt_h, prompt_feat = _f32(prompt_h, self.device), _f32(prompt_feat, self.device)
        yl = y_lens.to(device=self.device, dtype=torch.int32).contiguous()
        pl = prompt_lens.to(device=self.device, dtype=torch.int32).contiguous()
        mel = torch.empty_like(mu_y)
        ts = None
        if t_span is not None:
            ts_host = t_span.detach().to("cpu", torch.float32).contiguous()
            ts = (C.c_float * ts_host.numel())(*ts_host.tolist())
        check(self.lib.jv_cfm_solve_prompted(self._h, _ptr(mu_y), _ptr(yl), _ptr(prompt_h), _ptr(prompt_feat), _ptr(pl), _ptr(spks),
                                             B, Ty, prompt_h.shape[1], prompt_feat.shape[1], int(n_timesteps), float(temperature),
                                             ts, _ptr(mel), _stream(self.device)))
        return mel

    # ---- in-flight batching: requests join and leave a running solve between Euler steps ---------------------
    def cfm_pool(self, slots: int, max_frames: int) -> "CfmPool":
        """the caller-owned state pools of `slots` resident solves of at most `max_frames` (prompt + generated) frames"""
        return CfmPool(slots, max_frames, self.device)

    @staticmethod
    def _host_vec(who, name, values, ctype, B):
        values = [v for v in (values.tolist() if isinstance(values, torch.Tensor) else values)]
        if len(values) != B:
            raise ValueError(f"{who}: {name} must hold {B} entries, got {len(values)}")
        return (ctype * B)(*values)

    def cfm_pool_admit(self, pool, mu_y, y_lens, prompt_h, prompt_feat, prompt_lens, spks, slots, temperatures):
        """jv_cfm_pool_admit: pack B new requests into `slots` of `pool`.  mu_y [B,80,Ty], prompt_h [B,Ph,80] / prompt_feat
        [B,Pf,80] (or None: no prompts), spks [B,80] on the device; y_lens, prompt_lens, slots, temperatures: B host values
        each (lists or CPU tensors -- a device tensor would cost a synchronisation)"""
        who = "cfm_pool_admit"
        B, _, Ty = mu_y.shape
        mu_y, spks = _f32(mu_y, self.device), _f32(spks, self.device)
        if prompt_h is None or prompt_feat is None:
            prompt_h = prompt_feat = torch.zeros(B, 0, spec.N_FEATS, device=self.device)
        prompt_h, prompt_feat = _f32(prompt_h, self.device), _f32(prompt_feat, self.device)
        check(self.lib.jv_cfm_pool_admit(
            self._h, _ptr(mu_y) if Ty else None, _ptr(prompt_h) if prompt_h.shape[1] else None,
            _ptr(prompt_feat) if prompt_feat.shape[1] else None, _ptr(spks),
            self._host_vec(who, "y_lens", y_lens, C.c_int32, B), self._host_vec(who, "prompt_lens", prompt_lens, C.c_int32, B),
            self._host_vec(who, "slots", slots, C.c_int32, B), self._host_vec(who, "temperatures", temperatures, C.c_float, B),
            B, Ty, prompt_h.shape[1], prompt_feat.shape[1], _ptr(pool.x), _ptr(pool.mu), _ptr(pool.cond), _ptr(pool.spks),
            _ptr(pool.amax), pool.slots, pool.max_frames, _stream(self.device)))

    def cfm_pool_step(self, pool, slots, lens, t, dt, cfg=None, stage=None):
        """jv_cfm_pool_step: ONE Euler + CFG step of the listed slots, request b with lens[b] frames at (t[b], dt[b]); B host
        values each.  cfg: the guidance rate of every request in this step (jv_cfm_pool_step_g); None: 0.7 for all.  stage
        (jv_cfm_pool_step_s): the stage of every request's own solver in this step (_lib.STAGE_*), of which dt[b] is then the
        coefficient; the pool's x0 / k1 are allocated on first use.  Nothing comes back to the host."""
        who, B = "cfm_pool_step", len(slots)
        if stage is not None:
            pool.ensure_stage_pools()
            check(self.lib.jv_cfm_pool_step_s(
                self._h, _ptr(pool.x), _ptr(pool.mu), _ptr(pool.cond), _ptr(pool.spks), _ptr(pool.amax), _ptr(pool.x0), _ptr(pool.k1),
                pool.slots, pool.max_frames, self._host_vec(who, "slots", slots, C.c_int32, B),
                self._host_vec(who, "lens", lens, C.c_int32, B), self._host_vec(who, "t", t, C.c_float, B),
                self._host_vec(who, "dt", dt, C.c_float, B),
                self._host_vec(who, "cfg", [spec.CFG_RATE] * B if cfg is None else cfg, C.c_float, B),
                self._host_vec(who, "stage", stage, C.c_int32, B), B, _stream(self.device)))
            return
        args = (self._h, _ptr(pool.x), _ptr(pool.mu), _ptr(pool.cond), _ptr(pool.spks), _ptr(pool.amax), pool.slots, pool.max_frames,
                self._host_vec(who, "slots", slots, C.c_int32, B), self._host_vec(who, "lens", lens, C.c_int32, B),
                self._host_vec(who, "t", t, C.c_float, B), self._host_vec(who, "dt", dt, C.c_float, B))
        if cfg is None:
            check(self.lib.jv_cfm_pool_step(*args, B, _stream(self.device)))
        else:
            check(self.lib.jv_cfm_pool_step_g(*args, self._host_vec(who, "cfg", cfg, C.c_float, B), B, _stream(self.device)))

    def cfm_pool_fetch(self, pool, slots, first, lens, frames=None):
        """jv_cfm_pool_fetch: frames first[b] .. first[b] + lens[b] - 1 of the listed slots -> mel [B, 80, frames] (default: the
        longest), left-aligned, zeros behind lens[b]"""
        who, B = "cfm_pool_fetch", len(slots)
        Tm = int(max(lens)) if frames is None else int(frames)
        mel = torch.empty(B, spec.N_FEATS, Tm, device=self.device)
        check(self.lib.jv_cfm_pool_fetch(
            self._h, _ptr(pool.x), pool.slots, pool.max_frames, self._host_vec(who, "slots", slots, C.c_int32, B),
            self._host_vec(who, "first", first, C.c_int32, B), self._host_vec(who, "lens", lens, C.c_int32, B), B, Tm, _ptr(mel),
            _stream(self.device)))
        return mel

    # ---- prompt mel front-end --------------------------------------------------------------------------
    def load_mel_basis(self, basis: torch.Tensor):
        t = basis.detach().to("cpu", torch.float32).contiguous()
        check(self.lib.jv_load_mel_basis(self._h, t.data_ptr(), t.numel(), 0, _stream(self.device)))

    def mel_spectrogram(self, wav, lens=None):
        """utils/audio.py:18-63 with extract_speech_feat's parameters: wav [B, n] -> log-mel [B, 80, 1 + (n - 480) // 480].
        lens ([B] sample counts): recordings of different durations, recording b = wav[b, :lens[b]] with the reflect padding
        at its own end; returns (mel, mel_lens int32 [B]) with mel[b, :, mel_lens[b]:] = 0 (jv_mel_spectrogram_ragged)"""
        w = _f32(wav, self.device)
        B, n = w.shape
        T = 1 + (n - 480) // 480
        mel = torch.empty(B, spec.N_FEATS, max(T, 0), device=self.device)
        if lens is not None:
            wl = lens.to(device=self.device, dtype=torch.int32).contiguous()
            if wl.shape != (B,):
                raise ValueError(f"mel_spectrogram: lens must have shape [{B}], got {tuple(wl.shape)}")
            mel_lens = torch.empty(B, dtype=torch.int32, device=self.device)
            check(self.lib.jv_mel_spectrogram_ragged(self._h, _ptr(w), _ptr(wl), B, n, _ptr(mel), _ptr(mel_lens), _stream(self.device)))
            return mel, mel_lens
        check(self.lib.jv_mel_spectrogram(self._h, _ptr(w), B, n, _ptr(mel), _stream(self.device)))
        return mel

    # ---- sample-rate conversion ------------------------------------------------------------------------
    def resample(self, wav, orig_freq, new_freq, lens=None):
        """torchaudio.functional.resample(wav, orig_freq, new_freq) with its defaults (infer.py:368-382; jv_resample):
        wav [B, n] -> out [B, resample_length(n)].  lens ([B] sample counts, clamped to [0, n]): recording b = wav[b, :lens[b]],
        what lies behind is not read; returns (out, out_lens int32 [B]) with out[b, out_lens[b]:] = 0"""
        w = _f32(wav, self.device)
        if w.dim() != 2:
            raise ValueError(f"resample: wav must be [B, n], got {tuple(w.shape)}")
        B, n = w.shape
        n_out = int(self.lib.jv_resample_length(n, int(orig_freq), int(new_freq)))
        out = torch.empty(B, max(n_out, 0), device=self.device)
        wl = out_lens = None
        if lens is not None:
            wl = lens.to(device=self.device, dtype=torch.int32).contiguous()
            if wl.shape != (B,):
                raise ValueError(f"resample: lens must have shape [{B}], got {tuple(wl.shape)}")
            out_lens = torch.empty(B, dtype=torch.int32, device=self.device)
        check(self.lib.jv_resample(self._h, _ptr(w), _ptr(wl), B, n, int(orig_freq), int(new_freq), _ptr(out), out.shape[1],
                                   _ptr(out_lens), _stream(self.device)))
        return out if lens is None else (out, out_lens)

    # ---- levels: silence trim, peak, BS.1770 loudness, gain -------------------------------------------
    def _level_in(self, who, wav, lens):
        w = _f32(wav, self.device)
        if w.dim() != 2:
            raise ValueError(f"{who}: wav must be [B, n], got {tuple(w.shape)}")
        return w, self._level_vec(who, "lens", lens, w.shape[0], torch.int32)

    def _level_vec(self, who, name, v, B, dtype):
        if v is None:
            return None
        v = v.to(device=self.device, dtype=dtype).contiguous()
        if v.shape != (B,):
            raise ValueError(f"{who}: {name} must have shape [{B}], got {tuple(v.shape)}")
        return v

    def trim_bounds(self, wav, lens=None, top_db=60.0, frame_length=440, hop_length=220):
        """librosa.effects.trim's bounds with zero centre padding (jv_trim_bounds): wav [B, n], lens [B] sample counts or None
        -> (start, end) int32 [B] on the device; recording b without its leading / trailing silence is wav[b, start[b]:end[b]]"""
        who = "trim_bounds"
        w, wl = self._level_in(who, wav, lens)
        if not (isinstance(top_db, (int, float)) and top_db > 0 and top_db != float("inf")):
            raise ValueError(f"{who}: top_db must be positive and finite, got {top_db!r}")
        if not (isinstance(frame_length, int) and 1 <= frame_length <= 8192):
            raise ValueError(f"{who}: frame_length must be an int in [1, 8192], got {frame_length!r}")
        if not (isinstance(hop_length, int) and hop_length >= 1):
            raise ValueError(f"{who}: hop_length must be an int >= 1, got {hop_length!r}")
        B, n = w.shape
        start = torch.empty(B, dtype=torch.int32, device=self.device)
        end = torch.empty_like(start)
        check(self.lib.jv_trim_bounds(self._h, _ptr(w), _ptr(wl), B, n, float(top_db), frame_length, hop_length, _ptr(start),
                                      _ptr(end), _stream(self.device)))
        return start, end

    def peak(self, wav, lens=None, start=None, end=None):
        """max |wav[b, start[b]:end[b]]| (the whole recording without bounds), exact (jv_peak) -> [B] fp32 on the device"""
        who = "peak"
        w, wl = self._level_in(who, wav, lens)
        B, n = w.shape
        s, e = self._level_vec(who, "start", start, B, torch.int32), self._level_vec(who, "end", end, B, torch.int32)
        out = torch.empty(B, device=self.device)
        check(self.lib.jv_peak(self._h, _ptr(w), _ptr(wl), _ptr(s), _ptr(e), B, n, _ptr(out), _stream(self.device)))
        return out

    def loudness(self, wav, sample_rate, lens=None):
        """integrated loudness after ITU-R BS.1770-4, mono (jv_loudness): wav [B, n] at sample_rate -> [B] LUFS on the device;
        -inf for a recording shorter than 400 ms or with no block above -70 LUFS"""
        who = "loudness"
        w, wl = self._level_in(who, wav, lens)
        if not (isinstance(sample_rate, int) and 8000 <= sample_rate <= 192000):
            raise ValueError(f"{who}: sample_rate must be an int in [8000, 192000], got {sample_rate!r}")
        B, n = w.shape
        out = torch.empty(B, device=self.device)
        check(self.lib.jv_loudness(self._h, _ptr(w), _ptr(wl), B, n, sample_rate, _ptr(out), _stream(self.device)))
        return out

    def level_gain(self, lufs=None, peak=None, target=-23.0, ceiling=None):
        """the gain that brings a recording of `lufs` to `target`, limited so that its peak stays at `ceiling` (None: no limit);
        lufs None: the prompt rule, ceiling / peak where peak > ceiling, else 1 (jv_level_gain) -> [B] fp32 on the device"""
        who = "level_gain"
        if lufs is None and peak is None:
            raise ValueError(f"{who}: needs lufs, peak or both")
        B = (lufs if lufs is not None else peak).shape[0]
        lu, pk = self._level_vec(who, "lufs", lufs, B, torch.float32), self._level_vec(who, "peak", peak, B, torch.float32)
        if ceiling is not None and not (isinstance(ceiling, (int, float)) and 0 < ceiling < float("inf")):
            raise ValueError(f"{who}: ceiling must be positive and finite (or None), got {ceiling!r}")
        if ceiling is not None and pk is None:
            raise ValueError(f"{who}: a ceiling needs peak")
        if lu is None and ceiling is None:
            raise ValueError(f"{who}: without lufs (the prompt rule) a ceiling is needed")
        if lu is not None and not (isinstance(target, (int, float)) and abs(target) < float("inf")):
            raise ValueError(f"{who}: target must be finite, got {target!r}")
        out = torch.empty(B, device=self.device)
        check(self.lib.jv_level_gain(self._h, _ptr(lu), _ptr(pk), B, float(target), float(ceiling or 0.0), _ptr(out),
                                     _stream(self.device)))
        return out

    def level_apply(self, wav, lens=None, start=None, end=None, gain=None, tail=0):
        """out[b, :e - s] = wav[b, s:e] * gain[b], then `tail` zeros, exact zeros behind (jv_level_apply; bounds default to the
        recording, the gain to 1) -> (out [B, n + tail], out_lens int32 [B] = e - s + tail)"""
        who = "level_apply"
        w, wl = self._level_in(who, wav, lens)
        B, n = w.shape
        if not (isinstance(tail, int) and tail >= 0):
            raise ValueError(f"{who}: tail must be an int >= 0, got {tail!r}")
        s, e = self._level_vec(who, "start", start, B, torch.int32), self._level_vec(who, "end", end, B, torch.int32)
        g = self._level_vec(who, "gain", gain, B, torch.float32)
        out = torch.empty(B, n + tail, device=self.device)
        out_lens = torch.empty(B, dtype=torch.int32, device=self.device)
        check(self.lib.jv_level_apply(self._h, _ptr(w), _ptr(wl), _ptr(s), _ptr(e), _ptr(g), B, n, tail, _ptr(out), out.shape[1],
                                      _ptr(out_lens), _stream(self.device)))
        return out, out_lens

    # ---- reference-audio features at 16 kHz -----------------------------------------------------------
    def load_whisper_filters(self, filters: torch.Tensor):
        """the [128, 201] filterbank whisper ships (librosa.filters.mel(sr=16000, n_fft=400, n_mels=128)); jv_load_whisper_filters"""
        t = filters.detach().to("cpu", torch.float32).contiguous()
        check(self.lib.jv_load_whisper_filters(self._h, t.data_ptr(), t.numel(), 0, _stream(self.device)))

    def _feat16k(self, who, wav, lens):
        w = _f32(wav, self.device)
        if w.dim() != 2:
            raise ValueError(f"{who}: wav must be [B, n], got {tuple(w.shape)}")
        wl = out_lens = None
        if lens is not None:
            wl = lens.to(device=self.device, dtype=torch.int32).contiguous()
            if wl.shape != (w.shape[0],):
                raise ValueError(f"{who}: lens must have shape [{w.shape[0]}], got {tuple(wl.shape)}")
            out_lens = torch.empty(w.shape[0], dtype=torch.int32, device=self.device)
        return w, wl, out_lens

    def fbank(self, wav, lens=None, subtract_mean=True):
        """kaldi.fbank(wav, num_mel_bins=80, dither=0, sample_frequency=16000) [minus its mean over frames] (infer.py:148-163;
        jv_fbank): wav [B, n] at 16 kHz -> [B, Tmax, 80], Tmax = 1 + (n - 400) // 160.  lens ([B] sample counts, clamped to
        [0, n]): recording b = wav[b, :lens[b]], what lies behind is not read; returns (out, out_lens int32 [B]) with exact
        zeros behind each recording's frames.  Nothing comes back to the host."""
        w, wl, out_lens = self._feat16k("fbank", wav, lens)
        B, n = w.shape
        out = torch.empty(B, int(self.lib.jv_fbank_frames(n)), 80, device=self.device)
        check(self.lib.jv_fbank(self._h, _ptr(w), _ptr(wl), B, n, 1 if subtract_mean else 0, _ptr(out), _ptr(out_lens),
                                _stream(self.device)))
        return out if lens is None else (out, out_lens)

    def whisper_log_mel(self, wav, lens=None):
        """whisper.log_mel_spectrogram(wav, n_mels=128) (infer.py:98-145; jv_whisper_log_mel): wav [B, n] at 16 kHz ->
        [B, 128, n // 160]; the max - 8 clamp is taken per recording.  lens as in `fbank`."""
        w, wl, out_lens = self._feat16k("whisper_log_mel", wav, lens)
        B, n = w.shape
        out = torch.empty(B, 128, int(self.lib.jv_whisper_frames(n)), device=self.device)
        check(self.lib.jv_whisper_log_mel(self._h, _ptr(w), _ptr(wl), B, n, _ptr(out), _ptr(out_lens), _stream(self.device)))
        return out if lens is None else (out, out_lens)

    # ---- prompt branch --------------------------------------------------------------------------------
    def prompt_encoder(self, token, token_len):
        """FlowEncoder.forward (infer.py:66-83): token [B,Tk] int64, token_len [B] -> prompt_h [B, 2*Tk, 80]"""
        B, Tk = token.shape
        tok = token.to(device=self.device, dtype=torch.int64).contiguous()
        tl = token_len.to(device=self.device, dtype=torch.int64).contiguous()
        h = torch.empty(B, 2 * Tk, spec.N_FEATS, device=self.device)
        check(self.lib.jv_prompt_encoder_fwd(self._h, _ptr(tok), _ptr(tl), B, Tk, _ptr(h), _stream(self.device)))
        return h

    # ---- token-to-mel (flow/flow.py:300-358) -------------------------------------------------------------
    def _tok(self, t):
        return None if t is None else t.to(device=self.device, dtype=torch.int64).contiguous()

    def flow_encoder(self, prompt_token, prompt_len, token, token_len, streaming=False):
        """jv_flow_encoder_fwd: utterance b = [prompt_token[b, :p_b] | token[b, :n_b]] (prompt_token None or [B, 0]: no prompt)
        -> (h [B, 2*(P+N), 80], h_lens int32 [B]); zeros behind 2*(p_b + n_b)"""
        B, N = token.shape
        P = 0 if prompt_token is None else prompt_token.shape[1]
        tok, tl = self._tok(token), self._tok(token_len)
        ptok, pl = (self._tok(prompt_token), self._tok(prompt_len)) if P > 0 else (None, None)
        h = torch.empty(B, 2 * (P + N), spec.N_FEATS, device=self.device)
        hl = torch.empty(B, dtype=torch.int32, device=self.device)
        check(self.lib.jv_flow_encoder_fwd(self._h, _ptr(ptok), _ptr(pl), _ptr(tok), _ptr(tl), B, P, N, 1 if streaming else 0, _ptr(h),
                                           _ptr(hl), _stream(self.device)))
        return h, hl

    def flow_token2mel(self, prompt_token, prompt_len, token, token_len, prompt_feat, feat_len, embedding, streaming=False,
                       n_timesteps=10, temperature=1.0, t_span=None):
        """jv_flow_token2mel: tokens -> (mel [B, 80, 2*(P+N)], mel_lens int32 [B]): frames f_b .. T_b - 1 of each utterance,
        left-aligned, zeros behind.  prompt_feat [B, F, 80] (None: F = 0), feat_len [B] = f_b, embedding [B, 192] raw."""
        B, N = token.shape
        P = 0 if prompt_token is None else prompt_token.shape[1]
        F = 0 if prompt_feat is None else prompt_feat.shape[1]
        tok, tl = self._tok(token), self._tok(token_len)
        ptok, pl = (self._tok(prompt_token), self._tok(prompt_len)) if P > 0 else (None, None)
        pf = _f32(prompt_feat, self.device) if F > 0 else None
        fl = feat_len.to(device=self.device, dtype=torch.int32).contiguous()
        emb = _f32(embedding, self.device)
        mel = torch.empty(B, spec.N_FEATS, 2 * (P + N), device=self.device)
        ml = torch.empty(B, dtype=torch.int32, device=self.device)
        ts = None
        if t_span is not None:
            ts_host = t_span.detach().to("cpu", torch.float32).contiguous()
            ts = (C.c_float * ts_host.numel())(*ts_host.tolist())
        check(self.lib.jv_flow_token2mel(self._h, _ptr(ptok), _ptr(pl), _ptr(tok), _ptr(tl), _ptr(pf), _ptr(fl), _ptr(emb), B, P, N, F,
                                         1 if streaming else 0, int(n_timesteps), float(temperature), ts, _ptr(mel), _ptr(ml),
                                         _stream(self.device)))
        return mel, ml

    def flow_encoder_partial(self, prompt_token, prompt_len, token, token_len, streaming=False):
        """jv_flow_encoder_fwd_partial (B = 1): the last 3 of the P + N tokens are look-ahead context only -> (h [1, 2*(P+N-3), 80],
        h_lens int32 [1])"""
        B, N = token.shape
        P = 0 if prompt_token is None else prompt_token.shape[1]
        if B != 1 or P + N < 4:
            raise ValueError(f"flow_encoder_partial(): B must be 1 and P + N at least 4, got B = {B}, P + N = {P + N}")
        tok, tl = self._tok(token), self._tok(token_len)
        ptok, pl = (self._tok(prompt_token), self._tok(prompt_len)) if P > 0 else (None, None)
        h = torch.empty(1, 2 * (P + N - 3), spec.N_FEATS, device=self.device)
        hl = torch.empty(1, dtype=torch.int32, device=self.device)
        check(self.lib.jv_flow_encoder_fwd_partial(self._h, _ptr(ptok), _ptr(pl), _ptr(tok), _ptr(tl), P, N, 1 if streaming else 0,
                                                   _ptr(h), _ptr(hl), _stream(self.device)))
        return h, hl

    def flow_token2mel_partial(self, prompt_token, prompt_len, token, token_len, prompt_feat, feat_len, embedding, streaming=False,
                               n_timesteps=10, temperature=1.0, t_span=None):
        """jv_flow_token2mel_partial (B = 1): as flow_token2mel on the first L = P + N - 3 tokens, the last three being the look-ahead
        convolution's context -> (mel [1, 80, 2 L], mel_lens int32 [1] = 2 L - f)"""
        B, N = token.shape
        P = 0 if prompt_token is None else prompt_token.shape[1]
        F = 0 if prompt_feat is None else prompt_feat.shape[1]
        if B != 1 or P + N < 4:
            raise ValueError(f"flow_token2mel_partial(): B must be 1 and P + N at least 4, got B = {B}, P + N = {P + N}")
        tok, tl = self._tok(token), self._tok(token_len)
        ptok, pl = (self._tok(prompt_token), self._tok(prompt_len)) if P > 0 else (None, None)
        pf = _f32(prompt_feat, self.device) if F > 0 else None
        fl = feat_len.to(device=self.device, dtype=torch.int32).contiguous()
        emb = _f32(embedding, self.device)
        mel = torch.empty(1, spec.N_FEATS, 2 * (P + N - 3), device=self.device)
        ml = torch.empty(1, dtype=torch.int32, device=self.device)
        ts = None
        if t_span is not None:
            ts_host = t_span.detach().to("cpu", torch.float32).contiguous()
            ts = (C.c_float * ts_host.numel())(*ts_host.tolist())
        check(self.lib.jv_flow_token2mel_partial(self._h, _ptr(ptok), _ptr(pl), _ptr(tok), _ptr(tl), _ptr(pf), _ptr(fl), _ptr(emb), P, N,
                                                 F, 1 if streaming else 0, int(n_timesteps), float(temperature), ts, _ptr(mel),
                                                 _ptr(ml), _stream(self.device)))
        return mel, ml

    def flow_encoder_ctx(self, prompt_token, prompt_len, token, token_len, ctx_lens, streaming=False):
        """jv_flow_encoder_fwd_ctx: flow_encoder with a look-ahead context per utterance (ctx_lens [B], each 0 or 3) ->
        (h [B, 2*(P+N), 80], h_lens int32 [B] = 2 (p_b + n_b - ctx_b)); zeros behind"""
        B, N = token.shape
        P = 0 if prompt_token is None else prompt_token.shape[1]
        tok, tl = self._tok(token), self._tok(token_len)
        ptok, pl = (self._tok(prompt_token), self._tok(prompt_len)) if P > 0 else (None, None)
        cl = self._lens32("flow_encoder_ctx", ctx_lens, B)
        h = torch.empty(B, 2 * (P + N), spec.N_FEATS, device=self.device)
        hl = torch.empty(B, dtype=torch.int32, device=self.device)
        check(self.lib.jv_flow_encoder_fwd_ctx(self._h, _ptr(ptok), _ptr(pl), _ptr(tok), _ptr(tl), _ptr(cl), B, P, N,
                                               1 if streaming else 0, _ptr(h), _ptr(hl), _stream(self.device)))
        return h, hl

    def upsample_encoder_tap(self, mode, prompt_token, prompt_len, token, token_len, tap, streaming=False, ctx_lens=None, out=None):
        """jv_upsample_encoder_tap: the launches of prompt_encoder ("prompt": prompt_token None), flow_encoder ("flow"),
        flow_encoder_partial ("partial") or flow_encoder_ctx ("ctx", with ctx_lens) up to and including the stage `tap` (a name of
        _lib.UPS_TAPS), that stage's buffer as [B, C, rate (P + N)] with zeros at and behind every utterance's live length -- for the
        tables of _lib.UPS_TABLES [2T - 1, 512], T = rate x the encoded width (P + N, "partial": P + N - 3).  (tap as a raw id, or
        `out` given: passed on as they are -- the library rejects an id it does not know and a buffer that is too small)"""
        B, N = token.shape
        P = 0 if prompt_token is None else prompt_token.shape[1]
        tok, tl = self._tok(token), self._tok(token_len)
        ptok, pl = (self._tok(prompt_token), self._tok(prompt_len)) if P > 0 else (None, None)
        cl = None if ctx_lens is None else self._lens32("upsample_encoder_tap", ctx_lens, B)
        tap_id, C_, rate = _lib.UPS_TAPS[tap] if isinstance(tap, str) else (int(tap), 1, 1)
        if out is None:
            T = rate * (P + N - (3 if mode == "partial" else 0))
            out = (torch.empty(2 * T - 1, 512, device=self.device) if tap in _lib.UPS_TABLES
                   else torch.empty(B, C_, rate * (P + N), device=self.device))
        check(self.lib.jv_upsample_encoder_tap(self._h, _lib.UPS_MODES[mode] if isinstance(mode, str) else int(mode), _ptr(ptok),
                                               _ptr(pl), _ptr(tok), _ptr(tl), _ptr(cl), B, P, N, 1 if streaming else 0, tap_id,
                                               _ptr(out), out.numel(), _stream(self.device)))
        return out

    def flow_token2mel_ctx(self, prompt_token, prompt_len, token, token_len, ctx_lens, prompt_feat, feat_len, embedding,
                           streaming=False, n_timesteps=10, temperature=1.0, t_span=None):
        """jv_flow_token2mel_ctx: flow_token2mel with a look-ahead context per utterance (ctx_lens [B], each 0 or 3) ->
        (mel [B, 80, 2*(P+N)], mel_lens int32 [B] = 2 (p_b + n_b - ctx_b) - f_b)"""
        B, N = token.shape
        P = 0 if prompt_token is None else prompt_token.shape[1]
        F = 0 if prompt_feat is None else prompt_feat.shape[1]
        tok, tl = self._tok(token), self._tok(token_len)
        ptok, pl = (self._tok(prompt_token), self._tok(prompt_len)) if P > 0 else (None, None)
        cl = self._lens32("flow_token2mel_ctx", ctx_lens, B)
        pf = _f32(prompt_feat, self.device) if F > 0 else None
        fl = feat_len.to(device=self.device, dtype=torch.int32).contiguous()
        emb = _f32(embedding, self.device)
        mel = torch.empty(B, spec.N_FEATS, 2 * (P + N), device=self.device)
        ml = torch.empty(B, dtype=torch.int32, device=self.device)
        ts = None
        if t_span is not None:
            ts_host = t_span.detach().to("cpu", torch.float32).contiguous()
            ts = (C.c_float * ts_host.numel())(*ts_host.tolist())
        check(self.lib.jv_flow_token2mel_ctx(self._h, _ptr(ptok), _ptr(pl), _ptr(tok), _ptr(tl), _ptr(cl), _ptr(pf), _ptr(fl), _ptr(emb),
                                             B, P, N, F, 1 if streaming else 0, int(n_timesteps), float(temperature), ts, _ptr(mel),
                                             _ptr(ml), _stream(self.device)))
        return mel, ml

    # ---- encoder --------------------------------------------------------------------------------------
    ENC_ATTENTION = {"auto": 0, "fused": 1, "gemm": 2}      # JV_ENC_ATTN_AUTO / _FUSED / _GEMM
    encoder_attention = "auto"                              # what set_encoder_attention() left on this context

    def set_encoder_attention(self, mode: str = "auto"):
        """the route of the text encoder's attention (jv_encoder_set_attention).  "auto" (default): four launches around a
        [B, 2, Tt, Tt] score buffer up to 512 tokens, the one-launch online-softmax kernel (encattn.hip) above; "fused": that kernel
        at every length; "gemm": the four launches, and texts beyond 512 tokens raise JvError.  Another name raises ValueError
        and leaves the mode as it was."""
        if mode not in self.ENC_ATTENTION:
            raise ValueError(f"encoder attention must be one of {sorted(self.ENC_ATTENTION)}, not {mode!r}")
        check(self.lib.jv_encoder_set_attention(self._h, self.ENC_ATTENTION[mode]))
        self.encoder_attention = mode

    def encoder(self, x, x_lengths, lang, tone, word_pos, syllable_pos, spk_embed):
        B, Tt = x.shape
        ids = [v.to(device=self.device, dtype=torch.int64).contiguous() for v in (x, lang, tone, word_pos, syllable_pos)]
        xl = x_lengths.to(device=self.device, dtype=torch.int64).contiguous()
        spk = _f32(spk_embed, self.device)
        h = torch.empty(B, spec.ENC_HIDDEN, Tt, device=self.device)
        mu_x = torch.empty(B, spec.N_FEATS, Tt, device=self.device)
        logw = torch.empty(B, 1, Tt, device=self.device)
        c = torch.empty(B, spec.N_FEATS, device=self.device)
        check(self.lib.jv_encoder_fwd(self._h, *[_ptr(v) for v in ids], _ptr(xl), _ptr(spk), B, Tt, _ptr(h), _ptr(mu_x),
                                      _ptr(logw), _ptr(c), _stream(self.device)))
        return h, mu_x, logw, c

    def encoder_tap(self, x, x_lengths, lang, tone, word_pos, syllable_pos, spk_embed, tap, out=None):
        """jv_encoder_fwd_tap: encoder()'s own launches up to and including the stage `tap` (a name of _lib.ENC_TAPS), that stage's
        buffer as [B, C, Tt]: zeros at and behind every utterance's length.  (tap as a raw id, or `out` given: passed on as they
        are -- the library rejects an id it does not know and a buffer that is too small)"""
        B, Tt = x.shape
        ids = [v.to(device=self.device, dtype=torch.int64).contiguous() for v in (x, lang, tone, word_pos, syllable_pos)]
        xl = x_lengths.to(device=self.device, dtype=torch.int64).contiguous()
        spk = _f32(spk_embed, self.device)
        tap_id, C = _lib.ENC_TAPS[tap] if isinstance(tap, str) else (int(tap), 1)
        if out is None:
            out = torch.empty(B, C, Tt, device=self.device)
        h = torch.empty(B, spec.ENC_HIDDEN, Tt, device=self.device)      # (scratch: the call returns ahead of some or all of the outputs)
        mu_x = torch.empty(B, spec.N_FEATS, Tt, device=self.device)
        logw = torch.empty(B, 1, Tt, device=self.device)
        c = torch.empty(B, spec.N_FEATS, device=self.device)
        check(self.lib.jv_encoder_fwd_tap(self._h, *[_ptr(v) for v in ids], _ptr(xl), _ptr(spk), B, Tt, _ptr(h), _ptr(mu_x),
                                          _ptr(logw), _ptr(c), tap_id, _ptr(out), out.numel(), _stream(self.device)))
        return out

    def length_regulate(self, logw, x_lengths, mu_x, length_scale=1.0, host_lengths=False):
        """host_lengths: also leave y_lengths as a list of ints in self.y_lengths_host (the voice-cloning batch sizes its
        workspace by max(p_b + y_b) without a synchronisation of its own)"""
        B, _, Tt = logw.shape
        xl = x_lengths.to(device=self.device, dtype=torch.int64).contiguous()
        w_ceil = torch.empty(B, 1, Tt, device=self.device)
        y_lengths = torch.empty(B, dtype=torch.int64, device=self.device)
        st = _stream(self.device)
        check(self.lib.jv_length_regulate(self._h, _ptr(logw), _ptr(xl), _ptr(mu_x), B, Tt, float(length_scale), _ptr(w_ceil),
                                          _ptr(y_lengths), 0, None, None, st))
        if host_lengths:      # the same one host sync, all B lengths instead of their maximum
            self.y_lengths_host = y_lengths.tolist()
            ty = int(max(self.y_lengths_host))
        else:
            ty = int(y_lengths.max().item())       # the reference's one host sync (jyutvoice_tts.py:187)
        attn = torch.empty(B, Tt, ty, device=self.device)
        mu_y = torch.empty(B, spec.N_FEATS, ty, device=self.device)
        check(self.lib.jv_length_regulate(self._h, _ptr(logw), _ptr(xl), _ptr(mu_x), B, Tt, float(length_scale), _ptr(w_ceil),
                                          _ptr(y_lengths), ty, _ptr(attn), _ptr(mu_y), st))
        return w_ceil, y_lengths, attn, mu_y

    # ---- evaluation forward(): alignment search and losses ------------------------------------------------
    def _lens32(self, who, lens, B):
        v = lens.to(device=self.device, dtype=torch.int32).contiguous()
        if tuple(v.shape) != (B,):
            raise ValueError(f"{who}: lengths must have shape [{B}], got {tuple(v.shape)}")
        return v

    def log_prior(self, mu_x, h, x_lens, y_lens):
        """jv_log_prior (jyutvoice_tts.py:306-314): mu_x [B,80,Tx], h [B,Ty,80] -> log_prior [B,Tx,Ty], zeros outside the utterance"""
        mu_x, h = _f32(mu_x, self.device), _f32(h, self.device)
        B, _, Tx = mu_x.shape
        Ty = h.shape[1]
        xl, yl = self._lens32("log_prior", x_lens, B), self._lens32("log_prior", y_lens, B)
        out = torch.empty(B, Tx, Ty, device=self.device)
        check(self.lib.jv_log_prior(self._h, _ptr(mu_x), _ptr(h), _ptr(xl), _ptr(yl), B, Tx, Ty, _ptr(out), _stream(self.device)))
        return out

    def maximum_path(self, value, x_lens, y_lens):
        """jv_maximum_path (monotonic_align/core.pyx): value [B,Tx,Ty] scores -> (attn fp32 [B,Tx,Ty] one-hot, frame_index int32
        [B,Ty], -1 behind y_lens; durations int32 [B,Tx]).  What lies behind the lengths is not read."""
        value = _f32(value, self.device)
        B, Tx, Ty = value.shape
        xl, yl = self._lens32("maximum_path", x_lens, B), self._lens32("maximum_path", y_lens, B)
        attn = torch.empty(B, Tx, Ty, device=self.device)
        fi = torch.empty(B, Ty, dtype=torch.int32, device=self.device)
        dur = torch.empty(B, Tx, dtype=torch.int32, device=self.device)
        check(self.lib.jv_maximum_path(self._h, _ptr(value), _ptr(xl), _ptr(yl), B, Tx, Ty, _ptr(attn), _ptr(fi), _ptr(dur),
                                       _stream(self.device)))
        return attn, fi, dur

    def align(self, mu_x, h, x_lens, y_lens, want_log_prior=False, want_attn=True):
        """jv_align: prior + search from mu_x [B,80,Tx] and h [B,Ty,80] -> (attn, frame_index, durations, log_prior or None)"""
        mu_x, h = _f32(mu_x, self.device), _f32(h, self.device)
        B, _, Tx = mu_x.shape
        Ty = h.shape[1]
        xl, yl = self._lens32("align", x_lens, B), self._lens32("align", y_lens, B)
        lp = torch.empty(B, Tx, Ty, device=self.device) if want_log_prior else None
        attn = torch.empty(B, Tx, Ty, device=self.device) if want_attn else None
        fi = torch.empty(B, Ty, dtype=torch.int32, device=self.device)
        dur = torch.empty(B, Tx, dtype=torch.int32, device=self.device)
        check(self.lib.jv_align(self._h, _ptr(mu_x), _ptr(h), _ptr(xl), _ptr(yl), B, Tx, Ty, _ptr(lp), _ptr(attn), _ptr(fi), _ptr(dur),
                                _stream(self.device)))
        return attn, fi, dur, lp

    def align_losses(self, logw, durations, x_lens, mu_x, h, frame_index, y_lens):
        """jv_align_losses -> (dur_loss, prior_loss: 0-d device tensors; mu_y [B,80,Ty])"""
        logw, mu_x, h = _f32(logw, self.device), _f32(mu_x, self.device), _f32(h, self.device)
        B, _, Tx = mu_x.shape
        Ty = h.shape[1]
        xl, yl = self._lens32("align_losses", x_lens, B), self._lens32("align_losses", y_lens, B)
        mu_y = torch.empty(B, spec.N_FEATS, Ty, device=self.device)
        losses = torch.empty(2, device=self.device)
        check(self.lib.jv_align_losses(self._h, _ptr(logw), _ptr(durations), _ptr(xl), _ptr(mu_x), _ptr(h), _ptr(frame_index), _ptr(yl),
                                       B, Tx, Ty, _ptr(mu_y), C.c_void_p(losses.data_ptr()), C.c_void_p(losses.data_ptr() + 4),
                                       _stream(self.device)))
        return losses[0], losses[1], mu_y

    def cfm_loss_inputs(self, x1, z, t, cfg_mask, cond_index, mu_y, spks):
        """jv_cfm_loss_inputs: t [B] already warped, cfg_mask [B] (0 / 1), cond_index [B] -> (y_t, u, mu_masked, spks_masked, cond)"""
        x1, z, mu_y, spks = (_f32(v, self.device) for v in (x1, z, mu_y, spks))
        t, m = _f32(t, self.device), _f32(cfg_mask, self.device)
        B, _, T = x1.shape
        k = self._lens32("cfm_loss_inputs", cond_index, B)
        y_t, u, mu_m, cond = (torch.empty_like(x1) for _ in range(4))
        spks_m = torch.empty_like(spks)
        check(self.lib.jv_cfm_loss_inputs(self._h, _ptr(x1), _ptr(z), _ptr(t), _ptr(m), _ptr(k), _ptr(mu_y), _ptr(spks), B, T, _ptr(y_t),
                                          _ptr(u), _ptr(mu_m), _ptr(spks_m), _ptr(cond), _stream(self.device)))
        return y_t, u, mu_m, spks_m, cond

    def masked_mse(self, a, b, lens):
        """jv_masked_mse: sum(((a - b) * mask)^2) / (sum(mask) * C) over [B,C,T] -> a 0-d device tensor"""
        a, b = _f32(a, self.device), _f32(b, self.device)
        B, Cc, T = a.shape
        ln = self._lens32("masked_mse", lens, B)
        out = torch.empty(1, device=self.device)
        check(self.lib.jv_masked_mse(self._h, _ptr(a), _ptr(b), _ptr(ln), B, Cc, T, _ptr(out), _stream(self.device)))
        return out[0]

    # ---- HiFT -----------------------------------------------------------------------------------------
    def hift_f0(self, mel, lens=None):
        B, _, T = mel.shape
        mel = _f32(mel, self.device)
        lens_d = None if lens is None else lens.to(device=self.device, dtype=torch.int32).contiguous()
        f0 = torch.empty(B, T, device=self.device)
        check(self.lib.jv_hift_f0(self._h, _ptr(mel), _ptr(lens_d), B, T, _ptr(f0), _stream(self.device)))
        return f0

    def hift_source(self, f0, phase, noise):
        B, T = f0.shape
        f0, phase, noise = _f32(f0, self.device), _f32(phase, self.device), _f32(noise, self.device)
        s = torch.empty(B, 1, T * spec.HIFT_UPSAMPLE_TOTAL, device=self.device)
        check(self.lib.jv_hift_source(self._h, _ptr(f0), _ptr(phase), _ptr(noise), B, T, _ptr(s), _stream(self.device)))
        return s

    def hift_source_seeded(self, f0, phase, seed: int, call: int):
        """the source signal with its N(0,1) noise drawn inside the kernel from (seed, call) -- no [B,9,480T] noise tensor"""
        B, T = f0.shape
        f0, phase = _f32(f0, self.device), _f32(phase, self.device)
        s = torch.empty(B, 1, T * spec.HIFT_UPSAMPLE_TOTAL, device=self.device)
        check(self.lib.jv_hift_source_seeded(self._h, _ptr(f0), _ptr(phase), C.c_uint64(seed & (2 ** 64 - 1)), C.c_uint32(call & 0xFFFFFFFF),
                                             B, T, _ptr(s), _stream(self.device)))
        return s

    def hift_source_cont(self, f0, phase, seed: int, call: int, sample0: int, cum):
        """jv_hift_source_cont: the next 480 T samples of a source signal whose first `sample0` samples came from earlier calls.
        cum: float64 [B, 9] on the device, zeros before the first piece; updated in place on the stream."""
        B, T = f0.shape
        if cum.dtype != torch.float64 or tuple(cum.shape) != (B, 9) or cum.device != self.device or not cum.is_contiguous():
            raise ValueError(f"hift_source_cont(): cum must be a contiguous float64 [{B}, 9] tensor on {self.device}, got "
                             f"{cum.dtype} {tuple(cum.shape)} on {cum.device}")
        if sample0 < 0:
            raise ValueError(f"hift_source_cont(): sample0 must be non-negative, got {sample0}")
        f0, phase = _f32(f0, self.device), _f32(phase, self.device)
        s = torch.empty(B, 1, T * spec.HIFT_UPSAMPLE_TOTAL, device=self.device)
        check(self.lib.jv_hift_source_cont(self._h, _ptr(f0), _ptr(phase), C.c_uint64(seed & (2 ** 64 - 1)), C.c_uint32(call & 0xFFFFFFFF),
                                           C.c_int64(sample0), _ptr(cum), B, T, _ptr(s), _stream(self.device)))
        return s

    def _dev_vec(self, who, name, t, dtype, B):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (B,) or t.device != self.device or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous {dtype} [{B}] tensor on {self.device}, got "
                             f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
        return t

    def hift_source_cont_rows(self, f0, phase, seeds, calls, sample0, lens, cum, out=None):
        """jv_hift_source_cont_rows: every row the continuation of a signal of its own.  f0 [B, T]; phase [B, 9]; seeds int64 [B]
        (the uint64 key's bit pattern), calls int32 [B] (uint32 likewise), sample0 int64 [B], lens int32 [B], cum float64 [B, 9]: all on
        the device, nothing is copied.  -> s [B, 1, 480 T]; a row with lens 0 is not written (with `out` it keeps what it held)."""
        who = "hift_source_cont_rows()"
        B, T = f0.shape
        if cum.dtype != torch.float64 or tuple(cum.shape) != (B, 9) or cum.device != self.device or not cum.is_contiguous():
            raise ValueError(f"{who}: cum must be a contiguous float64 [{B}, 9] tensor on {self.device}, got "
                             f"{cum.dtype} {tuple(cum.shape)} on {cum.device}")
        seeds = self._dev_vec(who, "seeds", seeds, torch.int64, B)
        calls = self._dev_vec(who, "calls", calls, torch.int32, B)
        sample0 = self._dev_vec(who, "sample0", sample0, torch.int64, B)
        lens = self._dev_vec(who, "lens", lens, torch.int32, B)
        f0, phase = _f32(f0, self.device), _f32(phase, self.device)
        if tuple(phase.shape) != (B, 9):
            raise ValueError(f"{who}: phase must be [{B}, 9], got {tuple(phase.shape)}")
        n = T * spec.HIFT_UPSAMPLE_TOTAL
        if out is None:
            out = torch.zeros(B, 1, n, device=self.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (B, 1, n) or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"{who}: out must be a contiguous float32 [{B}, 1, {n}] tensor on {self.device}")
        check(self.lib.jv_hift_source_cont_rows(self._h, _ptr(f0), _ptr(phase), _ptr(seeds), _ptr(calls), _ptr(sample0), _ptr(lens),
                                                _ptr(cum), B, T, _ptr(out), _stream(self.device)))
        return out

    def slab_copy(self, src, dst, desc, span: int, zero_fill: bool = False):
        """jv_slab_copy: src [rows, C, width], dst [rows', C, width'] (or 2-D, C = 1): contiguous float32 on the device; desc int32
        [B, 5] on the device, rows of (src_row, src_col, dst_row, dst_col, n); span: the widest slab (with zero_fill: every slab's
        destination is zeros from n up to span).  One launch, in place on `dst`."""
        who = "slab_copy()"
        for name, t in (("src", src), ("dst", dst)):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() not in (2, 3) or t.device != self.device
                    or not t.is_contiguous()):
                raise ValueError(f"{who}: {name} must be a contiguous float32 [rows, C, width] or [rows, width] tensor on {self.device}")
        cs, cd = (1 if src.dim() == 2 else src.shape[1]), (1 if dst.dim() == 2 else dst.shape[1])
        if cs != cd:
            raise ValueError(f"{who}: src has {cs} channels, dst {cd}")
        if (not isinstance(desc, torch.Tensor) or desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != 5
                or desc.device != self.device or not desc.is_contiguous()):
            raise ValueError(f"{who}: desc must be a contiguous int32 [B, 5] tensor on {self.device}")
        if span < 0:
            raise ValueError(f"{who}: span must be non-negative, got {span}")
        if src.numel() == 0 or dst.numel() == 0 or desc.shape[0] == 0 or span == 0:
            return dst
        check(self.lib.jv_slab_copy(self._h, _ptr(src), src.shape[0], src.shape[-1], _ptr(dst), dst.shape[0], dst.shape[-1], cs,
                                    _ptr(desc), desc.shape[0], int(span), 1 if zero_fill else 0, _stream(self.device)))
        return dst

    def hift_decode(self, mel, s, lens=None):
        B, _, T = mel.shape
        mel, s = _f32(mel, self.device), _f32(s, self.device)
        lens_d = None if lens is None else lens.to(device=self.device, dtype=torch.int32).contiguous()
        wav = torch.empty(B, T * spec.HIFT_UPSAMPLE_TOTAL, device=self.device)
        check(self.lib.jv_hift_decode(self._h, _ptr(mel), _ptr(s), _ptr(lens_d), B, T, _ptr(wav), _stream(self.device)))
        return wav

    def hift_decode_tap(self, mel, s, lens, tap, out=None):
        """jv_hift_decode_tap: hift_decode's own launches up to and including the stage `tap` (a name of _lib.HIFT_TAPS), that
        stage's buffer as [B, C, L]: zeros at and behind every utterance's length.  (tap as a raw id, or `out` given: passed on as
        they are -- the library rejects an id it does not know and a buffer that is too small)"""
        B, _, T = mel.shape
        mel, s = _f32(mel, self.device), _f32(s, self.device)
        lens_d = None if lens is None else lens.to(device=self.device, dtype=torch.int32).contiguous()
        tap_id = _lib.HIFT_TAPS[tap][0] if isinstance(tap, str) else int(tap)
        if out is None:
            _, C, mul, add = _lib.HIFT_TAPS[tap] if isinstance(tap, str) else (0, 1, 0, 1)
            out = torch.empty(B, C, T * mul + add, device=self.device)
        check(self.lib.jv_hift_decode_tap(self._h, _ptr(mel), _ptr(s), _ptr(lens_d), B, T, tap_id, _ptr(out), out.numel(),
                                          _stream(self.device)))
        return out


# ---- operator-level helpers for the parity tests (same kernels the stages launch) ------------------------
def op_conv_gemm(A, W, bias=None, ntaps=1, tap_row0=0, dil=1, M=None, act="none", prologue="none", alpha=None, slope=0.0,
                 ln=None, ln_eps=1e-5, rowmask=None, res=None):
    """A [rows, Cin] cuda fp32; W [N, ntaps*Cin]; returns out [M, N]."""
    lib = _lib.load()
    rows, cin = A.shape
    N = W.shape[0]
    M = rows if M is None else M
    out = torch.empty(M, N, device=A.device)
    g, b = (ln if ln is not None else (None, None))
    check(lib.jv_op_conv_gemm(_ptr(A), rows, M, cin, ntaps, tap_row0, dil, _ptr(W), N, _ptr(bias), _lib.ACT[act],
                              _lib.PRO[prologue], _ptr(alpha), float(slope), _ptr(g), _ptr(b), float(ln_eps), _ptr(rowmask),
                              _ptr(res), _ptr(out), _stream(A.device)))
    return out


def op_set_products(np: int = 3) -> None:
    """process-wide: fp16x3 products per step of the op_* hooks below (jv_op_set_products) -- 3, or 1 = the hi x hi product alone,
    what Engine.set_precision("fp16") selects on a context.  Nothing on the production path reads it."""
    check(_lib.load().jv_op_set_products(int(np)))


def op_linear_h3(A, W, bias=None, act="none", res=None, a_bound=None, presplit=0):
    """fp16x3 main loop (jv_flow_set_contraction): A [rows, K], W [N, K]; a_bound >= max |A| (default: measured);
    presplit=1: A goes through fp16 planes and LDS-DMA as in the estimator (2: reuse the previous planes, timing only)."""
    lib = _lib.load()
    rows, K = A.shape
    N = W.shape[0]
    out = torch.empty(rows, N, device=A.device)
    bound = float(A.abs().max()) if a_bound is None else float(a_bound)
    check(lib.jv_op_linear_h3(_ptr(A), rows, rows, K, _ptr(W), N, _ptr(bias), _lib.ACT[act], _ptr(res), bound, int(presplit),
                              _ptr(out), _stream(A.device)))
    return out


def op_attention(qkv, lens, B, G, S, L):
    lib = _lib.load()
    out = torch.zeros(qkv.shape[0], 512, device=qkv.device)
    check(lib.jv_op_attention(_ptr(qkv), _ptr(lens), B, G, S, L, _ptr(out), _stream(qkv.device)))
    return out


def op_rel_attention(qkv, p, u, v, lens, B, T, G, S, len_mul=1, chunk=0, fused=True):
    """the conformer block's relative-position attention (jv_op_rel_attention): qkv [rows, 1536] (rows G + b*S + t), p [2T-1, 512],
    u, v [8, 64], lens int64 [B] -> out [rows, 512]; fused: relattn.hip's one launch, else the three-GEMM sequence.  Rows the
    call does not own come back NaN."""
    lib = _lib.load()
    out = torch.full((qkv.shape[0], 512), float("nan"), device=qkv.device)
    lens = lens.to(device=qkv.device, dtype=torch.int64).contiguous()
    check(lib.jv_op_rel_attention(_ptr(qkv), _ptr(p), _ptr(u), _ptr(v), _ptr(lens), int(B), int(T), int(G), int(S), int(len_mul),
                                  int(chunk), 1 if fused else 0, _ptr(out), _stream(qkv.device)))
    return out


def op_enc_attention(qkv, lens, B, T, G, S, fused=True):
    """the text encoder's attention (jv_op_enc_attention): qkv [rows, 1728] (rows G + b*S + t; q | k | v, 2 heads of 288 each, RoPE
    applied), lens int64 [B] -> out [rows, 576]; fused: encattn.hip's one launch (rows at and behind a length are zeros), else the
    four-launch sequence (T <= 512; those rows hold an average of V).  Rows the call does not own come back NaN."""
    lib = _lib.load()
    out = torch.full((qkv.shape[0], 576), float("nan"), device=qkv.device)
    lens = lens.to(device=qkv.device, dtype=torch.int64).contiguous()
    check(lib.jv_op_enc_attention(_ptr(qkv), _ptr(lens), int(B), int(T), int(G), int(S), 1 if fused else 0, _ptr(out),
                                  _stream(qkv.device)))
    return out


def op_conv_h3_measured(A, W, bias=None, ntaps=1, tap_row0=0, dil=1, M=None, act="none", prologue="none", alpha=None,
                        slope=0.0, rowmask=None, res=None, amax_in=None, a_extra=0.0, amax_out=None):
    """conv_gemm with the fp16x3 scale derived on the device from amax_in (a 1-element cuda tensor >= max |A|) + a_extra;
    amax_out (1-element cuda tensor, zeroed by the caller) receives max |out|.  amax_in=None: bf16x6, tracking only."""
    lib = _lib.load()
    rows, cin = A.shape
    N = W.shape[0]
    M = rows if M is None else M
    out = torch.empty(M, N, device=A.device)
    check(lib.jv_op_conv_h3_measured(_ptr(A), rows, M, cin, ntaps, tap_row0, dil, _ptr(W), N, _ptr(bias), _lib.ACT[act],
                                     _lib.PRO[prologue], _ptr(alpha), float(slope), _ptr(rowmask), _ptr(res), _ptr(amax_in),
                                     float(a_extra), _ptr(amax_out), _ptr(out), _stream(A.device)))
    return out


def op_splitk(A, W, bias=None, M=None, ntaps=1, tap_row0=0, ln=None, act="none", rowmask=None, rowvec=None, row_sample=None,
              rowvec_ld=0, res=None, out=None, ln2=None, out2=None, ksplit_max=8, mode=0, amax_in=None, a_bound=0.0,
              slots=(0, 0, 1), amax_out=None):
    """the estimator's short-batch route (jv_op_splitk): split-K tiles + the row-wise reduce tail, through the launcher the
    estimator calls.  A [rows, Cin], W [256, ntaps * Cin]; ln / ln2 = (gain, offset); rowmask uint8 [rows] and row_sample int32 [rows];
    res and out: row-major views whose row strides become ldr / ldo (res may be out: in place; out may be the right half of a
    [rows, 512] buffer); mode 0 bf16x6, 1 fp16x3 from amax_in [nb] with slots = (G, S, nb) (S < 0: through row_sample), 2 fp16x3 from
    a_bound.  -> (out, out2); buffers allocated here come back NaN outside the M rows the launch owns."""
    lib = _lib.load()
    rows, cin = A.shape
    N = W.shape[0]
    M = rows if M is None else M
    if out is None:
        out = torch.full((rows, 256), float("nan"), device=A.device)
    g, b = (ln if ln is not None else (None, None))
    g2, b2 = (ln2 if ln2 is not None else (None, None))
    if ln2 is not None and out2 is None:
        out2 = torch.full((rows, 256), float("nan"), device=A.device)
    for t in (out, res):
        if t is not None and (t.dim() != 2 or t.stride(1) != 1 or t.shape[1] < 256):
            raise ValueError("op_splitk: out and res are row-major [rows, >= 256] views")
    G, S, nb = slots
    check(lib.jv_op_splitk(_ptr(A), rows, M, cin, ntaps, tap_row0, _ptr(W), N, _ptr(bias), _ptr(g), _ptr(b), _lib.ACT[act],
                           _ptr(rowmask), _ptr(rowvec), _ptr(row_sample), int(rowvec_ld), _ptr(res),
                           0 if res is None else res.stride(0), _ptr(out), out.stride(0), _ptr(g2), _ptr(b2), _ptr(out2),
                           int(ksplit_max), int(mode), _ptr(amax_in), float(a_bound), int(G), int(S), int(nb), _ptr(amax_out),
                           _stream(A.device)))
    return out, out2


def op_attention_h3(qkv, lens, B, G, S, L, bounds=None):
    """fp16x3 attention kernel; bounds = (|q|, |k|, |v|) maxima the caller vouches for (default: measured)"""
    lib = _lib.load()
    out = torch.zeros(qkv.shape[0], 512, device=qkv.device)
    if bounds is None:
        bounds = tuple(float(qkv[:, o:o + 512].abs().max()) for o in (0, 512, 1024))
    check(lib.jv_op_attention_h3(_ptr(qkv), _ptr(lens), B, G, S, L, float(bounds[0]), float(bounds[1]), float(bounds[2]),
                                 _ptr(out), _stream(qkv.device)))
    return out


def op_rowgemm(A, W, bias=None, epi="plain", res=None, ln=None, a_bound=None, out2_scale=1.0, presplit=0, amax_out=None):
    """the row-owning fp16x3 GEMM (rowgemm_kernel.h): returns out fp32 [M,N] (plain / res), the fp16 planes as an fp32
    tensor h + l (gelu), or (out, planes) for res+ln.  Planes come back un-scaled (divided by out2_scale)."""
    lib = _lib.load()
    rows, K = A.shape
    N = W.shape[0]
    code = {"plain": 0, "gelu": 1, "res": 2, "res_ln": 3}[epi]
    bound = float(A.abs().max()) if a_bound is None else float(a_bound)
    out = torch.empty(rows, N, device=A.device) if code != 1 else None
    pc = 256 if code == 3 else N
    out2 = torch.empty(2, rows, pc, dtype=torch.float16, device=A.device) if code in (1, 3) else None
    g, b = (ln if ln is not None else (None, None))
    check(lib.jv_op_rowgemm(_ptr(A), rows, rows, K, _ptr(W), N, _ptr(bias), code, _ptr(res), _ptr(g), _ptr(b), bound,
                            float(out2_scale), int(presplit), _ptr(out), _ptr(out2), _ptr(amax_out), _stream(A.device)))
    if presplit == 2:      # timing call: no post-processing
        return out
    planes = None if out2 is None else (out2[0].double() + out2[1].double()) / out2_scale
    if code == 1:
        return planes
    return (out, planes) if code == 3 else out


def op_attention_planes(qkv, lens, B, G, S, L, bounds=None, chunk=0, planes_out=False, out2_scale=256.0):
    """attention_pl.hip (K / V as fp16 planes by LDS-DMA); planes_out: the result through the fp16-plane output path, returned
    un-scaled as fp64"""
    lib = _lib.load()
    rows = qkv.shape[0]
    if bounds is None:
        bounds = tuple(float(qkv[:, o:o + 512].abs().max()) for o in (0, 512, 1024))
    out = torch.zeros(rows, 512, device=qkv.device)
    out2 = torch.zeros(2, rows, 512, dtype=torch.float16, device=qkv.device) if planes_out else None
    check(lib.jv_op_attention_planes(_ptr(qkv), rows, _ptr(lens), B, G, S, L, float(bounds[0]), float(bounds[1]), float(bounds[2]),
                                     int(chunk), float(out2_scale), _ptr(out), _ptr(out2), _stream(qkv.device)))
    if planes_out:
        return (out2[0].double() + out2[1].double()) / out2_scale
    return out


def op_rowconv(A, W, bias=None, ln=None, act="none", rowmask=None, rowvec=None, res=None, amax_in=None, amax_out=None):
    """rowconv_kernel.h: causal k = 3 conv to 256 channels + LayerNorm / act / mask / + rowvec / + res; W [256, 3 * Cin]"""
    lib = _lib.load()
    rows, cin = A.shape
    out = torch.empty(rows, 256, device=A.device)
    g, b = (ln if ln is not None else (None, None))
    if amax_in is None:
        amax_in = A.abs().max().reshape(1)
    check(lib.jv_op_rowconv(_ptr(A), rows, rows, cin, _ptr(W), _ptr(bias), _ptr(g), _ptr(b), _lib.ACT[act], _ptr(rowmask),
                            _ptr(rowvec), _ptr(res), _ptr(amax_in), _ptr(amax_out), _ptr(out), _stream(A.device)))
    return out


def op_hiftconv(A, W, bias, alpha, ntaps, dil, rowmask=None, res1=None, res2=None, out_scale=1.0, prev=None, amax_out=None,
                amax_in=None, slots=None):
    """hiftconv_kernel.h: the vocoder's ResBlock convolution on a [rows, C] row buffer (C = 64 / 128 / 256); W [C, ntaps * C]
    tap-major; prev: accumulate onto this tensor.  amax_in: per-utterance bounds of A with slots = (G, S, nb) or an int32 [rows]
    row -> utterance table (op_hiftpair's); both None: one slot for every row, its bound measured here"""
    lib = _lib.load()
    rows, C = A.shape
    out = prev.clone() if prev is not None else torch.empty(rows, C, device=A.device)
    if amax_in is None:
        masked = A if rowmask is None else A * rowmask[:, None].to(A.dtype)
        amax_in = torch.nan_to_num(masked).abs().max().reshape(1)
    table = slots if torch.is_tensor(slots) else None
    G, S, nb = (0, 0, int(amax_in.numel())) if (table is not None or slots is None) else slots
    extra = float((1.0 / (alpha + 1e-9)).max())
    check(lib.jv_op_hiftconv(_ptr(A), rows, C, int(ntaps), int(dil), _ptr(W), _ptr(bias), _ptr(alpha), _ptr(rowmask), _ptr(res1),
                             _ptr(res2), float(out_scale), 1 if prev is not None else 0, _ptr(amax_in), extra, int(G), int(S), int(nb),
                             _ptr(table), _ptr(amax_out), _ptr(out), _stream(A.device)))
    return out


# ---- the fused row-owning launches (tests/test_gpu_fused_ops.py).  Plane outputs come back un-scaled, as fp64 (h + l) / scale ------
def h3_scale(bound: float) -> float:
    """the power of two the library scales a tensor bounded by `bound` with (registry.hip h3_scale_for_bound)"""
    return float(_lib.load().jv_h3_scale_for_bound(float(bound)))


def _unscale(planes, scale):
    return (planes[0].double() + planes[1].double()) / scale


def _unscale_kv(kv2, k_bound, v_bound):
    kv = kv2[0].double() + kv2[1].double()
    return kv[:, :512] / h3_scale(k_bound), kv[:, 512:] / h3_scale(v_bound)


def op_rowgemm_qkv(A, W, a_bound, k_bound, v_bound, M=None, nsplit=0, rt=0, planes=None):
    """rowgemm's q | k | v epilogue: A [rows, K] fp32 (or planes=[2, rows, K] fp16 of A * h3_scale(a_bound), A then None),
    W [1536, K] -> (q fp32 [rows, 512], k, v fp64 [rows, 512], kv2 the raw planes).  Rows >= M are left as allocated (NaN)."""
    lib = _lib.load()
    src = A if planes is None else planes
    rows, K = src.shape[-2], src.shape[-1]
    M = rows if M is None else M
    q = torch.full((rows, 512), float("nan"), device=src.device)
    kv2 = torch.full((2, rows, 1024), float("nan"), dtype=torch.float16, device=src.device)
    check(lib.jv_op_rowgemm_qkv(_ptr(A if planes is None else None), _ptr(planes), rows, M, K, _ptr(W), float(a_bound), float(k_bound),
                                float(v_bound), int(nsplit), int(rt), _ptr(q), _ptr(kv2), _stream(src.device)))
    k, v = _unscale_kv(kv2, k_bound, v_bound)
    return q, k, v, kv2


def op_rowres(x, M, rowmask, amax_in, slots, w, lnf=None, lnf_bound=0.0, Wq=None, k_bound=0.0, v_bound=0.0, amax_out=None, out=None):
    """rowres_kernel.h through jv_op_rowres.  x [rows, Cin]; slots = (G, S, nb) or an int32 [rows] row -> utterance table (the
    compact addressing); w: dict W1 b1 ln1_g ln1_b Wr br temb W2 b2 ln2_g ln2_b; lnf = (g, b): the following LayerNorm1 -> planes
    (Wq None) or q | k | v.  Returns dict(out, lnf (fp64, un-scaled), lnf_planes (raw), q, k, v)."""
    lib = _lib.load()
    rows, cin = x.shape
    dev = x.device
    if out is None:
        out = torch.full((rows, 256), float("nan"), device=dev)
    table = slots if torch.is_tensor(slots) else None
    G, S, nb = (0, -1, int(amax_in.numel())) if table is not None else slots
    g, b = lnf if lnf is not None else (None, None)
    planes = torch.full((2, rows, 256), float("nan"), dtype=torch.float16, device=dev) if (lnf is not None and Wq is None) else None
    q = torch.full((rows, 512), float("nan"), device=dev) if Wq is not None else None
    kv2 = torch.full((2, rows, 1024), float("nan"), dtype=torch.float16, device=dev) if Wq is not None else None
    check(lib.jv_op_rowres(_ptr(x), rows, int(M), cin, _ptr(rowmask), _ptr(amax_in), int(G), int(S), int(nb), _ptr(table),
                           _ptr(w["W1"]), _ptr(w["b1"]), _ptr(w["ln1_g"]), _ptr(w["ln1_b"]), _ptr(w["Wr"]), _ptr(w["br"]),
                           _ptr(w["temb"]), _ptr(w["W2"]), _ptr(w["b2"]), _ptr(w["ln2_g"]), _ptr(w["ln2_b"]), _ptr(g), _ptr(b),
                           float(lnf_bound), _ptr(planes), _ptr(Wq), float(k_bound), float(v_bound), _ptr(q), _ptr(kv2),
                           _ptr(amax_out), _ptr(out), _stream(dev)))
    res = {"out": out, "lnf_planes": planes, "q": q}
    if planes is not None:
        res["lnf"] = _unscale(planes, h3_scale(lnf_bound))
    if Wq is not None:
        res["k"], res["v"] = _unscale_kv(kv2, k_bound, v_bound)
        res["kv2"] = kv2
    return res


def op_hiftpair(A, W1, b1, alpha1, W2, b2, alpha2, ntaps, dil, amax_in, slots, rowmask=None, res2=None, out_scale=1.0, prev=None,
                amax_out=None, out=None):
    """hiftpair_kernel.h through jv_op_hiftpair: A [rows, C]; W1, W2 [C, ntaps * C] tap-major; slots = (G, S, nb) or an int32
    [rows] row -> utterance table; prev: accumulate onto a copy of this tensor"""
    lib = _lib.load()
    rows, C = A.shape
    if out is None:
        out = prev.clone() if prev is not None else torch.full((rows, C), float("nan"), device=A.device)
    table = slots if torch.is_tensor(slots) else None
    G, S, nb = (0, 0, int(amax_in.numel())) if table is not None else slots
    check(lib.jv_op_hiftpair(_ptr(A), rows, C, int(ntaps), int(dil), _ptr(W1), _ptr(b1), _ptr(alpha1), _ptr(W2), _ptr(b2), _ptr(alpha2),
                             _ptr(rowmask), _ptr(amax_in), int(G), int(S), int(nb), _ptr(table), _ptr(res2), float(out_scale),
                             1 if prev is not None else 0, _ptr(amax_out), _ptr(out), _stream(A.device)))
    return out


def op_rowblock(att, h, M, w, bounds, mode="plain", fused=1, out_ld=None, row_slot=None, row_mask=None, nslots=0):
    """rowblock_kernel.h / rowffn through jv_op_rowblock.  att [rows, 512] (mode "ffn": x [rows, 256], the LayerNorm3 output),
    h [rows, 256] (copied: the caller's tensor is left alone); w: dict Wo bo ln3_g ln3_b W1 b1 W2 b2 (+ ln1_g ln1_b, Wq);
    bounds: dict att ln3 hid ln1 k v; mode "plain" / "ln" / "qkv" / "ffn"; out_ld = 512: out is a separate [rows, 512] buffer
    (columns 0..255 written) instead of h.  Returns dict(h, out, ln, ln_planes, q, k, v, kv2, amax_h, amax_out)."""
    lib = _lib.load()
    dev = att.device
    rows = h.shape[0]
    code = {"plain": 0, "ln": 1, "qkv": 2, "ffn": 3}[mode]
    h = h.clone()
    out = h if out_ld is None else torch.full((rows, out_ld), float("nan"), device=dev)
    follows = code in (1, 2) or (code == 3 and w.get("ln1_g") is not None)
    ln_planes = torch.full((2, rows, 256), float("nan"), dtype=torch.float16, device=dev) if (follows and code != 2) else None
    q = torch.full((rows, 512), float("nan"), device=dev) if code == 2 else None
    kv2 = torch.full((2, rows, 1024), float("nan"), dtype=torch.float16, device=dev) if code == 2 else None
    amax_h = torch.zeros(nslots, device=dev) if nslots else None
    amax_out = torch.zeros(nslots, device=dev) if nslots else None
    B = lambda k: float(bounds.get(k, 0.0))
    P = lambda k: _ptr(w.get(k))
    check(lib.jv_op_rowblock(_ptr(att), _ptr(h), rows, int(M), code, int(fused), B("att"), P("Wo"), P("bo"), P("ln3_g"), P("ln3_b"),
                             B("ln3"), P("W1"), P("b1"), B("hid"), P("W2"), P("b2"), P("ln1_g") if follows else None,
                             P("ln1_b") if follows else None, B("ln1"), P("Wq") if code == 2 else None, B("k"), B("v"), _ptr(out),
                             256 if out_ld is None else int(out_ld), _ptr(ln_planes), _ptr(q), _ptr(kv2), _ptr(amax_h), _ptr(amax_out),
                             _ptr(row_slot), _ptr(row_mask), _stream(dev)))
    res = {"h": h, "out": out, "ln_planes": ln_planes, "q": q, "kv2": kv2, "amax_h": amax_h, "amax_out": amax_out}
    if ln_planes is not None:
        res["ln"] = _unscale(ln_planes, h3_scale(B("ln1")))
    if code == 2:
        res["k"], res["v"] = _unscale_kv(kv2, B("k"), B("v"))
    return res


def op_layernorm(x, g, b, eps=1e-5):
    lib = _lib.load()
    out = torch.empty_like(x)
    check(lib.jv_op_layernorm(_ptr(x), _ptr(g), _ptr(b), float(eps), x.shape[0], x.shape[1], _ptr(out), _stream(x.device)))
    return out


def profile_enable(on: bool) -> None:
    check(_lib.load().jv_profile_enable(1 if on else 0))


def profile_report() -> dict:
    """per-kernel {launches, ms, flops, bytes} since the last report (synchronises the device)"""
    import json
    buf = C.create_string_buffer(1 << 16)
    check(_lib.load().jv_profile_report(buf, len(buf)))
    return json.loads(buf.value.decode())
