"""`JyutVoiceTTS` drop-in for the synthesis path and the evaluation `forward()` (jyutvoice/models/jyutvoice_tts.py:23-364).

Same constructor keywords, `load_state_dict` / `load_pretrain` key names, `synthesise()` signature, defaults,
return-dict keys and `ValueError` for batch != 1 as the reference.  `forward()` has the reference's positional signature and
returns its `(dur_loss, prior_loss, diff_loss, attn)` without gradients: validation losses, forced alignment, durations.
Backward passes, optimisers and the Lightning hooks are out of scope.  All arithmetic runs in libjyutvoice_hip.so; this class
only moves pointers.

Extension (opt-in): `synthesise(..., batched=True)` accepts B > 1 and is defined as looping the batch-1
reference over the utterances (padded frames of shorter utterances are returned as zeros).  With `prompt_lengths` ([B]
integers) every utterance brings a voice prompt of its own length: utterance b is the batch-1 reference called with
`prompt_feat[b:b+1, :p_b]` and `prompt_h[b:b+1, :p_b]` (p_b = 0: no prompt); `utils/prompt.py::pad_prompts` builds the
three tensors from per-utterance lists.
"""
from __future__ import annotations

import datetime as dt
import os
import random
from typing import Dict

import torch

from .. import spec
from ..engine import JV_MODEL_TTS
from ..flow.flow_matching import CausalConditionalCFM, check_scheduler, decoder_settings, resolve_guidance, resolve_solver, time_span
from ..runtime import get_runtime
from .duration_predictor import DurationPredictor
from .text_encoder import TextEncoder


class JyutVoiceTTS:
    def __init__(self, encoder: "TextEncoder", decoder: "CausalConditionalCFM", dp: "DurationPredictor", output_size=80,
                 spk_embed_dim=192, freeze_encoder=False, freeze_decoder=False, optimizer=None, scheduler=None,
                 pretrain_path=None, warmup_steps=100, device="cuda:0"):
        if output_size != spec.N_FEATS or spk_embed_dim != spec.SPK_EMBED_DIM:
            raise NotImplementedError("libjyutvoice_hip is built for output_size=80, spk_embed_dim=192")
        self.encoder, self.decoder, self.dp = encoder, decoder, dp
        self.n_feats = getattr(encoder, "n_feats", spec.N_FEATS)
        self.output_size = output_size
        self.freeze_encoder, self.freeze_decoder = freeze_encoder, freeze_decoder
        self.device = torch.device(device)
        if hasattr(decoder, "device"):
            decoder.device = self.device
        self._loaded = False
        self._sd: Dict[str, torch.Tensor] = {}
        self._missing = list(spec.TTS_INVENTORY)
        if pretrain_path:
            self.load_pretrain(pretrain_path)

    # ---- nn.Module-shaped plumbing used by infer.py:341-346 -----------------------------------------
    def to(self, device):
        self.device = torch.device(device)
        if hasattr(self.decoder, "device"):
            self.decoder.device = self.device
        return self

    def eval(self):
        return self

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        """Same key names / shapes / error text as the reference module.  With strict=False (what `load_pretrain` uses,
        jyutvoice_tts.py:104) keys accumulate across calls -- e.g. CosyVoice2's flow.pt (`decoder.*`,
        `spk_embed_affine_layer.*`) first, a fine-tuned encoder/dp checkpoint later -- and the weights go to the GPU once
        all 1041 tensors are known; until then synthesise() names what is missing (the reference would silently run the
        missing sub-modules with their random initialisation)."""
        missing = [k for k in spec.TTS_INVENTORY if k not in state_dict]
        unexpected = [k for k in state_dict if k not in spec.TTS_INVENTORY]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for JyutVoiceTTS: Missing key(s): {missing[:6]}; "
                               f"Unexpected key(s): {unexpected[:6]}")
        for k, v in state_dict.items():
            if k in spec.TTS_INVENTORY and tuple(v.shape) != tuple(spec.TTS_INVENTORY[k]):
                raise RuntimeError(f"size mismatch for {k}: copying a param with shape {tuple(v.shape)} from checkpoint, "
                                   f"the shape in current model is {tuple(spec.TTS_INVENTORY[k])}.")
        self._sd.update({k: v.detach() for k, v in state_dict.items() if k in spec.TTS_INVENTORY})
        self._missing = [k for k in spec.TTS_INVENTORY if k not in self._sd]
        if not self._missing:
            get_runtime(self.device).set_weights(JV_MODEL_TTS, {k: self._sd[k] for k in spec.TTS_INVENTORY})
            self._loaded = True
        return missing, unexpected

    def load_pretrain(self, pretrain_path):
        if not os.path.exists(pretrain_path):
            raise FileNotFoundError(f"Pretrain checkpoint not found: {pretrain_path}")
        ckpt = torch.load(pretrain_path, map_location="cpu")
        sd = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt
        return self.load_state_dict(sd, strict=False)

    @staticmethod
    def _check_prompt_lengths(prompt_lengths, prompt_feat, prompt_h, B):
        """host-side validation of the voice-cloning batch's arguments; returns the lengths as a list of ints (pass
        prompt_lengths on the host, as pad_prompts returns it: a device tensor costs a synchronisation here)"""
        if prompt_feat is None or prompt_h is None:
            raise ValueError("synthesise(): prompt_lengths needs prompt_feat and prompt_h")
        if not isinstance(prompt_lengths, torch.Tensor) or prompt_lengths.dtype not in (torch.int32, torch.int64):
            raise ValueError("synthesise(): prompt_lengths must be an int32 / int64 tensor, got "
                             f"{getattr(prompt_lengths, 'dtype', type(prompt_lengths).__name__)}")
        if tuple(prompt_lengths.shape) != (B,):
            raise ValueError(f"synthesise(): prompt_lengths must have shape [{B}], got {tuple(prompt_lengths.shape)}")
        for name, t in (("prompt_feat", prompt_feat), ("prompt_h", prompt_h)):
            if t.dim() != 3 or t.shape[0] != B or t.shape[2] != spec.N_FEATS:
                raise ValueError(f"synthesise(): {name} must be [{B}, frames, {spec.N_FEATS}], got {tuple(t.shape)}")
        limit = min(prompt_feat.shape[1], prompt_h.shape[1])
        p_host = prompt_lengths.tolist()
        for b, p in enumerate(p_host):
            if p < 0 or p > limit:
                raise ValueError(f"synthesise(): utterance {b}: prompt length {p} outside [0, {limit}] "
                                 f"(prompt_feat holds {prompt_feat.shape[1]} frames, prompt_h {prompt_h.shape[1]})")
        return p_host

    # ---- the hot path -----------------------------------------------------------------------------------------
    @torch.inference_mode()
    def synthesise(self, x, x_lengths, lang, tone, word_pos, syllable_pos, spk_embed, prompt_feat, prompt_h=None,
                   n_timesteps=10, temperature=1.0, length_scale=1.0, batched=False, prompt_lengths=None, streaming=False,
                   cfg_rate=None, cfg_schedule=None, t_scheduler=None, solver=None):
        """jyutvoice_tts.py:130-253.  Extensions beyond the reference's arguments: batched / prompt_lengths (a batch, one voice
        prompt per utterance); cfg_rate (the guidance rate of this call; None: the decoder's inference_cfg_rate), cfg_schedule (a
        sequence of n_timesteps rates, one per Euler step; wins over cfg_rate) and t_scheduler ("cosine" / "linear"; None: the
        decoder's) -- flow_matching.py:215-265, 387-389; solver ("euler" / "midpoint" / "heun"; None: the decoder's `solver`, "euler"
        unless set) -- n_timesteps second-order steps are 2 n_timesteps estimator evaluations.  The context is back on the default
        rate and on Euler after the call."""
        if streaming:
            raise NotImplementedError("synthesise() runs the non-streaming decoder (jyutvoice_tts.py:239 passes streaming=False)"
                                      + ("; prompt_lengths has no streaming form" if prompt_lengths is not None else ""))
        if not self._loaded:
            raise RuntimeError(f"JyutVoiceTTS: load_state_dict() has not provided all weights yet; {len(self._missing)} tensors "
                               f"missing, e.g. {self._missing[:4]}")
        t0 = dt.datetime.now()
        B, Tt = x.shape
        p_host = None if prompt_lengths is None else self._check_prompt_lengths(prompt_lengths, prompt_feat, prompt_h, B)
        conf_rate, conf_sched, conf_solver = decoder_settings(self.decoder)
        rates = resolve_guidance("synthesise()", n_timesteps, conf_rate, cfg_rate, cfg_schedule)
        solver = resolve_solver("synthesise()", conf_solver, solver)
        t_span = time_span(n_timesteps, check_scheduler("synthesise()", conf_sched if t_scheduler is None else t_scheduler))   # flow_matching.py:387-389
        rt = get_runtime(self.device)
        eng = rt.ensure(B, 64, Tt)
        # stage_events (a list, set by bench.py for its per-stage pass; None otherwise): events on the launch stream at the
        # start, after encoder + duration predictor + length regulation, and after the CFM loop
        ev = getattr(self, "stage_events", None)

        def mark():
            if ev is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record(torch.cuda.current_stream(self.device))
                ev.append(e)
        mark()
        h, mu_x, logw, c = eng.encoder(x, x_lengths, lang, tone, word_pos, syllable_pos, spk_embed)
        w_ceil, y_lengths, attn, mu_y = eng.length_regulate(logw, x_lengths, mu_x, length_scale,
                                                            host_lengths=prompt_lengths is not None)
        mark()
        encoder_outputs = mu_y
        if B != 1 and not batched:
            raise ValueError(f"synthesise() requires batch_size=1, got batch_size={B}. Please pass one sample at a time.")
        if prompt_lengths is not None:
            # voice-cloning batch, one prompt length per utterance: the glue of jyutvoice_tts.py:213-244 runs inside
            # jv_cfm_solve_prompted, the tensors go there as they came
            eng = rt.ensure(B, max(p + y for p, y in zip(p_host, eng.y_lengths_host)), Tt)
            with eng.guidance(rates), eng.solver(solver):
                dec = eng.cfm_solve_prompted(mu_y, y_lengths, prompt_h, prompt_feat, prompt_lengths, c, n_timesteps, temperature,
                                             t_span=t_span)
            return self._result(t0, B, encoder_outputs, dec, attn, y_lengths, mark)
        mel_len1 = 0
        if prompt_feat is not None and prompt_h is not None:
            # voice-cloning glue (jyutvoice_tts.py:213-225): prompt frames are prepended to mu / cond
            prompt_h = prompt_h.to(self.device, torch.float32)
            prompt_feat = prompt_feat.to(self.device, torch.float32)
            mu_y = torch.cat([prompt_h.transpose(1, 2), mu_y], dim=2)
            mel_len1 = prompt_feat.shape[1]
            conds = torch.zeros(B, mu_y.shape[2], self.output_size, device=self.device)
            conds[:, :mel_len1] = prompt_feat
            conds = conds.transpose(1, 2).contiguous()
            lens = (y_lengths + mel_len1) if B > 1 else torch.full((1,), mu_y.shape[2], dtype=torch.int64, device=self.device)
        else:
            conds = torch.zeros_like(mu_y)
            lens = y_lengths
        T = mu_y.shape[2]
        eng = rt.ensure(B, T, Tt)
        with eng.guidance(rates), eng.solver(solver):
            dec = eng.cfm_solve(mu_y.contiguous(), lens if B > 1 else None, c, conds, n_timesteps, temperature, t_span=t_span)
        dec = dec[:, :, mel_len1:]
        return self._result(t0, B, encoder_outputs, dec, attn, y_lengths, mark)

    # ---- evaluation: alignment and the three losses (jyutvoice_tts.py:255-364), no gradients ------------------------------
    @torch.inference_mode()
    def forward(self, x, x_lengths, y, y_lengths, lang, tone, word_pos, syllable_pos, spk_embed, decoder_h, *, t=None, z=None,
                cfg_mask=None, cond_index=None, generator=None, return_parts=False):
        """-> (dur_loss, prior_loss, diff_loss, attn): three 0-d device tensors and the alignment [B, T_text, T_mel].

        x .. decoder_h as in the reference: y [B, 80, T_mel] target mels, decoder_h [B, T_mel, 80] hidden states of the flow
        encoder.  Every utterance needs 1 <= x_lengths[b] <= y_lengths[b] <= T_mel (an alignment gives each token a frame;
        the reference reads out of bounds otherwise): ValueError naming the utterance, before anything is launched.

        The reference draws four random things; each may be supplied instead (keyword-only):
          t           [B] in [0, 1): the uniform draw of flow_matching.py:320, BEFORE the cosine warp (applied here as there)
          z           like y: the noise of flow_matching.py:324
          cfg_mask    [B] bool / 0-1: False drops mu, spks and cond of that utterance (flow_matching.py:331-334)
          cond_index  [B] ints k_b: cond[b, :, :k_b] = y[b, :, :k_b]; 0 = no condition (jyutvoice_tts.py:325-330)
          generator   a torch.Generator of this model's device for what is NOT supplied of t, z, cfg_mask (drawn on the device;
                      same seed, same losses); cond_index is drawn with Python's `random` as the reference draws it.
        return_parts=True appends a dict: log_prior [B, T_text, T_mel], frame_index [B, T_mel] int32 (-1 behind the length),
        durations [B, T_text] int32, mu_y, y_t, u, pred [B, 80, T_mel], logw, mu_x, t (warped), spks (the projected speaker
        vector [B, 80]) and the masked estimator inputs mu_masked, spks_masked, cond."""
        if not self._loaded:
            raise RuntimeError(f"JyutVoiceTTS: load_state_dict() has not provided all weights yet; {len(self._missing)} tensors "
                               f"missing, e.g. {self._missing[:4]}")
        B, Tt = x.shape
        if y.dim() != 3 or y.shape[0] != B or y.shape[1] != self.n_feats:
            raise ValueError(f"forward(): y must be [{B}, {self.n_feats}, T_mel], got {tuple(y.shape)}")
        Ty = y.shape[-1]
        if decoder_h.dim() != 3 or decoder_h.shape[0] != B or decoder_h.shape[2] != self.n_feats or decoder_h.shape[1] != Ty:
            raise ValueError(f"forward(): decoder_h must be [{B}, {Ty}, {self.n_feats}] (as many frames as y), "
                             f"got {tuple(decoder_h.shape)}")
        xl_host, yl_host = [int(v) for v in x_lengths.tolist()], [int(v) for v in y_lengths.tolist()]
        if len(xl_host) != B or len(yl_host) != B:
            raise ValueError(f"forward(): x_lengths and y_lengths must have shape [{B}]")
        for b, (nx, ny) in enumerate(zip(xl_host, yl_host)):
            if nx < 1 or nx > Tt:
                raise ValueError(f"forward(): utterance {b}: {nx} tokens outside [1, {Tt}]")
            if ny < nx or ny > Ty:
                raise ValueError(f"forward(): utterance {b}: {ny} frames outside [tokens = {nx}, {Ty}]: an alignment needs a "
                                 "frame for every token")
        dev = self.device
        if cond_index is None:      # jyutvoice_tts.py:326-330
            cond_index = [0 if random.random() < 0.5 else random.randint(0, int(0.3 * ny)) for ny in yl_host]
        k_host = [int(v) for v in (cond_index.tolist() if torch.is_tensor(cond_index) else cond_index)]
        if len(k_host) != B:
            raise ValueError(f"forward(): cond_index must hold {B} entries")
        for b, k in enumerate(k_host):
            if k < 0 or k > Ty:
                raise ValueError(f"forward(): utterance {b}: cond_index {k} outside [0, {Ty}]")
        t = torch.rand(B, device=dev, generator=generator) if t is None else t.to(dev, torch.float32).reshape(B)
        t = 1 - torch.cos(t * 0.5 * torch.pi)      # flow_matching.py:321-322 (t_scheduler == "cosine")
        y = y.to(dev, torch.float32).contiguous()
        decoder_h = decoder_h.to(dev, torch.float32).contiguous()
        if z is None:
            z = torch.randn(y.shape, device=dev, generator=generator)
        elif tuple(z.shape) != tuple(y.shape):
            raise ValueError(f"forward(): z must have y's shape {tuple(y.shape)}, got {tuple(z.shape)}")
        if cfg_mask is None:
            rate = getattr(self.decoder, "training_cfg_rate", 0.2)
            cfg_mask = torch.rand(B, device=dev, generator=generator) > rate if rate > 0 else torch.ones(B, device=dev)
        cfg_mask = cfg_mask.to(dev).reshape(B).ne(0).to(torch.float32)

        eng = get_runtime(dev).ensure(B, Ty, Tt)
        xl = torch.tensor(xl_host, dtype=torch.int32, device=dev)
        yl = torch.tensor(yl_host, dtype=torch.int32, device=dev)
        _, mu_x, logw, c = eng.encoder(x, xl, lang, tone, word_pos, syllable_pos, spk_embed)
        attn, frame_index, durations, log_prior = eng.align(mu_x, decoder_h, xl, yl, want_log_prior=return_parts)
        dur_loss, prior_loss, mu_y = eng.align_losses(logw, durations, xl, mu_x, decoder_h, frame_index, yl)
        y_t, u, mu_m, spks_m, cond = eng.cfm_loss_inputs(y, z, t, cfg_mask, torch.tensor(k_host, dtype=torch.int32), mu_y, c)
        pred = eng.flow_estimator(y_t, yl, mu_m, t, spks_m, cond)
        diff_loss = eng.masked_mse(pred, u, yl)
        if not return_parts:
            return dur_loss, prior_loss, diff_loss, attn
        parts = {"log_prior": log_prior, "frame_index": frame_index, "durations": durations, "mu_y": mu_y, "y_t": y_t, "u": u,
                 "pred": pred, "logw": logw, "mu_x": mu_x, "t": t, "spks": c, "mu_masked": mu_m, "spks_masked": spks_m, "cond": cond}
        return dur_loss, prior_loss, diff_loss, attn, parts

    __call__ = forward

    def _result(self, t0, B, encoder_outputs, dec, attn, y_lengths, mark):
        mark()
        torch.cuda.synchronize(self.device)      # the reference's rtf omits this and is meaningless on a GPU
        t = (dt.datetime.now() - t0).total_seconds()
        rtf = t * spec.SAMPLE_RATE / (dec.shape[-1] * spec.HOP_LENGTH * max(B, 1))
        return {"encoder_outputs": encoder_outputs, "decoder_outputs": dec, "attn": attn.unsqueeze(1), "mel": dec,
                "mel_lengths": y_lengths, "rtf": rtf}
