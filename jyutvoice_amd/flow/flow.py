"""`CausalMaskedDiffWithXvec` drop-in for token-to-mel inference (jyutvoice/flow/flow.py:187-358): speech tokens -> mel, the
CosyVoice2 flow of a `flow.pt` -- resynthesis, voice conversion from tokens, the output stage of a token language model.

Same constructor keywords, the 1121 state-dict key names of the reference module (206 `encoder.*`, 910 `decoder.*`,
`input_embedding.weight`, `spk_embed_affine_layer.{weight,bias}`, `encoder_proj.{weight,bias}`) and the `inference()` signature,
`AssertionError` for a batch other than 1 and `(mel.float(), None)` return value.  All arithmetic runs in libjyutvoice_hip.so
(jv_flow_token2mel: embedding of [prompt tokens | tokens], the UpsampleConformer encoder on the fused relative-position attention,
speaker projection, the Euler / CFG solver); this class validates and moves pointers.

`finalize=False` is not implemented: the reference itself raises TypeError there (flow.py:330-336 passes `context=` to
UpsampleConformerEncoder.forward, which has no such parameter).  Training `forward()` is out of scope.

Extension: `inference_partial(...)` is what that branch intends -- the last `pre_lookahead_len` = 3 tokens are the look-ahead
convolution's right context and nothing else (jv_flow_token2mel_partial) -- under a name of its own, so `finalize=False` keeps raising
as the reference does.  With `streaming=True` and an encoded length that is a multiple of 25 tokens its frames are final: they are the
first frames of `inference` on any longer sequence (jyutvoice_amd/stream.py builds the session on that).

Extension (opt-in): `inference(..., batched=True)` accepts B > 1 and is defined as the B = 1 reference looped over the utterances
with every tensor cut to the utterance's own length: tokens `token[b, :token_len[b]]`, prompt `prompt_token[b, :prompt_token_len[b]]`,
`prompt_feat[b, :prompt_feat_len[b]]`.  Nothing behind a length is read.  The mel comes back [B, 80, max_b y_b] with utterance b in
`[:y_b]`, y_b = 2 (p_b + n_b) - f_b, zeros behind; `mel_lengths` holds the y_b of the last call.

Extension: `inference_partial_batch(..., ctx_lens)` is both extensions at once -- a batch whose utterance b is a partial sequence
(`ctx_lens[b]` = 3: `inference_partial`) or a whole one (0: `inference`), in one library call (jv_flow_token2mel_ctx): the step of a
server that advances several streaming sessions together (jyutvoice_amd/stream.py, `Token2WavServer`)."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .. import spec
from ..engine import JV_MODEL_FLOW, JV_MODEL_PROMPT, JV_MODEL_TTS
from .encoder import DIV_TERM_KEY, div_term, extract_flow_weights
from .flow_matching import check_scheduler, decoder_settings, resolve_guidance, resolve_solver, time_span

_NAME = "CausalMaskedDiffWithXvec"


def _host_ints(t, name: str, B: int):
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"inference(): {name} must be an int32 / int64 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if t.numel() != B:
        raise ValueError(f"inference(): {name} must hold {B} entries, got shape {tuple(t.shape)}")
    return [int(v) for v in t.reshape(-1).tolist()]


class CausalMaskedDiffWithXvec:
    def __init__(self, input_size: int = 512, output_size: int = 80, spk_embed_dim: int = 192, output_type: str = "mel",
                 vocab_size: int = 4096, input_frame_rate: int = 50, only_mask_loss: bool = True, token_mel_ratio: int = 2,
                 pre_lookahead_len: int = 3, encoder=None, decoder=None, decoder_conf: Optional[Dict] = None,
                 mel_feat_conf: Optional[Dict] = None, device="cuda:0", runtime=None):
        got = (input_size, output_size, spk_embed_dim, output_type, vocab_size, token_mel_ratio, pre_lookahead_len)
        want = (spec.PROMPT_DIM, spec.N_FEATS, spec.SPK_EMBED_DIM, "mel", spec.PROMPT_VOCAB, spec.PROMPT_UP_STRIDE,
                spec.PROMPT_LOOKAHEAD)
        if got != want:
            raise NotImplementedError("libjyutvoice_hip is built for the CosyVoice2 flow (input_size, output_size, spk_embed_dim, "
                                      f"output_type, vocab_size, token_mel_ratio, pre_lookahead_len) = {want}; got {got}")
        chunk = getattr(encoder, "static_chunk_size", spec.PROMPT_STATIC_CHUNK)
        if chunk != spec.PROMPT_STATIC_CHUNK:
            raise NotImplementedError(f"libjyutvoice_hip is built for an encoder static_chunk_size of {spec.PROMPT_STATIC_CHUNK}; "
                                      f"got {chunk}")
        est_chunk = getattr(getattr(decoder, "estimator", None), "static_chunk_size", spec.EST_STATIC_CHUNK)
        if est_chunk != spec.EST_STATIC_CHUNK:
            raise NotImplementedError(f"libjyutvoice_hip is built for an estimator static_chunk_size of {spec.EST_STATIC_CHUNK}; "
                                      f"got {est_chunk}")
        self.input_size, self.output_size, self.vocab_size = input_size, output_size, vocab_size
        self.output_type, self.input_frame_rate, self.only_mask_loss = output_type, input_frame_rate, only_mask_loss
        self.token_mel_ratio, self.pre_lookahead_len = token_mel_ratio, pre_lookahead_len
        self.encoder, self.decoder = encoder, decoder
        self.decoder_conf, self.mel_feat_conf = decoder_conf, mel_feat_conf
        self.device = torch.device(device)
        self._runtime = runtime
        self._loaded = False
        self.mel_lengths = None

    # ---- nn.Module-shaped plumbing -------------------------------------------------------------------------------------
    def to(self, device):
        self.device = torch.device(device)
        return self

    def eval(self):
        return self

    def _rt(self):
        if self._runtime is None:
            from ..runtime import get_runtime
            self._runtime = get_runtime(self.device)
        return self._runtime

    def _solver_settings(self, who, n_timesteps, cfg_rate, cfg_schedule, t_scheduler, solver=None):
        """(what Engine.guidance takes, t_span, what Engine.solver takes) of a call: the decoder's inference_cfg_rate / t_scheduler /
        solver unless overridden"""
        conf_rate, conf_sched, conf_solver = decoder_settings(self.decoder)
        sched = check_scheduler(who, conf_sched if t_scheduler is None else t_scheduler)
        return (resolve_guidance(who, n_timesteps, conf_rate, cfg_rate, cfg_schedule), time_span(n_timesteps, sched),
                resolve_solver(who, conf_solver, solver))

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True, decoder: str = "own"):
        """The reference module's 1121 keys, split with `extract_flow_weights` into the flow encoder (JV_MODEL_PROMPT) and the
        decoder part (JV_MODEL_FLOW: `decoder.*`, `spk_embed_affine_layer.*`).  decoder="shared": the runtime already holds a
        finalized `JyutVoiceTTS`; its decoder is reused and only the encoder part of `state_dict` is taken (decoder keys may be
        present or absent)."""
        if decoder not in ("own", "shared"):
            raise ValueError(f"load_state_dict(): decoder must be 'own' or 'shared', got {decoder!r}")
        inventory = spec.PROMPT_INVENTORY if decoder == "shared" else spec.FLOW_INVENTORY
        missing = [k for k in inventory if k not in state_dict]
        unexpected = [k for k in state_dict if k not in spec.FLOW_INVENTORY]
        if missing or (strict and unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for {_NAME}: Missing key(s): {missing[:6]}; "
                               f"Unexpected key(s): {unexpected[:6]}")
        for k, shape in inventory.items():
            if tuple(state_dict[k].shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {k}: copying a param with shape {tuple(state_dict[k].shape)} from "
                                   f"checkpoint, the shape in current model is {tuple(shape)}.")
        enc, dec = extract_flow_weights({k: state_dict[k] for k in inventory})
        rt = self._rt()
        if decoder == "shared" and JV_MODEL_TTS not in rt.sds:
            raise RuntimeError(f"{_NAME}.load_state_dict(decoder='shared'): this runtime holds no finalized JyutVoiceTTS to share "
                               "a decoder with")
        if decoder == "own" and JV_MODEL_TTS in rt.sds:      # (Runtime.set_weights would refuse too, after the encoder went up)
            raise RuntimeError(f"{_NAME}.load_state_dict(): this runtime already holds a JyutVoiceTTS, whose decoder occupies the flow "
                               "decoder's slots: pass decoder='shared' to reuse it, or give the flow another Runtime")
        enc[DIV_TERM_KEY] = div_term()
        rt.set_weights(JV_MODEL_PROMPT, enc)
        if decoder == "own":
            rt.set_weights(JV_MODEL_FLOW, dec)
        self._loaded = True
        return missing, unexpected

    # ---- the hot path --------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def inference(self, token, token_len, prompt_token, prompt_token_len, prompt_feat, prompt_feat_len, embedding, streaming,
                  finalize, batched: bool = False, n_timesteps: int = 10, temperature: float = 1.0, cfg_rate=None, cfg_schedule=None,
                  t_scheduler=None, solver=None):
        """flow.py:300-358 -> (mel [B, 80, T_mel] float32, None).  token [B, N], prompt_token [B, P] int; prompt_feat [B, F, 80];
        embedding [B, 192] (raw: F.normalize and the affine layer run in the library); streaming: the chunk masks of the encoder
        (25 tokens / 50 frames) and of the estimator (50 frames).

        Without `batched` this is the reference: B must be 1, and `mel_len1 = prompt_feat.shape[1]` -- prompt_feat_len is not
        consulted, as in flow.py:337 -- so the mel has 2 (P + N) - prompt_feat.shape[1] frames.  With `batched=True` utterance b
        uses f_b = prompt_feat_len[b] frames of its prompt mel (see the module docstring).  The solve runs at the decoder's
        inference_cfg_rate and t_scheduler (flow_matching.py:215-265, 387-389); cfg_rate / cfg_schedule override the rate for this
        call (one rate / one per Euler step), t_scheduler the schedule ("cosine" / "linear") and solver the integrator ("euler" /
        "midpoint" / "heun"; None: the decoder's `solver`, "euler" unless set), here and in inference_partial / inference_partial_batch."""
        B = token.shape[0]
        if not batched:
            assert B == 1
        if finalize is not True:
            raise NotImplementedError("inference(finalize=False) is not implemented: the reference itself raises TypeError there -- "
                                      "flow.py:330-336 passes `context=` to UpsampleConformerEncoder.forward, which has no such "
                                      "parameter; chunk-cached encoding (forward_chunk) is out of scope")
        if prompt_token is None:
            prompt_token = torch.zeros(B, 0, dtype=torch.int64)
        if token.dim() != 2 or prompt_token.dim() != 2 or prompt_token.shape[0] != B:
            raise ValueError(f"inference(): token must be [B, N] and prompt_token [B, P], got {tuple(token.shape)} and "
                             f"{tuple(prompt_token.shape)}")
        N, P = token.shape[1], prompt_token.shape[1]
        if prompt_feat is None:
            prompt_feat = torch.zeros(B, 0, spec.N_FEATS)
        if prompt_feat.dim() != 3 or prompt_feat.shape[0] != B or prompt_feat.shape[2] != spec.N_FEATS:
            raise ValueError(f"inference(): prompt_feat must be [{B}, frames, {spec.N_FEATS}], got {tuple(prompt_feat.shape)}")
        if embedding.dim() != 2 or tuple(embedding.shape) != (B, spec.SPK_EMBED_DIM):
            raise ValueError(f"inference(): embedding must be [{B}, {spec.SPK_EMBED_DIM}], got {tuple(embedding.shape)}")
        F = prompt_feat.shape[1]
        n_host = _host_ints(token_len, "token_len", B)
        p_host = _host_ints(prompt_token_len, "prompt_token_len", B) if P > 0 else [0] * B
        if batched:
            f_host = _host_ints(prompt_feat_len, "prompt_feat_len", B) if F > 0 else [0] * B
            for b in range(B):
                if not 0 <= n_host[b] <= N:
                    raise ValueError(f"inference(): utterance {b}: token_len {n_host[b]} outside [0, {N}]")
                if not 0 <= p_host[b] <= P:
                    raise ValueError(f"inference(): utterance {b}: prompt_token_len {p_host[b]} outside [0, {P}]")
        else:
            # the reference concatenates the two token tensors at their full widths and masks by the summed length
            total = p_host[0] + n_host[0]
            if not P <= total <= P + N:
                raise ValueError(f"inference(): prompt_token_len + token_len = {total} outside [{P}, {P + N}]: the reference's "
                                 f"sequence is the {P} prompt columns followed by the tokens")
            p_host, n_host, f_host = [P], [total - P], [F]
        for b in range(B):
            tb = spec.PROMPT_UP_STRIDE * (p_host[b] + n_host[b])
            if not 0 <= f_host[b] <= min(F, tb):
                raise ValueError(f"inference(): utterance {b}: prompt_feat length {f_host[b]} outside [0, min(prompt_feat frames = "
                                 f"{F}, 2 * tokens = {tb})]")
        if not self._loaded:
            raise RuntimeError(f"{_NAME}: load_state_dict() has not been called")
        eng = self._rt().ensure(B, spec.PROMPT_UP_STRIDE * (P + N), 1)
        rates, t_span, solver = self._solver_settings("inference()", n_timesteps, cfg_rate, cfg_schedule, t_scheduler, solver)
        with eng.guidance(rates), eng.solver(solver):
            mel, lens = eng.flow_token2mel(prompt_token if P > 0 else None, torch.tensor(p_host), token, torch.tensor(n_host),
                                           prompt_feat if F > 0 else None, torch.tensor(f_host, dtype=torch.int32), embedding,
                                           streaming=bool(streaming), n_timesteps=n_timesteps, temperature=temperature, t_span=t_span)
        self.mel_lengths = lens
        y_host = [spec.PROMPT_UP_STRIDE * (p + n) - f for p, n, f in zip(p_host, n_host, f_host)]
        width = max(y_host) if batched else spec.PROMPT_UP_STRIDE * (P + N) - F      # flow.py:337,356
        return mel[:, :, :width].float(), None


    @torch.inference_mode()
    def inference_partial(self, token, token_len, prompt_token, prompt_token_len, prompt_feat, prompt_feat_len, embedding, streaming,
                          n_timesteps: int = 10, temperature: float = 1.0, cfg_rate=None, cfg_schedule=None, t_scheduler=None,
                          solver=None):
        """flow.py:327-336 as intended, B = 1 -> (mel [1, 80, 2 L - F] float32, None).  Of the m = P + N tokens the encoder runs on
        the first L = m - 3 (every length and mask uses L); the last three are embedded like the others (upsample_encoder.py:446-453)
        and read by PreLookaheadLayer.conv1 alone, in place of its zero padding (upsample_encoder.py:110-121).  F = prompt_feat.shape[1]
        (prompt_feat_len is not consulted, as in `inference`)."""
        if token.dim() != 2 or token.shape[0] != 1:
            raise ValueError(f"inference_partial(): token must be [1, N], got {tuple(token.shape)}")
        if prompt_token is None:
            prompt_token = torch.zeros(1, 0, dtype=torch.int64)
        if prompt_token.dim() != 2 or prompt_token.shape[0] != 1:
            raise ValueError(f"inference_partial(): prompt_token must be [1, P], got {tuple(prompt_token.shape)}")
        N, P = token.shape[1], prompt_token.shape[1]
        if prompt_feat is None:
            prompt_feat = torch.zeros(1, 0, spec.N_FEATS)
        if prompt_feat.dim() != 3 or prompt_feat.shape[0] != 1 or prompt_feat.shape[2] != spec.N_FEATS:
            raise ValueError(f"inference_partial(): prompt_feat must be [1, frames, {spec.N_FEATS}], got {tuple(prompt_feat.shape)}")
        if embedding.dim() != 2 or tuple(embedding.shape) != (1, spec.SPK_EMBED_DIM):
            raise ValueError(f"inference_partial(): embedding must be [1, {spec.SPK_EMBED_DIM}], got {tuple(embedding.shape)}")
        F = prompt_feat.shape[1]
        m = _host_ints(token_len, "token_len", 1)[0] + (_host_ints(prompt_token_len, "prompt_token_len", 1)[0] if P > 0 else 0)
        if not P <= m <= P + N:
            raise ValueError(f"inference_partial(): prompt_token_len + token_len = {m} outside [{P}, {P + N}]: the reference's "
                             f"sequence is the {P} prompt columns followed by the tokens")
        if m < spec.PROMPT_LOOKAHEAD + 1:
            raise ValueError(f"inference_partial(): {m} tokens: at least {spec.PROMPT_LOOKAHEAD + 1} are needed (the last "
                             f"{spec.PROMPT_LOOKAHEAD} are look-ahead context only)")
        L = m - spec.PROMPT_LOOKAHEAD
        if F > spec.PROMPT_UP_STRIDE * L:
            raise ValueError(f"inference_partial(): prompt_feat has {F} frames but the {L} encoded tokens give only "
                             f"{spec.PROMPT_UP_STRIDE * L}")
        if not self._loaded:
            raise RuntimeError(f"{_NAME}: load_state_dict() has not been called")
        eng = self._rt().ensure(1, spec.PROMPT_UP_STRIDE * (P + N), 1)
        rates, t_span, solver = self._solver_settings("inference_partial()", n_timesteps, cfg_rate, cfg_schedule, t_scheduler, solver)
        with eng.guidance(rates), eng.solver(solver):
            mel, lens = eng.flow_token2mel_partial(prompt_token if P > 0 else None, torch.tensor([P]), token, torch.tensor([m - P]),
                                                   prompt_feat if F > 0 else None, torch.tensor([F], dtype=torch.int32), embedding,
                                                   streaming=bool(streaming), n_timesteps=n_timesteps, temperature=temperature,
                                                   t_span=t_span)
        self.mel_lengths = lens
        return mel[:, :, :spec.PROMPT_UP_STRIDE * L - F].float(), None


    @torch.inference_mode()
    def inference_partial_batch(self, token, token_len, prompt_token, prompt_token_len, prompt_feat, prompt_feat_len, embedding,
                                ctx_lens, streaming=True, n_timesteps: int = 10, temperature: float = 1.0, cfg_rate=None,
                                cfg_schedule=None, t_scheduler=None, solver=None):
        """A batch that mixes partial and whole sequences -> (mel [B, 80, max_b y_b] float32, mel_lens int32 [B] on the device).
        Defined as the B = 1 calls looped over the utterances, every tensor cut to the utterance's own length as in
        `inference(batched=True)`: `inference_partial` where ctx_lens[b] = 3 (the last three of the p_b + n_b tokens are look-ahead
        context only), `inference(finalize=True)` where it is 0.  L_b = p_b + n_b - ctx_lens[b] tokens are encoded, f_b =
        prompt_feat_len[b] prompt frames cut, y_b = 2 L_b - f_b frames come back in `[b, :, :y_b]`, zeros behind.  Nothing behind a
        length is read.  One library call (jv_flow_token2mel_ctx): what a streaming server runs per step for all its sessions."""
        who = "inference_partial_batch()"
        if token.dim() != 2:
            raise ValueError(f"{who}: token must be [B, N], got {tuple(token.shape)}")
        B, N = token.shape
        if prompt_token is None:
            prompt_token = torch.zeros(B, 0, dtype=torch.int64)
        if prompt_token.dim() != 2 or prompt_token.shape[0] != B:
            raise ValueError(f"{who}: prompt_token must be [{B}, P], got {tuple(prompt_token.shape)}")
        P = prompt_token.shape[1]
        if prompt_feat is None:
            prompt_feat = torch.zeros(B, 0, spec.N_FEATS)
        if prompt_feat.dim() != 3 or prompt_feat.shape[0] != B or prompt_feat.shape[2] != spec.N_FEATS:
            raise ValueError(f"{who}: prompt_feat must be [{B}, frames, {spec.N_FEATS}], got {tuple(prompt_feat.shape)}")
        if embedding.dim() != 2 or tuple(embedding.shape) != (B, spec.SPK_EMBED_DIM):
            raise ValueError(f"{who}: embedding must be [{B}, {spec.SPK_EMBED_DIM}], got {tuple(embedding.shape)}")
        F = prompt_feat.shape[1]
        n_host = _host_ints(token_len, "token_len", B)
        p_host = _host_ints(prompt_token_len, "prompt_token_len", B) if P > 0 else [0] * B
        f_host = _host_ints(prompt_feat_len, "prompt_feat_len", B) if F > 0 else [0] * B
        c_host = _host_ints(torch.as_tensor(ctx_lens), "ctx_lens", B)
        y_host = []
        for b in range(B):
            if not 0 <= n_host[b] <= N:
                raise ValueError(f"{who}: utterance {b}: token_len {n_host[b]} outside [0, {N}]")
            if not 0 <= p_host[b] <= P:
                raise ValueError(f"{who}: utterance {b}: prompt_token_len {p_host[b]} outside [0, {P}]")
            if c_host[b] not in (0, spec.PROMPT_LOOKAHEAD):
                raise ValueError(f"{who}: utterance {b}: ctx_lens {c_host[b]}: the look-ahead length {spec.PROMPT_LOOKAHEAD} (a partial "
                                 "sequence) or 0 (a whole one)")
            m = p_host[b] + n_host[b]
            if c_host[b] and m < spec.PROMPT_LOOKAHEAD + 1:
                raise ValueError(f"{who}: utterance {b}: {m} tokens: at least {spec.PROMPT_LOOKAHEAD + 1} are needed (the last "
                                 f"{spec.PROMPT_LOOKAHEAD} are look-ahead context only)")
            if m < 1:
                raise ValueError(f"{who}: utterance {b}: no tokens")
            L = m - c_host[b]
            if not 0 <= f_host[b] <= F or f_host[b] > spec.PROMPT_UP_STRIDE * L:
                raise ValueError(f"{who}: utterance {b}: prompt_feat has {f_host[b]} frames (of {F}) but the {L} encoded tokens give only "
                                 f"{spec.PROMPT_UP_STRIDE * L}")
            y_host.append(spec.PROMPT_UP_STRIDE * L - f_host[b])
        if not self._loaded:
            raise RuntimeError(f"{_NAME}: load_state_dict() has not been called")
        eng = self._rt().ensure(B, spec.PROMPT_UP_STRIDE * (P + N), 1)
        rates, t_span, solver = self._solver_settings(who, n_timesteps, cfg_rate, cfg_schedule, t_scheduler, solver)
        with eng.guidance(rates), eng.solver(solver):
            mel, lens = eng.flow_token2mel_ctx(prompt_token if P > 0 else None, torch.tensor(p_host), token, torch.tensor(n_host),
                                               torch.tensor(c_host, dtype=torch.int32), prompt_feat if F > 0 else None,
                                               torch.tensor(f_host, dtype=torch.int32), embedding, streaming=bool(streaming),
                                               n_timesteps=n_timesteps, temperature=temperature, t_span=t_span)
        self.mel_lengths = lens
        return mel[:, :, :max(y_host)].float(), lens


def load_flow(flow_path, device="cuda:0", decoder: str = "own", runtime=None):
    """`CausalMaskedDiffWithXvec` with the weights of a CosyVoice2 `flow.pt` (the 1121-key state-dict)"""
    flow = CausalMaskedDiffWithXvec(vocab_size=spec.PROMPT_VOCAB, input_frame_rate=25, device=device, runtime=runtime)
    sd = torch.load(flow_path, map_location="cpu", weights_only=True)
    flow.load_state_dict(sd["state_dict"] if isinstance(sd, dict) and "state_dict" in sd else sd, decoder=decoder)
    return flow.eval()
