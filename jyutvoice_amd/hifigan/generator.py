"""`HiFTGenerator` drop-in for inference (jyutvoice/hifigan/generator.py:239-466): same constructor keywords,
state-dict key names (both weight-norm spellings), `inference(speech_feat, cache_source) -> (wav, s)` and
`decode(x, s)`.  All arithmetic runs in libjyutvoice_hip.so (jv_hift_f0 / jv_hift_source / jv_hift_decode).

The reference's sine generator draws Uniform(-pi, pi) phases and N(0,1) noise per call (generator.py:155-158,
171), so `inference` is stochastic there too; here the nine phases per utterance come from a torch generator on the GPU and
the per-sample N(0,1) noise from a counter-based generator INSIDE the source kernel (jv_hift_source_seeded: Philox keyed by
the seed, counted per call -- `manual_seed` makes both repeatable), so the 9 x 480 T noise tensor is never materialised.
The library owns no RNG state: (seed, call) are arguments.  `Engine.hift_source(f0, phase, noise)` (jv_hift_source) injects a
caller's draws instead -- what the parity tests do with the oracle's.

Extension: `stream()` opens a `HiFTStream`, which takes the mel in pieces and returns the samples that are final -- the same
waveform `inference` gives on the whole mel (module-level docstring of HiFTStream)."""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

from .. import spec
from ..engine import JV_MODEL_HIFT
from ..runtime import get_runtime
from .f0_predictor import ConvRNNF0Predictor


class HiFTGenerator:
    def __init__(self, in_channels: int = 80, base_channels: int = 512, nb_harmonics: int = 8, sampling_rate: int = 22050,
                 nsf_alpha: float = 0.1, nsf_sigma: float = 0.003, nsf_voiced_threshold: float = 10,
                 upsample_rates: List[int] = [8, 8], upsample_kernel_sizes: List[int] = [16, 16],
                 istft_params: Dict[str, int] = {"n_fft": 16, "hop_len": 4}, resblock_kernel_sizes: List[int] = [3, 7, 11],
                 resblock_dilation_sizes: List[List[int]] = [[1, 3, 5], [1, 3, 5], [1, 3, 5]],
                 source_resblock_kernel_sizes: List[int] = [7, 11],
                 source_resblock_dilation_sizes: List[List[int]] = [[1, 3, 5], [1, 3, 5]], lrelu_slope: float = 0.1,
                 audio_limit: float = 0.99, f0_predictor: Optional[ConvRNNF0Predictor] = None, device="cuda:0"):
        got = (in_channels, base_channels, nb_harmonics, sampling_rate, float(nsf_alpha), float(nsf_sigma),
               float(nsf_voiced_threshold), tuple(upsample_rates), tuple(upsample_kernel_sizes), istft_params["n_fft"],
               istft_params["hop_len"], tuple(resblock_kernel_sizes), tuple(map(tuple, resblock_dilation_sizes)),
               tuple(source_resblock_kernel_sizes), float(lrelu_slope), float(audio_limit))
        want = (spec.N_FEATS, spec.HIFT_BASE_CH, spec.HIFT_NB_HARMONICS, spec.SAMPLE_RATE, spec.HIFT_NSF_ALPHA,
                spec.HIFT_NSF_SIGMA, spec.HIFT_VOICED_THRESHOLD, spec.HIFT_UP_RATES, spec.HIFT_UP_KERNELS, spec.HIFT_NFFT,
                spec.HIFT_HOP, spec.HIFT_RB_KERNELS, (spec.HIFT_RB_DILATIONS,) * 3, spec.HIFT_SRC_RB_KERNELS,
                spec.HIFT_LRELU_SLOPE, spec.HIFT_AUDIO_LIMIT)
        if got != want:
            raise NotImplementedError(f"libjyutvoice_hip is built for the base.yaml HiFT generator {want}; got {got}")
        self.sampling_rate = sampling_rate
        self.f0_predictor = f0_predictor
        self.device = torch.device(device)
        self._loaded = False
        self._gen: Optional[torch.Generator] = None
        self._seed: Optional[int] = None      # of the in-kernel source noise; drawn on first use unless manual_seed() set it
        self._calls = 0

    def to(self, device):
        self.device = torch.device(device)
        return self

    def eval(self):
        return self

    def manual_seed(self, seed: int):
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(seed)
        self._seed, self._calls = int(seed), 0
        return self

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        missing = [k for k in spec.HIFT_INVENTORY if k not in state_dict]
        unexpected = [k for k in state_dict if k not in spec.HIFT_INVENTORY]
        if missing or (strict and unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for HiFTGenerator: Missing key(s): {missing[:6]}; "
                               f"Unexpected key(s): {unexpected[:6]}")
        for k, shape in spec.HIFT_INVENTORY.items():
            if tuple(state_dict[k].shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {k}: copying a param with shape {tuple(state_dict[k].shape)} from "
                                   f"checkpoint, the shape in current model is {tuple(shape)}.")
        get_runtime(self.device).set_weights(JV_MODEL_HIFT, {k: state_dict[k] for k in spec.HIFT_INVENTORY})
        self._loaded = True
        return missing, unexpected

    def _engine(self, B, T):
        if not self._loaded:
            raise RuntimeError("HiFTGenerator: load_state_dict() has not been called")
        rt = get_runtime(self.device)
        return rt.ensure(B, T, 1)

    def _source_draws(self, B):
        """the random draws of one source signal: (phase [B, 9] on the device, seed, call) -- one `inference`, or one stream"""
        phase = (torch.rand(B, 9, device=self.device, generator=self._gen) * 2 - 1) * math.pi
        if self._seed is None:      # (a host draw: no device synchronisation)
            self._seed = int(torch.empty((), dtype=torch.int64).random_().item())
        call = self._calls
        self._calls += 1
        return phase, self._seed, call

    def stream(self) -> "HiFTStream":
        """a chunked session (B = 1): `push(mel piece)` returns the samples that are now final, `finish()` the rest; the pieces
        concatenate to what `inference` returns for the whole mel after the same `manual_seed`"""
        if not self._loaded:
            raise RuntimeError("HiFTGenerator: load_state_dict() has not been called")
        return HiFTStream(self)

    def stream_batch(self, slots: int, max_frames: int) -> "HiFTStreamBatch":
        """`slots` chunked sessions advanced together: one f0, one source and one decode launch sequence per step for all of them
        (HiFTStreamBatch); each slot is a `stream()` of at most `max_frames` mel frames"""
        if not self._loaded:
            raise RuntimeError("HiFTGenerator: load_state_dict() has not been called")
        return HiFTStreamBatch(self, slots, max_frames)

    @torch.inference_mode()
    def decode(self, x: torch.Tensor, s: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """generator.py:396-432: mel [B,80,T] + source [B,1,480T] -> waveform [B,480T]"""
        B, _, T = x.shape
        return self._engine(B, T).hift_decode(x, s, lengths)

    @torch.inference_mode()
    def inference(self, speech_feat: torch.Tensor, cache_source: torch.Tensor = torch.zeros(1, 1, 0),
                  lengths: Optional[torch.Tensor] = None):
        """generator.py:450-466 -> (generated_speech [B,480T], s [B,1,480T])"""
        B, _, T = speech_feat.shape
        eng = self._engine(B, T)
        f0 = eng.hift_f0(speech_feat, lengths)
        phase, seed, call = self._source_draws(B)
        s = eng.hift_source_seeded(f0, phase, seed, call)
        if cache_source.shape[2] != 0:
            s[:, :, : cache_source.shape[2]] = cache_source.to(self.device)
        return eng.hift_decode(speech_feat, s, lengths), s


class HiFTStream:
    """One utterance through the vocoder in pieces, B = 1.  `push(mel [1, 80, t]) -> (wav [1, 480 k], s [1, 1, 480 k])` with the k
    frames that became final (k may be 0); `finish()` returns the rest.  Nothing is cross-faded: every emitted sample is the centre
    of a window wide enough that the one-shot decode of the whole mel computes the same value.

    With A frames received:
      f0      is final for frames < A - HIFT_F0_HALO (five k = 3 convolutions): jv_hift_f0 on a window with that halo on its left,
              cropped;
      source  appended for exactly those frames by jv_hift_source_cont -- the running phase sums live in `cum` on the device, the
              noise counters are absolute, so the assembled signal is bit for bit jv_hift_source_seeded on the f0 record;
      decode  jv_hift_decode on [E - HIFT_DECODE_HALO, A_src), E frames emitted so far, A_src frames of source; frames
              [E, A_src - HIFT_DECODE_HALO) are kept.  A window edge that is the utterance's true start (or, in finish(), end) needs
              no halo.
    The newest emitted frame trails the newest received one by 21 frames.  State: the mel and source of frames not yet retired, the
    f0 record (`f0`, [1, frames with a final f0]), `cum`, the counts.  Phases and (seed, call) are drawn once, when the stream is
    opened, the way `inference` draws them."""

    def __init__(self, hift):
        self._hift = hift
        self._phase, self._seed, self._call = hift._source_draws(1)
        dev = self._phase.device
        self.cum = torch.zeros(1, 9, dtype=torch.float64, device=dev)
        self.f0 = torch.zeros(1, 0, device=dev)
        self._mel = torch.zeros(1, spec.N_FEATS, 0, device=dev)      # frames [self._base, self.received)
        self._s = torch.zeros(1, 1, 0, device=dev)                  # samples of frames [self._base, self.sourced)
        self._base = 0
        self.received = self.sourced = self.emitted = 0
        self.finished = False

    def _check(self, mel):
        if self.finished:
            raise RuntimeError("HiFTStream: finish() has been called")
        if not isinstance(mel, torch.Tensor) or mel.dim() != 3 or mel.shape[0] != 1 or mel.shape[1] != spec.N_FEATS:
            raise ValueError(f"HiFTStream.push(): mel must be [1, {spec.N_FEATS}, frames], got "
                             f"{tuple(mel.shape) if isinstance(mel, torch.Tensor) else type(mel).__name__}")

    @torch.inference_mode()
    def push(self, mel: torch.Tensor):
        self._check(mel)
        return self._advance(mel, final=False)

    @torch.inference_mode()
    def finish(self, mel: Optional[torch.Tensor] = None):
        if mel is not None:
            self._check(mel)
        elif self.finished:
            raise RuntimeError("HiFTStream: finish() has been called")
        out = self._advance(mel, final=True)
        self.finished = True
        return out

    def _advance(self, mel, final):
        up, dev = spec.HIFT_UPSAMPLE_TOTAL, self._mel.device
        if mel is not None and mel.shape[2] > 0:
            self._mel = torch.cat([self._mel, mel.to(device=dev, dtype=torch.float32)], dim=2)
            self.received += mel.shape[2]
        A, base = self.received, self._base
        # f0 and source of the frames whose f0 no later frame can change
        f_hi = A if final else max(A - spec.HIFT_F0_HALO, self.sourced)
        if f_hi > self.sourced:
            lo = max(self.sourced - spec.HIFT_F0_HALO, 0)
            eng = self._hift._engine(1, A - lo)
            f0 = eng.hift_f0(self._mel[:, :, lo - base:])[:, self.sourced - lo: f_hi - lo]
            piece = eng.hift_source_cont(f0, self._phase, self._seed, self._call, up * self.sourced, self.cum)
            self.f0 = torch.cat([self.f0, f0], dim=1)
            self._s = torch.cat([self._s, piece], dim=2)
            self.sourced = f_hi
        # decode the frames that have a full halo of mel and source on their right
        E = self.emitted
        k_hi = self.sourced if final else max(self.sourced - spec.HIFT_DECODE_HALO, E)
        if k_hi > E:
            lo = max(E - spec.HIFT_DECODE_HALO, 0)
            eng = self._hift._engine(1, self.sourced - lo)
            s_win = self._s[:, :, up * (lo - base):]
            wav = eng.hift_decode(self._mel[:, :, lo - base: self.sourced - base], s_win)
            out = wav[:, up * (E - lo): up * (k_hi - lo)], s_win[:, :, up * (E - lo): up * (k_hi - lo)]
            self.emitted = k_hi
        else:
            out = torch.zeros(1, 0, device=dev), torch.zeros(1, 1, 0, device=dev)
        # retire what neither the next f0 window nor the next decode window reads
        keep = max(min(self.emitted - spec.HIFT_DECODE_HALO, self.sourced - spec.HIFT_F0_HALO), base)
        if keep > base:
            self._mel = self._mel[:, :, keep - base:]
            self._s = self._s[:, :, up * (keep - base):]
            self._base = keep
        return out


def stream_step(received: int, sourced: int, emitted: int, k: int, final: bool):
    """One step of HiFTStream's schedule from the counts alone (host only): a stream that has received / sourced / emitted that many
    frames takes k more (final: and finishes).  -> (A, f0 window or None, decode window or None): A frames received afterwards;
    f0 window (lo, crop0, crop1): jv_hift_f0 runs on frames [lo, A) and [crop0, crop1) get their f0 and source; decode window
    (lo, hi, keep0, keep1): jv_hift_decode runs on frames [lo, hi), hi the frames sourced afterwards, and [keep0, keep1) are emitted."""
    A = received + k
    f_hi = A if final else max(A - spec.HIFT_F0_HALO, sourced)
    fwin = (max(sourced - spec.HIFT_F0_HALO, 0), sourced, f_hi) if f_hi > sourced else None
    k_hi = f_hi if final else max(f_hi - spec.HIFT_DECODE_HALO, emitted)
    dwin = (max(emitted - spec.HIFT_DECODE_HALO, 0), f_hi, emitted, k_hi) if k_hi > emitted else None
    return A, fwin, dwin


class HiFTStreamBatch:
    """`slots` HiFTStreams advanced together.  Every slot follows HiFTStream's schedule (`stream_step`: HIFT_F0_HALO, HIFT_DECODE_HALO,
    true edges need no halo) and its own source signal -- `open()` draws (phase, seed, call) the way HiFTStream does, so the k-th slot
    opened after `manual_seed(s)` is the k-th `hift.stream()` after it -- but a step runs ONE jv_hift_f0, ONE jv_hift_source_cont_rows
    and ONE jv_hift_decode on the ragged windows of all slots that moved, with `lens` per row.

    State lives on the device in pools indexed by slot: `mel` [slots, 80, max_frames], `source` [slots, 1, 480 max_frames], `f0`
    [slots, max_frames] (a slot's whole record: with the capacity fixed up front nothing has to be retired), the phases and running
    sums [slots, 9], the noise keys.  Appending a piece, gathering the windows and cropping what they keep are jv_slab_copy launches
    -- eight per step however many slots move -- fed by descriptors that go up in one copy.

    `advance(mel, rows)`: mel [R, 80, W] on the device (or None), rows = [(slot, src_row, lo, hi, final)]: slot receives
    mel[src_row, :, lo:hi] (src_row None: nothing) and finishes if final.  -> {slot: (wav [1, 480 k], s [1, 1, 480 k])} for the
    slots in `rows`; `s` is a view of the slot's record, valid until the slot is opened again."""

    def __init__(self, hift, slots: int, max_frames: int):
        if not isinstance(slots, int) or slots < 1 or not isinstance(max_frames, int) or max_frames < 1:
            raise ValueError(f"HiFTStreamBatch: slots and max_frames must be positive ints, got {slots!r}, {max_frames!r}")
        self._hift, self.slots, self.max_frames = hift, slots, max_frames
        dev, up = hift.device, spec.HIFT_UPSAMPLE_TOTAL
        hift._engine(slots, max_frames)
        self.mel = torch.zeros(slots, spec.N_FEATS, max_frames, device=dev)
        self.source = torch.zeros(slots, 1, up * max_frames, device=dev)
        self.f0 = torch.zeros(slots, max_frames, device=dev)
        self.phase = torch.zeros(slots, 9, device=dev)
        self.cum = torch.zeros(slots, 9, dtype=torch.float64, device=dev)
        self.seeds = torch.zeros(slots, dtype=torch.int64, device=dev)
        self.calls = torch.zeros(slots, dtype=torch.int32, device=dev)
        self.state = [None] * slots      # per open slot: [received, sourced, emitted]
        self.last = [None] * slots       # the counts of the slot's last stream, once closed
        self.draws = [None] * slots      # (seed, call) of the slot's signal, on the host

    def open(self, slot: Optional[int] = None) -> int:
        if slot is None:
            free = [i for i, s in enumerate(self.state) if s is None]
            if not free:
                raise RuntimeError(f"HiFTStreamBatch: all {self.slots} slots are taken")
            slot = free[0]
        elif not 0 <= slot < self.slots or self.state[slot] is not None:
            raise RuntimeError(f"HiFTStreamBatch: slot {slot} is not free")
        phase, seed, call = self._hift._source_draws(1)
        self.phase[slot] = phase[0]
        self.cum[slot] = 0.0
        s64 = seed & (2 ** 64 - 1)
        self.seeds[slot] = s64 - 2 ** 64 if s64 >= 2 ** 63 else s64      # (the uint64 key's bit pattern)
        c32 = call & 0xFFFFFFFF
        self.calls[slot] = c32 - 2 ** 32 if c32 >= 2 ** 31 else c32
        self.state[slot], self.draws[slot] = [0, 0, 0], (seed, call)
        return slot

    def close(self, slot: int):
        """the slot is free again (its records stay readable until it is opened)"""
        self.last[slot], self.state[slot] = self.state[slot], None

    def records(self, slot: int):
        """views of a slot's records -- of its open stream, else of the one closed last: (mel [1, 80, received], source
        [1, 1, 480 emitted], f0 [1, sourced])"""
        r, s, e = self.state[slot] or self.last[slot]
        return (self.mel[slot:slot + 1, :, :r], self.source[slot:slot + 1, :, :spec.HIFT_UPSAMPLE_TOTAL * e], self.f0[slot:slot + 1, :s])

    @torch.inference_mode()
    def advance(self, mel, rows):
        up, dev = spec.HIFT_UPSAMPLE_TOTAL, self._hift.device
        seen = set()
        for slot, src_row, lo, hi, final in rows:
            if not 0 <= slot < self.slots or self.state[slot] is None or slot in seen:
                raise RuntimeError(f"HiFTStreamBatch.advance(): slot {slot} is not open, or named twice")
            seen.add(slot)
            k = 0 if src_row is None else hi - lo
            if k < 0 or (k > 0 and (mel is None or not 0 <= src_row < mel.shape[0] or lo < 0 or hi > mel.shape[2])):
                raise ValueError(f"HiFTStreamBatch.advance(): slot {slot}: frames [{lo}, {hi}) of row {src_row} are not in the mel batch")
            if self.state[slot][0] + k > self.max_frames:
                raise ValueError(f"HiFTStreamBatch.advance(): slot {slot}: {self.state[slot][0]} + {k} frames exceed max_frames = "
                                 f"{self.max_frames}")
        if not rows:
            return {}
        # ---- the step on the host: every slot's windows, as descriptors -------------------------------------------------------
        app, fgat, fcrop, frec, sapp, dmel, dsrc, wcrop = ([] for _ in range(8))
        lens_f, lens_d, lens_src, sample0 = [], [], [0] * self.slots, [0] * self.slots
        emit = {}      # slot -> (row of the decode batch or None, E, k_hi)
        for slot, src_row, lo, hi, final in rows:
            received, sourced, emitted = self.state[slot]
            k = 0 if src_row is None else hi - lo
            A, fwin, dwin = stream_step(received, sourced, emitted, k, final)
            if k > 0:
                app.append((src_row, lo, slot, received, k))
            if fwin is not None:
                f_lo, c0, c1 = fwin
                r = len(lens_f)
                lens_f.append(A - f_lo)
                fgat.append((slot, f_lo, r, 0, A - f_lo))
                fcrop.append((r, c0 - f_lo, slot, 0, c1 - c0))
                frec.append((slot, 0, slot, c0, c1 - c0))
                sapp.append((slot, 0, slot, up * c0, up * (c1 - c0)))
                lens_src[slot], sample0[slot] = c1 - c0, up * c0
                sourced = c1
            if dwin is not None:
                d_lo, d_hi, k0, k1 = dwin
                r = len(lens_d)
                lens_d.append(d_hi - d_lo)
                dmel.append((slot, d_lo, r, 0, d_hi - d_lo))
                dsrc.append((slot, up * d_lo, r, 0, up * (d_hi - d_lo)))
                wcrop.append((r, up * (k0 - d_lo), r, 0, up * (k1 - k0)))
                emit[slot] = (r, k0, k1)
                emitted = k1
            else:
                emit[slot] = (None, emitted, emitted)
            self.state[slot] = [A, sourced, emitted]
        sets = (app, fgat, fcrop, frec, sapp, dmel, dsrc, wcrop)
        n_desc = max(len(s) for s in sets)
        flat = []
        for s in sets:
            for d in s:
                flat.extend(d)
            flat.extend((0, 0, 0, 0, -1) * (n_desc - len(s)))      # (n < 0: a descriptor that moves nothing)
        ints = torch.tensor(flat + lens_f + lens_d + lens_src, dtype=torch.int32).to(dev)      # one copy up
        desc = ints[:8 * n_desc * 5].view(8, n_desc, 5)
        o = 8 * n_desc * 5
        lens_f_d, lens_d_d = ints[o:o + len(lens_f)], ints[o + len(lens_f):o + len(lens_f) + len(lens_d)]
        lens_src_d = ints[o + len(lens_f) + len(lens_d):]
        eng = self._hift._engine(self.slots, self.max_frames)      # (reserved at construction: no step rebuilds a context)

        def span(s):
            return max((d[4] for d in s), default=0)

        # ---- append, f0 and source of the frames whose f0 no later frame can change --------------------------------------------
        if app:
            eng.slab_copy(mel.to(device=dev, dtype=torch.float32).contiguous(), self.mel, desc[0, :len(app)], span(app))
        if fgat:
            Wf, Ts = span(fgat), span(fcrop)
            win = torch.empty(len(fgat), spec.N_FEATS, Wf, device=dev)
            eng.slab_copy(self.mel, win, desc[1, :len(fgat)], Wf, zero_fill=True)
            f0w = eng.hift_f0(win, lens_f_d)
            f0n = torch.empty(self.slots, Ts, device=dev)
            eng.slab_copy(f0w, f0n, desc[2, :len(fgat)], Ts, zero_fill=True)
            eng.slab_copy(f0n, self.f0, desc[3, :len(fgat)], Ts)
            s_new = torch.empty(self.slots, 1, up * Ts, device=dev)
            eng.hift_source_cont_rows(f0n, self.phase, self.seeds, self.calls, torch.tensor(sample0, dtype=torch.int64).to(dev),
                                      lens_src_d, self.cum, out=s_new)
            eng.slab_copy(s_new, self.source, desc[4, :len(fgat)], up * Ts)
        # ---- decode the frames that have a full halo of mel and source on their right -------------------------------------------
        out = None
        if dmel:
            Wd, K = span(dmel), span(wcrop) // up
            mwin = torch.empty(len(dmel), spec.N_FEATS, Wd, device=dev)
            swin = torch.empty(len(dmel), 1, up * Wd, device=dev)
            eng.slab_copy(self.mel, mwin, desc[5, :len(dmel)], Wd, zero_fill=True)
            eng.slab_copy(self.source, swin, desc[6, :len(dmel)], up * Wd, zero_fill=True)
            wav = eng.hift_decode(mwin, swin, lens_d_d)
            out = torch.empty(len(dmel), up * K, device=dev)
            eng.slab_copy(wav, out, desc[7, :len(dmel)], up * K, zero_fill=True)
        res = {}
        for slot, (r, k0, k1) in emit.items():
            wav = out[r:r + 1, :up * (k1 - k0)] if r is not None else torch.zeros(1, 0, device=dev)
            res[slot] = (wav, self.source[slot:slot + 1, :, up * k0:up * k1])
        return res
