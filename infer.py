#!/usr/bin/env python3
"""`infer.py`-compatible CLI for the MI355X-native synthesis path.

Flag names and defaults follow the reference CLI (infer.py:272-329 of indiejoseph/JyutVoice): --text/--lang/--phone/
--ref_audio/--output/--config/--tts_checkpoint/--flow_encoder/--speech_tokenizer/--campplus/--hift/--n_timesteps/
--length_scale (default 0.9).  What is in scope here is the call sequence of infer.py:341-351 and :419-441 --
load the two state-dicts, `tts.synthesise(...)`, `hift.inference(mel)`, write a 24 kHz wav.

The reference's front-ends are NOT part of this build: text -> ids needs its G2P stack
(pycantonese / pypinyin / g2p_en), and --ref_audio needs two external ONNX models (speech tokenizer, speaker embedding) and a
mel extractor.  Instead this CLI takes their outputs directly:

    --tokens tokens.json     {"x": [...], "lang": [...], "tone": [...], "word_pos": [...], "syllable_pos": [...]}
                             (equal-length int lists = the output contract of jyutvoice/text/__init__.py:20-35 after
                             `intersperse`; with "interspersed": false the raw text_to_sequence lists, which get their
                             blanks here -- jyutvoice_amd/utils/text.py validates either form), optionally
                             "spk_embed": [192 floats], and for voice cloning
                             "prompt_token": [speech-token ids] + either "prompt_feat": [[80 floats] per frame] or
                             "prompt_wav_24k": "ref_24k.wav" (16-bit mono; its mel is extracted on the GPU as
                             infer.py:386 does) or "prompt_wav": "ref.wav" (any rate, PCM or float, any number of channels:
                             read by jyutvoice_amd.utils.audio.load_wav and resampled to 24 kHz on the GPU as infer.py:368-382
                             does) -- what infer.py:386-392 gets from --ref_audio; the prompt encoder
                             (--flow_encoder) then runs on the GPU exactly as infer.py:390-392 runs it
                             A JSON *list* of such objects is synthesised as ONE batch, every utterance with its own
                             prompt of its own length (or none); the results go to OUTPUT with _000, _001, ... before the
                             extension.  Each utterance's prompt_h (2 frames per prompt token) and prompt mel are trimmed
                             to the shorter of the two first: the batch takes one prompt length per utterance
    --sample_rate R          write the audio at R Hz instead of 24000 (resampled on the GPU, the whole batch in one call)
    --prompt-trim-db DB      every "prompt_wav" / "prompt_wav_24k" recording is conditioned on the GPU, at its own rate, before the
    --prompt-peak V          resample, as the CosyVoice2 front-ends condition theirs: energy trim DB below the loudest frame (frame
    --prompt-tail SECONDS    440, hop 220), scaled down to a peak of V, SECONDS of silence appended (upstream: 60, 0.8, 0.2)
    --loudness LUFS          every output is brought to LUFS (ITU-R BS.1770-4 integrated loudness, measured and applied on the GPU
    [--peak V]               before the output resample), the gain limited so that no sample exceeds V; the measured loudness and the
                             applied gain are printed per output.  Not with --stream-hop: it needs the whole utterance
    --dump-ref-features DIR  every request with a "prompt_wav" (or "prompt_wav_24k") also gets what infer.py:98-163 feeds the two ONNX
                             front-ends from the recording's 16 kHz copy: DIR/ref_NNN_fbank.npy (kaldi fbank minus its mean over
                             frames, [T, 80]) and DIR/ref_NNN_logmel.npy (whisper log-mel, [128, T]), NNN the request's number; all
                             requests of a list in one GPU batch per feature (the ONNX sessions themselves are not loaded here)
    --token2wav list.json    speech tokens -> audio without the text side: CosyVoice2's token-to-mel flow (--flow flow.pt, the
                             1121-key CausalMaskedDiffWithXvec state-dict) and the vocoder.  A JSON list of requests, each
                             {"speech_token": [ids], "embedding": [192 floats]} plus optionally "prompt_token": [ids] and either
                             "prompt_feat": [[80 floats] per frame] or "prompt_wav": "ref.wav" (any rate) / "prompt_wav_24k"; the
                             list runs as ONE batch through inference(batched=True) and HiFTGenerator.inference and is written
                             to OUTPUT with _000, _001, ... before the extension.  A prompt mel longer than the request's
                             2 * tokens frames is trimmed to them.  --streaming: the chunk-causal masks of the encoder and the
                             estimator (streaming=True of flow.py:300-358).  With --synthetic 1: key-hashed weights.
    --stream-sessions S      with --token2wav --stream-hop K: the requests run through ONE server (jyutvoice_amd.stream.Token2WavServer),
                             S sessions at a time, each step one batched solve and one batched vocoder advance for all of them
    --stream-hop K           with --token2wav: every request runs through a streaming session of its own
                             (jyutvoice_amd.stream.Token2WavStream, always on the streaming masks), its tokens pushed K at a time;
                             the same files are written, and the time to the first audio is printed per request
    --synthetic N            no checkpoint / no tokens: N synthetic tokens, key-hashed weights (smoke / demo)
    --synthetic-prompt K     with --synthetic: also a synthetic K-token voice prompt through the prompt encoder
    --enc-attention MODE     text encoder attention: auto (four launches up to 512 tokens, one online-softmax launch above), fused
                             (that launch at every length) or gemm (the four launches; texts beyond 512 tokens fail)

With --text and no --tokens it explains what is missing instead of guessing.
"""
import argparse
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def write_wav(path: str, wav, sample_rate: int = 24000) -> None:
    """16-bit PCM mono wav (torchaudio is not available in this image; infer.py:441 uses torchaudio.save)"""
    import torch
    pcm = (wav.detach().cpu().flatten().clamp(-1, 1) * 32767.0).round().to(torch.int16).numpy().tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(pcm)) + b"WAVEfmt " +
                struct.pack("<IHHIIHH", 16, 1, 1, sample_rate, sample_rate * 2, 2, 16) + b"data" + struct.pack("<I", len(pcm)))
        f.write(pcm)


def read_wav_24k(path: str):
    """16-bit PCM mono 24 kHz wav -> [1, n] float in [-1, 1] (torchaudio.load + resampling of infer.py:368-382 are front-end)"""
    import torch
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise SystemExit(f"{path}: not a RIFF/WAVE file")
    pos, fmt, pcm = 12, None, None
    while pos + 8 <= len(data):
        tag, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        if tag == b"fmt ":
            fmt = struct.unpack("<HHIIHH", data[pos + 8:pos + 24])
        elif tag == b"data":
            pcm = data[pos + 8:pos + 8 + size]
        pos += 8 + size + (size & 1)
    if fmt is None or pcm is None or fmt[0] != 1 or fmt[1] != 1 or fmt[2] != 24000 or fmt[5] != 16:
        raise SystemExit(f"{path}: need 16-bit PCM, mono, 24 kHz (resample with the reference's front-end first)")
    return (torch.frombuffer(bytearray(pcm), dtype=torch.int16).float() / 32768.0).unsqueeze(0)


PROMPT_SOURCES = ("prompt_feat", "prompt_wav_24k", "prompt_wav")


def read_prompt_wav(tok):
    """the recording of a request, from `prompt_wav` (any format load_wav reads) or `prompt_wav_24k`: ([1, n] float, sample rate)"""
    if "prompt_wav" in tok:
        from jyutvoice_amd.utils.audio import load_wav
        try:
            return load_wav(tok["prompt_wav"])
        except (OSError, ValueError) as e:
            raise SystemExit(str(e))
    return read_wav_24k(tok["prompt_wav_24k"]), 24000


def prompt_conditioning(args):
    """the --prompt-* flags as condition_prompt's arguments, or None when none of them is given"""
    if args.prompt_trim_db is None and args.prompt_peak is None and args.prompt_tail is None:
        return None
    return dict(top_db=args.prompt_trim_db, peak=args.prompt_peak, tail_seconds=args.prompt_tail or 0.0)


def prompt_mels(recs, args, device):
    """the prompt mels of (recording, rate) pairs in one ragged pass at 24 kHz, conditioned first when a --prompt-* flag asks"""
    from jyutvoice_amd.utils.audio import condition_prompt, extract_speech_feat_batch
    wavs, rates = [w for w, _ in recs], [r for _, r in recs]
    cond = prompt_conditioning(args)
    if cond is None:
        return extract_speech_feat_batch(wavs, device, sample_rates=rates)
    try:
        rows, lens = condition_prompt(wavs, rates, device=device, **cond)
    except ValueError as e:
        raise SystemExit(str(e))
    return extract_speech_feat_batch(rows, device, sample_rates=rates, lengths=lens)


def output_loudness(wav, samples, args, first=0):
    """--loudness: wav [B, n] at 24 kHz, utterance b in [:samples[b]] -> the same batch at args.loudness LUFS (one set of calls)"""
    if args.loudness is None:
        return wav
    from jyutvoice_amd.utils.audio import normalize_loudness
    wav, lufs, gain = normalize_loudness(wav, 24000, args.loudness, args.peak, lens=samples)
    for b, (l, g) in enumerate(zip(lufs.tolist(), gain.tolist())):
        print(f"output {first + b}: measured {l:.2f} LUFS, gain {g:.4f}")
    return wav


def dump_ref_features(toks, args, device):
    """--dump-ref-features: the speaker fbank and the tokenizer log-mel of every request's recording, one ragged batch per feature"""
    import numpy as np

    from jyutvoice_amd.utils.audio import extract_spk_feat_batch, extract_token_feat_batch
    idx = [b for b, t in enumerate(toks) if "prompt_wav" in t or "prompt_wav_24k" in t]
    if not idx:
        return
    recs = [read_prompt_wav(toks[b]) for b in idx]
    wavs, rates = [w for w, _ in recs], [r for _, r in recs]
    try:
        fb, fb_len = extract_spk_feat_batch(wavs, rates, device)
        lm, lm_len = extract_token_feat_batch(wavs, rates, device)
    except ValueError as e:
        raise SystemExit(f"--dump-ref-features: {e}")
    os.makedirs(args.dump_ref_features, exist_ok=True)
    for i, b in enumerate(idx):
        stem = os.path.join(args.dump_ref_features, f"ref_{b:03d}")
        np.save(stem + "_fbank.npy", fb[i, : int(fb_len[i])].cpu().numpy())
        np.save(stem + "_logmel.npy", lm[i, :, : int(lm_len[i])].cpu().numpy())
    print(f"Reference features of {len(idx)} recordings saved to: {args.dump_ref_features}")


def guidance_kw(args, decoder):
    """--cfg-rate / --cfg-window / --t-scheduler / --solver as the keywords of synthesise(), of the flow's inference calls and of the
    streaming sessions.  A flag that was not given says nothing: `decoder`'s own inference_cfg_rate / t_scheduler / solver hold (the
    window is placed on the t of the schedule the solve will run)."""
    from jyutvoice_amd.flow.flow_matching import decoder_settings
    kw = {}
    if args.t_scheduler is not None:
        kw["t_scheduler"] = args.t_scheduler
    if args.solver is not None:
        kw["solver"] = args.solver
    if args.cfg_window is not None:
        from jyutvoice_amd.serve import guidance_rates
        conf_rate, conf_sched, _ = decoder_settings(decoder)
        try:
            kw["cfg_schedule"] = guidance_rates(args.n_timesteps, conf_rate if args.cfg_rate is None else args.cfg_rate,
                                                tuple(args.cfg_window), args.t_scheduler or conf_sched)
        except ValueError as e:
            raise SystemExit(f"--cfg-rate / --cfg-window: {e}")
    elif args.cfg_rate is not None:
        kw["cfg_rate"] = args.cfg_rate
    return kw


def synthesise_list(toks, args, tts, hift, device):
    """--tokens with a JSON list: all utterances in one batch through synthesise(batched=True, prompt_lengths=...)"""
    import torch

    from jyutvoice_amd.utils.prompt import pad_prompts
    from jyutvoice_amd.utils.text import FIELDS, load_tokens_json
    B = len(toks)
    if B == 0:
        raise SystemExit(f"{args.tokens}: empty list")
    if args.dump_ref_features:
        dump_ref_features(toks, args, device)
    try:
        ids = [load_tokens_json(t) for t in toks]
    except ValueError as e:
        raise SystemExit(str(e))
    x_lengths = torch.cat([i["x_lengths"] for i in ids])
    Tt = int(x_lengths.max())
    batch = {k: torch.zeros(B, Tt, dtype=torch.int64) for k in FIELDS}
    for b, i in enumerate(ids):
        for k in FIELDS:
            batch[k][b, : i[k].shape[1]] = i[k][0]
    spk = torch.cat([torch.tensor(t["spk_embed"], dtype=torch.float32).view(1, 192) if "spk_embed" in t else torch.randn(1, 192)
                     for t in toks])
    # prompts: the prompt encoder on the ragged token batch, the prompt mels of all recordings in one ragged pass
    empty = torch.zeros(0, 80)
    feats, hs = [empty] * B, [empty] * B
    with_prompt = [b for b, t in enumerate(toks) if "prompt_token" in t and any(k in t for k in PROMPT_SOURCES)]
    if with_prompt:
        from jyutvoice_amd.flow.encoder import load_flow_encoder
        from jyutvoice_amd.utils.audio import extract_speech_feat_batch
        if args.synthetic:
            from jyutvoice_amd import synth
            from jyutvoice_amd.flow.encoder import FlowEncoder
            flow_encoder = FlowEncoder(device=device)
            flow_encoder.load_state_dict(synth.prompt_state_dict())
        else:
            print(f"Loading flow encoder from {args.flow_encoder}...")
            flow_encoder = load_flow_encoder(args.flow_encoder, device)
        plens = torch.tensor([len(toks[b]["prompt_token"]) for b in with_prompt], dtype=torch.int64)
        ptok = torch.zeros(len(with_prompt), int(plens.max()), dtype=torch.int64)
        for i, b in enumerate(with_prompt):
            ptok[i, : plens[i]] = torch.tensor(toks[b]["prompt_token"], dtype=torch.int64)
        h, h_len = flow_encoder(ptok, plens)
        from_wav = [b for b in with_prompt if "prompt_wav_24k" in toks[b] or "prompt_wav" in toks[b]]
        if from_wav and (any("prompt_wav" in toks[b] for b in from_wav) or prompt_conditioning(args)):
            # recordings at rates of their own: grouped by rate, (conditioned and) resampled on the GPU
            mel, mel_len = prompt_mels([read_prompt_wav(toks[b]) for b in from_wav], args, device)
        elif from_wav:
            mel, mel_len = extract_speech_feat_batch([read_wav_24k(toks[b]["prompt_wav_24k"]) for b in from_wav], device)
        for i, b in enumerate(with_prompt):
            if b in from_wav:
                j = from_wav.index(b)
                f = mel[j, : int(mel_len[j])]
            else:
                f = torch.tensor(toks[b]["prompt_feat"], dtype=torch.float32).view(-1, 80)
            n_h, n_f = 2 * int(plens[i]), f.shape[0]
            p = min(n_h, n_f)
            if n_h != n_f:
                print(f"utterance {b}: prompt_h has {n_h} frames, the prompt mel {n_f}: both trimmed to {p}")
            feats[b], hs[b] = f[:p].cpu(), h[i, :p].cpu()
    if args.inflight:
        return synthesise_inflight(toks, ids, spk, feats, hs, args, tts, hift)
    prompt_feat, prompt_h, prompt_lengths = pad_prompts(feats, hs)

    print(f"Running TTS synthesis of {B} utterances as one batch...")
    start = time.time()
    result = tts.synthesise(x=batch["x"], x_lengths=x_lengths, lang=batch["lang"], tone=batch["tone"], word_pos=batch["word_pos"],
                            syllable_pos=batch["syllable_pos"], prompt_feat=prompt_feat, prompt_h=prompt_h, spk_embed=spk,
                            n_timesteps=args.n_timesteps, length_scale=args.length_scale, batched=True,
                            prompt_lengths=prompt_lengths, **guidance_kw(args, tts.decoder))
    wav, _ = hift.inference(result["mel"], lengths=result["mel_lengths"])
    torch.cuda.synchronize()
    print(f"Synthesis time: {time.time() - start:.2f} s (rtf of synthesise(): {result['rtf']:.4f})")
    samples = result["mel_lengths"] * 480
    dump_mels(args, [result["mel"][b, :, :n] for b, n in enumerate(result["mel_lengths"].tolist())])
    wav = output_loudness(wav, samples, args)
    if args.sample_rate != 24000:      # the whole batch in one ragged call, each utterance at its own length
        from jyutvoice_amd.utils.audio import resample
        wav, samples = resample(wav, 24000, args.sample_rate, lengths=samples)
    stem, ext = os.path.splitext(args.output)
    for b, n in enumerate(samples.tolist()):
        path = f"{stem}_{b:03d}{ext}"
        write_wav(path, wav[b, :n], args.sample_rate)
        print(f"Generated audio saved to: {path} ({n / args.sample_rate:.2f} seconds)")


def dump_mels(args, mels):
    """--dump-mel: mel b [80, y_b] -> DIR/mel_NNN.npy"""
    if not args.dump_mel:
        return
    import numpy as np
    os.makedirs(args.dump_mel, exist_ok=True)
    for b, m in enumerate(mels):
        np.save(os.path.join(args.dump_mel, f"mel_{b:03d}.npy"), m.cpu().numpy())


def synthesise_inflight(toks, ids, spk, feats, hs, args, tts, hift):
    """--tokens list.json --inflight S: the list through one SynthServer with at most S resident requests, a new request submitted
    every --arrive-every steps; the same out_NNN files as the list route.  A request's own "n_timesteps", "temperature",
    "length_scale", "seed", "cfg_rate", "cfg_window" and "solver" keys override the command line's (seed: --seed + its index)."""
    import torch

    from jyutvoice_amd.serve import SynthServer
    B = len(toks)
    if args.inflight < 1 or args.arrive_every < 1:
        raise SystemExit("--inflight and --arrive-every must be positive")
    tokens = max(i["x"].shape[1] for i in ids)
    # the pool's frame capacity is fixed up front, before any duration is known: room for 20 frames per token behind the longest prompt
    frames = max(f.shape[0] for f in feats) + 20 * tokens
    server = SynthServer(tts, hift, max_sessions=min(args.inflight, B), max_frames=frames, max_tokens=tokens)
    print(f"Serving {B} requests through {server.max_sessions} slots, one arrival every {args.arrive_every} step(s)...")
    start, out, step = time.time(), {}, 0
    while len(out) < B:
        b = step // args.arrive_every
        if step % args.arrive_every == 0 and b < B:
            t, p = toks[b], feats[b].shape[0]
            try:
                i = ids[b]
                server.submit(i["x"], i["x_lengths"], i["lang"], i["tone"], i["word_pos"], i["syllable_pos"], spk[b:b + 1],
                              prompt_feat=feats[b][None] if p else None, prompt_h=hs[b][None] if p else None,
                              n_timesteps=int(t.get("n_timesteps", args.n_timesteps)), temperature=float(t.get("temperature", 1.0)),
                              length_scale=float(t.get("length_scale", args.length_scale)), seed=int(t.get("seed", args.seed + b)),
                              loudness=args.loudness, peak=args.peak, cfg_rate=t.get("cfg_rate", args.cfg_rate),
                              cfg_window=t.get("cfg_window", args.cfg_window), t_scheduler=args.t_scheduler,
                              solver=t.get("solver", args.solver))
            except ValueError as e:
                raise SystemExit(f"{args.tokens}: {e}")
        out.update(server.step())
        step += 1
    torch.cuda.synchronize()
    print(f"Synthesis time: {time.time() - start:.2f} s over {server.steps} pool steps")
    bad = {rid: r["error"] for rid, r in out.items() if "error" in r}
    if bad:
        raise SystemExit(f"{args.tokens}: " + "; ".join(bad.values()))
    dump_mels(args, [out[b]["mel"][0] for b in range(B)])
    stem, ext = os.path.splitext(args.output)
    for b in range(B):
        wav, n = out[b]["wav"], 480 * out[b]["mel_length"]
        if "lufs" in out[b]:
            print(f"output {b}: measured {out[b]['lufs']:.2f} LUFS, gain {out[b]['gain']:.4f}")
        if args.sample_rate != 24000:
            from jyutvoice_amd.utils.audio import resample
            wav, lens = resample(wav, 24000, args.sample_rate, lengths=torch.tensor([n]))
            n = int(lens[0])
        path = f"{stem}_{b:03d}{ext}"
        write_wav(path, wav[0, :n], args.sample_rate)
        print(f"Generated audio saved to: {path} ({n / args.sample_rate:.2f} seconds)")


def token2wav_list(reqs, args, device):
    """--token2wav: speech tokens (+ voice prompt) -> mel -> wav for a JSON list of requests, as one batch"""
    import torch

    import jyutvoice_amd
    from jyutvoice_amd import synth
    from jyutvoice_amd.flow.flow import CausalMaskedDiffWithXvec, load_flow
    if not isinstance(reqs, list) or not reqs:
        raise SystemExit(f"{args.token2wav}: need a non-empty JSON list of requests")
    B = len(reqs)
    for b, r in enumerate(reqs):
        if "speech_token" not in r or "embedding" not in r or len(r["embedding"]) != 192:
            raise SystemExit(f"{args.token2wav}: request {b}: needs \"speech_token\" and an \"embedding\" of 192 floats")
    _, hift = jyutvoice_amd.build_default(device)
    # the flow's decoder takes the slots a JyutVoiceTTS would: a process that already holds one on this device (a caller of main())
    # gives the flow a runtime of its own
    from jyutvoice_amd.engine import JV_MODEL_TTS
    from jyutvoice_amd.runtime import Runtime, get_runtime
    rt = Runtime(str(device)) if JV_MODEL_TTS in get_runtime(device).sds else None
    if rt is not None:
        rt.set_precision(args.estimator_precision)
    if args.synthetic:
        flow = CausalMaskedDiffWithXvec(vocab_size=6561, input_frame_rate=25, device=device, runtime=rt)
        sd = synth.prompt_state_dict()
        sd.update({k: v for k, v in synth.tts_state_dict().items() if k.startswith(("decoder.", "spk_embed_affine_layer."))})
        flow.load_state_dict(sd)
        hift.load_state_dict(synth.hift_state_dict())
    else:
        print(f"Loading flow from {args.flow}...")
        flow = load_flow(args.flow, device, runtime=rt)
        print(f"Loading HiFT vocoder from {args.hift}...")
        hift.load_state_dict(torch.load(args.hift, map_location="cpu"))
    hift = hift.eval().to(device)
    hift.manual_seed(args.seed)

    def pad_ids(key):
        lens = torch.tensor([len(r.get(key, [])) for r in reqs], dtype=torch.int64)
        out = torch.zeros(B, int(lens.max()), dtype=torch.int64)
        for b, r in enumerate(reqs):
            out[b, : lens[b]] = torch.tensor(r.get(key, []), dtype=torch.int64)
        return out, lens

    token, token_len = pad_ids("speech_token")
    prompt_token, prompt_token_len = pad_ids("prompt_token")
    embedding = torch.tensor([r["embedding"] for r in reqs], dtype=torch.float32)
    # prompt mels: given, or extracted from the recordings in one ragged GPU pass (at their own rates)
    feats = [torch.zeros(0, 80)] * B
    from_wav = [b for b, r in enumerate(reqs) if "prompt_wav" in r or "prompt_wav_24k" in r]
    if from_wav:
        mel, mel_len = prompt_mels([read_prompt_wav(reqs[b]) for b in from_wav], args, device)
        for j, b in enumerate(from_wav):
            feats[b] = mel[j, : int(mel_len[j])].cpu()
    for b, r in enumerate(reqs):
        if b not in from_wav and "prompt_feat" in r:
            feats[b] = torch.tensor(r["prompt_feat"], dtype=torch.float32).view(-1, 80)
        limit = 2 * int(prompt_token_len[b] + token_len[b])
        if feats[b].shape[0] > limit:
            print(f"request {b}: the prompt mel has {feats[b].shape[0]} frames, the utterance {limit}: trimmed")
            feats[b] = feats[b][:limit]
    feat_len = torch.tensor([f.shape[0] for f in feats], dtype=torch.int32)
    prompt_feat = torch.zeros(B, int(feat_len.max()), 80)
    for b, f in enumerate(feats):
        prompt_feat[b, : f.shape[0]] = f

    if args.stream_sessions and not args.stream_hop:
        raise SystemExit("--stream-sessions needs --stream-hop")
    if args.stream_hop and args.stream_sessions:
        wav, samples = token2wav_server(args, flow, hift, token, token_len, prompt_token, prompt_token_len, prompt_feat, feat_len,
                                        embedding)
    elif args.stream_hop:
        wav, samples = token2wav_sessions(args, flow, hift, token, token_len, prompt_token, prompt_token_len, prompt_feat, feat_len,
                                          embedding)
    else:
        print(f"Running token-to-mel of {B} requests as one batch" + (" (streaming masks)" if args.streaming else "") + "...")
        start = time.time()
        try:
            mel, _ = flow.inference(token, token_len, prompt_token, prompt_token_len, prompt_feat, feat_len, embedding, args.streaming,
                                    True, batched=True, n_timesteps=args.n_timesteps, **guidance_kw(args, flow.decoder))
        except ValueError as e:
            raise SystemExit(f"{args.token2wav}: {e}")
        wav, _ = hift.inference(mel, lengths=flow.mel_lengths)
        torch.cuda.synchronize()
        print(f"Synthesis time: {time.time() - start:.2f} s")
        samples = flow.mel_lengths.to(torch.int64) * 480
    wav = output_loudness(wav, samples, args)
    if args.sample_rate != 24000:
        from jyutvoice_amd.utils.audio import resample
        wav, samples = resample(wav, 24000, args.sample_rate, lengths=samples)
    stem, ext = os.path.splitext(args.output)
    for b, n in enumerate(samples.tolist()):
        path = f"{stem}_{b:03d}{ext}"
        write_wav(path, wav[b, :n], args.sample_rate)
        print(f"Generated audio saved to: {path} ({n / args.sample_rate:.2f} seconds)")


def token2wav_sessions(args, flow, hift, token, token_len, prompt_token, prompt_token_len, prompt_feat, feat_len, embedding):
    """--stream-hop K: one Token2WavStream per request, its tokens pushed K at a time -> (wav [B, longest], samples [B])"""
    import torch

    from jyutvoice_amd.stream import Token2WavStream
    if args.stream_hop < 1:
        raise SystemExit("--stream-hop must be positive")
    if not args.streaming:
        print("--stream-hop: a session always runs on the streaming masks (--streaming is implied)")
    pieces_all = []
    for b in range(token.shape[0]):
        n, p, f = int(token_len[b]), int(prompt_token_len[b]), int(feat_len[b])
        start = time.time()
        first = None
        try:
            session = Token2WavStream(flow, hift, prompt_token[b:b + 1, :p], prompt_feat[b:b + 1, :f], embedding[b:b + 1], max(n, 1),
                                      n_timesteps=args.n_timesteps, **guidance_kw(args, flow.decoder))
            pieces = []
            for i in range(0, n, args.stream_hop):
                pieces.append(session.push(token[b, i:min(i + args.stream_hop, n)]))
                if first is None and pieces[-1].shape[1] > 0:
                    torch.cuda.synchronize()
                    first = time.time() - start
            pieces.append(session.finish())
        except ValueError as e:
            raise SystemExit(f"{args.token2wav}: request {b}: {e}")
        torch.cuda.synchronize()
        total = time.time() - start
        first = total if first is None else first
        print(f"request {b}: {n} tokens in hops of {args.stream_hop}: first audio after {first:.3f} s, all of it after {total:.3f} s")
        pieces_all.append(torch.cat(pieces, dim=1)[0])
    samples = torch.tensor([w.shape[0] for w in pieces_all], dtype=torch.int64)
    wav = torch.zeros(len(pieces_all), int(samples.max()), device=pieces_all[0].device)
    for b, w in enumerate(pieces_all):
        wav[b, : w.shape[0]] = w
    return wav, samples


def token2wav_server(args, flow, hift, token, token_len, prompt_token, prompt_token_len, prompt_feat, feat_len, embedding):
    """--stream-hop K --stream-sessions S: the requests through ONE Token2WavServer, S sessions at a time, every live session
    receiving K tokens per step -> (wav [B, longest], samples [B]).  A request takes a slot as soon as one is free."""
    import torch

    from jyutvoice_amd.stream import Token2WavServer
    if args.stream_hop < 1 or args.stream_sessions < 1:
        raise SystemExit("--stream-hop and --stream-sessions must be positive")
    if not args.streaming:
        print("--stream-hop: a session always runs on the streaming masks (--streaming is implied)")
    B = token.shape[0]
    try:
        server = Token2WavServer(flow, hift, min(args.stream_sessions, B), max(int(token_len.max()), 1), n_timesteps=args.n_timesteps,
                                 max_prompt_tokens=max(int(prompt_token_len.max()), (int(feat_len.max()) + 1) // 2), **guidance_kw(args, flow.decoder))
    except ValueError as e:
        raise SystemExit(f"{args.token2wav}: {e}")
    pieces, live, pos, waiting, steps = [[] for _ in range(B)], {}, {}, list(range(B)), 0
    start = time.time()
    while waiting or live:
        try:
            while waiting and len(live) < server.max_sessions:
                b = waiting.pop(0)
                p, f = int(prompt_token_len[b]), int(feat_len[b])
                live[b] = server.open(prompt_token[b:b + 1, :p], prompt_feat[b:b + 1, :f], embedding[b:b + 1])
                pos[b] = 0
            for b, sid in live.items():
                n = int(token_len[b])
                if pos[b] < n:
                    server.push(sid, token[b, pos[b]:min(pos[b] + args.stream_hop, n)])
                    pos[b] = min(pos[b] + args.stream_hop, n)
                else:
                    server.close(sid)
            out = server.step()
        except ValueError as e:
            raise SystemExit(f"{args.token2wav}: {e}")
        steps += 1
        for b, sid in list(live.items()):
            if sid in out:
                pieces[b].append(out[sid])
            if server.finished(sid):
                del live[b]
    torch.cuda.synchronize()
    print(f"{B} requests, {server.max_sessions} sessions at a time, hops of {args.stream_hop}: {steps} steps in {time.time() - start:.3f} s")
    waves = [torch.cat(p, dim=1)[0] for p in pieces]
    samples = torch.tensor([w.shape[0] for w in waves], dtype=torch.int64)
    wav = torch.zeros(B, int(samples.max()), device=waves[0].device)
    for b, w in enumerate(waves):
        wav[b, : w.shape[0]] = w
    return wav, samples


def main(argv=None):
    p = argparse.ArgumentParser(description="JyutVoice TTS inference on MI355X (jyutvoice_amd)")
    p.add_argument("--text", default=None, help="Text to synthesize (needs the reference's G2P front-end; see --tokens)")
    p.add_argument("--lang", default=None, choices=["en", "zh", "yue", "multilingual"], help="Language of the text")
    p.add_argument("--phone", default=None, help="Phonetic transcription (for Cantonese, optional)")
    p.add_argument("--ref_audio", default=None, help="Reference audio (needs the reference's ONNX front-ends; see --tokens)")
    p.add_argument("--output", required=True, help="Output audio file path")
    p.add_argument("--config", default="configs/base.yaml", help="accepted for compatibility; the base.yaml constants are built in")
    p.add_argument("--tts_checkpoint", default="pretrained_models/epoch=0-step=55872.ckpt", help="Path to TTS model checkpoint")
    p.add_argument("--flow_encoder", default="pretrained_models/flow_encoder.pt", help="Path to flow encoder weights (voice prompt)")
    p.add_argument("--speech_tokenizer", default="pretrained_models/speech_tokenizer_v2.onnx", help="unused (front-end)")
    p.add_argument("--campplus", default="pretrained_models/campplus.onnx", help="unused (front-end)")
    p.add_argument("--hift", default="pretrained_models/hift.pt", help="Path to HiFT vocoder weights")
    p.add_argument("--n_timesteps", type=int, default=10, help="Number of diffusion timesteps")
    p.add_argument("--length_scale", type=float, default=0.9, help="Length scale for speech duration control")
    p.add_argument("--tokens", default=None, help="JSON with the five id lists (and optionally spk_embed)")
    p.add_argument("--token2wav", default=None, metavar="LIST.json",
                   help="JSON list of {speech_token, embedding[, prompt_token, prompt_feat | prompt_wav]}: token-to-mel flow + vocoder")
    p.add_argument("--flow", default="pretrained_models/flow.pt", help="Path to the CosyVoice2 flow weights (--token2wav)")
    p.add_argument("--streaming", action="store_true", help="--token2wav: chunk-causal masks in the flow encoder and the estimator")
    p.add_argument("--stream-hop", type=int, default=0, metavar="K",
                   help="--token2wav: a streaming session per request, its tokens pushed K at a time")
    p.add_argument("--stream-sessions", type=int, default=0, metavar="S",
                   help="--token2wav --stream-hop K: serve the list through one Token2WavServer, S sessions at a time")
    p.add_argument("--inflight", type=int, default=0, metavar="S",
                   help="--tokens with a JSON list: serve the list through one SynthServer with at most S resident requests (in-flight "
                        "batching); a request may carry its own n_timesteps, temperature, length_scale and seed keys")
    p.add_argument("--arrive-every", type=int, default=1, metavar="K", help="--inflight: a new request is submitted every K steps")
    p.add_argument("--dump-mel", default=None, metavar="DIR", help="--tokens with a JSON list: also save every mel as DIR/mel_NNN.npy")
    p.add_argument("--synthetic", type=int, default=0, help="use N synthetic tokens and synthetic weights (with a --tokens list: the "
                                                            "synthetic weights and the list's utterances)")
    p.add_argument("--synthetic-prompt", type=int, default=0, help="with --synthetic: K synthetic prompt tokens (voice-cloning path)")
    p.add_argument("--estimator-precision", default="fp32", choices=["fp32", "fp16"],
                   help="fp16: the CFM estimator as the reference's fp16 TensorRT plan runs it (fp16 operands, fp32 accumulation); "
                        "encoders and vocoder unchanged (every route: ids, --token2wav, streaming, server)")
    p.add_argument("--enc-attention", default="auto", choices=["auto", "fused", "gemm"],
                   help="text encoder attention: auto = four launches around a score buffer up to 512 tokens, one online-softmax "
                        "launch above; fused = that launch at every length; gemm = the four launches (texts beyond 512 tokens fail)")
    p.add_argument("--cfg-rate", type=float, default=None, metavar="R",
                   help="classifier-free-guidance rate of the CFM solve, >= 0 (default: the decoder's inference_cfg_rate, 0.7); 0 runs "
                        "the solve without unconditional twins.  Every mode takes it")
    p.add_argument("--cfg-window", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="guide only the Euler steps whose t lies in [LO, HI); the others run at rate 0, without twins")
    p.add_argument("--t-scheduler", default=None, choices=["cosine", "linear"],
                   help="time schedule of the Euler steps (default: the decoder's t_scheduler, cosine in configs/base.yaml)")
    p.add_argument("--solver", default=None, choices=["euler", "midpoint", "heun"],
                   help="integrator of the CFM solve (default: the decoder's, euler): midpoint and heun take --n_timesteps second-order "
                        "steps of two estimator evaluations each.  Every mode that takes --cfg-rate takes it; with --inflight a request "
                        "of the list may carry its own \"solver\"")
    p.add_argument("--seed", type=int, default=0, help="seed of the vocoder's source-noise draws")
    p.add_argument("--sample_rate", type=int, default=24000, help="sample rate of the written audio (resampled on the GPU)")
    p.add_argument("--dump-ref-features", default=None, metavar="DIR",
                   help="also write each request's reference-recording features (fbank, whisper log-mel) as .npy files into DIR")
    p.add_argument("--prompt-trim-db", type=float, default=None, metavar="DB",
                   help="trim each prompt recording's leading / trailing silence, DB below its loudest frame (upstream: 60)")
    p.add_argument("--prompt-peak", type=float, default=None, metavar="V",
                   help="scale a prompt recording down to a peak of V when it exceeds it (upstream: 0.8)")
    p.add_argument("--prompt-tail", type=float, default=None, metavar="SECONDS",
                   help="append SECONDS of silence to each prompt recording (upstream: 0.2)")
    p.add_argument("--loudness", type=float, default=None, metavar="LUFS",
                   help="bring every output to LUFS (ITU-R BS.1770-4 integrated loudness), on the GPU, before the output resample")
    p.add_argument("--peak", type=float, default=None, metavar="V", help="--loudness: limit the gain so that no sample exceeds V")
    args = p.parse_args(argv)
    if args.loudness is not None and (args.stream_hop or args.stream_sessions):
        p.error("--loudness cannot be combined with --stream-hop / --stream-sessions: integrated loudness needs the whole utterance, "
                "and a streaming session hands its audio out piece by piece")
    if args.peak is not None and args.loudness is None:
        p.error("--peak limits the gain of --loudness: give --loudness LUFS too")
    if args.loudness is not None and not abs(args.loudness) < float("inf"):
        p.error("--loudness must be finite")
    for name in ("peak", "prompt_peak", "prompt_trim_db"):
        v = getattr(args, name)
        if v is not None and not 0 < v < float("inf"):
            p.error(f"--{name.replace('_', '-')} must be positive and finite")
    if args.prompt_tail is not None and not 0 <= args.prompt_tail < float("inf"):
        p.error("--prompt-tail must be >= 0 and finite")
    if args.sample_rate <= 0:
        raise SystemExit("--sample_rate must be positive")
    if args.sample_rate != 24000:      # a rate whose filter table the library refuses: say so before anything is loaded
        from jyutvoice_amd import _lib
        if _lib.load().jv_resample_table(24000, args.sample_rate, None, 0, None, None, None) != 0:
            raise SystemExit("--sample_rate: " + _lib.load().jv_last_error().decode("utf-8", "replace"))

    import torch

    import jyutvoice_amd
    from jyutvoice_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("no AMD GPU visible: jyutvoice_amd has no CPU path")
    device = torch.device("cuda:0")
    print(f"Using device: {device} ({torch.cuda.get_device_name(0)})")
    from jyutvoice_amd.runtime import get_runtime
    get_runtime(device).set_precision(args.estimator_precision)      # every route below runs on this runtime's context
    get_runtime(device).set_encoder_attention(args.enc_attention)
    if args.token2wav:
        return token2wav_list(json.load(open(args.token2wav)), args, device)
    tts, hift = jyutvoice_amd.build_default(device)

    prompt_feat = prompt_h = None
    if args.inflight and not args.tokens:
        raise SystemExit("--inflight needs --tokens with a JSON list")
    if args.synthetic:
        tts.load_state_dict(synth.tts_state_dict())
        hift.load_state_dict(synth.hift_state_dict())
        if args.tokens and isinstance(json.load(open(args.tokens)), list):      # synthetic weights, the list's utterances
            hift.manual_seed(args.seed)
            return synthesise_list(json.load(open(args.tokens)), args, tts.eval().to(device), hift.eval().to(device), device)
        u = synth.batch(1, args.synthetic)
        ids = {k: u[k] for k in ("x", "lang", "tone", "word_pos", "syllable_pos")}
        spk = u["spk_embed"]
        if args.synthetic_prompt:
            from jyutvoice_amd.flow.encoder import FlowEncoder
            flow_encoder = FlowEncoder(device=device)
            flow_encoder.load_state_dict(synth.prompt_state_dict())
            ptok, plen = synth.prompt_tokens(1, args.synthetic_prompt)
            prompt_h, _ = flow_encoder(ptok, plen)
            prompt_feat = torch.randn(1, 2 * args.synthetic_prompt, 80, generator=torch.Generator().manual_seed(args.seed))
    else:
        if not args.tokens:
            raise SystemExit("--text/--ref_audio need the reference's G2P and ONNX front-ends, which are outside this build; "
                             "pass --tokens tokens.json (five id lists [+ spk_embed]) or --synthetic N")
        print(f"Loading TTS model from {args.tts_checkpoint}...")
        ckpt = torch.load(args.tts_checkpoint, map_location="cpu", weights_only=False)
        tts.load_state_dict(ckpt["state_dict"] if "state_dict" in ckpt else ckpt)
        print(f"Loading HiFT vocoder from {args.hift}...")
        hift.load_state_dict(torch.load(args.hift, map_location="cpu"))
        from jyutvoice_amd.utils.text import load_tokens_json
        tok = json.load(open(args.tokens))
        if isinstance(tok, list):
            hift.manual_seed(args.seed)
            return synthesise_list(tok, args, tts.eval().to(device), hift.eval().to(device), device)
        try:      # the contract of get_text (infer.py:189-206): equal lengths, ids inside the embedding tables, blanks in place
            ids = load_tokens_json(tok)
        except ValueError as e:
            raise SystemExit(str(e))
        spk = torch.tensor(tok["spk_embed"], dtype=torch.float32).view(1, 192) if "spk_embed" in tok else torch.randn(1, 192)
        if args.dump_ref_features:
            dump_ref_features([tok], args, device)
        if "prompt_token" in tok and any(k in tok for k in PROMPT_SOURCES):   # infer.py:386-392
            from jyutvoice_amd.flow.encoder import load_flow_encoder
            print(f"Loading flow encoder from {args.flow_encoder}...")
            flow_encoder = load_flow_encoder(args.flow_encoder, device)
            ptok = torch.tensor(tok["prompt_token"], dtype=torch.int64).view(1, -1)
            prompt_h, _ = flow_encoder(ptok, torch.tensor([ptok.shape[1]], dtype=torch.int64))
            if ("prompt_wav" in tok or "prompt_wav_24k" in tok) and prompt_conditioning(args):
                mel, mel_len = prompt_mels([read_prompt_wav(tok)], args, device)
                prompt_feat = mel[:, : int(mel_len[0])]
            elif "prompt_wav" in tok:      # infer.py:368-382: the recording at its own rate -> 24 kHz on the GPU
                from jyutvoice_amd.utils.audio import extract_speech_feat, resample
                speech, rate = read_prompt_wav(tok)
                prompt_feat, _ = extract_speech_feat(resample(speech, rate, 24000, device=device), device)
            elif "prompt_wav_24k" in tok:
                from jyutvoice_amd.utils.audio import extract_speech_feat
                prompt_feat, _ = extract_speech_feat(read_wav_24k(tok["prompt_wav_24k"]), device)
            else:
                prompt_feat = torch.tensor(tok["prompt_feat"], dtype=torch.float32).view(1, -1, 80)
    tts = tts.eval().to(device)
    hift = hift.eval().to(device)
    hift.manual_seed(args.seed)
    x_lengths = torch.tensor([ids["x"].shape[1]], dtype=torch.int64)

    print("Running TTS synthesis...")
    start = time.time()
    result = tts.synthesise(x=ids["x"], x_lengths=x_lengths, lang=ids["lang"], tone=ids["tone"], word_pos=ids["word_pos"],
                            syllable_pos=ids["syllable_pos"], prompt_feat=prompt_feat, prompt_h=prompt_h, spk_embed=spk,
                            n_timesteps=args.n_timesteps, length_scale=args.length_scale, **guidance_kw(args, tts.decoder))
    wav, _ = hift.inference(result["mel"])
    torch.cuda.synchronize()
    print(f"Synthesis time: {time.time() - start:.2f} s (rtf of synthesise(): {result['rtf']:.4f})")
    wav = output_loudness(wav, None, args)
    if args.sample_rate != 24000:
        from jyutvoice_amd.utils.audio import resample
        wav = resample(wav, 24000, args.sample_rate)
    print(f"Saving audio to {args.output}...")
    write_wav(args.output, wav[0], args.sample_rate)
    print(f"Generated audio saved to: {args.output}")
    print(f"Audio duration: {wav.shape[1] / args.sample_rate:.2f} seconds")


if __name__ == "__main__":
    main()
