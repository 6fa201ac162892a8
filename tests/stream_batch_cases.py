"""Shared by test_stream_batch_host.py and test_gpu_stream_batch.py (a plain module, not a conftest): the sessions of the server
cases, the timeline that mixes them, and drivers that play the timeline into a `Token2WavServer` and into one `Token2WavStream` per
session.

Three sessions (P prompt tokens, F prompt frames, tokens, hop) = (0, 0, 53, 21), (10, 20, 77, 25), (7, 14, 40, 13) opened at
different steps, and a fourth short one that takes the slot the first leaves.  The timeline is the smallest in which one step mixes
every kind of row: a chunk of 25 + 3 tokens, a session with nothing due (its aligned prefix has not grown: it is not in the batch), a
final solve (ctx = 0) beside push solves (ctx = 3), a session that closes while the others are in mid-stream, a reused slot."""
import torch

SESSIONS = {          # name -> (P, F, tokens, seed)
    "a": (0, 0, 53, 11),
    "b": (10, 20, 77, 12),
    "c": (7, 14, 40, 13),
    "d": (0, 0, 30, 14),
}
MAX_SESSIONS, MAX_TOKENS, MAX_PROMPT = 3, 77, 10
N_TIMESTEPS = 2

# one list of actions per server step; ("open", name), ("push", name, n tokens), ("close", name)
TIMELINE = [
    [("open", "a"), ("push", "a", 21)],                                                 # a: 21 tokens, no chunk with its look-ahead yet
    [("push", "a", 21), ("open", "b"), ("push", "b", 25)],                              # a: 25 + 3 of 42 tokens; b: 25 + 3 of 35
    [("push", "a", 11), ("push", "b", 25), ("open", "c"), ("push", "c", 13)],           # a: 53, b: 53, c: nothing due (20 tokens)
    [("close", "a"), ("push", "b", 25), ("push", "c", 13)],                             # ctx (0, 3, 3): a final, b: 78, c: 28
    [("open", "d"), ("push", "d", 30), ("push", "b", 2), ("push", "c", 13)],            # d in a's slot: 28; b and c: nothing due
    [("close", "b"), ("push", "c", 1)],                                                 # b final alone; c: nothing due
    [("close", "c"), ("close", "d")],                                                   # two final rows
]
# the rows of every step as (name, tokens solved, ctx, first frame, end frame), worked out by hand from the schedule's description:
# L = 25 floor((m - 3) / 25) of the m tokens known, solved with 3 more when it has grown and 2 L > F; frames 2 L - F; a close
# solves all m tokens
ROWS = [
    [],
    [("a", 28, 3, 0, 50), ("b", 28, 3, 0, 30)],
    [("a", 53, 3, 50, 100), ("b", 53, 3, 30, 80)],
    [("a", 53, 0, 100, 106), ("b", 78, 3, 80, 130), ("c", 28, 3, 0, 36)],
    [("d", 28, 3, 0, 50)],
    [("b", 87, 0, 130, 154)],
    [("c", 47, 0, 36, 80), ("d", 30, 0, 50, 60)],
]


def inputs(name):
    """-> token [1, N], prompt_token [1, P], prompt_feat [1, F, 80], embedding [1, 192] of a session (CPU)"""
    from jyutvoice_amd import synth
    P, F, N, seed = SESSIONS[name]
    tok, _ = synth.prompt_tokens(1, N, first_index=200 + seed)
    ptok, _ = synth.prompt_tokens(1, P, first_index=300 + seed)
    g = torch.Generator().manual_seed(2000 + seed)
    return tok, ptok, torch.randn(1, F, 80, generator=g), torch.randn(1, 192, generator=g)


def pushes(name):
    """the calls a session makes over the timeline: [(step, n tokens or None for the close)]"""
    out = []
    for i, acts in enumerate(TIMELINE):
        for a in acts:
            if a[1] == name and a[0] != "open":
                out.append((i, a[2] if a[0] == "push" else None))
    return out


def play_server(server, timeline=TIMELINE, only=None, on_step=None):
    """the timeline into a server -> {name: [wav of every step in which the session was live, in order]}, {name: sid}.  only: the
    names that take part (the others' actions are skipped).  on_step(i, {name: wav} of the step, {name: sid} so far): called after every
    step."""
    sids, pos, wavs = {}, {}, {}
    for i, acts in enumerate(timeline):
        for a in acts:
            name = a[1]
            if only is not None and name not in only:
                continue
            if a[0] == "open":
                tok, ptok, feat, emb = inputs(name)
                sids[name] = server.open(ptok if ptok.shape[1] else None, feat if feat.shape[1] else None, emb, seed=SESSIONS[name][3])
                pos[name], wavs[name] = 0, []
            elif a[0] == "push":
                tok = inputs(name)[0]
                server.push(sids[name], tok[0, pos[name]:pos[name] + a[2]])
                pos[name] += a[2]
            else:
                server.close(sids[name])
        out = server.step()
        got = {n: out[sid] for n, sid in sids.items() if sid in out}
        for n, w in got.items():
            wavs[n].append((i, w))
        if on_step is not None:
            on_step(i, got, sids)
    return wavs, sids


def play_single(flow, hift, name):
    """the same calls into a Token2WavStream -> (session, [(step, wav)]) with the calls that returned audio"""
    from jyutvoice_amd.stream import Token2WavStream
    tok, ptok, feat, emb = inputs(name)
    P, F, N, seed = SESSIONS[name]
    session = Token2WavStream(flow, hift, ptok if P else None, feat if F else None, emb, max_tokens=N, n_timesteps=N_TIMESTEPS, seed=seed)
    out, pos = [], 0
    for step, n in pushes(name):
        if n is None:
            wav = session.finish()
        else:
            wav = session.push(tok[0, pos:pos + n])
            pos += n
        if wav.shape[1]:
            out.append((step, wav))
    return session, out
