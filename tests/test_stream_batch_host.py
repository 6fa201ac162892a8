"""CPU: the host logic of concurrent streaming sessions (jyutvoice_amd.stream.batch_plan / Token2WavServer, HiFTStreamBatch's
`stream_step`), without a device.

  * `batch_plan` per session equals `frame_schedule` -- and the rows worked out by hand in stream_batch_cases -- for sessions with
    different (P, F) and hop patterns; a session with nothing due is not in a step's rows; a closing session gets ctx = 0;
  * `stream_step` over any split equals HiFTStream's counts (stream_ref.hift_stream_counts);
  * the argument errors of open / push / close / step that are raised before any device call, and those of
    `inference_partial_batch`."""
import pytest
import torch

import stream_batch_cases as sb
import stream_ref as sr


# ---- the schedule -----------------------------------------------------------------------------------------------------------------
def simulate(timeline):
    """the timeline through batch_plan alone: the server's bookkeeping restated -> per step [(name, solve, ctx, lo, hi)]"""
    from jyutvoice_amd.stream import batch_plan
    state, order, steps = {}, [], []
    for acts in timeline:
        for a in acts:
            if a[0] == "open":
                P, F, _, _ = sb.SESSIONS[a[1]]
                state[a[1]] = [P, F, 0, 0, 0, False]
                order.append(a[1])
            elif a[0] == "push":
                state[a[1]][2] += a[2]
            else:
                state[a[1]][5] = True
        live = [n for n in order if n in state]
        rows = batch_plan([tuple(state[n]) for n in live])
        steps.append([(live[i], solve, ctx, lo, hi) for i, solve, ctx, lo, hi in rows])
        for i, solve, ctx, lo, hi in rows:
            st = state[live[i]]
            st[3], st[4] = solve - ctx, hi
            if st[5]:
                del state[live[i]]
    return steps


def test_batch_plan_of_the_timeline():
    steps = simulate(sb.TIMELINE)
    assert steps == sb.ROWS
    # one step mixes a final row with push rows, and sessions with nothing due are left out
    assert [c for _, _, c, _, _ in steps[3]] == [0, 3, 3]
    assert [n for n, *_ in steps[2]] == ["a", "b"] and [n for n, *_ in steps[4]] == ["d"]
    assert steps[0] == []


@pytest.mark.parametrize("name", sorted(sb.SESSIONS))
def test_batch_plan_equals_frame_schedule_per_session(name):
    """what the server solves for a session, step by step, is what the B = 1 session's schedule says for the same calls"""
    from jyutvoice_amd.stream import frame_schedule
    P, F, N, _ = sb.SESSIONS[name]
    calls = sb.pushes(name)
    assert calls[-1][1] is None and sum(n for _, n in calls[:-1]) == N
    want = frame_schedule(P, F, [n for _, n in calls[:-1]], finish=0)
    assert want == sr.schedule_ref(P, F, [n for _, n in calls[:-1]], 0)
    got = {i: row for i, rows in enumerate(simulate(sb.TIMELINE)) for row in rows if row[0] == name}
    for (step, n), (solve, lo, hi) in zip(calls, want):
        if solve:
            assert got[step][1:] == (solve, 0 if n is None else 3, lo, hi), (name, step)
        else:
            assert step not in got, (name, step)
    assert len(got) == sum(1 for s, _, _ in want if s)


def test_batch_plan_other_hops():
    """one token at a time and one big push, P / F with the first chunk inside the prompt: a step's row is next_step's answer"""
    from jyutvoice_amd.stream import batch_plan, frame_schedule
    cases = [(30, 60, [1] * 40), (3, 10, [27]), (26, 51, [5, 25, 1, 24])]
    for P, F, hops in cases:
        want = frame_schedule(P, F, hops, finish=0)
        n = L_done = done = 0
        for k, hop in enumerate(hops + [0]):
            n += hop
            closing = k == len(hops)
            rows = batch_plan([(0, 0, 0, 0, 0, False), (P, F, n, L_done, done, closing)])      # (an idle neighbour ahead of it)
            solve, lo, hi = want[k]
            if solve:
                assert rows == [(1, solve, 0 if closing else 3, lo, hi)]
                L_done, done = solve - rows[0][2], hi
            else:
                assert rows == []
    with pytest.raises(ValueError, match="fewer than the 14 prompt frames"):
        batch_plan([(2, 14, 3, 0, 0, True)])


@pytest.mark.parametrize("split", [[50, 50, 30], [1] * 130, [7, 123], [130]])
def test_stream_step_is_hift_streams_schedule(split):
    from jyutvoice_amd import spec
    from jyutvoice_amd.hifigan.generator import stream_step
    counts, rest = sr.hift_stream_counts(split, spec.HIFT_F0_HALO, spec.HIFT_DECODE_HALO)
    received = sourced = emitted = 0
    for call, (t, want) in enumerate(zip(split + [0], counts + [rest])):
        final = call == len(split)
        A, fwin, dwin = stream_step(received, sourced, emitted, t, final)
        assert A == received + t
        if fwin is not None:
            lo, c0, c1 = fwin
            assert c0 == sourced and c1 == (A if final else A - 5) and lo == max(sourced - 5, 0)
            sourced = c1
        if dwin is not None:
            lo, hi, k0, k1 = dwin
            assert hi == sourced and k0 == emitted and lo == max(emitted - 16, 0) and k1 == (sourced if final else sourced - 16)
            emitted = k1
            assert k1 - k0 == want
        else:
            assert want == 0
        received = A
    assert received == sourced == emitted == sum(split)


# ---- argument errors before the device -----------------------------------------------------------------------------------------------
class _Runtime:
    def ensure(self, *a):
        return None


class _Flow:
    """stands in for a loaded flow: a reservation that does nothing, and no solve"""
    def _rt(self):
        return _Runtime()

    def inference_partial_batch(self, *a, **k):
        raise AssertionError("a device call was reached")


class _Hift:
    """stands in for a loaded HiFTGenerator: the draws and pools on the CPU, and nothing that could launch"""
    device = torch.device("cpu")
    seeds = []

    def manual_seed(self, seed):
        self.seeds.append(seed)

    def _source_draws(self, B):
        return torch.zeros(B, 9), 2 ** 64 - 1, len(self.seeds)

    def _engine(self, B, T):
        return None

    def stream_batch(self, slots, max_frames):
        from jyutvoice_amd.hifigan.generator import HiFTStreamBatch
        return HiFTStreamBatch(self, slots, max_frames)


def test_server_argument_errors():
    from jyutvoice_amd.stream import Token2WavServer
    ptok, feat, emb = torch.zeros(1, 7, dtype=torch.int64), torch.zeros(1, 14, 80), torch.zeros(1, 192)
    for kw, word in (({"max_sessions": 0, "max_tokens": 5}, "max_sessions must be a positive int"),
                     ({"max_sessions": 2, "max_tokens": 2.5}, "max_tokens must be a positive int"),
                     ({"max_sessions": 2, "max_tokens": 5, "n_timesteps": 0}, "n_timesteps must be positive")):
        with pytest.raises(ValueError, match=word):
            Token2WavServer(None, None, **kw)      # (flow / hift = None: reaching them would be an AttributeError)
    server = Token2WavServer(_Flow(), _Hift(), max_sessions=2, max_tokens=30, n_timesteps=2, max_prompt_tokens=8)
    # the B = 1 shape messages
    for (a, b, c), word in [((ptok[0], feat, emb), "prompt_token must be an integer"), ((ptok.float(), feat, emb), "prompt_token must be an integer"),
                            ((ptok, feat[0], emb), "prompt_feat must be"), ((ptok, torch.zeros(1, 14, 79), emb), "prompt_feat must be"),
                            ((ptok, feat, torch.zeros(192)), "embedding must be"),
                            ((torch.zeros(1, 9, dtype=torch.int64), feat, emb), "exceeds max_prompt_tokens = 8")]:
        with pytest.raises(ValueError, match=word):
            server.open(a, b, c)
    s0 = server.open(ptok, feat, emb, seed=5)
    s1 = server.open(None, None, emb)
    assert s0 != s1 and _Hift.seeds[-1] == 5
    with pytest.raises(RuntimeError, match="all 2 sessions are taken"):
        server.open(ptok, feat, emb)
    # push
    for bad in (torch.zeros(2, 3, dtype=torch.int64), torch.zeros(3), torch.zeros(1, 1, 3, dtype=torch.int64)):
        with pytest.raises(ValueError, match="tokens must be an integer \\[n\\] or \\[1, n\\] tensor"):
            server.push(s0, bad)
    server.push(s0, torch.zeros(10, dtype=torch.int64))
    server.push(s0, [1, 2, 3])
    with pytest.raises(ValueError, match="13 \\+ 18 tokens exceed the session's max_tokens = 30"):
        server.push(s0, torch.zeros(1, 18, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="unknown session"):
        server.push(99, [1])
    with pytest.raises(RuntimeError, match="unknown session"):
        server.close(99)
    # 7 + 13 and 10 tokens: neither session has a chunk with its look-ahead yet.  Nothing is due: nothing is launched
    server.push(s1, torch.zeros(10, dtype=torch.int64))
    assert server.step() == {}
    # close: the final solve needs at least the prompt's frames
    with pytest.raises(ValueError, match="fewer than the 14 prompt frames"):
        short = Token2WavServer(_Flow(), _Hift(), max_sessions=1, max_tokens=30, max_prompt_tokens=8)
        short.close(short.open(ptok[:, :2], feat, emb))
    server.close(s1)
    with pytest.raises(RuntimeError, match="close\\(\\) has been called"):
        server.push(s1, [1])
    # a finished session is gone for push and close
    server._sessions[s1].finished = True
    with pytest.raises(RuntimeError, match="has finished"):
        server.push(s1, [1])
    with pytest.raises(RuntimeError, match="has finished"):
        server.close(s1)


def test_inference_partial_batch_errors_before_the_device():
    from jyutvoice_amd.flow.flow import CausalMaskedDiffWithXvec
    flow = CausalMaskedDiffWithXvec(vocab_size=6561, input_frame_rate=25)
    emb = torch.zeros(2, 192)
    tok = torch.zeros(2, 10, dtype=torch.int64)
    lens = torch.tensor([10, 3])

    def run(ctx, token=tok, token_len=lens, feat=None, feat_len=None, embedding=emb):
        return flow.inference_partial_batch(token, token_len, None, None, feat, feat_len, embedding, ctx)

    with pytest.raises(ValueError, match="utterance 1: ctx_lens 2"):
        run([3, 2])
    with pytest.raises(ValueError, match="utterance 0: ctx_lens -3"):
        run(torch.tensor([-3, 0]))
    with pytest.raises(ValueError, match="utterance 1: 3 tokens: at least 4 are needed"):
        run([3, 3])
    with pytest.raises(ValueError, match="utterance 1: prompt_feat has 7 frames \\(of 15\\) but the 3 encoded tokens give only 6"):
        run([3, 0], feat=torch.zeros(2, 15, 80), feat_len=torch.tensor([14, 7]))
    with pytest.raises(ValueError, match="utterance 0: prompt_feat has 15 frames \\(of 15\\) but the 7 encoded tokens give only 14"):
        run([3, 0], feat=torch.zeros(2, 15, 80), feat_len=torch.tensor([15, 6]))
    with pytest.raises(ValueError, match="utterance 0: token_len 11 outside \\[0, 10\\]"):
        run([3, 0], token_len=torch.tensor([11, 3]))
    with pytest.raises(ValueError, match="ctx_lens must hold 2 entries"):
        run([3])
    with pytest.raises(ValueError, match="embedding must be \\[2, 192\\]"):
        run([3, 0], embedding=torch.zeros(1, 192))
    with pytest.raises(RuntimeError, match="load_state_dict"):      # a mixed vector with three tokens on the whole-sequence row is fine
        run([3, 0])
