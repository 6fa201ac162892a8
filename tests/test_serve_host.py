"""CPU: the host side of in-flight batching (jyutvoice_amd/serve.py) -- the per-request step table, the admission plan, the order
and number of steps a `SynthServer` gives every request (over a stub engine that records calls), its argument errors, and the
three new C-ABI entries (declared, exported, bound with the header's argument counts)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO

from jyutvoice_amd import serve, spec
from jyutvoice_amd.serve import FLOW_G, FLOW_GAP, SynthServer, admit_plan, step_rows, step_table

HEADER = os.path.join(REPO, "include", "jyutvoice_hip.h")
NEW = {"jv_cfm_pool_admit": 21, "jv_cfm_pool_step": 14, "jv_cfm_pool_fetch": 11}


# ---- schedule ----------------------------------------------------------------------------------------------------------------------
def reference_recurrence(n):
    """ConditionalCFM.solve_euler's running (t, dt) (flow_matching.py:230, 260-263) over the cosine t_span of :387-389, restated on
    fp32 tensors as the reference computes it"""
    t_span = 1 - torch.cos(torch.linspace(0, 1, n + 1, dtype=torch.float32) * 0.5 * torch.pi)
    t, dt = t_span[0], t_span[1] - t_span[0]
    tt, dts = [], []
    for step in range(1, len(t_span)):
        tt.append(float(t))
        dts.append(float(dt))
        t = t + dt
        if step < len(t_span) - 1:
            dt = t_span[step + 1] - t
    return tt, dts


@pytest.mark.parametrize("n", [1, 2, 4, 10, 32])
def test_step_table_is_the_reference_recurrence(n):
    tt, dts = step_table(n)
    rt, rd = reference_recurrence(n)
    assert len(tt) == len(dts) == n
    assert tt == rt and dts == rd      # bit for bit: both are fp32 values held in Python floats
    for v in tt + dts:
        assert float(torch.tensor(v, dtype=torch.float32)) == v      # representable in fp32
    assert tt[0] == 0.0 and abs(tt[-1] + dts[-1] - 1.0) < 1e-6


def test_step_table_rejects_bad_n():
    for bad in (0, -1, 2.0, None):
        with pytest.raises(ValueError):
            step_table(bad)


# ---- admission ---------------------------------------------------------------------------------------------------------------------
def test_step_rows():
    assert step_rows([]) == FLOW_G
    assert step_rows([44, 61, 97]) == 4 + 2 * (48 + 65 + 101) == 432
    lens12 = [150, 61, 97, 133, 60, 149, 88, 120, 75, 142, 101, 66]
    assert step_rows(lens12[:3]) == 644 and step_rows(lens12) == 2584


def test_admit_plan_is_fifo_and_bounded():
    big = 10 ** 9
    assert admit_plan([50, 60, 70], [], 3, big) == [0, 1, 2]
    assert admit_plan([50, 60, 70], [], 2, big) == [0, 1]                 # never more than the free slots
    assert admit_plan([50, 60, 70], [100], 0, big) == []
    assert admit_plan([], [100], 3, big) == []
    # rows: FLOW_G + sum 2 (len + FLOW_GAP) over active + admitted never exceeds the capacity
    cap = step_rows([100, 50, 60])
    assert admit_plan([50, 60, 70], [100], 3, cap) == [0, 1]
    assert admit_plan([50, 60, 70], [100], 3, cap - 1) == [0]
    # strictly first in, first out: a request that does not fit stops the line, a shorter one behind it does not overtake it
    assert admit_plan([500, 10], [100], 2, step_rows([100, 10])) == []
    # ... and it is admitted as soon as it is first in line and fits
    assert admit_plan([500, 10], [], 2, step_rows([500])) == [0]
    g = torch.Generator().manual_seed(1)
    for _ in range(200):
        waiting = torch.randint(1, 300, (int(torch.randint(0, 8, (1,), generator=g)),), generator=g).tolist()
        active = torch.randint(1, 300, (int(torch.randint(0, 5, (1,), generator=g)),), generator=g).tolist()
        free = int(torch.randint(0, 5, (1,), generator=g))
        cap = int(torch.randint(FLOW_G, 3000, (1,), generator=g))
        take = admit_plan(waiting, active, free, cap)
        assert take == list(range(len(take))) and len(take) <= free
        if take:
            assert step_rows(active + [waiting[i] for i in take]) <= cap
        if len(take) < min(free, len(waiting)):      # the next in line really did not fit
            assert step_rows(active + [waiting[i] for i in take] + [waiting[len(take)]]) > cap


# ---- a server over a stub engine -----------------------------------------------------------------------------------------------------
class StubPool:
    def __init__(self, slots, max_frames):
        self.slots, self.max_frames = slots, max_frames


class StubEngine:
    """records what the server asks of the library; a request of k tokens gets 2 k frames"""

    def __init__(self):
        self.calls = []
        self.y_lengths_host = None

    def cfm_pool(self, slots, max_frames):
        return StubPool(slots, max_frames)

    def encoder(self, x, xl, lang, tone, word_pos, syllable_pos, spk):
        B, Tt = x.shape
        self.calls.append(("encoder", B, Tt))
        return torch.zeros(B, 4, Tt), torch.zeros(B, 80, Tt), torch.zeros(B, 1, Tt), torch.zeros(B, 80)

    def length_regulate(self, logw, xl, mu_x, length_scale, host_lengths=False):
        assert host_lengths
        self.y_lengths_host = [int(round(2 * int(n) * length_scale)) for n in xl.tolist()]
        self.calls.append(("length_regulate", float(length_scale), list(self.y_lengths_host)))
        B, ty = logw.shape[0], max(self.y_lengths_host)
        return None, torch.tensor(self.y_lengths_host), None, torch.zeros(B, 80, ty)

    def cfm_pool_admit(self, pool, mu_y, y_lens, prompt_h, prompt_feat, prompt_lens, spks, slots, temperatures):
        self.calls.append(("admit", list(slots), list(y_lens), list(prompt_lens), list(temperatures)))

    def cfm_pool_step(self, pool, slots, lens, t, dt):
        self.calls.append(("step", list(slots), list(lens), list(t), list(dt)))

    def cfm_pool_fetch(self, pool, slots, first, lens, frames=None):
        self.calls.append(("fetch", list(slots), list(first), list(lens)))
        return torch.zeros(len(slots), 80, max(lens))


class StubVocoder:
    def __init__(self, hift):
        self.hift, self.opened, self.state = hift, [], {}

    def open(self, slot):
        assert slot not in self.state
        self.state[slot] = self.hift.seed
        self.opened.append((slot, self.hift.seed))
        return slot

    def advance(self, mel, rows):
        return {slot: (torch.zeros(1, 480 * (hi - lo)), torch.zeros(1, 1, 480 * (hi - lo))) for slot, r, lo, hi, final in rows}

    def close(self, slot):
        del self.state[slot]


class StubHift:
    device, seed = torch.device("cpu"), None

    def manual_seed(self, seed):
        self.seed = seed

    def stream_batch(self, slots, max_frames):
        self.vocoder = StubVocoder(self)
        return self.vocoder


class StubTts:
    device = torch.device("cpu")


def request(tokens, **kw):
    ids = torch.ones(1, tokens, dtype=torch.int64)
    return (ids, torch.tensor([tokens]), ids, ids, ids, ids, torch.zeros(1, spec.SPK_EMBED_DIM)), kw


def test_server_gives_every_request_its_own_steps_in_order():
    eng, hift = StubEngine(), StubHift()
    server = SynthServer(StubTts(), hift, max_sessions=3, max_frames=128, max_tokens=32, engine=eng)
    ns = [3, 4, 5, 6, 3, 4, 5]
    tokens = [10, 12, 14, 16, 18, 20, 22]
    rids = []
    for n, k in zip(ns, tokens):      # all seven are waiting before the first step: 3 slots, so four of them queue
        args, kw = request(k, n_timesteps=n, temperature=0.5 + 0.1 * n, seed=100 + k)
        rids.append(server.submit(*args, **kw))
    assert rids == list(range(7)) and server.pending() == 7
    finished_at, t = {}, 0
    while server.pending():
        out = server.step()
        t += 1
        assert t < 40
        for rid, res in out.items():
            finished_at[rid] = t
            assert res["mel_length"] == 2 * tokens[rid] and res["wav"].shape == (1, 480 * 2 * tokens[rid])
    assert sorted(finished_at) == rids                                   # no request starves
    # admission is first in, first out: request i never finishes its first step later than request i + 1 does
    slot_of, seq, first_step, order = {}, {r: [] for r in rids}, {}, []
    owner, step_no = {}, 0
    for c in eng.calls:
        if c[0] == "admit":
            _, slots, y_lens, p_lens, temps = c
            for s, y, p, tmp in zip(slots, y_lens, p_lens, temps):
                rid = tokens.index(y // 2)
                assert s not in owner and p == 0 and tmp == pytest.approx(0.5 + 0.1 * ns[rid])
                owner[s] = rid
                slot_of.setdefault(rid, s)
                order.append(rid)
        elif c[0] == "step":
            step_no += 1
            _, slots, lens, ts, dts = c
            assert len(set(slots)) == len(slots) <= 3                    # a slot once per step, never more than the pool holds
            for s, n, tv, dv in zip(slots, lens, ts, dts):
                rid = owner[s]
                assert n == 2 * tokens[rid]
                seq[rid].append((tv, dv))
                first_step.setdefault(rid, step_no)
        elif c[0] == "fetch":
            _, slots, first, lens = c
            for s, f, n in zip(slots, first, lens):
                rid = owner.pop(s)                                       # the slot is free for its next occupant
                assert f == 0 and n == 2 * tokens[rid]
    assert order == rids
    for rid, n in zip(rids, ns):                                         # exactly n_r steps, its own (t, dt) sequence, in order
        tt, dts = step_table(n)
        assert seq[rid] == list(zip(tt, dts)), rid
        assert finished_at[rid] == first_step[rid] + n - 1               # a resident request takes part in every step
    assert [first_step[r] for r in rids] == sorted(first_step[r] for r in rids)
    assert first_step[0] == first_step[1] == first_step[2] == 1         # admitted in a step = first Euler step in that step
    assert first_step[3] == finished_at[0] + 1                           # the slot a request frees is taken in the next step
    assert len(set(slot_of.values())) == 3 and len(slot_of) == 7         # slots are reused
    # a source signal per request: each vocoder slot was opened after manual_seed(seed_r)
    assert sorted(seed for _, seed in hift.vocoder.opened) == sorted(100 + k for k in tokens)
    for slot, seed in hift.vocoder.opened:
        assert any(slot_of[r] == slot and 100 + tokens[r] == seed for r in rids)


def test_server_batches_the_encoder_per_length_scale_and_arrivals_join_between_steps():
    eng = StubEngine()
    server = SynthServer(StubTts(), StubHift(), max_sessions=4, max_frames=256, max_tokens=32, engine=eng)
    for k, scale in ((8, 1.0), (9, 1.5), (10, 1.0)):
        args, kw = request(k, n_timesteps=3, length_scale=scale)
        server.submit(*args, **kw)
    server.step()
    assert [c for c in eng.calls if c[0] == "length_regulate"] == [("length_regulate", 1.0, [16, 20]), ("length_regulate", 1.5, [27])]
    assert [c[1:3] for c in eng.calls if c[0] == "encoder"] == [(2, 10), (1, 9)]      # padded to the group's longest text
    args, kw = request(5, n_timesteps=2)
    late = server.submit(*args, **kw)      # arrives while the others are at step 1 of 3
    out = server.step()
    assert out == {} and eng.calls[-1][0] == "step" and len(eng.calls[-1][1]) == 4
    tt2, _ = step_table(2)
    tt3, _ = step_table(3)
    assert sorted(eng.calls[-1][3]) == sorted([tt3[1]] * 3 + [tt2[0]])      # one estimator call, two different t
    out = server.step()
    assert sorted(out) == [0, 1, 2, late]
    assert server.pending() == 0 and server.step() == {}


def test_a_request_too_long_once_its_durations_are_known_fails_alone():
    eng = StubEngine()
    server = SynthServer(StubTts(), StubHift(), max_sessions=2, max_frames=40, max_tokens=32, engine=eng)
    a, kw = request(10, n_timesteps=1)
    ok = server.submit(*a, **kw)
    b, kw = request(30, n_timesteps=1, length_scale=0.9)      # 54 frames: known only after length regulation
    bad = server.submit(*b, **kw)
    out = server.drain()
    assert sorted(out) == [ok, bad] and "error" in out[bad] and f"request {bad}" in out[bad]["error"] and "wav" in out[ok]


def test_submit_errors_name_the_request():
    server = SynthServer(StubTts(), StubHift(), max_sessions=2, max_frames=64, max_tokens=16, engine=StubEngine())
    good, _ = request(8)

    def bad(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            server.submit(*args, **kw)

    x, xl, lang, tone, wp, sp, spk = good
    bad("request 0: x must be", x[0], xl, lang, tone, wp, sp, spk)                              # not [1, tokens]
    bad("request 0: x must be", x.float(), xl, lang, tone, wp, sp, spk)
    bad("request 0: lang has shape", x, xl, lang[:, :4], tone, wp, sp, spk)
    bad("request 0: .*max_tokens", *request(17)[0])
    bad("request 0: x_lengths", x, torch.tensor([9]), lang, tone, wp, sp, spk)
    bad("request 0: spk_embed", x, xl, lang, tone, wp, sp, torch.zeros(1, 10))
    bad("request 0: prompt_feat and prompt_h", *good, prompt_feat=torch.zeros(1, 5, 80))
    bad("request 0: prompt_h must be", *good, prompt_feat=torch.zeros(1, 5, 80), prompt_h=torch.zeros(1, 80, 5))
    bad("request 0: prompt_feat has 5 frames", *good, prompt_feat=torch.zeros(1, 5, 80), prompt_h=torch.zeros(1, 6, 80))
    for n in (0, -3, 2.5, 2000):
        bad("request 0: n_timesteps", *good, n_timesteps=n)
    bad("request 0: temperature", *good, temperature=float("nan"))
    bad("request 0: length_scale", *good, length_scale=0.0)
    # longer than max_frames: 60 prompt frames + at least one per token
    bad("request 0: at least 68 frames", *good, prompt_feat=torch.zeros(1, 60, 80), prompt_h=torch.zeros(1, 60, 80))
    assert server.pending() == 0
    assert server.submit(*good) == 0 and server.submit(*good, prompt_feat=torch.zeros(1, 20, 80), prompt_h=torch.zeros(1, 20, 80)) == 1
    with pytest.raises(ValueError, match="request 2"):
        server.submit(*good, n_timesteps=0)
    for kw in (dict(max_sessions=0), dict(max_frames=0), dict(max_tokens=-1), dict(row_capacity=3)):
        with pytest.raises(ValueError):
            SynthServer(StubTts(), StubHift(), **{**dict(max_sessions=2, max_frames=64, max_tokens=16, engine=StubEngine()), **kw})


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
def header_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(jv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = params.strip()
        out[name] = 0 if params in ("", "void") else len(params.split(","))
    return out


def test_pool_entries_declared_exported_and_bound():
    from jyutvoice_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    lib = _lib.load()
    protos = header_prototypes()
    for name, nargs in NEW.items():
        assert protos.get(name) == nargs, f"{name}: the header declares {protos.get(name)} parameters"
        assert hasattr(lib, name), f"{name} not exported by the library"
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
    _, a = _lib.SIGNATURES["jv_cfm_pool_step"]
    assert a[6:8] == [ctypes.c_int] * 2 and a[12] is ctypes.c_int      # slots, Tcap, ..., B
    from jyutvoice_amd._lib import JvError, check
    null = ctypes.c_void_p()
    with pytest.raises(JvError, match="null context"):
        check(lib.jv_cfm_pool_step(null, None, None, None, None, None, 1, 1, None, None, None, None, 1, None))
    from jyutvoice_amd.engine import CfmPool
    pool = CfmPool(3, 16, "cpu")      # plain tensors owned by the caller
    assert [tuple(t.shape) for t in pool.tensors()] == [(3, 16, 80)] * 3 + [(3, 80), (3, 3, 2)]
    assert serve.FLOW_G == 4 and serve.FLOW_GAP == 4
    text = open(os.path.join(REPO, "jyutvoice_amd", "csrc", "flow_ws.h")).read()
    assert "FLOW_G = 4" in text and "FLOW_GAP = 4" in text and "max_steps = 1024" in text      # serve.py restates them
