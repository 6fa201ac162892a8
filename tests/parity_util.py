"""Shared by test_gpu_lengths.py, test_gpu_positions.py, test_gpu_vocoder_unclipped.py and test_vocoder_inputs_host.py (a plain
module, not a conftest): error measures in fp64, the same models evaluated in fp64, a JSON recorder for the output directory, the in-library
profiler read for WHICH geometry / regime a call took, and the vocoder inputs the clamp does not hide.

The vocoder recipe.  `mel = 1.5 randn, s = tanh(0.3 randn)` (the older tests') drives the synthetic checkpoints far past
HIFT_AUDIO_LIMIT: four reference samples in five sit on +-0.99, where both sides of a comparison read the clamp whatever the
kernels computed.  `mel = randn, s = tanh(0.05 randn)` keeps the clamped share of the fp64 reference at or below 0.11 % (waveform
RMS ~0.28).  CLAMP_CAP is a condition on the reference alone: every case asserts it before anything is compared, and
test_vocoder_inputs_host.py asserts it without a GPU for every case listed here, on both checkpoints."""
import json
import os

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CLAMP_CAP = 0.01          # at most 1 % of the fp64 reference's samples may have |w| >= 0.99
AUDIO_LIMIT = 0.99        # spec.HIFT_AUDIO_LIMIT

# name -> (seed, T, lengths): the inputs of test_gpu_vocoder_unclipped.py (shapes and seeds of the four tests they twin) and of the
# vocoder part of test_gpu_positions.py (one utterance each: the batch is that utterance replicated)
VOCODER_CASES = {
    "ragged_24": (77, 24, [24, 13]),
    "pair_61": (123, 61, [61, 37, 50]),
    "pair_151": (321, 151, [151, 97, 150, 12]),
    "compact_70": (5, 70, [70, 31, 70, 12, 55, 64]),
    "tiny_1": (51, 1, [1]),
    "tiny_2": (52, 2, [2]),
    "tiny_5": (55, 5, [5]),
    "positions_61": (6100, 61, [61]),
    "positions_151": (15100, 151, [151]),
}
# which checkpoint(s) the GPU cases run each input on ("tame": synth.hift_state_dict, "hostile": synth.hostile_hift_state_dict);
# the host test runs every input on both
GPU_CHECKPOINTS = {"pair_61": ("tame", "hostile")}


def md(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def rms(a, b):
    return float((a.double().cpu() - b.double().cpu()).pow(2).mean().sqrt())


def quiet_vocoder_inputs(name):
    """(mel [B,80,T], s [B,1,480 T], lengths) of a VOCODER_CASES entry: mel = randn, s = tanh(0.05 randn)"""
    seed, T, lens = VOCODER_CASES[name]
    g = torch.Generator().manual_seed(seed)
    mel = torch.randn(len(lens), 80, T, generator=g)
    s = torch.tanh(torch.randn(len(lens), 1, 480 * T, generator=g) * 0.05)
    return mel, s, lens


def hift_checkpoint(kind):
    from jyutvoice_amd import synth
    return synth.hift_state_dict() if kind == "tame" else synth.hostile_hift_state_dict()


def hift_folded(sd):
    """(fp32, fp64) weights of the vocoder oracle: fold_weight_norm's output, and the same cast to double"""
    from oracle import hift as ohift
    w = ohift.fold_weight_norm(sd)
    return w, {k: v.double() if v.is_floating_point() else v for k, v in w.items()}


def hift_fp64(w64, mel, s, L):
    """utterance [1,80,T] / [1,1,480 T] cut to its L frames through the oracle in fp64"""
    from oracle import hift as ohift
    with torch.inference_mode():
        return ohift.decode(w64, mel[:, :, :L].double(), s[:, :, :480 * L].double())


def hift_fp32(w32, mel, s, L):
    from oracle import hift as ohift
    with torch.inference_mode():
        return ohift.decode(w32, mel[:, :, :L], s[:, :, :480 * L])


def clamp_share(wav):
    return float((wav.abs() >= AUDIO_LIMIT).double().mean())


def cfm_oracles(sd, noise, mu, spks, n_steps):
    """one utterance ([1,80,T], cond = 0) through oracle.flow.cfm_solve: (fp32 oracle, the same model with the `decoder.*`
    weights, the noise and the inputs cast to double)"""
    from oracle import flow as oflow
    T = mu.shape[2]
    with torch.inference_mode():
        m32 = oflow.cfm_solve(sd, noise, mu, torch.ones(1, 1, T), spks, torch.zeros(1, 80, T), n_steps, 1.0)
        sd64 = {k: v.double() for k, v in sd.items() if k.startswith("decoder.")}
        m64 = oflow.cfm_solve(sd64, noise.double(), mu.double(), torch.ones(1, 1, T, dtype=torch.float64), spks.double(),
                              torch.zeros(1, 80, T, dtype=torch.float64), n_steps, 1.0)
    return m32, m64


class Recorder:
    """measured figures -> <output directory>/<name> (JV_OUT as the tools/ scripts read it, default out/), rewritten after every
    entry (a later failure keeps what was measured)"""

    def __init__(self, name, header, columns=None):
        self.name, self.doc, self.columns = name, dict(header, measured={}), columns
        if columns:
            self.doc["columns"] = list(columns)

    def __call__(self, key, **vals):
        self.doc["measured"].setdefault(key, {}).update({k: float(f"{v:.3e}") for k, v in vals.items()})
        self.write()
        print(f"[{self.name}] {key}: " + ", ".join(f"{k}={v:.3e}" for k, v in vals.items()))

    def table(self, key, rows):
        """a test that measures hundreds of figures: rows = {sub-key: {column: value}} become ONE entry, each row a list in the order
        of `columns`, behind one rewrite of the file, which then keeps an entry on one line"""
        self.doc["measured"][key] = {k: [float(f"{v[c]:.3e}") for c in self.columns] for k, v in rows.items()}
        self.write()
        print(f"[{self.name}] {key}: {len(rows)} rows of {self.columns}")

    def write(self):
        out = os.environ.get("JV_OUT") or os.path.join(REPO, "out")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, self.name), "w") as fh:
            if not self.columns:
                json.dump(self.doc, fh, indent=1, sort_keys=True)
                return
            head = json.dumps({k: v for k, v in self.doc.items() if k != "measured"}, indent=1, sort_keys=True)
            lines = [f'  {json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in sorted(self.doc["measured"].items())]
            fh.write(head[:head.rindex("}")].rstrip() + ',\n "measured": {\n' + ",\n".join(lines) + "\n }\n}\n")


# ---- which geometry / regime did a call take?  Read from the in-library profiler, as tools/route_census.py does -----------------
def profiled(fn):
    """run fn() under the in-library profiler: {kernel name: {launches, ms, flops, bytes}}"""
    from jyutvoice_amd import engine
    engine.profile_enable(True)
    try:
        fn()
        return engine.profile_report()
    finally:
        engine.profile_enable(False)


def flops_of(report, prefix, suffix=">"):
    """summed algorithmic flops of the kernels whose profiler name starts / ends so.  A launch's figure is proportional to the
    REAL frames of its call: all B T of them in the uniform geometry, the sum of the clamped lengths in the compact one
    (Geo::alg_rows, HGeo::frames) -- so the ratio of two runs of one batch says which geometry each took."""
    hit = {k: v for k, v in report.items() if k.startswith(prefix) and k.endswith(suffix)}
    assert hit, (prefix, suffix, sorted(report))
    return sum(v["flops"] for v in hit.values())


def assert_compact_taken(compact_report, uniform_report, lens, T, prefix, suffix=">", mul=1, add=0):
    """the run behind `compact_report` laid its rows out compactly and the one behind `uniform_report` did not: the frames their
    launches account for are sum(min(max(len, 0), T)) against B T (at a level of `mul` rows per frame, + `add` per utterance in
    the uniform geometry: the vocoder's last level)"""
    real = sum(min(max(int(n), 0), T) for n in lens) * mul
    full = len(lens) * (T * mul + add)
    assert real < full
    got = flops_of(compact_report, prefix, suffix) / flops_of(uniform_report, prefix, suffix)
    assert abs(got - real / full) <= 1e-6, (got, real / full, "the compact geometry was not taken")


def solve_frames(report):
    """the real frames (CFG twins included) every fused transformer-block launch of a solve accounted for: its flops are
    2 frames (512 x 256 + 2 x 256 x 1024 MACs, + 256 x 1536 where q | k | v rides along) (rowblock.hip)"""
    seen = set()
    for k, v in report.items():
        if k.startswith("rowblock_h3<"):
            macs = 256.0 * 512 + 2.0 * 256 * 1024 + (256.0 * 1536 if k.endswith(",qkv>") else 0.0)
            frames = v["flops"] / (v["launches"] * 2.0 * macs)      # (the report prints nine digits)
            assert abs(frames - round(frames)) < 0.01, (k, frames)
            seen.add(int(round(frames)))
    assert len(seen) == 1, (seen, sorted(report))
    return seen.pop()


def assert_solve_compact(compact_report, uniform_report, lens, T):
    """the solve behind `compact_report` laid its rows out compactly (its launches account for the clamped lengths' sum), the one
    behind `uniform_report` padded every utterance to T"""
    real = 2 * sum(min(max(int(n), 0), T) for n in lens)
    assert real < 2 * len(lens) * T
    assert solve_frames(compact_report) == real, (solve_frames(compact_report), real, "the compact geometry was not taken")
    assert solve_frames(uniform_report) == 2 * len(lens) * T, (solve_frames(uniform_report), 2 * len(lens) * T)


# the row arithmetic of a solve, as flow.hip / estimator.hip est_route / rowgemm.hip rowgemm_tile do it (FLOW_G = FLOW_GAP = 4)
def flow_rows(lens, T=None):
    """rows of a solve of these lengths: compact (T None: every utterance and its CFG twin own len + 4 rows) or uniform"""
    return 4 + 2 * sum((n if T is None else T) + 4 for n in lens)


def rowgemm_tile(M):
    if M <= 2048:
        return 0
    cdiv = lambda a, b: -(-a // b)
    return min(range(2, 6), key=lambda rt: (cdiv(cdiv(M, 16 * rt), 256) * rt, -rt))      # fewest rounds x rows; ties: the taller tile


def qkv_regime(M):
    """est_route's q | k | v decision at M rows: 'tiles' (no row-owning kernels), 'split6' / 'split3' / 'split2' (q | k | v in a
    launch of its own, its column chunks dealt over that many workgroups per 80 rows) or 'fused' (inside the block launch)"""
    tile = rowgemm_tile(M)
    if tile == 0:
        return "tiles"
    if -(-M // (16 * tile)) > 192:
        return "fused"
    tiles = -(-M // 80)
    return "split6" if tiles * 6 <= 256 else "split3" if tiles * 3 <= 256 else "split2"


def assert_qkv_regime(report, M, want):
    """the regime the row count selects is `want`, and the launches show its side of the fused / split line: in a split regime
    the blocks hand their LayerNorm planes on (rowblock_h3<..,ln>) to a q | k | v launch of 80-row tiles (rowgemm_h3<80x256,qkv>)
    and none carries q | k | v; in the fused one they carry it (rowblock_h3<..,qkv>) and none writes planes.  (The column split
    itself, 6 / 3 / 2, is a grid dimension: it follows from M by est_route's rule, mirrored in qkv_regime.)"""
    assert qkv_regime(M) == want, (M, qkv_regime(M), want)
    ln = sum(v["launches"] for k, v in report.items() if k.startswith("rowblock_h3<") and k.endswith(",ln>"))
    riding = sum(v["launches"] for k, v in report.items() if k.startswith("rowblock_h3<") and k.endswith(",qkv>"))
    if want.startswith("split"):
        assert ln > 0 and riding == 0 and "rowgemm_h3<80x256,qkv>" in report, (want, ln, riding, sorted(report))
    else:
        assert want == "fused" and ln == 0 and riding > 0, (want, ln, riding, sorted(report))
