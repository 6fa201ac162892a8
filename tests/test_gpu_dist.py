"""GPU, two ranks on the one card: utterance data parallelism end to end.

Two fresh processes (one per rank, as `torch.distributed.run` starts them; rendezvous over gloo on 127.0.0.1) each
synthesise their contiguous shard of an 8-utterance ragged batch and all-gather the mels; the gathered result must equal
the single-process synthesis of the whole batch BIT FOR BIT -- the measured fp16x3 bounds are per utterance and every
kernel sums a row in the same order wherever the row sits, so an utterance's result does not depend on how the batch is
sharded.  That holds while the shards and the whole batch run the same kernel set, which the engine picks from the batch's
row count M = 2 B (T + 4) + 4 (split-K below 2049 rows, the row-owning GEMM once its grid fills the chip, the
tile kernels between): the first case keeps both sides under the split-K limit, the second puts the whole batch above it
and the shards below, where a row's K sum is grouped differently and the agreement is to rounding (<= 2e-5) -- as for
test_gpu_pipeline.py::test_full_size_batch_invariance.  The benchmarked data-parallel job is weak-scaling (every rank runs
the same 32 x 300 batch as the one-GPU job), so there every rank is in the one-GPU regime."""
import os
import socket
import subprocess
import sys

import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("tokens,same_kernels", [(10, True), (24, False)])
def test_two_rank_shards_equal_single_process(tmp_path, tts_sd, tokens, same_kernels):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    import jyutvoice_amd
    from jyutvoice_amd import synth
    utts, steps = 8, 3
    out = str(tmp_path / "gathered.pt")
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(REPO, "tests", "dist_worker.py"), "--out", out,
                                       "--utts", str(utts), "--tokens", str(tokens), "--steps", str(steps)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=420)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        logs.append(o.decode(errors="replace")[-2000:])
    assert all(p.returncode == 0 for p in procs), logs
    got = torch.load(out)
    # the same batch in this process, unsharded
    tts, _ = jyutvoice_amd.build_default("cuda:0")
    tts.load_state_dict(tts_sd)
    lengths = [tokens - 3 * (i % 4) for i in range(utts)]
    b = synth.batch(utts, tokens, first_index=200, lengths=lengths)
    keys = ("x", "x_lengths", "lang", "tone", "word_pos", "syllable_pos", "spk_embed")
    res = tts.synthesise(*[b[k] for k in keys], None, n_timesteps=steps, batched=True)
    assert torch.equal(got["lens"], res["mel_lengths"].cpu())
    want = res["mel"].cpu()
    assert got["mel"].shape == want.shape
    rows = 2 * utts * (want.shape[-1] + 4) + 4
    assert (rows <= 2048) == same_kernels, ("the case no longer sits on the side of the split-K limit it was sized for", rows)
    if same_kernels:
        assert torch.equal(got["mel"], want), float((got["mel"] - want).abs().max())
    else:
        assert float((got["mel"] - want).abs().max()) <= 2e-5


@pytest.mark.parametrize("strong", [False])      # (True passes too -- `--strong --total-batch 6` -- and costs another minute of start-up)
def test_bench_script_runs_with_two_ranks(strong):
    """bench.py itself as the driver starts it for N = 2 -- one process per rank, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in
    the environment -- rehearsed on the one card with gloo (JV_DIST_BACKEND=gloo; the modulo in bench.py puts both ranks on
    GPU 0): every rank must reach the end (a collective entered by rank 0 alone, as the per-stage passes once did, hangs here
    until the timeout), rank 0 prints ONE JSON line for the whole job, the others print none"""
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    import json
    port = _free_port()
    flags = ["--gpus", "2", "--tokens", "20", "--timesteps", "2", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-exact-range"]
    flags += ["--strong", "--total-batch", "6"] if strong else ["--batch", "3"]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   JV_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(REPO, "bench.py"), *flags], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE))
    outs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            o, e = p.communicate()
        outs.append((p.returncode, o.decode(errors="replace"), e.decode(errors="replace")[-1500:]))
    assert all(rc == 0 for rc, _, _ in outs), outs
    lines0 = [ln for ln in outs[0][1].splitlines() if ln.startswith("{")]
    lines1 = [ln for ln in outs[1][1].splitlines() if ln.startswith("{")]
    assert len(lines0) == 1 and not lines1, (lines0, lines1)
    d = json.loads(lines0[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["steps"] == 2 and d["scaling"] == ("strong" if strong else "weak")
    assert d["config"]["global_batch"] == 6
    assert d["stage_ms"]["cfm_loop"] > 0          # rank 0's per-stage passes ran (without the collective)
    # whole-job frames over the slowest rank's time
    assert abs(d["value"] - 6 * 40 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-3 * d["value"]

