"""Writes tests/golden/G17_fp16.npz: the fp64 oracle's results for the cases of tests/test_gpu_fp16_estimator.py and the distance of
the FP16-mode emulation (tests/fp16_ref.py) from them.  From the oracle and fp16_ref only; nothing here loads the library.

    python tests/golden/make_golden_fp16.py        (CPU, a few minutes: 70 transformer blocks in fp64, 70 evaluations)"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import fp16_ref as fr      # noqa: E402
from jyutvoice_amd import synth      # noqa: E402
from oracle import flow as oflow      # noqa: E402


def main():
    noise = synth.rand_noise().double()
    out = {}
    for name in fr.CASES:
        c = fr.case_inputs(name)
        sd64 = fr.decoder64(fr.case_state_dict(name))
        utts, t0 = c["utts"], time.time()
        lens = c["lens"][list(utts)]
        stream = c["chunk"] > 0
        with torch.inference_mode():
            args = fr.cfg_batch(c, utts, torch.float64)
            est = oflow.estimator(sd64, *args, streaming=stream, chunk=c["chunk"] or 50)
            ref = fr.estimator(sd64, *args, streaming=stream, chunk=c["chunk"] or 50)
            mu, spks = c["mu"][list(utts)].double(), c["spks"][list(utts)].double()
            mask = args[1][:len(utts)]
            e_or = fr.streaming_est(oflow.estimator, c["chunk"]) if stream else None
            e_rf = fr.streaming_est(fr.estimator, c["chunk"]) if stream else fr.estimator
            mel = oflow.cfm_solve(sd64, noise, mu, mask, spks, torch.zeros_like(mu), c["steps"], 1.0, est=e_or).double()
            mel_ref = oflow.cfm_solve(sd64, noise, mu, mask, spks, torch.zeros_like(mu), c["steps"], 1.0, est=e_rf).double()
        out[name + "_est"] = est.numpy()
        out[name + "_mel"] = mel.numpy()
        out[name + "_est_floor"] = np.float64(fr.valid_dist(ref, est, torch.cat([lens, lens])))
        out[name + "_mel_floor"] = np.float64(fr.valid_dist(mel_ref, mel, lens))
        print(f"case {name}: d(fp16_ref, fp64 oracle) estimator {out[name + '_est_floor']:.3e}, {c['steps']}-step mel "
              f"{out[name + '_mel_floor']:.3e}  ({time.time() - t0:.0f} s)", flush=True)
    np.savez_compressed(os.path.join(HERE, "G17_fp16.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    main()
