#!/usr/bin/env python3
"""Time PnP-ADMM iterations on the grids beyond 224 x 224 (report only; bench.py stays the yardstick):
   python3 tools/grid_admm_times.py [--iters 20] [--reps 3]
For 224^2 spiral (the headline grid, for scale), 256^2 spiral and 192 x 256 EPI, all T = 200, s = 10, the full UNetRes
(structured weights): the best wall time of `reps` calls of `iters` iterations, ms per iteration, the LSQR iteration counts and the
stage split of the last call (profile level 3: stage marks read after the call, no wait inside it).  One JSON line per grid."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qmri_pnp_recon_poc_amd import engine as E, synth  # noqa: E402


def run(N, M, mask, iters, reps):
    T, s = 200, 10
    dic = synth.make_dictionary(T=T, n_t1=32, n_t2=16, s=s)
    L = max(N, M)
    X0 = synth.synthesize_tsmi(synth.make_phantom_qmaps(L, seed=0), dic)[(L - N) // 2:(L - N) // 2 + N, (L - M) // 2:(L - M) // 2 + M]
    fp, k = E.build_spiral(N, 771, T) if mask == "spiral" else E.build_epi(N, M, 1 / 65, T)
    e = E.Engine(0)
    e.set_operator(N, M, dic["V"], fp, k)
    e.set_denoiser(synth.structured_weights(seed=2, eps=0.3), N, M)
    y = synth.awgn_measured(e.forward(np.ascontiguousarray(X0)), 30.0, seed=0)
    e.pnp_admm(y, iters=2)                                            # warm-up: plans, code objects, calibration
    best, li = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        _, _, li = e.pnp_admm(y, iters=iters)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    e.profile_enable(3)
    e.pnp_admm(y, iters=iters)
    e.profile_enable(0)
    h = e.health()
    e.close()
    return {"grid": f"{N}x{M}", "mask": mask, "m": int(fp[-1]), "iters": iters, "ms_per_iter": round(best * 1e3 / iters, 4),
            "lsqr_iters": li.tolist(), "lsqr_one_launch": h["lsqr_one_launch"],
            "stage_ms_per_iter": {kk: round(v / iters, 4) for kk, v in h["last_call_stage_ms"].items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for N, M, mask in ((224, 224, "spiral"), (256, 256, "spiral"), (192, 256, "epi")):
        print(json.dumps(run(N, M, mask, a.iters, a.reps)), flush=True)


if __name__ == "__main__":
    main()
