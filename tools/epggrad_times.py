#!/usr/bin/env python3
"""Time of the EPG derivative simulation and its Cramer-Rao bound (qmri_dict_simulate_grad_dev) against the plain simulation
(qmri_dict_simulate_dev) in the same process.

    python3 tools/epggrad_times.py [--K 98304] [--T 1000] [--S 32] [--s 10] [--reps 20] [--out profiles/epggrad_times.json]

t1, t2 (a 384 x 256 log-spaced grid when K = 98304) are put on the device once and every output buffer is allocated once.  The variants -- the plain
simulation, and for P = 2 and P = 3 the bound alone (uncompressed, and in a T x s subspace) and the call that also writes F and dF -- are timed in
turn, variant after variant within each of --reps rounds, after one warm-up round: the host clock around calls that return after their kernel has
finished.  Per variant the least and the median time, and the ratio of the least to the plain simulation's.  The arithmetic of the recursion is
(1 + P) x the plain simulation's plus the projection; that factor is the yardstick the ratios are read against.  Writes one JSON document."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from epg_times import atoms  # noqa: E402  (the same atom grid as tools/epg_times.py)


def measure(K, T, S, s, reps):
    from qmri_pnp_recon_poc_amd import engine, synth
    from qmri_pnp_recon_poc_amd._lib import EpgGradParams, EpgParams
    t1, t2 = atoms(K)
    alpha, tr, te = synth.flip_angle_train(T), np.full(T, 0.012), np.full(T, 0.002)
    V = np.ascontiguousarray(np.linalg.qr(np.cos(0.37 * np.outer(np.arange(T) + 1.0, np.arange(s) + 1.0)))[0].ravel(order="F"))
    eng, hip = engine.Engine(0), engine._hip_runtime()
    d_t1, d_t2, d_F, d_dF, d_crb, d_fl = ptrs = [C.c_void_p() for _ in range(6)]
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    p = EpgParams(S, 1, 0.0, 1.0, 1)
    try:
        for d, nb in ((d_t1, K * 8), (d_t2, K * 8), (d_F, K * T * 8), (d_dF, 3 * K * T * 8), (d_crb, 4 * K * 8), (d_fl, K * 4)):
            assert hip.hipMalloc(C.byref(d), nb) == 0
        assert hip.hipMemcpy(d_t1, t1.ctypes.data, K * 8, 1) == 0 and hip.hipMemcpy(d_t2, t2.ctypes.data, K * 8, 1) == 0

        def plain():
            eng._check(eng.L.qmri_dict_simulate_dev(eng.h, K, T, vp(alpha), vp(tr), vp(te), d_t1, d_t2, None, C.byref(p), d_F))

        def grad(P, sv, outputs):
            gp = EpgGradParams(P, sv, V.ctypes.data if sv else None)
            return lambda: eng._check(eng.L.qmri_dict_simulate_grad_dev(eng.h, K, T, vp(alpha), vp(tr), vp(te), d_t1, d_t2, None, C.byref(p), C.byref(gp),
                                                                        d_F if outputs else None, d_dF if outputs else None, d_crb, d_fl))

        variants = [("simulate", plain)]
        for P in (2, 3):
            variants += [(f"P{P}_bound_only", grad(P, 0, False)), (f"P{P}_bound_only_s{s}", grad(P, s, False)), (f"P{P}_with_outputs", grad(P, 0, True))]
        times = {name: [] for name, _ in variants}
        for rnd in range(reps + 1):                                  # (the first round warms up: code objects, allocator)
            for name, fn in variants:
                t0 = time.perf_counter()
                fn()
                if rnd:
                    times[name].append(1e3 * (time.perf_counter() - t0))
        fl = np.empty(K, np.int32)
        assert hip.hipMemcpy(fl.ctypes.data, d_fl, K * 4, 2) == 0
    finally:
        for d in ptrs:
            hip.hipFree(d)
        eng.close()
    base = min(times["simulate"])
    rows = {name: {"min_ms": min(t), "median_ms": float(np.median(t)), "ratio_to_simulate": min(t) / base} for name, t in times.items()}
    return {"K": K, "T": T, "S": S, "s": s, "reps": reps, "singular_atoms_last_call": int(np.sum(fl == 1)), "variants": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=98304)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--S", type=int, default=32)
    ap.add_argument("--s", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epggrad_times.json"))
    a = ap.parse_args()
    r = measure(a.K, a.T, a.S, a.s, a.reps)
    print(json.dumps(r), flush=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/epggrad_times.py", "device": "MI355X", "runs": [r]}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
