#!/usr/bin/env python3
"""Time of the EPG simulation of prepared, repeated trains (qmri_dict_simulate_seq_dev) against the plain simulation
(qmri_dict_simulate_dev) in the same process.

    python3 tools/epgseq_times.py [--K 98304] [--T 1000] [--S 32] [--runs 5] [--calls 25] [--out profiles/epgseq_times.json]

Three arms on the same atoms (a 384 x 256 log-spaced grid when K = 98304, on the device once; one output buffer):
    simulate        qmri_dict_simulate_dev with an inversion (TI 21 ms, efficiency 0.95): the call this project had before
    seq_degenerate  qmri_dict_simulate_seq_dev with the one block that states the same experiment, one cycle (the same numbers)
    seq_four_block  qmri_dict_simulate_seq_dev with four blocks (none; inversion, wait 0.3 s; T2 40 ms, wait 0.25 s; T2 80 ms, wait 0.01 s) whose
                    boundaries are no multiples of 16, two cycles: twice the atom-frames
A run is --calls calls in a row under the host clock (every call returns after its kernel has finished); the arms alternate, run after run, for
--runs runs each after one warm-up run each.  Per arm: the time per call of every run, their least, median and spread (largest - least) and the
time per simulated atom-frame (K T cycles).  Before the timing the degenerate form's output is compared with the plain call's at the timed size.
Writes one JSON document."""
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


def four_blocks(T):
    """The four-block list of the tests stretched to T frames: lengths in the ratio 5 : 16 : 17 : 10, nudged off the multiples of 16."""
    n = [max(1, T * w // 48) for w in (5, 16, 17)]
    n = [x + 1 if x % 16 == 0 else x for x in n]
    n.append(T - sum(n))
    assert n[3] >= 1
    return [dict(nframes=n[0]), dict(nframes=n[1], prep="inversion", wait=0.3, prep_time=0.021, prep_eff=0.95),
            dict(nframes=n[2], prep="t2", wait=0.25, prep_time=0.040), dict(nframes=n[3], prep="t2", wait=0.01, prep_time=0.080, prep_eff=0.9)]


def measure(K, T, S, runs, calls):
    from qmri_pnp_recon_poc_amd import engine, synth
    from qmri_pnp_recon_poc_amd._lib import EpgParams
    t1, t2 = atoms(K)
    alpha, tr, te = synth.flip_angle_train(T), np.full(T, 0.012), np.full(T, 0.002)
    eng, hip = engine.Engine(0), engine._hip_runtime()
    d_t1, d_t2, d_F = ptrs = [C.c_void_p() for _ in range(3)]
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    p_inv, p_seq = EpgParams(S, 1, 0.021, 0.95, 1), EpgParams(S, 0, 0.0, 1.0, 1)
    one = engine.sequence_arguments([dict(nframes=T, prep="inversion", prep_time=0.021, prep_eff=0.95)], 1, T)
    four = engine.sequence_arguments(four_blocks(T), 2, T)
    try:
        for d, nb in ((d_t1, K * 8), (d_t2, K * 8), (d_F, K * T * 8)):
            assert hip.hipMalloc(C.byref(d), nb) == 0
        assert hip.hipMemcpy(d_t1, t1.ctypes.data, K * 8, 1) == 0 and hip.hipMemcpy(d_t2, t2.ctypes.data, K * 8, 1) == 0

        def plain():
            eng._check(eng.L.qmri_dict_simulate_dev(eng.h, K, T, vp(alpha), vp(tr), vp(te), d_t1, d_t2, None, C.byref(p_inv), d_F))

        def seq(sq):
            return lambda: eng._check(eng.L.qmri_dict_simulate_seq_dev(eng.h, K, T, vp(alpha), vp(tr), vp(te), d_t1, d_t2, None, C.byref(p_seq), C.byref(sq[1]), d_F))

        arms = [("simulate", plain, 1), ("seq_degenerate", seq(one), 1), ("seq_four_block", seq(four), 2)]
        outs = []
        for _, fn, _ in arms[:2]:                                    # the same numbers at the timed size
            fn()
            F = np.empty(K * T, np.float64)
            assert hip.hipMemcpy(F.ctypes.data, d_F, F.nbytes, 2) == 0
            outs.append(F)
        same = bool(np.array_equal(outs[0], outs[1]))
        del outs, F
        times = {name: [] for name, _, _ in arms}
        for rnd in range(runs + 1):                                  # (the first round warms up: code objects, allocator)
            for name, fn, _ in arms:
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                if rnd:
                    times[name].append(1e3 * (time.perf_counter() - t0) / calls)
    finally:
        for d in ptrs:
            hip.hipFree(d)
        eng.close()
    rows = {}
    for name, _, cycles in arms:
        t = times[name]
        rows[name] = {"ms_per_call_runs": t, "min_ms": min(t), "median_ms": float(np.median(t)), "spread_ms": max(t) - min(t), "cycles": cycles,
                      "ps_per_atom_frame": 1e9 * float(np.median(t)) / (float(K) * T * cycles), "ratio_to_simulate": float(np.median(t)) / float(np.median(times["simulate"]))}
    return {"K": K, "T": T, "S": S, "runs": runs, "calls_per_run": calls, "four_block_nframes": [b["nframes"] for b in four_blocks(T)],
            "degenerate_equals_simulate": same, "arms": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=98304)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--S", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epgseq_times.json"))
    a = ap.parse_args()
    r = measure(a.K, a.T, a.S, a.runs, a.calls)
    print(json.dumps(r), flush=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/epgseq_times.py", "device": "MI355X", "runs": [r]}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
