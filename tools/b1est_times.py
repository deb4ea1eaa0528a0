#!/usr/bin/env python3
"""Device time of the B1 estimate from the fingerprints (qmri_dict_group_scores_dev, qmri_b1_pool_dev, qmri_b1_estimate_dev)
beside two routes to the same products that exist without it.

    python3 tools/b1est_times.py [--side 224] [--G 21] [--grid 128 128] [--window 4] [--reps 20] [--out profiles/b1est_times.json]

Workload: that of tools/dictg_times.py -- side x side pixels, s = 10, G groups of grid[0] x grid[1] atoms each (21 x 16 384 = 344 064 by
default), every pixel a noisy scaled atom of the group a smooth B1 map names.  Each step runs in a process of its own under its own time limit
and times its launches with hipEvents on the engine's stream (median and least of --reps after 3 warm-up calls; every array stays on the device):
  scores      stage 1: one qmri_dict_group_scores_dev call
  pool        stage 2: one qmri_b1_pool_dev call on the scores of stage 1
  estimate    the composed qmri_b1_estimate_dev call
  all_atoms   one qmri_dict_match_dev call over all K atoms (the same products behind the f16 filter, B1 left free per pixel)
  grouped_G   G qmri_dict_match_grouped_dev calls, call g with the constant selector group_val[g] (what stage 1 is defined by)
Writes one JSON document with the ratios scores / all_atoms and scores / grouped_G and stage 2's streaming floor."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
STEPS = ("scores", "pool", "estimate", "all_atoms", "grouped_G")
STEP_LIMIT_S = 300
HBM_BYTES_PER_S = 6.29e12           # the MI355X's measured HBM copy bandwidth (8.0e12 by the data sheet): the yardstick of the streaming floor


def step(name, a):
    from dictg_times import Dev, workload
    from qmri_pnp_recon_poc_amd import engine
    w = workload(a.side, a.G, a.grid)
    npix, s, Q, G = w["X"].shape[0], w["X"].shape[1], w["lut"].shape[1], a.G
    eng = engine.Engine(0)
    dev = Dev(eng)
    name_buf = C.create_string_buffer(256)
    dev.hip.hipDeviceGetName.argtypes = [C.c_char_p, C.c_int, C.c_int]
    out = {"npix": npix, "K": int(w["D"].shape[0]), "G": G, "s": s, "window": a.window,
           "device": name_buf.value.decode() if dev.hip.hipDeviceGetName(name_buf, 256, 0) == 0 else "unknown"}
    try:
        dX = dev.put(w["X"].ravel(order="F"))
        eng.set_dictionary(w["D"], w["normD"], w["lut"])
        b1, grp, conf = dev.put(nbytes=8 * npix), dev.put(nbytes=4 * npix), dev.put(nbytes=8 * npix)
        if name in ("scores", "pool", "estimate", "grouped_G"):
            eng.set_dictionary_groups(w["gp"], w["gv"])
        if name == "scores":
            dS = dev.put(nbytes=4 * npix * G)
            out.update(dev.time(lambda: eng.group_scores_dev(dX, npix, dS), a.reps))
        elif name == "pool":
            dS = dev.put(nbytes=4 * npix * G)
            eng.group_scores_dev(dX, npix, dS)
            eng.synchronize()
            out.update(dev.time(lambda: eng.b1_pool_dev(w["gv"], a.side, a.side, 1, dS, 0, a.window, b1, grp, conf), a.reps))
        elif name == "estimate":
            out.update(dev.time(lambda: eng.estimate_b1_dev(dX, a.side, a.side, 1, 0, a.window, b1, grp, conf), a.reps))
        elif name == "all_atoms":
            o = [dev.put(nbytes=4 * npix * Q), dev.put(nbytes=8 * npix), dev.put(nbytes=4 * npix), dev.put(nbytes=4 * npix)]
            out.update(dev.time(lambda: eng.dict_match_dev(dX, npix, *o), a.reps))
        else:
            mt = [dev.put(nbytes=4 * npix) for _ in range(G)]
            sel = [dev.put(np.full(npix, v)) for v in w["gv"]]

            def calls():
                for g in range(G):
                    eng.dict_match_dev(dX, npix, d_mt=mt[g], d_sel=sel[g])
            out.update(dev.time(calls, a.reps))
    finally:
        eng.synchronize()
        dev.free()
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--G", type=int, default=21)
    ap.add_argument("--grid", type=int, nargs=2, default=[128, 128])
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "b1est_times.json"))
    a = ap.parse_args()
    if a.step:                                                        # a child: one step, one JSON line
        print("B1EST_STEP " + json.dumps(step(a.step, a)), flush=True)
        return
    res = {"tool": "tools/b1est_times.py", "device": None, "side": a.side, "G": a.G, "grid": a.grid, "window": a.window}
    for name in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--side", str(a.side), "--G", str(a.G), "--grid", str(a.grid[0]), str(a.grid[1]),
                                "--window", str(a.window), "--reps", str(a.reps)], check=True, capture_output=True, text=True, timeout=STEP_LIMIT_S)
            res[name] = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("B1EST_STEP "))[len("B1EST_STEP "):])
        except (subprocess.SubprocessError, StopIteration) as e:
            res[name] = {"error": (getattr(e, "stderr", None) or repr(e))[-600:]}
            print(json.dumps(res), flush=True)
            break                                                     # (nothing more is started on the device after a failed step)
        res["device"] = res[name].pop("device", res["device"])
        print(name, json.dumps(res[name]), flush=True)
    else:
        res["scores_over_all_atoms"] = res["scores"]["median_ms"] / res["all_atoms"]["median_ms"]
        res["scores_over_grouped_G"] = res["scores"]["median_ms"] / res["grouped_G"]["median_ms"]
        npix = res["scores"]["npix"]
        # stage 2 as built: pass 1 reads the scores (4 B) and writes T (8 B), pass 2 reads T (8 B); the outputs are 20 B per pixel
        res["pool_floor_ms"] = 1e3 * (a.G * npix * (4 + 8 + 8) + npix * 20) / HBM_BYTES_PER_S
        res["pool_over_floor"] = res["pool"]["median_ms"] / res["pool_floor_ms"]
        print(json.dumps({k: res[k] for k in ("scores_over_all_atoms", "scores_over_grouped_G", "pool_floor_ms", "pool_over_floor")}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
