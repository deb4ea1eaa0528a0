#!/usr/bin/env python3
"""Device time of the grouped dictionary match (qmri_dict_match_grouped_dev) against what the ungrouped match can do on the
same inputs.

    python3 tools/dictg_times.py [--side 224] [--G 21] [--grid 128 128] [--reps 20] [--out profiles/dictg_times.json]

Workload: side x side pixels, s = 10, G groups of grid[0] x grid[1] atoms each (21 x 16 384 = 344 064 by default), a smooth B1 map over the
groups' range; every pixel is a noisy scaled atom of its own group.  Each step runs in a process of its own under its own time limit and times
its launches with hipEvents on the engine's stream (median of --reps after 3 warm-up calls; X, sel and the outputs stay on the device):
  grouped     one qmri_dict_match_grouped_dev call
  all_atoms   (a) one qmri_dict_match_dev call over all K atoms
  per_group   (b) G qmri_dict_match_dev calls, each on the host-gathered pixels of one group against that group's sub-dictionary
              (qmri_set_dictionary per group is NOT timed: the sum is the matches alone)
  kernels     the grouped step under `rocprofv3 --kernel-trace --stats`: the share of the bucketing kernels (k_dictg_*) in the call's kernel time
Writes one JSON document with the ratios grouped / all_atoms and grouped / per_group."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = {"grouped": 240, "all_atoms": 240, "per_group": 420, "kernels": 420}


def workload(side, G, grid, s=10, seed=0):
    from qmri_pnp_recon_poc_amd import synth
    rng = np.random.default_rng(seed)
    d0 = synth.make_dictionary(T=200, n_t1=grid[0], n_t2=grid[1], s=s)
    n = d0["D"].shape[0]
    w = rng.standard_normal((G, s)).astype(np.float32)
    D = np.concatenate([d0["D"] * (1.0 + 0.05 * w[g])[None, :] for g in range(G)]).astype(np.float32)   # the same (T1, T2) grid seen through G transmit scales
    D /= np.linalg.norm(D, axis=1, keepdims=True).astype(np.float32)
    gv = np.linspace(0.7, 1.3, G) if G > 1 else np.array([1.0])
    lut = np.concatenate([np.tile(d0["lut"], (G, 1)), np.repeat(gv, n)[:, None].astype(np.float32)], axis=1)
    nd = np.tile(d0["normD"], G).astype(np.float32)
    yy, xx = np.mgrid[0:side, 0:side] / max(side - 1, 1)
    b1 = (gv[0] + (gv[-1] - gv[0]) * (0.7 * xx + 0.3 * yy * yy)).ravel()
    gp = np.arange(G + 1) * n
    grp = np.abs(b1[:, None] - gv[None, :]).argmin(1)
    atom = gp[grp] + rng.integers(0, n, b1.size)
    X = D[atom].astype(np.complex128) * ((0.5 + rng.random(b1.size)) * np.exp(2j * np.pi * rng.random(b1.size)))[:, None]
    X += 0.01 * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    return {"D": D, "normD": nd, "lut": lut, "gp": gp, "gv": gv, "b1": b1, "grp": grp, "X": X}


class Dev:
    """device buffers and hipEvent timing on a stream the engine is given"""
    def __init__(self, eng):
        from qmri_pnp_recon_poc_amd import engine
        self.hip, self.bufs = engine._hip_runtime(), []
        h = self.hip
        h.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        h.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        h.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        h.hipEventSynchronize.argtypes = [C.c_void_p]
        h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.stream, self.e0, self.e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert h.hipStreamCreate(C.byref(self.stream)) == 0 and h.hipEventCreate(C.byref(self.e0)) == 0 and h.hipEventCreate(C.byref(self.e1)) == 0
        eng.set_stream(self.stream.value)

    def put(self, a=None, nbytes=0):
        d = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(d), a.nbytes if a is not None else nbytes) == 0
        if a is not None:
            a = np.ascontiguousarray(a)
            assert self.hip.hipMemcpy(d, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
        self.bufs.append(d)
        return d.value

    def time(self, fn, reps):
        ms = []
        for i in range(reps + 3):
            assert self.hip.hipEventRecord(self.e0, self.stream) == 0
            fn()
            assert self.hip.hipEventRecord(self.e1, self.stream) == 0 and self.hip.hipEventSynchronize(self.e1) == 0
            t = C.c_float(0)
            assert self.hip.hipEventElapsedTime(C.byref(t), self.e0, self.e1) == 0
            if i >= 3:
                ms.append(t.value)
        return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": reps}

    def free(self):
        for d in self.bufs:
            self.hip.hipFree(d)


def step(name, a):
    from qmri_pnp_recon_poc_amd import engine
    w = workload(a.side, a.G, a.grid)
    npix, s, Q = w["X"].shape[0], w["X"].shape[1], w["lut"].shape[1]
    eng = engine.Engine(0)
    dev = Dev(eng)
    name_buf = C.create_string_buffer(256)
    dev.hip.hipDeviceGetName.argtypes = [C.c_char_p, C.c_int, C.c_int]
    out = {"npix": npix, "K": int(w["D"].shape[0]), "G": a.G, "s": s,
           "device": name_buf.value.decode() if dev.hip.hipDeviceGetName(name_buf, 256, 0) == 0 else "unknown"}
    try:
        o = [dev.put(nbytes=4 * npix * Q), dev.put(nbytes=8 * npix), dev.put(nbytes=4 * npix), dev.put(nbytes=4 * npix)]
        if name in ("grouped", "all_atoms"):
            dX = dev.put(w["X"].ravel(order="F"))
            eng.set_dictionary(w["D"], w["normD"], w["lut"])
            if name == "grouped":
                eng.set_dictionary_groups(w["gp"], w["gv"])
                dsel, dgrp = dev.put(w["b1"]), dev.put(nbytes=4 * npix)
                out.update(dev.time(lambda: eng.dict_match_dev(dX, npix, *o, d_sel=dsel, d_grp=dgrp), a.reps))
            else:
                out.update(dev.time(lambda: eng.dict_match_dev(dX, npix, *o), a.reps))
        else:
            per = []
            for g in range(a.G):
                idx = np.nonzero(w["grp"] == g)[0]
                if idx.size == 0:
                    continue
                lo, hi = w["gp"][g], w["gp"][g + 1]
                eng.set_dictionary(w["D"][lo:hi], w["normD"][lo:hi], w["lut"][lo:hi])
                dXg = dev.put(w["X"][idx].ravel(order="F"))
                per.append(dict(dev.time(lambda: eng.dict_match_dev(dXg, idx.size, *o), a.reps), group=g, npix=int(idx.size)))
            out.update(median_ms=float(sum(p["median_ms"] for p in per)), min_ms=float(sum(p["min_ms"] for p in per)), groups=per, reps=a.reps)
    finally:
        eng.synchronize()
        dev.free()
        eng.close()
    return out


def kernel_share(a):
    """the grouped step under rocprofv3 --kernel-trace --stats (a run of its own): total time per kernel name"""
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--step", "grouped",
                        "--side", str(a.side), "--G", str(a.G), "--grid", str(a.grid[0]), str(a.grid[1]), "--reps", str(a.reps)],
                       check=True, capture_output=True, timeout=STEP_LIMIT_S["kernels"])
        tot = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                m = re.search(r"k_dict\w*", r["Name"])
                if m:
                    tot[m.group(0)] = tot.get(m.group(0), 0.0) + float(r["TotalDurationNs"]) / 1e6
    call = {k: v for k, v in tot.items() if k != "k_dictg_repack"}
    allms = sum(call.values())
    return {"total_ms_by_kernel": tot, "bucketing_share": (sum(v for k, v in call.items() if k.startswith("k_dictg_")) / allms) if allms else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--G", type=int, default=21)
    ap.add_argument("--grid", type=int, nargs=2, default=[128, 128])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", choices=["grouped", "all_atoms", "per_group"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dictg_times.json"))
    a = ap.parse_args()
    if a.step:                                                        # a child: one step, one JSON line
        print("DICTG_STEP " + json.dumps(step(a.step, a)), flush=True)
        return
    res = {"tool": "tools/dictg_times.py", "device": None, "side": a.side, "G": a.G, "grid": a.grid}
    for name in ("grouped", "all_atoms", "per_group"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--side", str(a.side), "--G", str(a.G), "--grid", str(a.grid[0]), str(a.grid[1]),
                                "--reps", str(a.reps)], check=True, capture_output=True, text=True, timeout=STEP_LIMIT_S[name])
            res[name] = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("DICTG_STEP "))[len("DICTG_STEP "):])
        except (subprocess.SubprocessError, StopIteration) as e:
            res[name] = {"error": (getattr(e, "stderr", None) or repr(e))[-600:]}
            print(json.dumps(res), flush=True)
            break                                                     # (nothing more is started on the device after a failed step)
        res["device"] = res[name].pop("device", res["device"])
        print(name, json.dumps({k: v for k, v in res[name].items() if k != "groups"}), flush=True)
    else:
        res["grouped_over_all_atoms"] = res["grouped"]["median_ms"] / res["all_atoms"]["median_ms"]
        res["grouped_over_per_group"] = res["grouped"]["median_ms"] / res["per_group"]["median_ms"]
        try:
            res["kernels"] = kernel_share(a)
        except (subprocess.SubprocessError, OSError, KeyError, ValueError) as e:
            res["kernels"] = {"error": repr(e)[:400]}
        print(json.dumps({k: res[k] for k in ("grouped_over_all_atoms", "grouped_over_per_group", "kernels")}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
