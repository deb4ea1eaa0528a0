"""The sub-grid refinement of a dictionary match on one MI355X at 224 x 224 pixels against the K = 98 304 dictionary
(384 x 256 grid, s = 10), cols (T1, T2), with the grid match of the same pixels as the yardstick.

Prints one JSON line and writes it to profiles/refine_times.json (or --out):
  refine.host_ms     qmri_dict_refine_dev on device arrays, all six outputs (launch + wait), host clock, best and median of 20 after 3 warm-ups
  refine.kernel_us   k_dict_refine alone from a kernel trace (rocprofv3 --kernel-trace) of the same 23 calls in a run of its own: best and median
  match.host_ms      qmri_dict_match_dev of the same pixels (qmap, pd, mt, dm), the same way
  flags              pixels per flag of the refinement, and the error of T1 / T2 against the truth before and after (median, relative)
  bound              bytes of atom rows a pixel gathers (128 per row, 1 + 2 P rows per centre visited) and the streaming floor of X and the outputs at
                     the HBM rate in --hbm-gbs; the kernel is not expected near the floor: the work is a dependent chain of 16-lane butterflies
The pixels are off-grid fingerprints of the dictionary's own signal model with a random complex PD and 40 dB noise.
Every step runs as a child process of its own under `timeout -k 10 <seconds>`; the first one that fails or runs out of time ends the run, and
nothing more is started on the GPU.

    python tools/refine_times.py
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, S_CH, T, N1, N2 = 224, 10, 200, 384, 256
WARMUP, REPS = 3, 20
STEP_LIMIT_S = 240


def case():
    from qmri_pnp_recon_poc_amd import synth
    dic = synth.make_dictionary(T=T, n_t1=N1, n_t2=N2, s=S_CH)
    rng = np.random.default_rng(30)
    npix = N * N
    t1 = np.exp(np.interp(rng.uniform(1.0, N1 - 2.0, npix), np.arange(N1), np.log(dic["t1_grid"])))
    t2 = np.exp(np.interp(rng.uniform(1.0, N2 - 2.0, npix), np.arange(N2), np.log(dic["t2_grid"])))
    pd = rng.uniform(0.5, 2.0, npix) * np.exp(2j * np.pi * rng.uniform(0, 1, npix))
    X = (synth.simulate_fingerprints(T, t1, t2) @ dic["V"]) * pd[:, None]
    sig = np.sqrt(np.mean(np.abs(X) ** 2) / 10 ** 4.0 / 2)
    X = X + sig * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    return dic, X, np.stack([t1, t2], axis=1)


def step(which):
    from qmri_pnp_recon_poc_amd import engine as E
    dic, X, truth = case()
    npix, Q, P = N * N, 2, 2
    e = E.Engine(0)
    e.set_dictionary(dic["D"], dic["normD"], dic["lut"])
    t0 = time.perf_counter()
    info = e.set_refine((0, 1))
    set_ms = 1e3 * (time.perf_counter() - t0)
    hip = E._hip_runtime()
    xb = np.ascontiguousarray(X.ravel(order="F"))
    sizes = {"X": xb.nbytes, "mq": 4 * npix * Q, "mpd": 8 * npix, "mt": 4 * npix, "dm": 4 * npix, "qmap": 8 * npix * Q, "pd": 16 * npix, "res": 8 * npix,
             "t": 8 * npix * P, "centre": 4 * npix, "flags": 4 * npix}
    d = {k: C.c_void_p() for k in sizes}
    for k, nb in sizes.items():
        assert hip.hipMalloc(C.byref(d[k]), nb) == 0
    assert hip.hipMemcpy(d["X"], xb.ctypes.data_as(C.c_void_p), xb.nbytes, 1) == 0

    def match():
        e.dict_match_dev(d["X"].value, npix, d_qmap=d["mq"].value, d_pd=d["mpd"].value, d_mt=d["mt"].value, d_dm=d["dm"].value)

    def refine():
        e.dict_refine_dev(d["X"].value, npix, d["dm"].value, d_qmap=d["qmap"].value, d_pd=d["pd"].value, d_res=d["res"].value, d_t=d["t"].value,
                          d_centre=d["centre"].value, d_flags=d["flags"].value)

    match()                                                            # dm for the refinement
    e.synchronize()
    times = []
    for _ in range(WARMUP + REPS):
        t0 = time.perf_counter()
        (match if which == "match" else refine)()
        e.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    out = {"step": which, "host_ms": round(min(times[WARMUP:]), 4), "host_median_ms": round(float(np.median(times[WARMUP:])), 4)}
    if which == "refine":
        flags, mq, rq = np.empty(npix, np.int32), np.empty(npix * Q, np.float32), np.empty(npix * Q, np.float64)
        for a, k in ((flags, "flags"), (mq, "mq"), (rq, "qmap")):
            assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), d[k], a.nbytes, 2) == 0
        eg = np.abs(mq.reshape((npix, Q), order="F") - truth) / truth
        er = np.abs(rq.reshape((npix, Q), order="F") - truth) / truth
        out.update({"set_refine_ms": round(set_ms, 2), "count": info["count"].tolist(),
                    "flags": {name: int(np.count_nonzero(flags & bit)) for name, bit in E.REFINE_FLAGS.items()},
                    "grid_median_rel_err": [float(v) for v in np.median(eg, axis=0)], "refined_median_rel_err": [float(v) for v in np.median(er, axis=0)],
                    "better_than_grid": [float(v) for v in np.mean(er < eg, axis=0)]})
    for v in d.values():
        hip.hipFree(v)
    e.close()
    return out


def kernel_times(trace_dir, name):
    """Durations in microseconds of the launches whose kernel name contains `name`, from the kernel-trace CSVs under trace_dir."""
    out = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if name in row.get("Kernel_Name", ""):
                out.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return out


def child(args, trace_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    if trace_dir:                                                      # (the program itself goes after `--`; a trace and nothing else)
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "--"] + cmd
    r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return None
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("match", "refine"))
    ap.add_argument("--hbm-gbs", type=float, default=6300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_times.json"))
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step)))
        return 0
    P = 2
    out = {"N": N, "s": S_CH, "pixels": N * N, "K": N1 * N2, "cols": [0, 1], "snr_db": 40, "warmup": WARMUP, "reps": REPS, "hbm_gbs": a.hbm_gbs}
    for which in ("match", "refine"):
        r = child(["--step", which])
        if r is None:
            print(json.dumps({"failed_step": which, **out}))
            return 1
        out[which] = r
    with tempfile.TemporaryDirectory() as td:                          # the kernel trace: a run of its own
        if child(["--step", "refine"], trace_dir=td) is None:
            print(json.dumps({"failed_step": "trace", **out}))
            return 1
        ks = kernel_times(td, "k_dict_refine")[WARMUP:]
    npix = N * N
    moved = out["refine"]["flags"]["moved"]
    floor_us = npix * (16.0 * S_CH + 4.0 + 8.0 * 2 + 16.0 + 8.0 + 8.0 * P + 4.0 + 4.0) / (a.hbm_gbs * 1e9) * 1e6
    out["refine"].update({"kernel_us": round(min(ks), 2), "kernel_median_us": round(float(np.median(ks)), 2), "launches_traced": len(ks)})
    out["bound"] = {"row_bytes_per_centre": 128 * (1 + 2 * P), "centres_per_pixel_at_least": round(1.0 + moved / npix, 3),
                    "atom_table_mb": round(N1 * N2 * 128 / 1e6, 1), "stream_floor_us": round(floor_us, 2), "times_floor": round(min(ks) / floor_us, 2)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
