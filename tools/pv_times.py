"""The tissue-fraction unmixing on one MI355X at 224 x 224 pixels of s = 10 channels, for C = 3 and C = 8 components, in
both modes.

Prints one JSON line and writes it to profiles/pv_times.json (or --out); per (C, mode):
  host_ms        qmri_dict_unmix_dev on device arrays, all five outputs (launch + wait), host clock, best and median of 20 after 3 warm-ups
  kernel_us      k_pv_unmix alone from a kernel trace (rocprofv3 --kernel-trace) of the same 23 calls in a run of its own: best and median
  floor_us       one read of 16 s bytes and one write of 8 (2 C + 3) + 4 bytes per pixel at the HBM rate in --hbm-gbs; times_floor = best kernel
                 time / floor (the kernel is not expected near it: the work is the per-pixel active-set iteration, in fp64)
The pixels are mixtures of the components with about 40 % of the weights exactly 0 plus 1 % noise, the family the tests use.
Every step runs as a child process of its own under `timeout -k 10 <seconds>`; the first one that fails or runs out of time ends the run, and
nothing more is started on the GPU.

    python tools/pv_times.py
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
N, S_CH = 224, 10
# (T1, T2) in seconds of the components: white matter, grey matter, CSF; then fat, two lesions, a short and a long species (nearly dependent in ten
# channels: the unit-diagonal Gram matrix has condition 1e9, so C = 8 is the slow end of what the entry point accepts)
TISSUES = [(0.85, 0.065), (1.40, 0.095), (2.80, 0.28), (0.35, 0.07), (1.90, 0.16), (1.10, 0.045), (0.20, 0.02), (3.80, 0.55)]
CONFIGS = ((3, "real"), (3, "phase"), (8, "real"), (8, "phase"))
WARMUP, REPS = 3, 20
STEP_LIMIT_S = 120


def step(nc, mode):
    from qmri_pnp_recon_poc_amd import engine as E, synth
    dic = synth.make_dictionary(T=200, n_t1=32, n_t2=16, s=S_CH)
    e = E.Engine(0)
    e.set_dictionary(dic["D"], dic["normD"], dic["lut"])
    atoms = e.nearest_atoms(TISSUES[:nc])
    info = e.set_components(atoms)
    A = (dic["normD"][atoms - 1].astype(np.float64)[:, None] * dic["D"][atoms - 1].astype(np.float64)).T
    rng = np.random.default_rng(nc)
    npix = N * N
    wt = rng.uniform(0.05, 1.0, (npix, nc)) * (rng.uniform(size=(npix, nc)) >= 0.4)
    B = wt @ A.T + 0.01 * np.linalg.norm(A, axis=0).mean() * rng.standard_normal((npix, S_CH))
    X = B * np.exp(1j * rng.uniform(-np.pi, np.pi, npix))[:, None] if mode == "phase" else B.astype(np.complex128)
    hip = E._hip_runtime()
    xb = np.ascontiguousarray(X.ravel(order="F"))
    sizes = {"X": xb.nbytes, "w": 8 * npix * nc, "frac": 8 * npix * nc, "pd": 16 * npix, "res": 8 * npix, "flags": 4 * npix}
    d = {k: C.c_void_p() for k in sizes}
    for k, nb in sizes.items():
        assert hip.hipMalloc(C.byref(d[k]), nb) == 0
    assert hip.hipMemcpy(d["X"], xb.ctypes.data_as(C.c_void_p), xb.nbytes, 1) == 0
    times = []
    for _ in range(WARMUP + REPS):
        t0 = time.perf_counter()
        e.tissue_fractions_dev(d["X"].value, npix, mode=mode, d_w=d["w"].value, d_frac=d["frac"].value, d_pd=d["pd"].value, d_res=d["res"].value,
                               d_flags=d["flags"].value)
        e.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    flags = np.empty(npix, np.int32)
    assert hip.hipMemcpy(flags.ctypes.data_as(C.c_void_p), d["flags"], flags.nbytes, 2) == 0
    for v in d.values():
        hip.hipFree(v)
    e.close()
    return {"C": nc, "mode": mode, "min_pivot": info["min_pivot"], "host_ms": round(min(times[WARMUP:]), 4),
            "host_median_ms": round(float(np.median(times[WARMUP:])), 4), "pixels_at_the_cap": int(np.count_nonzero(flags & 1))}


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
    ap.add_argument("--step", nargs=2)
    ap.add_argument("--hbm-gbs", type=float, default=6300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pv_times.json"))
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(int(a.step[0]), a.step[1])))
        return 0
    out = {"N": N, "s": S_CH, "pixels": N * N, "warmup": WARMUP, "reps": REPS, "hbm_gbs": a.hbm_gbs, "configs": []}
    for nc, mode in CONFIGS:
        cfg = child(["--step", str(nc), mode])
        if cfg is None:
            print(json.dumps({"failed_step": f"C={nc} {mode}", **out}))
            return 1
        with tempfile.TemporaryDirectory() as td:                      # the kernel trace: a run of its own
            if child(["--step", str(nc), mode], trace_dir=td) is None:
                print(json.dumps({"failed_step": f"trace C={nc} {mode}", **out}))
                return 1
            ks = kernel_times(td, "k_pv_unmix")[WARMUP:]
        floor_us = N * N * (16.0 * S_CH + 8.0 * (2 * nc + 3) + 4.0) / (a.hbm_gbs * 1e9) * 1e6
        cfg.update({"kernel_us": round(min(ks), 2), "kernel_median_us": round(float(np.median(ks)), 2), "launches_traced": len(ks),
                    "floor_us": round(floor_us, 2), "times_floor": round(min(ks) / floor_us, 2)})
        out["configs"].append(cfg)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
