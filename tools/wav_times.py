"""Joint wavelet soft-thresholding on one MI355X, at 224 x 224 x 10 with 3 levels of Daubechies-2, joint, complex, for one
slice and for 30 slices.

Prints one JSON line and writes it to profiles/wav_times.json (or --out); per slice count:
  prox_host_ms       qmri_wavelet_prox_dev on device arrays without cmax (2 L + 1 launches + wait), host clock, best of 20 after 3 warm-ups
  launch_us          the 2 L + 1 launches of one prox in their order (fwd 1 .. L, shrink, inv L .. 1) from a kernel trace (rocprofv3 --kernel-trace) of
                     the same 23 calls in a run of its own: the median of each launch over the calls
  kernels_sum_us     their sum per call: best and median;  span_us: first launch's start to last launch's end, best and median (the gaps between
                     dependent launches are the difference)
  floor_us           the streaming floor (8/3 + 2 + 8/3) x 16 N M s bytes per slice -- each transform reads and writes 1 + 1/4 + 1/16 + ... of the stack, the
                     shrink reads and writes it once -- at the HBM rate in --hbm-gbs (default 6300, the rate section 25 uses); times_floor = best sum / floor
  admm_wav_ms_per_iter
                     one ADMM iteration (qmri_pnp_admm_dev's wall clock / iterations, best of 3 calls of 10 iterations) with the wavelet step on the
                     operator of tools/llr_times.py (gridded spiral, S = 771, T = 200), and its stage split
Every step runs as a child process of its own under `timeout -k 10 <seconds>`; the first one that fails or runs out of time ends the run, and
nothing more is started on the GPU.

    python tools/wav_times.py
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
N, S_CH, LEVELS, FILTER, TAU = 224, 10, 3, "db2", 0.05
SLICES = (1, 30)
WARMUP, REPS = 3, 20
ADMM_ITERS, ADMM_CALLS = 10, 3
STEP_LIMIT_S = 150
NL = 2 * LEVELS + 1
NAMES = [f"fwd{l}" for l in range(1, LEVELS + 1)] + ["shrink"] + [f"inv{l}" for l in range(LEVELS, 0, -1)]


def data(S):
    rng = np.random.default_rng(0)
    a, b = np.meshgrid(np.arange(N) / N, np.arange(N) / N, indexing="ij")
    comps = np.stack([np.exp(-((a - 0.4) ** 2 + (b - 0.55) ** 2) * 8.0), np.cos(2 * np.pi * (a + 0.5 * b)), ((a - 0.6) ** 2 + (b - 0.3) ** 2 < 0.06) * 1.0], -1)
    mix = (rng.standard_normal((3, S_CH)) + 1j * rng.standard_normal((3, S_CH))) * (0.5 ** np.arange(S_CH))
    X = comps @ mix + 1e-3 * (rng.standard_normal((N, N, S_CH)) + 1j * rng.standard_normal((N, N, S_CH)))
    return np.stack([X * (1.0 + 0.01 * k) for k in range(S)])


def step_prox(S):
    from qmri_pnp_recon_poc_amd import engine as E
    e = E.Engine(0)
    hip = E._hip_runtime()
    xb = np.concatenate([E._cbuf(x) for x in data(S)])
    d_x, d_o = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_x), xb.nbytes) == 0 and hip.hipMalloc(C.byref(d_o), xb.nbytes) == 0
    assert hip.hipMemcpy(d_x, xb.ctypes.data_as(C.c_void_p), xb.nbytes, 1) == 0
    times, P = [], 1 << LEVELS
    for k in range(WARMUP + REPS):
        t0 = time.perf_counter()
        e.wavelet_prox_dev(d_x.value, (N, N, S_CH, S), TAU, d_o.value, levels=LEVELS, filter=FILTER, offset=(k % P, (3 * k) % P), want_cmax=False)
        times.append(1e3 * (time.perf_counter() - t0))
    hip.hipFree(d_x)
    hip.hipFree(d_o)
    e.close()
    return {"slices": S, "prox_host_ms": round(min(times[WARMUP:]), 4), "prox_host_median_ms": round(float(np.median(times[WARMUP:])), 4)}


def step_admm(S):
    from qmri_pnp_recon_poc_amd import engine as E, synth
    dic = synth.make_dictionary(T=200, n_t1=32, n_t2=16, s=S_CH)
    fp, k = E.build_spiral(N, 771, 200)
    e = E.Engine(0)
    e.set_operator(N, N, dic["V"], fp, k, max_batch=S)
    e.set_wavelet(TAU, levels=LEVELS, filter=FILTER, shift=True)
    X = data(1)[0].real + 0j
    y = e.forward(X)
    ys = np.stack([y * (1.0 + 0.01 * j) for j in range(S)])
    e.pnp_admm_batch(ys, slices_per_launch=S, iters=2)                 # warm-up
    walls = []
    e.profile_enable(0)
    for _ in range(ADMM_CALLS):
        e.pnp_admm_batch(ys, slices_per_launch=S, iters=ADMM_ITERS)
        walls.append(e.health()["last_call_wall_ms"])
    e.profile_enable(3)                                                # the stage split, from marks that are not waited for inside the loop
    e.pnp_admm_batch(ys, slices_per_launch=S, iters=ADMM_ITERS)
    st = e.health()["last_call_stage_ms"]
    e.close()
    return {"slices": S, "ms_per_iter": round(min(walls) / ADMM_ITERS, 4), "stage_ms_per_iter": {k_: round(v / ADMM_ITERS, 4) for k_, v in st.items()}}


def wav_launches(trace_dir):
    """(start, end) in microseconds of the k_wav_* launches in the kernel-trace CSVs under trace_dir, in start order."""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "k_wav_" in row.get("Kernel_Name", ""):
                rows.append((int(row["Start_Timestamp"]) / 1e3, int(row["End_Timestamp"]) / 1e3))
    return sorted(rows)


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
    ap.add_argument("--step", nargs="+")
    ap.add_argument("--hbm-gbs", type=float, default=6300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wav_times.json"))
    a = ap.parse_args()
    if a.step:
        kind, S = a.step[0], int(a.step[1])
        print(json.dumps(step_prox(S) if kind == "prox" else step_admm(S)))
        return 0
    out = {"N": N, "s": S_CH, "levels": LEVELS, "filter": FILTER, "joint": 1, "tau": TAU, "warmup": WARMUP, "reps": REPS, "admm_iters": ADMM_ITERS,
           "hbm_gbs": a.hbm_gbs, "launch_names": NAMES, "configs": []}
    for S in SLICES:
        cfg = child(["--step", "prox", str(S)])
        if cfg is None:
            print(json.dumps({"failed_step": f"prox slices={S}", **out}))
            return 1
        with tempfile.TemporaryDirectory() as td:                      # the kernel trace: a run of its own
            if child(["--step", "prox", str(S)], trace_dir=td) is None:
                print(json.dumps({"failed_step": f"prox trace slices={S}", **out}))
                return 1
            ls = wav_launches(td)
        if len(ls) != NL * (WARMUP + REPS):
            print(json.dumps({"failed_step": f"prox trace slices={S}: {len(ls)} launches traced", **out}))
            return 1
        calls = np.array(ls).reshape(WARMUP + REPS, NL, 2)[WARMUP:]
        dur = calls[:, :, 1] - calls[:, :, 0]
        sums, span = dur.sum(axis=1), calls[:, -1, 1] - calls[:, 0, 0]
        floor_us = (8.0 / 3 + 2 + 8.0 / 3) * 16.0 * N * N * S_CH * S / (a.hbm_gbs * 1e9) * 1e6
        cfg.update({"launch_us": [round(float(v), 2) for v in np.median(dur, axis=0)], "kernels_sum_us": round(float(sums.min()), 2),
                    "kernels_sum_median_us": round(float(np.median(sums)), 2), "span_us": round(float(span.min()), 2),
                    "span_median_us": round(float(np.median(span)), 2), "calls_traced": int(len(dur)), "floor_us": round(floor_us, 2),
                    "times_floor": round(float(sums.min()) / floor_us, 2)})
        admm = child(["--step", "admm", str(S)])
        if admm is None:
            print(json.dumps({"failed_step": f"admm slices={S}", **out}))
            return 1
        cfg.update({"admm_wav_ms_per_iter": admm["ms_per_iter"], "admm_wav_stage_ms_per_iter": admm["stage_ms_per_iter"]})
        out["configs"].append(cfg)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
