"""The locally low-rank proximal step on one MI355X, at 224 x 224 x 10 with block side 8, for one slice and for 30 slices.

Prints one JSON line and writes it to profiles/llr_times.json (or --out); per slice count:
  prox_host_ms     qmri_llr_prox_dev on device arrays without sigma_max (launch + wait), host clock, best of 20 after 3 warm-ups
  prox_kernel_us   k_llr_prox alone from a kernel trace (rocprofv3 --kernel-trace) of the same 23 calls in a run of its own: best and median
  dual_kernel_us   k_llr_dual (Step 3) from the kernel trace of the ADMM run below
  floor_us         one read and one write of 16 N M s bytes per slice at the HBM rate in --hbm-gbs (default 6300: the achievable streaming rate of the part, 8000 being its
                   specification); times_floor = best kernel time / floor
  admm_llr_ms_per_iter / admm_net_ms_per_iter
                   one ADMM iteration (qmri_pnp_admm_dev's wall clock / iterations, best of 3 calls of 10 iterations) with the LLR step and with the
                   default UNetRes on random weights, same operator (gridded spiral, S = 771, T = 200), same box; the stage split of the LLR loop
Every step runs as a child process of its own under `timeout -k 10 <seconds>`; the first one that fails or runs out of time ends the run, and
nothing more is started on the GPU.

    python tools/llr_times.py
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
N, S_CH, BLOCK, TAU = 224, 10, 8, 0.05
SLICES = (1, 30)
WARMUP, REPS = 3, 20
ADMM_ITERS, ADMM_CALLS = 10, 3
STEP_LIMIT_S = 240


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
    times = []
    for k in range(WARMUP + REPS):
        t0 = time.perf_counter()
        e.llr_prox_dev(d_x.value, (N, N, S_CH, S), TAU, d_o.value, block=BLOCK, offset=(k % BLOCK, (3 * k) % BLOCK), want_sigma_max=False)
        times.append(1e3 * (time.perf_counter() - t0))
    hip.hipFree(d_x)
    hip.hipFree(d_o)
    e.close()
    return {"slices": S, "prox_host_ms": round(min(times[WARMUP:]), 4), "prox_host_median_ms": round(float(np.median(times[WARMUP:])), 4)}


def step_admm(S, which):
    from qmri_pnp_recon_poc_amd import engine as E, synth
    dic = synth.make_dictionary(T=200, n_t1=32, n_t2=16, s=S_CH)
    fp, k = E.build_spiral(N, 771, 200)
    e = E.Engine(0)
    e.set_operator(N, N, dic["V"], fp, k, max_batch=S)
    if which == "net":
        e.set_denoiser(synth.random_weights(in_nc=S_CH, out_nc=S_CH), N, N, in_nc=S_CH, out_nc=S_CH, max_batch=S)
    else:
        e.set_llr(TAU, block=BLOCK, shift=True)
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
    return {"slices": S, "which": which, "ms_per_iter": round(min(walls) / ADMM_ITERS, 4),
            "stage_ms_per_iter": {k_: round(v / ADMM_ITERS, 4) for k_, v in st.items()}}


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
    ap.add_argument("--step", nargs="+")
    ap.add_argument("--hbm-gbs", type=float, default=6300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "llr_times.json"))
    a = ap.parse_args()
    if a.step:
        kind, S = a.step[0], int(a.step[1])
        print(json.dumps(step_prox(S) if kind == "prox" else step_admm(S, a.step[2])))
        return 0
    out = {"N": N, "s": S_CH, "block": BLOCK, "tau": TAU, "warmup": WARMUP, "reps": REPS, "admm_iters": ADMM_ITERS, "hbm_gbs": a.hbm_gbs, "configs": []}
    for S in SLICES:
        cfg = child(["--step", "prox", str(S)])
        if cfg is None:
            print(json.dumps({"failed_step": f"prox slices={S}", **out}))
            return 1
        with tempfile.TemporaryDirectory() as td:                      # the kernel trace: a run of its own
            if child(["--step", "prox", str(S)], trace_dir=td) is None:
                print(json.dumps({"failed_step": f"prox trace slices={S}", **out}))
                return 1
            ks = kernel_times(td, "k_llr_prox")[WARMUP:]
        floor_us = 2 * 16.0 * N * N * S_CH * S / (a.hbm_gbs * 1e9) * 1e6
        cfg.update({"prox_kernel_us": round(min(ks), 2), "prox_kernel_median_us": round(float(np.median(ks)), 2), "launches_traced": len(ks),
                    "floor_us": round(floor_us, 2), "times_floor": round(min(ks) / floor_us, 2)})
        with tempfile.TemporaryDirectory() as td:
            llr = child(["--step", "admm", str(S), "llr"], trace_dir=td)
            if llr is None:
                print(json.dumps({"failed_step": f"admm llr slices={S}", **out}))
                return 1
            kd, kp = kernel_times(td, "k_llr_dual"), kernel_times(td, "k_llr_prox")
        llr = child(["--step", "admm", str(S), "llr"])                 # (timed without the tracer)
        net = child(["--step", "admm", str(S), "net"]) if llr is not None else None
        if llr is None or net is None:
            print(json.dumps({"failed_step": f"admm slices={S}", **out}))
            return 1
        cfg.update({"dual_kernel_us": round(float(np.median(kd)), 2), "prox_kernel_in_loop_us": round(float(np.median(kp)), 2),
                    "admm_llr_ms_per_iter": llr["ms_per_iter"], "admm_llr_stage_ms_per_iter": llr["stage_ms_per_iter"],
                    "admm_net_ms_per_iter": net["ms_per_iter"], "admm_net_stage_ms_per_iter": net["stage_ms_per_iter"]})
        out["configs"].append(cfg)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
