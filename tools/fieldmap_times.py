"""Field-map estimate on one MI355X: the fused iteration (halo tiles in LDS, 8 iterations per launch; knob fmap_fuse = 1)
against one launch per iteration (fmap_fuse = 0, the default).

Workload: 224^2, L = 3 echoes at 0, 2, 5 ms, the field 100 (sin 2 pi a cos pi b + 0.6 b + 0.2) Hz, a smooth object with noise of 0.02 max|x|, 200
iterations, beta 0.01; 1 and 8 coils, 1 and 30 slices.  Prints one JSON line and writes it to profiles/fieldmap_times.json (or --out); per
configuration:
  fused_ms / plain_ms   qmri_field_map_estimate_dev on device arrays, the whole call (pairs, scaling, 200 iterations, both costs, the read-back of info;
                        it returns after completion): median wall clock of 10 calls after 2 warm-ups, the two forms alternating call by call
  same_bits             the two forms' maps compared bit for bit
Every configuration runs as a child process of its own under `timeout -k 10 <seconds>`; the first one that fails or runs out of time ends the run,
and nothing more is started on the GPU.

    python tools/fieldmap_times.py
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, T_S, ITERS, BETA = 224, (0.0, 2e-3, 5e-3), 200, 0.01
CONFIGS = ((1, 1), (8, 1), (1, 30), (8, 30))          # (coils, slices)
WARMUP, REPS = 2, 10
STEP_LIMIT_S = 240


def echoes(Cc, S):
    """[S][L][C][n2][n1] complex128: one noisy slice per coil set, the slices scaled copies of it."""
    a, b = np.meshgrid((np.arange(N) - N / 2) / N, (np.arange(N) - N / 2) / N, indexing="ij")
    f = 100.0 * (np.sin(2 * np.pi * a) * np.cos(np.pi * b) + 0.6 * b + 0.2)
    x = 1.0 / (1.0 + np.exp((np.sqrt((a / 0.38) ** 2 + (b / 0.42) ** 2) - 1.0) * 12.0))
    rng = np.random.default_rng(0)
    Y = np.empty((len(T_S), Cc, N, N), np.complex128)
    for c in range(Cc):
        th = 2 * np.pi * c / Cc + 0.3
        coil = np.exp(-((a - 0.45 * np.cos(th)) ** 2 + (b - 0.45 * np.sin(th)) ** 2) / (2 * 0.45 ** 2)) * np.exp(1j * (1.5 * a * np.cos(th) + 0.4 * c))
        for l, t in enumerate(T_S):
            Y[l, c] = x * coil * np.exp(-2j * np.pi * f * t) + 0.02 * (rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N)))
    Yt = np.ascontiguousarray(np.swapaxes(Y, 2, 3))
    return np.stack([Yt * (1.0 + 0.01 * k) for k in range(S)])


def step(Cc, S):
    from qmri_pnp_recon_poc_amd import engine as E
    e = E.Engine(0)
    hip = E._hip_runtime()
    Y = echoes(Cc, S)
    t = np.array(T_S)
    d_Y, d_f = C.c_void_p(), C.c_void_p()
    nf = S * N * N * 8
    assert hip.hipMalloc(C.byref(d_Y), Y.nbytes) == 0 and hip.hipMalloc(C.byref(d_f), nf) == 0
    assert hip.hipMemcpy(d_Y, Y.ctypes.data_as(C.c_void_p), Y.nbytes, 1) == 0
    times, maps = {"fused": [], "plain": []}, {}

    def run(form):
        e._check(e.L.qmri_debug_knob(b"fmap_fuse", 1 if form == "fused" else 0))
        t0 = time.perf_counter()
        e.estimate_field_map_dev(d_Y.value, (S, len(T_S), Cc, N, N), t, d_f.value, iters=ITERS, beta=BETA)
        return 1e3 * (time.perf_counter() - t0)

    for form in ("fused", "plain"):
        for _ in range(WARMUP):
            run(form)
        maps[form] = np.empty(S * N * N)
        assert hip.hipMemcpy(maps[form].ctypes.data_as(C.c_void_p), d_f, nf, 2) == 0
    for _ in range(REPS):
        for form in ("fused", "plain"):
            times[form].append(run(form))
    e._check(e.L.qmri_debug_knob(b"fmap_fuse", 0))
    hip.hipFree(d_Y)
    hip.hipFree(d_f)
    e.close()
    return {"coils": Cc, "slices": S, "fused_ms": round(float(np.median(times["fused"])), 3), "plain_ms": round(float(np.median(times["plain"])), 3),
            "fused_min_ms": round(min(times["fused"]), 3), "plain_min_ms": round(min(times["plain"]), 3),
            "same_bits": bool(np.array_equal(maps["fused"], maps["plain"])), "f_min": float(maps["fused"].min()), "f_max": float(maps["fused"].max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, nargs=2, metavar=("COILS", "SLICES"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fieldmap_times.json"))
    a = ap.parse_args()
    if a.config is not None:
        print(json.dumps(step(*a.config)))
        return 0
    out = {"N": N, "echo_times_s": list(T_S), "iters": ITERS, "beta": BETA, "warmup": WARMUP, "reps": REPS, "configs": []}
    for Cc, S in CONFIGS:                                              # each under its own time limit; nothing is started after a failure
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--config", str(Cc), str(S)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(json.dumps({"failed_step": f"coils={Cc} slices={S}", "returncode": r.returncode, **out}))
            return 1
        out["configs"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
