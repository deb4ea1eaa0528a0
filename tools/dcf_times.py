"""Density compensation on one MI355X: what the set-up costs and what the weighted adjoint costs beside the plain one.

Workload: 224^2, s = 10, the exact spiral with S = 800 points per frame, T = 200 and T = 1000 frames (m = 160 000 / 800 000), kernel width 12.
Prints one JSON line and writes it to profiles/dcf_times.json; per T:
  setup_ms                   qmri_nufft_dcf, 20 iterations (the default), weights left on the device
  adjoint_ms / adjoint_w_ms  qmri_adjoint_dev / qmri_adjoint_w_dev, one slice on device arrays
Every figure is the median of 20 calls after 3 warm-ups, timed by a pair of events on the stream the library launches on.  Every (T, step) -- set-up, adjoint, weighted adjoint -- runs as
a child process of its own under `timeout -k 10 <seconds>`; the first one that fails or runs out of time ends the run, and nothing more is
started on the GPU.

    python tools/dcf_times.py
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, S_INT, s, WIDTH = 224, 800, 10, 12
FRAMES = (200, 1000)
WARMUP, REPS = 3, 20
STEP_LIMIT_S = {"setup": 240, "adjoint": 180, "adjoint_w": 180}


def median_ms(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return round(float(np.median(times)), 4)


def step(name, T):
    import torch
    from qmri_pnp_recon_poc_amd import engine as E
    V = np.linalg.qr(np.random.default_rng(0).standard_normal((T, s)))[0]
    fp, om = E.build_spiral_traj(N, S_INT, T)
    e = E.Engine(0)
    e.set_trajectory(N, N, V, fp, om, width=WIDTH)
    e.set_stream(torch.cuda.current_stream().cuda_stream)             # the events below bracket the library's launches
    out = {"m": int(fp[-1])}
    if name == "setup":
        out["setup_ms"] = median_ms(lambda: e._check(e.L.qmri_nufft_dcf(e.h, None, None, None)))
        w, info = e.density_weights()
        out.update({"niter": info["iters"], "dev": info["dev"], "weight_max_over_min": float(w.max() / w.min())})
    else:
        e.density_weights()
        rng = np.random.default_rng(1)
        y = torch.from_numpy(rng.standard_normal(e.m) + 1j * rng.standard_normal(e.m)).cuda()
        x = torch.zeros(N * N * s, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        vp = lambda t: C.c_void_p(t.data_ptr())
        call = e.L.qmri_adjoint_w_dev if name == "adjoint_w" else e.L.qmri_adjoint_dev
        out[name + "_ms"] = median_ms(lambda: e._check(call(e.h, vp(y), vp(x), 1)))
    e.set_stream(None)
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S))
    ap.add_argument("--frames", type=int, default=FRAMES[0])
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step, a.frames)))
        return 0
    out = {"N": N, "s": s, "S": S_INT, "width": WIDTH, "warmup": WARMUP, "reps": REPS}
    for T in FRAMES:
        for name in ("setup", "adjoint", "adjoint_w"):                            # each under its own time limit; nothing is started after a failure
            cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[name]), sys.executable, os.path.abspath(__file__), "--step", name, "--frames", str(T)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                print(json.dumps({"failed_step": f"{name} T={T}", "returncode": r.returncode, **out}))
                return 1
            out.setdefault(f"T{T}", {}).update(json.loads(r.stdout.strip().splitlines()[-1]))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    json.dump(out, open(os.path.join(ROOT, "profiles", "dcf_times.json"), "w"), indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
