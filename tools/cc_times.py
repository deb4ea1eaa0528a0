"""Coil compression (extension, no reference counterpart): its cost per slice, and what it saves in the multi-coil PnP-ADMM.

Workload: 224^2 spiral (771 interleaves x T = 200 frames, m = 123 604 samples per coil), s = 10, 32 smooth coils, one slice per launch.
Run mode (GPU) prints one JSON line:
  cc_ms_per_slice               host wall time of qmri_coil_compress_dev on device arrays, 32 -> 8 coils (best of 5; ends synchronised; one host
                                eigensolve of 32 x 32 included)
  admm_ms_per_iter_per_slice    pnp_admm_mc_batch wall time over its ADMM iterations (tools/mc_batch_times.py's method), at 32 coils uncompressed and
                                on the stack compressed to 8, with the LSQR iteration counts of both
Trace mode (CPU) reads the kernel trace of a run-mode call under `rocprofv3 --kernel-trace` and prints, per k_cc_* kernel, calls and mean
microseconds, the compression's kernel time per slice, and the covariance pass's bandwidth: its ALGORITHMIC bytes (m x ncoil x 16, each sample
read once) over its kernel time, against 8 TB/s.

    python tools/cc_times.py [--iters 3]
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/cc_times.py --iters 1 --skip-admm
    python tools/cc_times.py --trace OUT/.../kernel_trace.csv [--m 123604]   (m: the run's m_per_coil)
"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, T, S_INT, s, NC, NV = 224, 200, 771, 10, 32, 8


def maps_for(N, nc, phase):
    hh, ww = np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, N), indexing="ij")
    m = np.stack([np.exp(-((hh - np.cos(a)) ** 2 + (ww - np.sin(a)) ** 2)) * np.exp(1j * (a + hh * ww))
                  for a in phase + np.linspace(0, 2 * np.pi, nc, endpoint=False)], axis=2)
    return m / np.sqrt(np.sum(np.abs(m) ** 2, axis=2, keepdims=True))


def parse_trace(path, m):
    rows = list(csv.DictReader(open(path)))
    per = {}
    for r in rows:
        name = r.get("Kernel_Name", "")
        if "k_cc_" not in name:
            continue
        short = re.search(r"k_cc_[a-z_]+", name).group(0)
        d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
        per.setdefault(short, []).append(d)
    calls = len(per.get("k_cc_cov_reduce", [])) or 1
    out = {"m_per_coil": m, "kernels": {k: {"calls": len(v), "mean_us": round(float(np.mean(v)), 2)} for k, v in sorted(per.items())},
           "cc_kernel_us_per_slice": round(sum(sum(v) for v in per.values()) / calls, 2)}
    if "k_cc_cov_part" in per:
        us = float(np.mean(per["k_cc_cov_part"]))
        bytes_ = m * NC * 16
        out["cov_pass"] = {"bytes": bytes_, "us": round(us, 2), "TBps": round(bytes_ / (us * 1e-6) / 1e12, 3),
                           "fraction_of_8TBs": round(bytes_ / (us * 1e-6) / 8e12, 4)}
    if "k_cc_proj" in per:
        # the projection runs twice per call: samples (m x (NC + NV) x 16 bytes) and maps (N^2 x (NC + NV) x 16)
        out["proj_bytes_per_call"] = (m + N * N) * (NC + NV) * 16
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--skip-admm", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--m", type=int, default=123604)
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(parse_trace(args.trace, args.m), separators=(",", ":")))
        return
    from qmri_pnp_recon_poc_amd import engine as E, synth
    from qmri_pnp_recon_poc_amd._lib import CcParams
    from qmri_pnp_recon_poc_amd.engine import _cbuf
    import bench
    dic = bench.cached_dictionary(synth, T, 32, 16, s)
    fp, k = E.build_spiral(N, S_INT, T)
    eng = E.Engine(0)
    eng.set_operator(N, N, dic["V"], fp, k)
    m = eng.m
    maps = maps_for(N, NC, 0.0)[None]
    X0 = synth.synthesize_tsmi(synth.make_phantom_qmaps(N, seed=0), dic)
    eng.set_coils(maps[0])
    ys = np.stack([synth.awgn_measured(col, 30.0, seed=j) for j, col in enumerate(eng.forward_mc(X0).T)], axis=1)[None]
    out = {"workload": "EXTENSION: coil compression 32 -> 8 coils, 224^2 spiral, T = 200, s = 10, one slice", "m_per_coil": int(m),
           "ncoil": NC, "nv": NV, "cov_bytes": int(m * NC * 16)}
    # the device entry point on device arrays (buffers from the HIP runtime libqmri itself uses)
    path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
    hip = C.CDLL(path)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    hy, hm = _cbuf(ys[0]), _cbuf(maps[0])
    bufs = {n_: C.c_void_p() for n_ in ("y", "m", "yo", "mo")}
    for n_, nb in (("y", hy.nbytes), ("m", hm.nbytes), ("yo", hy.nbytes), ("mo", hm.nbytes)):
        assert hip.hipMalloc(C.byref(bufs[n_]), nb) == 0
    assert hip.hipMemcpy(bufs["y"], hy.ctypes.data_as(C.c_void_p), hy.nbytes, 1) == 0
    assert hip.hipMemcpy(bufs["m"], hm.ctypes.data_as(C.c_void_p), hm.nbytes, 1) == 0
    p = CcParams(NV, 0.99, 0)
    got = C.c_int(0)
    best = 1e9
    for _ in range(6):                                                         # the first call warms up (buffers, code objects)
        t0 = time.perf_counter()
        eng._check(eng.L.qmri_coil_compress_dev(eng.h, 1, NC, bufs["y"], bufs["m"], None, C.byref(p), C.byref(got), bufs["yo"], bufs["mo"], None, None))
        best = min(best, time.perf_counter() - t0)
    out["cc_ms_per_slice"] = round(best * 1e3, 3)
    for v in bufs.values():
        hip.hipFree(v)
    if not args.skip_admm:
        cc = eng.coil_compress(ys, maps, nv=NV)
        out["energy_kept"] = round(float(cc["eig"][0][:NV].sum() / cc["eig"][0].sum()), 6)
        eng.set_denoiser(synth.structured_weights(seed=2, eps=0.02), N, N)
        res = {}
        for label, (mm, yy) in (("uncompressed_32", (maps, ys)), ("compressed_8", (cc["maps"], cc["y"]))):
            eng.pnp_admm_mc_batch(mm, yy, iters=1)                               # warm-up: buffers, plans
            dt, li = 1e9, None
            for _ in range(2):
                t0 = time.perf_counter()
                _, li = eng.pnp_admm_mc_batch(mm, yy, iters=args.iters)
                dt = min(dt, time.perf_counter() - t0)
            res[label] = {"ms_per_admm_iter_per_slice": round(dt * 1e3 / args.iters, 3), "lsqr_iters": li[0].tolist(),
                          "ms_per_lsqr_iter": round(dt * 1e3 / max(int(np.sum(li)), 1), 4)}
        res["speedup_per_admm_iter"] = round(res["uncompressed_32"]["ms_per_admm_iter_per_slice"] / res["compressed_8"]["ms_per_admm_iter_per_slice"], 2)
        out["admm"] = res
    eng.close()
    print(json.dumps(out, separators=(",", ":")))


if __name__ == "__main__":
    main()
