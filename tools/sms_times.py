"""Simultaneous multi-slice groups on one MI355X: one group of Z = 2 and Z = 3 slices at 224 x 224 x 10, gridded spiral
(S = 771, T = 200), 8 coils, max_batch 4, beside the yardstick -- the multi-coil solver on Z unaliased slices with Z times the data -- on the same
box in the same run, the two alternated call by call.

Prints one JSON line and the table of section 31, and writes both to profiles/sms_times.json (or --out); per Z:
  lsqr_ms_per_iter           the joint LSQR alone: xupdate_sms with tol = 0 run for LSQR_IT iterations minus the same call with maxit = 0 (copies and the
                             initial step cancel), over LSQR_IT; best of 4 alternations.  mc_lsqr_ms_per_iter: xupdate_mc_batch of Z slices, the same way
  admm_ms_per_iter           pnp_admm_sms with the LLR step (block 8, shifted), wall clock of a call of ADMM_ITERS iterations over ADMM_ITERS, best of 3;
                             mc_admm_ms_per_iter: pnp_admm_mc_batch of Z slices per launch, the same way
  kernel_us_per_iter         from a kernel trace (rocprofv3 --kernel-trace) of LSQR calls in a run of its own: the summed duration of every kernel of
                             one iteration, by kernel name; new_kernel_share: k_sms_combine + k_sms_expand + k_sms_coil_mul + k_sms_scalar over all of them
Every step runs as a child process of its own under `timeout -k 10 <seconds>`; the first one that fails or runs out of time ends the run, and
nothing more is started on the GPU.

    python tools/sms_times.py
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, S_CH, T, SPIRAL, NC, MAXB = 224, 10, 200, 771, 8, 4
ZS = (2, 3)
LSQR_IT, ADMM_ITERS = 16, 3
TRACE_CALLS = 3
STEP_LIMIT_S = 170
NEW = ("k_sms_combine", "k_sms_expand", "k_sms_coil_mul", "k_sms_scalar")


def maps_for(nc, phase):
    hh, ww = np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, N), indexing="ij")
    m = np.stack([np.exp(-((hh - np.cos(a)) ** 2 + (ww - np.sin(a)) ** 2)) * np.exp(1j * (a + hh * ww))
                  for a in phase + np.linspace(0, 2 * np.pi, nc, endpoint=False)], axis=2)
    return m / np.sqrt(np.sum(np.abs(m) ** 2, axis=2, keepdims=True))


def setup(Z):
    from qmri_pnp_recon_poc_amd import engine as E, synth
    dic = synth.make_dictionary(T=T, n_t1=32, n_t2=16, s=S_CH)
    fp, k = E.build_spiral(N, SPIRAL, T)
    e = E.Engine(0)
    e.set_operator(N, N, dic["V"], fp, k, max_batch=MAXB)
    e.set_sms(E.caipi_phases(T, Z))
    rng = np.random.default_rng(Z)
    a, b = np.meshgrid(np.arange(N) / N, np.arange(N) / N, indexing="ij")
    base = np.stack([np.exp(-((a - 0.4) ** 2 + (b - 0.55) ** 2) * 8.0) * 0.5 ** c for c in range(S_CH)], axis=2)
    x = np.stack([base * (1.0 + 0.2 * z) + 1e-3 * rng.standard_normal(base.shape) for z in range(Z)])[None] + 0j
    maps = np.stack([maps_for(NC, 0.3 * z) for z in range(Z)])[None]
    y = e.forward_sms(maps, x)
    ymc = []                                                            # the yardstick's data: every slice measured on its own
    for z in range(Z):
        e.set_coils(maps[0, z])
        ymc.append(e.forward_mc(x[0, z]))
    return e, maps, y, np.stack(ymc), x


def step_lsqr(Z):
    e, maps, y, ymc, x = setup(Z)
    zs = np.zeros_like(x)
    t_sms, t_mc = {0: 1e9, LSQR_IT: 1e9}, {0: 1e9, LSQR_IT: 1e9}
    for it in (0, LSQR_IT) * 4:                                          # best of 4, the two solvers alternated (the first round warms up)
        t0 = time.perf_counter()
        _, n_s, _ = e.xupdate_sms(maps, y, zs, 0.05, tol=0.0, maxit=it)
        t_sms[it] = min(t_sms[it], time.perf_counter() - t0)
        t0 = time.perf_counter()
        _, n_m, _ = e.xupdate_mc_batch(maps[0], ymc, zs[0], 0.05, tol=0.0, maxit=it)
        t_mc[it] = min(t_mc[it], time.perf_counter() - t0)
    assert np.all(n_s == LSQR_IT) and np.all(n_m == LSQR_IT), (n_s, n_m)
    e.close()
    return {"Z": Z, "lsqr_ms_per_iter": round((t_sms[LSQR_IT] - t_sms[0]) * 1e3 / LSQR_IT, 4),
            "mc_lsqr_ms_per_iter": round((t_mc[LSQR_IT] - t_mc[0]) * 1e3 / LSQR_IT, 4)}


def step_admm(Z):
    e, maps, y, ymc, _ = setup(Z)
    e.set_llr(0.02, block=8, shift=True)
    d_sms = d_mc = 1e9
    for k in range(4):                                                   # the first round warms up; best of 3, alternated
        t0 = time.perf_counter()
        _, li = e.pnp_admm_sms(maps, y, groups_per_launch=1, iters=ADMM_ITERS, tsmi_domain="complex")
        t1 = time.perf_counter()
        _, lm = e.pnp_admm_mc_batch(maps[0], ymc, slices_per_launch=Z, iters=ADMM_ITERS, tsmi_domain="complex")
        t2 = time.perf_counter()
        if k:
            d_sms, d_mc = min(d_sms, t1 - t0), min(d_mc, t2 - t1)
    e.close()
    return {"Z": Z, "admm_ms_per_iter": round(d_sms * 1e3 / ADMM_ITERS, 3), "lsqr_iters": li[0].tolist(),
            "mc_admm_ms_per_iter": round(d_mc * 1e3 / ADMM_ITERS, 3), "mc_lsqr_iters_max": np.max(lm, axis=0).tolist()}


def step_trace(Z):
    e, maps, y, _, x = setup(Z)
    for _ in range(TRACE_CALLS):
        e.xupdate_sms(maps, y, np.zeros_like(x), 0.05, tol=0.0, maxit=LSQR_IT)
    e.close()
    return {"Z": Z}


def kernel_sums(trace_dir):
    """Summed duration in microseconds per kernel name over the trace, from the first k_sms_ launch on (the set-up's launches come before it)."""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row.get("Kernel_Name", "")))
    rows.sort()
    first = next((i for i, r in enumerate(rows) if "k_sms_coil_mul" in r[2]), len(rows))
    # (back to the k_mcl_ub launch that opens the first solve)
    while first > 0 and "k_mcl_ub" not in rows[first][2]:
        first -= 1
    sums = {}
    for s, t, name in rows[first:]:
        km = re.search(r"\b(k_\w+)", name)
        if not km:                                                       # (copy and fill kernels of the runtime: not part of an iteration)
            continue
        short = km.group(1)
        sums[short] = sums.get(short, 0.0) + (t - s) / 1e3
    return sums


def child(args, trace_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    if trace_dir:                                                        # (the program itself goes after `--`; a trace and nothing else)
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "--"] + cmd
    r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return None
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def table(out):
    rows = ["| Z | LSQR ms / iteration | multi-coil, Z slices | ratio | ADMM ms / iteration (LLR) | multi-coil, Z slices | new kernels' share of an iteration |",
            "|---|---|---|---|---|---|---|"]
    for c in out["configs"]:
        rows.append(f"| {c['Z']} | {c['lsqr_ms_per_iter']:.3f} | {c['mc_lsqr_ms_per_iter']:.3f} | {c['lsqr_ms_per_iter'] / c['mc_lsqr_ms_per_iter']:.2f} | "
                    f"{c['admm_ms_per_iter']:.2f} | {c['mc_admm_ms_per_iter']:.2f} | {100 * c['new_kernel_share']:.1f} % |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", nargs="+")
    ap.add_argument("--box", default="", help="what to record as the machine the figures were taken on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sms_times.json"))
    a = ap.parse_args()
    if a.step:
        kind, Z = a.step[0], int(a.step[1])
        print(json.dumps({"lsqr": step_lsqr, "admm": step_admm, "trace": step_trace}[kind](Z)))
        return 0
    out = {"workload": "EXTENSION: one simultaneous multi-slice group, gridded spiral, host arrays", "N": N, "s": S_CH, "T": T, "spiral": SPIRAL, "ncoil": NC,
           "max_batch": MAXB, "lsqr_it": LSQR_IT, "admm_iters": ADMM_ITERS, "box": a.box, "date": time.strftime("%Y-%m-%d"), "configs": []}
    for Z in ZS:
        cfg = child(["--step", "lsqr", str(Z)])
        if cfg is None:
            print(json.dumps({"failed_step": f"lsqr Z={Z}", **out}))
            return 1
        admm = child(["--step", "admm", str(Z)])
        if admm is None:
            print(json.dumps({"failed_step": f"admm Z={Z}", **out}))
            return 1
        cfg.update(admm)
        with tempfile.TemporaryDirectory() as td:                        # the kernel trace: a run of its own
            if child(["--step", "trace", str(Z)], trace_dir=td) is None:
                print(json.dumps({"failed_step": f"trace Z={Z}", **out}))
                return 1
            sums = kernel_sums(td)
        total = sum(sums.values())
        if not total or not any(k in sums for k in NEW):
            print(json.dumps({"failed_step": f"trace Z={Z}: no k_sms_ launches traced", **out}))
            return 1
        per_iter = TRACE_CALLS * (LSQR_IT + 1)                          # (the initial step counted as one iteration: it runs both transforms once)
        cfg["kernel_us_per_iter"] = {k: round(v / per_iter, 2) for k, v in sorted(sums.items(), key=lambda kv: -kv[1])}
        cfg["new_kernel_share"] = round(sum(v for k, v in sums.items() if k in NEW) / total, 4)
        out["configs"].append(cfg)
    out["table_md"] = table(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))
    print(out["table_md"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
