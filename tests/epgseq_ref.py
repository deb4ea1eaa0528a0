"""numpy restatement of the EPG simulation of prepared, repeated FISP trains (include/qmri.h qmri_dict_simulate_seq): what
the GPU tests compare against -- never the device's own output.  Vectorised over the atoms, a loop over cycles, blocks and frames; the frame is
that of tests/epg_ref.py, statement for statement, and the spoiler is epg_ref.shift.

Per atom the state starts at equilibrium (Z_0 = 1).  The block list is played ncycles times; in front of its frames a block waits (free
relaxation, no dephasing), then plays its preparation (inversion: Z <- -eff Z, relaxation over TI, F+- <- 0; T2 preparation: Z <- eff Z exp(-TE_prep
/ T2), F+- <- 0; neither is scaled by b1).  Only the last cycle is recorded."""
import numpy as np

import epg_ref as R

PREPS = ("none", "inversion", "t2")


def epg_fisp_seq(alpha, tr, te, t1, t2, blocks, ncycles=1, b1=None, nstates=32, dtype=np.float64, exp=None):
    """F [K, T] in `dtype` (np.float64 or np.longdouble).  alpha [T] radians; tr, te scalars or [T], seconds; t1, t2, b1 [K] (b1 None: 1); blocks:
    dicts(nframes, prep, wait, prep_time, prep_eff) as Engine.simulate_dictionary_seq takes them, nframes summing to T.
    exp: replaces np.exp everywhere (the sensitivity hook: every exponential moved to its fp64 neighbour)."""
    ex = np.exp if exp is None else exp
    alpha = np.asarray(alpha, dtype=dtype).ravel()
    T, S = alpha.size, int(nstates)
    tr = np.broadcast_to(np.asarray(tr, dtype=dtype), (T,))
    te = np.broadcast_to(np.asarray(te, dtype=dtype), (T,))
    t1, t2 = np.asarray(t1, dtype=dtype).ravel(), np.asarray(t2, dtype=dtype).ravel()
    K = t1.size
    b1 = np.ones(K, dtype=dtype) if b1 is None else np.asarray(b1, dtype=dtype).ravel()
    assert sum(int(b["nframes"]) for b in blocks) == T and all(b.get("prep", "none") in PREPS for b in blocks)
    one, half = dtype(1), dtype(0.5)
    fp, fm, z = np.zeros((K, S), dtype), np.zeros((K, S), dtype), np.zeros((K, S), dtype)
    z[:, 0] = one
    F = np.empty((K, T), dtype)
    for cycle in range(int(ncycles)):
        t0 = 0
        for b in blocks:
            wait, prep, pt, eff = dtype(b.get("wait", 0.0)), b.get("prep", "none"), dtype(b.get("prep_time", 0.0)), dtype(b.get("prep_eff", 1.0))
            if wait > 0:
                e1, e2 = ex(-wait / t1), ex(-wait / t2)
                fp, fm, z = fp * e2[:, None], fm * e2[:, None], z * e1[:, None]
                z[:, 0] += one - e1
            if prep == "inversion":
                e = ex(-pt / t1)
                z0 = (-eff * z[:, 0]) * e + (one - e)
                z = (-eff * z) * e[:, None]
                z[:, 0] = z0
                fp, fm = np.zeros_like(fp), np.zeros_like(fm)
            elif prep == "t2":
                e2 = ex(-pt / t2)
                z = (eff * z) * e2[:, None]
                fp, fm = np.zeros_like(fp), np.zeros_like(fm)
            for t in range(t0, t0 + int(b["nframes"])):
                a = alpha[t] * b1
                c, s = np.cos(a)[:, None], np.sin(a)[:, None]
                c2, s2 = (one + c) * half, (one - c) * half
                fp, fm, z = c2 * fp - s2 * fm + s * z, -s2 * fp + c2 * fm + s * z, -half * s * (fp + fm) + c * z
                for step, dt in enumerate((te[t], tr[t] - te[t])):
                    e1, e2 = ex(-dt / t1), ex(-dt / t2)
                    fp, fm, z = fp * e2[:, None], fm * e2[:, None], z * e1[:, None]
                    z[:, 0] += one - e1
                    if step == 0:
                        F[:, t] = fp[:, 0]
                fp, fm = R.shift(fp, fm)
            t0 += int(b["nframes"])
    return F


def blk(nframes, prep="none", wait=0.0, prep_time=0.0, prep_eff=1.0):
    return dict(nframes=nframes, prep=prep, wait=wait, prep_time=prep_time, prep_eff=prep_eff)


def degenerate_blocks(inp):
    """The one block that states the experiment of an epg_ref fixture (epg_ref.case_inputs)."""
    T = np.asarray(inp["alpha"]).size
    return [blk(T, "inversion", 0.0, inp["ti"], inp["inv_eff"])] if inp["inversion"] else [blk(T)]


def tiled(alpha, tr, te, blocks, C):
    """The C-fold tiled train and block list: one cycle of it is C cycles of the original."""
    T = np.asarray(alpha).size
    return (np.tile(np.asarray(alpha, dtype=np.float64), C), np.tile(np.broadcast_to(np.asarray(tr, dtype=np.float64), (T,)), C),
            np.tile(np.broadcast_to(np.asarray(te, dtype=np.float64), (T,)), C), list(blocks) * C)


# four blocks whose boundaries 5, 21, 38 fall inside the kernel's 16-frame blocks, one of them exactly 16 long
MIX = [blk(5), blk(16, "inversion", 0.3, 0.021, 0.95), blk(17, "t2", 0.25, 0.040), blk(10, "t2", 0.01, 0.080, 0.9)]
_CYCLE3 = (("inversion", 0.021, 0.95), ("none", 0.0, 1.0), ("t2", 0.040, 1.0))
_CMRF = (("inversion", 0.021, 1.0), ("none", 0.0, 1.0), ("t2", 0.040, 1.0), ("t2", 0.080, 1.0))
CHAIN_RR = (0.92, 1.01, 0.87, 1.10, 0.95, 1.00)


def _blocks(kind):
    if kind == "mix":
        return MIX
    if kind == "b16":                                        # boundaries on multiples of 16
        return [blk(16, "inversion", 0.0, 0.021, 0.95), blk(16, "t2", 0.3, 0.040), blk(16, "none", 0.2)]
    if kind == "ones":                                       # 48 one-frame blocks, the preparations alternating
        return [blk(1, _CYCLE3[i % 3][0], 0.02 * (i % 4), *_CYCLE3[i % 3][1:]) for i in range(48)]
    if kind == "k1":
        return [blk(1, "t2", 0.5, 0.040, 0.9)]
    if kind == "t1024":                                      # 64 heartbeats of 16 frames
        return [blk(16, _CMRF[i % 4][0], 0.0 if i == 0 else 0.6 + 0.01 * (i % 7), *_CMRF[i % 4][1:]) for i in range(64)]
    if kind == "k5000":
        return [blk(13, "inversion", 0.4, 0.021, 0.95), blk(19, "t2", 0.3, 0.040)]
    if kind == "chain":
        from qmri_pnp_recon_poc_amd import synth
        return synth.cmrf_blocks(CHAIN_RR, 8, R.TR0)
    raise KeyError(kind)


# The GPU fixtures: name -> dict(T, grid (n_t1, n_t2), blocks (a kind of _blocks), C, and what differs from nstates = 32, constant TR = 12 ms /
# TE = 2 ms, b1 = None).  alpha = synth.flip_angle_train(T).
CASES = {("s%d" % S): dict(T=48, grid=(9, 5), nstates=S, blocks="mix", C=2) for S in (1, 2, 16, 17, 32, 33, 64, 65, 128, 129, 256)}
CASES.update({
    "b16": dict(T=48, grid=(9, 5), blocks="b16", C=2),
    "ones": dict(T=48, grid=(9, 5), blocks="ones", C=2),
    "k1": dict(T=1, grid=(1, 1), blocks="k1", C=3),
    "t1024": dict(T=1024, grid=(9, 5), blocks="t1024", C=16),
    "k5000": dict(T=32, grid=(100, 50), nstates=16, blocks="k5000", C=2),
    "timing": dict(T=48, grid=(9, 5), timing="varying", blocks="mix", C=2),
    "b1": dict(T=48, grid=(9, 5), b1="ramp", blocks="mix", C=2),
    "chain": dict(T=48, grid=(24, 11), blocks="chain", C=1),
})

# name -> (|fp64 - longdouble|_max, max over the two directions of |fp64 - fp64 with every exponential one ulp away|_max): the figures
# tests/test_epgseq_host.py measures on the restatement, rounded up with a factor 2 of room and asserted there.  The GPU tolerance is 16 x the
# larger, epg_ref's rule with epg_ref's reasons: a 2-ulp device exp / sincos and fused multiply-adds, which numpy does not form.  (DESIGN.md
# section 33 holds the table.)
SENS = {
    "s1": (5.7e-16, 1.7e-15), "s2": (9.7e-16, 4e-15), "b16": (6.9e-16, 3.4e-15), "ones": (2.8e-16, 7.1e-16), "k1": (1.1e-18, 1.4e-18),
    "t1024": (9.9e-16, 4.7e-15), "k5000": (1.1e-15, 2.8e-15), "timing": (5e-16, 4.2e-15), "b1": (8.6e-16, 3.6e-15), "chain": (9.3e-16, 4.4e-15),
}
SENS.update({("s%d" % S): (9.9e-16, 4.3e-15) for S in (16, 17, 32, 33, 64, 65, 128, 129, 256)})


def atol(name):
    """Absolute tolerance on F (|F| <= 1) of the GPU tests for a fixture of CASES."""
    return 16.0 * max(SENS[name])


def case_inputs(name):
    """dict(alpha, tr, te, t1, t2, b1, nstates, blocks, ncycles) of a fixture, float64."""
    from qmri_pnp_recon_poc_amd import synth
    c = CASES[name]
    T = c["T"]
    t1, t2 = R.grid(*c["grid"])
    tr, te = R._timing_varying(T) if c.get("timing") == "varying" else (np.full(T, R.TR0), np.full(T, R.TE0))
    b1 = np.linspace(0.8, 1.2, t1.size) if c.get("b1") == "ramp" else None
    return dict(alpha=synth.flip_angle_train(T), tr=tr, te=te, t1=t1, t2=t2, b1=b1, nstates=c.get("nstates", 32), blocks=_blocks(c["blocks"]),
                ncycles=c["C"])


_refs = {}


def case_ref(name):
    """The float64 reference of a fixture, computed once and left unchanged."""
    if name not in _refs:
        F = epg_fisp_seq(**case_inputs(name))
        F.setflags(write=False)
        _refs[name] = F
    return _refs[name]
