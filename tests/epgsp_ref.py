"""numpy restatement of the slice-profile-aware FISP simulation (include/qmri.h qmri_dict_simulate_sp) on top of
epg_ref.epg_fisp: what the GPU tests compare against -- never the device's own output.

F[k, t] = sum_q w_q f_q[k, t], the sum starting from 0 and running in ascending q, where f_q is the plain simulation whose RF argument in frame t
is a = (alpha_t b1_k) prof[t, q], in that product order.  epg_fisp forms alpha_t * b1_k itself, so it is called once per sub-slice and per distinct
b1 value with the flip angles (alpha_t b1) prof[t, q] and b1 = None (a product with exactly 1)."""
import numpy as np

import epg_ref as R


def profile_2d(prof, T):
    """prof [Q] (the same in every frame) or [T, Q] as [T, Q] float64."""
    prof = np.asarray(prof, dtype=np.float64)
    return np.broadcast_to(prof, (T, prof.shape[-1])) if prof.ndim == 1 else prof


def epg_fisp_sp(alpha, tr, te, t1, t2, b1=None, prof=(1.0,), w=None, nstates=32, inversion=True, ti=0.0, inv_eff=1.0, dtype=np.float64, exp=None,
                arg=0):
    """F [K, T] in `dtype`.  prof [Q] or [T, Q]; w [Q] (None: 1 / Q), not normalised.  exp: as in epg_fisp.  arg: +1 / -1 moves every RF argument
    (alpha_t b1) prof[t, q] to its fp64 neighbour above / below (the sensitivity hook for the product order)."""
    alpha = np.asarray(alpha, dtype=np.float64).ravel()
    t1, t2 = np.asarray(t1, dtype=np.float64).ravel(), np.asarray(t2, dtype=np.float64).ravel()
    K, T = t1.size, alpha.size
    prof = profile_2d(prof, T)
    Q = prof.shape[1]
    w = np.full(Q, 1.0 / Q) if w is None else np.asarray(w, dtype=np.float64).ravel()
    b1 = np.ones(K) if b1 is None else np.asarray(b1, dtype=np.float64).ravel()
    F = np.zeros((K, T), dtype)
    for q in range(Q):
        f = np.empty((K, T), dtype)
        for b in np.unique(b1):
            sel = b1 == b
            a = (alpha * b) * prof[:, q]
            if arg:
                a = np.nextafter(a, np.inf * arg)
            f[sel] = R.epg_fisp(a, tr, te, t1[sel], t2[sel], None, nstates=nstates, inversion=inversion, ti=ti, inv_eff=inv_eff, dtype=dtype, exp=exp)
        F = F + dtype(w[q]) * f
    return F


def sinc_envelope(P=32, tbw=4.0):
    """A Hamming-windowed sinc of time-bandwidth product tbw on P sub-pulses."""
    x = (np.arange(P) + 0.5) / P - 0.5
    return np.sinc(tbw * x) * (0.54 + 0.46 * np.cos(2 * np.pi * x))


TBW = 4.0


def rf_profile(T, Q):
    """(prof [T, Q], w [Q]) of the fixtures' pulse on the fixtures' flip-angle train."""
    from qmri_pnp_recon_poc_amd import synth
    return synth.rf_slice_profile(synth.flip_angle_train(T), sinc_envelope(), TBW, Q)


P4 = (1.0, 0.9, 0.6, 0.25)       # the frame-constant 4-point profile of the host tests and of the per_frame = 0 GPU test

# The GPU fixtures: name -> the keywords of epg_ref.CASES plus Q, and `profile`: "rf" (per frame, from synth.rf_slice_profile; the default),
# "p4" (frame-constant P4), "one" (Q = 1, w = 1, prof = 1); `w`: explicit weights.  K = 45 (9 x 5), T = 48, S = 32 unless given.
CASES = {("s%d" % S): dict(T=48, grid=(9, 5), nstates=S, Q=5) for S in (1, 16, 17, 33, 65, 129, 256)}
CASES.update({("q%d" % Q): dict(T=48, grid=(9, 5), Q=Q) for Q in (1, 2, 5, 16, 17, 33, 64)})
CASES.update({
    "k1": dict(T=1, grid=(1, 1), Q=1),
    "t17": dict(T=17, grid=(3, 1), Q=5),
    "q64s256": dict(T=48, grid=(2, 1), Q=64, nstates=256),
    "timing": dict(T=48, grid=(9, 5), Q=5, timing="varying"),
    "noinv": dict(T=48, grid=(9, 5), Q=5, inversion=False),
    "inveff": dict(T=48, grid=(9, 5), Q=5, inv_eff=0.9, ti=0.020),
    "b1": dict(T=48, grid=(9, 5), Q=5, b1="ramp"),
    "wzero": dict(T=48, grid=(9, 5), Q=5, w=(0.25, 0.25, 0.0, 0.25, 0.25)),
    "p4": dict(T=48, grid=(9, 5), Q=4, profile="p4"),
    "p4b1": dict(T=48, grid=(9, 5), Q=4, profile="p4", b1="ramp"),
    "one": dict(T=48, grid=(9, 5), Q=1, profile="one"),
})
CHAIN = dict(T=48, grid=(24, 11), Q=5, b1_grid=(0.8, 1.0, 1.2), s=6)

# name -> (|fp64 - longdouble|_max, |fp64 - every exponential one ulp away|_max, |fp64 - every RF argument one ulp away|_max; the last two the
# larger of the two directions): the figures tests/test_epgsp_host.py measures on the restatement, rounded up with a factor 2 of room and asserted
# there from above and, at a quarter, from below.  The GPU tolerance is 16 x the largest: room for a 2-ulp device exp / sincos and for fused
# multiply-adds, which numpy does not form.  (DESIGN.md section 26 holds the table.)
SENS = {
    "s1": (6.4e-16, 2.7e-15, 1.7e-16), "s17": (1.7e-15, 6.8e-15, 3.4e-16), "q1": (2.1e-15, 8.2e-15, 3.9e-16), "q2": (1.8e-15, 6.9e-15, 3.4e-16),
    "q33": (1.8e-15, 6.8e-15, 1.7e-16), "k1": (6e-18, 4.2e-17, 1.4e-17), "t17": (3e-16, 1.9e-15, 8.4e-17), "q64s256": (2.4e-16, 2.3e-15, 8.4e-17),
    "timing": (4.9e-16, 6.8e-15, 2.8e-16), "noinv": (4.4e-16, 6.6e-16, 2.8e-16), "inveff": (1.7e-15, 6.3e-15, 2.5e-16),
    "b1": (1.9e-15, 7.4e-15, 2.8e-16), "wzero": (1.6e-15, 6.5e-15, 2.3e-16), "p4": (2.5e-15, 9.4e-15, 3.4e-16), "p4b1": (2.7e-15, 1.1e-14, 3.4e-16),
    "one": (3e-15, 1.3e-14, 5.6e-16), "chain": (2.1e-15, 7.4e-15, 3.4e-16),
}
SENS.update({n: (1.8e-15, 6.8e-15, 2.3e-16) for n in ("s16", "s33", "s65", "s129", "s256", "q5", "q16", "q17", "q64")})


def atol(name):
    """Absolute tolerance on F of the GPU tests for a fixture of CASES (or "chain")."""
    return 16.0 * max(SENS[name])


def case_inputs(name):
    """The keyword arguments of epg_fisp_sp for a fixture, float64."""
    from qmri_pnp_recon_poc_amd import synth
    c = CHAIN if name == "chain" else CASES[name]
    T, Q = c["T"], c["Q"]
    t1, t2 = R.grid(*c["grid"])
    tr, te = R._timing_varying(T) if c.get("timing") == "varying" else (np.full(T, R.TR0), np.full(T, R.TE0))
    b1 = np.linspace(0.8, 1.2, t1.size) if c.get("b1") == "ramp" else None
    if "b1_grid" in c:
        bg = np.asarray(c["b1_grid"], dtype=np.float64)
        n = t1.size
        t1, t2, b1 = np.tile(t1, bg.size), np.tile(t2, bg.size), np.repeat(bg, n)
    kind = c.get("profile", "rf")
    if kind == "rf":
        prof, w = rf_profile(T, Q)
    elif kind == "p4":
        prof, w = np.array(P4), np.full(4, 0.25)
    else:
        prof, w = np.ones(1), np.ones(1)
    if "w" in c:
        w = np.array(c["w"], dtype=np.float64)
    return dict(alpha=synth.flip_angle_train(T), tr=tr, te=te, t1=t1, t2=t2, b1=b1, prof=prof, w=w, nstates=c.get("nstates", 32),
                inversion=c.get("inversion", True), ti=c.get("ti", 0.0), inv_eff=c.get("inv_eff", 1.0))


def engine_kwargs(inp, **more):
    """The fixture as Engine.simulate_dictionary takes it."""
    kw = {k: v for k, v in inp.items() if k not in ("prof", "w")}
    kw.update(slice_profile=inp["prof"], slice_weights=inp["w"], **more)
    return kw


_refs = {}


def case_ref(name):
    """The float64 reference of a fixture, computed once and left unchanged."""
    if name not in _refs:
        F = epg_fisp_sp(**case_inputs(name))
        F.setflags(write=False)
        _refs[name] = F
    return _refs[name]


def measure(name):
    """(fp64 against longdouble, exponentials one ulp away, RF arguments one ulp away) of a fixture: what SENS records."""
    inp, F = case_inputs(name), case_ref(name)
    ld = float(np.max(np.abs(F - epg_fisp_sp(**inp, dtype=np.longdouble))))
    ex = max(float(np.max(np.abs(F - epg_fisp_sp(**inp, exp=R.exp_neighbour(d))))) for d in (+1, -1))
    ar = max(float(np.max(np.abs(F - epg_fisp_sp(**inp, arg=d)))) for d in (+1, -1))
    return ld, ex, ar
