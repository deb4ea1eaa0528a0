"""GPU parity of the TSMI synthesis (synth_kernels.hip: k_nn_lut, k_nn_combine, k_synth_tsmi, k_synth_tsmi_complex) against the oracle's
sequential loop (oracle/orc_lrtv.c), bit for bit: every split of the look-up table the host plan can produce, exact distance ties inside a
tile, across the tiles of a slice and across slices, non-finite inputs, look-up tables of three columns, and every fragment pack dict_atom
reads D from.  No tolerances: indices with np.array_equal, X on its uint32 view (signs of zeros included)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# The host plan of synthesize_impl (qmri_pnp_recon_poc_amd/csrc/synth_kernels.hip), restated: NNT = 256 threads x NN_PPT = 4 pixels per
# workgroup, the table in NN_TILE = 1024-entry LDS tiles, cut into slices of whole tiles over blockIdx.y so that about
# NN_KSPLIT_TARGET = 1024 workgroups exist.  A retuned constant there changes the plans below; the tests assert the plan they were
# chosen for and fail when their coverage is gone.
NN_THREADS, NN_PIX_PER_THREAD, NN_TILE, NN_BLOCK_TARGET = 256, 4, 1024, 1024


def nn_plan(npix, K):
    """(nbx, nslice, kslice, tiles per slice, entries in the last slice) of k_nn_lut's launch for npix pixels and K entries."""
    per_block = NN_THREADS * NN_PIX_PER_THREAD
    nbx = (npix + per_block - 1) // per_block
    nslice = max(1, min(NN_BLOCK_TARGET // max(nbx, 1), (K + NN_TILE - 1) // NN_TILE))
    kslice = (((K + nslice - 1) // nslice) + NN_TILE - 1) // NN_TILE * NN_TILE
    nslice = (K + kslice - 1) // kslice
    return nbx, nslice, kslice, kslice // NN_TILE, K - (nslice - 1) * kslice


def atom_layout(s):
    """The pack qmri_set_dictionary (api_dict.cpp) builds for s channels: 4 or 8 floats per lane up to 16 channels, the wide pack above."""
    if s > 16:
        return "wide"
    return "narrow4" if (s + 1) // 2 <= 4 else "narrow8"


def test_plan_helper_on_the_shapes_the_kernel_comments_state():
    # the reference's size (230 x 230 pixels, K = 98 304): 16 slices of 6 tiles; the shape of tests/test_synthesis.py: two slices of one tile
    assert nn_plan(230 * 230, 98304) == (52, 16, 6144, 6, 6144)
    assert nn_plan(97 * 97, 48 * 40) == (10, 2, 1024, 1, 896)
    assert [atom_layout(s) for s in (1, 8, 9, 16, 17)] == ["narrow4", "narrow4", "narrow8", "narrow8", "wide"]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _assert_same(Xg, ig, Xo, io, what):
    assert ig.dtype == io.dtype and ig.shape == io.shape and Xg.shape == Xo.shape and Xg.dtype == np.float32, what
    assert np.array_equal(ig, io), f"{what}: {int(np.sum(ig != io))} of {ig.size} indices differ"
    nb = int(np.sum(_bits(Xg) != _bits(Xo)))
    assert nb == 0, f"{what}: {nb} of {Xg.size} values differ in their bits"


# ---------------------------------------------------------------------------------------------------------------------------------
# the split of the table, with exact ties
# ---------------------------------------------------------------------------------------------------------------------------------
K_TABLE, S_TABLE, NPIX_BIG = 49189, 6, 255 * 257
N_SAMPLE = 1000


def _first_minimum(q, lut):
    """Plain numpy in fp64 on the pixels q [n, 2]: d = d1*d1 + d2*d2 elementwise (two roundings, as the oracle compiles it), the first
    minimum and all tied entries per pixel."""
    l1, l2 = lut[:, 0].astype(np.float64), lut[:, 1].astype(np.float64)
    first, tied = [], []
    for a, b in q:
        d1, d2 = a - l1, b - l2
        d = d1 * d1 + d2 * d2
        t = np.flatnonzero(d == d.min())
        first.append(int(t[0]))
        tied.append(t)
    return np.array(first), tied


class _Table:
    """K = 49 189 entries of s = 6 channels.  Half of the entries on a dyadic grid (T1 in eighths below 20, T2 in 64ths below 0.75: 7 680
    cells, each hit about three times), half continuous, rows permuted so that duplicates land in different tiles and slices; queries half on
    the twice finer dyadic grid (grid points and exact midpoints), half continuous.  Differences and squares of such dyadic values are exact
    in fp64, so equal distances are equal bits."""

    def __init__(self, oracle):
        rng = np.random.default_rng(20240607)
        K, n = K_TABLE, NPIX_BIG
        kd = K // 2
        lut = np.empty((K, 2), np.float64)
        lut[:kd, 0], lut[:kd, 1] = rng.integers(0, 160, kd) / 8.0, rng.integers(0, 48, kd) / 64.0
        lut[kd:, 0], lut[kd:, 1] = rng.uniform(0, 20, K - kd), rng.uniform(0, 0.75, K - kd)
        self.lut = lut[rng.permutation(K)].astype(np.float32)
        self.D = rng.standard_normal((K, S_TABLE)).astype(np.float32)
        self.normD = rng.uniform(0.5, 1.5, K).astype(np.float32)
        nd = n // 2
        q = np.empty((n, 3), np.complex128)
        q[:nd, 0], q[:nd, 1] = rng.integers(0, 320, nd) / 16.0, rng.integers(0, 96, nd) / 128.0
        q[nd:, 0], q[nd:, 1] = rng.uniform(0, 20, n - nd), rng.uniform(0, 0.75, n - nd)
        q = q[rng.permutation(n)]
        q[:, 2] = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        self.q = q                                                   # complex PD; the real mode is given q.real
        self.sample = np.linspace(0, n - 1, N_SAMPLE).astype(np.int64)
        self.oracle = oracle
        self._ref = {}

    def maps(self, npix, mode, first=0):
        q = self.q[first:first + npix]
        return q if mode == "complex" else np.ascontiguousarray(q.real)

    def reference(self, npix, K, mode, first=0):
        key = (npix, K, mode, first)
        if key not in self._ref:
            X, idx = self.oracle.synthesize_tsmi(self.maps(npix, mode, first), self.D[:K], self.normD[:K], self.lut[:K], mode=mode)
            X.setflags(write=False); idx.setflags(write=False)
            self._ref[key] = (X, idx)
        return self._ref[key]


@pytest.fixture(scope="module")
def table(oracle):
    return _Table(oracle)


@pytest.fixture(scope="module")
def table_ties(table):
    """numpy's first minimum and the tied entries of the fixed 1000-pixel sample at the 65 535-pixel shape."""
    first, tied = _first_minimum(table.q[table.sample, :2].real, table.lut)
    return first, tied


def _run(engine_mod, table, npix, K, mode, first=0):
    e = engine_mod.Engine(0)
    try:
        e.set_dictionary(table.D[:K], table.normD[:K], table.lut[:K])
        return e.synthesize_tsmi(table.maps(npix, mode, first), mode=mode)
    finally:
        e.close()


def test_fixture_has_the_ties_it_is_meant_to_have(table, table_ties):
    """Conditions on the test's own inputs (none of them a measurement of the device): without them the tests below could pass vacuously.
    Measured with this fixture: 276 sample pixels tie across slices, 53 have two tied entries inside one tile, 23 610 distinct winners."""
    nbx, nslice, kslice, tiles, last = nn_plan(NPIX_BIG, K_TABLE)
    first, tied = table_ties
    cross = sum(1 for t in tied if len(t) > 1 and len(np.unique(t // kslice)) > 1)
    in_tile = sum(1 for t in tied if len(t) > 1 and len(np.unique(t // NN_TILE)) < len(t))
    _, io = table.reference(NPIX_BIG, K_TABLE, "real")
    distinct = len(np.unique(io))
    print(f"sample of {N_SAMPLE}: ties across slices {cross}, two tied entries in one tile {in_tile}; distinct winning entries {distinct}")
    assert cross >= 150 and in_tile >= 5
    assert np.array_equal(io[table.sample], first + 1)               # the oracle does not vouch for itself
    assert distinct > 10000


@pytest.mark.parametrize("mode", ["real", "complex"])
def test_thirteen_slices_of_four_tiles_with_a_ragged_last_tile(engine_mod, table, table_ties, mode):
    """65 535 pixels x 49 189 entries: the tile loop of a slice runs four times, the last slice is one tile of 37 entries (fewer than the 256
    threads that fill it), k_nn_combine merges 13 slices, the last workgroup has one idle pixel slot."""
    assert nn_plan(NPIX_BIG, K_TABLE) == (64, 13, 4096, 4, 37)
    assert NPIX_BIG == 64 * NN_THREADS * NN_PIX_PER_THREAD - 1
    Xg, ig = _run(engine_mod, table, NPIX_BIG, K_TABLE, mode)
    Xo, io = table.reference(NPIX_BIG, K_TABLE, mode)
    first, _ = table_ties
    assert np.array_equal(ig[table.sample], first + 1)               # the first of equal distances, as plain numpy finds it
    _assert_same(Xg, ig, Xo, io, f"13 slices x 4 tiles, mode {mode}")
    assert Xg.shape == (NPIX_BIG, S_TABLE if mode == "real" else 2 * S_TABLE)


@pytest.mark.parametrize("mode", ["real", "complex"])
@pytest.mark.parametrize("npix", [1, 1025])
def test_forty_nine_slices_of_one_tile(engine_mod, table, table_ties, npix, mode):
    """Few pixels: every tile is a slice of its own, the widest combine; at 1025 pixels the second workgroup column holds one pixel.  The
    single pixel is one whose tied entries sit in different slices (of this plan too: other 4096-slices are other tiles)."""
    assert nn_plan(npix, K_TABLE) == ((npix + 1023) // 1024, 49, 1024, 1, 37)
    first = 0
    if npix == 1:
        _, tied = table_ties
        first = int(next(table.sample[i] for i, t in enumerate(tied) if len(np.unique(t // 4096)) > 1))
    Xg, ig = _run(engine_mod, table, npix, K_TABLE, mode, first)
    Xo, io = table.reference(npix, K_TABLE, mode, first)
    _assert_same(Xg, ig, Xo, io, f"49 slices, {npix} pixels, mode {mode}")
    if npix == 1025:                                                 # the same pixels as the first 1025 of the large shape: the plan changes nothing
        assert np.array_equal(ig, table.reference(NPIX_BIG, K_TABLE, mode)[1][:1025])


@pytest.mark.parametrize("mode", ["real", "complex"])
@pytest.mark.parametrize("K", [37, 1])
def test_one_slice_of_one_short_tile(engine_mod, table, K, mode):
    """A table below one tile, and below the 256 threads that load a tile."""
    assert nn_plan(1025, K) == (2, 1, 1024, 1, K) and K < NN_THREADS
    Xg, ig = _run(engine_mod, table, 1025, K, mode)
    Xo, io = table.reference(1025, K, mode)
    _assert_same(Xg, ig, Xo, io, f"K = {K}, mode {mode}")
    assert ig.min() >= 1 and ig.max() <= K
    if K == 37:
        assert len(np.unique(ig)) > 20


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs the search must survive
# ---------------------------------------------------------------------------------------------------------------------------------
def test_non_finite_map_values_keep_the_first_entry(engine_mod, oracle, table):
    """NaN or infinite T1 / T2: no distance compares below infinity, in any slice, so the index stays 1 (knnsearch has no such case; the
    oracle's loop defines it)."""
    q = table.maps(1025, "real").copy()
    q[7, 0] = np.nan
    q[300, 1] = np.inf
    q[1024, 0], q[1024, 1] = np.nan, np.inf
    e = engine_mod.Engine(0)
    try:
        e.set_dictionary(table.D, table.normD, table.lut)
        Xg, ig = e.synthesize_tsmi(q)
    finally:
        e.close()
    Xo, io = oracle.synthesize_tsmi(q, table.D, table.normD, table.lut)
    assert ig[7] == 1 and ig[300] == 1 and ig[1024] == 1
    _assert_same(Xg, ig, Xo, io, "non-finite maps")


def test_nan_table_entries_are_never_chosen(engine_mod, oracle, table):
    """NaN in T1 at the first and last entry of tiles and slices (the 49-slice plan of 1025 pixels and the 4096-entry slices alike)."""
    assert nn_plan(1025, K_TABLE)[1:4] == (49, 1024, 1)
    bad = np.array([0, 1023, 1024, 4095, 4096, K_TABLE - 1])
    lut = table.lut.copy()
    lut[bad, 0] = np.nan
    q = table.maps(1025, "real")
    e = engine_mod.Engine(0)
    try:
        e.set_dictionary(table.D, table.normD, lut)
        Xg, ig = e.synthesize_tsmi(q)
    finally:
        e.close()
    Xo, io = oracle.synthesize_tsmi(q, table.D, table.normD, lut)
    assert not np.isin(ig, bad + 1).any()
    _assert_same(Xg, ig, Xo, io, "NaN table entries")


def test_third_table_column_is_ignored(engine_mod, table):
    """Q = 3 (what harness.simulate_dictionary(..., b1_grid=...) produces): the search sees T1 and T2 only."""
    rng = np.random.default_rng(3)
    lut3 = np.concatenate([table.lut, (1e6 * rng.standard_normal((K_TABLE, 1))).astype(np.float32)], axis=1)
    e = engine_mod.Engine(0)
    try:
        e.set_dictionary(table.D, table.normD, lut3)
        assert e.dict_shape == (K_TABLE, S_TABLE, 3)
        for mode in ("real", "complex"):
            Xg, ig = e.synthesize_tsmi(table.maps(1025, mode), mode=mode)
            Xo, io = table.reference(1025, K_TABLE, mode)            # the oracle on the two-column table
            _assert_same(Xg, ig, Xo, io, f"Q = 3, mode {mode}")
    finally:
        e.close()


def test_one_column_table_is_refused(engine_mod, table):
    e = engine_mod.Engine(0)
    try:
        e.set_dictionary(table.D[:37], table.normD[:37], table.lut[:37, :1])
        for mode in ("real", "complex"):
            with pytest.raises(engine_mod.QmriError, match="Q >= 2"):
                e.synthesize_tsmi(table.maps(5, mode), mode=mode)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# every atom layout
# ---------------------------------------------------------------------------------------------------------------------------------
S_LAYOUTS = (1, 2, 7, 8, 9, 15, 16, 17, 24, 40, 129, 1000)


@pytest.mark.parametrize("K", [33, 97, 130, 257])
def test_every_atom_layout(engine_mod, oracle, K):
    """dict_atom (dict_device.h) reads D back from the 4-float pack (s <= 8), the 8-float pack (s <= 16) and the wide pack (s > 16); atom counts
    that fill neither a 32-atom tile nor the wide pack's 128.  About a third of the atoms have a negative first channel, ten have a first channel
    of exactly 0, and each of them is the nearest entry of a pixel placed on its own (T1, T2): the sign alignment with sign(0) = 0
    (main_synthesize_tsmis.m:93-95) is exercised on every pack.  PD holds +-0, negative values and magnitudes over 24 decades."""
    npix = 300
    visited = set()
    e = engine_mod.Engine(0)
    try:
        for s in S_LAYOUTS:
            rng = np.random.default_rng(1000 * K + s)
            D = rng.standard_normal((K, s)).astype(np.float32)
            neg = rng.random(K) < 1.0 / 3.0
            D[:, 0] = np.abs(D[:, 0]) * np.where(neg, -1.0, 1.0).astype(np.float32)
            zero = rng.choice(K, 10, replace=False)
            D[zero, 0] = 0.0
            neg[zero] = False
            assert np.all(D[zero, 1:] != 0) and np.all(D[~np.isin(np.arange(K), zero), 0] != 0)
            normD = rng.uniform(0.5, 1.5, K).astype(np.float32)
            lut = np.stack([rng.uniform(0, 5, K), rng.uniform(0, 0.5, K)], axis=1).astype(np.float32)
            assert len(np.unique(lut, axis=0)) == K
            special = np.concatenate([zero, np.flatnonzero(neg)])
            assert 10 < special.size < npix
            q = np.empty((npix, 3), np.complex128)
            q[:, 0], q[:, 1] = rng.uniform(0, 5, npix), rng.uniform(0, 0.5, npix)
            q[:special.size, :2] = lut[special].astype(np.float64)      # on the atom's own entry: distance 0, and no other entry is there
            mag = 10.0 ** rng.uniform(-12, 12, (npix, 2))
            pd = mag * np.where(rng.random((npix, 2)) < 0.5, -1.0, 1.0)
            pd[rng.choice(npix, 12, replace=False)] = 0.0
            pd[5, 0], pd[6, 1] = -0.0, -0.0
            q[:, 2].real, q[:, 2].imag = pd[:, 0], pd[:, 1]
            q = q[rng.permutation(npix)]
            e.set_dictionary(D, normD, lut)
            visited.add(atom_layout(s))
            qr = np.ascontiguousarray(q.real)
            Xg, ig = e.synthesize_tsmi(qr)
            Xo, io = oracle.synthesize_tsmi(qr, D, normD, lut)
            assert np.isin(special + 1, io).all()                       # every such atom is some pixel's nearest entry
            big = np.abs(Xo[Xo != 0])
            assert np.all(np.isfinite(Xo)) and big.min() >= np.finfo(np.float32).tiny   # all products normal floats
            _assert_same(Xg, ig, Xo, io, f"K = {K}, s = {s}, real")
            assert Xg.shape == (npix, s) and np.all(Xg[:, 0] >= 0)
            on_zero = np.isin(ig - 1, zero)
            assert on_zero.sum() >= 10 and np.all(Xg[on_zero] == 0)      # sign(0) = 0: the whole pixel is zero
            lit = ~on_zero & (qr[:, 2] != 0)
            assert np.all(Xg[lit, 0] > 0)
            if s > 1:
                assert np.all(np.any(Xg[lit, 1:] != 0, axis=1))
            Xg, ig = e.synthesize_tsmi(q, mode="complex")
            Xo, io = oracle.synthesize_tsmi(q, D, normD, lut, mode="complex")
            _assert_same(Xg, ig, Xo, io, f"K = {K}, s = {s}, complex")
            assert Xg.shape == (npix, 2 * s)
            base = D[ig - 1] * normD[ig - 1, None]                      # the 2s-channel stack: real parts, then imaginary parts
            want = np.concatenate([base * q[:, 2].real.astype(np.float32)[:, None], base * q[:, 2].imag.astype(np.float32)[:, None]], axis=1)
            assert np.array_equal(_bits(Xg), _bits(want))
    finally:
        e.close()
    assert visited == {"narrow4", "narrow8", "wide"}


# ---------------------------------------------------------------------------------------------------------------------------------
# ties that exist only while d1*d1 + d2*d2 is left unfused
# ---------------------------------------------------------------------------------------------------------------------------------
def _fused(a, b):
    """fma(a, a, b*b) in fp64, correctly rounded, from exact rational arithmetic."""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(a) + Fraction(b * b))


def test_mirrored_entries_tie_only_without_contraction(engine_mod, oracle):
    """The dyadic ties above are exact whatever the compiler does with d1*d1 + d2*d2.  Here pixel i sits at (c, c) with a full 53-bit c, and
    the table holds (x, y) and its mirror (y, x) at two random places: the differences are exact in fp64, their squares are not, and
    rn(a*a) + rn(b*b) is the same number in both orders, so the two entries tie and the lower index wins.  Under fp contraction the sums
    become fma(a, a, rn(b*b)) and fma(b, b, rn(a*a)), which differ in the last bit for a good share of the pairs, and the later entry would
    win there: synth_kernels.hip is compiled with contraction off for this reason."""
    M = 1500
    K = 2 * M
    assert nn_plan(M, K) == (2, 3, 1024, 1, K - 2048)
    rng = np.random.default_rng(11)
    c = 0.5 + 0.3 * (np.arange(M) + 0.5 * rng.random(M)) / M        # pixels 1e-4 apart or more on the diagonal
    x = (c + rng.uniform(1e-6, 2e-5, M)).astype(np.float32)         # the pair 2e-5 away at the most: nearer than any other pair
    y = (c - rng.uniform(1e-6, 2e-5, M)).astype(np.float32)
    pos = rng.permutation(K)
    pa, pb = pos[:M], pos[M:]
    lut = np.empty((K, 2), np.float32)
    lut[pa, 0], lut[pa, 1] = x, y
    lut[pb, 0], lut[pb, 1] = y, x
    q = np.stack([c, c, rng.standard_normal(M)], axis=1)
    D = rng.standard_normal((K, 3)).astype(np.float32)
    normD = rng.uniform(0.5, 1.5, K).astype(np.float32)
    first, tied = _first_minimum(q[:, :2], lut)
    want = np.minimum(pa, pb)
    assert np.array_equal(first, want) and all(len(t) == 2 for t in tied)         # exact two-way ties, every pixel
    a, b = x.astype(np.float64) - c, y.astype(np.float64) - c
    fab, fba = np.array([_fused(u, v) for u, v in zip(a, b)]), np.array([_fused(v, u) for u, v in zip(a, b)])
    # (x, y) has d1 = -a, d2 = -b: fma(d1, d1, d2*d2) = fab there and fba at the mirror; fma(d2, d2, d1*d1) the other way round
    later_1 = int(np.sum(np.where(pa < pb, fba < fab, fab < fba)))
    later_2 = int(np.sum(np.where(pa < pb, fab < fba, fba < fab)))
    same_tile = int(np.sum(pa // NN_TILE == pb // NN_TILE))
    print(f"mirrored pairs: fused, the later entry would win on {later_1} (fma on d1) or {later_2} (fma on d2) of {M} pixels; pairs inside one tile {same_tile}")
    assert min(later_1, later_2) >= M // 10 and same_tile >= M // 10 and M - same_tile >= M // 10
    Xo, io = oracle.synthesize_tsmi(q, D, normD, lut)
    assert np.array_equal(io, want + 1)
    e = engine_mod.Engine(0)
    try:
        e.set_dictionary(D, normD, lut)
        Xg, ig = e.synthesize_tsmi(q)
    finally:
        e.close()
    _assert_same(Xg, ig, Xo, io, "mirrored pairs")
