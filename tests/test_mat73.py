"""MATLAB -v7.3 (HDF5) reader: pinned on a file MATLAB wrote, then exercised on files from tests/h5_writer.py and compared with what
scipy.io reads from the same variables saved as v5 -- the harness must not care which format a data file of the reference is in."""
import os

import numpy as np
import pytest
import scipy.io

from qmri_pnp_recon_poc_amd import harness as H
from qmri_pnp_recon_poc_amd import mat73

from h5_writer import write_mat73

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_file_written_by_matlab():
    """scipy's own test datum testhdf5_7.4_GLNX86.mat (MATLAB 7.4, `testdouble = 0:pi/4:2*pi`), against its v5 twin testdouble_7.4_GLNX86.mat
    (both from scipy's test data, stored under tests/golden/)"""
    path = os.path.join(GOLD, "testhdf5_7.4_GLNX86.mat")
    assert mat73.is_mat73(path)
    with pytest.raises(NotImplementedError):
        scipy.io.loadmat(path)                                   # (what the harness used to surface as "re-save with -v7")
    d = mat73.load_mat73(path, squeeze_me=False)
    assert list(d) == ["testdouble"]
    assert d["testdouble"].shape == (1, 9) and d["testdouble"].dtype == np.float64
    np.testing.assert_array_equal(d["testdouble"][0], np.arange(9) * (np.pi / 4))
    v5 = scipy.io.loadmat(os.path.join(GOLD, "testdouble_7.4_GLNX86.mat"))
    np.testing.assert_array_equal(d["testdouble"], v5["testdouble"])
    assert H.load_mat(path)["testdouble"].shape == (9,)


def _variables(rng):
    X = (rng.standard_normal((23, 17, 10)) + 1j * rng.standard_normal((23, 17, 10))).astype(np.complex64)
    return {
        "X": X,
        "A": rng.standard_normal((5, 7)),
        "v": np.arange(12, dtype=np.int32),
        "u8": rng.integers(0, 255, (3, 4, 5), dtype=np.uint8),
        "flag": np.array([[True, False], [False, True]]),
        "name": "cut3",
        "nothing": np.zeros((0, 3)),
        "dict": {"D": rng.standard_normal((300, 10)).astype(np.float32), "V": rng.standard_normal((40, 10)) + 0j,
                 "lut": rng.random((300, 3)).astype(np.float32), "normD": rng.random(300).astype(np.float32),
                 "meta": {"cut": np.float64(3), "label": "FISP"}},
        "c": [np.float64(1.5), "two", np.arange(3.0)],
    }


def _check(got, want, path="") -> None:
    if isinstance(want, dict):
        assert isinstance(got, mat73.Struct), path
        assert sorted(got._fieldnames) == sorted(want)
        for k in want: _check(getattr(got, k), want[k], path + "." + k)
    elif isinstance(want, str):
        assert got == want, path
    elif isinstance(want, list):
        assert got.dtype == object and got.shape == (1, len(want)), path
        for g, w in zip(got[0], want): _check(g, w, path + "{}")
    else:
        w = np.asarray(want)
        if w.ndim < 2: w = w.reshape(1, -1) if w.ndim == 1 else w.reshape(1, 1)
        assert got.shape == w.shape, (path, got.shape, w.shape)
        assert got.dtype == w.dtype, (path, got.dtype, w.dtype)
        np.testing.assert_array_equal(got, w)


@pytest.mark.parametrize("opts", [dict(), dict(chunk_elems=64, deflate=0, shuffle=False), dict(chunk_elems=16, deflate=6, shuffle=True),
                                  dict(chunk_elems=50, deflate=1, shuffle=False, force_chunked=True)],
                         ids=["contiguous+chunked", "many_chunks_two_level_tree", "tiny_chunks_deflate_shuffle", "everything_chunked"])
def test_round_trip_all_value_kinds(tmp_path, opts):
    rng = np.random.default_rng(7)
    want = _variables(rng)
    p = str(tmp_path / "all.mat")
    write_mat73(p, want, **opts)
    got = mat73.load_mat73(p, squeeze_me=False)
    assert sorted(got) == sorted(want)
    for k in want: _check(got[k], want[k], k)


def test_same_values_as_scipy_reads_from_v5(tmp_path):
    """the same variables saved as v5 (scipy.io.savemat) and as v7.3: load_mat must return the same thing"""
    rng = np.random.default_rng(11)
    X = (rng.standard_normal((30, 20, 4)) + 1j * rng.standard_normal((30, 20, 4))).astype(np.complex64)
    qmap = rng.random((6, 3, 12, 9)).astype(np.float32)
    dic = {"D": rng.standard_normal((64, 10)).astype(np.float32), "V": rng.standard_normal((25, 10)), "lut": rng.random((64, 3)).astype(np.float32),
           "normD": rng.random((64, 1)).astype(np.float32)}
    v5, v73 = str(tmp_path / "v5.mat"), str(tmp_path / "v73.mat")
    scipy.io.savemat(v5, {"X": X, "qmap": qmap, "dict": dic})
    write_mat73(v73, {"X": X, "qmap": qmap, "dict": dic}, chunk_elems=500)
    a, b = H.load_mat(v5), H.load_mat(v73)
    assert sorted(a) == sorted(b)
    for k in ("X", "qmap"):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype
        np.testing.assert_array_equal(a[k], b[k])
    for f in dic:
        x, y = np.asarray(getattr(a["dict"], f)), np.asarray(getattr(b["dict"], f))
        assert x.shape == y.shape and x.dtype == y.dtype, f
        np.testing.assert_array_equal(x, y)
    da, db = H.load_dictionary(v5), H.load_dictionary(v73)
    for f in da: np.testing.assert_array_equal(da[f], db[f])


def test_harness_loaders_on_v73_files(tmp_path):
    """load_tsmi / load_qmaps crop and permute a -v7.3 volume exactly as a v5 one (main_recon_tsmis_FFT.m:177-212)"""
    rng = np.random.default_rng(3)
    X = (rng.standard_normal((230, 230, 2)) + 1j * rng.standard_normal((230, 230, 2))).astype(np.complex64)
    qmap = rng.random((2, 3, 230, 230)).astype(np.float32)
    v5, v73 = str(tmp_path / "v5.mat"), str(tmp_path / "v73.mat")
    scipy.io.savemat(v5, {"X": X, "qmap": qmap})
    write_mat73(v73, {"X": X, "qmap": qmap})
    np.testing.assert_array_equal(H.load_tsmi(v5), H.load_tsmi(v73))
    assert H.load_tsmi(v73).shape == (224, 224, 2)
    np.testing.assert_array_equal(H.load_qmaps(v5, 2), H.load_qmaps(v73, 2))


def test_unsupported_features_are_named(tmp_path):
    p = str(tmp_path / "bad.mat")
    write_mat73(p, {"A": np.eye(3)})
    b = bytearray(open(p, "rb").read())
    b[512 + 8] = 7                                                # superblock version nobody wrote yet
    open(p, "wb").write(bytes(b))
    with pytest.raises(NotImplementedError, match="superblock version 7"):
        mat73.load_mat73(p)
    with pytest.raises(ValueError, match="no HDF5 signature"):
        q = str(tmp_path / "v5.mat")
        scipy.io.savemat(q, {"A": np.eye(3)})
        mat73.load_mat73(q)
