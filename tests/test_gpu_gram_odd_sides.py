"""The Gram path's two-site SVD (aqc_svd_debug variant 7, svd_gram.h) at Gram sides C that leave
remainders in its row loops.  test_gpu_svd.py runs C in {72, 80, 96, 128}: whole 8-row chunks in
S5's factorisation and solves, 7 rows after the Sturm count's groups of 8 (rows 1 .. C - 1).  The
sides here leave 1, 3 and 5 Sturm rows ((C - 1) % 8) and S5 tails of 2, 4 and 6 rows (C % 8), below
one chunk (C < 8), on both sides of S3's tail switch at 64, and in both orientations of theta.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIDES = [4, 6, 10, 12, 14, 18, 62, 66, 100, 126]
SHAPES = [(128, c) for c in SIDES] + [(14, 128), (100, 128)]


def _gram_ticks():
    """Phase ticks accumulated since the last call (the call resets them)."""
    from adaptaqc_amd import _lib

    t = np.zeros(12)
    _lib.check(_lib.lib().aqc_svd_gram_ticks(_lib.ptr(t)))
    return t


def _spectrum_theta(m, n, s, seed):
    rng = np.random.default_rng(seed)
    c = min(m, n)
    u, _ = np.linalg.qr(rng.standard_normal((m, c)) + 1j * rng.standard_normal((m, c)))
    v, _ = np.linalg.qr(rng.standard_normal((n, c)) + 1j * rng.standard_normal((n, c)))
    return (u * s[None, :]) @ v.conj().T


def _run_gram(theta):
    from adaptaqc_amd import _lib

    m, n = theta.shape
    c = min(m, n)
    th = np.asfortranarray(theta.astype(np.complex128)).ravel(order="F").copy()
    w = np.zeros(c * c, np.complex128)
    sig = np.zeros(c)
    perm = np.zeros(c, np.int32)
    sw = ctypes.c_int()
    _lib.check(_lib.lib().aqc_svd_debug(th.ctypes.data, m, n, 7, 0, w.ctypes.data, sig.ctypes.data,
                                        perm.ctypes.data, ctypes.byref(sw)))
    return w.reshape(c, c).T, sig  # columns of W as columns


@pytest.mark.parametrize("m,n", SHAPES)
def test_gram_path_odd_sides_vs_numpy(m, n):
    """Spectrum 0.93^i: the Gram path runs to the end and returns the top K = min(64, C) triplets:
    sigma to 1e-12 sigma_1, the kept right subspace of X (theta or theta^H, L >= C) to 1e-10,
    V^H V - I to 1e-11 (the tolerances of test_gpu_svd.py::test_gram_path_vs_numpy)."""
    c = min(m, n)
    theta = _spectrum_theta(m, n, 0.93 ** np.arange(c), 7 + m + n)
    _gram_ticks()
    w, sig = _run_gram(theta)
    assert _gram_ticks()[4] > 0, "the Gram path declined"
    K = min(64, c)
    x = theta if m >= n else theta.conj().T
    _, s_ref, vh = np.linalg.svd(x)
    order = np.argsort(-sig)
    got = sig[order]
    np.testing.assert_allclose(got[:K], s_ref[:K], rtol=0, atol=1e-12 * s_ref[0])
    assert np.all(got[K:] == 0.0)
    V = w[:, order[:K]] / got[None, :K]
    Vr = vh[:K].conj().T
    assert np.linalg.norm(V @ V.conj().T - Vr @ Vr.conj().T, 2) < 1e-10
    assert np.max(np.abs(V.conj().T @ V - np.eye(K))) < 1e-11
