"""The inputs and references of big_svd_ref.py pinned on the host, so that test_gpu_big_svd.py can
be trusted without a GPU: every built state hands the oracle's two-site update the prescribed
spectrum, the side conditions under which the metrics are well defined hold, numpy's own Gram form
stays two orders under the device bars on every case, and the metrics see an error of known size."""
import os

import numpy as np
import pytest

import big_svd_ref as R
from oracle import gates as G
from oracle import mps as M

INPUTS = sorted({(shape, kind) for shape, kind, _, _ in R.CASES})
CUTS = sorted({(shape, kind, max_chi) for shape, kind, max_chi, _ in R.CASES}, key=str)
GRAM_FLOOR = 1e-9  # kGbRelFloor (gram_big.hip): lambda_K > 1e-9 lambda_1 or the job declines


def _id(t):
    return "-".join(f"{x[0]}x{x[1]}" if isinstance(x, tuple) else str(x) for x in t)


@pytest.fixture(scope="module", autouse=True)
def _blas_threads():
    """numpy's BLAS on up to 16 threads for the n = 20 / 21 inputs (importing bench pins it to one)."""
    from threadpoolctl import threadpool_limits

    with threadpool_limits(limits=min(16, os.cpu_count() or 1)):
        yield


@pytest.mark.parametrize("shape,kind", INPUTS, ids=[_id(t) for t in INPUTS])
def test_update_sees_the_prescribed_spectrum(shape, kind):
    """The oracle's cx on the built state decomposes a (2 chi_l) x (2 chi_r) matrix of unit norm whose
    singular values are the prescribed ones to 1e-13; every bond of the input fits the capacity the
    device test gives it and no Schmidt value is zero."""
    b = R.built(shape, kind)
    n, p = b["n"], b["p"]
    m = M.MPS.from_aer(b["aer"])
    assert m.n == n == R.SHAPES[shape][1]
    assert (2 * m.g[p].shape[1], 2 * m.g[p + 1].shape[2]) == shape
    assert max(len(x) for x in m.l) <= 1024 and all(np.all(x > 0) for x in m.l)
    if kind != "rank10":
        assert len(m.l[p]) == min(shape)
    m.svd_log = []
    m.apply_2q(p, p + 1, G.CX)
    (site, s), = m.svd_log
    assert site == p and s.shape == b["sigma"].shape
    assert np.max(np.abs(s - b["sigma"])) <= 1e-13
    assert abs(np.linalg.norm(b["theta"]) - 1.0) <= 1e-13
    assert np.max(np.abs(b["svd"][1] - s)) <= 1e-14  # (metrics' theta' is the matrix the oracle factored)


@pytest.mark.parametrize("shape,kind,max_chi", CUTS, ids=[_id(t) for t in CUTS])
def test_cut_is_well_defined(shape, kind, max_chi):
    """Where values are dropped the rank-K part of theta' is unique only with a gap at K:
    (sigma_K^2 - sigma_K+1^2) / sigma_1^2 >= 5e-6.  `threshold` drops at least 20 values by a clear
    tail comparison; `below_floor` keeps everything and its last value is under the Gram floor; every
    other case keeps its values above the floor, so the Gram path has no reason to decline."""
    s = R.SPECTRA[kind](min(shape))
    thr = R.case_thr(kind)
    K = M.truncation_rank(s, thr, max_chi)
    assert K == R.kept(R.built(shape, kind), kind, max_chi)
    C = len(s)
    if K < C:
        assert (s[K - 1] ** 2 - s[K] ** 2) / s[0] ** 2 >= 5e-6
    if max_chi is not None:
        assert K == max_chi
    if kind == "threshold":
        k2, margin = R.threshold_margin(s, thr)
        assert k2 == K and C - K >= 20 and margin > 1e-3
        assert np.all(s * s > M.CHOP)  # (the tail rule, not CHOP, dropped them)
    if kind == "rank10":
        assert K == 10
    if kind == "below_floor":
        assert K == C and s[-1] ** 2 > M.CHOP and (s[-1] / s[0]) ** 2 < GRAM_FLOOR
    else:
        assert (s[K - 1] / s[0]) ** 2 > 5 * GRAM_FLOOR


@pytest.mark.parametrize("shape,kind,max_chi", CUTS, ids=[_id(t) for t in CUTS])
def test_gram_form_reference_under_1e13(shape, kind, max_chi):
    """numpy's Gram form on the same theta': (a) weighted, (b), (c) and (d) at or under 1e-13 -- the
    device bars (1e-12, 1e-11) ask nothing the Gram form cannot give."""
    b = R.built(shape, kind)
    got = R.gram_form_reference(b["theta"], R.kept(b, kind, max_chi), b["svd"])
    print(_id((shape, kind, max_chi)), " ".join(f"{k}={got[k]:.2e}" for k in R.KEYS))
    for k in ("sig_w", "theta", "iso_direct", "iso_derived"):
        assert got[k] <= 1e-13, (k, got)


def test_metrics_on_the_oracles_own_update_and_a_known_error():
    """metrics on the oracle's read-back (LAPACK) is at rounding; a column of the left tensor moved by
    1e-7 of its neighbour shows as 1e-7 in that side's isometry and as 1e-7 lam_i in (b): linear."""
    shape, kind = (256, 136), "decay"
    b = R.built(shape, kind)
    p, K = b["p"], 68
    m = M.MPS.from_aer(b["aer"])
    m.apply_2q(p, p + 1, G.CX, 1e-16, K)
    got = R.metrics(b["theta"], K, m.to_aer(), p, b["svd"])
    assert all(got[k] <= 1e-13 for k in R.KEYS), got
    d = 1e-7
    m.g[p][:, :, 3] += d * m.g[p][:, :, 4]
    bad = R.metrics(b["theta"], K, m.to_aer(), p, b["svd"])
    lam = m.l[p]
    assert abs(bad["theta"] - d * lam[3]) <= 1e-3 * d * lam[3]
    assert abs(bad["iso_derived"] - d * lam[3] * lam[4] / lam[0] ** 2) <= 1e-3 * d  # (the left side is derived here)
    assert bad["iso_direct"] <= 1e-13 and bad["sig"] <= 1e-13
    # the same on the Gram side of the transposed shape
    b = R.built((136, 256), kind)
    m = M.MPS.from_aer(b["aer"])
    m.apply_2q(p, p + 1, G.CX, 1e-16, K)
    m.g[p][:, :, 3] += d * m.g[p][:, :, 4]
    bad = R.metrics(b["theta"], K, m.to_aer(), p, b["svd"])
    assert abs(bad["iso_direct"] - d) <= 1e-3 * d
    m.l[p][5] += 1e-9
    assert abs(R.metrics(b["theta"], K, m.to_aer(), p, b["svd"])["sig"] - 1e-9) <= 1e-12
