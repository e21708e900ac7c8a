"""One large two-site update (2 chi > 128: gram_big.hip, and bjacobi.hip where it declines) against
the LAPACK SVD of the same theta', per update and linearly in the error.

The end-to-end tests of this path (test_gpu_gram_big.py, test_gpu_bigchi.py) compare fidelities,
which move by delta^2 / 2 for a state error delta, on random states with generic spectra and square
theta' at the kernels' template sizes.  Here one DeviceMPS per case loads a state built so that its
cx(a, a + 1) decomposes a prescribed matrix (big_svd_ref.state_with_theta): exact and near
multiplicities, a cluster of C - 16 members, a rank-10 theta', a tail threshold deciding the kept
count, kept counts off every tile size, and shapes that pad (C < CT), transpose (2 chi_l < 2 chi_r)
and use the long layout (L > CT).  After the gate: the new bond dimension is truncation_rank's K,
every other tensor is bit-identical, the path that ran is the expected one (gram_big_stats), and
big_svd_ref.metrics against LAPACK stays under the bars the 2 chi <= 128 kernels already meet in
test_gpu_svd.py -- all relative to a theta' of unit norm:

  (a) Schmidt values             <= 1e-9   (1e-12 weighted by sigma_i / sigma_1: the error in sigma^2)
  (b) ||theta_dev - theta_K||_F  <= 1e-12
  (c) isometry, direct side      <= 1e-11  (max |A^H A - I|; the Gram side: the shorter one, the right
                                           one when they are equal)
  (d) isometry, derived side     <= 1e-12  (weighted by lam'_i lam'_j / lam'_1^2)
  below_floor (the block Jacobi answers, no Gram squaring): (a) unweighted and (b) <= 1e-12 too, and
  its direct side is the other one: it rotates the columns of X (the longer side, the left one when
  they are equal) and derives the shorter side as X^H U / sigma.  Measured with (c) on the shorter
  side as for the Gram path: 1e-8 ... 4e-8 unweighted at sigma_C / sigma_1 = 1e-6 (the eps sigma_1 /
  sigma_j of that division, 3e-14 weighted), against 6e-14 on the side the rotations orthogonalise.

numpy's own Gram form reaches 2e-14 on all of these inputs (test_big_svd_ref_host.py).

Worst measured value per kind and class on the MI355X (over the kind's shapes, cuts and modes):

  kind         class  (a)      (a) wtd  (b)      (c)      (d)
  decay          256  6.8e-15  4.8e-16  6.2e-15  2.8e-14  1.5e-15
  clusters       256  4.0e-15  6.7e-16  1.2e-14  4.3e-14  2.9e-15
  pairs          256  4.3e-15  5.3e-16  6.7e-15  4.9e-14  8.9e-16
  plateau        256  9.2e-14  2.2e-15  5.7e-15  8.6e-14  4.4e-15
  rank10         256  3.3e-16  2.3e-16  2.1e-15  1.4e-15  4.4e-16
  threshold      256  4.7e-16  4.5e-16  6.6e-15  5.5e-14  1.0e-15
  below_floor    256  8.2e-15  7.9e-15  2.8e-13  5.7e-14  1.7e-13
  decay          512  1.8e-15  3.3e-16  3.9e-15  1.8e-14  8.4e-16
  clusters       512  2.8e-15  5.0e-16  1.6e-14  2.2e-14  3.4e-15
  pairs          512  2.5e-15  4.3e-16  3.8e-15  1.7e-14  1.6e-15
  plateau        512  9.8e-14  4.7e-15  1.2e-14  2.4e-13  1.1e-14
  rank10         512  4.4e-16  3.3e-16  2.1e-15  2.0e-15  6.5e-16
  below_floor    512  1.3e-14  1.3e-14  2.7e-13  5.9e-14  1.9e-13
  decay         1024  2.5e-16  2.3e-16  8.8e-15  1.1e-14  9.7e-16
  clusters      1024  2.9e-15  2.2e-16  4.5e-15  1.1e-14  2.4e-15

Before k_gb_gs's cluster gap went from 1e-7 to 1e-5 ||T|| (gram_big.hip kGbClusterGap) the same run
missed the bars on 14 cases: `pairs` on every shape but 256 x 136, with (b) up to 1.5e-12, (d) up to
2.1e-12 and (c) up to 1.2e-10 (200 x 200; 8.7e-11 on 400 x 400); `clusters` at K = C on 400 x 400 with
(c) 2.6e-11 (the small sigma^2 of the geometric run, whose absolute gaps are 1e-7 ... 1e-6 ||T||).
"""
import numpy as np
import pytest

import big_svd_ref as R
from bench import vidal_from_tensors
from conftest import to_circuit

pytestmark = pytest.mark.gpu

BARS = {"sig": 1e-9, "sig_w": 1e-12, "theta": 1e-12, "iso_direct": 1e-11, "iso_derived": 1e-12}
DEFAULT_MODE = {"aqc_gb_set_stages": 2, "aqc_gb_set_tail": 1}


def _blas_threads():
    """numpy's BLAS on up to 16 threads for the inputs' canonical forms and the LAPACK references
    (importing bench pins it to one for the CPU baseline's workers)."""
    import os

    from threadpoolctl import threadpool_limits

    return threadpool_limits(limits=min(16, os.cpu_count() or 1))


def _assert_rest_untouched(before, after, p):
    (gb, lb), (ga, la) = before, after
    for i, ((a0, a1), (b0, b1)) in enumerate(zip(gb, ga)):
        if i not in (p, p + 1):
            np.testing.assert_array_equal(a0, b0, err_msg=f"site {i}")
            np.testing.assert_array_equal(a1, b1, err_msg=f"site {i}")
    for i, (x, y) in enumerate(zip(lb, la)):
        if i != p:
            np.testing.assert_array_equal(x, y, err_msg=f"bond {i}")


@pytest.mark.parametrize("case", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_one_update_against_lapack(case):
    from adaptaqc_amd import _lib
    from adaptaqc_amd.circuit import device_ops
    from adaptaqc_amd.device import DeviceMPS

    shape, kind, max_chi, mode = case
    with _blas_threads():
        b = R.built(shape, kind)
    n, p, aer = b["n"], b["p"], b["aer"]
    K = R.kept(b, kind, max_chi)
    cap = max(len(x) for x in aer[1])
    d = DeviceMPS(n, cap, R.case_thr(kind), max_chi)
    d.load_aer(aer)
    lib = _lib.load()
    if mode:
        _lib.check(getattr(lib, mode[0])(mode[1]))
    try:
        _lib.gram_big_stats()
        d.apply(device_ops(to_circuit(n, [("cx", (p, p + 1), ())])))
        st = _lib.gram_big_stats()
    finally:
        if mode:
            _lib.check(getattr(lib, mode[0])(DEFAULT_MODE[mode[0]]))
    after = d.to_aer()
    d.close()
    with _blas_threads():
        got = R.metrics(b["theta"], K, after, p, b["svd"], jacobi=kind == "below_floor") if len(after[1][p]) == K else None
    print(f"{R.case_id(case)}: K = {len(after[1][p])} (want {K}) {st}", flush=True)
    if got:
        print(f"{R.case_id(case)}: " + " ".join(f"{k}={got[k]:.2e}" for k in R.KEYS), flush=True)
    assert len(after[1][p]) == K
    _assert_rest_untouched(aer, after, p)
    assert st["calls"] == 1, st
    if kind == "below_floor":
        assert st["declined_floor"] == 1 and st["taken"] == 0, st
    else:
        assert st["taken"] == 1 and st["timeouts"] == 0, st
        assert st["declined_floor"] == 0 and st["declined_certificate"] == 0, st
    if kind == "rank10":
        assert st["certificates"] == 1 and st["certified"] == 1, st
    bars = dict(BARS, sig=1e-12) if kind == "below_floor" else BARS
    missed = {k: got[k] for k in R.KEYS if not got[k] <= bars[k]}
    assert not missed, (missed, got)


# bonds 0 .. 20 of the mixed wave's state: the pairs (7, 8), (10, 11), (14, 15) have outer bonds
# (100, 100), (150, 150), (60, 16): sides 200, 300 and 120
MIXED_DIMS = [1, 2, 4, 8, 16, 32, 64, 100, 100, 100, 150, 150, 150, 100, 60, 32, 16, 8, 4, 2, 1]
MIXED_PAIRS = [(7, 8), (10, 11), (14, 15)]


def test_mixed_class_wave_equals_sequential():
    """mps.hip picks each job's SVD kernel from the job's own side, so a wave that mixes classes --
    side 120 (the 2 chi <= 128 kernels), 200 (class 256) and 300 (class 512) -- equals the same three
    gates applied one call at a time, bit for bit."""
    from adaptaqc_amd import _lib
    from adaptaqc_amd.circuit import device_ops
    from adaptaqc_amd.device import DeviceMPS

    n, cap = 20, max(MIXED_DIMS)
    rng = np.random.default_rng(20)
    dims = MIXED_DIMS
    with _blas_threads():
        aer = vidal_from_tensors([rng.standard_normal((2, dims[i], dims[i + 1])) + 1j * rng.standard_normal((2, dims[i], dims[i + 1]))
                                  for i in range(n)])
    assert [len(x) for x in aer[1]] == dims[1:-1]
    for a, _ in MIXED_PAIRS:
        assert 2 * max(dims[a], dims[a + 2]) in (120, 200, 300)
    ops = [("cx", pr, ()) for pr in MIXED_PAIRS]
    one = DeviceMPS(n, cap, 1e-16, cap)
    one.load_aer(aer)
    _lib.gram_big_stats()
    one.apply(device_ops(to_circuit(n, ops)))
    st = _lib.gram_big_stats()
    assert st["calls"] == 2 and st["taken"] == 2, st  # (classes 256 and 512, one job each)
    seq = DeviceMPS(n, cap, 1e-16, cap)
    seq.load_aer(aer)
    for op in ops:
        seq.apply(device_ops(to_circuit(n, [op])))
    np.testing.assert_array_equal(one.dims(), seq.dims())
    assert [int(one.dims()[a + 1]) for a, _ in MIXED_PAIRS] == [cap, cap, 32]  # (2 chi capped; 2 * 16)
    (g1, l1), (g2, l2) = one.to_aer(), seq.to_aer()
    for (a0, a1), (b0, b1) in zip(g1, g2):
        np.testing.assert_array_equal(a0, b0)
        np.testing.assert_array_equal(a1, b1)
    for x, y in zip(l1, l2):
        np.testing.assert_array_equal(x, y)
