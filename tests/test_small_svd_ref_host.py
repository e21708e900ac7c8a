"""The inputs and references of small_svd_ref.py pinned on the host, so that test_gpu_small_svd.py
can be trusted without a GPU: every built state fits its capacity and hands the oracle's two-site
update the prescribed spectrum under the case's own gate matrix, every cut is decided clear of the
rules' edges, and numpy's own Gram form (LAPACK re-factorised from its own rank-K product where the
Jacobi answers) stays at or below a tenth of every device bar on every case."""
import numpy as np
import pytest

import big_svd_ref as R
import small_svd_ref as S
from oracle import gates as G
from oracle import mps as M
from test_gpu_big_svd import BARS

JACOBI_BARS = dict(BARS, sig=1e-12)
INPUTS = sorted({S.case_input(c) for c in S.CASES}, key=str)
CUTS = sorted({S.case_input(c) + (c[3],) for c in S.CASES}, key=str)


def _id(t):
    return "-".join(f"{x[0]}x{x[1]}" if isinstance(x, tuple) else str(x) for x in t)


def test_gate_layouts():
    """op4_of_matrix is the layout apply_2q gives a gate on (p, p + 1) (big_svd_ref.OP4 for cx),
    matrix_of_op4 its inverse, reversed_matrix the same gate named from the other qubit."""
    rng = np.random.default_rng(1)
    np.testing.assert_array_equal(S.op4_of_matrix(G.CX), R.OP4)
    u = R.matrix_with_spectrum(4, 4, np.ones(4), rng)
    np.testing.assert_array_equal(S.matrix_of_op4(S.op4_of_matrix(u)), u)
    np.testing.assert_array_equal(S.reversed_matrix(u).reshape(2, 2, 2, 2), S.op4_of_matrix(u))
    a, b = R._isometry(rng, 2, 2), R._isometry(rng, 2, 2)
    # little-endian over (p, p + 1): the first qubit is the low bit, so A on site p is kron(B, A)
    np.testing.assert_allclose(S.matrix_of_op4(S.product_op4(a, b)), np.kron(b, a), atol=1e-15)
    np.testing.assert_allclose(S.matrix_of_op4(S.dressed_cx_op4(a, b)), np.kron(b, a) @ G.CX, atol=1e-15)


def test_spectra_for_any_length():
    """At 128 values the kinds are big_svd_ref's; shorter runs drop the pairs that do not fit (at 64 the
    entry (50, 1e-5)) and the kinds that are undefined."""
    assert S.pair_gaps(128) == R.PAIR_GAPS
    np.testing.assert_array_equal(S.spectrum("pairs", 128), R._pairs(128))
    assert (50, 1e-5) not in S.pair_gaps(64) and (40, 1e-5) in S.pair_gaps(64)
    assert S.pair_gaps(8) == ((4, 5e-8),)
    for kind, r in (("clusters", 16), ("plateau", 16), ("threshold", 24), ("rank10", 10)):
        assert S.spectrum(kind, r) is None and S.spectrum(kind, r + 1) is not None
    for kind in S.ALL_KINDS:
        for r in (8, 12, 24, 40, 64, 72, 100, 128):
            s = S.spectrum(kind, r)
            if s is not None:
                assert s.shape == (r,) and abs(np.linalg.norm(s) - 1) < 1e-14 and np.all(np.diff(s) <= 0)


def test_table_reaches_every_route_and_shape():
    for route in S.ROUTES:
        shapes = {c[1] for c in S.CASES if c[0] == route}
        assert shapes == set(S.SHAPES[route]) | (set(S.ENDS) if route in S.END_ROUTES else set()), route
    assert [c[1:] for c in S.CASES if c[0] == "L128"] == [c[1:] for c in S.CASES if c[0] == "F128"]
    kinds = {c[2] for c in S.CASES if c[0] == "L128"}
    assert kinds == set(S.ALL_KINDS)
    # the headline regime: capacity 64, theta' 128 x 128 of full rank, max_chi = 64 cutting it
    assert ("F128", (128, 128), "pairs", 64) in S.CASES and ("F128", (128, 128), "clusters", 64) in S.CASES
    # the wide S5 / S6 (K > 64) and the classes that differ from 2 x capacity
    assert ("W128", (128, 128), "pairs", None) in S.CASES and ("W128", (128, 128), "clusters", 69) in S.CASES
    assert S.svd_class("W128", (64, 64)) == 64 and S.svd_class("W128", (32, 32)) == 32
    assert S.svd_class("W128", (128, 40)) == 128 and S.svd_class("L128", (2, 4)) == 128


@pytest.mark.parametrize("fam,shape,kind", INPUTS, ids=[_id(t) for t in INPUTS])
def test_update_sees_the_prescribed_spectrum(fam, shape, kind):
    """Every bond of the input fits the smallest capacity a case gives it; the oracle's update under the
    case's gate matrix -- named from either qubit -- decomposes a (2 chi_l) x (2 chi_r) matrix of unit
    norm with the prescribed singular values to 1e-13."""
    b = S.built(fam, shape, kind)
    n, p = b["n"], b["p"]
    m = M.MPS.from_aer(b["aer"])
    assert m.n == n <= 14
    assert (2 * m.g[p].shape[1], 2 * m.g[p + 1].shape[2]) == shape
    caps = {S.case_cap(c[0], c[1]) for c in S.CASES if S.case_input(c) == (fam, shape, kind)}
    assert max([len(x) for x in m.l] + [1]) <= min(caps)
    if fam == "lim":
        assert max(len(x) for x in m.l) <= max(shape) // 2
        if kind != "rank10":
            assert len(m.l[p]) == min(shape) // 2  # (half of theta's rank: max_chi has to cut)
            off = b["theta"].reshape(2, shape[0] // 2, 2, shape[1] // 2)
            assert np.linalg.norm(off[0, :, 1, :]) > 0.1 and np.linalg.norm(off[1, :, 0, :]) > 0.1  # (dense)
    for qubits, mat in (((p, p + 1), b["gate"]), ((p + 1, p), S.reversed_matrix(b["gate"]))):
        o = m.copy()
        o.svd_log = []
        o.apply_2q(qubits[0], qubits[1], mat)
        (site, s), = o.svd_log
        assert site == p and s.shape == b["sigma"].shape
        assert np.max(np.abs(s - b["sigma"])) <= 1e-13
    assert abs(np.linalg.norm(b["theta"]) - 1.0) <= 1e-13
    assert np.max(np.abs(b["svd"][1] - b["sigma"])) <= 1e-13
    assert np.max(np.abs(b["svd"][1] - s)) <= 1e-14  # (metrics' theta' is the matrix the oracle factored)


@pytest.mark.parametrize("fam,shape,kind,max_chi", CUTS, ids=[_id(t) for t in CUTS])
def test_cut_is_decided_and_the_bars_are_attainable(fam, shape, kind, max_chi):
    """truncation_rank on the built theta' gives the K of the table; `threshold` clears both deciding
    comparisons by 0.3 thr; lambda_K is a factor 5 away from the Gram floor on either side; and the
    condition that keeps the device test honest: numpy's Gram form, where the Gram path's own rule
    lambda_K > 1e-9 lambda_1 holds, and LAPACK's SVD re-factorised from its own rank-K product, on every
    case, stay at or below a tenth of every device bar."""
    b = S.built(fam, shape, kind)
    s, thr = b["sigma"], R.case_thr(kind)
    K = S.kept(b, kind, max_chi)
    cases = [c for c in S.CASES if S.case_input(c) + (c[3],) == (fam, shape, kind, max_chi)]
    for c in cases:
        assert S.cut_admitted(s, kind, max_chi, S.case_cap(c[0], c[1])) == K
    if max_chi is not None:
        assert K == max_chi
    if kind == "threshold" and max_chi is None:
        k2, margin = R.threshold_margin(s, thr)
        assert k2 == K and margin >= 0.3
    if kind == "rank10":
        assert K == min(10, max_chi or 10)
    ratio = (s[K - 1] / s[0]) ** 2
    assert not 0.2 * S.GRAM_FLOOR <= ratio <= 5 * S.GRAM_FLOOR
    if ratio > S.GRAM_FLOOR:
        got = R.gram_form_reference(b["theta"], K, b["svd"])
        print(_id((fam, shape, kind, max_chi)), "gram form:", " ".join(f"{k}={got[k]:.2e}" for k in S.KEYS))
        assert all(got[k] <= BARS[k] / 10 for k in S.KEYS), got
    u, sv, vh = b["svd"]
    u2, s2, vh2 = np.linalg.svd((u[:, :K] * sv[:K]) @ vh[:K], full_matrices=False)
    got = R._numbers(b["theta"], b["svd"], K, u2[:, :K], s2[:K] / np.linalg.norm(s2[:K]), vh2[:K])
    print(_id((fam, shape, kind, max_chi)), "LAPACK again:", " ".join(f"{k}={got[k]:.2e}" for k in S.KEYS))
    assert all(got[k] <= JACOBI_BARS[k] / 10 for k in S.KEYS), got


def test_expected_paths():
    """expected_path names each of its five answers somewhere in the table, and every route's cases
    are the ones its switches can reach."""
    seen = {}
    for c in S.CASES:
        b = S.built(*S.case_input(c))
        path = S.expected_path(c, b["sigma"], S.kept(b, c[2], c[3]))
        seen.setdefault(c[0], set()).add(path)
    assert seen["J128"] == seen["J64"] == seen["J32"] == {"jacobi"}
    assert seen["L128"] == seen["F128"] == {"gram", "certified", "floor", "shape"}
    assert seen["W128"] == {"gram", "certified", "floor", "jacobi"}
