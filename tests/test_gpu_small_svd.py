"""One small two-site update (2 chi <= 128) on every SVD route against the LAPACK SVD of the same
theta', per update and linearly in the error.

The end-to-end tests of this path (test_gpu_mps.py, test_gpu_threshold.py, test_gpu_headline.py)
compare overlaps and fidelities, which move by delta^2 / 2 for a state error delta, and
test_gpu_svd.py drives the SVD kernel alone on smoothly decaying spectra.  Here one DeviceMPS per case
loads a state built so that one gate matrix on (p, p + 1) decomposes a prescribed theta'
(small_svd_ref.py: exact and near multiplicities, a plateau, a rank-10 theta', a tail threshold
deciding the kept count, kept counts off every tile size, shapes that pad and transpose, the chain's
ends), so that k_theta, the SVD, k_rank and k_split_* -- or the fused k_chain's own phases -- all run.
After the gate: the new bond is truncation_rank's K, every other tensor is bit-identical, gram_stats
names the path that small_svd_ref.expected_path derives from svd_gram.h's rules, and
big_svd_ref.metrics against LAPACK stays under test_gpu_big_svd.BARS (theta' of unit norm):

  (a) Schmidt values 1e-9 (1e-12 weighted by sigma_i / sigma_1; 1e-12 unweighted where the Jacobi
  answers), (b) ||theta_dev - theta_K||_F 1e-12, (c) isometry of the direct side 1e-11, (d) isometry
  of the derived side, weighted by lam'_i lam'_j / lam'_1^2, 1e-12.

The direct side: both small kernels deliver W = V Sigma on X's column side (TwoSiteJob::qr = 1; X =
theta' or theta'^H, the longer side down), and split_copy_body copies W / sigma into the Gamma of that
side (tr = (M < N) != qr): the shorter side of theta', the right one when they are equal -- for the
register Jacobi too, so metrics' jacobi flag (the block Jacobi's other side) stays off here.

Routes (small_svd_ref.ROUTES): L128 lock-step launches at capacity 64 (k_theta, k_svd_gram, k_rank,
k_split_copy, k_split_gemm), F128 the fused k_chain on the same inputs (and its theta against
L128's: 1e-12, 1e-9 under a certificate; measured <= 3.0e-14), J128 k_jacobi_reg<128, 8> on the same
inputs, J64 / J32 capacities 32 / 16, W128 capacity 128 (100) with generic full-rank inputs: the class
from the job's side, K up to 128 (the wide S5, S6 in two passes).  k_theta32 is reached by a batch of
64, the gate named from its right qubit by two cases, a wave of classes 32, 64 and 128 by one.

numpy's own Gram form, and LAPACK's SVD re-factorised from its own rank-K product, stay a tenth under
every bar on every case (test_small_svd_ref_host.py).

Worst measured value per route, class and kind on the MI355X (over the kind's shapes and cuts):

  route  class  kind         cases  (a)      (a) wtd  (b)      (c)      (d)
  L128     128  decay           17  3.1e-15  6.7e-16  8.6e-15  2.0e-12  7.7e-16
  L128     128  clusters        11  5.4e-15  3.9e-16  2.2e-14  6.2e-12  2.0e-15
  L128     128  pairs            9  6.7e-15  5.6e-16  8.4e-15  6.5e-13  1.0e-15
  L128     128  rank10           5  5.0e-16  2.4e-16  2.3e-15  1.9e-15  8.9e-16
  L128     128  threshold       11  8.1e-16  4.1e-16  7.8e-15  1.6e-14  6.8e-16
  L128     128  plateau          1  1.5e-13  3.3e-16  2.2e-15  1.4e-15  4.2e-16
  L128     128  below_floor      1  5.6e-16  4.4e-16  1.1e-14  8.4e-15  9.5e-15
  F128     128  decay           17  9.0e-15  6.7e-16  8.2e-15  4.0e-13  6.7e-16
  F128     128  clusters        11  2.1e-14  3.9e-16  2.2e-14  2.2e-12  1.9e-15
  F128     128  pairs            9  9.2e-15  6.1e-16  1.0e-14  4.9e-13  8.0e-16
  F128     128  rank10           5  5.0e-16  2.4e-16  2.1e-15  1.3e-15  8.9e-16
  F128     128  threshold       11  5.0e-16  3.7e-16  7.5e-15  2.0e-14  1.2e-15
  F128     128  plateau          1  2.0e-13  4.4e-16  2.2e-15  1.4e-15  2.9e-16
  F128     128  below_floor      1  7.2e-16  4.4e-16  1.1e-14  8.4e-15  9.4e-15
  J128     128  decay           11  2.1e-15  2.1e-15  4.0e-14  2.8e-14  3.6e-14
  J128     128  clusters        11  9.4e-16  8.3e-16  4.1e-14  2.8e-14  3.5e-14
  J128     128  pairs            9  1.9e-15  1.9e-15  4.4e-14  2.8e-14  3.5e-14
  J128     128  rank10           5  5.0e-16  2.4e-16  6.8e-15  1.1e-14  7.8e-15
  J128     128  threshold       11  2.4e-15  2.4e-15  4.7e-14  2.8e-14  3.6e-14
  J128     128  plateau          1  5.0e-16  2.2e-16  1.1e-14  8.9e-15  1.0e-14
  J128     128  below_floor      1  5.6e-16  4.4e-16  1.1e-14  8.4e-15  9.5e-15
  J64       64  decay            7  8.9e-16  8.9e-16  1.2e-14  1.4e-14  8.6e-15
  J64       64  clusters         6  3.9e-16  3.9e-16  1.4e-14  1.4e-14  1.7e-14
  J64       64  pairs            7  8.9e-16  8.9e-16  1.4e-14  1.4e-14  1.3e-14
  J64       64  rank10           3  3.3e-16  2.3e-16  4.3e-15  1.1e-14  4.7e-15
  J64       64  threshold        2  1.1e-15  9.9e-16  1.0e-14  1.4e-14  1.4e-14
  J64       64  plateau          2  6.4e-16  4.4e-16  3.4e-15  4.6e-14  5.9e-15
  J64       64  below_floor      1  2.2e-16  1.2e-16  8.3e-15  5.2e-15  5.5e-15
  J32       32  decay           11  3.6e-16  3.3e-16  4.9e-15  6.3e-15  3.5e-15
  J32       32  clusters         1  3.3e-16  3.3e-16  4.8e-15  5.3e-15  6.4e-15
  J32       32  pairs            5  5.0e-16  4.4e-16  5.0e-15  6.8e-15  4.1e-15
  J32       32  plateau          1  4.4e-16  3.5e-16  6.8e-15  6.8e-15  6.1e-15
  J32       32  rank10           3  4.4e-16  4.4e-16  2.3e-15  5.1e-15  2.1e-15
  J32       32  threshold        1  2.2e-16  2.2e-16  4.6e-15  2.2e-15  1.1e-14
  J32       32  below_floor      3  3.3e-16  2.2e-16  3.3e-15  8.1e-16  3.3e-15
  W128     128  decay           15  1.6e-14  6.7e-16  8.5e-15  4.0e-12  1.3e-15
  W128     128  clusters        15  1.2e-14  5.6e-16  1.5e-14  5.1e-12  3.9e-15
  W128     128  pairs           13  6.2e-15  5.3e-16  1.0e-14  2.9e-12  7.9e-16
  W128     128  plateau          5  1.8e-13  7.8e-16  2.9e-15  2.4e-15  1.1e-15
  W128     128  rank10           5  1.0e-15  7.0e-16  2.4e-15  3.1e-15  6.7e-16
  W128     128  below_floor      5  2.0e-15  1.6e-15  5.7e-14  2.8e-14  3.5e-14
  W128     128  threshold       13  6.1e-16  5.1e-16  8.1e-15  2.8e-14  8.9e-16
  W128      64  decay            3  1.5e-15  1.5e-15  1.4e-14  1.4e-14  8.6e-15
  W128      64  clusters         3  3.3e-16  3.3e-16  1.1e-14  1.3e-14  1.2e-14
  W128      64  pairs            3  9.4e-16  8.5e-16  1.2e-14  1.4e-14  1.3e-14
  W128      64  plateau          1  1.8e-15  1.8e-15  2.5e-14  1.4e-14  1.8e-14
  W128      64  rank10           1  3.3e-16  3.3e-16  1.8e-15  2.7e-15  9.9e-16
  W128      64  below_floor      1  7.2e-16  6.7e-16  1.8e-14  1.4e-14  1.8e-14
  W128      64  threshold        3  1.3e-15  1.3e-15  1.6e-14  1.4e-14  1.6e-14
  W128      32  decay            3  2.8e-16  1.4e-16  6.5e-15  7.0e-15  5.6e-15
  W128      32  clusters         3  5.0e-16  5.0e-16  5.9e-15  4.0e-15  7.1e-15
  W128      32  pairs            2  4.4e-16  2.3e-16  6.5e-15  7.0e-15  6.7e-15
  W128      32  plateau          2  3.3e-16  3.3e-16  1.0e-14  7.7e-15  5.8e-15
  W128      32  rank10           1  3.3e-16  2.3e-16  1.5e-15  5.6e-16  2.4e-16
  W128      32  below_floor      1  6.7e-16  6.7e-16  5.6e-15  7.0e-15  9.4e-15
  W128      32  threshold        1  7.2e-16  3.7e-16  5.8e-15  4.1e-15  1.0e-14

Before the sweep stop rule of jacobi_reg_body (mps.hip) also asked for every pair's cosine to be at most
kStopCos = 3e-13, two cases missed the bars by five orders: `plateau` at K = C where the register
Jacobi answers, J128-128x40 ((b) 2.0e-7, (c) 1.9e-7, (d) 1.2e-7) and W128-64x64 (k_jacobi_reg<64, 4>:
(b) 2.5e-7, (c) 1.9e-7, (d) 1.9e-7).  The error sat between a large column (sigma = 0.6) and the
plateau's columns (sigma = 6e-5): |V^H V| = 1.9e-7 there, 1.9e-3 on the derived side.  A sweep whose
rotations all moved at most jtiny^2 of their pair's squared norms was the last; that mass is relative
to the larger norm, so a large and a small column passed at cosines up to jtiny |a| / |b|, and a
rotation inside the plateau moves no mass at any angle while it carries what one plateau column still
has against a large column into a column that was visited already.  (A cosine bound of jtiny = 1e-6
left (c) at 1.9e-7: the carried part is linear in it.)  After: (b) 1.1e-14 and 2.5e-14, (c) 8.9e-15
and 1.4e-14; test_gpu_svd.py's sweep bounds hold.

Before gs_clusters (svd_gram.h; S5 of k_svd_gram and k_chain) clustered below 1e-5 ||T|| where the gap
is also below 5% of the eigenvalues (below 1e-7 ||T|| as before whatever they are)
(aqc::kGramClusterGap, shared with gram_big.hip) and re-iterated collapsed members, the same run
missed the bars on 6 Gram cases: `pairs` on W128 128x128 at every cut, (b) 1.1e-12 with (c) 7.3e-12
((b) 6.0e-13 ... 8.3e-13 on L128 / F128); and `clusters` on F128 72x128, (b) 4.5e-12, (c) 1.8e-11, (d)
4.4e-12 against 1.1e-14 in L128 on a theta that differs in its last bits (two members of the 8-fold
sigma = 0.5 came out as the same eigenvector to ~1e-5, and one Gram-Schmidt pass scaled the rounding
noise of what was left up), with F128 and L128 1.1e-12 apart on 72x128 `pairs`.  Worst of those kinds
before: (b) 4.5e-12, (c) 1.8e-11, (d) 4.4e-12; after: (b) 2.2e-14, (c) 6.2e-12 (the small sigma^2 of `clusters`' geometric run, 9.5% apart, stay on
their own), (d) 3.9e-15.  With the
gap set to 0 on a scratch build (of the plain 1e-5 rule) 77 more tests fail: every `clusters` and `pairs` case on L128, F128
and W128, `plateau` where the Gram path answers, the batch of 64 and the reversed L128 case; the first
of them is L128-128x128-clusters-K64.
"""
import numpy as np
import pytest

import big_svd_ref as R
import small_svd_ref as S
from bench import vidal_from_tensors
from oracle import mps as M
from test_gpu_big_svd import BARS, _assert_rest_untouched

pytestmark = pytest.mark.gpu

JACOBI_BARS = dict(BARS, sig=1e-12)  # where the Jacobi answers: no Gram squaring in the Schmidt values
ZERO = {"calls": 0, "taken": 0, "declined_shape": 0, "declined_floor": 0, "certificates": 0, "certified": 0}
STATS = {
    "jacobi": ZERO,
    "shape": dict(ZERO, calls=1, declined_shape=1),
    "floor": dict(ZERO, calls=1, declined_floor=1),
    "gram": dict(ZERO, calls=1, taken=1),
    "certified": dict(ZERO, calls=1, taken=1, certificates=1, certified=1),
}


class _Switches:
    """A route's aqc_mps_set_fused_chain / aqc_mps_set_svd_path, restored to the defaults on exit."""

    def __init__(self, route):
        self.spec = S.ROUTES[route]

    def __enter__(self):
        from adaptaqc_amd import _lib

        L = _lib.lib()
        _lib.check(L.aqc_mps_set_fused_chain(self.spec["fused"]))
        _lib.check(L.aqc_mps_set_svd_path(self.spec["gram"], 64))

    def __exit__(self, *exc):
        from adaptaqc_amd import _lib

        L = _lib.lib()
        _lib.check(L.aqc_mps_set_fused_chain(1))
        _lib.check(L.aqc_mps_set_svd_path(1, 64))


def _run(case, reverse=False):
    """The case's one update on the device: (state read back, gram_stats of the update)."""
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import DeviceMPS

    route, shape, kind, max_chi = case
    b = S.built(*S.case_input(case))
    p = b["p"]
    op = (S.reversed_matrix(b["gate"]), (p + 1, p)) if reverse else (b["gate"], (p, p + 1))
    with _Switches(route):
        d = DeviceMPS(b["n"], S.case_cap(route, shape), R.case_thr(kind), max_chi)
        d.load_aer(b["aer"])
        _lib.gram_stats()
        d.apply([op])
        st = _lib.gram_stats()
        after = d.to_aer()
        d.close()
    return after, st


_LOCKSTEP_THETA = {}


def _lockstep_theta(case):
    """theta read back after the L128 run of the case's input and cut (kept for its F128 twin)."""
    key = case[1:]
    if key not in _LOCKSTEP_THETA:
        after, _ = _run(("L128",) + key)
        _LOCKSTEP_THETA[key] = M.MPS.from_aer(after).theta_matrix(S.built(*S.case_input(case))["p"])
    return _LOCKSTEP_THETA[key]


def _check(case, after, st, label):
    """The assertions of one update: K, the rest of the state, the route, the bars."""
    route, shape, kind, max_chi = case
    b = S.built(*S.case_input(case))
    p = b["p"]
    K = S.kept(b, kind, max_chi)
    path = S.expected_path(case, b["sigma"], K)
    k_dev = len(after[1][p])
    got = R.metrics(b["theta"], K, after, p, b["svd"]) if k_dev == K else None
    print(f"{label}: K = {k_dev} (want {K}) class {S.svd_class(route, shape)} path {path} {st}", flush=True)
    if got:
        print(f"{label}: " + " ".join(f"{k}={got[k]:.2e}" for k in S.KEYS), flush=True)
    assert k_dev == K
    _assert_rest_untouched(b["aer"], after, p)
    if st is not None:
        assert st == STATS[path], (path, st)
    bars = BARS if path in ("gram", "certified") else JACOBI_BARS
    missed = {k: got[k] for k in S.KEYS if not got[k] <= bars[k]}
    assert not missed, (missed, got)
    return path


@pytest.mark.parametrize("case", S.CASES, ids=[S.case_id(c) for c in S.CASES])
def test_one_update_against_lapack(case):
    """One gate on one state per case of small_svd_ref.CASES: K, the untouched rest, the route by
    gram_stats, the bars."""
    after, st = _run(case)
    p = S.built(*S.case_input(case))["p"]
    if case[0] == "L128":
        _LOCKSTEP_THETA[case[1:]] = M.MPS.from_aer(after).theta_matrix(p)
    path = _check(case, after, st, S.case_id(case))
    if case[0] == "F128":
        # the fused chain against the lock-step launches on the same input: the same K (both checked
        # against truncation_rank's above) and the same theta, to the accuracy that
        # test_fused_chain_matches_lockstep_and_oracle documents
        diff = np.linalg.norm(M.MPS.from_aer(after).theta_matrix(p) - _lockstep_theta(case))
        print(f"{S.case_id(case)}: |theta_F128 - theta_L128| = {diff:.2e}", flush=True)
        assert diff <= (1e-9 if path == "certified" else 1e-12)


REVERSED = [("L128", (128, 128), "pairs", 64), ("J32", (32, 32), "clusters", 16)]


@pytest.mark.parametrize("case", REVERSED, ids=[S.case_id(c) for c in REVERSED])
def test_gate_named_from_the_right_qubit(case):
    """The same gate as (matrix', (p + 1, p)), the matrix conjugated by SWAP: same K, same bars."""
    assert case in S.CASES
    after, st = _run(case, reverse=True)
    _check(case, after, st, S.case_id(case) + "-reversed")


THETA32 = ("L128", (128, 128), "clusters", 64)


def test_theta32_batch_of_64():
    """k_theta32 launches only when a wave has 256 tiles of 32 x 32, 64 jobs at capacity 64: 64 copies of
    one L128 input in one apply_batch with the fused chain off.  The first and the last state are under
    the bars and all 64 are bit-identical."""
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import DeviceMPS, apply_batch

    case = THETA32
    assert case in S.CASES
    route, shape, kind, max_chi = case
    b = S.built(*S.case_input(case))
    ns, cap = 64, S.case_cap(route, shape)
    assert ((cap + 31) // 32) ** 2 * ns >= 256 > ((cap + 31) // 32) ** 2 * (ns - 1)
    with _Switches(route):
        states = [DeviceMPS(b["n"], cap, R.case_thr(kind), max_chi) for _ in range(ns)]
        for d in states:
            d.load_aer(b["aer"])
        _lib.gram_stats()
        apply_batch(states, [[(b["gate"], (b["p"], b["p"] + 1))]] * ns)
        st = _lib.gram_stats()
        out = [d.to_aer() for d in states]
        for d in states:
            d.close()
    assert st == {k: ns * v for k, v in STATS["gram"].items()}, st
    _check(case, out[0], None, "theta32-first")
    _check(case, out[-1], None, "theta32-last")
    for o in out[1:]:
        for (a0, a1), (b0, b1) in zip(out[0][0], o[0]):
            np.testing.assert_array_equal(a0, b0)
            np.testing.assert_array_equal(a1, b1)
        for x, y in zip(out[0][1], o[1]):
            np.testing.assert_array_equal(x, y)


# bonds 0 .. 18 of the mixed wave's state: the pairs (4, 5), (7, 8), (10, 11) have outer bonds (16, 16),
# (32, 32), (64, 64): sides 32, 64 and 128
MIXED_DIMS = [1, 2, 4, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 32, 16, 8, 4, 2, 1]
MIXED_PAIRS = [(4, 5), (7, 8), (10, 11)]


def test_mixed_small_class_wave_equals_sequential():
    """A capacity-128 state takes its kernel class from each job's own side, so one wave with sides 32,
    64 and 128 (k_jacobi_reg<32>, <64> and k_svd_gram) equals the same three gates applied one call at
    a time, bit for bit -- test_mixed_class_wave_equals_sequential's counterpart below 2 chi = 128."""
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import DeviceMPS

    n, cap, dims = 18, 128, MIXED_DIMS
    rng = np.random.default_rng(18)
    aer = vidal_from_tensors([rng.standard_normal((2, dims[i], dims[i + 1])) + 1j * rng.standard_normal((2, dims[i], dims[i + 1]))
                              for i in range(n)])
    assert [len(x) for x in aer[1]] == dims[1:-1]
    assert [2 * max(dims[a], dims[a + 2]) for a, _ in MIXED_PAIRS] == [32, 64, 128]
    ops = [(S.matrix_of_op4(R.OP4), pr) for pr in MIXED_PAIRS]
    one = DeviceMPS(n, cap, 1e-16, cap)
    one.load_aer(aer)
    _lib.gram_stats()
    one.apply(ops)
    st = _lib.gram_stats()
    assert st["calls"] == 1 and st["declined_shape"] == 0, st  # (the side-128 job alone)
    seq = DeviceMPS(n, cap, 1e-16, cap)
    seq.load_aer(aer)
    for op in ops:
        seq.apply([op])
    np.testing.assert_array_equal(one.dims(), seq.dims())
    got = [int(one.dims()[a + 1]) for a, _ in MIXED_PAIRS]
    assert got[:2] == [32, 64] and 64 < got[2] <= 128, got  # (2 chi; CHOP may take a few of the 128: the wide S5 / S6)
    (g1, l1), (g2, l2) = one.to_aer(), seq.to_aer()
    for (a0, a1), (b0, b1) in zip(g1, g2):
        np.testing.assert_array_equal(a0, b0)
        np.testing.assert_array_equal(a1, b1)
    for x, y in zip(l1, l2):
        np.testing.assert_array_equal(x, y)
