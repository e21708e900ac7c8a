"""numpy inputs and references (complex128, LAPACK, no device code) for one small two-site update,
2 chi <= 128 (mps.hip: k_theta / k_theta32, k_svd_gram / k_jacobi_reg, k_rank, k_split_*, and the
fused k_chain; svd_gram.h), and the one table of cases that the host test
(test_small_svd_ref_host.py) and the device test (test_gpu_small_svd.py) share.  The spectra, the
state builder and the metrics are big_svd_ref's, imported.

Gates are handed to the device as 4 x 4 matrices, so the gate of an input need not be a named one.
Two families of inputs:

  gen  generic: T = U diag(sigma) V^H with Haar U, V, reached through cx (big_svd_ref.state_with_theta
       as it is).  theta' has rank <= 2 x the middle bond, so a full-rank T needs a middle bond of
       min(2 chi_l, 2 chi_r): these run on states of capacity 128 (or 100), where mps.hip takes the
       kernel class from the job's own side, and at the chain's ends.
  lim  capacity-limited, the headline regime (capacity 64, every bond <= 64, theta' 128 x 128 of full
       rank, max_chi cutting it): T_block is non-zero in the s1 = s2 blocks only, T[0, :, 0, :] =
       E diag(sigma_a) Z^H and T[1, :, 1, :] = F diag(sigma_b) Z^H with isometries E, F (chi_l x m), Z
       (chi_r x m), m = min(chi_l, chi_r), and sigma_a, sigma_b the even and odd members of the
       prescribed 2 m values (near-equal neighbours land in different blocks).  T' = (A (x) B) T_block
       with Haar 2 x 2 unitaries A on s1 and B on s2 is dense, and the gate is G = (A (x) B) cx as one
       matrix: G^H T' = cx T_block has both blocks in the s2 = 0 columns, rank m.  So every bond of the
       input is <= max(chi_l, chi_r) and theta' has the prescribed 2 m singular values.
       `rank10` (exact zeros, where the Gram path's certificate runs) is a generic T of rank 10 under
       the product gate A (x) B, which preserves the rank.

theta' is (2 chi_l) x (2 chi_r), rows (s1, l), columns (s2, r), as oracle.mps.MPS.theta_matrix."""
import numpy as np

import big_svd_ref as R
from oracle import gates as G
from oracle import mps as M

KEYS = R.KEYS
SWAP = np.asarray(G.SWAP, dtype=complex).reshape(4, 4)


# ---- gates as matrices ---------------------------------------------------------------------------
def op4_of_matrix(m):
    """op4[s1', s2', s1, s2] (s1 the left site) of a 4 x 4 gate applied as (m, (p, p + 1)): the matrix is
    little-endian over its qubits, [b1', b0', b1, b0] with b0 the first one (oracle.mps.MPS.apply_2q)."""
    return np.asarray(m, dtype=complex).reshape(2, 2, 2, 2).transpose(1, 0, 3, 2)


def matrix_of_op4(op4):
    """The 4 x 4 matrix that (matrix, (p, p + 1)) hands to the device for op4 -- op4_of_matrix's inverse."""
    return np.ascontiguousarray(np.asarray(op4, dtype=complex).transpose(1, 0, 3, 2).reshape(4, 4))


def reversed_matrix(m):
    """The matrix of the same gate applied as (matrix', (p + 1, p)): conjugated by SWAP."""
    return SWAP @ np.asarray(m, dtype=complex) @ SWAP


def product_op4(a, b):
    """A on the left site, B on the right one."""
    return np.einsum("ca,db->cdab", a, b)


def dressed_cx_op4(a, b):
    """(A (x) B) cx, the control on the left site."""
    return np.einsum("ce,df,efab->cdab", a, b, R.OP4)


# ---- spectra for any length ----------------------------------------------------------------------
MIN_LENGTH = {"clusters": 17, "plateau": 17, "threshold": R.THRESHOLD_DROPPED + 1, "rank10": 11}
ALL_KINDS = R.ALL_KINDS


def pair_gaps(r):
    """The (position, gap) entries of big_svd_ref.PAIR_GAPS that a run of r values admits: the position
    exists, and the gap is below half of the geometric run's own gap there (so the pair stays a pair
    and the run stays strictly decreasing)."""
    lam = np.geomspace(1.0, 1e-6, r)
    return tuple((pos, g) for pos, g in R.PAIR_GAPS if pos + 1 < r and g < 0.5 * (lam[pos] - lam[pos + 1]))


def _pairs(r):
    lam = np.geomspace(1.0, 1e-6, r)  # sigma^2 / sigma_1^2, as big_svd_ref._pairs
    for pos, g in pair_gaps(r):
        lam[pos + 1] = lam[pos] - g
    assert np.all(np.diff(lam) < 0)
    s = np.sqrt(lam)
    return s / np.linalg.norm(s)


def spectrum(kind, r):
    """The kind's r singular values (unit norm, descending), or None where the kind is undefined."""
    if r < MIN_LENGTH.get(kind, 2):
        return None
    if kind == "pairs":
        return _pairs(r) if pair_gaps(r) else None
    return R.SPECTRA[kind](r)


# ---- the inputs ----------------------------------------------------------------------------------
def _sites(shape):
    """(n, a): sites left of the pair a with 2^a >= chi_l, as many right of it as chi_r needs."""
    chl, chr_ = shape[0] // 2, shape[1] // 2
    a, b = int(np.ceil(np.log2(chl))), int(np.ceil(np.log2(chr_)))
    return a + 2 + b, a


def limited_matrix(shape, sigma, rng):
    """(T', op4) of the capacity-limited family (module docstring); sigma: 2 min(chi_l, chi_r) values."""
    chl, chr_ = shape[0] // 2, shape[1] // 2
    m = min(chl, chr_)
    assert len(sigma) == 2 * m
    e, f, z = R._isometry(rng, chl, m), R._isometry(rng, chl, m), R._isometry(rng, chr_, m)
    a, b = R._isometry(rng, 2, 2), R._isometry(rng, 2, 2)
    blk = np.zeros((2, chl, 2, chr_), dtype=complex)
    blk[0, :, 0, :] = (e * sigma[0::2][None, :]) @ z.conj().T
    blk[1, :, 1, :] = (f * sigma[1::2][None, :]) @ z.conj().T
    t = np.einsum("ca,db,aibj->cidj", a, b, blk).reshape(shape)
    return t, dressed_cx_op4(a, b)


_BUILT = {}


def built(fam, shape, kind):
    """The input of a (family, shape, kind), computed once; callers do not modify it.  dict: n, p (the
    left site of the pair), aer (the input state), op4 and gate (the 4 x 4 matrix for (p, p + 1)), sigma
    (the prescribed spectrum), theta (theta' of the input state, unit norm), svd (its LAPACK SVD)."""
    key = (fam, shape, kind)
    if key not in _BUILT:
        n, a = _sites(shape)
        rng = np.random.default_rng([fam == "lim", shape[0], shape[1], ALL_KINDS.index(kind)])
        sigma = spectrum(kind, min(shape))
        if fam == "gen":
            T, op4 = R.matrix_with_spectrum(shape[0], shape[1], sigma, rng), R.OP4
        elif kind == "rank10":
            T = R.matrix_with_spectrum(shape[0], shape[1], sigma, rng)
            op4 = product_op4(R._isometry(rng, 2, 2), R._isometry(rng, 2, 2))
        else:
            T, op4 = limited_matrix(shape, sigma, rng)
        aer = R.state_with_theta(T, a, n - 2 - a, op4, rng)
        theta = M.MPS.from_aer(aer).theta_matrix(a, op4)
        _BUILT[key] = dict(n=n, p=a, aer=aer, op4=op4, gate=matrix_of_op4(op4), sigma=sigma, theta=theta,
                           svd=np.linalg.svd(theta, full_matrices=False))
    return _BUILT[key]


def kept(b, kind, max_chi):
    """truncation_rank's K of a built input at the case's threshold and cap."""
    return M.truncation_rank(b["svd"][1], R.case_thr(kind), max_chi)


# ---- the table -----------------------------------------------------------------------------------
GRAM_FLOOR = 1e-9  # kGramRelFloor (svd_gram.h): lambda_K > 1e-9 lambda_1 or the Gram path declines
# A cut that drops values is admitted only with a gap at K, (sigma_K^2 - sigma_K+1^2) / sigma_1^2 >=
# 5e-6 as in test_big_svd_ref_host.py, and not between the two members of a `pairs` pair (gaps up to
# 1e-5): the rank-K part of theta' moves by eps sigma_1^2 / (sigma_K^2 - sigma_K+1^2) for every method,
# so there not even numpy's Gram form stays a tenth under the bars (the host test measures it on every
# case).  It keeps cuts out of `plateau` and out of the first two `clusters` groups.
CUT_GAP = 5e-6

# route -> (capacity, input family, fused chain, Gram path); fused 1 / gram 1 are the defaults
ROUTES = {
    "L128": dict(cap=64, fam="lim", fused=0, gram=1),
    "F128": dict(cap=64, fam="lim", fused=2, gram=1),
    "J128": dict(cap=64, fam="lim", fused=0, gram=0),
    "J64": dict(cap=32, fam="lim", fused=1, gram=1),
    "J32": dict(cap=16, fam="lim", fused=1, gram=1),
    "W128": dict(cap=128, fam="gen", fused=1, gram=1),
}
SHAPES = {
    "L128": ((128, 128), (128, 72), (72, 128), (100, 100), (128, 40)),
    "J64": ((64, 64), (64, 24), (40, 40)),
    "J32": ((32, 32), (32, 12), (8, 8)),
    "W128": ((128, 128), (128, 72), (72, 128), (100, 100), (128, 40), (64, 64), (32, 32)),
}
SHAPES["F128"] = SHAPES["J128"] = SHAPES["L128"]
ENDS = ((2, 4), (4, 2), (2, 2))  # p = 0, p = n - 2, and both on a two-qubit state; generic inputs
END_ROUTES = ("L128", "F128", "J32")


def case_cap(route, shape):
    return 100 if route == "W128" and shape == (100, 100) else ROUTES[route]["cap"]


def case_fam(route, shape):
    return "gen" if shape in ENDS else ROUTES[route]["fam"]


def cut_admitted(sigma, kind, max_chi, cap):
    """K if the cut keeps K <= cap values with a gap below them (or keeps them all), else None."""
    k = M.truncation_rank(sigma, R.case_thr(kind), max_chi)
    if max_chi is not None and k != max_chi:
        return None
    if k > cap:
        return None
    if k < len(sigma) and (sigma[k - 1] ** 2 - sigma[k] ** 2) / sigma[0] ** 2 < CUT_GAP:
        return None
    if kind == "pairs" and any(pos == k - 1 for pos, _ in pair_gaps(len(sigma))):
        return None
    return k


def _cases():
    """(route, shape, kind, max_chi)."""
    out = []
    for route, spec in ROUTES.items():
        shapes = SHAPES[route] + (ENDS if route in END_ROUTES else ())
        for shape in shapes:
            c, cap, fam = min(shape), case_cap(route, shape), case_fam(route, shape)
            kinds = ("decay",) if shape in ENDS else ALL_KINDS
            for kind in kinds:
                sigma = spectrum(kind, c)
                if sigma is None:
                    continue
                cuts = [None, c // 2, c // 2 + 5] + ([cap] if fam == "lim" else [])
                seen = set()
                for max_chi in cuts:
                    if max_chi is not None and not 1 <= max_chi < c:
                        continue
                    if max_chi in seen or cut_admitted(sigma, kind, max_chi, cap) is None:
                        continue
                    seen.add(max_chi)
                    out.append((route, shape, kind, max_chi))
    return out


CASES = _cases()


def case_id(case):
    route, shape, kind, max_chi = case
    return f"{route}-{shape[0]}x{shape[1]}-{kind}-K{max_chi if max_chi else 'all'}"


def case_input(case):
    route, shape, kind, _ = case
    return case_fam(route, shape), shape, kind


def svd_class(route, shape):
    """The kernel class mps.hip gives the job: 2 x the capacity up to capacity 64, the job's own side above."""
    cap = case_cap(route, shape)
    if 2 * cap <= 128:
        return 2 * cap
    side = max(shape)
    return 32 if side <= 32 else 64 if side <= 64 else 128


def expected_path(case, sigma, K):
    """What answers the case's SVD, from svd_gram.h's own rules: 'jacobi' (k_jacobi_reg launched, no
    Gram call), 'shape' (the Gram path declines C < 4 and the Jacobi behind it runs), 'floor' (it
    declines lambda_K <= 1e-9 lambda_1), 'certified' (exact zeros: taken under the certificate) or
    'gram'."""
    route, shape, kind, _ = case
    if ROUTES[route]["gram"] == 0 or svd_class(route, shape) < 128:
        return "jacobi"
    if min(shape) < 4:
        return "shape"
    if (sigma[K - 1] / sigma[0]) ** 2 <= GRAM_FLOOR:
        return "floor"
    return "certified" if kind == "rank10" else "gram"
