"""numpy references (complex128, LAPACK, no device code) for one large two-site update, 2 chi > 128
(gram_big.hip, bjacobi.hip), and the one table of inputs that the host test
(test_big_svd_ref_host.py) and the device test (test_gpu_big_svd.py) share.

``state_with_theta`` builds an MPS whose two-site matrix after one cx is a prescribed matrix T, so
that a single update is handed a chosen spectrum and shape; ``metrics`` measures the decomposition
the device read back against the LAPACK SVD of the same matrix, linearly in the error;
``gram_form_reference`` gives the same numbers for numpy's own Gram form (eigh(X^H X), V, X V), the
best the Gram path can do.

theta' is (2 chi_l) x (2 chi_r), rows (s1, l), columns (s2, r), as oracle.mps.MPS.theta_matrix."""
import numpy as np

from bench import vidal_from_tensors
from oracle import gates as G
from oracle import mps as M

# cx(a, a + 1) as oracle.mps.MPS.apply_2q hands it to the two-site update (control on the left site)
OP4 = G.CX.reshape(2, 2, 2, 2).transpose(1, 0, 3, 2)
RANK_TOL = 1e-13  # numerical rank of the centre split, relative to its largest singular value


# ---- spectra -----------------------------------------------------------------------------------
def _unit(s):
    s = np.asarray(s, dtype=float)
    return s / np.linalg.norm(s)


def _decay(C):
    return _unit(np.geomspace(1.0, 1e-3, C))


def _clusters(C):
    return _unit(np.concatenate([np.ones(8), 0.5 * np.ones(8), np.geomspace(0.25, 1e-3, C - 16)]))


PAIR_GAPS = ((4, 5e-8), (10, 5e-8), (20, 3e-7), (30, 3e-7), (40, 1e-5), (50, 1e-5))  # (position, g)


def _pairs(C):
    lam = np.geomspace(1.0, 1e-6, C)  # sigma^2 / sigma_1^2
    for pos, g in PAIR_GAPS:
        lam[pos + 1] = lam[pos] - g
    assert np.all(np.diff(lam) < 0)
    return _unit(np.sqrt(lam))


def _plateau(C):
    return _unit(np.concatenate([0.8 ** np.arange(16), 1e-4 * np.ones(C - 16)]))


def _rank10(C):
    return _unit(np.concatenate([0.7 ** np.arange(10), np.zeros(C - 10)]))


def _below_floor(C):
    return _unit(np.geomspace(1.0, 1e-6, C))


THRESHOLD = 1e-8


def threshold_margin(s, thr):
    """(K, margin) of truncation_rank's tail rule on s: margin = the smallest |sum - thr| / thr over
    the comparison that stops the rule (tail + s_K^2 >= thr) and the last one that dropped a value."""
    k = M.truncation_rank(s, thr, None)
    tail = float(np.sum(s[k:] ** 2))
    return k, min(abs(tail + s[k - 1] ** 2 - thr), abs(tail - thr)) / thr


THRESHOLD_DROPPED = 24


def _threshold(C):
    """Two geometric runs: C - 24 values with sigma down to 1e-2 sigma_1, then 24 values whose sigma^2
    fall by a factor 30 and add up to 0.6 thr, so the tail rule at thr = 1e-8 drops exactly those (the
    last dropping comparison is clear by 0.4 thr, the stopping one by far) and the kept count is
    decided by the accumulated tail alone, not by CHOP or a cap.  The dropped sigma^2 lie around the
    Gram path's 1e-9 sigma_1^2 floor, which only kept values have to clear.  (One geometric run cannot
    serve: where its tail sum crosses 1e-8 its neighbouring sigma^2 differ by ~1e-9 sigma_1^2, and the
    rank-K part of theta' is then ill-conditioned for every method.)"""
    head = np.geomspace(1.0, 1e-2, C - THRESHOLD_DROPPED)
    tail2 = np.geomspace(1.0, 1.0 / 30.0, THRESHOLD_DROPPED)
    tail2 *= 0.6 * THRESHOLD * np.sum(head ** 2) / np.sum(tail2)
    return _unit(np.concatenate([head, np.sqrt(tail2)]))


SPECTRA = {
    "decay": _decay,
    "clusters": _clusters,
    "pairs": _pairs,
    "plateau": _plateau,
    "rank10": _rank10,
    "below_floor": _below_floor,
    "threshold": _threshold,
}


# ---- the input state ---------------------------------------------------------------------------
def _cnormal(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _isometry(rng, rows, cols):
    """rows x cols with orthonormal columns (rows >= cols)."""
    q, _ = np.linalg.qr(_cnormal(rng, (rows, cols)))
    return q


def matrix_with_spectrum(m, n, sigma, rng):
    """A random m x n matrix with singular values sigma (min(m, n) of them)."""
    c = min(m, n)
    assert len(sigma) == c
    return (_isometry(rng, m, c) * np.asarray(sigma)[None, :]) @ _isometry(rng, n, c).conj().T


def state_with_theta(T, a, b, op4, rng):
    """An Aer-format MPS on a + 2 + b qubits whose two-site matrix at sites (a, a + 1) after op4 is T,
    up to unitary gauges on the two outer bonds (they act on l and r alone, so the singular values
    are T's and the singular vectors T's in another basis).  Left of the pair random left-isometric
    tensors with bonds min(2^k, chi_l), right of it their mirror image, the centre theta = op4^H T
    split by an exact SVD at its numerical rank; then bench.vidal_from_tensors.

    A rank-deficient T (`rank10`) has no canonical form with these outer bonds: a state of Schmidt
    rank k across the middle has at most 2 k non-zero Schmidt values on the bonds beside it, and
    vidal_from_tensors would divide by the rest.  Its input keeps the outer sites and outer lambdas
    of a full-rank companion (the same shape with the `decay` spectrum) and takes only the middle from
    T: Gamma_a = U / lam_l, lam_a = S, Gamma_a+1 = V^H / lam_r of theta = U S V^H at its numerical rank,
    so that lam_l Gamma_a lam_a Gamma_a+1 lam_r is theta itself.  The update reads nothing else (as
    test_gram_big_rank_deficient_certified, which zeroes a middle bond of a canonical state)."""
    T = np.asarray(T, dtype=complex)
    chl, chr_ = T.shape[0] // 2, T.shape[1] // 2
    assert 2 ** a >= chl and 2 ** b >= chr_
    theta = np.einsum("cdab,cidj->aibj", np.conj(op4), T.reshape(2, chl, 2, chr_)).reshape(2 * chl, 2 * chr_)
    u, s, vh = np.linalg.svd(theta, full_matrices=False)
    k = int(np.sum(s > RANK_TOL * s[0]))
    if k < len(s):
        full = matrix_with_spectrum(T.shape[0], T.shape[1], _decay(min(T.shape)), rng)
        gam, lam = state_with_theta(full, a, b, op4, rng)
        ga = u[:, :k].reshape(2, chl, k) / lam[a - 1][None, :, None]
        gb = vh[:k].reshape(k, 2, chr_).transpose(1, 0, 2) / lam[a + 1][None, None, :]
        gam[a] = (ga[0].copy(), ga[1].copy())
        gam[a + 1] = (gb[0].copy(), gb[1].copy())
        lam[a] = s[:k] / np.linalg.norm(s[:k])
        return gam, lam
    A = []
    for k_ in range(a):
        l, r = min(2 ** k_, chl), min(2 ** (k_ + 1), chl)
        A.append(_isometry(rng, 2 * l, r).reshape(l, 2, r).transpose(1, 0, 2))
    A.append(u[:, :k].reshape(2, chl, k))
    A.append((s[:k, None] * vh[:k]).reshape(k, 2, chr_).transpose(1, 0, 2))
    for j in range(b):
        l, r = min(2 ** (b - j), chr_), min(2 ** (b - j - 1), chr_)
        A.append(_isometry(rng, 2 * r, l).conj().T.reshape(l, 2, r).transpose(1, 0, 2))
    gam, lam = vidal_from_tensors(A)
    assert all(np.all(x > 0.0) for x in lam), "a zero Schmidt value entered the Vidal form"
    return gam, lam


# ---- the four numbers --------------------------------------------------------------------------
KEYS = ("sig", "sig_w", "theta", "iso_direct", "iso_derived")


def _numbers(theta_prime, svd, K, left, lam, right, theta_dev=None, jacobi=False):
    """left (2 chi_l x K), lam (K), right (K x 2 chi_r): a rank-K factorisation of theta' with the
    kept values renormalised, against the LAPACK svd = (u, s, vh) of theta'.  jacobi: the one-sided
    Jacobi made it (its direct side is the other one, see metrics)."""
    u, s, vh = svd
    want = s[:K] / np.linalg.norm(s[:K])
    assert lam.shape == want.shape
    dl = np.abs(lam - want)
    if theta_dev is None:
        theta_dev = (left * lam[None, :]) @ right
    ref = (u[:, :K] * want[None, :]) @ vh[:K]
    el = left.conj().T @ left - np.eye(K)
    er = right @ right.conj().T - np.eye(K)
    direct_right = theta_prime.shape[0] >= theta_prime.shape[1]  # G = X^H X on the shorter side
    if jacobi:
        direct_right = not direct_right
    eg, ed = (er, el) if direct_right else (el, er)
    return {
        "sig": float(np.max(dl)),
        "sig_w": float(np.max(dl * s[:K] / s[0])),
        "theta": float(np.linalg.norm(theta_dev - ref)),
        "iso_direct": float(np.max(np.abs(eg))),
        "iso_derived": float(np.max(np.abs(lam[:, None] * ed * lam[None, :])) / want[0] ** 2),
    }


def metrics(theta_prime, K, after_state, p, svd=None, jacobi=False):
    """The device's read-back after the gate (Aer format) against the LAPACK SVD of theta' (unit norm):
    sig          (a) max |lam'_i - sigma_i / ||sigma_:K|||
    sig_w        (a) weighted by sigma_i / sigma_1: the error in sigma^2
    theta        (b) ||theta_dev - U_K Sigma_K V_K^H / ||sigma_:K|| ||_F with theta_dev = lam_l Gamma_p lam'
                 Gamma_p+1 lam_r read back: gauge-free and linear in the error (unique while
                 sigma_K > sigma_K+1)
    iso_direct   (c) max |A^H A - I| of the site matrix (outer bond weighted by its lambda) on the side
                 the method orthogonalises itself.  The Gram path: the eigenvectors of G = X^H X, on the
                 shorter side of theta', the right one when they are equal.  jacobi = True (the block
                 Jacobi answered): it rotates the columns of X = theta' or theta'^H, which span the longer
                 side, the left one when they are equal -- the opposite side.
    iso_derived  (d) max |Lam' (A^H A - I) Lam'| / lam'_1^2 on the other side, which both methods derive
                 by a product and a division by sigma (X V / sigma; X^H U / sigma): the error there grows
                 as eps sigma_1^2 / (sigma_i sigma_j) resp. eps sigma_1 / sigma_j, so only the weighted
                 form is small
    svd: the LAPACK SVD of theta' where the caller has it already."""
    theta_prime = np.asarray(theta_prime)
    if svd is None:
        svd = np.linalg.svd(theta_prime, full_matrices=False)
    m = M.MPS.from_aer(after_state)
    ll = m.l[p - 1] if p > 0 else np.ones(1)
    lr = m.l[p + 1] if p + 1 < m.n - 1 else np.ones(1)
    left = (m.g[p] * ll[None, :, None]).reshape(theta_prime.shape[0], -1)
    right = (m.g[p + 1] * lr[None, None, :]).transpose(1, 0, 2).reshape(-1, theta_prime.shape[1])
    return _numbers(theta_prime, svd, K, left, m.l[p], right, m.theta_matrix(p), jacobi)


def gram_form_reference(theta_prime, K, svd=None):
    """The same numbers for numpy's Gram form of theta': X = theta' or theta'^H (the longer side down),
    eigh(X^H X), the top K eigenvectors V, X V and its column norms."""
    theta_prime = np.asarray(theta_prime)
    if svd is None:
        svd = np.linalg.svd(theta_prime, full_matrices=False)
    tr = theta_prime.shape[0] < theta_prime.shape[1]
    x = theta_prime.conj().T if tr else theta_prime
    _, v = np.linalg.eigh(x.conj().T @ x)
    v = v[:, ::-1][:, :K]
    w = x @ v
    sig = np.linalg.norm(w, axis=0)
    uc = w / sig[None, :]
    lam = sig / np.linalg.norm(sig)
    left, right = (v, uc.conj().T) if tr else (uc, v.conj().T)  # theta' = X^H = V Sigma Uc^H when tr
    return _numbers(theta_prime, svd, K, left, lam, right)


# ---- the shared inputs -------------------------------------------------------------------------
# shape (2 chi_l, 2 chi_r) -> (class CT of big_svd, qubits n, sites left of the pair a)
SHAPES = {
    (256, 256): (256, 16, 7),
    (256, 136): (256, 16, 7),
    (136, 256): (256, 16, 7),
    (200, 200): (256, 16, 7),
    (264, 264): (512, 18, 8),
    (512, 320): (512, 18, 8),
    (400, 400): (512, 18, 8),
    (520, 1024): (1024, 20, 9),
    (1040, 520): (1024, 21, 10),  # L = 1040 > CT: the long layout
}
ALL_KINDS = ("decay", "clusters", "pairs", "plateau", "rank10", "below_floor", "threshold")


def _cases():
    """(shape, kind, max_chi, mode): mode None, or the (512, 320) switch (setter name, value)."""
    out = []
    for shape, (ct, _, _) in SHAPES.items():
        c = min(shape)
        if ct == 256:
            for kind in ALL_KINDS:
                out.append((shape, kind, None, None))
            for kind in ("decay", "clusters", "pairs"):
                out.append((shape, kind, c // 2, None))
                out.append((shape, kind, c // 2 + 5, None))
        elif ct == 512:
            modes = [None]
            if shape == (512, 320):
                modes = [("aqc_gb_set_stages", 1), ("aqc_gb_set_stages", 2), ("aqc_gb_set_tail", 0), ("aqc_gb_set_tail", 1)]
            for kind in ("decay", "clusters", "pairs", "plateau", "rank10"):
                for mode in modes:
                    out.append((shape, kind, None, mode))
            out.append((shape, "clusters", c // 2, None))
            if shape == (264, 264):
                out.append((shape, "below_floor", None, None))
    out.append(((520, 1024), "clusters", None, None))
    out.append(((1040, 520), "decay", 260, None))
    return out


CASES = _cases()


def case_id(case):
    shape, kind, max_chi, mode = case
    s = f"{shape[0]}x{shape[1]}-{kind}-K{max_chi if max_chi else 'all'}"
    return s + (f"-{mode[0][11:]}{mode[1]}" if mode else "")


def case_thr(kind):
    return THRESHOLD if kind == "threshold" else 1e-16


_BUILT = {}


def built(shape, kind):
    """The input of a (shape, kind), computed once; callers do not modify it.  dict: n, p (the left
    site of the pair), aer (the input state), sigma (the prescribed spectrum), theta (theta' of the input
    state, unit norm), svd (its LAPACK SVD)."""
    key = (shape, kind)
    if key not in _BUILT:
        ct, n, a = SHAPES[shape]
        seed = [ct, shape[0], shape[1], ALL_KINDS.index(kind)]
        rng = np.random.default_rng(seed)
        sigma = SPECTRA[kind](min(shape))
        T = matrix_with_spectrum(shape[0], shape[1], sigma, rng)
        aer = state_with_theta(T, a, n - 2 - a, OP4, rng)
        theta = M.MPS.from_aer(aer).theta_matrix(a, OP4)
        _BUILT[key] = dict(n=n, p=a, aer=aer, sigma=sigma, theta=theta, svd=np.linalg.svd(theta, full_matrices=False))
    return _BUILT[key]


def kept(b, kind, max_chi):
    """truncation_rank's K of a built input at the case's threshold and cap."""
    return M.truncation_rank(b["svd"][1], case_thr(kind), max_chi)
