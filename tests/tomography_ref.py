"""numpy restatements of the pair-tomography routines (adaptaqc_amd/csrc/tomo.hip), for the
tomography tests.

Conventions (include/aqc_hip.h): pair (a, b) as hi = max, lo = min; RDM index 2 bit_hi + bit_lo
(= np.kron(hi, lo)); basis codes 0 X, 1 Y, 2 Z; setting s = 3 b_hi + b_lo; outcome o = 2 o_hi +
o_lo with 0 the +1 eigenstate.
"""
import numpy as np

from sampling_ref import uniforms

_R = 1 / np.sqrt(2)
PAULI = [np.eye(2, dtype=complex), np.array([[0, 1], [1, 0]], dtype=complex),
         np.array([[0, -1j], [1j, 0]]), np.diag([1.0 + 0j, -1.0])]  # I, X, Y, Z


# The end-to-end states of the tomography tests, as oracle ops [(name, qubits, params)], with the
# shots and seed they are drawn with (test_tomography_host.py checks on the CPU that the
# restatement chain stays inside the tests' statistical margins for exactly these).
SHOTS = 8192
SEED = 5
MARGIN = 10 / np.sqrt(SHOTS)


def _brickwork4():
    from sampling_ref import brickwork

    return brickwork(4, 4, 21)


STATES = {
    "bell_in_3": (3, [("h", (0,), ()), ("cx", (0, 2), ()), ("ry", (1,), (0.4,))]),
    "ghz4": (4, [("h", (0,), ())] + [("cx", (q, q + 1), ()) for q in range(3)]),
    "product": (3, [("ry", (0,), (0.7,)), ("rx", (1,), (1.9,)), ("h", (2,), ()), ("rz", (2,), (0.3,))]),
    "brickwork4": (4, _brickwork4()),
}


def exact_measure(method, rho):
    """oracle.entanglement.measure, with the entanglement of formation of an unentangled state as 0:
    there the oracle's concurrence is a rounding residue, x = (1 + sqrt(1 - C^2)) / 2 rounds to 1 and
    its formula evaluates 0 log 0 (nan); the limit is 0."""
    from oracle import entanglement as OE

    v = OE.measure(method, rho)
    if method == "eof" and np.isnan(v) and OE.concurrence(rho) < 1e-6:
        return 0.0
    return v


def all_pairs(n):
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


def eigvec(basis, outcome):
    """The +1 (outcome 0) / -1 (outcome 1) eigenvector of X (0), Y (1) or Z (2)."""
    sg = 1 if outcome == 0 else -1
    if basis == 2:
        return np.array([1, 0], dtype=complex) if outcome == 0 else np.array([0, 1], dtype=complex)
    return _R * np.array([1, sg if basis == 0 else 1j * sg], dtype=complex)


def product_vectors():
    """[9, 4, 4]: the product eigenvector of (setting, outcome)."""
    v = np.zeros((9, 4, 4), dtype=complex)
    for s in range(9):
        for o in range(4):
            v[s, o] = np.kron(eigvec(s // 3, o >> 1), eigvec(s % 3, o & 1))
    return v


def pair_tomo_probs(rdms):
    """[npairs, 9, 4]: max(0, <v|rho|v>), not renormalised."""
    r = np.asarray(rdms, dtype=complex).reshape(-1, 4, 4)
    v = product_vectors()
    return np.maximum(0.0, np.einsum("soi,pij,soj->pso", v.conj(), r, v).real)


def concurrence_bound_probs(rdms):
    """[npairs, 3]: P("1111"), P("0011"), P("1100"); rho_1 the marginal of the lower qubit."""
    r = np.asarray(rdms, dtype=complex).reshape(-1, 2, 2, 2, 2)  # [p, hi, lo, hi', lo']
    lo = np.einsum("pabac->pbc", r)
    hi = np.einsum("pabcb->pac", r)
    t1 = np.sum(np.abs(lo) ** 2, axis=(1, 2))
    t2 = np.sum(np.abs(hi) ** 2, axis=(1, 2))
    t12 = np.sum(np.abs(r) ** 2, axis=(1, 2, 3, 4))
    return np.maximum(0.0, np.stack([(1 - t1 - t2 + t12) / 4, (1 - t1) / 2, (1 - t2) / 2], axis=1))


def multinomial_counts(probs, shots, seed=0, run=0, u=None):
    """int64[njobs, K]: shot t of job j takes the smallest k with C_k > u[t, j] * P (C: sequential
    inclusive sums, P = C_{K-1}), or the last k with p_k > 0 where rounding leaves none."""
    p = np.asarray(probs, dtype=np.float64)
    njobs, K = p.shape
    if u is None:
        u = uniforms(seed, run, shots, njobs)
    u = np.asarray(u, dtype=np.float64)
    c = np.zeros_like(p)
    acc = np.zeros(njobs)
    for k in range(K):  # sequential adds
        acc = acc + p[:, k]
        c[:, k] = acc
    total = c[:, -1]
    if not np.all(total > 0):
        raise ValueError("a job with zero total probability")
    target = u * total[None, :]  # a single product
    k = (c[None, :, :] <= target[:, :, None]).sum(axis=2)
    lastnz = K - 1 - np.argmax(p[:, ::-1] > 0, axis=1)
    k = np.where(k >= K, lastnz[None, :], k)
    out = np.zeros((njobs, K), dtype=np.int64)
    for j in range(njobs):
        out[j] = np.bincount(k[:, j], minlength=K)
    return out


def linear_inversion(counts):
    """[npairs, 4, 4]: rho_lin = 1/4 sum T[P][Q] P (x) Q from count tables [npairs, 9, 4]."""
    c = np.asarray(counts, dtype=np.float64).reshape(-1, 9, 4)
    tot = c.sum(axis=2)
    if not np.all(tot > 0):
        raise ValueError("a setting with no counts")
    f = c / tot[:, :, None]
    s_hi = np.array([1, 1, -1, -1.0])
    s_lo = np.array([1, -1, 1, -1.0])
    T = np.zeros((len(c), 4, 4))
    T[:, 0, 0] = 1.0
    for s in range(9):
        a, b = s // 3 + 1, s % 3 + 1
        T[:, a, b] = f[:, s] @ (s_hi * s_lo)
        T[:, a, 0] += f[:, s] @ s_hi / 3.0
        T[:, 0, b] += f[:, s] @ s_lo / 3.0
    rho = np.zeros((len(c), 4, 4), dtype=complex)
    for a in range(4):
        for b in range(4):
            rho += 0.25 * T[:, a, b, None, None] * np.kron(PAULI[a], PAULI[b])[None]
    return rho


def psd_rescale(h):
    """Smolin, Gambetta, Smith (PRL 108, 070502) on one Hermitian matrix, then trace 1."""
    mu, v = np.linalg.eigh(np.asarray(h, dtype=complex))
    mu, v = mu[::-1].copy(), v[:, ::-1]  # descending
    a, i = 0.0, len(mu)
    while i > 0 and mu[i - 1] + a / i < 0:
        a += mu[i - 1]
        mu[i - 1] = 0.0
        i -= 1
    mu[:i] += a / i
    rho = (v * mu[None, :]) @ v.conj().T
    return rho / np.trace(rho).real


def tomo_fit(counts):
    return np.stack([psd_rescale(r) for r in linear_inversion(counts)])


def tomography(rdms, shots, seed, run=0):
    """The chain probs -> counts (job index pair 9 + s) -> fit.  Returns (rho_fit, counts)."""
    pr = pair_tomo_probs(rdms)
    counts = multinomial_counts(pr.reshape(-1, 4), shots, seed, run).reshape(-1, 9, 4)
    return tomo_fit(counts), counts


def concurrence_lower_bounds(rdms, shots, seed, run=0):
    """max(8 f_pmpm - 4 f_ipm, 8 f_pmpm - 4 f_pmi) from three binomial jobs a pair (index pair 3 + c)."""
    pr = concurrence_bound_probs(rdms).reshape(-1)
    counts = multinomial_counts(np.stack([pr, 1 - pr], axis=1), shots, seed, run)
    f = (counts[:, 0] / shots).reshape(-1, 3)
    return np.maximum(8 * f[:, 0] - 4 * f[:, 2], 8 * f[:, 0] - 4 * f[:, 1])
