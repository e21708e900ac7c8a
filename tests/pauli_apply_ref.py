"""numpy restatement of aqc_sv_pauli_apply and of small Hamiltonians, for the ground-state tests.

P = i^popcount(x & z) X^x Z^z (a qubit in both masks is Y; bit q = qubit q), so
(P psi)[j] = i^ny (-1)^popcount((j ^ x) & z) psi[j ^ x].  Labels are qiskit's: the rightmost character is
qubit 0.  Nothing here uses the package or the GPU.
"""
import numpy as np

_X = {"I": 0, "X": 1, "Y": 1, "Z": 0}
_Z = {"I": 0, "X": 0, "Y": 1, "Z": 1}


def label_masks(label):
    x = z = 0
    for q, ch in enumerate(reversed(label)):
        x |= _X[ch] << q
        z |= _Z[ch] << q
    return x, z


def _parity(v):
    v = v.copy()
    for s in (32, 16, 8, 4, 2, 1):
        v ^= v >> np.uint64(s)
    return (v & np.uint64(1)).astype(bool)


def apply_masks(xmask, zmask, coeffs, psi):
    """sum_t c_t P_t psi from (x, z) masks."""
    psi = np.asarray(psi, dtype=np.complex128)
    j = np.arange(psi.size, dtype=np.uint64)
    out = np.zeros_like(psi)
    for x, z, c in zip(xmask, zmask, coeffs):
        x, z = int(x), int(z)
        k = j ^ np.uint64(x)
        sign = np.where(_parity(k & np.uint64(z)), -1.0, 1.0)
        out += complex(c) * (1, 1j, -1, -1j)[bin(x & z).count("1") & 3] * sign * psi[k]
    return out


def apply_operator(operator, psi):
    """sum_t c_t P_t psi of a {label: coefficient} dict."""
    masks = [label_masks(s) for s in operator]
    return apply_masks([m[0] for m in masks], [m[1] for m in masks], list(operator.values()), psi)


def dense_hamiltonian(operator, n):
    """The 2^n x 2^n matrix of a {label: coefficient} dict, n <= 10; index bit q = qubit q."""
    assert n <= 10
    dim = 1 << n
    h = np.zeros((dim, dim), dtype=np.complex128)
    j = np.arange(dim, dtype=np.uint64)
    for label, c in operator.items():
        assert len(label) == n
        x, z = label_masks(label)
        k = j ^ np.uint64(x)
        sign = np.where(_parity(k & np.uint64(z)), -1.0, 1.0)
        # (P psi)[j] = phase sign[j] psi[k[j]]: one entry a row
        h[j.astype(np.int64), k.astype(np.int64)] += complex(c) * (1, 1j, -1, -1j)[bin(x & z).count("1") & 3] * sign
    return h


def spectrum(operator, n):
    """(eigenvalues ascending, eigenvectors in columns) by numpy's eigh."""
    return np.linalg.eigh(dense_hamiltonian(operator, n))


def weight(operator):
    """S = sum_t |c_t|."""
    return float(sum(abs(complex(c)) for c in operator.values()))
