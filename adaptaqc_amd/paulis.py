"""Pauli-string labels for the device expectation kernels (aqc_sv_pauli_expect / aqc_mps_pauli_expect).

Labels follow qiskit: the rightmost character acts on qubit 0 (``"XIZ"`` is X on qubit 2 and Z on
qubit 0).  The kernels take them either as per-qubit codes (0 I, 1 X, 2 Y, 3 Z; column q = qubit q)
or as bit masks (bit q = qubit q; X sets the x mask, Z the z mask, Y both).  Host-only: nothing here
touches the GPU.
"""
import numpy as np

CODES = {"I": 0, "X": 1, "Y": 2, "Z": 3}
LETTERS = "IXYZ"


def label_to_codes(label, n=None):
    """uint8[n] of codes, entry q for qubit q.  ``n``: the expected number of qubits."""
    if not isinstance(label, str):
        raise ValueError(f"a Pauli label must be a string, got {type(label).__name__}")
    if n is not None and len(label) != int(n):
        raise ValueError(f"Pauli label {label!r} has {len(label)} characters for {n} qubits")
    try:
        return np.array([CODES[c] for c in reversed(label)], dtype=np.uint8)
    except KeyError as e:
        raise ValueError(f"unknown Pauli letter {e.args[0]!r} in label {label!r} (use I, X, Y, Z)") from None


def codes_to_label(codes):
    return "".join(LETTERS[int(c)] for c in reversed(np.asarray(codes).reshape(-1)))


def terms_to_codes(terms, n):
    """(nterms, n) contiguous uint8 codes from a list of labels or an array of codes."""
    n = int(n)
    if isinstance(terms, str):
        terms = [terms]
    if isinstance(terms, np.ndarray):
        codes = terms
        if codes.ndim != 2 or codes.shape[1] != n:
            raise ValueError(f"a code array must have shape (nterms, {n}), got {codes.shape}")
        if codes.size and (codes.min() < 0 or codes.max() > 3):
            raise ValueError("Pauli codes must be 0 (I), 1 (X), 2 (Y) or 3 (Z)")
        return np.ascontiguousarray(codes, dtype=np.uint8)
    terms = list(terms)
    out = np.zeros((len(terms), n), dtype=np.uint8)
    for t, label in enumerate(terms):
        out[t] = label_to_codes(label, n)
    return out


def codes_to_masks(codes):
    """(xmask, zmask) uint64[nterms] of an (nterms, n) code array, n <= 64: bit q = qubit q."""
    codes = np.asarray(codes)
    if codes.ndim != 2:
        raise ValueError("codes_to_masks: an (nterms, n) array")
    if codes.shape[1] > 64:
        raise ValueError("bit masks hold at most 64 qubits")
    bit = np.uint64(1) << np.arange(codes.shape[1], dtype=np.uint64)
    isx = (codes == 1) | (codes == 2)
    isz = (codes == 3) | (codes == 2)
    x = (isx * bit[None, :]).sum(axis=1, dtype=np.uint64)
    z = (isz * bit[None, :]).sum(axis=1, dtype=np.uint64)
    return np.ascontiguousarray(x, dtype=np.uint64), np.ascontiguousarray(z, dtype=np.uint64)


def label_to_masks(label, n=None):
    """(x, z) Python ints of one label."""
    x, z = codes_to_masks(label_to_codes(label, n)[None, :])
    return int(x[0]), int(z[0])


def operator_to_masks(operator, n):
    """(xmask, zmask, coeffs) of a Pauli sum on n qubits: a ``{label: coefficient}`` dict, or
    ``(terms, coeffs)`` with terms as ``terms_to_codes`` takes them.  coeffs: complex128[nterms]."""
    if isinstance(operator, dict):
        terms, coeffs = list(operator.keys()), list(operator.values())
    else:
        terms, coeffs = operator
    x, z = codes_to_masks(terms_to_codes(terms, n))
    coeffs = np.ascontiguousarray(np.asarray(coeffs, dtype=np.complex128).reshape(-1))
    if len(coeffs) != len(x):
        raise ValueError(f"a Pauli sum needs one coefficient per term: {len(x)} terms, {len(coeffs)} coefficients")
    return x, z, coeffs


def group_by_xmask(xmask, zmask, coeffs):
    """The grouping aqc_sv_pauli_apply does on the host, restated: with P = i^popcount(x & z) X^x Z^z,
    (sum_t c_t P_t psi)[j] = sum_g psi[j ^ X_g] sum_{t in g} c'_t (-1)^popcount((j ^ X_g) & z_t),
    c'_t = i^popcount(x_t & z_t) c_t.  Returns a list of ``(X_g, [(z_t, c'_t), ...])``: groups in order
    of first appearance of their x mask, terms of a group in input order (the order the kernel sums
    in).  The phase is applied by exchanging and negating the parts, so c' holds the bits of c."""
    xmask = [int(v) for v in np.asarray(xmask).reshape(-1)]
    zmask = [int(v) for v in np.asarray(zmask).reshape(-1)]
    coeffs = [complex(c) for c in np.asarray(coeffs).reshape(-1)]
    if not len(xmask) == len(zmask) == len(coeffs):
        raise ValueError("group_by_xmask: one x mask, z mask and coefficient per term")
    index = {}
    groups = []
    for x, z, c in zip(xmask, zmask, coeffs):
        ny = bin(x & z).count("1") & 3
        cp = (c, complex(-c.imag, c.real), -c, complex(c.imag, -c.real))[ny]
        if x not in index:
            index[x] = len(groups)
            groups.append((x, []))
        groups[index[x]][1].append((z, cp))
    return groups


def parity_from_counts(counts, qubits):
    """Average of (-1)^(number of ones among ``qubits``) over a counts dict; keys are qiskit
    bitstrings, read right to left (qubit q is character -1 - q).  Spaces (register separators)
    are ignored."""
    qubits = [int(q) for q in qubits]
    total = 0
    acc = 0
    for key, value in counts.items():
        bits = key.replace(" ", "")
        ones = 0
        for q in qubits:
            if q >= len(bits):
                raise ValueError(f"counts key {key!r} has no bit for qubit {q}")
            ones += bits[len(bits) - 1 - q] == "1"
        acc += (-value if ones & 1 else value)
        total += value
    if total == 0:
        raise ValueError("parity_from_counts: empty counts")
    return acc / total
