"""numpy restatements for the density-matrix engine's tests (adaptaqc_amd/csrc/dm.hip).

- ``replay``: the steps of aqc_dm_plan applied to vec(rho) with the index conventions of
  include/aqc_hip.h -- entry (r, c) of rho at r + (c << n); a step acts on the 4 or 16 entries that
  share every other index bit, local index j = r_q0 + 2 c_q0, or (r_q0 + 2 r_q1) + 4 (c_q0 + 2 c_q1);
- ``pair_rdm``: the 4x4 partial trace of a full density matrix, index 2 bit_hi + bit_lo;
- ``kron_all``: the Kronecker product of per-factor matrices, factor 0 on the lowest qubits.
"""
import numpy as np


def _local_axes(n, step):
    """The axes of rho.reshape((2,) * 2n) (axis 0 = column bit n-1 ... axis 2n-1 = row bit 0) that make
    up the step's local index, most significant first."""
    def axis(bit):  # index bit b of r + (c << n) is axis 2n - 1 - b
        return 2 * n - 1 - bit

    q0, q1 = int(step["q0"]), int(step["q1"])
    if int(step["nq"]) == 1:
        return [axis(n + q0), axis(q0)]  # j = r + 2 c
    return [axis(n + q1), axis(n + q0), axis(q1), axis(q0)]  # J = r0 + 2 r1 + 4 c0 + 8 c1


def replay(n, steps):
    """rho [2^n, 2^n] after the steps from |0...0><0...0|."""
    dim = 2 ** n
    vec = np.zeros(dim * dim, dtype=complex)
    vec[0] = 1.0
    for st in steps:
        nq = int(st["nq"])
        d = 2 ** nq
        m = np.asarray(st["m"], dtype=np.float64).view(np.complex128)
        axes = _local_axes(n, st)
        t = np.moveaxis(vec.reshape((2,) * (2 * n)), axes, range(len(axes))).reshape(d * d, -1)
        if int(st["kind"]) == 0:  # X <- U X U^dag with X[r, c] = x[r + d c]
            u = m[: d * d].reshape(d, d)
            x = t.reshape(d, d, -1)  # [c, r, rest]
            t = np.einsum("ar,crk,bc->bak", u, x, u.conj()).reshape(d * d, -1)
        else:
            s = m[: d ** 4].reshape(d * d, d * d)
            t = s @ t
        vec = np.moveaxis(t.reshape((2,) * len(axes) + (2,) * (2 * n - len(axes))), range(len(axes)), axes).reshape(-1)
    return np.ascontiguousarray(vec.reshape(dim, dim).T)  # vec index r + (c << n)


def pair_rdm(rho, n, a, b):
    """The 4x4 RDM of qubits (a, b) of rho [2^n, 2^n], index 2 bit_hi + bit_lo (hi = max)."""
    hi, lo = max(a, b), min(a, b)
    t = rho.reshape((2,) * (2 * n))  # row qubits n-1 .. 0, then column qubits n-1 .. 0
    r = np.moveaxis(t, [n - 1 - hi, n - 1 - lo, 2 * n - 1 - hi, 2 * n - 1 - lo], [0, 1, 2, 3])
    r = r.reshape(2, 2, 2, 2, 2 ** (n - 2), 2 ** (n - 2))
    return np.trace(r, axis1=4, axis2=5).reshape(4, 4)


def kron_all(factors):
    """(x) of the factors, factor 0 on the lowest qubits (index bit q = qubit q)."""
    out = np.eye(1, dtype=complex)
    for f in factors:
        out = np.kron(f, out)
    return out
