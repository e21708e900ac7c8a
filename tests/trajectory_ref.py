"""numpy restatements of the trajectory sampler (adaptaqc_amd/csrc/traj.hip), for the noise tests.

- ``trajectories``: the per-shot rule of aqc_sv_traj_sample (include/aqc_hip.h) on a program of
  aqc_op_t rows, all shots at once: outcomes, Kraus choices and a ``near`` flag per shot;
- ``density_matrix``: the same program as an evolution of the full density matrix (small n).
"""
import numpy as np

import sampling_ref as ref

KRAUS1 = 1  # AQC_OP_KRAUS1


def _matrices(row):
    """A row's matrices: [the gate's 2x2 / 4x4], or the Kraus row's 2x2 operators."""
    m = np.asarray(row["m"], dtype=np.float64).view(np.complex128)
    if int(row["flags"]) == KRAUS1:
        return [m[4 * k: 4 * k + 4].reshape(2, 2) for k in range(int(row["q1"]))]
    return [m[:4].reshape(2, 2)] if int(row["nq"]) == 1 else [m[:16].reshape(4, 4)]


def _qubits(row):
    return (int(row["q0"]),) if int(row["nq"]) == 1 else (int(row["q0"]), int(row["q1"]))


def apply(psi, n, mat, qubits):
    """mat (2x2, or 4x4 with index 2 b1 + b0) on ``qubits`` of every row of psi [S, 2^n]."""
    s = psi.shape[0]
    t = psi.reshape((s,) + (2,) * n)
    ax = [n - q for q in qubits]  # qubit q is axis n - q (axis 0: the shots)
    if len(qubits) == 1:
        t = np.moveaxis(np.tensordot(mat, t, axes=([1], [ax[0]])), 0, ax[0])
    else:
        m = np.asarray(mat).reshape(2, 2, 2, 2)  # [b1', b0', b1, b0]
        t = np.moveaxis(np.tensordot(m, t, axes=([2, 3], [ax[1], ax[0]])), [0, 1], [ax[1], ax[0]])
    return np.ascontiguousarray(t).reshape(s, -1)


def trajectories(n, rows, u):
    """(outcomes int64[S], choices uint8[S, E], near bool[S]) of the program under uniforms u [S, E+1].
    At event e: p_k = |K_k psi|^2, C_k the in-order inclusive sums, P = C_last; the smallest k with
    C_k > u_e P, else the last k with p_k > 0; psi <- K_k psi / sqrt(p_k).  The final draw is
    sampling_ref.sv_sample with u_E.  near: some |C_k - u P| < 1e-12 P, or the final draw's flag."""
    u = np.asarray(u, dtype=np.float64)
    shots = u.shape[0]
    n_events = u.shape[1] - 1
    psi = np.zeros((shots, 2 ** n), dtype=complex)
    psi[:, 0] = 1.0
    choices = np.zeros((shots, n_events), dtype=np.uint8)
    near = np.zeros(shots, dtype=bool)
    e = 0
    for row in rows:
        mats = _matrices(row)
        if int(row["flags"]) != KRAUS1:
            psi = apply(psi, n, mats[0], _qubits(row))
            continue
        phis = np.stack([apply(psi, n, k, (int(row["q0"]),)) for k in mats])  # [K, S, dim]
        p = np.sum(np.abs(phis) ** 2, axis=2)  # [K, S]
        c = np.cumsum(p, axis=0)
        total = c[-1]
        target = u[:, e] * total
        above = c > target[None, :]
        k = np.where(above.any(axis=0), np.argmax(above, axis=0), 0)
        last_nz = len(mats) - 1 - np.argmax((p > 0)[::-1], axis=0)
        k = np.where(above.any(axis=0), k, last_nz)
        near |= (np.abs(c - target[None, :]) < 1e-12 * total[None, :]).any(axis=0)
        choices[:, e] = k
        idx = np.arange(shots)
        psi = phis[k, idx] / np.sqrt(p[k, idx])[:, None]
        e += 1
    assert e == n_events, "u does not have one column per Kraus row plus one"
    out = np.zeros(shots, dtype=np.int64)
    for s in range(shots):
        o, nr = ref.sv_sample(psi[s], u[s, n_events:])
        out[s] = o[0]
        near[s] |= nr[0]
    return out, choices, near


def density_matrix(n, rows):
    """rho [2^n, 2^n] after the program from |0...0><0...0| (index bit q = qubit q)."""
    dim = 2 ** n
    rho = np.zeros((dim, dim), dtype=complex)
    rho[0, 0] = 1.0
    eye = np.eye(dim, dtype=complex)
    for row in rows:
        mats = _matrices(row)
        qs = _qubits(row) if int(row["flags"]) != KRAUS1 else (int(row["q0"]),)
        # rows of apply(eye) are U|i>: its transpose is the full operator
        full = [apply(eye, n, m, qs).T for m in mats]
        rho = sum(f @ rho @ f.conj().T for f in full)
    return rho


def counts_array(samples, n):
    return np.bincount(np.asarray(samples).astype(np.int64), minlength=2 ** n)
