"""numpy restatement of the MPS trajectory sampler (adaptaqc_amd/csrc/mps_traj.hip) on a dense state,
for the noise tests above the statevector sampler.

``trajectories``: the per-shot rule of aqc_mps_traj_sample (include/aqc_hip.h) on a program of aqc_op_t
rows, all shots at once: the Kraus events as trajectory_ref.trajectories, then the qubits measured one by
one, q = 0 .. n-1, with bit = [u_{E+q} (p0 + p1) >= p0] and the projection.

A shot is ``near`` when some |C_k - u P| < 1e-6 P.  The band is 1e-6, not the statevector test's 1e-12:
the engine's reduce_zeros chops sigma^2 <= 1e-16, so amplitudes move by up to 1e-8, and 1e-6 is the
oracle's tolerance for truncated MPS.
"""
import numpy as np

import trajectory_ref as tref

KRAUS1 = tref.KRAUS1
BAND = 1e-6


def trajectories(n, rows, u):
    """(words uint64[S, (n+63)//64], choices uint8[S, E], near bool[S]) under uniforms u [S, E + n]."""
    u = np.asarray(u, dtype=np.float64)
    shots = u.shape[0]
    n_events = u.shape[1] - n
    psi = np.zeros((shots, 2 ** n), dtype=complex)
    psi[:, 0] = 1.0
    choices = np.zeros((shots, n_events), dtype=np.uint8)
    near = np.zeros(shots, dtype=bool)
    idx = np.arange(shots)
    e = 0
    for row in rows:
        mats = tref._matrices(row)
        if int(row["flags"]) != KRAUS1:
            psi = tref.apply(psi, n, mats[0], tref._qubits(row))
            continue
        phis = np.stack([tref.apply(psi, n, k, (int(row["q0"]),)) for k in mats])  # [K, S, dim]
        p = np.sum(np.abs(phis) ** 2, axis=2)
        c = np.cumsum(p, axis=0)
        total = c[-1]
        target = u[:, e] * total
        above = c > target[None, :]
        last_nz = len(mats) - 1 - np.argmax((p > 0)[::-1], axis=0)
        k = np.where(above.any(axis=0), np.argmax(above, axis=0), last_nz)
        near |= (np.abs(c - target[None, :]) < BAND * total[None, :]).any(axis=0)
        choices[:, e] = k
        psi = phis[k, idx] / np.sqrt(p[k, idx])[:, None]
        e += 1
    assert e == n_events, "u does not have one column per Kraus row plus one per qubit"
    words = np.zeros((shots, (n + 63) // 64), dtype=np.uint64)
    basis = np.arange(2 ** n)
    for q in range(n):
        one = ((basis >> q) & 1).astype(bool)
        p1 = np.sum(np.abs(psi[:, one]) ** 2, axis=1)
        p0 = np.sum(np.abs(psi[:, ~one]) ** 2, axis=1)
        target = u[:, n_events + q] * (p0 + p1)
        bit = target >= p0
        near |= np.abs(target - p0) < BAND * (p0 + p1)
        psi = np.where(one[None, :] == bit[:, None], psi, 0.0) / np.sqrt(np.where(bit, p1, p0))[:, None]
        words[:, q // 64] |= bit.astype(np.uint64) << np.uint64(q % 64)
    return words, choices, near


def outcomes(words):
    """Basis indices (bit q = qubit q) of one-word outcomes, for trajectory_ref.counts_array."""
    w = np.asarray(words, dtype=np.uint64)
    assert w.shape[1] == 1
    return w[:, 0].astype(np.int64)
