"""numpy restatement of noisy pair tomography on the MPS engine (adaptaqc_amd/csrc/mps_traj.hip,
aqc_mps_traj_pair_tomo) on a dense state.

``pair_tomography``: the per-trajectory rule of aqc_mps_traj_pair_tomo (include/aqc_hip.h), all
trajectories at once.  The trajectory is evolved as mps_trajectory_ref.trajectories evolves it, without
its measurement part; the pair RDM, the setting probabilities and the draw follow traj_tomography_ref.

A trajectory is ``near`` when any Kraus boundary or any pair boundary lies within BAND = 1e-6 of u P:
the band mps_trajectory_ref.py justifies for this engine (reduce_zeros chops sigma^2 <= 1e-16, so
amplitudes move by up to 1e-8), not the statevector test's 1e-12.

Conventions as traj_tomography_ref.py: hi = max, lo = min; RDM index 2 bit_hi + bit_lo; setting
s = 3 b_hi + b_lo = t % 9; outcome o = 2 o_hi + o_lo; u [T, E + npairs], events first, then pairs.
"""
import numpy as np

import mps_trajectory_ref as mref
import traj_tomography_ref as ttref
import trajectory_ref as tref

BAND = mref.BAND


def evolve(n, rows, u):
    """(psi [S, 2^n], choices uint8[S, E], near bool[S], E) after the program's rows under the event
    uniforms u [S, >= E]: the Kraus part of mps_trajectory_ref.trajectories."""
    u = np.asarray(u, dtype=np.float64)
    shots = u.shape[0]
    n_events = int(np.count_nonzero(rows["flags"] == tref.KRAUS1))
    psi = np.zeros((shots, 2 ** n), dtype=complex)
    psi[:, 0] = 1.0
    choices = np.zeros((shots, n_events), dtype=np.uint8)
    near = np.zeros(shots, dtype=bool)
    idx = np.arange(shots)
    e = 0
    for row in rows:
        mats = tref._matrices(row)
        if int(row["flags"]) != tref.KRAUS1:
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
    return psi, choices, near, n_events


def draw(p, u):
    """traj_tomography_ref.draw with the band of this engine: (o int[S], near bool[S])."""
    c = np.zeros_like(p)
    acc = np.zeros(p.shape[0])
    for o in range(p.shape[1]):
        acc = acc + p[:, o]
        c[:, o] = acc
    total = c[:, -1]
    target = u * total
    above = c > target[:, None]
    last_nz = p.shape[1] - 1 - np.argmax((p > 0)[:, ::-1], axis=1)
    o = np.where(above.any(axis=1), np.argmax(above, axis=1), last_nz)
    near = (np.abs(c - target[:, None]) < BAND * total[:, None]).any(axis=1)
    return o, near


def trajectory_probs(n, rows, pairs, effects, u):
    """(p [npairs, T, 4], near bool[T] of the Kraus boundaries, E): every trajectory's outcome
    probabilities in its setting t % 9, for every pair."""
    psi, _, near, n_events = evolve(n, rows, u)
    setting = np.arange(psi.shape[0]) % 9
    p = np.stack([ttref.setting_probs(psi, n, max(a, b), min(a, b), effects, setting) for a, b in pairs])
    return p, near, n_events


def pair_tomography(n, rows, pairs, effects, u):
    """(outcomes uint8[T, npairs], counts int64[npairs, 9, 4], near bool[T]) under u [T, E + npairs],
    T = 9 shots."""
    u = np.asarray(u, dtype=np.float64)
    ntraj, npairs = u.shape[0], len(pairs)
    assert ntraj % 9 == 0
    p, near, n_events = trajectory_probs(n, rows, pairs, effects, u)
    assert u.shape[1] == n_events + npairs, "u does not have one column per Kraus row and per pair"
    outcomes = np.zeros((ntraj, npairs), dtype=np.uint8)
    near = near.copy()
    for j in range(npairs):
        o, nr = draw(p[j], u[:, n_events + j])
        outcomes[:, j] = o
        near |= nr
    return outcomes, ttref.counts_of(outcomes), near
