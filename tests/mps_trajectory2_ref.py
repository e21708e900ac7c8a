"""numpy restatements of the MPS trajectory engine (adaptaqc_amd/csrc/mps_traj.hip) on a dense state for
programs that hold correlated two-qubit groups (AQC_OP_KRAUS2) beside one-qubit Kraus rows.

``evolve`` is trajectory2_ref's event loop -- a group is one event, p_k = |K_k psi|^2 from the full
state, the same choice rule -- with the band of this engine: a shot is ``near`` when some
|C_k - u P| < BAND P, BAND = mps_trajectory_ref.BAND = 1e-6, which that file justifies by reduce_zeros'
1e-16 chop on sigma^2 (amplitudes move by up to 1e-8).  What follows the events is what the other
restatements do, through their own helpers:
- ``trajectories``: the qubit-by-qubit measurement of mps_trajectory_ref (aqc_mps_traj_sample);
- ``pair_tomography``: the pair draws of mps_traj_tomography_ref (aqc_mps_traj_pair_tomo);
- ``pauli_counts``: the Pauli draws of mps_traj_pauli_ref (aqc_mps_traj_pauli_counts).
"""
import numpy as np

import mps_traj_pauli_ref as mpref
import mps_traj_tomography_ref as mtref
import mps_trajectory_ref as mref
import pauli_traj_ref as pref
import traj_tomography_ref as ttref
import trajectory2_ref as t2ref
from trajectory_ref import apply

BAND = mref.BAND


def evolve(n, rows, u):
    """(psi [S, 2^n], choices uint8[S, E], near bool[S], E) after the rows under the event uniforms
    u [S, >= E]: trajectory2_ref.evolve with the band BAND."""
    u = np.asarray(u, dtype=np.float64)
    shots = u.shape[0]
    steps = t2ref.events(rows)
    total_events = sum(1 for _, _, ev in steps if ev)
    psi = np.zeros((shots, 2 ** n), dtype=complex)
    psi[:, 0] = 1.0
    choices = np.zeros((shots, total_events), dtype=np.uint8)
    near = np.zeros(shots, dtype=bool)
    idx = np.arange(shots)
    e = 0
    for mats, qs, is_event in steps:
        if not is_event:
            psi = apply(psi, n, mats[0], qs)
            continue
        phis = np.stack([apply(psi, n, k, qs) for k in mats])  # [K, S, dim]
        p = np.sum(np.abs(phis) ** 2, axis=2)  # [K, S]
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
    return psi, choices, near, total_events


def measure(psi, n, u):
    """(words uint64[S, (n+63)//64], near bool[S]) of the qubits measured one by one, q = 0 .. n-1, under
    u [S, n]: bit = [u_q (p0 + p1) >= p0], then the projection (mps_trajectory_ref.trajectories' ending)."""
    shots = psi.shape[0]
    words = np.zeros((shots, (n + 63) // 64), dtype=np.uint64)
    near = np.zeros(shots, dtype=bool)
    basis = np.arange(2 ** n)
    for q in range(n):
        one = ((basis >> q) & 1).astype(bool)
        p1 = np.sum(np.abs(psi[:, one]) ** 2, axis=1)
        p0 = np.sum(np.abs(psi[:, ~one]) ** 2, axis=1)
        target = u[:, q] * (p0 + p1)
        bit = target >= p0
        near |= np.abs(target - p0) < BAND * (p0 + p1)
        psi = np.where(one[None, :] == bit[:, None], psi, 0.0) / np.sqrt(np.where(bit, p1, p0))[:, None]
        words[:, q // 64] |= bit.astype(np.uint64) << np.uint64(q % 64)
    return words, near


def trajectories(n, rows, u):
    """(words, choices uint8[S, E], near bool[S]) under uniforms u [S, E + n]."""
    u = np.asarray(u, dtype=np.float64)
    psi, choices, near, n_events = evolve(n, rows, u)
    assert u.shape[1] == n_events + n, "u does not have one column per event plus one per qubit"
    words, near_m = measure(psi, n, u[:, n_events:])
    return words, choices, near | near_m


def pair_tomography(n, rows, pairs, effects, u):
    """(outcomes uint8[T, npairs], counts int64[npairs, 9, 4], near bool[T]) under u [T, E + npairs],
    T = 9 shots: mps_traj_tomography_ref.pair_tomography behind this file's ``evolve``."""
    u = np.asarray(u, dtype=np.float64)
    ntraj, npairs = u.shape[0], len(pairs)
    assert ntraj % 9 == 0
    psi, _, near, n_events = evolve(n, rows, u)
    assert u.shape[1] == n_events + npairs, "u does not have one column per event and per pair"
    setting = np.arange(ntraj) % 9
    outcomes = np.zeros((ntraj, npairs), dtype=np.uint8)
    near = near.copy()
    for j, (a, b) in enumerate(pairs):
        p = ttref.setting_probs(psi, n, max(a, b), min(a, b), effects, setting)
        o, nr = mtref.draw(p, u[:, n_events + j])
        outcomes[:, j] = o
        near |= nr
    return outcomes, ttref.counts_of(outcomes), near


def pauli_counts(n, rows, codes, effects, u):
    """(values [S, nterms], outcomes uint8 [S, nterms], plus int64 [nterms], near bool [S, nterms]):
    mps_traj_pauli_ref.pauli_counts behind this file's ``evolve``."""
    u = np.asarray(u, dtype=np.float64)
    codes = np.asarray(codes)
    psi, _, near_events, n_events = evolve(n, rows, u)
    assert u.shape[1] == n_events + len(codes), "u does not have one column per event and per term"
    v = pref.values(psi, n, codes, effects)
    outcomes, near = mpref.draw(v, np.ones(psi.shape[0]), u[:, n_events:])
    return v, outcomes, pref.plus_of(outcomes), near | near_events[:, None]
