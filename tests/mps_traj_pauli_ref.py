"""numpy restatement of the noisy Pauli readout on the MPS engine (adaptaqc_amd/csrc/mps_traj.hip,
aqc_mps_traj_pauli_counts) on a dense state, built from what the other restatements hold.

``pauli_counts``: the per-trajectory rule of aqc_mps_traj_pauli_counts (include/aqc_hip.h), all
trajectories at once.  The trajectory is evolved by mps_traj_tomography_ref.evolve (the Kraus part of
the MPS sampler's restatement), v = Re <psi|M_j|psi> comes from pauli_traj_ref.values, and w = 1: the
dense state is normalised, so this restatement does not model a truncated MPS.  The draw:
  p+ = max(0, (w + v) / 2), p- = max(0, (w - v) / 2), outcome 1 (parity -1) iff u (p+ + p-) >= p+.

An entry is ``near`` when its own boundary p+ lies within BAND (p+ + p-) of u (p+ + p-), or any Kraus
boundary of its trajectory does: BAND = mps_trajectory_ref.BAND (1e-6), the band that file justifies
for this engine (reduce_zeros chops sigma^2 <= 1e-16, so amplitudes move by up to 1e-8).

Codes: 0 I, 1 X, 2 Y, 3 Z, column q = qubit q; u [S, E + nterms], events first, then terms.
"""
import numpy as np

import mps_traj_tomography_ref as mtref
import mps_trajectory_ref as mref
import pauli_traj_ref as pref

BAND = mref.BAND


def draw(v, w, u):
    """(outcome uint8, near bool) of the values v [S, nterms], the norms w [S] and the uniforms u (as v)."""
    pp = np.maximum(0.0, (w[:, None] + v) / 2)
    pm = np.maximum(0.0, (w[:, None] - v) / 2)
    total = pp + pm
    return (u * total >= pp).astype(np.uint8), np.abs(pp - u * total) < BAND * total


def pauli_counts(n, rows, codes, effects, u):
    """(values [S, nterms], outcomes uint8 [S, nterms], plus int64 [nterms], near bool [S, nterms])."""
    u = np.asarray(u, dtype=np.float64)
    codes = np.asarray(codes)
    psi, _, near_events, n_events = mtref.evolve(n, rows, u)
    assert u.shape[1] == n_events + len(codes), "u does not have one column per Kraus row and per term"
    v = pref.values(psi, n, codes, effects)
    outcomes, near = draw(v, np.ones(psi.shape[0]), u[:, n_events:])
    return v, outcomes, pref.plus_of(outcomes), near | near_events[:, None]
