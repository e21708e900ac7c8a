"""numpy restatement of the noisy Pauli readout (adaptaqc_amd/csrc/traj.hip, aqc_sv_traj_pauli_counts),
for the trajectory Pauli tests.

- ``factor``: D_q = E[q][c - 1][0] - E[q][c - 1][1] of one qubit of a term;
- ``parity_operator``: M = (x)_q D_q (identity outside the support) as a dense Kronecker product;
- ``values``: Re <psi|M|psi> of every state and term -- through the dense M up to DENSE_MAX_QUBITS
  qubits, above it by applying the D_q to the state one qubit at a time (the same operator; a dense M
  of 13 qubits would take a gigabyte);
- ``pauli_counts``: the per-trajectory rule of aqc_sv_traj_pauli_counts (include/aqc_hip.h) on a
  program of aqc_op_t rows, all trajectories at once: values, outcomes, ``plus`` and a ``near`` flag
  per (trajectory, term); psi per trajectory from trajectory2_ref.evolve, which handles groups;
- ``exact_values``: Tr(rho M) from trajectory2_ref.density_matrix.

Codes: 0 I, 1 X, 2 Y, 3 Z, column q = qubit q (paulis.terms_to_codes).
"""
import numpy as np

import traj_tomography_ref as ttref
import trajectory2_ref as t2ref
from trajectory_ref import apply

DENSE_MAX_QUBITS = 10


def factor(effects, q, c):
    """The Hermitian 2x2 D_q of code c = 1 .. 3 on qubit q."""
    return ttref.unpack(effects[q, c - 1, 0]) - ttref.unpack(effects[q, c - 1, 1])


def parity_operator(n, codes_row, effects):
    """M [2^n, 2^n], index bit q = qubit q: the Kronecker product runs from qubit n-1 down to qubit 0."""
    m = np.eye(1, dtype=complex)
    for q in range(n - 1, -1, -1):
        c = int(codes_row[q])
        m = np.kron(m, factor(effects, q, c) if c else np.eye(2, dtype=complex))
    return m


def apply_parity(psi, n, codes_row, effects):
    """M psi for every row of psi [S, 2^n], one qubit of the support at a time."""
    out = psi
    for q in range(n):
        c = int(codes_row[q])
        if c:
            out = apply(out, n, factor(effects, q, c), (q,))
    return out


def values(psi, n, codes, effects):
    """[S, nterms]: Re <psi_t|M_j|psi_t>."""
    out = np.zeros((psi.shape[0], len(codes)))
    for j, row in enumerate(codes):
        if n <= DENSE_MAX_QUBITS:
            mpsi = psi @ parity_operator(n, row, effects).T
        else:
            mpsi = apply_parity(psi, n, row, effects)
        out[:, j] = np.einsum("sk,sk->s", psi.conj(), mpsi).real
    return out


def draw(v, u):
    """(outcome uint8, near bool) of values v and uniforms u (same shape): p+ = min(1, max(0, (1 + v) / 2)),
    outcome 1 iff u >= p+.  near as traj_tomography_ref.draw flags a boundary: the inclusive sum C = p+
    of a two-outcome draw with P = 1, |C - u P| < 1e-12 P."""
    pp = np.minimum(1.0, np.maximum(0.0, (1.0 + v) / 2))
    return (u >= pp).astype(np.uint8), np.abs(pp - u) < 1e-12


def pauli_counts(n, rows, codes, effects, u):
    """(values [S, nterms], outcomes uint8 [S, nterms], plus int64 [nterms], near bool [S, nterms]) under
    uniforms u [S, E + nterms]: trajectory t runs the rows with u[t, :E] and draws term j with
    u[t, E + j].  near: the term's own boundary flag, or any event boundary of its trajectory."""
    u = np.asarray(u, dtype=np.float64)
    codes = np.asarray(codes)
    psi, _, near_events, n_events = t2ref.evolve(n, rows, u)
    assert u.shape[1] == n_events + len(codes), "u does not have one column per event and per term"
    v = values(psi, n, codes, effects)
    outcomes, near = draw(v, u[:, n_events:])
    return v, outcomes, plus_of(outcomes), near | near_events[:, None]


def plus_of(outcomes, keep=None):
    """int64 [nterms]: the outcome-0 draws, over the (trajectory, term) entries of ``keep`` only."""
    mask = np.ones(outcomes.shape, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    return np.sum((outcomes == 0) & mask, axis=0).astype(np.int64)


def exact_values(n, rows, codes, effects):
    """[nterms]: Tr(rho M_j) with rho the density matrix after the program."""
    rho = t2ref.density_matrix(n, rows)
    return np.array([np.trace(rho @ parity_operator(n, row, effects)).real for row in codes])


def branch_values(n, rows, codes, effects):
    """exact_values by enumeration: every sequence of Kraus choices is one branch (its state normalised
    as a trajectory's, and its probability); the probability-weighted sum of the branches' values.
    Small programs only."""
    branches = [(1.0, np.eye(1, 2 ** n, dtype=complex))]
    for mats, qs, is_event in t2ref.events(rows):
        if not is_event:
            branches = [(w, apply(psi, n, mats[0], qs)) for w, psi in branches]
            continue
        grown = []
        for w, psi in branches:
            for k in mats:
                phi = apply(psi, n, k, qs)
                p = float(np.sum(np.abs(phi) ** 2))
                if p > 0:
                    grown.append((w * p, phi / np.sqrt(p)))
        branches = grown
    return sum(w * values(psi, n, codes, effects)[0] for w, psi in branches)


def mixed_effects(n, noisy, clean_qubits):
    """``noisy`` [n, 3, 2, 4] with the noiseless projectors on ``clean_qubits``."""
    from adaptaqc_amd.noise import readout_effects

    out = np.array(noisy, dtype=np.float64)
    out[list(clean_qubits)] = readout_effects(n, None)[list(clean_qubits)]
    return out
