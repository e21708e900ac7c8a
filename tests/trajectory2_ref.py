"""numpy restatements of the trajectory sampler (adaptaqc_amd/csrc/traj.hip) for programs that hold both
kinds of Kraus rows: one-qubit rows (AQC_OP_KRAUS1) and correlated two-qubit groups (AQC_OP_KRAUS2, nk
consecutive rows, one 4x4 operator each, one event).

- ``events``: the program as a list of steps -- a gate, or an event with its operators and qubits;
- ``trajectories``: the per-shot rule of aqc_sv_traj_sample, all shots at once: outcomes, choices and a
  ``near`` flag per shot;
- ``evolve``: the states after the rows only (the pair readout of traj_tomography_ref follows it);
- ``density_matrix``: the same program as an evolution of the full density matrix (small n).

p_k is |K_k psi|^2 from the full state, never through a reduced density matrix.
"""
import numpy as np

import sampling_ref as ref
from trajectory_ref import KRAUS1, _matrices, _qubits, apply

KRAUS2 = 3  # AQC_OP_KRAUS2


def events(rows):
    """[(operators, qubits, is_event)] in program order; a group of KRAUS2 rows is one entry."""
    out = []
    i = 0
    while i < len(rows):
        row = rows[i]
        flags = int(row["flags"])
        if flags & 0xFF == KRAUS2:
            nk = (flags >> 16) & 0xFF
            assert (flags >> 8) & 0xFF == 0 and 1 <= nk <= 16 and i + nk <= len(rows), "a group starts at k = 0"
            mats = []
            for k in range(nk):
                r = rows[i + k]
                assert int(r["flags"]) == KRAUS2 | (k << 8) | (nk << 16)
                assert (int(r["q0"]), int(r["q1"])) == (int(row["q0"]), int(row["q1"]))
                mats.append(np.asarray(r["m"], dtype=np.float64).view(np.complex128).reshape(4, 4))
            out.append((mats, (int(row["q0"]), int(row["q1"])), True))
            i += nk
        elif flags == KRAUS1:
            out.append((_matrices(row), (int(row["q0"]),), True))
            i += 1
        else:
            assert flags == 0
            out.append((_matrices(row), _qubits(row), False))
            i += 1
    return out


def n_events(rows):
    return sum(1 for _, _, ev in events(rows) if ev)


def evolve(n, rows, u):
    """(psi [S, 2^n], choices uint8[S, E], near bool[S], E) after the rows under the event uniforms
    u [S, >= E].  At an event: p_k = |K_k psi|^2, C_k the in-order inclusive sums, P = C_last; the smallest
    k with C_k > u_e P, else the last k with p_k > 0; psi <- K_k psi / sqrt(p_k).  near: some
    |C_k - u P| < 1e-12 P."""
    u = np.asarray(u, dtype=np.float64)
    shots = u.shape[0]
    steps = events(rows)
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
        near |= (np.abs(c - target[None, :]) < 1e-12 * total[None, :]).any(axis=0)
        choices[:, e] = k
        psi = phis[k, idx] / np.sqrt(p[k, idx])[:, None]
        e += 1
    return psi, choices, near, total_events


def trajectories(n, rows, u):
    """(outcomes int64[S], choices uint8[S, E], near bool[S]) of the program under uniforms u [S, E+1]:
    ``evolve``, then the final draw sampling_ref.sv_sample with u_E.  near: an event's flag, or the
    final draw's."""
    u = np.asarray(u, dtype=np.float64)
    psi, choices, near, total_events = evolve(n, rows, u)
    assert u.shape[1] == total_events + 1, "u does not have one column per event plus one"
    out = np.zeros(u.shape[0], dtype=np.int64)
    for s in range(u.shape[0]):
        o, nr = ref.sv_sample(psi[s], u[s, total_events:])
        out[s] = o[0]
        near[s] |= nr[0]
    return out, choices, near


def density_matrix(n, rows):
    """rho [2^n, 2^n] after the program from |0...0><0...0| (index bit q = qubit q); a group's
    operators are summed over."""
    dim = 2 ** n
    rho = np.zeros((dim, dim), dtype=complex)
    rho[0, 0] = 1.0
    eye = np.eye(dim, dtype=complex)
    for mats, qs, _ in events(rows):
        full = [apply(eye, n, m, qs).T for m in mats]  # rows of apply(eye) are U|i>
        rho = sum(f @ rho @ f.conj().T for f in full)
    return rho


# ---- the models and programs the tests share ------------------------------------------------------
T1, T2 = 50e3, 70e3


def collective_decay(gamma):
    """K0 = diag(1, 1, 1, sqrt(1 - gamma)), K1 = sqrt(gamma) |00><11|."""
    k1 = np.zeros((4, 4), dtype=complex)
    k1[0, 3] = np.sqrt(gamma)
    return [np.diag([1.0, 1.0, 1.0, np.sqrt(1 - gamma)]).astype(complex), k1]


def random_channel(seed=7):
    """Three dense complex 4x4 operators: the blocks of the Q factor of a 12x4 complex Gaussian matrix."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((12, 4)) + 1j * rng.standard_normal((12, 4)))
    return [q[4 * k: 4 * k + 4] for k in range(3)]


def cx_error(which):
    from adaptaqc_amd import noise

    if which == "a":
        return noise.depolarizing_error(0.05, 2)
    if which == "b":
        return noise.QuantumError.two_qubit(collective_decay(0.3))
    assert which == "c"
    return noise.QuantumError.two_qubit(random_channel())


def model(which):
    """Thermal relaxation for 5000 after rx / ry / rz (test_gpu_trajectories._model) and on cx one of:
    "a" depolarizing_error(0.05, 2); "b" collective decay, gamma = 0.3; "c" the seeded random channel."""
    from adaptaqc_amd import noise

    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(noise.thermal_relaxation_error(T1, T2, 5000), ["rx", "ry", "rz"])
    nm.add_all_qubit_quantum_error(cx_error(which), "cx")
    return nm


def ops(n, depth):
    """The seeded brickwork of the trajectory tests; on 3 qubits with cx the other way round and on
    non-adjacent qubits appended."""
    out = ref.brickwork(n, depth, 100 + n)
    if n == 3:
        out += [("cx", (2, 0), ()), ("ry", (1,), (0.4,)), ("cx", (0, 2), ()), ("cx", (1, 0), ())]
    return out


def program(n, depth, which):
    """(circuit, rows, n_events) of ``ops(n, depth)`` under ``model(which)``."""
    from adaptaqc_amd.noise import trajectory_program
    from conftest import to_circuit

    qc = to_circuit(n, ops(n, depth))
    rows, total_events, _ = trajectory_program(qc, model(which))
    return qc, rows, total_events
