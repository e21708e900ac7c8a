"""numpy restatements of noisy pair tomography (adaptaqc_amd/csrc/traj.hip, aqc_sv_traj_pair_tomo), for
the trajectory-tomography tests.

- ``readout_effects_ref``: the POVM effects of a noisy Pauli-basis measurement from Kraus lists;
- ``pair_tomography``: the per-trajectory rule of aqc_sv_traj_pair_tomo (include/aqc_hip.h) on a
  program of aqc_op_t rows, all trajectories at once: outcomes, counts and a ``near`` flag each;
- ``exact_tables``: the outcome probabilities of the nine settings of every pair from the
  density-matrix evolution of the program.

Conventions as tests/tomography_ref.py: hi = max, lo = min; RDM index 2 bit_hi + bit_lo; basis codes
0 X, 1 Y, 2 Z; setting s = 3 b_hi + b_lo; outcome o = 2 o_hi + o_lo.
"""
import numpy as np

import trajectory_ref as tref

H = np.array([[1, 1], [1, -1]], dtype=complex) / np.sqrt(2)
SDG = np.diag([1.0 + 0j, -1j])


def _adjoint(kraus, e):
    return e if not kraus else sum(k.conj().T @ e @ k for k in kraus)


def pack(e):
    """(E00, E11, Re E01, Im E01) of a Hermitian 2x2 matrix."""
    return np.array([e[0, 0].real, e[1, 1].real, e[0, 1].real, e[0, 1].imag])


def unpack(w):
    """The Hermitian 2x2 matrix of (E00, E11, Re E01, Im E01)."""
    z = w[2] + 1j * w[3]
    return np.array([[w[0], z], [np.conj(z), w[1]]], dtype=complex)


def readout_effects_ref(n, kraus_of):
    """[n, 3, 2, 4]: E = Sdg^dag A_sdg( H^dag A_h( A_meas(|o><o|) ) H ) Sdg with A_x the adjoint of the
    channel whose Kraus list is ``kraus_of(x, q)`` (an empty list: no error); H / A_h for X and Y
    only, Sdg / A_sdg for Y only."""
    out = np.zeros((n, 3, 2, 4))
    for q in range(n):
        for b in range(3):
            for o in range(2):
                e = np.zeros((2, 2), dtype=complex)
                e[o, o] = 1.0
                e = _adjoint(kraus_of("measure", q), e)
                if b < 2:
                    e = H.conj().T @ _adjoint(kraus_of("h", q), e) @ H
                if b == 1:
                    e = SDG.conj().T @ _adjoint(kraus_of("sdg", q), e) @ SDG
                out[q, b, o] = pack(e)
    return out


def pair_effects(effects, hi, lo):
    """[9, 4, 4, 4]: E[hi][b_hi][o_hi] (x) E[lo][b_lo][o_lo] for (setting, outcome)."""
    out = np.zeros((9, 4, 4, 4), dtype=complex)
    for s in range(9):
        for o in range(4):
            out[s, o] = np.kron(unpack(effects[hi, s // 3, o >> 1]), unpack(effects[lo, s % 3, o & 1]))
    return out


def pair_rdms(psi, n, hi, lo):
    """[S, 4, 4]: the RDM of qubits (hi, lo) of every row of psi [S, 2^n], index 2 bit_hi + bit_lo."""
    s = psi.shape[0]
    t = psi.reshape((s,) + (2,) * n)
    t = np.moveaxis(t, [n - hi, n - lo], [1, 2]).reshape(s, 4, -1)
    return np.einsum("sar,sbr->sab", t, t.conj())


def evolve(n, rows, u):
    """(psi [S, 2^n], near bool[S], E) after the program's rows under the event uniforms u [S, >= E],
    by the rule of trajectory_ref.trajectories; E = the number of Kraus rows."""
    u = np.asarray(u, dtype=np.float64)
    shots = u.shape[0]
    psi = np.zeros((shots, 2 ** n), dtype=complex)
    psi[:, 0] = 1.0
    near = np.zeros(shots, dtype=bool)
    idx = np.arange(shots)
    e = 0
    for row in rows:
        mats = tref._matrices(row)
        if int(row["flags"]) != tref.KRAUS1:
            psi = tref.apply(psi, n, mats[0], tref._qubits(row))
            continue
        phis = np.stack([tref.apply(psi, n, k, (int(row["q0"]),)) for k in mats])
        p = np.sum(np.abs(phis) ** 2, axis=2)
        c = np.cumsum(p, axis=0)
        total = c[-1]
        target = u[:, e] * total
        above = c > target[None, :]
        last_nz = len(mats) - 1 - np.argmax((p > 0)[::-1], axis=0)
        k = np.where(above.any(axis=0), np.argmax(above, axis=0), last_nz)
        near |= (np.abs(c - target[None, :]) < 1e-12 * total[None, :]).any(axis=0)
        psi = phis[k, idx] / np.sqrt(p[k, idx])[:, None]
        e += 1
    return psi, near, e


def draw(p, u):
    """(o int[S], near bool[S]): the smallest o with C_o > u P (C the in-order inclusive sums of
    p [S, 4], P = C_last), else the last o with p_o > 0."""
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
    near = (np.abs(c - target[:, None]) < 1e-12 * total[:, None]).any(axis=1)
    return o, near


def setting_probs(psi, n, hi, lo, effects, setting):
    """[S, 4]: max(0, Re Tr[(E_hi (x) E_lo) rho]) of row t of psi in setting[t]."""
    rho = pair_rdms(psi, n, hi, lo)
    eff = pair_effects(effects, hi, lo)[setting]  # [S, 4, 4, 4]
    return np.maximum(0.0, np.einsum("toab,tba->to", eff, rho).real)


def pair_tomography(n, rows, pairs, effects, u):
    """(outcomes uint8[T, npairs], counts int64[npairs, 9, 4], near bool[T]) under uniforms
    u [T, E + npairs], T = 9 shots: trajectory t runs the rows with u[t, :E] and serves setting
    t % 9 of every pair j with u[t, E + j].  near: any Kraus boundary or any pair boundary with
    |C - u P| < 1e-12 P."""
    u = np.asarray(u, dtype=np.float64)
    ntraj, npairs = u.shape[0], len(pairs)
    assert ntraj % 9 == 0
    psi, near, n_events = evolve(n, rows, u)
    assert u.shape[1] == n_events + npairs, "u does not have one column per Kraus row and per pair"
    setting = np.arange(ntraj) % 9
    outcomes = np.zeros((ntraj, npairs), dtype=np.uint8)
    for j, (a, b) in enumerate(pairs):
        hi, lo = max(a, b), min(a, b)
        p = setting_probs(psi, n, hi, lo, effects, setting)
        o, nr = draw(p, u[:, n_events + j])
        outcomes[:, j] = o
        near |= nr
    return outcomes, counts_of(outcomes), near


def counts_of(outcomes, keep=None):
    """int64[npairs, 9, 4] from outcomes [T, npairs] (trajectory t: setting t % 9), over the
    trajectories of ``keep`` (a bool mask) only."""
    ntraj, npairs = outcomes.shape
    setting = np.arange(ntraj) % 9
    mask = np.ones(ntraj, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    counts = np.zeros((npairs, 9, 4), dtype=np.int64)
    for j in range(npairs):
        np.add.at(counts[j], (setting[mask], outcomes[mask, j]), 1)
    return counts


def tables_of(rho_full, n, pairs, effects):
    """[npairs, 9, 4]: Re Tr[(E_hi (x) E_lo) rho_pair] of the full density matrix rho_full."""
    out = np.zeros((len(pairs), 9, 4))
    t = rho_full.reshape((2,) * (2 * n))  # axes: row qubits n-1 .. 0, then column qubits n-1 .. 0
    for j, (a, b) in enumerate(pairs):
        hi, lo = max(a, b), min(a, b)
        r = np.moveaxis(t, [n - 1 - hi, n - 1 - lo, 2 * n - 1 - hi, 2 * n - 1 - lo], [0, 1, 2, 3])
        r = r.reshape(2, 2, 2, 2, 2 ** (n - 2), 2 ** (n - 2))
        rdm = np.trace(r, axis1=4, axis2=5).reshape(4, 4)
        out[j] = np.einsum("soab,ba->so", pair_effects(effects, hi, lo), rdm).real
    return out


def exact_tables(n, rows, pairs, effects):
    """[npairs, 9, 4]: the outcome probabilities of every (pair, setting) after the program, from
    trajectory_ref.density_matrix."""
    return tables_of(tref.density_matrix(n, rows), n, pairs, effects)


def branch_tables(n, rows, pairs, effects):
    """[npairs, 9, 4]: exact_tables by enumeration -- every sequence of Kraus choices is one branch
    (its state, normalised as a trajectory's, and its probability); the tables are the
    probability-weighted sums of the branches' setting_probs.  Small programs only."""
    branches = [(1.0, np.eye(1, 2 ** n, dtype=complex))]
    for row in rows:
        mats = tref._matrices(row)
        if int(row["flags"]) != tref.KRAUS1:
            branches = [(w, tref.apply(psi, n, mats[0], tref._qubits(row))) for w, psi in branches]
            continue
        grown = []
        for w, psi in branches:
            for k in mats:
                phi = tref.apply(psi, n, k, (int(row["q0"]),))
                p = float(np.sum(np.abs(phi) ** 2))
                if p > 0:
                    grown.append((w * p, phi / np.sqrt(p)))
        branches = grown
    out = np.zeros((len(pairs), 9, 4))
    for j, (a, b) in enumerate(pairs):
        hi, lo = max(a, b), min(a, b)
        for w, psi in branches:
            out[j] += w * setting_probs(np.repeat(psi, 9, axis=0), n, hi, lo, effects, np.arange(9))
    return out


# ---- the model and programs the tests share ------------------------------------------------------
T1 = 50e3


def model(t2=70e3, readout=True):
    """test_gpu_trajectories._model (relaxation after rx / ry / rz and on both qubits of cx); with
    ``readout`` also errors on h, sdg and measure, one of them local to a qubit."""
    from adaptaqc_amd import noise

    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(noise.thermal_relaxation_error(T1, t2, 5000), ["rx", "ry", "rz"])
    two = noise.thermal_relaxation_error(T1, t2, 15000)
    nm.add_all_qubit_quantum_error(two.expand(two), "cx")
    if readout:
        nm.add_all_qubit_quantum_error(noise.thermal_relaxation_error(T1, t2, 6000), "h")
        nm.add_all_qubit_quantum_error(noise.depolarizing_error(0.03), "sdg")
        nm.add_all_qubit_quantum_error(noise.thermal_relaxation_error(T1, t2, 20000), "measure")
        nm.add_quantum_error(noise.phase_damping_error(0.1), "h", (1,))
    return nm


def kraus_of(noise_model):
    """The ``kraus_of(name, q)`` of readout_effects_ref for a NoiseModel."""
    def lookup(name, q):
        return [k for _, e in noise_model.channels(name, (q,)) for k in e.kraus] if noise_model is not None else []

    return lookup


def program(n, depth, t2=70e3, readout=True):
    """(circuit, rows, n_events, effects) of the seeded brickwork of the trajectory tests under model()."""
    import sampling_ref as ref
    from adaptaqc_amd.noise import trajectory_program
    from conftest import to_circuit

    qc = to_circuit(n, ref.brickwork(n, depth, 100 + n))
    nm = model(t2, readout)
    rows, n_events, _ = trajectory_program(qc, nm)
    return qc, rows, n_events, readout_effects_ref(n, kraus_of(nm))
