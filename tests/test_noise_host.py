"""Host side of noisy sampling: the noise model (adaptaqc_amd/noise.py), the trajectory program and
the reference's create_noisemodel / zero_noise_extrapolate.  No GPU needed."""
import pickle

import numpy as np
import pytest

import trajectory_ref as tref
from adaptaqc_amd import noise
from adaptaqc_amd.circuit import QuantumCircuit
from adaptaqc_amd.utils import circuit_operations as co


def _channel(err, rho):
    return sum(k @ rho @ k.conj().T for k in err.kraus)


def _complete(err):
    return np.max(np.abs(sum(k.conj().T @ k for k in err.kraus) - np.eye(2)))


@pytest.mark.parametrize("err", [
    noise.thermal_relaxation_error(50e3, 70e3, 5000), noise.thermal_relaxation_error(50e3, 30e3, 300),
    noise.thermal_relaxation_error(50e3, 100e3, 1000), noise.thermal_relaxation_error(1.0, 1.0, 0.0),
    noise.amplitude_damping_error(0.3), noise.phase_damping_error(0.2), noise.depolarizing_error(0.1),
    noise.pauli_error([("X", 0.25), ("I", 0.5), ("Z", 0.25)]),
])
def test_kraus_completeness(err):
    assert 1 <= len(err.kraus) <= 4 and all(k.shape == (2, 2) for k in err.kraus)
    assert _complete(err) < 1e-12


def test_quantum_error_validation():
    with pytest.raises(ValueError):
        noise.QuantumError([0.9 * np.eye(2)])
    with pytest.raises(ValueError):
        noise.QuantumError([np.eye(2) / np.sqrt(5)] * 5)
    with pytest.raises(NotImplementedError):
        noise.QuantumError([np.eye(4)])
    assert noise.QuantumError([np.eye(2)]).is_identity()
    assert noise.thermal_relaxation_error(50.0, 70.0, 0).is_identity()
    assert noise.pauli_error([("I", 1.0)]).is_identity()
    assert not noise.depolarizing_error(0.01).is_identity()
    a, b = noise.amplitude_damping_error(0.1), noise.phase_damping_error(0.2)
    assert a.expand(b).pair == (a, b) and a.tensor(b).pair == (b, a) and a.expand(b).num_qubits == 2
    with pytest.raises(NotImplementedError):
        a.expand(b).expand(a)
    with pytest.raises(ValueError):
        noise.pauli_error([("X", 0.5)])
    # depolarizing: rho -> (1 - p) rho + p I / 2
    rho = np.array([[0.7, 0.2 - 0.1j], [0.2 + 0.1j, 0.3]])
    np.testing.assert_allclose(_channel(noise.depolarizing_error(0.3), rho), 0.7 * rho + 0.3 * np.eye(2) / 2, atol=1e-14)


@pytest.mark.parametrize("t1,t2", [(50e3, 30e3), (50e3, 70e3), (50e3, 100e3)])
def test_thermal_relaxation_map(t1, t2):
    """rho11 -> e^(-t/T1) rho11 and rho01 -> e^(-t/T2) rho01, for t2 < t1 and t1 < t2 <= 2 t1."""
    time = 7000.0
    rho = np.array([[0.35, 0.3 + 0.2j], [0.3 - 0.2j, 0.65]])
    out = _channel(noise.thermal_relaxation_error(t1, t2, time), rho)
    assert abs(out[1, 1] - np.exp(-time / t1) * rho[1, 1]) < 1e-14
    assert abs(out[0, 1] - np.exp(-time / t2) * rho[0, 1]) < 1e-14
    assert abs(np.trace(out) - 1) < 1e-14 and abs(out[1, 0] - np.conj(out[0, 1])) < 1e-15


def test_thermal_relaxation_refusals():
    for bad in ((50.0, 101.0, 1.0), (0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (50.0, 70.0, -1.0)):
        with pytest.raises(ValueError):
            noise.thermal_relaxation_error(*bad)


def test_create_noisemodel_names_and_times():
    nm = co.create_noisemodel(50e-3, 70e-3, log_fidelities=True)
    t1, t2 = 50e3, 70e3
    table = nm.instructions()
    want = {0: ["u1", "p", "rz", "z", "s", "sdg", "t", "tdg"], 50: ["u2", "h", "sx", "sxdg"],
            100: ["u3", "u", "rx", "ry", "x", "y"], 1000: ["measure", "reset"]}
    assert set(table) == {n for names in want.values() for n in names} | {"cx"}
    for time, names in want.items():
        for name in names:
            err = table[name]
            assert err.num_qubits == 1
            assert abs(err.kraus[0][1, 1] - np.exp(-time / t2)) < 1e-15, name
            assert abs(err.kraus[1][0, 1] ** 2 - (1 - np.exp(-time / t1))) < 1e-15, name
    cx = table["cx"]
    assert cx.num_qubits == 2
    for half in cx.pair:
        assert abs(half.kraus[0][1, 1] - np.exp(-300 / t2)) < 1e-15
    assert table["rz"].is_identity() and not table["h"].is_identity()
    assert nm.channels("cz", (0, 1)) == [] and nm.channels("rz", (0,)) == []
    assert [q for q, _ in nm.channels("cx", (3, 1))] == [3, 1]
    # the no-jump weight that is logged as the fidelity
    assert abs(table["x"].no_jump_weight() - (1 + np.exp(-2 * 100 / t2)) / 2) < 1e-15


def test_noise_model_lookup_and_refusals():
    nm = noise.NoiseModel()
    a, b = noise.amplitude_damping_error(0.1), noise.phase_damping_error(0.2)
    nm.add_all_qubit_quantum_error(a, ["h", "cx", "ccx"])
    nm.add_quantum_error(b, "h", [2])
    nm.add_quantum_error(a.expand(b), "cz", [0, 1])
    assert nm.channels("h", (0,)) == [(0, a)] and nm.channels("h", (2,)) == [(2, b)]
    assert nm.channels("cx", (1, 0)) == [(1, a), (0, a)]  # a one-qubit error on both qubits
    assert nm.channels("cz", (0, 1)) == [(0, a), (1, b)] and nm.channels("cz", (1, 0)) == []
    with pytest.raises(NotImplementedError):
        nm.channels("ccx", (0, 1, 2))
    nm.add_all_qubit_quantum_error(a.expand(b), "x")
    with pytest.raises(ValueError):
        nm.channels("x", (0,))


def test_trajectory_program_rows():
    a, b = noise.amplitude_damping_error(0.1), noise.phase_damping_error(0.2)
    m = noise.depolarizing_error(0.05)
    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(a, "h")
    nm.add_all_qubit_quantum_error(a.expand(b), "cx")
    nm.add_all_qubit_quantum_error(noise.thermal_relaxation_error(5.0, 5.0, 0.0), "rz")  # identity: no row
    nm.add_all_qubit_quantum_error(m, "measure")
    nm.add_all_qubit_quantum_error(b.tensor(noise.QuantumError([np.eye(2)])), "cz")
    qc = QuantumCircuit(3)
    qc.h(1)
    qc.rz(0.3, 0)
    qc.cx(2, 0)
    qc.x(1)
    qc.cz(0, 1)  # tensor: b on the second listed qubit, the identity on the first
    qc.measure(2, 0)
    qc.measure(0, 1)
    rows, n_events, measured = noise.trajectory_program(qc, nm)
    assert measured == {2: 0, 0: 1} and n_events == 6
    got = [(int(r["flags"]), int(r["nq"]), int(r["q0"]), int(r["q1"])) for r in rows]
    assert got == [(0, 1, 1, 0), (1, 1, 1, 2),        # h(1), a on 1
                   (0, 1, 0, 0),                      # rz(0): its channel is the identity
                   (0, 2, 2, 0), (1, 1, 2, 2), (1, 1, 0, 2),  # cx(2, 0): a on 2, then b on 0
                   (0, 1, 1, 0),                      # x(1): no error attached
                   (0, 2, 0, 1), (1, 1, 1, 2),        # cz(0, 1): b on qubit 1 only
                   (1, 1, 2, 4), (1, 1, 0, 4)]        # the measures, in circuit order, last
    k = rows[5]["m"][:16].view(np.complex128).reshape(2, 2, 2)
    np.testing.assert_array_equal(k, np.stack(b.kraus))
    # no model / an all-identity model: gate rows only
    for model in (None, noise.NoiseModel()):
        r0, e0, _ = noise.trajectory_program(qc, model)
        assert e0 == 0 and len(r0) == 5 and not r0["flags"].any()
    # the density-matrix restatement keeps the trace and shows the damping
    rho = tref.density_matrix(3, rows)
    assert abs(np.trace(rho) - 1) < 1e-12 and np.max(np.abs(rho - rho.conj().T)) < 1e-12
    nm3 = noise.NoiseModel()
    nm3.add_all_qubit_quantum_error(a, "ccx")
    q3 = QuantumCircuit(3)
    q3.ccx(0, 1, 2)
    with pytest.raises(NotImplementedError):
        noise.trajectory_program(q3, nm3)
    assert noise.trajectory_program(q3, nm)[1] == 0  # no error attached: noiseless, 15 gate rows
    mid = QuantumCircuit(2)
    mid.measure(0, 0)
    mid.h(0)
    with pytest.raises(NotImplementedError):
        noise.trajectory_program(mid, nm)


def test_restatement_agrees_with_density_matrix():
    """The trajectory restatement's outcome frequencies follow the density matrix's diagonal
    (chi-square below dof + 6 sqrt(2 dof)), and not the noiseless |psi|^2."""
    import sampling_ref as ref
    from conftest import to_circuit

    n, shots = 3, 4096
    err = noise.thermal_relaxation_error(50e3, 70e3, 5000)
    err2 = noise.thermal_relaxation_error(50e3, 70e3, 15000)
    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(err, ["rx", "ry", "rz"])
    nm.add_all_qubit_quantum_error(err2.expand(err2), "cx")
    qc = to_circuit(n, ref.brickwork(n, 3, 100 + n))
    rows, n_events, _ = noise.trajectory_program(qc, nm)
    u = ref.uniforms(2 ** 40 + 3 + n, 1, shots, n_events + 1)
    out, choices, near = tref.trajectories(n, rows, u)
    assert near.sum() == 0 and choices.max() <= 2 and choices.any()
    probs = np.real(np.diag(tref.density_matrix(n, rows)))
    stat, dof = ref.chi_square(tref.counts_array(out, n), probs, shots)
    assert stat < dof + 6 * np.sqrt(2 * dof)
    clean = np.real(np.diag(tref.density_matrix(n, noise.trajectory_program(qc, None)[0])))
    stat0, dof0 = ref.chi_square(tref.counts_array(out, n), clean, shots)
    assert stat0 > dof0 + 6 * np.sqrt(2 * dof0)


def _cx_chain(ncx):
    qc = QuantumCircuit(2)
    qc.h(0)
    for _ in range(ncx):
        qc.cx(0, 1)
    qc.rz(0.1, 1)
    return qc


def test_zero_noise_extrapolate_fit_and_restore():
    a, b, c = 0.2, 0.7, 40.0
    qc = _cx_chain(20)
    before = list(qc.data)
    seen = []

    def measure():
        ncx = sum(ins.operation.name == "cx" for ins in qc.data)
        seen.append(ncx)
        return a + b * np.exp(-ncx / c)

    got = co.zero_noise_extrapolate(qc, measure, num_points=10, rng=np.random.default_rng(5))
    assert qc.data == before and all(x is y for x, y in zip(qc.data, before))
    assert seen[0] == 20 and seen[-1] == 60 and len(seen) == 10 and all(s % 2 == 0 for s in seen)
    # the function's own fit of the values it saw, restated
    from scipy.optimize import curve_fit

    def f(x, i, amp, d):
        return i + amp * np.exp(-x / d)

    vals = [a + b * np.exp(-s / c) for s in seen]
    popt, _ = curve_fit(f, np.linspace(0, 1, 10), vals, [0, vals[0], 1])
    assert abs(got - f(-0.5, *popt)) < 1e-9
    # the values fall with the number of cx, so the extrapolation to x = -0.5 lies above the measured one
    assert got > vals[0]
    # without an rng numpy's global generator is used, as in the reference
    np.random.seed(1)
    assert np.isfinite(co.zero_noise_extrapolate(qc, measure, num_points=5))
    assert qc.data == before


def test_zero_noise_extrapolate_fit_failure(monkeypatch):
    import scipy.optimize

    def failing(*args, **kwargs):
        raise RuntimeError("Optimal parameters not found")

    monkeypatch.setattr(scipy.optimize, "curve_fit", failing)
    qc = _cx_chain(3)
    calls = []

    def measure():
        calls.append(len(qc.data))
        return 0.25

    assert co.zero_noise_extrapolate(qc, measure, num_points=4, rng=np.random.default_rng(0)) == 0.25
    assert len(calls) == 5 and calls[-1] == 5  # once more after the failure, on the restored circuit


def test_noise_model_pickles():
    nm = co.create_noisemodel(50e-3, 70e-3, log_fidelities=False)
    nm.add_quantum_error(noise.depolarizing_error(0.1), "cz", [0, 1])
    back = pickle.loads(pickle.dumps(nm))
    qc = _cx_chain(2)
    qc.measure(0, 0)
    r0, e0, m0 = noise.trajectory_program(qc, nm)
    r1, e1, m1 = noise.trajectory_program(qc, back)
    assert e0 == e1 == 6 and m0 == m1 and r0.tobytes() == r1.tobytes()
    assert [q for q, _ in back.channels("cz", (0, 1))] == [0, 1]
