"""The noisy Pauli readout, the host side (no GPU): the parity operators of tests/pauli_traj_ref.py
against the density-matrix evolution of the reference's per-term circuits, the argument checks of
aqc_sv_traj_pauli_counts, and the ``pauli_terms`` option of QiskitSamplingBackend."""
import ctypes

import numpy as np
import pytest

import pauli_traj_ref as pref
import sampling_ref as ref
import traj_tomography_ref as ttref
import trajectory2_ref as t2ref
import trajectory_ref as tref
from conftest import to_circuit

PAULI = {1: np.array([[0, 1], [1, 0]], dtype=complex), 2: np.array([[0, -1j], [1j, 0]]), 3: np.diag([1.0 + 0j, -1.0])}


def _codes(labels, n):
    from adaptaqc_amd.paulis import terms_to_codes

    return terms_to_codes(labels, n)


def test_kraus_branches_of_the_restatement_average_to_the_exact_values():
    """2 qubits, a one-qubit event and a correlated group: the restatement's per-trajectory values,
    weighted over every sequence of Kraus choices, are Tr(rho M); and its draws follow that law."""
    from adaptaqc_amd import noise
    from adaptaqc_amd.circuit import QuantumCircuit

    qc = QuantumCircuit(2)
    qc.ry(0.8, 0)
    qc.cx(0, 1)
    qc.rx(0.3, 1)
    nm = t2ref.model("b")
    rows, n_events, _ = noise.trajectory_program(qc, nm)
    assert n_events == 3 and noise.has_correlated_rows(rows)
    effects = noise.readout_effects(2, ttref.model())
    codes = _codes(["IX", "ZI", "XY", "ZZ", "YX"], 2)
    want = pref.exact_values(2, rows, codes, effects)
    got = pref.branch_values(2, rows, codes, effects)
    assert np.max(np.abs(got - want)) < 1e-12
    shots = 4000
    u = ref.uniforms(5, 0, shots, n_events + len(codes))
    v, outcomes, plus, near = pref.pauli_counts(2, rows, codes, effects, u)
    assert v.shape == outcomes.shape == near.shape == (shots, len(codes)) and not near.any()
    assert np.array_equal(plus, pref.plus_of(outcomes)) and np.all(np.abs(v) <= 1 + 1e-12)
    p = (1 + want) / 2
    assert np.all(np.abs(plus / shots - p) <= 6 * np.sqrt(p * (1 - p) / shots))


def test_exact_values_follow_the_rotated_circuits():
    """The parity operator against the reference's own procedure: per term the circuit with its basis
    rotations and a measure on every qubit, through trajectory_program and the density-matrix evolution;
    the parity of the term's support averaged over its diagonal."""
    from adaptaqc_amd.noise import readout_effects, trajectory_program
    from adaptaqc_amd.utils.circuit_operations import add_pauli_measurement_rotations

    n = 4
    nm = ttref.model()
    base = to_circuit(n, ref.brickwork(n, 3, 100 + n))
    labels = ["IIXI", "ZIIY", "XYZI", "YYXZ", "ZZII"]
    codes = _codes(labels, n)
    rows, n_events, _ = trajectory_program(base, nm)
    assert n_events > 0
    got = pref.exact_values(n, rows, codes, readout_effects(n, nm))
    idx = np.arange(2 ** n)
    for j, label in enumerate(labels):
        rotated = base.copy()
        add_pauli_measurement_rotations(rotated, label)
        for q in range(n):
            rotated.measure(q, q)
        diag = np.real(np.diag(tref.density_matrix(n, trajectory_program(rotated, nm)[0])))
        parity = np.zeros(2 ** n, dtype=int)
        for q in np.flatnonzero(codes[j]):
            parity ^= (idx >> q) & 1
        want = float(np.sum(diag * (1 - 2 * parity)))
        assert abs(got[j] - want) < 1e-12, label
    clean = pref.exact_values(n, trajectory_program(base, None)[0], codes, readout_effects(n, None))
    assert np.max(np.abs(got - clean)) > 1e-2  # the noise is visible in these values


def test_factors_without_a_model_are_the_paulis():
    from adaptaqc_amd import noise

    for nm in (None, noise.NoiseModel(), ttref.model(readout=False)):
        effects = noise.readout_effects(3, nm)
        for q in range(3):
            for c in (1, 2, 3):
                assert np.max(np.abs(pref.factor(effects, q, c) - PAULI[c])) < 1e-15
    # so M of a label is the Pauli string
    m = pref.parity_operator(3, _codes(["XIY"], 3)[0], noise.readout_effects(3, None))
    assert np.max(np.abs(m - np.kron(PAULI[1], np.kron(np.eye(2), PAULI[2])))) < 1e-15


def test_relaxation_on_the_readout_gives_an_identity_part():
    """Why the kernel takes general Hermitian factors: under create_noisemodel, relaxation during
    ``measure`` gives E0 = diag(1, g), E1 = diag(0, 1 - g), and no D_q is a multiple of a Pauli matrix."""
    from adaptaqc_amd.noise import readout_effects
    from adaptaqc_amd.utils.circuit_operations import create_noisemodel

    effects = readout_effects(2, create_noisemodel(0.05, 0.07, log_fidelities=False))
    g = -np.expm1(-1000 / 50e3)
    assert np.allclose(ttref.unpack(effects[0, 2, 0]), np.diag([1.0, g]), atol=1e-15)
    assert np.allclose(ttref.unpack(effects[0, 2, 1]), np.diag([0.0, 1 - g]), atol=1e-15)
    for c in (1, 2, 3):
        d = pref.factor(effects, 0, c)
        assert abs(np.trace(d).real / 2) > 1e-3, c  # the identity part
        assert abs(np.trace(d @ PAULI[c]).real / 2) > 0.9  # beside most of the Pauli


def test_dense_operator_and_factor_by_factor_agree():
    n = 4
    _, rows, n_events, effects = ttref.program(n, 2)
    u = ref.uniforms(9, 0, 3, n_events)
    psi = t2ref.evolve(n, rows, u)[0]
    for row in _codes(["XYZI", "IIIZ", "YXXY"], n):
        want = psi @ pref.parity_operator(n, row, effects).T
        assert np.max(np.abs(pref.apply_parity(psi, n, row, effects) - want)) < 1e-14


def _call(lib, n, rows, codes, nterms, effects, nshots, u=None, plus=True):
    from adaptaqc_amd import _lib

    out = np.zeros(max(nterms, 1), dtype=np.int64)
    return lib.aqc_sv_traj_pauli_counts(n, _lib.ptr(rows), len(rows), _lib.ptr(codes), nterms, _lib.ptr(effects), nshots,
                                        ctypes.c_uint64(1), ctypes.c_uint64(0), _lib.ptr(u),
                                        _lib.ptr(out) if plus else None, None, None)


def test_malformed_arguments_answer_err_arg_on_the_host():
    """Every check runs before any device call: AQC_ERR_ARG (-1) without a GPU."""
    from adaptaqc_amd import _lib, noise

    lib = _lib.load()  # (does not touch the GPU)
    n = 5
    _, rows, n_events, noisy = ttref.program(n, 1)
    rows = np.ascontiguousarray(rows)
    noisy = np.ascontiguousarray(noisy)
    clean = np.ascontiguousarray(noise.readout_effects(n, None))
    ok = _codes(["IIXZY", "ZIIII"], n)

    def bad_code():
        c = ok.copy()
        c[1, 2] = 4
        return c

    def bad_rows():
        r = rows.copy()
        r["flags"][0] = 7
        return r

    def bad_effects():
        e = clean.copy()
        e[2, 1, 0, 0] += 1e-6
        return e

    u = np.full((4, n_events + 2), 0.5)
    u_bad = u.copy()
    u_bad[3, -1] = 1.0
    wide = np.zeros((1, 25), dtype=np.uint8)
    wide[0, 0] = 3
    cases = {
        "n = 0": lambda: _call(lib, 0, rows[:0], ok, 2, clean, 4),
        "n = 25": lambda: _call(lib, 25, rows[:0], wide, 1, np.ascontiguousarray(noise.readout_effects(25, None)), 4),
        "nterms = 0": lambda: _call(lib, n, rows, ok, 0, clean, 4),
        "nterms = 65537": lambda: _call(lib, n, rows, ok, 65537, clean, 4),
        "nshots = 0": lambda: _call(lib, n, rows, ok, 2, clean, 0),
        "nshots = 2^30 + 1": lambda: _call(lib, n, rows, ok, 2, clean, 2 ** 30 + 1),
        "a code above 3": lambda: _call(lib, n, rows, bad_code(), 2, clean, 4),
        "an all-identity term": lambda: _call(lib, n, rows, _codes(["IIXZY", "IIIII"], n), 2, clean, 4),
        "5 general factors": lambda: _call(lib, n, rows, _codes(["XYZXZ"], n), 1, noisy, 4),
        "effects that do not sum to I": lambda: _call(lib, n, rows, ok, 2, bad_effects(), 4),
        "a u outside [0, 1)": lambda: _call(lib, n, rows, ok, 2, clean, 4, u=u_bad),
        "a malformed row": lambda: _call(lib, n, bad_rows(), ok, 2, clean, 4),
        "no plus": lambda: _call(lib, n, rows, ok, 2, clean, 4, plus=False),
        "no codes": lambda: _call(lib, n, rows, None, 2, clean, 4),
        "no effects": lambda: _call(lib, n, rows, ok, 2, None, 4),
    }
    for label, call in cases.items():
        assert call() == -1, label
    assert _call(lib, n, rows, _codes(["XYZXZ"], n), 1, noisy, 4) == -1
    assert "4" in lib.aqc_last_error().decode() and "general" in lib.aqc_last_error().decode()


class _CountingSimulator:
    """Any simulator that honours ``run().result().get_counts()``: every shot reads all zeros."""

    def __init__(self):
        self.circuits = []

    def run(self, circuit, shots=1024, **kwargs):
        from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingJob, SamplingResult

        self.circuits.append(circuit)
        return SamplingJob(SamplingResult({"0" * circuit.num_qubits: int(shots)}))


def test_pauli_terms_validation():
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator

    assert QiskitSamplingBackend(SamplingSimulator()).pauli_terms is None
    assert QiskitSamplingBackend(SamplingSimulator(), pauli_terms="device").pauli_terms == "device"
    for bad in ("circuits", "Device", True, 1):
        with pytest.raises(ValueError, match="pauli_terms"):
            QiskitSamplingBackend(SamplingSimulator(), pauli_terms=bad)
    with pytest.raises(TypeError, match="pauli_counts"):
        QiskitSamplingBackend(_CountingSimulator(), pauli_terms="device")
    sim = SamplingSimulator()
    with pytest.raises(ValueError, match="all-identity"):
        sim.pauli_counts(to_circuit(2, [("h", (0,), ())]), ["XI", "II"], shots=10)
    assert sim.runs == 0


def test_default_route_still_runs_one_circuit_per_term():
    """pauli_terms=None: the simulator sees one run per non-identity term, each with the term's
    rotations and a measure on every qubit -- today's route, untouched."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend
    from adaptaqc_amd.utils.circuit_operations import expectation_value_of_pauli_operator, expectation_values_of_pauli_terms

    n = 3
    qc = to_circuit(n, ref.brickwork(n, 1, 3))
    sim = _CountingSimulator()
    be = QiskitSamplingBackend(sim)
    labels = ["XIZ", "III", "IYI", "ZZZ"]
    got = expectation_values_of_pauli_terms(qc, labels, be, execute_kwargs={"shots": 50, "noise_model": ttref.model()})
    assert len(sim.circuits) == 3 and got.tolist() == [1.0, 1.0, 1.0, 1.0]
    for circuit, label in zip(sim.circuits, ["XIZ", "IYI", "ZZZ"]):
        names = [ins.operation.name for ins in circuit.data][len(qc.data):]
        want = {"XIZ": ["h"], "IYI": ["sdg", "h"], "ZZZ": []}[label] + ["measure"] * n
        assert names == want, label
    value = expectation_value_of_pauli_operator(qc, {"XIZ": 0.5, "III": 2.0}, be, execute_kwargs={"shots": 50})
    assert len(sim.circuits) == 4 and value == 2.5
