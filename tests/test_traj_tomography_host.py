"""Noisy pair tomography, the host side (no GPU): the POVM effects of noise.readout_effects, and the
numpy restatement of tests/traj_tomography_ref.py against the density-matrix evolution of the
reference's nine rotated circuits."""
import itertools

import numpy as np
import pytest

import sampling_ref as ref
import tomography_ref as tomo
import traj_tomography_ref as ttref
import trajectory_ref as tref
from conftest import to_circuit


def test_readout_effects_equal_the_restatement():
    from adaptaqc_amd.noise import readout_effects

    n = 4
    for nm in (ttref.model(70e3), ttref.model(30e3), ttref.model(70e3, readout=False)):
        got = readout_effects(n, nm)
        assert got.shape == (n, 3, 2, 4) and got.dtype == np.float64
        assert np.max(np.abs(got - ttref.readout_effects_ref(n, ttref.kraus_of(nm)))) < 1e-15
    # the local error on h of qubit 1 replaces the all-qubit one there, and nowhere else
    got = readout_effects(n, ttref.model())
    assert np.max(np.abs(got[1, 0] - got[0, 0])) > 1e-3
    assert np.array_equal(got[2], got[0]) and np.array_equal(got[1, 2], got[0, 2])


def test_effects_without_a_model_are_the_projectors():
    from adaptaqc_amd import noise

    identity = noise.NoiseModel()
    identity.add_all_qubit_quantum_error(noise.thermal_relaxation_error(50.0, 70.0, 0.0), ["h", "sdg", "measure"])
    for nm in (None, noise.NoiseModel(), identity, ttref.model(readout=False)):
        got = noise.readout_effects(3, nm)
        for q, b, o in itertools.product(range(3), range(3), range(2)):
            v = tomo.eigvec(b, o)
            assert np.max(np.abs(ttref.unpack(got[q, b, o]) - np.outer(v, v.conj()))) < 1e-15


def test_effects_sum_to_the_identity_and_are_positive():
    from adaptaqc_amd.noise import readout_effects

    got = readout_effects(3, ttref.model(30e3))
    for q, b in itertools.product(range(3), range(3)):
        e0, e1 = ttref.unpack(got[q, b, 0]), ttref.unpack(got[q, b, 1])
        assert np.max(np.abs(e0 + e1 - np.eye(2))) < 1e-15
        assert min(np.linalg.eigvalsh(e0)[0], np.linalg.eigvalsh(e1)[0]) > -1e-15


def test_exact_tables_follow_the_nine_rotated_circuits():
    """The effects formula against the reference's own procedure: per pair and setting the circuit
    with its basis rotations and measure(lo -> 0), measure(hi -> 1), through trajectory_program and
    the density-matrix evolution; the marginal of its diagonal over the pair's two bits."""
    from adaptaqc_amd.noise import readout_effects, trajectory_program
    from adaptaqc_amd.utils.circuit_operations import add_pauli_measurement_rotations

    n = 5
    nm = ttref.model()
    base = to_circuit(n, ref.brickwork(n, 3, 100 + n))
    pairs = [(0, 1), (4, 1), (2, 4)]
    rows, n_events, _ = trajectory_program(base, nm)
    assert n_events > 0
    got = ttref.exact_tables(n, rows, pairs, readout_effects(n, nm))
    worst = 0.0
    for j, (a, b) in enumerate(pairs):
        hi, lo = max(a, b), min(a, b)
        for s in range(9):
            label = ["I"] * n
            label[n - 1 - hi] = "XYZ"[s // 3]
            label[n - 1 - lo] = "XYZ"[s % 3]
            rotated = base.copy()
            add_pauli_measurement_rotations(rotated, "".join(label))
            rotated.measure(lo, 0)
            rotated.measure(hi, 1)
            diag = np.real(np.diag(tref.density_matrix(n, trajectory_program(rotated, nm)[0])))
            idx = np.arange(2 ** n)
            o = 2 * ((idx >> hi) & 1) + ((idx >> lo) & 1)
            want = np.bincount(o, weights=diag, minlength=4)
            worst = max(worst, float(np.max(np.abs(got[j, s] - want))))
    print(f"largest difference in an outcome probability: {worst:.2e}")
    assert worst < 1e-12
    assert np.max(np.abs(got.sum(axis=2) - 1)) < 1e-12
    # the noise is visible in these tables
    clean = ttref.exact_tables(n, trajectory_program(base, None)[0], pairs, readout_effects(n, None))
    assert np.max(np.abs(got - clean)) > 1e-2


def test_kraus_branches_of_the_restatement_sum_to_the_exact_tables():
    """Two Kraus events on two qubits: the restatement's per-trajectory probabilities, weighted over
    every sequence of Kraus choices, are the density matrix's."""
    from adaptaqc_amd import noise
    from adaptaqc_amd.circuit import QuantumCircuit

    qc = QuantumCircuit(2)
    qc.ry(0.8, 0)
    qc.cx(0, 1)
    nm = ttref.model()
    rows, n_events, _ = noise.trajectory_program(qc, nm)
    assert n_events == 3
    rows = rows[:-1]  # two events: drop the last Kraus row (on the cx's second qubit)
    assert int(np.count_nonzero(rows["flags"] == 1)) == 2
    effects = noise.readout_effects(2, nm)
    want = ttref.exact_tables(2, rows, [(1, 0)], effects)
    got = ttref.branch_tables(2, rows, [(1, 0)], effects)
    assert np.max(np.abs(got - want)) < 1e-12
    # and the restatement's shots follow that law: outcomes drawn by it from given uniforms
    shots = 2000
    u = ref.uniforms(3, 0, 9 * shots, 2 + 1)
    outcomes, counts, near = ttref.pair_tomography(2, rows, [(1, 0)], effects, u)
    assert counts.sum(axis=2).tolist() == [[shots] * 9] and not near.any()
    assert np.array_equal(counts, ttref.counts_of(outcomes))
    assert np.max(np.abs(counts[0] / shots - want[0])) < 6 * 0.5 / np.sqrt(shots)


def test_default_backend_still_refuses_a_noise_model():
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator

    qc = to_circuit(3, ref.brickwork(3, 1, 1))
    be = QiskitSamplingBackend(SamplingSimulator(), tomography="device")
    assert be.trajectory_tomography is False
    with pytest.raises(NotImplementedError, match="noise_model") as err:
        be.pair_tomography(qc, [(0, 1)], {"shots": 100, "noise_model": ttref.model()})
    assert "trajectory_tomography" in str(err.value)
    flagged = QiskitSamplingBackend(SamplingSimulator(), tomography="device", trajectory_tomography=True)
    with pytest.raises(NotImplementedError, match="noise_model"):
        flagged.concurrence_lower_bounds(qc, [(0, 1)], {"shots": 100, "noise_model": ttref.model()})


def test_flag_needs_the_device_route():
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator

    for mode in (None, "circuits"):
        with pytest.raises(TypeError, match="trajectory_tomography"):
            QiskitSamplingBackend(SamplingSimulator(), tomography=mode, trajectory_tomography=True)
    assert QiskitSamplingBackend(SamplingSimulator(), tomography="device", trajectory_tomography=True).trajectory_tomography
