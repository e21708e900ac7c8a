"""Noisy shot sampling on the device (csrc/traj.hip, aqc_sv_traj_sample) against the numpy restatements
of tests/trajectory_ref.py, and through SamplingSimulator / QiskitSamplingBackend."""
import numpy as np
import pytest

import sampling_ref as ref
import trajectory_ref as tref
from conftest import FakeCompiler, to_circuit

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 3
T1 = 50e3


def _ops(n, depth):
    if n == 1:
        return [("rx", (0,), (0.7,)), ("rz", (0,), (1.1,))]
    return ref.brickwork(n, depth, 100 + n)


def _model(t2=70e3):
    """Thermal relaxation for 5000 after every one-qubit gate and 15000 on both qubits of cx."""
    from adaptaqc_amd import noise

    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(noise.thermal_relaxation_error(T1, t2, 5000), ["rx", "ry", "rz"])
    two = noise.thermal_relaxation_error(T1, t2, 15000)
    nm.add_all_qubit_quantum_error(two.expand(two), "cx")
    return nm


def _program(n, depth, t2=70e3):
    from adaptaqc_amd.noise import trajectory_program

    qc = to_circuit(n, _ops(n, depth))
    rows, n_events, _ = trajectory_program(qc, _model(t2))
    return qc, rows, n_events


# (n, depth, shots, t2): the smallest state; more shots than workgroups; t2 on either side of t1; the
# pair count against the thread count (9, 10); the largest LDS-resident state; the first global one
CASES = [(1, 0, 512, 70e3), (3, 3, 4097, 70e3), (5, 3, 2048, 70e3), (5, 3, 2048, 30e3), (9, 2, 300, 70e3),
         (10, 2, 256, 70e3), (13, 2, 64, 70e3), (14, 2, 32, 70e3)]


@pytest.mark.parametrize("n,depth,shots,t2", CASES)
def test_shot_by_shot_against_restatement(n, depth, shots, t2):
    """Outcome and Kraus choices of every shot (not flagged near a boundary) equal the restatement's,
    with u passed in and with u drawn on the device from (seed, run)."""
    from adaptaqc_amd.device import trajectory_sample

    _, rows, n_events = _program(n, depth, t2)
    assert n_events > 0
    seed, run = SEED + n, 1
    u = ref.uniforms(seed, run, shots, n_events + 1)
    want, want_k, near = tref.trajectories(n, rows, u)
    print(f"n={n} shots={shots} rows={len(rows)} events={n_events} near={int(near.sum())}")
    assert near.sum() <= 2
    keep = ~near
    for kwargs in ({"u": u}, {}):
        got, got_k = trajectory_sample(n, rows, n_events, shots, seed, run, return_choices=True, **kwargs)
        assert got.dtype == np.uint64 and got.shape == (shots,) and got_k.shape == (shots, n_events)
        bad = np.flatnonzero((got.astype(np.int64) != want) & keep)
        assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
        assert np.array_equal(got_k[keep], want_k[keep])
    assert np.array_equal(trajectory_sample(n, rows, n_events, shots, seed, run), got)  # without choices


def _counts_to_array(counts, n):
    out = np.zeros(2 ** n, dtype=np.int64)
    for key, c in counts.items():
        out[int(key, 2)] = c
    return out


def test_distribution_follows_the_density_matrix():
    """65536 noisy shots through SamplingSimulator.run: Pearson chi-square against the diagonal of
    the density-matrix evolution below dof + 6 sqrt(2 dof); against the noiseless |psi|^2 above it."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.noise import trajectory_program

    n, shots = 5, 65536
    qc, rows, _ = _program(n, 3)
    counts = SamplingSimulator(seed=SEED).run(qc, shots=shots, noise_model=_model()).result().get_counts()
    obs = _counts_to_array(counts, n)
    assert obs.sum() == shots
    probs = np.real(np.diag(tref.density_matrix(n, rows)))
    stat, dof = ref.chi_square(obs, probs, shots)
    clean = np.real(np.diag(tref.density_matrix(n, trajectory_program(qc, None)[0])))
    stat0, dof0 = ref.chi_square(obs, clean, shots)
    print(f"chi-square noisy {stat:.1f} at {dof} dof, against the noiseless law {stat0:.1f} at {dof0} dof")
    assert stat < dof + 6 * np.sqrt(2 * dof)
    assert stat0 > dof0 + 6 * np.sqrt(2 * dof0)


def test_known_answers():
    """x(0) followed by relaxation for a time far beyond T1 reads 0 in every shot; for time 0, 1."""
    from adaptaqc_amd import noise
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.circuit import QuantumCircuit
    from adaptaqc_amd.device import trajectory_sample

    qc = QuantumCircuit(2)
    qc.x(0)
    for time, key in ((1e6, "00"), (0.0, "01")):
        nm = noise.NoiseModel()
        nm.add_all_qubit_quantum_error(noise.thermal_relaxation_error(50.0, 70.0, time), "x")
        counts = SamplingSimulator(seed=3).run(qc, shots=1000, noise_model=nm).result().get_counts()
        assert counts == {key: 1000}
    # a program without a Kraus row on the trajectory kernel itself
    rows, n_events, _ = noise.trajectory_program(qc, None)
    assert n_events == 0
    out, choices = trajectory_sample(2, rows, 0, 100, 1, return_choices=True)
    assert np.all(out == 1) and choices.shape == (100, 0)


def test_determinism_and_runs():
    from adaptaqc_amd.device import trajectory_sample

    n, shots = 6, 3000
    _, rows, n_events = _program(n, 3)
    a = trajectory_sample(n, rows, n_events, shots, 11, 2, return_choices=True)
    b = trajectory_sample(n, rows, n_events, shots, 11, 2, return_choices=True)
    c = trajectory_sample(n, rows, n_events, shots, 11, 3, return_choices=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[1], c[1])
    # a shot depends on (seed, run, shot) only: a shorter call is a prefix of a longer one
    assert np.array_equal(trajectory_sample(n, rows, n_events, 100, 11, 2), a[0][:100])


def test_ideal_model_gives_the_noiseless_counts():
    from adaptaqc_amd import noise
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator

    qc = to_circuit(5, ref.brickwork(5, 4, 2))
    qc.measure(1, 0)
    qc.measure(4, 1)
    identity = noise.NoiseModel()
    identity.add_all_qubit_quantum_error(noise.thermal_relaxation_error(50.0, 70.0, 0.0), ["rx", "cx", "measure"])
    sim = SamplingSimulator()
    want = sim.run(qc, shots=2000, seed_simulator=7).result().get_counts()
    for nm in (None, noise.NoiseModel(), identity):
        assert sim.run(qc, shots=2000, seed_simulator=7, noise_model=nm).result().get_counts() == want
    # unseeded runs advance the same run counter with and without a model
    sim_a, sim_b = SamplingSimulator(seed=5), SamplingSimulator(seed=5)
    sim_a.run(qc, shots=10, noise_model=_model())
    sim_b.run(qc, shots=10)
    assert sim_a.runs == sim_b.runs == 1
    assert sim_a.run(qc, shots=500).result().get_counts() == sim_b.run(qc, shots=500).result().get_counts()


def test_backend_global_cost_under_noise():
    """U U^-1 on 4 qubits: the noiseless cost is exactly 0; under the model it is a binomial mean of
    p = 1 - rho_{0..0}, so it lies within 6 sqrt(p (1 - p) / shots) of p and is positive."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.noise import trajectory_program
    from adaptaqc_amd.utils.circuit_operations import create_noisemodel

    n, shots = 4, 8192
    u = to_circuit(n, ref.brickwork(n, 2, 9))
    qc = u.compose(u.inverse())
    for q in range(n):
        qc.measure(q, q)
    nm = create_noisemodel(50e-3, 70e-3, log_fidelities=False)
    be = QiskitSamplingBackend(SamplingSimulator(seed=4))
    comp = FakeCompiler(qc)
    comp.total_num_qubits = n
    comp.general_initial_state = False
    comp.execute_kwargs = {"shots": shots, "seed_simulator": 21}
    assert be.evaluate_global_cost(comp) == 0
    comp.execute_kwargs = {"shots": shots, "seed_simulator": 21, "noise_model": nm}
    cost = be.evaluate_global_cost(comp)
    rows, n_events, measured = trajectory_program(qc, nm)
    assert measured == {q: q for q in range(n)} and n_events > n
    p = 1 - float(np.real(tref.density_matrix(n, rows)[0, 0]))
    print(f"cost {cost:.5f}, p = {p:.5f}, bound {6 * np.sqrt(p * (1 - p) / shots):.5f}")
    assert cost > 0
    assert abs(cost - p) < 6 * np.sqrt(p * (1 - p) / shots)
    z = be.measure_qubit_expectation_values(comp)
    assert len(z) == n and all(0 < v <= 1 for v in z)


def test_compiler_passes_the_noise_model_through():
    """execute_kwargs={"noise_model": ...} through AdaptCompiler unchanged: the first cost it evaluates
    is the binomial mean of 1 - rho_{0..0} of its full circuit under the model, two layers compile,
    and the kwargs pickle (the compiler pickles itself at checkpoints)."""
    import pickle

    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig
    from adaptaqc_amd.noise import trajectory_program

    shots = 8192
    target = to_circuit(3, [("ry", (0,), (0.9,)), ("cx", (0, 1), ()), ("rx", (2,), (0.4,)), ("cx", (1, 2), ())])
    nm = _model()
    comp = AdaptCompiler(target, backend=QiskitSamplingBackend(), execute_kwargs={"shots": shots, "seed_simulator": 7,
                                                                                   "noise_model": nm},
                         adapt_config=AdaptConfig(method="expectation", max_layers=2))
    cost = comp.evaluate_cost()
    rows, n_events, _ = trajectory_program(comp.full_circuit, nm)
    p = 1 - float(np.real(tref.density_matrix(comp.full_circuit.num_qubits, rows)[0, 0]))
    assert n_events > 0 and abs(cost - p) < 6 * np.sqrt(p * (1 - p) / shots)
    result = comp.compile()
    assert len(result.global_cost_history) >= 2 and all(0 <= c <= 1 for c in result.global_cost_history)
    back = pickle.loads(pickle.dumps(comp.execute_kwargs))
    assert trajectory_program(target, back["noise_model"])[0].tobytes() == trajectory_program(target, nm)[0].tobytes()


def test_refusals():
    from adaptaqc_amd import noise
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.device import trajectory_sample

    qc, rows, n_events = _program(3, 1)
    nm = _model()
    with pytest.raises(NotImplementedError, match="trajectories"):
        SamplingSimulator(method="matrix_product_state").run(qc, shots=10, noise_model=nm)
    be = QiskitSamplingBackend(SamplingSimulator(), tomography="device")
    with pytest.raises(NotImplementedError, match="noise_model"):
        be.pair_tomography(qc, [(0, 1)], {"shots": 100, "noise_model": nm})
    with pytest.raises(NotImplementedError, match="noise_model"):
        be.concurrence_lower_bounds(qc, [(0, 1)], {"shots": 100, "noise_model": nm})
    with pytest.raises(AqcError, match="-1"):
        trajectory_sample(25, rows, n_events, 4, 1)
    with pytest.raises(AqcError, match="-1"):
        trajectory_sample(3, rows, n_events, 0, 1)
    u = np.full((4, n_events + 1), 0.5)
    u[2, 1] = 1.0
    with pytest.raises(AqcError, match="-1"):
        trajectory_sample(3, rows, n_events, 4, 1, u=u)
    bad = rows.copy()
    k = int(np.flatnonzero(bad["flags"] == 1)[0])
    bad["m"][k, 0] = 0.5  # sum K^dag K is no longer the identity
    with pytest.raises(AqcError, match="-1"):
        trajectory_sample(3, bad, n_events, 4, 1)
    bad = rows.copy()
    bad["q1"][k] = 5
    with pytest.raises(AqcError, match="-1"):
        trajectory_sample(3, bad, n_events, 4, 1)
    assert trajectory_sample(3, rows, n_events, 4, 1).shape == (4,)  # the library still runs after refusals
