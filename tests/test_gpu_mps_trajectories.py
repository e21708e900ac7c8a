"""Noisy shot sampling on the MPS engine (csrc/mps_traj.hip, aqc_mps_traj_sample) against the dense
restatement of tests/mps_trajectory_ref.py, and through SamplingSimulator(mps_trajectories=True)."""
import functools

import numpy as np
import pytest

import mps_trajectory_ref as mref
import sampling_ref as ref
import trajectory_ref as tref
from conftest import to_circuit

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 11
T1 = 50e3


def _ops(n, depth):
    if n == 1:
        return [("rx", (0,), (0.7,)), ("rz", (0,), (1.1,))]
    return ref.brickwork(n, depth, 200 + n)


def _model(t2=70e3):
    """Thermal relaxation for 5000 after every one-qubit gate and 15000 on both qubits of cx."""
    from adaptaqc_amd import noise

    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(noise.thermal_relaxation_error(T1, t2, 5000), ["rx", "ry", "rz"])
    two = noise.thermal_relaxation_error(T1, t2, 15000)
    nm.add_all_qubit_quantum_error(two.expand(two), "cx")
    return nm


@functools.lru_cache(maxsize=None)
def _case(n, depth, shots, t2, seed, run):
    """(rows, n_events, u, reference words, choices, near), computed once per case."""
    from adaptaqc_amd.noise import trajectory_program

    rows, n_events, _ = trajectory_program(to_circuit(n, _ops(n, depth)), _model(t2))
    u = ref.uniforms(seed, run, shots, n_events + n)
    return (rows, n_events, u) + mref.trajectories(n, rows, u)


# (n, depth, shots, chi_cap, t2): the smallest state; capacities that the state fills (4, 8, 32); 70
# states at capacity 64, where a batch without Kraus rows would take the fused chain; t2 on either side of t1
CASES = [(1, 0, 64, 1, 70e3), (4, 3, 300, 4, 70e3), (6, 3, 200, 8, 30e3), (8, 2, 70, 64, 70e3), (10, 2, 40, 32, 70e3)]


@pytest.mark.parametrize("n,depth,shots,chi_cap,t2", CASES)
def test_shot_by_shot_against_restatement(n, depth, shots, chi_cap, t2):
    """Outcome words and Kraus choices of every shot not flagged near a boundary equal the restatement's,
    with u passed in and with u drawn on the device from (seed, run); at most 1 % of the shots flagged."""
    from adaptaqc_amd.device import mps_trajectory_sample

    seed, run = SEED + n, 1
    rows, n_events, u, want, want_k, near = _case(n, depth, shots, t2, seed, run)
    assert n_events > 0
    print(f"n={n} shots={shots} rows={len(rows)} events={n_events} near={int(near.sum())}")
    assert near.sum() <= shots // 100
    keep = ~near
    for kwargs in ({"u": u}, {}):
        got, got_k = mps_trajectory_sample(n, rows, n_events, shots, seed, run, return_choices=True, chi_cap=chi_cap,
                                           **kwargs)
        assert got.dtype == np.uint64 and got.shape == (shots, 1) and got_k.shape == (shots, n_events)
        bad = np.flatnonzero((got != want).any(axis=1) & keep)
        assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
        assert np.array_equal(got_k[keep], want_k[keep])
    assert np.array_equal(mps_trajectory_sample(n, rows, n_events, shots, seed, run, chi_cap=chi_cap), got)


def test_batch_independence_and_runs():
    """70 shots at capacity 64: a forced batch of 32 (three batches, the last one short) and the default
    (one batch of 70) give the same bits; so do two identical calls; another run does not; a shorter
    call is a prefix of a longer one."""
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import mps_trajectory_sample

    n, shots = 8, 70
    rows, n_events = _case(n, 2, shots, 70e3, SEED + n, 1)[:2]
    a = mps_trajectory_sample(n, rows, n_events, shots, 11, 2, return_choices=True, chi_cap=64)
    _lib.check(_lib.lib().aqc_mps_traj_set_batch(32))
    try:
        b = mps_trajectory_sample(n, rows, n_events, shots, 11, 2, return_choices=True, chi_cap=64)
    finally:
        _lib.check(_lib.lib().aqc_mps_traj_set_batch(0))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = mps_trajectory_sample(n, rows, n_events, shots, 11, 2, return_choices=True, chi_cap=64)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    d = mps_trajectory_sample(n, rows, n_events, shots, 11, 3, return_choices=True, chi_cap=64)
    assert not np.array_equal(a[0], d[0]) and not np.array_equal(a[1], d[1])
    assert np.array_equal(mps_trajectory_sample(n, rows, n_events, 9, 11, 2, chi_cap=64), a[0][:9])


BLOCKS, BLOCK_N = 6, 5


def _block_ops(b):
    return ref.brickwork(BLOCK_N, 2, 300 + b) + [("cx", (0, 3), ()), ("ry", (2,), (0.3 + 0.1 * b,)), ("cx", (4, 1), ())]


def test_thirty_qubits_follow_the_density_matrix():
    """Six independent 5-qubit blocks, each with non-adjacent cx, on 30 qubits -- beyond any statevector
    route -- through SamplingSimulator(method="automatic", mps_trajectories=True).  Every block's marginal
    histogram: Pearson chi-square below dof + 6 sqrt(2 dof) against the diagonal of that block's
    density-matrix evolution, and above it against the block's noiseless law."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.noise import trajectory_program

    # 305 two-site updates per shot; 535 of them take 111 ms for 256 shots (profiles/mps_trajectory.json)
    n, shots = BLOCKS * BLOCK_N, 2048
    ops = [(name, tuple(q + BLOCK_N * b for q in qs), params) for b in range(BLOCKS) for name, qs, params in _block_ops(b)]
    nm = _model()
    counts = SamplingSimulator(method="automatic", seed=SEED, mps_trajectories=True).run(
        to_circuit(n, ops), shots=shots, noise_model=nm).result().get_counts()
    assert sum(counts.values()) == shots and all(len(k) == n for k in counts)
    for b in range(BLOCKS):
        obs = np.zeros(2 ** BLOCK_N, dtype=np.int64)
        for key, c in counts.items():
            obs[int(key[n - BLOCK_N * (b + 1): n - BLOCK_N * b], 2)] += c
        qc = to_circuit(BLOCK_N, _block_ops(b))
        probs = np.real(np.diag(tref.density_matrix(BLOCK_N, trajectory_program(qc, nm)[0])))
        clean = np.real(np.diag(tref.density_matrix(BLOCK_N, trajectory_program(qc, None)[0])))
        stat, dof = ref.chi_square(obs, probs, shots)
        stat0, dof0 = ref.chi_square(obs, clean, shots)
        print(f"block {b}: chi-square {stat:.1f} at {dof} dof, against the noiseless law {stat0:.1f} at {dof0} dof")
        assert stat < dof + 6 * np.sqrt(2 * dof)
        assert stat0 > dof0 + 6 * np.sqrt(2 * dof0)


def test_known_answers_in_two_words():
    """66 qubits: x(65) followed by relaxation for time 0 reads bit 65 (word 1, bit 1) in every shot; for
    a time far beyond T1 every shot reads zero."""
    from adaptaqc_amd import noise
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.circuit import QuantumCircuit
    from adaptaqc_amd.device import mps_trajectory_sample

    n, shots = 66, 40
    qc = QuantumCircuit(n)
    qc.x(65)
    gate = noise.trajectory_program(qc, None)[0]
    for time, word1 in ((0.0, 2), (1e6, 0)):
        rows = np.concatenate([gate, noise.kraus_row(noise.thermal_relaxation_error(50.0, 70.0, time), 65)])
        out, choices = mps_trajectory_sample(n, rows, 1, shots, 5, return_choices=True, chi_cap=2)
        assert out.shape == (shots, 2) and np.all(out[:, 0] == 0) and np.all(out[:, 1] == word1)
        assert np.all(choices == (0 if word1 else 1))
    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(noise.thermal_relaxation_error(50.0, 70.0, 1e6), "x")
    sim = SamplingSimulator(method="matrix_product_state", seed=3, mps_trajectories=True)
    assert sim.run(qc, shots=shots, noise_model=nm).result().get_counts() == {"0" * n: shots}


def _rank4_ops():
    # two Bell-like pairs across the middle bond of 4 qubits: Schmidt rank 4 there
    return [("ry", (0,), (np.pi / 2,)), ("cx", (0, 2), ()), ("ry", (1,), (np.pi / 2,)), ("cx", (1, 3), ())]


def test_capacity_error_and_growth(monkeypatch):
    """chi_cap = 2 on a circuit that needs 4: the capacity error from the C entry.  The simulator's
    route, started at capacity 2, grows it and returns the restatement's shots."""
    from adaptaqc_amd import mps_operations as mops
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.device import counts_from_samples, mps_trajectory_sample
    from adaptaqc_amd.noise import trajectory_program

    n, shots = 4, 64
    qc = to_circuit(n, _rank4_ops())
    nm = _model()
    rows, n_events, _ = trajectory_program(qc, nm)
    with pytest.raises(AqcError, match=r"capacity \(chi_cap\) exceeded"):
        mps_trajectory_sample(n, rows, n_events, shots, 9, chi_cap=2)
    assert mps_trajectory_sample(n, rows, n_events, shots, 9, chi_cap=4).shape == (shots, 1)
    tried = []

    def small_start(n_, max_chi, loaded_max=1, learned=None):
        tried.append(max(2, (learned or {}).get(n_, 0)))
        return tried[-1]

    monkeypatch.setattr(mops, "chi_cap_for", small_start)
    sim = SamplingSimulator(method="matrix_product_state", mps_trajectories=True)
    counts = sim.run(qc, shots=shots, seed_simulator=9, noise_model=nm).result().get_counts()
    assert tried == [2, 4]
    words, _, near = mref.trajectories(n, rows, ref.uniforms(9, 0, shots, n_events + n))
    assert not near.any()
    assert counts == counts_from_samples(words, n)


def test_ideal_model_gives_the_noiseless_counts():
    from adaptaqc_amd import noise
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator

    qc = to_circuit(5, ref.brickwork(5, 4, 2))
    qc.measure(1, 0)
    qc.measure(4, 1)
    identity = noise.NoiseModel()
    identity.add_all_qubit_quantum_error(noise.thermal_relaxation_error(50.0, 70.0, 0.0), ["rx", "cx", "measure"])
    sim = SamplingSimulator(method="matrix_product_state", mps_trajectories=True)
    want = sim.run(qc, shots=2000, seed_simulator=7).result().get_counts()
    for nm in (None, noise.NoiseModel(), identity):
        assert sim.run(qc, shots=2000, seed_simulator=7, noise_model=nm).result().get_counts() == want


def test_measured_clbits_under_noise():
    """Measures into chosen clbits read the trajectory's outcome words as the noiseless path reads its own."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.device import counts_from_samples
    from adaptaqc_amd.noise import trajectory_program

    n, shots = 4, 64
    qc = to_circuit(n, _rank4_ops())
    qc.measure(3, 0)
    qc.measure(0, 1)
    nm = _model()
    rows, n_events, measured = trajectory_program(qc, nm)
    words, _, near = mref.trajectories(n, rows, ref.uniforms(9, 0, shots, n_events + n))
    assert not near.any() and measured == {3: 0, 0: 1}
    sim = SamplingSimulator(method="matrix_product_state", mps_trajectories=True)
    counts = sim.run(qc, shots=shots, seed_simulator=9, noise_model=nm).result().get_counts()
    assert counts == counts_from_samples(words, n, measured)


def test_refusals():
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.device import mps_trajectory_sample

    n = 3
    rows, n_events = _case(n, 1, 4, 70e3, 1, 0)[:2]
    qc = to_circuit(n, _ops(n, 1))
    nm = _model()
    with pytest.raises(NotImplementedError, match="mps_trajectories=True"):
        SamplingSimulator(method="matrix_product_state").run(qc, shots=10, noise_model=nm)
    with pytest.raises(NotImplementedError, match="trajectories"):
        SamplingSimulator(method="matrix_product_state").run(qc, shots=10, noise_model=nm)
    big = to_circuit(25, [("rx", (24,), (0.3,))])
    with pytest.raises(NotImplementedError, match="mps_trajectories=True"):
        SamplingSimulator().run(big, shots=10, noise_model=nm)
    with pytest.raises(AqcError, match="-1"):
        mps_trajectory_sample(0, rows[:0], 0, 4, 1)
    with pytest.raises(AqcError, match="-1"):
        mps_trajectory_sample(2, rows, n_events, 4, 1)  # rows on qubit 2 of a 2-qubit register
    with pytest.raises(AqcError, match="-1"):
        mps_trajectory_sample(n, rows, n_events, 0, 1)
    u = np.full((4, n_events + n), 0.5)
    u[2, 1] = 1.0
    with pytest.raises(AqcError, match="-1"):
        mps_trajectory_sample(n, rows, n_events, 4, 1, u=u)
    bad = rows.copy()
    k = int(np.flatnonzero(bad["flags"] == 1)[0])
    bad["m"][k, 0] = 0.5  # sum K^dag K is no longer the identity
    with pytest.raises(AqcError, match="-1"):
        mps_trajectory_sample(n, bad, n_events, 4, 1)
    bad = rows.copy()
    bad["q1"][k] = 5
    with pytest.raises(AqcError, match="-1"):
        mps_trajectory_sample(n, bad, n_events, 4, 1)
    with pytest.raises(AqcError, match="-1"):
        mps_trajectory_sample(n, rows, n_events, 4, 1, chi_cap=0)
    assert mps_trajectory_sample(n, rows, n_events, 4, 1).shape == (4, 1)  # the library still runs after refusals
