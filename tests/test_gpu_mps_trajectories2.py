"""Correlated two-qubit errors on the MPS trajectory engine (csrc/mps_traj.hip under
aqc_mps_traj_set_correlated): shots, pair tomography and the Pauli readout against the dense restatement
of tests/mps_trajectory2_ref.py, the general path against the product-unitary one, and through
SamplingSimulator(mps_trajectories=True, mps_correlated=True) up to an ISL compile.

k_mps_kraus2_rho sums rho in slices of RHO_SLICE = 1024 (l, r) positions of theta, one workgroup each,
the grid sized by the capacity: capacity 4 is 1 slice, capacity 64 is 4, and the wide-bond case fills 16
slices with data (128 x 128 positions)."""
import functools

import numpy as np
import pytest

import mps_trajectory2_ref as m2ref
import sampling_ref as ref
import traj_tomography_ref as ttref
import trajectory2_ref as t2ref
from conftest import to_circuit

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 23
RHO_SLICE = 1024


@pytest.fixture(autouse=True)
def _mode_restored():
    """Every test leaves the engine's process-wide switch at 0."""
    from adaptaqc_amd import _lib

    yield
    _lib.check(_lib.lib().aqc_mps_traj_set_correlated(0))


@functools.lru_cache(maxsize=None)
def _case(n, depth, which, shots):
    """(rows, n_events, seed, run, u, reference words, choices, near), computed once per case."""
    _, rows, n_events = t2ref.program(n, depth, which)
    seed, run = SEED + n, 1
    u = ref.uniforms(seed, run, shots, n_events + n)
    out = (rows, n_events, seed, run, u) + m2ref.trajectories(n, rows, u)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# (n, depth, model, shots, chi_cap): the smallest state; 3 qubits hold cx in both listing orders and on
# non-adjacent qubits; capacities the state fills (4, 8, 32); 70 states at capacity 64, the 2 chi = 128 class
CASES = [(2, 1, "b", 64, 2), (3, 1, "a", 300, 4), (3, 1, "c", 300, 4), (4, 3, "c", 300, 4), (6, 3, "a", 200, 8),
         (8, 2, "b", 70, 64), (10, 2, "a", 40, 32)]
assert all((cap * cap + RHO_SLICE - 1) // RHO_SLICE == (4 if cap == 64 else 1) for *_, cap in CASES)


def _check_shots(n, rows, n_events, seed, run, u, want, want_k, near, chi_cap, correlated=True):
    from adaptaqc_amd.device import mps_trajectory_sample

    shots = len(want)
    keep = ~near
    for kwargs in ({"u": u}, {}):
        got, got_k = mps_trajectory_sample(n, rows, n_events, shots, seed, run, return_choices=True, chi_cap=chi_cap,
                                           correlated=correlated, **kwargs)
        assert got.dtype == np.uint64 and got.shape == want.shape and got_k.shape == (shots, n_events)
        assert np.array_equal(got_k[keep], want_k[keep])
        bad = np.flatnonzero((got != want).any(axis=1) & keep)
        assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    return got, got_k


@pytest.mark.parametrize("n,depth,which,shots,chi_cap", CASES, ids=[f"n{c[0]}{c[2]}" for c in CASES])
def test_shot_by_shot_against_restatement(n, depth, which, shots, chi_cap):
    """Outcome words and choices (0 .. 15 for a group) of every shot not flagged near a boundary equal the
    restatement's, with u passed in and with u drawn on the device from (seed, run); at most 1 % of the
    shots flagged."""
    rows, n_events, seed, run, u, want, want_k, near = _case(n, depth, which, shots)
    assert n_events > 0 and t2ref.n_events(rows) == n_events
    print(f"n={n} model {which} shots={shots} rows={len(rows)} events={n_events} near={int(near.sum())}")
    assert near.sum() <= shots // 100
    _, got_k = _check_shots(n, rows, n_events, seed, run, u, want, want_k, near, chi_cap)
    if which == "a":
        assert got_k.max() > 3  # a group's choice beyond what a one-qubit row can hold


def _wide_ops():
    n = 14
    ops = []
    for i in range(7):
        ops += [("ry", (i,), (np.pi / 2,)), ("cx", (i, i + 7), ())]
    return n, ops + [("cx", (7, 6), ())]


def test_wide_bonds():
    """14 qubits, seven pairs across the middle: every trajectory's middle bond has rank 128 and the last
    group acts on a theta of side 256 (the big_svd class), its rho summed over 16 slices."""
    from adaptaqc_amd.noise import trajectory_program

    n, ops = _wide_ops()
    rows, n_events, _ = trajectory_program(to_circuit(n, ops), t2ref.model("c"))
    assert n_events == 15
    shots, seed, run = 8, SEED + n, 1
    u = ref.uniforms(seed, run, shots, n_events + n)
    want, want_k, near = m2ref.trajectories(n, rows, u)
    print(f"near={int(near.sum())}")
    assert not near.any()
    _check_shots(n, rows, n_events, seed, run, u, want, want_k, near, 128)


def test_general_path_against_product_path():
    """Model a at n = 6 under mode 1 (one-site unitaries, constant weights) and mode 2 (the same groups as
    two-site updates chosen on the device): equal choices, equal words outside near."""
    from adaptaqc_amd.device import mps_trajectory_sample

    n, depth, which, shots, chi_cap = CASES[4]
    rows, n_events, seed, run, u, want, want_k, near = _case(n, depth, which, shots)
    one = mps_trajectory_sample(n, rows, n_events, shots, seed, run, return_choices=True, chi_cap=chi_cap, correlated=1)
    two = mps_trajectory_sample(n, rows, n_events, shots, seed, run, return_choices=True, chi_cap=chi_cap, correlated=2)
    assert np.array_equal(one[1], two[1])
    assert np.array_equal(one[0][~near], two[0][~near])
    assert np.array_equal(two[0][~near], want[~near]) and np.array_equal(two[1][~near], want_k[~near])


def test_batch_independence_and_runs():
    """70 shots of a model-b program at capacity 64: a forced batch of 32 (three batches, the last one
    short) and the default give the same bits; so do two identical calls; another run does not; a shorter
    call is a prefix of a longer one."""
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import mps_trajectory_sample

    n, shots = 8, 70
    rows, n_events = _case(n, 2, "b", shots)[:2]

    def run(count, r):
        return mps_trajectory_sample(n, rows, n_events, count, 11, r, return_choices=True, chi_cap=64, correlated=True)

    a = run(shots, 2)
    _lib.check(_lib.lib().aqc_mps_traj_set_batch(32))
    try:
        b = run(shots, 2)
    finally:
        _lib.check(_lib.lib().aqc_mps_traj_set_batch(0))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = run(shots, 2)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    d = run(shots, 3)
    assert not np.array_equal(a[0], d[0]) and not np.array_equal(a[1], d[1])
    assert np.array_equal(run(9, 2)[0], a[0][:9])


# ---- the two readouts -----------------------------------------------------------------------------------
def _readout_model(which):
    """t2ref.model(which) with errors on h, sdg and measure (traj_tomography_ref.model's)."""
    from adaptaqc_amd import noise

    nm = t2ref.model(which)
    nm.add_all_qubit_quantum_error(noise.thermal_relaxation_error(t2ref.T1, t2ref.T2, 6000), "h")
    nm.add_all_qubit_quantum_error(noise.depolarizing_error(0.03), "sdg")
    nm.add_all_qubit_quantum_error(noise.thermal_relaxation_error(t2ref.T1, t2ref.T2, 20000), "measure")
    nm.add_quantum_error(noise.phase_damping_error(0.1), "h", (1,))
    return nm


@functools.lru_cache(maxsize=None)
def _readout_program(n, depth, which):
    from adaptaqc_amd.noise import trajectory_program

    nm = _readout_model(which)
    rows, n_events, _ = trajectory_program(to_circuit(n, t2ref.ops(n, depth)), nm)
    effects = ttref.readout_effects_ref(n, ttref.kraus_of(nm))
    return rows, n_events, effects


@pytest.mark.parametrize("n,depth,which", [(4, 3, "b"), (4, 3, "a"), (6, 3, "b"), (6, 3, "a")])
def test_pair_tomography_against_restatement(n, depth, which):
    """Every pair, 9 x 16 trajectories: each (trajectory, pair) outcome outside near equals the
    restatement's; at most 1 % of the trajectories flagged."""
    from adaptaqc_amd.device import mps_trajectory_pair_tomography

    rows, n_events, effects = _readout_program(n, depth, which)
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    shots, seed, run = 16, SEED + n, 1
    u = ref.uniforms(seed, run, 9 * shots, n_events + len(pairs))
    want, want_counts, near = m2ref.pair_tomography(n, rows, pairs, effects, u)
    print(f"n={n} model {which}: events={n_events} pairs={len(pairs)} near={int(near.sum())}")
    assert near.sum() <= near.size // 100
    for kwargs in ({"u": u}, {}):
        counts, got = mps_trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, seed, run,
                                                     return_outcomes=True, chi_cap=8, correlated=True, **kwargs)
        assert np.array_equal(got[~near], want[~near])
        assert np.array_equal(counts, ttref.counts_of(got)) and np.all(counts.sum(axis=2) == shots)
        if not near.any():
            assert np.array_equal(counts, want_counts)


def _mixed_labels(n, count):
    """Labels of weight 1 .. 4 (the statevector entry's limit on general factors), one on qubits 0 and n - 1."""
    rng = np.random.default_rng(n)
    out = ["Y" + "I" * (n - 2) + "X"]
    while len(out) < count:
        label = "".join(rng.choice(list("IIXYZ"), size=n))
        if 1 <= n - label.count("I") <= 4 and label not in out:
            out.append(label)
    return out


@pytest.mark.parametrize("which", ["b", "a"])
def test_pauli_readout_against_restatement_and_statevector(which):
    """n = 6, 12 mixed labels, 64 shots under readout noise: each (trajectory, term) outcome outside near
    equals the restatement's and aqc_sv_traj_pauli_counts' for the same (seed, run); values within 1e-6;
    at most 1 % of the entries flagged."""
    from adaptaqc_amd.device import mps_trajectory_pauli_counts, trajectory_pauli_counts
    from adaptaqc_amd.paulis import terms_to_codes

    n, shots = 6, 64
    rows, n_events, effects = _readout_program(n, 3, which)
    labels = _mixed_labels(n, 12)
    codes = terms_to_codes(labels, n)
    seed, run = SEED + n, 1
    u = ref.uniforms(seed, run, shots, n_events + len(labels))
    want_v, want, want_plus, near = m2ref.pauli_counts(n, rows, codes, effects, u)
    print(f"model {which}: events={n_events} near={int(near.sum())} of {near.size}")
    assert near.sum() <= near.size // 100
    _, sv = trajectory_pauli_counts(n, rows, n_events, codes, effects, shots, seed, run, return_outcomes=True)
    for kwargs in ({"u": u}, {}):
        plus, values, got = mps_trajectory_pauli_counts(n, rows, n_events, codes, effects, shots, seed, run,
                                                        return_values=True, return_outcomes=True, chi_cap=8,
                                                        correlated=True, **kwargs)
        assert float(np.max(np.abs(values - want_v))) <= 1e-6
        assert np.array_equal(got[~near], want[~near])
        assert np.array_equal(got[~near], sv[~near])
        assert np.array_equal(plus, (got == 0).sum(axis=0))
        if not near.any():
            assert np.array_equal(plus, want_plus)


# ---- the law ----------------------------------------------------------------------------------------------
BLOCKS, BLOCK_N = 6, 5


def _block_ops(b):
    return ref.brickwork(BLOCK_N, 2, 300 + b) + [("cx", (0, 3), ()), ("ry", (2,), (0.3 + 0.1 * b,)), ("cx", (4, 1), ())]


@pytest.mark.parametrize("which", ["a", "b"])
def test_thirty_qubits_follow_the_density_matrix(which):
    """Six independent 5-qubit blocks on 30 qubits through SamplingSimulator(method="automatic",
    mps_trajectories=True, mps_correlated=True).  Every block's marginal histogram: Pearson chi-square
    below dof + 6 sqrt(2 dof) against the diagonal of that block's density-matrix evolution, and above it
    against the block's noiseless law."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.noise import trajectory_program

    n, shots = BLOCKS * BLOCK_N, 2048
    ops = [(name, tuple(q + BLOCK_N * b for q in qs), params) for b in range(BLOCKS) for name, qs, params in _block_ops(b)]
    nm = t2ref.model(which)
    sim = SamplingSimulator(method="automatic", seed=SEED, mps_trajectories=True, mps_correlated=True)
    counts = sim.run(to_circuit(n, ops), shots=shots, noise_model=nm).result().get_counts()
    assert sum(counts.values()) == shots and all(len(k) == n for k in counts)
    for b in range(BLOCKS):
        obs = np.zeros(2 ** BLOCK_N, dtype=np.int64)
        for key, c in counts.items():
            obs[int(key[n - BLOCK_N * (b + 1): n - BLOCK_N * b], 2)] += c
        qc = to_circuit(BLOCK_N, _block_ops(b))
        probs = np.real(np.diag(t2ref.density_matrix(BLOCK_N, trajectory_program(qc, nm)[0])))
        clean = np.real(np.diag(t2ref.density_matrix(BLOCK_N, trajectory_program(qc, None)[0])))
        stat, dof = ref.chi_square(obs, probs, shots)
        stat0, dof0 = ref.chi_square(obs, clean, shots)
        print(f"block {b}: chi-square {stat:.1f} at {dof} dof, against the noiseless law {stat0:.1f} at {dof0} dof")
        assert stat < dof + 6 * np.sqrt(2 * dof)
        assert stat0 > dof0 + 6 * np.sqrt(2 * dof0)


# ---- end to end ---------------------------------------------------------------------------------------------
def _rank4_ops():
    # two Bell-like pairs across the middle bond of 4 qubits: Schmidt rank 4 there
    return [("ry", (0,), (np.pi / 2,)), ("cx", (0, 2), ()), ("ry", (1,), (np.pi / 2,)), ("cx", (1, 3), ())]


@pytest.mark.parametrize("which", ["a", "b"])
def test_counts_and_capacity_growth(monkeypatch, which):
    """With seed_simulator the counts of an n = 4 circuit are the restatement's; the simulator's route,
    started at capacity 2 on a circuit that needs 4, grows it and returns the same shots; without
    mps_correlated the refusal stands."""
    from adaptaqc_amd import mps_operations as mops
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.device import counts_from_samples, mps_trajectory_sample
    from adaptaqc_amd.noise import trajectory_program

    n, shots = 4, 64
    qc = to_circuit(n, _rank4_ops())
    nm = t2ref.model(which)
    rows, n_events, _ = trajectory_program(qc, nm)
    words, _, near = m2ref.trajectories(n, rows, ref.uniforms(9, 0, shots, n_events + n))
    assert not near.any()
    sim = SamplingSimulator(method="matrix_product_state", mps_trajectories=True, mps_correlated=True)
    assert sim.run(qc, shots=shots, seed_simulator=9, noise_model=nm).result().get_counts() == counts_from_samples(words, n)
    with pytest.raises(AqcError, match=r"capacity \(chi_cap\) exceeded"):
        mps_trajectory_sample(n, rows, n_events, shots, 9, chi_cap=2, correlated=True)
    tried = []

    def small_start(n_, max_chi, loaded_max=1, learned=None):
        tried.append(max(2, (learned or {}).get(n_, 0)))
        return tried[-1]

    monkeypatch.setattr(mops, "chi_cap_for", small_start)
    sim = SamplingSimulator(method="matrix_product_state", mps_trajectories=True, mps_correlated=True)
    counts = sim.run(qc, shots=shots, seed_simulator=9, noise_model=nm).result().get_counts()
    assert tried == [2, 4]
    assert counts == counts_from_samples(words, n)
    with pytest.raises(NotImplementedError, match="correlated.*24 qubits"):
        SamplingSimulator(method="matrix_product_state", mps_trajectories=True).run(qc, shots=4, noise_model=nm)
    with pytest.raises(NotImplementedError, match="correlated.*24 qubits"):
        mps_trajectory_sample(n, rows, n_events, shots, 9, chi_cap=4)


def test_isl_compiles_under_a_correlated_noise_model():
    """ISL, the shot backend and depolarizing_error(0.05, 2) on cx together on the MPS engine: two layers
    with the tolerances at the shot noise of 1024 shots (test_gpu_mps_traj_tomography's settings)."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig

    target = to_circuit(4, [("ry", (0,), (0.9,)), ("cx", (0, 1), ()), ("rx", (3,), (0.4,))])
    sim = SamplingSimulator(method="matrix_product_state", mps_trajectories=True, mps_correlated=True)
    backend = QiskitSamplingBackend(sim, tomography="device", trajectory_tomography=True)
    config = AdaptConfig(method="ISL", max_layers=2, rotoselect_tol=3e-2, rotosolve_tol=3e-2, rotosolve_frequency=2)
    comp = AdaptCompiler(target, backend=backend, adapt_config=config,
                         execute_kwargs={"shots": 1024, "seed_simulator": 7, "noise_model": t2ref.model("a")})
    result = comp.compile()
    assert len(result.global_cost_history) >= 2
    assert all(0 <= c <= 1 for c in result.global_cost_history)
    assert "ISL" in result.method_history


@pytest.mark.parametrize("which", ["a", "c"])
def test_thirty_qubits_block_by_block(which):
    """The same 30 qubits shot by shot: the blocks are independent, so a block's bits and choices are those
    of the dense restatement of the block alone under the columns of the global uniforms that belong to
    it (its events are contiguous, its qubits' measurements follow all events) -- chunks of the schedule,
    waves that hold several events and sites far from 0 included."""
    from adaptaqc_amd.device import mps_trajectory_sample
    from adaptaqc_amd.noise import trajectory_program

    n, shots, seed = BLOCKS * BLOCK_N, 256, SEED
    ops = [(name, tuple(q + BLOCK_N * b for q in qs), params) for b in range(BLOCKS) for name, qs, params in _block_ops(b)]
    nm = t2ref.model(which)
    rows, n_events, _ = trajectory_program(to_circuit(n, ops), nm)
    u = ref.uniforms(seed, 0, shots, n_events + n)
    words, choices = mps_trajectory_sample(n, rows, n_events, shots, seed, 0, return_choices=True, chi_cap=8,
                                           correlated=True)
    bits = ref.unpack_bits(words, n)
    e0 = flagged = 0
    for b in range(BLOCKS):
        brows, be, _ = trajectory_program(to_circuit(BLOCK_N, _block_ops(b)), nm)
        ub = np.concatenate([u[:, e0: e0 + be], u[:, n_events + BLOCK_N * b: n_events + BLOCK_N * (b + 1)]], axis=1)
        want, want_k, near = m2ref.trajectories(BLOCK_N, brows, ub)
        keep = ~near
        flagged += int(near.sum())
        assert np.array_equal(bits[keep, BLOCK_N * b: BLOCK_N * (b + 1)], ref.unpack_bits(want, BLOCK_N)[keep]), b
        assert np.array_equal(choices[keep, e0: e0 + be], want_k[keep]), b
        e0 += be
    assert e0 == n_events and flagged <= BLOCKS * shots // 100
