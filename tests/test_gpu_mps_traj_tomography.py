"""Noisy pair tomography on the MPS engine (csrc/mps_traj.hip, aqc_mps_traj_pair_tomo) against the dense
restatement of tests/mps_traj_tomography_ref.py and the statevector entry, and through
QiskitSamplingBackend(SamplingSimulator(mps_trajectories=True), trajectory_tomography=True) up to an ISL
compile under a noise model."""
import functools

import numpy as np
import pytest

import mps_traj_tomography_ref as mtref
import sampling_ref as ref
import tomography_ref as tomo
import traj_tomography_ref as ttref
import trajectory_ref as tref
from conftest import to_circuit

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 11

# (n, depth, shots, chi_cap, t2, pairs): the smallest state, the pair given hi-first; a capacity the
# state fills; t2 < t1; 72 handles at capacity 64, where a list without Kraus rows would take the fused
# chain; the widest pair, an adjacent one and three others
CASES = [
    (2, 1, 16, 2, 70e3, ((1, 0),)),
    (4, 3, 60, 4, 70e3, tuple(tomo.all_pairs(4))),
    (6, 3, 30, 8, 30e3, tuple(tomo.all_pairs(6))),
    (8, 2, 8, 64, 70e3, ((0, 7), (7, 6), (3, 4), (5, 1))),
    (10, 2, 5, 32, 70e3, ((0, 9), (1, 0), (8, 9), (4, 5), (7, 2), (3, 6))),
]
N6, N8 = CASES[2], CASES[3]


@functools.lru_cache(maxsize=None)
def _case(n, depth, shots, chi_cap, t2, pairs):
    """The program, the uniforms of (seed, run) and the restatement's answer, computed once."""
    _, rows, n_events, effects = ttref.program(n, depth, t2)
    seed, run = SEED + n, 1
    u = ref.uniforms(seed, run, 9 * shots, n_events + len(pairs))
    want, want_counts, near = mtref.pair_tomography(n, rows, list(pairs), effects, u)
    for a in (rows, effects, u, want, want_counts, near):
        a.setflags(write=False)
    return rows, n_events, effects, seed, run, u, want, want_counts, near


@pytest.mark.parametrize("n,depth,shots,chi_cap,t2,pairs", CASES)
def test_shot_by_shot_against_restatement(n, depth, shots, chi_cap, t2, pairs):
    """The outcome of every pair in every trajectory not flagged near a boundary equals the restatement's,
    with u passed in and with u drawn on the device from (seed, run); the counts are those of the
    outcomes and every row sums to shots; at most 1 % of the trajectories flagged."""
    from adaptaqc_amd.device import mps_trajectory_pair_tomography

    rows, n_events, effects, seed, run, u, want, want_counts, near = _case(n, depth, shots, chi_cap, t2, pairs)
    assert n_events > 0
    print(f"n={n} trajectories={9 * shots} rows={len(rows)} events={n_events} pairs={len(pairs)} near={int(near.sum())}")
    assert near.sum() <= 9 * shots // 100
    keep = ~near
    for kwargs in ({"u": u}, {}):
        counts, got = mps_trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, seed, run,
                                                     return_outcomes=True, chi_cap=chi_cap, **kwargs)
        assert got.dtype == np.uint8 and got.shape == (9 * shots, len(pairs))
        assert counts.dtype == np.int64 and counts.shape == (len(pairs), 9, 4)
        bad = np.argwhere((got != want) & keep[:, None])
        assert bad.size == 0, (bad[:5], got[tuple(bad[:5].T)], want[tuple(bad[:5].T)])
        assert np.array_equal(counts, ttref.counts_of(got)) and np.all(counts.sum(axis=2) == shots)
        if not near.any():
            assert np.array_equal(counts, want_counts)
    # without the outcomes
    assert np.array_equal(
        mps_trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, seed, run, chi_cap=chi_cap), counts)


def test_agrees_with_the_statevector_entry():
    """n = 6, the same (seed, run): the outcomes of aqc_sv_traj_pair_tomo on every trajectory not flagged."""
    from adaptaqc_amd.device import mps_trajectory_pair_tomography, trajectory_pair_tomography

    n, _, shots, chi_cap, _, pairs = N6
    rows, n_events, effects, seed, run, _, _, _, near = _case(*N6)
    _, sv = trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, seed, run, return_outcomes=True)
    _, mps = mps_trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, seed, run, return_outcomes=True,
                                            chi_cap=chi_cap)
    assert np.array_equal(sv[~near], mps[~near])


def test_batch_independence_runs_and_prefix():
    """72 trajectories at capacity 64: a forced batch of 32 (three batches, the last of 8) and the default
    (one batch) give the same bits; so does a batch of 32 read out in sub-batches of 5; so do two identical
    calls; another run does not; fewer shots give a prefix."""
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import mps_trajectory_pair_tomography

    n, _, shots, chi_cap, _, pairs = N8
    rows, n_events, effects = _case(*N8)[:3]

    def call(shots=shots, run=2):
        return mps_trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, 11, run, return_outcomes=True,
                                              chi_cap=chi_cap)

    a = call()
    try:
        _lib.check(_lib.lib().aqc_mps_traj_set_batch(32))
        b = call()
        _lib.check(_lib.lib().aqc_mps_traj_set_readout_batch(5))
        c = call()
    finally:
        _lib.check(_lib.lib().aqc_mps_traj_set_batch(0))
        _lib.check(_lib.lib().aqc_mps_traj_set_readout_batch(0))
    for other in (b, c, call()):
        assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1])
    d = call(run=3)
    assert not np.array_equal(a[0], d[0]) and not np.array_equal(a[1], d[1])
    short = call(shots=3)
    assert np.array_equal(short[1], a[1][:27]) and np.array_equal(short[0], ttref.counts_of(a[1][:27]))


def _chi_square_of_pair(counts, tables, shots):
    """Pearson's chi-square of a pair's nine independent tables, summed, with the summed dof."""
    stat = dof = 0
    for s in range(9):
        x, d = ref.chi_square(counts[s], tables[s], shots)
        stat, dof = stat + x, dof + d
    return stat, dof


def test_law_follows_the_density_matrix():
    """n = 5, every pair, capacity 4: per pair, the chi-square over its nine tables against the exact
    noisy tables below dof + 6 sqrt(2 dof); against the noiseless tables above it for at least one pair.
    (Not pooled over pairs: their tables share trajectories.)  16 shots a setting: the smallest power of
    two at which the restatement's own counts under these uniforms meet both conditions (at 8 a pair misses
    the first one; checked on the CPU with mps_traj_tomography_ref.pair_tomography, which flags no
    trajectory here)."""
    from adaptaqc_amd.device import mps_trajectory_pair_tomography
    from adaptaqc_amd.noise import readout_effects, trajectory_program

    n, shots = 5, 16
    pairs = tomo.all_pairs(n)
    qc, rows, n_events, effects = ttref.program(n, 3)
    counts = mps_trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, SEED, 0, chi_cap=4)
    assert np.all(counts.sum(axis=2) == shots)
    exact = ttref.exact_tables(n, rows, pairs, effects)
    clean = ttref.exact_tables(n, trajectory_program(qc, None)[0], pairs, readout_effects(n, None))
    above = 0
    for j, pair in enumerate(pairs):
        stat, dof = _chi_square_of_pair(counts[j], exact[j], shots)
        stat0, dof0 = _chi_square_of_pair(counts[j], clean[j], shots)
        print(f"pair {pair}: chi-square {stat:.1f} at {dof} dof; against the noiseless law {stat0:.1f} at {dof0} dof")
        assert stat < dof + 6 * np.sqrt(2 * dof)
        above += stat0 > dof0 + 6 * np.sqrt(2 * dof0)
    assert above >= 1


BLOCKS, BLOCK_N = 6, 5


def _block_ops(b):
    return ref.brickwork(BLOCK_N, 2, 300 + b) + [("cx", (0, 3), ()), ("ry", (2,), (0.3 + 0.1 * b,)), ("cx", (4, 1), ())]


def test_thirty_qubits_follow_the_density_matrix(monkeypatch):
    """Six independent 5-qubit blocks, each with non-adjacent cx, on 30 qubits -- beyond any statevector
    route -- through the backend on SamplingSimulator(method="automatic", mps_trajectories=True).  Two pairs
    inside every block: the chi-square of the counts the fit inverts, below dof + 6 sqrt(2 dof) against
    that block's exact tables.  One pair across two blocks: against the product of the two qubits'
    marginals."""
    from adaptaqc_amd import device, noise
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator

    n, shots = BLOCKS * BLOCK_N, 256
    ops = [(name, tuple(q + BLOCK_N * b for q in qs), params) for b in range(BLOCKS) for name, qs, params in _block_ops(b)]
    nm = ttref.model()
    effects = noise.readout_effects(n, nm)
    inside = [(0, 3), (4, 2)]
    pairs = [(a + BLOCK_N * b, c + BLOCK_N * b) for b in range(BLOCKS) for a, c in inside] + [(2, 28)]
    be = QiskitSamplingBackend(SamplingSimulator(method="automatic", seed=SEED, mps_trajectories=True),
                               tomography="device", trajectory_tomography=True)
    seen = []
    fit = device.tomo_fit

    def recording_fit(counts):
        seen.append(np.array(counts))
        return fit(counts)

    monkeypatch.setattr(device, "tomo_fit", recording_fit)
    rho, vals = be.pair_tomography(to_circuit(n, ops), pairs, {"shots": shots, "noise_model": nm}, "concurrence")
    (counts,) = seen
    assert rho.shape == (len(pairs), 4, 4) and np.all(np.isfinite(vals)) and np.all(counts.sum(axis=2) == shots)
    marginal = {}
    for b in range(BLOCKS):
        rows = noise.trajectory_program(to_circuit(BLOCK_N, _block_ops(b)), nm)[0]
        dm = tref.density_matrix(BLOCK_N, rows)
        exact = ttref.tables_of(dm, BLOCK_N, inside, effects[BLOCK_N * b: BLOCK_N * (b + 1)])
        for k, pair in enumerate(inside):
            stat, dof = _chi_square_of_pair(counts[2 * b + k], exact[k], shots)
            print(f"block {b} pair {pair}: chi-square {stat:.1f} at {dof} dof")
            assert stat < dof + 6 * np.sqrt(2 * dof)
        for q in range(BLOCK_N):
            marginal[BLOCK_N * b + q] = _one_qubit_marginal(dm, BLOCK_N, q)
    lo, hi = 2, 28
    product = np.kron(marginal[hi], marginal[lo])  # index 2 bit_hi + bit_lo: a two-qubit register (1, 0)
    exact = ttref.tables_of(product, 2, [(1, 0)], effects[[lo, hi]])
    stat, dof = _chi_square_of_pair(counts[-1], exact[0], shots)
    print(f"pair ({lo}, {hi}) across blocks: chi-square {stat:.1f} at {dof} dof")
    assert stat < dof + 6 * np.sqrt(2 * dof)


def _one_qubit_marginal(dm, n, q):
    """The 2x2 reduced density matrix of qubit q of the n-qubit density matrix dm."""
    t = dm.reshape((2,) * (2 * n))  # axes: row qubits n-1 .. 0, then column qubits n-1 .. 0
    t = np.moveaxis(t, [n - 1 - q, 2 * n - 1 - q], [0, 1]).reshape(2, 2, 2 ** (n - 1), 2 ** (n - 1))
    return np.trace(t, axis1=2, axis2=3)


def test_known_answers_on_forty_qubits():
    """x(39) followed by relaxation for time 0: qubit 39 reads 1 in basis Z in every trajectory of the ZZ
    setting (o = 2 for the pair (39, 0)); for a time far beyond T1 it reads 0."""
    from adaptaqc_amd import noise
    from adaptaqc_amd.circuit import QuantumCircuit
    from adaptaqc_amd.device import mps_trajectory_pair_tomography

    n, shots = 40, 12
    qc = QuantumCircuit(n)
    qc.x(39)
    gate = noise.trajectory_program(qc, None)[0]
    effects = noise.readout_effects(n, None)
    for time, o in ((0.0, 2), (1e6, 0)):
        rows = np.concatenate([gate, noise.kraus_row(noise.thermal_relaxation_error(50.0, 70.0, time), 39)])
        counts, outcomes = mps_trajectory_pair_tomography(n, rows, 1, [(39, 0)], effects, shots, 5, return_outcomes=True,
                                                          chi_cap=2)
        assert np.all(outcomes[8::9, 0] == o)
        want = [0, 0, 0, 0]
        want[o] = shots
        assert np.array_equal(counts[0, 8], want) and np.all(counts.sum(axis=2) == shots)


def _rank4_ops():
    # two Bell-like pairs across the middle bond of 4 qubits: Schmidt rank 4 there
    return [("ry", (0,), (np.pi / 2,)), ("cx", (0, 2), ()), ("ry", (1,), (np.pi / 2,)), ("cx", (1, 3), ())]


def test_backend_runs_the_device_call():
    """With method "matrix_product_state" and mps_trajectories, pair_tomography is tomo_fit and
    entanglement_measures of the device call with the same (seed, run) at chi_cap_for's capacity; an
    all-identity model takes the pure-state route bit for bit."""
    from adaptaqc_amd import noise
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.device import entanglement_measures, mps_trajectory_pair_tomography, tomo_fit
    from adaptaqc_amd.mps_operations import chi_cap_for

    n, shots = 4, 200
    nm = ttref.model()
    qc, rows, n_events, _ = ttref.program(n, 2)
    qc.measure(0, 0)  # tomography strips the classical operations
    pairs = [(0, 1), (3, 1), (2, 3)]
    effects = noise.readout_effects(n, nm)

    def backend(**flags):
        return QiskitSamplingBackend(SamplingSimulator(method="matrix_product_state", seed=5, mps_trajectories=True),
                                     tomography="device", **flags)

    be = backend(trajectory_tomography=True)
    for kwargs, seed, run in (({"seed_simulator": 7}, 7, 0), ({}, 5, 0), ({}, 5, 1)):
        rho, vals = be.pair_tomography(qc, pairs, dict(kwargs, shots=shots, noise_model=nm), "concurrence")
        want = tomo_fit(mps_trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, seed, run,
                                                       chi_cap=chi_cap_for(n, None)))
        assert np.array_equal(rho, want) and np.array_equal(vals, entanglement_measures(want, "concurrence"))
    assert be.simulator.runs == 2
    # no effective error: today's pure-state route
    identity = noise.NoiseModel()
    identity.add_all_qubit_quantum_error(noise.thermal_relaxation_error(50.0, 70.0, 0.0), ["rx", "cx", "h", "measure"])
    rho0, vals0 = backend().pair_tomography(qc, pairs, {"shots": shots, "seed_simulator": 7}, "eof")
    for model in (None, noise.NoiseModel(), identity):
        rho1, vals1 = be.pair_tomography(qc, pairs, {"shots": shots, "seed_simulator": 7, "noise_model": model}, "eof")
        assert np.array_equal(rho0, rho1) and np.array_equal(vals0, vals1)


def test_capacity_error_and_growth(monkeypatch):
    """chi_cap = 2 on a circuit that needs 4: the capacity error from the C entry.  The backend's route,
    started at a learned capacity of 2, grows it and returns the fit of the same trajectories."""
    from adaptaqc_amd import mps_operations as mops
    from adaptaqc_amd import noise
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.device import mps_trajectory_pair_tomography, tomo_fit

    n, shots = 4, 8
    qc = to_circuit(n, _rank4_ops())
    nm = ttref.model()
    rows, n_events, _ = noise.trajectory_program(qc, nm)
    effects = noise.readout_effects(n, nm)
    pairs = [(0, 2), (3, 1)]
    with pytest.raises(AqcError, match=r"capacity \(chi_cap\) exceeded"):
        mps_trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, 9, chi_cap=2)
    want = mps_trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, 9, chi_cap=4)
    assert want.shape == (2, 9, 4)  # the library still runs
    tried = []

    def small_start(n_, max_chi, loaded_max=1, learned=None):
        tried.append(max(2, (learned or {}).get(n_, 0)))
        return tried[-1]

    monkeypatch.setattr(mops, "chi_cap_for", small_start)
    be = QiskitSamplingBackend(SamplingSimulator(method="matrix_product_state", mps_trajectories=True),
                               tomography="device", trajectory_tomography=True)
    rho, _ = be.pair_tomography(qc, pairs, {"shots": shots, "seed_simulator": 9, "noise_model": nm})
    assert tried == [2, 4]
    assert np.array_equal(rho, tomo_fit(want))


def test_isl_compiles_under_a_noise_model():
    """ISL, the shot backend and a noise model together on the MPS engine.  The Rotoselect / Rotosolve
    tolerances sit at the shot noise of 1024 shots (3e-2): the defaults (1e-5, 1e-3) are never met by a
    sampled cost, and every cycle they add is a few noisy runs of 1024 MPS trajectories; with
    rotosolve_frequency = 2 the multi-layer Rotosolve, which adds nothing to what is tested here, does not
    run within the two layers."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig

    target = to_circuit(4, [("ry", (0,), (0.9,)), ("cx", (0, 1), ()), ("rx", (3,), (0.4,))])
    backend = QiskitSamplingBackend(SamplingSimulator(method="matrix_product_state", mps_trajectories=True),
                                    tomography="device", trajectory_tomography=True)
    config = AdaptConfig(method="ISL", max_layers=2, rotoselect_tol=3e-2, rotosolve_tol=3e-2, rotosolve_frequency=2)
    comp = AdaptCompiler(target, backend=backend, adapt_config=config,
                         execute_kwargs={"shots": 1024, "seed_simulator": 7, "noise_model": ttref.model()})
    result = comp.compile()
    history = result.entanglement_measures_history
    assert len(history) == len(result.qubit_pair_history) >= 1
    for ems in history:
        assert isinstance(ems, list) and len(ems) == len(comp.coupling_map)
        assert all(np.isfinite(v) and v >= 0 for v in ems)
    assert "ISL" in result.method_history
    assert all(0 <= c <= 1 for c in result.global_cost_history)


def test_refusals():
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.device import mps_trajectory_pair_tomography
    from adaptaqc_amd.noise import readout_effects, trajectory_program

    _, rows, n_events, effects = ttref.program(3, 1)
    for pairs in ([(0, 0)], [(0, 3)], [(-1, 1)], []):  # a bad pair; npairs = 0
        with pytest.raises(AqcError, match="-1"):
            mps_trajectory_pair_tomography(3, rows, n_events, pairs, effects, 4, 1)
    bad = effects.copy()
    bad[1, 1, 0, 0] += 1e-6  # E0 + E1 is no longer the identity
    with pytest.raises(AqcError, match="-1"):
        mps_trajectory_pair_tomography(3, rows, n_events, [(0, 1)], bad, 4, 1)
    bad = effects.copy()
    bad[2, 0, 0], bad[2, 0, 1] = (1.5, 0.5, 0, 0), (-0.5, 0.5, 0, 0)  # sums to I, but not positive
    with pytest.raises(AqcError, match="-1"):
        mps_trajectory_pair_tomography(3, rows, n_events, [(0, 1)], bad, 4, 1)
    bad = effects.copy()
    bad[0, 2, 1, 3] = np.nan
    with pytest.raises(AqcError, match="-1"):
        mps_trajectory_pair_tomography(3, rows, n_events, [(0, 1)], bad, 4, 1)
    u = np.full((36, n_events + 1), 0.5)
    u[20, n_events] = 1.0
    with pytest.raises(AqcError, match="-1"):
        mps_trajectory_pair_tomography(3, rows, n_events, [(0, 1)], effects, 4, 1, u=u)
    with pytest.raises(AqcError, match="-1"):
        mps_trajectory_pair_tomography(3, rows, n_events, [(0, 1)], effects, 0, 1)
    with pytest.raises(AqcError, match="-1"):  # n = 1: no pair
        mps_trajectory_pair_tomography(1, rows[:0], 0, [(0, 1)], effects[:1], 4, 1)
    with pytest.raises(AqcError, match="-1"):
        mps_trajectory_pair_tomography(3, rows, n_events, [(0, 1)], effects, 4, 1, chi_cap=0)
    with pytest.raises(ValueError, match="shape"):
        mps_trajectory_pair_tomography(3, rows, n_events, [(0, 1)], effects, 4, 1, u=u[:9])
    with pytest.raises(ValueError, match="n_events"):
        mps_trajectory_pair_tomography(3, rows, n_events + 1, [(0, 1)], effects, 4, 1)
    # chi_cap = 2 on a circuit that needs 4: the capacity error
    rank4 = trajectory_program(to_circuit(4, _rank4_ops()), None)[0]
    with pytest.raises(AqcError, match=r"capacity \(chi_cap\) exceeded"):
        mps_trajectory_pair_tomography(4, rank4, 0, [(0, 2)], readout_effects(4, None), 2, 1, chi_cap=2)
    # the library still runs after refusals
    assert mps_trajectory_pair_tomography(3, rows, n_events, [(0, 1)], effects, 4, 1).shape == (1, 9, 4)
