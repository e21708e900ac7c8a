"""Noisy pair tomography on the device (csrc/traj.hip, aqc_sv_traj_pair_tomo) against the numpy
restatements of tests/traj_tomography_ref.py, and through QiskitSamplingBackend's
``trajectory_tomography`` flag up to an ISL compile under a noise model."""
import functools

import numpy as np
import pytest

import sampling_ref as ref
import tomography_ref as tomo
import traj_tomography_ref as ttref
from conftest import to_circuit

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 11

# (n, depth, shots, t2, pairs): one quadruple, the pair given hi-first; more trajectories than
# workgroups in flight; t2 on either side of t1 with every pair; the quadruple count against the
# thread count (9, 10), the widest and adjacent pairs; the largest LDS-resident state; the first
# global one
CASES = [
    (2, 1, 64, 70e3, ((1, 0),)),
    (3, 3, 500, 70e3, ((0, 1), (2, 0), (1, 2))),
    (5, 3, 200, 70e3, tuple(tomo.all_pairs(5))),
    (5, 3, 200, 30e3, tuple(tomo.all_pairs(5))),
    (9, 2, 16, 70e3, ((0, 8), (0, 1), (8, 7), (3, 4), (6, 2), (5, 7))),
    (10, 2, 16, 70e3, ((0, 9), (1, 0), (8, 9), (4, 5), (7, 2), (3, 6))),
    (13, 2, 4, 70e3, ((0, 12), (6, 5), (11, 3))),
    (14, 2, 2, 70e3, ((13, 0), (7, 8))),
]


@functools.lru_cache(maxsize=None)
def _case(n, depth, shots, t2, pairs):
    """The program, the uniforms of (seed, run) and the restatement's answer, computed once."""
    _, rows, n_events, effects = ttref.program(n, depth, t2)
    seed, run = SEED + n, 1
    u = ref.uniforms(seed, run, 9 * shots, n_events + len(pairs))
    want, want_counts, near = ttref.pair_tomography(n, rows, list(pairs), effects, u)
    for a in (rows, effects, u, want, want_counts, near):
        a.setflags(write=False)
    return rows, n_events, effects, seed, run, u, want, want_counts, near


@pytest.mark.parametrize("n,depth,shots,t2,pairs", CASES)
def test_shot_by_shot_against_restatement(n, depth, shots, t2, pairs):
    """The outcome of every pair in every trajectory (not flagged near a boundary) equals the
    restatement's, and so do the counts once the flagged trajectories are taken out of both; with u
    passed in and with u drawn on the device from (seed, run)."""
    from adaptaqc_amd.device import trajectory_pair_tomography

    rows, n_events, effects, seed, run, u, want, want_counts, near = _case(n, depth, shots, t2, pairs)
    assert n_events > 0
    print(f"n={n} trajectories={9 * shots} rows={len(rows)} events={n_events} pairs={len(pairs)} near={int(near.sum())}")
    assert near.sum() <= 2
    keep = ~near
    for kwargs in ({"u": u}, {}):
        counts, got = trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, seed, run,
                                                 return_outcomes=True, **kwargs)
        assert got.dtype == np.uint8 and got.shape == (9 * shots, len(pairs))
        assert counts.dtype == np.int64 and counts.shape == (len(pairs), 9, 4)
        bad = np.argwhere((got != want) & keep[:, None])
        assert bad.size == 0, (bad[:5], got[tuple(bad[:5].T)], want[tuple(bad[:5].T)])
        assert np.array_equal(counts, ttref.counts_of(got)) and np.all(counts.sum(axis=2) == shots)
        assert np.array_equal(ttref.counts_of(got, keep), ttref.counts_of(want, keep))
        if not near.any():
            assert np.array_equal(counts, want_counts)
    # without the outcomes
    assert np.array_equal(trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, seed, run), counts)


def _chi_square_of_pair(counts, tables, shots):
    """Pearson's chi-square of a pair's nine independent tables, summed, with the summed dof (27 less
    the merged cells)."""
    stat = dof = 0
    for s in range(9):
        x, d = ref.chi_square(counts[s], tables[s], shots)
        stat, dof = stat + x, dof + d
    return stat, dof


def test_law_follows_the_density_matrix():
    """n = 5, every pair, 4096 shots a setting: per pair, the chi-square over its nine tables against
    the exact noisy tables below dof + 6 sqrt(2 dof); against the noiseless tables above it for at
    least one pair.  (Not pooled over pairs: their tables share trajectories.)"""
    from adaptaqc_amd.device import trajectory_pair_tomography
    from adaptaqc_amd.noise import readout_effects, trajectory_program

    n, shots = 5, 4096
    pairs = tomo.all_pairs(n)
    qc, rows, n_events, effects = ttref.program(n, 3)
    counts = trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, SEED, 0)
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


def test_known_answers():
    from adaptaqc_amd import noise
    from adaptaqc_amd.circuit import QuantumCircuit
    from adaptaqc_amd.device import trajectory_pair_tomography

    shots = 300
    relax = noise.thermal_relaxation_error(50.0, 70.0, 1e6)
    # a Bell pair, then relaxation far beyond T1 on both qubits of cx: |00>, so ZZ reads 0 0
    bell = QuantumCircuit(3)
    bell.h(0)
    bell.cx(0, 2)
    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(relax.expand(relax), "cx")
    rows, n_events, _ = noise.trajectory_program(bell, nm)
    assert n_events == 2
    pairs = [(0, 2), (1, 0), (2, 1)]
    counts = trajectory_pair_tomography(3, rows, n_events, pairs, noise.readout_effects(3, nm), shots, 5)
    assert np.array_equal(counts[:, 8], [[shots, 0, 0, 0]] * 3)
    # x(0) with that relaxation on measure only: qubit 0 is |1>, and reads 0 in basis Z in every shot
    flip = QuantumCircuit(2)
    flip.x(0)
    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(relax, "measure")
    rows, n_events, _ = noise.trajectory_program(flip, nm)
    assert n_events == 0
    counts = trajectory_pair_tomography(2, rows, 0, [(0, 1)], noise.readout_effects(2, nm), shots, 5)
    assert np.all(counts[0, [2, 5, 8]][:, [1, 3]] == 0) and np.array_equal(counts[0, 8], [shots, 0, 0, 0])
    # with the projectors instead it reads 1
    counts = trajectory_pair_tomography(2, rows, 0, [(0, 1)], noise.readout_effects(2, None), shots, 5)
    assert np.array_equal(counts[0, 8], [0, shots, 0, 0])


def test_determinism_runs_and_prefix():
    from adaptaqc_amd.device import trajectory_pair_tomography

    n, shots = 6, 300
    pairs = tomo.all_pairs(n)
    _, rows, n_events, effects = ttref.program(n, 3)
    a = trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, 11, 2, return_outcomes=True)
    b = trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, 11, 2, return_outcomes=True)
    c = trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, 11, 3, return_outcomes=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[1], c[1])
    # a trajectory depends on (seed, run, t) only: a shorter call is a prefix of a longer one
    short = trajectory_pair_tomography(n, rows, n_events, pairs, effects, 10, 11, 2, return_outcomes=True)
    assert np.array_equal(short[1], a[1][:90]) and np.array_equal(short[0], ttref.counts_of(a[1][:90]))


def test_backend_runs_the_device_call():
    """With the flag, pair_tomography is tomo_fit and entanglement_measures of the device call with
    the same (seed, run); an all-identity model takes the pure-state route bit for bit."""
    from adaptaqc_amd import noise
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.device import entanglement_measures, tomo_fit, trajectory_pair_tomography
    from adaptaqc_amd.utils.entanglement_measures import EM_TOMOGRAPHY_CONCURRENCE, calculate_entanglement_measure

    n, shots = 4, 2000
    nm = ttref.model()
    qc, rows, n_events, _ = ttref.program(n, 2)
    qc.measure(0, 0)  # tomography strips the classical operations
    pairs = [(0, 1), (3, 1), (2, 3)]
    effects = noise.readout_effects(n, nm)
    be = QiskitSamplingBackend(SamplingSimulator(seed=5), tomography="device", trajectory_tomography=True)
    for kwargs, seed, run in (({"seed_simulator": 7}, 7, 0), ({}, 5, 0), ({}, 5, 1)):
        rho, vals = be.pair_tomography(qc, pairs, dict(kwargs, shots=shots, noise_model=nm), "concurrence")
        want = tomo_fit(trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, seed, run))
        assert np.array_equal(rho, want) and np.array_equal(vals, entanglement_measures(want, "concurrence"))
    assert be.simulator.runs == 2
    # the single-pair entry point of utils/entanglement_measures.py passes the kwargs through
    one = calculate_entanglement_measure(EM_TOMOGRAPHY_CONCURRENCE, qc, 3, 1, be,
                                         execute_kwargs={"shots": shots, "seed_simulator": 7, "noise_model": nm})
    want = tomo_fit(trajectory_pair_tomography(n, rows, n_events, [(3, 1)], effects, shots, 7, 0))
    assert one == float(entanglement_measures(want, "concurrence")[0])
    # no effective error: today's pure-state route
    identity = noise.NoiseModel()
    identity.add_all_qubit_quantum_error(noise.thermal_relaxation_error(50.0, 70.0, 0.0), ["rx", "cx", "h", "measure"])
    plain = QiskitSamplingBackend(SamplingSimulator(seed=5), tomography="device")
    rho0, vals0 = plain.pair_tomography(qc, pairs, {"shots": shots, "seed_simulator": 7}, "eof")
    for model in (None, noise.NoiseModel(), identity):
        rho1, vals1 = be.pair_tomography(qc, pairs, {"shots": shots, "seed_simulator": 7, "noise_model": model}, "eof")
        assert np.array_equal(rho0, rho1) and np.array_equal(vals0, vals1)


def test_backend_refusals():
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.circuit import QuantumCircuit

    nm = ttref.model()
    qc = to_circuit(3, ref.brickwork(3, 1, 1))
    kwargs = {"shots": 50, "noise_model": nm}
    mps = QiskitSamplingBackend(SamplingSimulator(method="matrix_product_state"), tomography="device",
                                trajectory_tomography=True)
    with pytest.raises(NotImplementedError, match="matrix_product_state"):
        mps.pair_tomography(qc, [(0, 1)], kwargs)
    big = QuantumCircuit(25)
    big.rx(0.3, 0)
    for method in ("statevector", "automatic"):
        be = QiskitSamplingBackend(SamplingSimulator(method=method), tomography="device", trajectory_tomography=True)
        with pytest.raises(NotImplementedError, match="24 qubits"):
            be.pair_tomography(big, [(0, 1)], kwargs)
        with pytest.raises(NotImplementedError, match="noise_model"):
            be.concurrence_lower_bounds(qc, [(0, 1)], kwargs)
        assert be.pair_tomography(qc, [(0, 1)], kwargs)[0].shape == (1, 4, 4)


def test_isl_compiles_under_a_noise_model():
    """The reference's defaults together -- ISL, the shot backend, a noise model -- on 3 qubits."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig

    target = to_circuit(3, [("ry", (0,), (0.9,)), ("cx", (0, 1), ()), ("rx", (2,), (0.4,)), ("cx", (1, 2), ())])
    comp = AdaptCompiler(target, backend=QiskitSamplingBackend(tomography="device", trajectory_tomography=True),
                         adapt_config=AdaptConfig(method="ISL", max_layers=2),
                         execute_kwargs={"shots": 2048, "seed_simulator": 7, "noise_model": ttref.model()})
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
    from adaptaqc_amd.device import trajectory_pair_tomography

    _, rows, n_events, effects = ttref.program(3, 1)
    for pairs in ([(0, 0)], [(0, 3)], [(-1, 1)], []):  # a bad pair; npairs = 0
        with pytest.raises(AqcError, match="-1"):
            trajectory_pair_tomography(3, rows, n_events, pairs, effects, 4, 1)
    bad = effects.copy()
    bad[1, 1, 0, 0] += 1e-6  # E0 + E1 is no longer the identity
    with pytest.raises(AqcError, match="-1"):
        trajectory_pair_tomography(3, rows, n_events, [(0, 1)], bad, 4, 1)
    bad = effects.copy()
    bad[2, 0, 0], bad[2, 0, 1] = (1.5, 0.5, 0, 0), (-0.5, 0.5, 0, 0)  # sums to I, but not positive
    with pytest.raises(AqcError, match="-1"):
        trajectory_pair_tomography(3, rows, n_events, [(0, 1)], bad, 4, 1)
    bad = effects.copy()
    bad[0, 2, 1, 3] = np.nan
    with pytest.raises(AqcError, match="-1"):
        trajectory_pair_tomography(3, rows, n_events, [(0, 1)], bad, 4, 1)
    u = np.full((36, n_events + 1), 0.5)
    u[20, n_events] = 1.0
    with pytest.raises(AqcError, match="-1"):
        trajectory_pair_tomography(3, rows, n_events, [(0, 1)], effects, 4, 1, u=u)
    with pytest.raises(AqcError, match="-1"):
        trajectory_pair_tomography(3, rows, n_events, [(0, 1)], effects, 0, 1)
    with pytest.raises(ValueError, match="shape"):
        trajectory_pair_tomography(3, rows, n_events, [(0, 1)], effects, 4, 1, u=u[:9])
    with pytest.raises(ValueError, match="n_events"):
        trajectory_pair_tomography(3, rows, n_events + 1, [(0, 1)], effects, 4, 1)
    # the library still runs after refusals
    assert trajectory_pair_tomography(3, rows, n_events, [(0, 1)], effects, 4, 1).shape == (1, 9, 4)
