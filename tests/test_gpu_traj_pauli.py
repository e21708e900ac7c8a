"""The noisy Pauli readout on the device (csrc/traj.hip, aqc_sv_traj_pauli_counts) against the numpy
restatement of tests/pauli_traj_ref.py, and through QiskitSamplingBackend's ``pauli_terms="device"`` up
to a zero-noise extrapolation of an energy."""
import functools
import logging

import numpy as np
import pytest

import pauli_traj_ref as pref
import sampling_ref as ref
import traj_tomography_ref as ttref
import trajectory2_ref as t2ref
from conftest import to_circuit

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 23

TERMS_9 = ("IIIIIIIIX", "YIIIIIIII", "IIIIZIIII", "XIIIIIIIZ", "IIIYYIIII", "ZIZIIIIII", "IIIIIIXYI", "XIIIYIIIZ",
           "IIZZZIIII", "YYIIIIIIX", "IXIXIXIII", "XYZXIIIII", "IIIIIZZZZ", "YIYIYIYII", "XIIZIIYIX", "IIIIIIIZZ",
           "ZIIIIIIIZ", "IIIIXIIII", "IYIIIIIYI", "IIXXIIIII")
TERMS_11 = tuple(t + "II" for t in TERMS_9[:10]) + tuple("II" + t for t in TERMS_9[10:])

# (name, n, depth, shots, program, effects, terms).  program: "k1" the brickwork under
# traj_tomography_ref.model (one-qubit events), "k2b" trajectory2_ref's model "b" (a correlated group: the
# K2 kernels).  effects: "noisy" those of traj_tomography_ref.model (every factor general), "clean" the
# projectors (every factor a Pauli), ("mixed", qubits) noisy with the projectors on the named qubits.
# Threads are a quarter of the amplitudes within 64 .. 512: one wave up to 8 qubits, 2 at 9, 8 from 11.
CASES = [
    ("one term", 1, 2, 64, "k1", "noisy", ("Y",)),
    ("a K2 program, weights 1-3", 3, 2, 300, "k2b", "noisy", ("IIX", "IYI", "ZIY", "XXI", "XYZ", "ZZZ")),
    # 32 amplitudes, fewer than a wave; every weight; exactly 4 general factors, alone and beside a Pauli
    ("fewer amplitudes than a wave", 5, 3, 200, "k1", ("mixed", (2,)),
     ("IIIIZ", "IIYII", "XIIIY", "IZXII", "YIXIZ", "ZZYII", "XYIZX", "YYZZZ", "XYXZY", "ZZZZZ")),
    ("weight 5, every factor a Pauli", 5, 3, 200, "k1", "clean", ("XYZYX", "YYYYY", "ZZZZZ", "XXXXX", "YYIII", "IYYYI")),
    ("exactly 64 amplitudes", 6, 2, 100, "k1", "noisy", ("IIIIIX", "ZIIIIY", "XYIIZI", "IZZZZI")),
    # 2 waves, 20 terms; 2048 workgroups fit the device together, so some carry a second trajectory
    ("more terms than waves, more trajectories than workgroups", 9, 2, 2100, "k1", "noisy", TERMS_9),
    ("8 waves, 20 terms", 11, 2, 8, "k1", ("mixed", (4,)), TERMS_11),
    ("largest LDS state, fewer terms than waves", 13, 2, 4, "k1", "noisy",
     ("IIIIIIIIIIIIX", "ZIIIIIYIIIIIX", "IYIIZIIIIXIIY")),
    ("first global state", 14, 2, 2, "k1", "noisy", ("XIIIIIIIIIIIIZ", "IIIIIIYYIIIIII")),
]


def _effects(kind, n):
    from adaptaqc_amd.noise import readout_effects

    if kind == "clean":
        return readout_effects(n, None)
    noisy = readout_effects(n, ttref.model())
    return noisy if kind == "noisy" else pref.mixed_effects(n, noisy, kind[1])


@functools.lru_cache(maxsize=None)
def _case(n, depth, shots, program, effects_kind, terms):
    """The program, the uniforms of (seed, run) and the restatement's answer, computed once."""
    from adaptaqc_amd.paulis import terms_to_codes

    if program == "k2b":
        _, rows, n_events = t2ref.program(n, depth, "b")
    else:
        _, rows, n_events, _ = ttref.program(n, depth)
    effects = _effects(effects_kind, n)
    codes = terms_to_codes(list(terms), n)
    seed, run = SEED + n, 1
    u = ref.uniforms(seed, run, shots, n_events + len(terms))
    values, outcomes, plus, near = pref.pauli_counts(n, rows, codes, effects, u)
    for a in (rows, effects, codes, u, values, outcomes, plus, near):
        a.setflags(write=False)
    return rows, n_events, effects, codes, seed, run, u, values, outcomes, plus, near


@pytest.mark.parametrize("name,n,depth,shots,program,effects_kind,terms", CASES, ids=[c[0] for c in CASES])
def test_values_and_outcomes_against_restatement(name, n, depth, shots, program, effects_kind, terms):
    """Every value within 1e-10 (the statevector parity tolerance) of the restatement's, every outcome not
    flagged near a boundary equal to it, ``plus`` the count of the outcomes; with u passed in and with u
    drawn on the device from (seed, run)."""
    from adaptaqc_amd import noise
    from adaptaqc_amd.device import trajectory_pauli_counts

    rows, n_events, effects, codes, seed, run, u, want_v, want_o, want_plus, near = _case(
        n, depth, shots, program, effects_kind, terms)
    assert n_events > 0 and noise.has_correlated_rows(rows) == (program == "k2b")
    print(f"n={n} trajectories={shots} rows={len(rows)} events={n_events} terms={len(terms)} near={int(near.sum())}")
    assert near.sum() <= 2
    keep = ~near
    for kwargs in ({"u": u}, {}):
        plus, values, got = trajectory_pauli_counts(n, rows, n_events, list(terms), effects, shots, seed, run,
                                                    return_values=True, return_outcomes=True, **kwargs)
        assert plus.dtype == np.int64 and plus.shape == (len(terms),)
        assert values.shape == got.shape == (shots, len(terms)) and got.dtype == np.uint8
        worst = float(np.max(np.abs(values - want_v)))
        print(f"  largest difference in a value: {worst:.2e}")
        assert worst <= 1e-10
        bad = np.argwhere((got != want_o) & keep)
        assert bad.size == 0, (bad[:5], got[tuple(bad[:5].T)], want_o[tuple(bad[:5].T)])
        assert np.array_equal(plus, pref.plus_of(got))
        assert np.array_equal(pref.plus_of(got, keep), pref.plus_of(want_o, keep))
        if not near.any():
            assert np.array_equal(plus, want_plus)
    # a code array instead of labels, and without the optional outputs
    assert np.array_equal(trajectory_pauli_counts(n, rows, n_events, codes, effects, shots, seed, run), plus)


def _heisenberg_labels(n):
    from adaptaqc_amd.utils.hamiltonians import heisenberg_hamiltonian

    return heisenberg_hamiltonian(n, 1.0, 0.8, 0.6, hx=0.3, hz=0.5)


def test_law_follows_the_density_matrix():
    """n = 5, the Heisenberg terms, 4096 shots: per term plus / shots within 6 sqrt(p (1 - p) / shots) of
    the exact noisy p = (1 + Tr(rho M)) / 2; against the noiseless p at least one term outside that band."""
    from adaptaqc_amd.device import trajectory_pauli_counts
    from adaptaqc_amd.noise import readout_effects, trajectory_program
    from adaptaqc_amd.paulis import terms_to_codes

    n, shots = 5, 4096
    labels = list(_heisenberg_labels(n))
    codes = terms_to_codes(labels, n)
    qc, rows, n_events, effects = ttref.program(n, 3)
    plus = trajectory_pauli_counts(n, rows, n_events, labels, effects, shots, SEED, 0)
    p = (1 + pref.exact_values(n, rows, codes, effects)) / 2
    p0 = (1 + pref.exact_values(n, trajectory_program(qc, None)[0], codes, readout_effects(n, None))) / 2
    outside = 0
    for j, label in enumerate(labels):
        f = plus[j] / shots
        print(f"{label}: {f:.4f}; exact noisy p {p[j]:.4f}, noiseless {p0[j]:.4f}")
        assert abs(f - p[j]) <= 6 * np.sqrt(p[j] * (1 - p[j]) / shots), label
        outside += abs(f - p0[j]) > 6 * np.sqrt(p0[j] * (1 - p0[j]) / shots)
    assert outside >= 1


def test_same_law_as_the_circuit_route():
    """n = 4, an energy through expectation_value_of_pauli_operator with both ``pauli_terms`` settings at
    equal shots: every term of either route is a mean of ``shots`` +-1 draws of mean 2 p - 1, so the
    two energies differ by less than 6 combined standard deviations, sd^2 = 2 sum c^2 4 p (1 - p) / shots
    from the exact per-term p; each lies within 6 of its own of the exact energy."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.noise import readout_effects, trajectory_program
    from adaptaqc_amd.paulis import terms_to_codes
    from adaptaqc_amd.utils.circuit_operations import expectation_value_of_pauli_operator

    n, shots = 4, 2048
    nm = ttref.model()
    qc = to_circuit(n, ref.brickwork(n, 3, 100 + n))
    ham = _heisenberg_labels(n)
    ham["I" * n] = 0.25
    kwargs = {"shots": shots, "noise_model": nm}
    old = expectation_value_of_pauli_operator(qc, ham, QiskitSamplingBackend(SamplingSimulator(seed=11)), execute_kwargs=kwargs)
    new = expectation_value_of_pauli_operator(qc, ham, QiskitSamplingBackend(SamplingSimulator(seed=12), pauli_terms="device"),
                                              execute_kwargs=kwargs)
    labels = [label for label in ham if set(label) != {"I"}]
    coeff = np.array([ham[label] for label in labels])
    rows = trajectory_program(qc, nm)[0]
    v = pref.exact_values(n, rows, terms_to_codes(labels, n), readout_effects(n, nm))
    exact = 0.25 + float(coeff @ v)
    sd = np.sqrt(np.sum(coeff ** 2 * (1 - v ** 2)) / shots)  # 4 p (1 - p) = 1 - v^2
    print(f"exact {exact:.4f}, per-term circuits {old:.4f}, device {new:.4f}, sd of one route {sd:.4f}")
    assert abs(old - new) <= 6 * np.sqrt(2) * sd
    assert abs(old - exact) <= 6 * sd and abs(new - exact) <= 6 * sd


def test_known_answers():
    from adaptaqc_amd import noise
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.circuit import QuantumCircuit
    from adaptaqc_amd.device import trajectory_pauli_counts

    shots = 4000
    sim = SamplingSimulator(seed=3)
    # x, then Z through amplitude damping on measure: |1> reads +1 with probability gamma
    gamma = 0.3
    one = QuantumCircuit(2)
    one.x(1)
    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(noise.amplitude_damping_error(gamma), "measure")
    rows, n_events, _ = noise.trajectory_program(one, nm)
    assert n_events == 0  # readout errors only: still the trajectory route
    plus, values = trajectory_pauli_counts(2, rows, 0, ["ZI"], noise.readout_effects(2, nm), shots, 5,
                                           return_values=True)
    assert np.max(np.abs(values - (2 * gamma - 1))) < 1e-12
    assert abs(plus[0] / shots - gamma) <= 6 * np.sqrt(gamma * (1 - gamma) / shots)
    assert np.array_equal(sim.pauli_counts(one, ["ZI"], shots=shots, seed_simulator=5, noise_model=nm), plus)
    # |+> with depolarizing_error(p) on the readout h: <X> = 1 - p
    p = 0.2
    plus_state = QuantumCircuit(1)
    plus_state.ry(np.pi / 2, 0)
    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(noise.depolarizing_error(p), "h")
    got = sim.pauli_counts(plus_state, ["X"], shots=shots, noise_model=nm)
    q = 1 - p / 2
    assert abs(got[0] / shots - q) <= 6 * np.sqrt(q * (1 - q) / shots)
    # the noiseless device route on a Bell pair: ZZ and XX read +1 in every shot, YY never
    bell = QuantumCircuit(2)
    bell.h(0)
    bell.cx(0, 1)
    assert sim.pauli_counts(bell, ["ZZ", "XX", "YY"], shots=shots).tolist() == [shots, shots, 0]
    half = sim.pauli_counts(bell, ["ZI"], shots=shots)[0] / shots
    assert abs(half - 0.5) <= 6 * 0.5 / np.sqrt(shots)
    # and the same under a model without an effective error
    assert sim.pauli_counts(bell, ["ZZ", "XX"], shots=shots, noise_model=noise.NoiseModel()).tolist() == [shots, shots]


def test_deterministic_and_prefix():
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.device import trajectory_pauli_counts
    from adaptaqc_amd.noise import readout_effects
    from adaptaqc_amd.utils.circuit_operations import expectation_values_of_pauli_terms

    n, shots = 5, 700
    qc, rows, n_events, _ = ttref.program(n, 3)
    nm = ttref.model()
    effects = readout_effects(n, nm)
    labels = ["IIXZY", "YIIII", "ZZIXX", "IIIYI"]
    first = trajectory_pauli_counts(n, rows, n_events, labels, effects, shots, SEED, 2, return_values=True,
                                    return_outcomes=True)
    again = trajectory_pauli_counts(n, rows, n_events, labels, effects, shots, SEED, 2, return_values=True,
                                    return_outcomes=True)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)  # the same bits
    fewer = trajectory_pauli_counts(n, rows, n_events, labels, effects, 300, SEED, 2, return_values=True,
                                    return_outcomes=True)
    assert np.array_equal(fewer[1], first[1][:300]) and np.array_equal(fewer[2], first[2][:300])
    assert np.array_equal(fewer[0], pref.plus_of(first[2][:300]))
    other = trajectory_pauli_counts(n, rows, n_events, labels, effects, shots, SEED, 3, return_outcomes=True)
    assert not np.array_equal(other[1], first[2])
    # seed and run counter as SamplingSimulator.run: seed_simulator alone, else (seed, runs++)
    be = QiskitSamplingBackend(SamplingSimulator(seed=5), pauli_terms="device")
    for kwargs, seed, run in (({"seed_simulator": 7}, 7, 0), ({}, 5, 0), ({}, 5, 1)):
        got = expectation_values_of_pauli_terms(qc, ["IIIII"] + labels, be,
                                                execute_kwargs=dict(kwargs, shots=shots, noise_model=nm))
        want = trajectory_pauli_counts(n, rows, n_events, labels, effects, shots, seed, run)
        assert got[0] == 1.0 and np.array_equal(got[1:], (2.0 * want - shots) / shots)
    assert be.simulator.runs == 2


def test_refusals():
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.device import trajectory_pauli_counts
    from adaptaqc_amd.noise import readout_effects

    n = 5
    qc, rows, n_events, _ = ttref.program(n, 1)
    nm = ttref.model()
    effects = readout_effects(n, nm)

    def valid():
        plus = trajectory_pauli_counts(n, rows, n_events, ["XYZXI"], effects, 16, 1)
        assert plus.shape == (1,) and 0 <= plus[0] <= 16

    with pytest.raises(AqcError, match="general factors"):
        trajectory_pauli_counts(n, rows, n_events, ["XYZXZ"], effects, 16, 1)
    valid()
    sim = SamplingSimulator(method="matrix_product_state", mps_trajectories=True)
    with pytest.raises(NotImplementedError, match="Pauli readout of MPS trajectories is not built"):
        sim.pauli_counts(qc, ["XYZXI"], shots=16, noise_model=nm)
    assert sim.runs == 0
    valid()
    wide = np.zeros((1, 25), dtype=np.uint8)
    wide[0, 24] = 3
    with pytest.raises(AqcError, match="1 .. 24"):
        trajectory_pauli_counts(25, rows[:0], 0, wide, readout_effects(25, None), 16, 1)
    valid()


class _CountingSampler:
    """A SamplingSimulator that counts its ``pauli_counts`` and ``run`` calls."""

    def __new__(cls, **kwargs):
        from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator

        class Counting(SamplingSimulator):
            pauli_calls = run_calls = 0

            def pauli_counts(self, *args, **kw):
                self.pauli_calls += 1
                return super().pauli_counts(*args, **kw)

            def run(self, *args, **kw):
                self.run_calls += 1
                return super().run(*args, **kw)

        return Counting(**kwargs)


def test_zero_noise_extrapolation_of_an_energy(caplog):
    """The workflow the route is for: zero_noise_extrapolate with a 3-qubit energy under
    create_noisemodel as the measurement function -- one pauli_counts call (one trajectory launch) per
    point, no per-term circuit, a finite result."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend
    from adaptaqc_amd.utils.circuit_operations import (create_noisemodel, expectation_value_of_pauli_operator,
                                                       zero_noise_extrapolate)

    n, points = 3, 5
    qc = to_circuit(n, ref.brickwork(n, 3, 7))
    ham = _heisenberg_labels(n)
    nm = create_noisemodel(0.05, 0.07, log_fidelities=False)
    sim = _CountingSampler(seed=9)
    be = QiskitSamplingBackend(sim, pauli_terms="device")
    kwargs = {"noise_model": nm, "shots": 1024}
    with caplog.at_level(logging.WARNING):
        value = zero_noise_extrapolate(qc, lambda: expectation_value_of_pauli_operator(qc, ham, be, execute_kwargs=kwargs),
                                       num_points=points, rng=np.random.default_rng(1))
    refits = sum("Failed to zero-noise-extrapolate" in r.getMessage() for r in caplog.records)
    assert np.isfinite(value) and abs(value) <= sum(abs(c) for c in ham.values())
    assert sim.pauli_calls == points + refits and sim.run_calls == 0 and sim.runs == sim.pauli_calls
