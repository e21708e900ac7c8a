"""The noisy Pauli readout on the MPS engine (csrc/mps_traj.hip, aqc_mps_traj_pauli_counts) against the
dense restatement of tests/mps_traj_pauli_ref.py, the statevector entry and the noiseless MPS engine,
and through QiskitSamplingBackend(SamplingSimulator(mps_trajectories=True, mps_pauli_readout=True),
pauli_terms="device") above 24 qubits and up to a zero-noise extrapolation of an energy."""
import functools
import itertools
import logging

import numpy as np
import pytest

import mps_traj_pauli_ref as mpref
import pauli_traj_ref as pref
import sampling_ref as ref
import traj_tomography_ref as ttref
from conftest import to_circuit

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 23


def _labels_of_weight(n, weights):
    """Every label of n qubits whose weight is in ``weights``, in a fixed order."""
    out = []
    for w in weights:
        for qs in itertools.combinations(range(n), w):
            for letters in itertools.product("XYZ", repeat=w):
                label = ["I"] * n
                for q, c in zip(qs, letters):
                    label[n - 1 - q] = c
                out.append("".join(label))
    return tuple(out)


def _mixed_labels(n, count):
    """One full-weight label, one with letters on qubits 0 and n - 1 only, the rest random over IIXYZ."""
    rng = np.random.default_rng(n)
    out = ["XYZ" * n, "Y" + "I" * (n - 2) + "X"]
    out[0] = out[0][:n]
    while len(out) < count:
        label = "".join(rng.choice(list("IIXYZ"), size=n))
        if set(label) != {"I"} and label not in out:
            out.append(label)
    return tuple(out)


# (n, depth, shots, chi_cap, t2, terms, forced readout sub-batch): the smallest case (lo = 0, hi = n - 1,
# dims 1 / 2 / 1); every support, identity gaps inside a support, lo > 0 and hi < n - 1; t2 < t1 and, read
# out 16 states at a time, 154 x 16 = 2464 items for a grid bounded by 2048, so the item loop wraps; a
# capacity far above the bonds (row stride != extent); the longest chains
CASES = [
    (2, 1, 64, 2, 70e3, _labels_of_weight(2, (1, 2)), 0),
    (4, 3, 60, 4, 70e3, _labels_of_weight(4, (1, 2, 3, 4)), 0),
    (6, 3, 32, 8, 30e3, _labels_of_weight(6, (1, 2)), 16),
    (8, 2, 24, 64, 70e3, _mixed_labels(8, 40), 0),
    (10, 2, 12, 32, 70e3, _mixed_labels(10, 24), 0),
]
N6, N8 = CASES[2], CASES[3]
assert [len(c[5]) for c in CASES] == [15, 255, 153, 40, 24]


@functools.lru_cache(maxsize=None)
def _case(n, depth, shots, chi_cap, t2, terms, readout):
    """The program, the uniforms of (seed, run) and the restatement's answer, computed once."""
    from adaptaqc_amd.paulis import terms_to_codes

    _, rows, n_events, effects = ttref.program(n, depth, t2)
    codes = terms_to_codes(list(terms), n)
    seed, run = SEED + n, 1
    u = ref.uniforms(seed, run, shots, n_events + len(terms))
    values, outcomes, plus, near = mpref.pauli_counts(n, rows, codes, effects, u)
    for a in (rows, effects, codes, u, values, outcomes, plus, near):
        a.setflags(write=False)
    return rows, n_events, effects, codes, seed, run, u, values, outcomes, plus, near


class _forced:
    """aqc_mps_traj_set_batch / aqc_mps_traj_set_readout_batch for the block, the defaults after it."""

    def __init__(self, batch=0, readout=0):
        self.batch, self.readout = batch, readout

    def __enter__(self):
        from adaptaqc_amd import _lib

        _lib.check(_lib.lib().aqc_mps_traj_set_batch(self.batch))
        _lib.check(_lib.lib().aqc_mps_traj_set_readout_batch(self.readout))

    def __exit__(self, *exc):
        from adaptaqc_amd import _lib

        _lib.check(_lib.lib().aqc_mps_traj_set_batch(0))
        _lib.check(_lib.lib().aqc_mps_traj_set_readout_batch(0))


@pytest.mark.parametrize("n,depth,shots,chi_cap,t2,terms,readout", CASES, ids=[f"n{c[0]}" for c in CASES])
def test_shot_by_shot_against_restatement(n, depth, shots, chi_cap, t2, terms, readout):
    """Every (trajectory, term) outcome not flagged near a boundary equals the restatement's, every value
    within 1e-6 of it (the project's MPS parity tolerance), every norm within 1e-6 of 1, ``plus`` the count
    of the outcomes; with u passed in and with u drawn on the device from (seed, run); at most 1 % of the
    entries flagged."""
    from adaptaqc_amd.device import mps_trajectory_pauli_counts

    rows, n_events, effects, codes, seed, run, u, want_v, want_o, want_plus, near = _case(
        n, depth, shots, chi_cap, t2, terms, readout)
    assert n_events > 0
    print(f"n={n} trajectories={shots} rows={len(rows)} events={n_events} terms={len(terms)} near={int(near.sum())}")
    assert near.sum() <= near.size // 100
    keep = ~near
    with _forced(readout=readout):
        for kwargs in ({"u": u}, {}):
            plus, values, norms, got = mps_trajectory_pauli_counts(
                n, rows, n_events, list(terms), effects, shots, seed, run, return_values=True, return_norms=True,
                return_outcomes=True, chi_cap=chi_cap, **kwargs)
            assert plus.dtype == np.int64 and plus.shape == (len(terms),)
            assert values.shape == got.shape == (shots, len(terms)) and got.dtype == np.uint8 and norms.shape == (shots,)
            worst, worst_w = float(np.max(np.abs(values - want_v))), float(np.max(np.abs(norms - 1.0)))
            print(f"  largest difference in a value: {worst:.2e}, in a norm: {worst_w:.2e}")
            assert worst <= 1e-6 and worst_w <= 1e-6
            bad = np.argwhere((got != want_o) & keep)
            assert bad.size == 0, (bad[:5], got[tuple(bad[:5].T)], want_o[tuple(bad[:5].T)])
            assert np.array_equal(plus, pref.plus_of(got))
            if not near.any():
                assert np.array_equal(plus, want_plus)
        # a code array instead of labels, and without the optional outputs
        assert np.array_equal(
            mps_trajectory_pauli_counts(n, rows, n_events, codes, effects, shots, seed, run, chi_cap=chi_cap), plus)


def test_agrees_with_the_statevector_entry():
    """n = 6 (at most 2 general factors a term, inside the statevector entry's 4), the same (seed, run):
    the outcomes of aqc_sv_traj_pauli_counts on every entry not flagged."""
    from adaptaqc_amd.device import mps_trajectory_pauli_counts, trajectory_pauli_counts

    n, _, shots, chi_cap, _, terms, _ = N6
    rows, n_events, effects, codes, seed, run = _case(*N6)[:6]
    near = _case(*N6)[-1]
    _, sv = trajectory_pauli_counts(n, rows, n_events, codes, effects, shots, seed, run, return_outcomes=True)
    _, mps = mps_trajectory_pauli_counts(n, rows, n_events, codes, effects, shots, seed, run, return_outcomes=True,
                                         chi_cap=chi_cap)
    assert np.array_equal(sv[~near], mps[~near])


def test_batch_independence_runs_and_prefix():
    """72 trajectories at capacity 64: the default batch, a forced batch of 32 (three batches, the last of
    8), that batch read out in sub-batches of 5 and a repeat call give the same bits in every output;
    another run does not; fewer shots give a prefix."""
    from adaptaqc_amd.device import mps_trajectory_pauli_counts

    n, _, _, chi_cap, _, terms, _ = N8
    rows, n_events, effects, codes = _case(*N8)[:4]

    def call(shots=72, run=2):
        return mps_trajectory_pauli_counts(n, rows, n_events, codes, effects, shots, 11, run, return_values=True,
                                           return_norms=True, return_outcomes=True, chi_cap=chi_cap)

    a = call()
    with _forced(batch=32):
        b = call()
    with _forced(batch=32, readout=5):
        c = call()
    for other in (b, c, call()):
        assert len(other) == 4
        for x, y in zip(a, other):
            assert np.array_equal(x, y)  # the same bits
    d = call(run=3)
    assert not np.array_equal(a[3], d[3])
    short = call(shots=10)
    assert np.array_equal(short[3], a[3][:10]) and np.array_equal(short[1], a[1][:10])
    assert np.array_equal(short[2], a[2][:10]) and np.array_equal(short[0], pref.plus_of(a[3][:10]))


# (depth, max_chi, where the norm lies).  The engine's truncation renormalises the kept singular values, so
# a truncated state loses or gains norm only through later updates of its no longer canonical bonds.  As
# measured on the device with DeviceMPS, the n = 6 brickwork of depth 3 under max_chi = 2 keeps
# <psi|psi> = 1 to nine digits, and under max_chi = 1 any circuit does (a renormalised product state);
# depth 8 under max_chi = 3 gives 0.999823 and depth 6 under max_chi = 2 gives 1.021436.
TRUNCATED = [(3, 2, "at 1"), (8, 3, "below 1"), (6, 2, "above 1")]


@pytest.mark.parametrize("depth,max_chi,norm_lies", TRUNCATED, ids=[f"depth{c[0]}_chi{c[1]}" for c in TRUNCATED])
def test_truncated_trajectories_against_the_noiseless_engine(depth, max_chi, norm_lies):
    """The n = 6 circuit without a noise model (no events, every D a Pauli) under a bond limit: every
    trajectory's values equal DeviceMPS.pauli_expect of the same circuit under the same truncation and its
    norm that state's all-identity term, both within 1e-6 (the project's truncated-MPS parity figure); the
    norm lies more than 1e-6 below 1 (above it in the third case: w > 1 is as little renormalised); the
    outcomes follow the rule of the header from the returned (values, norms, u)."""
    from adaptaqc_amd.circuit import device_ops_array
    from adaptaqc_amd.device import DeviceMPS, mps_trajectory_pauli_counts
    from adaptaqc_amd.noise import readout_effects, trajectory_program
    from adaptaqc_amd.paulis import terms_to_codes

    n, _, shots, chi_cap, _, terms, _ = N6
    qc = to_circuit(n, ref.brickwork(n, depth, 100 + n))
    rows, n_events, _ = trajectory_program(qc, None)
    assert n_events == 0
    effects = readout_effects(n, None)
    codes = terms_to_codes(list(terms), n)
    seed, run = SEED + n, 1
    u = ref.uniforms(seed, run, shots, len(terms))
    plus, values, norms, got = mps_trajectory_pauli_counts(n, rows, 0, codes, effects, shots, seed, run,
                                                           return_values=True, return_norms=True,
                                                           return_outcomes=True, chi_cap=chi_cap, max_chi=max_chi)
    mps = DeviceMPS(n, chi_cap, 1e-16, max_chi)
    mps.apply(device_ops_array(qc))
    want = mps.pauli_expect(np.concatenate([codes, np.zeros((1, n), dtype=np.uint8)]))
    mps.close()
    worst = float(np.max(np.abs(values - want[None, :-1])))
    worst_w = float(np.max(np.abs(norms - want[-1])))
    print(f"norm {want[-1]:.9f}; largest difference in a value: {worst:.2e}, in a norm: {worst_w:.2e}")
    assert worst <= 1e-6 and worst_w <= 1e-6
    if norm_lies == "below 1":
        assert np.all(norms < 1 - 1e-6)  # the case truncates
    elif norm_lies == "above 1":
        assert np.all(norms > 1 + 1e-6)
    pp = np.maximum(0.0, (norms[:, None] + values) / 2)
    pm = np.maximum(0.0, (norms[:, None] - values) / 2)
    clear = np.abs(pp - u * (pp + pm)) >= 1e-9 * (pp + pm)
    assert clear.mean() > 0.99
    assert np.array_equal(got[clear], (u * (pp + pm) >= pp).astype(np.uint8)[clear])
    assert np.array_equal(plus, pref.plus_of(got))


def test_law_follows_the_density_matrix():
    """n = 5, capacity 4, the 105 labels of weight 1 and 2, 64 shots: per term |plus - 64 p| below
    6 sqrt(64 p (1 - p)) for the exact noisy p = (1 + Tr(rho M)) / 2; against the noiseless p at least one
    term with p0 in [0.05, 0.95] beyond it.  (Per term, not pooled: terms share trajectories.  On the CPU
    the restatement's counts under these uniforms lie within 2.6 sigma of the noisy law and 6 terms beyond
    6 sigma of the noiseless one.)"""
    from adaptaqc_amd.device import mps_trajectory_pauli_counts
    from adaptaqc_amd.noise import readout_effects, trajectory_program
    from adaptaqc_amd.paulis import terms_to_codes

    n, shots = 5, 64
    labels = list(_labels_of_weight(n, (1, 2)))
    assert len(labels) == 105
    codes = terms_to_codes(labels, n)
    qc, rows, n_events, effects = ttref.program(n, 3)
    plus = mps_trajectory_pauli_counts(n, rows, n_events, labels, effects, shots, SEED, 0, chi_cap=4)
    p = (1 + pref.exact_values(n, rows, codes, effects)) / 2
    p0 = (1 + pref.exact_values(n, trajectory_program(qc, None)[0], codes, readout_effects(n, None))) / 2
    outside = 0
    for j, label in enumerate(labels):
        assert abs(plus[j] - shots * p[j]) < 6 * np.sqrt(shots * p[j] * (1 - p[j])), label
        if 0.05 <= p0[j] <= 0.95:
            outside += abs(plus[j] - shots * p0[j]) > 6 * np.sqrt(shots * p0[j] * (1 - p0[j]))
    print(f"terms beyond 6 sigma of the noiseless law: {outside}")
    assert outside >= 1


def test_twenty_six_qubits_end_to_end():
    """Above the statevector trajectories' 24 qubits: x on every qubit, each followed by full amplitude
    damping, so every qubit reads 0 with certainty -- every Z and ZZ value is exactly 1.0; one call
    advances the run counter once; without mps_pauli_readout the refusal stands."""
    from adaptaqc_amd import noise
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.circuit import QuantumCircuit
    from adaptaqc_amd.utils.circuit_operations import expectation_values_of_pauli_terms

    n, shots = 26, 8
    qc = QuantumCircuit(n)
    for q in range(n):
        qc.x(q)
    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(noise.amplitude_damping_error(1.0), "x")

    def label(letters):
        out = ["I"] * n
        for q, c in letters:
            out[n - 1 - q] = c
        return "".join(out)

    labels = ([label([(q, "Z")]) for q in range(n)] + [label([(q, "Z"), (q + 1, "Z")]) for q in range(n - 1)]
              + [label([(7, "X")])])
    kwargs = {"shots": shots, "noise_model": nm}
    sim = SamplingSimulator(seed=3, mps_trajectories=True, mps_pauli_readout=True)
    got = expectation_values_of_pauli_terms(qc, labels, QiskitSamplingBackend(sim, pauli_terms="device"),
                                            execute_kwargs=kwargs)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (2 * n,)
    assert np.all(got[:-1] == 1.0)
    assert -1.0 <= got[-1] <= 1.0
    assert sim.runs == 1
    plain = SamplingSimulator(seed=3, mps_trajectories=True)
    with pytest.raises(NotImplementedError, match="Pauli readout of MPS trajectories is not built"):
        expectation_values_of_pauli_terms(qc, labels, QiskitSamplingBackend(plain, pauli_terms="device"),
                                          execute_kwargs=kwargs)
    assert plain.runs == 0


def test_zero_noise_extrapolation_of_an_energy(caplog):
    """test_gpu_traj_pauli's workflow on the MPS engine: zero_noise_extrapolate with a 3-qubit energy under
    create_noisemodel -- one pauli_counts call per point, no per-term circuit, a finite result; and the
    unscaled energy is that of a direct mps_trajectory_pauli_counts call with the same (seed, run)."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.device import mps_trajectory_pauli_counts
    from adaptaqc_amd.mps_operations import chi_cap_for
    from adaptaqc_amd.noise import readout_effects, trajectory_program
    from adaptaqc_amd.utils.circuit_operations import (create_noisemodel, expectation_value_of_pauli_operator,
                                                       zero_noise_extrapolate)
    from adaptaqc_amd.utils.hamiltonians import heisenberg_hamiltonian

    class Counting(SamplingSimulator):
        pauli_calls = run_calls = 0

        def pauli_counts(self, *args, **kw):
            self.pauli_calls += 1
            return super().pauli_counts(*args, **kw)

        def run(self, *args, **kw):
            self.run_calls += 1
            return super().run(*args, **kw)

    n, points, shots = 3, 5, 1024
    qc = to_circuit(n, ref.brickwork(n, 3, 7))
    ham = heisenberg_hamiltonian(n, 1.0, 0.8, 0.6, hx=0.3, hz=0.5)
    nm = create_noisemodel(0.05, 0.07, log_fidelities=False)
    kwargs = {"noise_model": nm, "shots": shots}

    def simulator():
        return Counting(method="matrix_product_state", seed=9, mps_trajectories=True, mps_pauli_readout=True)

    # the unscaled energy: run 0 of seed 9
    sim = simulator()
    energy = expectation_value_of_pauli_operator(qc, ham, QiskitSamplingBackend(sim, pauli_terms="device"),
                                                 execute_kwargs=kwargs)
    assert sim.pauli_calls == 1 and sim.run_calls == 0 and sim.runs == 1
    labels = [label for label in ham if set(label) != {"I"}]
    rows, n_events, _ = trajectory_program(qc, nm)
    plus = mps_trajectory_pauli_counts(n, rows, n_events, labels, readout_effects(n, nm), shots, 9, 0,
                                       chi_cap=chi_cap_for(n, None, 1, {}))
    want = sum(ham[label] * (2.0 * plus[j] - shots) / shots for j, label in enumerate(labels))
    want += sum(c for label, c in ham.items() if set(label) == {"I"})
    assert abs(energy - want) <= 1e-12 * max(1.0, abs(want))

    sim = simulator()
    be = QiskitSamplingBackend(sim, pauli_terms="device")
    with caplog.at_level(logging.WARNING):
        value = zero_noise_extrapolate(qc, lambda: expectation_value_of_pauli_operator(qc, ham, be, execute_kwargs=kwargs),
                                       num_points=points, rng=np.random.default_rng(1))
    refits = sum("Failed to zero-noise-extrapolate" in r.getMessage() for r in caplog.records)
    assert np.isfinite(value) and abs(value) <= sum(abs(c) for c in ham.values())
    assert sim.pauli_calls == points + refits and sim.run_calls == 0 and sim.runs == sim.pauli_calls


def test_capacity_error_and_growth(monkeypatch):
    """chi_cap = 2 on a circuit that needs 4 (two Bell-like pairs across the middle bond): the capacity
    error from the C entry.  pauli_counts, started at a learned capacity of 2, grows it and returns the
    counts of the same trajectories, the run counter advanced once."""
    from adaptaqc_amd import mps_operations as mops
    from adaptaqc_amd import noise
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.device import mps_trajectory_pauli_counts

    n, shots = 4, 16
    qc = to_circuit(n, [("ry", (0,), (np.pi / 2,)), ("cx", (0, 2), ()), ("ry", (1,), (np.pi / 2,)), ("cx", (1, 3), ())])
    nm = ttref.model()
    rows, n_events, _ = noise.trajectory_program(qc, nm)
    effects = noise.readout_effects(n, nm)
    labels = ["IZIZ", "XIXI", "YYII", "IIIZ", "ZZZZ"]
    with pytest.raises(AqcError, match=r"capacity \(chi_cap\) exceeded"):
        mps_trajectory_pauli_counts(n, rows, n_events, labels, effects, shots, 9, chi_cap=2)
    want = mps_trajectory_pauli_counts(n, rows, n_events, labels, effects, shots, 9, chi_cap=4)
    assert want.shape == (len(labels),)  # the library still runs
    tried = []

    def small_start(n_, max_chi, loaded_max=1, learned=None):
        tried.append(max(2, (learned or {}).get(n_, 0)))
        return tried[-1]

    monkeypatch.setattr(mops, "chi_cap_for", small_start)
    sim = SamplingSimulator(method="matrix_product_state", seed=9, mps_trajectories=True, mps_pauli_readout=True)
    got = sim.pauli_counts(qc, labels, shots=shots, noise_model=nm)
    assert tried == [2, 4] and sim.runs == 1
    assert np.array_equal(got, want)
