"""Correlated two-qubit errors on the device's statevector trajectories (csrc/traj.hip: the Kraus groups of
aqc_sv_traj_sample and aqc_sv_traj_pair_tomo) against the numpy restatements of tests/trajectory2_ref.py,
and through SamplingSimulator / QiskitSamplingBackend.

The models: thermal relaxation after rx / ry / rz, so one-qubit Kraus rows interleave with the groups,
and on cx (a) depolarizing_error(0.05, 2): sixteen operators, weights independent of the state;
(b) collective decay, gamma = 0.3: two operators, state-dependent; (c) a seeded random channel of three
dense complex operators, state-dependent."""
import numpy as np
import pytest

import sampling_ref as ref
import traj_tomography_ref as ttref
import trajectory2_ref as t2ref
from conftest import to_circuit

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 3
KRAUS2 = t2ref.KRAUS2


def _compare(n, rows, n_events, shots, seed, run=1):
    """Outcome and choices of every shot not flagged near a boundary equal the restatement's, with u
    passed in and with u drawn on the device from (seed, run); at most 2 shots are flagged."""
    from adaptaqc_amd.device import trajectory_sample

    u = ref.uniforms(seed, run, shots, n_events + 1)
    want, want_k, near = t2ref.trajectories(n, rows, u)
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
    return got_k


# (n, depth, shots, model): the pair is the whole register (one quadruple, fewer than threads); more shots
# than workgroups, cx with q0 > q1 and on non-adjacent qubits; both kinds of group at 5 qubits; the
# quadruple count on either side of the thread count (9, 10); the largest LDS-resident state with the
# grown side area; the global-workspace path
CASES = [(2, 1, 512, "a"), (2, 1, 512, "b"), (2, 1, 512, "c"), (3, 2, 4097, "b"), (5, 3, 2048, "a"),
         (5, 3, 2048, "c"), (9, 2, 300, "c"), (10, 2, 256, "c"), (13, 2, 64, "b"), (14, 2, 32, "c"),
         (14, 2, 32, "a")]


@pytest.mark.parametrize("n,depth,shots,which", CASES)
def test_shot_by_shot_against_restatement(n, depth, shots, which):
    _, rows, n_events = t2ref.program(n, depth, which)
    firsts = np.flatnonzero((rows["flags"] & 0xFFFF) == KRAUS2)
    assert firsts.size > 0 and np.count_nonzero(rows["flags"] == 1) > 0  # both row kinds
    if n == 3:  # cx the other way round, and on non-adjacent qubits
        pairs = {(int(rows["q0"][i]), int(rows["q1"][i])) for i in firsts}
        assert (2, 0) in pairs and (0, 2) in pairs and (1, 0) in pairs and (0, 1) in pairs
    choices = _compare(n, rows, n_events, shots, SEED + n)
    if shots >= 512:  # the groups' events take more than the no-jump operator
        group_events = [e for e, (_, qs, ev) in enumerate(s for s in t2ref.events(rows) if s[2]) if len(qs) == 2]
        assert (choices[:, group_events] > 0).any()


def _padded_program(which, layout):
    """A 4-qubit program under model ``which`` from ``layout``: an int pads with that many noiseless
    one-qubit gates (h, x), a pair is a cx followed by its group, "r" an rx with its Kraus row."""
    from adaptaqc_amd.noise import trajectory_program

    ops, q = [], 0
    for item in layout:
        if isinstance(item, int):
            for _ in range(item):
                ops.append((("h", "x", "h")[q % 3], (q % 4,), ()))
                q += 1
        elif item == "r":
            ops.append(("rx", (q % 4,), (0.9,)))
            q += 1
        else:
            ops.append(("cx", item, ()))
    rows, n_events, _ = trajectory_program(to_circuit(4, ops), t2ref.model(which))
    return rows, n_events


def test_groups_across_chunks_of_sixteen_rows():
    """The kernel stages 16 rows at a time.  A sixteen-operator group that starts at row 10 of a chunk
    runs into the next one; so does a group whose first row is row 15, or row 14, of a chunk."""
    rows, n_events = _padded_program("a", [9, (0, 1), 4, (2, 1), "r", 2])
    firsts = [int(i) for i in np.flatnonzero((rows["flags"] & 0xFFFF) == KRAUS2)]
    assert firsts == [10, 31] and all(int(rows["flags"][i]) >> 16 == 16 for i in firsts)
    assert firsts[0] % 16 == 10 and firsts[0] // 16 != (firsts[0] + 15) // 16   # rows 10 .. 25
    assert firsts[1] % 16 == 15                                                   # rows 31 .. 46
    assert int(rows["flags"][48]) == 1 and n_events == 3
    _compare(4, rows, n_events, 1024, SEED + 31)
    # state-dependent groups of three: first rows at 15 and at 14 of a chunk
    rows, n_events = _padded_program("c", [14, (1, 3), "r", 9, (3, 0), "r", 1])
    firsts = [int(i) for i in np.flatnonzero((rows["flags"] & 0xFFFF) == KRAUS2)]
    assert firsts == [15, 30] and firsts[1] % 16 == 14 and all(int(rows["flags"][i]) >> 16 == 3 for i in firsts)
    assert n_events == 4
    _compare(4, rows, n_events, 1024, SEED + 32)


def _counts_to_array(counts, n):
    out = np.zeros(2 ** n, dtype=np.int64)
    for key, c in counts.items():
        out[int(key, 2)] = c
    return out


@pytest.mark.parametrize("which", ["a", "b"])
def test_distribution_follows_the_density_matrix(which):
    """65536 noisy shots through SamplingSimulator.run: Pearson chi-square against the diagonal of the
    density-matrix evolution below dof + 6 sqrt(2 dof); against the noiseless |psi|^2 above it."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.noise import trajectory_program

    n, shots = 5, 65536
    qc, rows, _ = t2ref.program(n, 3, which)
    counts = SamplingSimulator(seed=SEED).run(qc, shots=shots, noise_model=t2ref.model(which)).result().get_counts()
    obs = _counts_to_array(counts, n)
    assert obs.sum() == shots
    probs = np.real(np.diag(t2ref.density_matrix(n, rows)))
    stat, dof = ref.chi_square(obs, probs, shots)
    clean = np.real(np.diag(t2ref.density_matrix(n, trajectory_program(qc, None)[0])))
    stat0, dof0 = ref.chi_square(obs, clean, shots)
    print(f"model {which}: chi-square noisy {stat:.1f} at {dof} dof, against the noiseless law {stat0:.1f} at {dof0} dof")
    assert stat < dof + 6 * np.sqrt(2 * dof)
    assert stat0 > dof0 + 6 * np.sqrt(2 * dof0)


def test_known_answers():
    from adaptaqc_amd import noise
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.circuit import QuantumCircuit

    # collective decay with gamma = 1 on cx: K0 = diag(1, 1, 1, 0), K1 = |00><11|.
    # x(0) x(1) cx(0, 1): |11> -> qubit 0 = 1, qubit 1 = 0, index 2 b(q1) + b(q0) = 1, which K0 keeps: "01".
    # x(0) cx(0, 1): -> |11>, index 3, which K1 takes to |00>: "00".
    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(noise.QuantumError.two_qubit(t2ref.collective_decay(1.0)), "cx")
    for both, key in ((True, "01"), (False, "00")):
        qc = QuantumCircuit(2)
        qc.x(0)
        if both:
            qc.x(1)
        qc.cx(0, 1)
        assert SamplingSimulator(seed=3).run(qc, shots=1000, noise_model=nm).result().get_counts() == {key: 1000}
    # on non-adjacent qubits, the higher one listed first: x(2) cx(2, 0) -> both 1, which K1 takes to 0
    qc = QuantumCircuit(3)
    qc.x(2)
    qc.cx(2, 0)
    assert SamplingSimulator(seed=3).run(qc, shots=1000, noise_model=nm).result().get_counts() == {"000": 1000}
    # depolarizing after cx on |00>, rho -> (1 - p) rho + p I / 4: the uniform law over two qubits at
    # p = 1; at the bound p = 16/15 the identity has weight 0 and the fifteen Paulis 1/15 each, three of
    # which (IZ, ZI, ZZ) keep |00>: the law (3, 4, 4, 4) / 15, which a chi-square tells from the uniform one
    qc = QuantumCircuit(2)
    qc.cx(0, 1)
    shots = 16384
    bound = 3 + 6 * np.sqrt(2 * 3)
    for p, law in ((1.0, np.full(4, 0.25)), (16 / 15, np.array([3, 4, 4, 4]) / 15)):
        full = noise.NoiseModel()
        full.add_all_qubit_quantum_error(noise.depolarizing_error(p, 2), "cx")
        counts = SamplingSimulator(seed=5).run(qc, shots=shots, noise_model=full).result().get_counts()
        stat, dof = ref.chi_square(_counts_to_array(counts, 2), law, shots)
        print(f"p = {p:.4f}: chi-square {stat:.2f} at {dof} dof against {law}")
        assert dof == 3 and stat < bound
        if p > 1:
            assert ref.chi_square(_counts_to_array(counts, 2), np.full(4, 0.25), shots)[0] > bound
    # p = 0: the noiseless counts, bit for bit
    qc = to_circuit(5, ref.brickwork(5, 4, 2))
    zero = noise.NoiseModel()
    zero.add_all_qubit_quantum_error(noise.depolarizing_error(0.0, 2), "cx")
    sim = SamplingSimulator()
    want = sim.run(qc, shots=2000, seed_simulator=7).result().get_counts()
    assert sim.run(qc, shots=2000, seed_simulator=7, noise_model=zero).result().get_counts() == want


def test_determinism_and_runs():
    from adaptaqc_amd.device import trajectory_sample

    n, shots = 6, 3000
    for which in ("a", "c"):
        _, rows, n_events = t2ref.program(n, 3, which)
        a = trajectory_sample(n, rows, n_events, shots, 11, 2, return_choices=True)
        b = trajectory_sample(n, rows, n_events, shots, 11, 2, return_choices=True)
        c = trajectory_sample(n, rows, n_events, shots, 11, 3, return_choices=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[1], c[1])
        # a shot depends on (seed, run, shot) only: a shorter call is a prefix of a longer one
        assert np.array_equal(trajectory_sample(n, rows, n_events, 100, 11, 2), a[0][:100])


def test_pair_tomography_outcomes_against_restatement():
    """aqc_sv_traj_pair_tomo under model (c): every trajectory's outcome for every pair equals the
    restatement's (the state from trajectory2_ref.evolve, then the pair-draw rule of
    traj_tomography_ref), and the count table is the sum of the outcomes."""
    from adaptaqc_amd.device import trajectory_pair_tomography

    n, shots = 4, 60
    _, rows, n_events = t2ref.program(n, 2, "c")
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    pairs[1] = pairs[1][::-1]  # either way round
    effects = ttref.readout_effects_ref(n, ttref.kraus_of(ttref.model()))
    ntraj = 9 * shots
    u = ref.uniforms(SEED, 4, ntraj, n_events + len(pairs))
    psi, _, near, counted = t2ref.evolve(n, rows, u)
    assert counted == n_events
    setting = np.arange(ntraj) % 9
    want = np.zeros((ntraj, len(pairs)), dtype=np.uint8)
    for j, (a, b) in enumerate(pairs):
        p = ttref.setting_probs(psi, n, max(a, b), min(a, b), effects, setting)
        want[:, j], nr = ttref.draw(p, u[:, n_events + j])
        near |= nr
    print(f"pair tomography: {ntraj} trajectories, {n_events} events, near={int(near.sum())}")
    assert near.sum() <= 2
    counts, got = trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, SEED, 4, u=u, return_outcomes=True)
    assert got.shape == (ntraj, len(pairs)) and np.array_equal(got[~near], want[~near])
    assert np.array_equal(counts, ttref.counts_of(got)) and np.all(counts.sum(axis=2) == shots)
    drawn = trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, SEED, 4)  # u from (seed, run)
    assert np.array_equal(drawn, counts)


def test_backend_pair_tomography_under_depolarizing():
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator

    n = 4
    qc, _, _ = t2ref.program(n, 2, "a")
    be = QiskitSamplingBackend(SamplingSimulator(seed=9), tomography="device", trajectory_tomography=True)
    pairs = [(0, 1), (1, 2), (0, 3)]
    rho, measures = be.pair_tomography(qc, pairs, {"shots": 2048, "seed_simulator": 3, "noise_model": t2ref.model("a")},
                                       measure="concurrence")
    assert rho.shape == (3, 4, 4) and measures.shape == (3,)
    for r in rho:
        assert np.max(np.abs(r - r.conj().T)) < 1e-12 and abs(np.trace(r) - 1) < 1e-12
        assert np.linalg.eigvalsh(r).min() >= -1e-12
    # the fitted matrices lie near the exact noisy pair RDMs
    exact = t2ref.density_matrix(n, t2ref.program(n, 2, "a")[1])
    t = exact.reshape((2,) * (2 * n))
    for (a, b), r in zip(pairs, rho):
        hi, lo = max(a, b), min(a, b)
        m = np.moveaxis(t, [n - 1 - hi, n - 1 - lo, 2 * n - 1 - hi, 2 * n - 1 - lo], [0, 1, 2, 3])
        rdm = np.trace(m.reshape(2, 2, 2, 2, 2 ** (n - 2), 2 ** (n - 2)), axis1=4, axis2=5).reshape(4, 4)
        assert np.max(np.abs(r - rdm)) < 10 / np.sqrt(2048)


def test_compiler_runs_under_depolarizing_on_cx():
    """execute_kwargs={"noise_model": ...} with depolarizing_error(p, 2) on cx through AdaptCompiler: the
    first cost is the binomial mean of 1 - rho_{0..0} of its full circuit, and two layers compile."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig
    from adaptaqc_amd.noise import trajectory_program

    shots = 8192
    target = to_circuit(3, [("ry", (0,), (0.9,)), ("cx", (0, 1), ()), ("rx", (2,), (0.4,)), ("cx", (1, 2), ())])
    nm = t2ref.model("a")
    comp = AdaptCompiler(target, backend=QiskitSamplingBackend(),
                         execute_kwargs={"shots": shots, "seed_simulator": 7, "noise_model": nm},
                         adapt_config=AdaptConfig(method="expectation", max_layers=2))
    cost = comp.evaluate_cost()
    rows, n_events, _ = trajectory_program(comp.full_circuit, nm)
    p = 1 - float(np.real(t2ref.density_matrix(comp.full_circuit.num_qubits, rows)[0, 0]))
    assert n_events > 0 and abs(cost - p) < 6 * np.sqrt(p * (1 - p) / shots)
    result = comp.compile()
    assert len(result.global_cost_history) >= 2 and all(0 <= c <= 1 for c in result.global_cost_history)


def test_refusals():
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.device import trajectory_sample

    qc, rows, n_events = t2ref.program(3, 1, "a")
    nm = t2ref.model("a")
    match = "correlated.*24 qubits"
    for sim in (SamplingSimulator(method="matrix_product_state", mps_trajectories=True),):
        with pytest.raises(NotImplementedError, match=match):
            sim.run(qc, shots=10, noise_model=nm)
        be = QiskitSamplingBackend(sim, tomography="device", trajectory_tomography=True)
        with pytest.raises(NotImplementedError, match=match):
            be.pair_tomography(qc, [(0, 1)], {"shots": 10, "noise_model": nm})
    with pytest.raises(NotImplementedError):  # without mps_trajectories: the existing refusal
        SamplingSimulator(method="matrix_product_state").run(qc, shots=10, noise_model=nm)
    with pytest.raises(ValueError):
        trajectory_sample(3, rows, n_events + 1, 4, 1)  # n_events counts groups, not rows
    assert trajectory_sample(3, rows, n_events, 4, 1).shape == (4,)  # the library still runs afterwards
    plain = t2ref.program(3, 1, "a")[0]
    assert sum(SamplingSimulator(seed=1).run(plain, shots=50).result().get_counts().values()) == 50
