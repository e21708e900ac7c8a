"""The density-matrix engine on the device (csrc/dm.hip) against the numpy density-matrix evolution that the
trajectory tests already hold (trajectory2_ref.density_matrix, pauli_traj_ref.exact_values), its readers,
and DensityMatrixSimulator / DensityMatrixBackend on top of it.

Tolerance: the project's statevector parity tolerance, 1e-10 -- all arithmetic is FP64 and the entries of
rho are bounded by 1."""
import functools

import numpy as np
import pytest

import dm_ref
import pauli_traj_ref as ptref
import sampling_ref as ref
import traj_tomography_ref as ttref
import trajectory2_ref as t2ref
import trajectory_ref as tref
from conftest import to_circuit

pytestmark = pytest.mark.gpu

TOL = 1e-10


@functools.lru_cache(maxsize=None)
def _case(n, depth, which):
    """(rows, rho_ref) of t2ref.program, computed once and shared (read-only)."""
    _, rows, _ = t2ref.program(n, depth, which)
    rho = t2ref.density_matrix(n, rows)
    rho.setflags(write=False)
    return rows, rho


@functools.lru_cache(maxsize=None)
def _readout_case(n):
    """(circuit, rows, effects, rho_ref) of traj_tomography_ref.program(n, 3): relaxation after every gate,
    product errors on cx, errors on h / sdg / measure in the effects (general factors)."""
    qc, rows, _, effects = ttref.program(n, 3)
    rho = t2ref.density_matrix(n, rows)
    rho.setflags(write=False)
    return qc, rows, effects, rho


def _evolved(n, rows):
    from adaptaqc_amd.device import DeviceDM

    dev = DeviceDM(n)
    dev.run(rows)
    return dev


# n = 1, 2: the register is smaller than a two-qubit step's padding; 3: reversed and non-adjacent cx;
# 6: rho is exactly one 12-bit tile; 7: several workgroups and forced segment cuts; 9: column bits high in
# the index, 64 workgroups
RHO_CASES = [(1, 3, "a"), (2, 3, "a"), (2, 3, "b"), (2, 3, "c"), (3, 3, "a"), (3, 3, "b"), (3, 3, "c"),
             (6, 3, "a"), (6, 3, "c"), (7, 3, "a"), (7, 3, "b"), (7, 3, "c"), (9, 4, "c")]


@pytest.mark.parametrize("n,depth,which", RHO_CASES)
def test_rho_against_numpy_evolution(n, depth, which):
    from adaptaqc_amd.device import dm_plan

    rows, want = _case(n, depth, which)
    dev = _evolved(n, rows)
    got = dev.get()
    err = np.max(np.abs(got - want))
    herm = np.max(np.abs(got - got.conj().T))
    print(f"n={n} {which}: plan {dm_plan(n, rows)}, max entry error {err:.3e}, |Tr - 1| {abs(dev.trace() - 1):.3e}, "
          f"hermiticity {herm:.3e}")
    assert err <= TOL
    assert abs(dev.trace() - 1) <= TOL and abs(np.trace(got).real - 1) <= TOL
    assert herm <= TOL
    assert abs(dev.prob0() - want[0, 0].real) <= TOL
    dev.reset()
    assert dev.prob0() == 1.0 and dev.trace() == 1.0
    dev.close()


def test_two_runs_give_the_same_bits():
    rows, _ = _case(7, 3, "a")
    a = _evolved(7, rows)
    b = _evolved(7, rows)
    first = a.get()
    assert np.array_equal(first.view(np.float64), b.get().view(np.float64))
    a.reset()
    a.run(rows)
    assert np.array_equal(first.view(np.float64), a.get().view(np.float64))


def test_fusion_changes_nothing():
    """One run call against one row (or one group: a group is one channel) per call, which fuses nothing
    across calls: only the association of the folded matrix products differs, a rounding bound."""
    from adaptaqc_amd.device import DeviceDM

    rows, want = _case(7, 3, "a")
    whole = _evolved(7, rows).get()
    dev = DeviceDM(7)
    i = 0
    while i < len(rows):
        flags = int(rows["flags"][i])
        width = (flags >> 16) & 0xFF if flags & 0xFF == t2ref.KRAUS2 else 1
        dev.run(rows[i: i + width])
        i += width
    piecewise = dev.get()
    diff = np.max(np.abs(whole - piecewise))
    print(f"fused against row by row: max entry difference {diff:.3e}")
    assert diff <= 1e-12
    assert np.max(np.abs(piecewise - want)) <= TOL


def _terms(n):
    """Weight 1, 2 and n, mixed X / Y / Z, and one term of 5 factors (all general under the readout model)."""
    labels = ["I" * (n - 1) + "Z", "X" + "I" * (n - 1), "I" * (n - 2) + "YI", "I" * (n - 2) + "XZ",
              "Z" + "I" * (n - 2) + "Y", "XYZ" * n, "Z" * n, "I" * (n - 5) + "XYZYX"]
    return [lab[:n] for lab in labels]


@pytest.mark.parametrize("n", [5, 8])
def test_pauli_reader(n):
    from adaptaqc_amd.noise import readout_effects
    from adaptaqc_amd.paulis import terms_to_codes

    _, rows, effects, _ = _readout_case(n)
    labels = _terms(n)
    codes = terms_to_codes(labels, n)
    dev = _evolved(n, rows)
    # under the readout model every factor has an identity part: as many general factors as the weight
    want = ptref.exact_values(n, rows, codes, effects)
    got = dev.pauli_expect(labels, effects)
    print(f"n={n} noisy readout: max error {np.max(np.abs(got - want)):.3e}")
    assert np.max(np.abs(got - want)) <= TOL
    plain = ptref.exact_values(n, rows, codes, readout_effects(n, None))
    for eff in (None, readout_effects(n, None)):
        got = dev.pauli_expect(codes, eff)
        assert np.max(np.abs(got - plain)) <= TOL
    mixed = ptref.mixed_effects(n, effects, [0, n - 1])  # mask terms and general factors in one term
    assert np.max(np.abs(dev.pauli_expect(labels, mixed) - ptref.exact_values(n, rows, codes, mixed))) <= TOL
    assert np.array_equal(dev.pauli_expect(labels, effects), dev.pauli_expect(labels, effects))


@pytest.mark.parametrize("n", [5, 8])
def test_pair_rdms(n):
    from adaptaqc_amd.device import entanglement_measures

    _, rows, _, rho = _readout_case(n)
    pairs = [(a, b) for a in range(n) for b in range(n) if a != b]
    dev = _evolved(n, rows)
    got = dev.pair_rdms(pairs)
    want = np.stack([dm_ref.pair_rdm(rho, n, a, b) for a, b in pairs])
    print(f"n={n}: {len(pairs)} pairs, max error {np.max(np.abs(got - want)):.3e}")
    assert np.max(np.abs(got - want)) <= TOL
    for name in ("concurrence", "negativity"):
        em = entanglement_measures(got, name)
        assert np.max(np.abs(em - entanglement_measures(want, name))) <= 1e-8
    assert np.array_equal(got, dev.pair_rdms(pairs))


def test_diagonal_readers():
    n = 7
    rows, rho = _case(n, 3, "b")
    diag = np.diag(rho).real
    dev = _evolved(n, rows)
    probs = dev.probabilities()
    assert probs.shape == (2 ** n,) and np.max(np.abs(probs - diag)) <= TOL
    z_ref = np.array([np.sum(diag * (1 - 2 * ((np.arange(2 ** n) >> q) & 1))) for q in range(n)])
    assert np.max(np.abs(dev.z_all() - z_ref)) <= TOL
    shots = 4096
    u = np.random.default_rng(11).random(shots)
    got = dev.sample(shots, 5, u=u)
    want, near = ref.sv_sample(np.sqrt(probs), u)
    print(f"{int(near.sum())} of {shots} shots within 1e-12 of a CDF boundary")
    assert near.sum() <= shots // 100
    assert np.array_equal(got.astype(np.int64)[~near], want[~near])
    assert np.array_equal(dev.sample(shots, 5, 3), dev.sample(shots, 5, 3))
    # a statevector of another size is refused and left as it was
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import DeviceSV

    other = DeviceSV(n + 1)
    assert _lib.lib().aqc_dm_diag_sv(dev.h, other.h) == -1
    assert other.amp0() == 1.0


def test_largest_size_product_form():
    """n = 13 (1 GiB: byte offsets past 2^31) with a product-form program: one rotation and one relaxation
    row per qubit, a depolarized cx on (11, 12) and on (0, 1); the expected rho is the Kronecker product of
    the pairs' 4x4 and the other qubits' 2x2 matrices, evolved in numpy."""
    from adaptaqc_amd import noise
    from adaptaqc_amd.noise import trajectory_program

    n = 13
    rng = np.random.default_rng(13)
    angles = rng.uniform(0.3, 2.8, n)
    names = [["rx", "ry"][q % 2] for q in range(n)]
    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(noise.thermal_relaxation_error(50e3, 70e3, 9000), ["rx", "ry"])
    nm.add_all_qubit_quantum_error(noise.depolarizing_error(0.05, 2), "cx")

    def program(qubits, cx):
        ops = [(names[q], (i,), (angles[q],)) for i, q in enumerate(qubits)] + [("cx", c, ()) for c in cx]
        return trajectory_program(to_circuit(len(qubits), ops), nm)[0]

    ops = [(names[q], (q,), (angles[q],)) for q in range(n)] + [("cx", (11, 12), ()), ("cx", (0, 1), ())]
    rows = trajectory_program(to_circuit(n, ops), nm)[0]
    # the factors, lowest qubits first: (0, 1), 2 .. 10, (11, 12)
    factors = [t2ref.density_matrix(2, program((0, 1), [(0, 1)]))]
    factors += [t2ref.density_matrix(1, program((q,), [])) for q in range(2, 11)]
    factors += [t2ref.density_matrix(2, program((11, 12), [(0, 1)]))]
    first = [0] + list(range(2, 11)) + [11]  # a factor's lowest qubit
    paulis = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0])}

    def value(label):  # qiskit order: rightmost character = qubit 0
        out = 1.0
        for f, q0 in zip(factors, first):
            width = 1 if f.shape[0] == 2 else 2
            op = dm_ref.kron_all([paulis[label[n - 1 - (q0 + i)]] for i in range(width)])
            out *= np.trace(f @ op).real
        return out

    def label(**at):
        chars = ["I"] * n
        for q, c in at.items():
            chars[n - 1 - int(q[1:])] = c
        return "".join(chars)

    labels = [label(q12="Z"), label(q11="X", q12="X"), label(q0="Z"), label(q0="Y", q1="X"), label(q5="Z", q6="Z"),
              label(q1="Z", q7="X", q11="Y", q12="Z")]
    dev = _evolved(n, rows)
    prob0 = np.prod([f[0, 0].real for f in factors])
    z_ref = np.array([value(label(**{f"q{q}": "Z"})) for q in range(n)])
    got = dev.pauli_expect(labels)
    want = np.array([value(lab) for lab in labels])
    print(f"n=13: prob0 error {abs(dev.prob0() - prob0):.3e}, |Tr - 1| {abs(dev.trace() - 1):.3e}, "
          f"z error {np.max(np.abs(dev.z_all() - z_ref)):.3e}, Pauli error {np.max(np.abs(got - want)):.3e}")
    assert abs(dev.prob0() - prob0) <= TOL and abs(dev.trace() - 1) <= TOL
    assert np.max(np.abs(dev.z_all() - z_ref)) <= TOL
    assert np.max(np.abs(got - want)) <= TOL
    rdm = dev.pair_rdms([(12, 11), (3, 12)])
    assert np.max(np.abs(rdm[0] - factors[-1])) <= TOL
    assert np.max(np.abs(rdm[1] - np.kron(np.trace(factors[-1].reshape(2, 2, 2, 2), axis1=1, axis2=3), factors[2]))) <= TOL
    dev.close()


def test_simulator_counts_and_pauli_counts():
    from adaptaqc_amd.backends import DensityMatrixSimulator, QiskitSamplingBackend
    from adaptaqc_amd.noise import readout_effects, trajectory_program
    from adaptaqc_amd.paulis import terms_to_codes

    n, shots = 5, 8192
    qc, rows, _ = t2ref.program(n, 3, "b")
    nm = t2ref.model("b")
    sim = DensityMatrixSimulator(seed=17)
    counts = sim.run(qc, shots=shots, seed_simulator=5, noise_model=nm).result().get_counts()
    assert sum(counts.values()) == shots and all(len(k) == n for k in counts)
    obs = np.zeros(2 ** n)
    for k, v in counts.items():
        obs[int(k, 2)] = v
    probs = np.diag(_case(n, 3, "b")[1]).real
    clean = np.diag(t2ref.density_matrix(n, trajectory_program(qc, None)[0])).real
    stat, dof = ref.chi_square(obs, probs, shots)
    stat0, dof0 = ref.chi_square(obs, clean, shots)
    print(f"chi-square noisy {stat:.1f} at {dof} dof, against the noiseless law {stat0:.1f} at {dof0} dof")
    assert stat < dof + 6 * np.sqrt(2 * dof)
    assert stat0 > dof0 + 6 * np.sqrt(2 * dof0)
    assert sim.run(qc, shots=shots, seed_simulator=5, noise_model=nm).result().get_counts() == counts
    assert sim.run(qc, shots=shots, noise_model=nm).result().get_counts() != \
        sim.run(qc, shots=shots, noise_model=nm).result().get_counts()  # the run counter advances
    # measured circuits: keys over the classical bits, an unmeasured one reads 0
    part = qc.copy()
    part.measure(3, 0)
    part.measure(1, 2)
    keys = sim.run(part, shots=256, seed_simulator=1, noise_model=nm).result().get_counts()
    assert all(len(k) == 3 and k[1] == "0" for k in keys)
    # the Pauli readout under the readout model
    qc2, rows2, _, _ = _readout_case(n)
    nm2 = ttref.model()
    labels = _terms(n)
    want = ptref.exact_values(n, rows2, terms_to_codes(labels, n), readout_effects(n, nm2))
    assert np.max(np.abs(sim.pauli_values(qc2, labels, nm2) - want)) <= TOL
    plus = sim.pauli_counts(qc2, labels, shots=shots, seed_simulator=9, noise_model=nm2)
    est = (2 * plus - shots) / shots
    sd = np.sqrt(np.maximum(1 - want ** 2, 0) / shots)
    print("pauli_counts: estimate - exact in standard deviations", np.round((est - want) / sd, 2))
    assert np.all(np.abs(est - want) <= 6 * sd)
    assert np.array_equal(plus, sim.pauli_counts(qc2, labels, shots=shots, seed_simulator=9, noise_model=nm2))
    # through the sampling backend as it is
    be = QiskitSamplingBackend(DensityMatrixSimulator(seed=2), pauli_terms="device", tomography="circuits")
    rho, _ = be.pair_tomography(qc2, [(0, 1)], {"shots": 2048, "seed_simulator": 3, "noise_model": nm2})
    assert rho.shape == (1, 4, 4) and abs(np.trace(rho[0]).real - 1) < 1e-9


def _measured_rows(circuit, nm):
    from adaptaqc_amd.noise import trajectory_program

    qc = circuit.copy()
    qc.data = [ins for ins in qc.data if ins.operation.name != "measure"]
    for q in range(qc.num_qubits):
        qc.measure(q, q)
    return trajectory_program(qc, nm)[0]


def test_backend_costs_and_isl_compile():
    from adaptaqc_amd.backends import DensityMatrixBackend
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig

    nm = ttref.model()
    target = to_circuit(4, ref.brickwork(4, 2, 104))
    be = DensityMatrixBackend()
    comp = AdaptCompiler(target, backend=be, execute_kwargs={"noise_model": nm})
    before = [ins.operation.name for ins in comp.full_circuit.data]
    rho = tref.density_matrix(4, _measured_rows(comp.full_circuit, nm))
    diag = np.diag(rho).real
    cost = be.evaluate_global_cost(comp)
    marginal = np.mean([np.sum(diag[((np.arange(16) >> q) & 1) == 1]) for q in range(4)])
    local = be.evaluate_local_cost(comp)
    print(f"global cost {cost:.12f} (error {abs(cost - (1 - diag[0])):.3e}), local cost {local:.12f} "
          f"(error {abs(local - marginal):.3e})")
    assert abs(cost - (1 - diag[0])) <= TOL and abs(local - marginal) <= TOL
    assert be.evaluate_global_cost(comp) == cost and be.evaluate_local_cost(comp) == local
    z = be.measure_qubit_expectation_values(comp)
    assert np.max(np.abs(np.array(z) - [np.sum(diag * (1 - 2 * ((np.arange(16) >> q) & 1))) for q in range(4)])) <= TOL
    dist = be.evaluate_circuit(comp)
    assert abs(sum(dist.values()) - 1) <= TOL and abs(dist["0000"] - diag[0]) <= TOL
    assert [ins.operation.name for ins in comp.full_circuit.data] == before  # the compiler's circuit is untouched

    target = to_circuit(3, [("ry", (0,), (0.9,)), ("cx", (0, 1), ()), ("rx", (2,), (0.4,)), ("cx", (1, 2), ())])
    comp = AdaptCompiler(target, backend=DensityMatrixBackend(), adapt_config=AdaptConfig(method="ISL", max_layers=3),
                         execute_kwargs={"noise_model": nm})
    result = comp.compile()
    assert "ISL" in result.method_history and len(result.entanglement_measures_history) >= 1
    final = result.global_cost_history[-1]
    rho = tref.density_matrix(3, _measured_rows(comp.full_circuit, nm))
    print(f"ISL: final cost {final:.12f}, recomputed {1 - rho[0, 0].real:.12f}, history {result.global_cost_history}")
    assert abs(final - (1 - rho[0, 0].real)) <= 1e-9
    assert abs(result.overlap - rho[0, 0].real) <= 1e-9
