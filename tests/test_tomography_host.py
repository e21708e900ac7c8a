"""Host side of shot-based pair tomography (no GPU): the identities of the numpy restatements
(tomography_ref.py), the "circuits" route on a stub simulator, and the constructor rules."""
import numpy as np
import pytest

import tomography_ref as tref


def _random_density(seed, rank=4, trace=1.0):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((4, rank)) + 1j * rng.standard_normal((4, rank))
    rho = g @ g.conj().T
    return trace * rho / np.trace(rho).real


def test_eigenvectors_and_rotation_convention():
    """Outcome 0 is the +1 eigenstate, and the measurement rotation (sdg then h for Y, h for X)
    maps the +1 / -1 eigenstates onto |0> / |1>."""
    h = np.array([[1, 1], [1, -1]]) / np.sqrt(2)
    sdg = np.diag([1, -1j])
    rot = [h, h @ sdg, np.eye(2)]
    for b in range(3):
        for o in range(2):
            v = tref.eigvec(b, o)
            np.testing.assert_allclose(tref.PAULI[b + 1] @ v, (1 - 2 * o) * v, atol=1e-15)
            assert abs(abs((rot[b] @ v)[o]) - 1) < 1e-15


def test_probabilities_sum_to_the_trace_per_setting():
    rhos = np.stack([_random_density(s, rank=1 + s % 4, trace=0.9 if s % 2 else 1.0) for s in range(8)])
    p = tref.pair_tomo_probs(rhos)
    assert p.shape == (8, 9, 4) and (p >= 0).all()
    np.testing.assert_allclose(p.sum(axis=2), np.trace(rhos, axis1=1, axis2=2).real[:, None] * np.ones(9), atol=1e-14)


def test_fit_of_exact_probabilities_returns_rho():
    rhos = np.stack([_random_density(s, rank=1 + s % 4) for s in range(8)])
    p = tref.pair_tomo_probs(rhos)
    np.testing.assert_allclose(tref.linear_inversion(p), rhos, atol=1e-14)
    np.testing.assert_allclose(tref.tomo_fit(p), rhos, atol=1e-13)
    # an unnormalised rho (a truncated MPS) comes back with trace 1
    np.testing.assert_allclose(tref.tomo_fit(0.8 * p), rhos, atol=1e-13)


@pytest.mark.parametrize("negative", [1, 2])
def test_psd_rescale_keeps_the_eigenvectors(negative):
    rng = np.random.default_rng(negative)
    q, _ = np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))
    mu = np.array([0.8, 0.45, -0.05, -0.2]) if negative == 2 else np.array([0.7, 0.3, 0.1, -0.1])
    h = (q * mu[None, :]) @ q.conj().T
    rho = tref.psd_rescale(h)
    lam = np.linalg.eigvalsh(rho)
    assert lam.min() >= -1e-15 and abs(np.trace(rho).real - 1) < 1e-14
    np.testing.assert_allclose(rho, rho.conj().T, atol=1e-15)
    np.testing.assert_allclose(rho @ h, h @ rho, atol=1e-14)  # same eigenvectors
    # the rule by hand: two negative -> a = -0.25, i = 2: (0.675, 0.325); one -> a = -0.1, i = 3
    want = [0.675, 0.325, 0, 0] if negative == 2 else [0.7 - 0.1 / 3, 0.3 - 0.1 / 3, 0.1 - 0.1 / 3, 0]
    np.testing.assert_allclose(np.sort(lam)[::-1], want, atol=1e-14)


def test_bound_probabilities_equal_the_two_copy_projectors():
    """P("1111") = Tr[(P- on the copies of qubit_1) (P- on the copies of qubit_2) rho (x) rho] and the
    one-sided ones, with P- = (1 - SWAP) / 2; rho_1 is the lower qubit (RDM index 2 hi + lo)."""
    swap = np.eye(4)[[0, 2, 1, 3]]
    pm = (np.eye(4) - swap) / 2
    for seed in range(4):
        rho = _random_density(seed, rank=1 + seed)

        # the operators on the 16-dimensional space of rho (x) rho (factors hiA, loA, hiB, loB)
        def on(qubits):  # P- on the two listed tensor factors
            op = np.zeros((16, 16))
            for i in range(16):
                for j in range(16):
                    bi = [(i >> (3 - k)) & 1 for k in range(4)]
                    bj = [(j >> (3 - k)) & 1 for k in range(4)]
                    if all(bi[k] == bj[k] for k in range(4) if k not in qubits):
                        a, b = qubits
                        op[i, j] = pm[2 * bi[a] + bi[b], 2 * bj[a] + bj[b]]
            return op

        p_hi, p_lo = on((0, 2)), on((1, 3))
        big = np.kron(rho, rho)
        want = [np.trace(p_lo @ p_hi @ big).real, np.trace(p_lo @ big).real, np.trace(p_hi @ big).real]
        np.testing.assert_allclose(tref.concurrence_bound_probs(rho[None])[0], want, atol=1e-14)


def test_multinomial_restatement_rule():
    p = np.array([[0, 0.25, 0.25, 0.5, 0]])
    for u, k in ((0.0, 1), (0.25, 2), (0.4999, 2), (0.5, 3), (np.nextafter(1.0, 0.0), 3)):
        got = tref.multinomial_counts(p, 1, u=np.array([[u]]))
        assert got.tolist() == [[int(j == k) for j in range(5)]], (u, got)
    c = tref.multinomial_counts(np.array([[0.1, 0.2, 0.3, 0.4], [4.0, 0.0, 0.0, 4.0]]), 1000, seed=3, run=1)
    assert c.dtype == np.int64 and c.sum(axis=1).tolist() == [1000, 1000] and c[1, 1] == c[1, 2] == 0
    with pytest.raises(ValueError):
        tref.multinomial_counts(np.zeros((1, 4)), 10, seed=1)


class TableSimulator:
    """Serves counts from a table keyed by the gates appended after the base circuit; records every
    circuit it is given."""

    def __init__(self, table, base_len):
        self.table = table
        self.base_len = base_len
        self.circuits = []
        self.kwargs = []

    def run(self, circuit, **kwargs):
        from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingJob, SamplingResult

        self.circuits.append(circuit)
        self.kwargs.append(kwargs)
        tail = tuple((i.operation.name, tuple(i.qubits)) for i in circuit.data[self.base_len:]
                     if i.operation.name != "measure")
        return SamplingJob(SamplingResult(self.table(tail) if callable(self.table) else self.table[tail]))


def _target():
    from adaptaqc_amd.circuit import QuantumCircuit

    qc = QuantumCircuit(4)
    qc.h(0)
    qc.cx(0, 3)
    qc.ry(0.3, 1)
    for q in range(4):
        qc.measure(q, q)
    return qc


def test_circuits_route_marginalisation_and_clbit_order():
    from adaptaqc_amd.backends.qiskit_sampling_backend import tomography_counts_from_circuits

    qc = _target()
    before = qc.copy()
    rot = {0: lambda q: (("h", (q,)),), 1: lambda q: (("sdg", (q,)), ("h", (q,))), 2: lambda q: ()}

    def table(tail):  # the setting is recognised by its rotations; counts differ per setting
        for s in range(9):
            if tail == rot[s % 3](1) + rot[s // 3](3):  # qubits ascending: lo = 1 first, then hi = 3
                return {"00": 10 + s, "01": 20 + s, "10": 30 + s, "11": 40 + s}
        raise AssertionError(f"unexpected rotations {tail}")

    sim = TableSimulator(table, base_len=3)
    got = tomography_counts_from_circuits(qc, 3, 1, sim, {"shots": 100, "seed_simulator": 4})
    # key "ab": a = clbit 1 = hi (qubit 3), b = clbit 0 = lo (qubit 1); o = 2 o_hi + o_lo
    want = np.array([[10 + s, 20 + s, 30 + s, 40 + s] for s in range(9)])
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert len(sim.circuits) == 9 and all(k == {"shots": 100, "seed_simulator": 4} for k in sim.kwargs)
    for c in sim.circuits:
        measures = [(i.qubits[0], i.clbits[0]) for i in c.data if i.operation.name == "measure"]
        assert measures == [(1, 0), (3, 1)] and c.num_clbits == 2
        assert [i.operation.name for i in c.data[-2:]] == ["measure", "measure"]
    assert qc == before and qc.num_clbits == 4  # the circuit passed in is left unmodified


def test_circuits_route_counts_follow_the_clbits():
    """Asymmetric counts: only "01" (hi reads 0, lo reads 1) -> column o = 1 whichever order the pair
    is given in."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import tomography_counts_from_circuits

    for pair in ((1, 3), (3, 1)):
        sim = TableSimulator(lambda tail: {"01": 7}, base_len=3)
        got = tomography_counts_from_circuits(_target(), *pair, sim, {})
        assert np.array_equal(got, np.tile([0, 7, 0, 0], (9, 1)))


def test_bound_circuits_route():
    from adaptaqc_amd.backends.qiskit_sampling_backend import concurrence_bound_counts_from_circuits

    qc = _target()
    sim = TableSimulator(lambda tail: {"1111": 10, "0011": 20, "1100": 30, "0000": 40}, base_len=6)
    got = concurrence_bound_counts_from_circuits(qc, 3, 1, sim, {"shots": 100})
    assert got == (0.1, 0.2, 0.3)
    assert [c.num_qubits for c in sim.circuits] == [8, 8, 8]
    m = [[(i.qubits[0], i.clbits[0]) for i in c.data if i.operation.name == "measure"] for c in sim.circuits]
    assert m == [[(3, 0), (7, 1), (1, 2), (5, 3)], [(3, 0), (7, 1)], [(1, 2), (5, 3)]]
    tail = [(i.operation.name, tuple(i.qubits)) for i in sim.circuits[0].data[6:] if i.operation.name != "measure"]
    assert tail == [("cx", (3, 7)), ("h", (3,)), ("cx", (1, 5)), ("h", (1,))]
    # both copies carry the gates
    assert [(i.operation.name, tuple(i.qubits)) for i in sim.circuits[0].data[:6]] == [
        ("h", (0,)), ("cx", (0, 3)), ("ry", (1,)), ("h", (4,)), ("cx", (4, 7)), ("ry", (5,))]


def test_constructor_rules():
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.circuit import QuantumCircuit
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig

    stub = TableSimulator({}, 0)
    qc = QuantumCircuit(3)
    qc.h(0)
    qc.cx(0, 1)
    assert QiskitSamplingBackend(stub).tomography is None
    with pytest.raises(NotImplementedError):  # tomography=None: ISL still raises
        AdaptCompiler(qc, backend=QiskitSamplingBackend(stub), adapt_config=AdaptConfig(method="ISL"))
    with pytest.raises(NotImplementedError):
        QiskitSamplingBackend(stub).pair_tomography(qc, [(0, 1)])
    with pytest.raises(TypeError):
        QiskitSamplingBackend(stub, tomography="device")
    with pytest.raises(ValueError):
        QiskitSamplingBackend(stub, tomography="tomography")
    assert QiskitSamplingBackend(SamplingSimulator(seed=1), tomography="device").tomography == "device"
    comp = AdaptCompiler(qc, backend=QiskitSamplingBackend(stub, tomography="circuits"),
                         adapt_config=AdaptConfig(method="ISL"))
    assert comp.adapt_config.method == "ISL" and comp.is_sampling_backend
    with pytest.raises(NotImplementedError, match="comm"):
        AdaptCompiler(qc, backend=QiskitSamplingBackend(stub, tomography="circuits"),
                      adapt_config=AdaptConfig(method="ISL"), comm=object())


@pytest.mark.parametrize("state", list(tref.STATES))
def test_restatement_chain_stays_inside_the_statistical_margin(state):
    """The margins of the GPU end-to-end tests, checked on the restatement alone for the states, shots
    and seed those tests use: the four measures of the fitted rho lie within 10 / sqrt(shots) of the
    exact ones (the scratch prototype measured a worst |C_fit - C_exact| of 5.2 / sqrt(shots) over
    200 Haar-random states; the margin is twice that), every entry of rho too, the lower bound
    does not exceed C^2 by more than the margin, and two independent draws (the device and the
    circuits route) differ by less than the margin per entry."""
    from oracle import entanglement as OE
    from oracle import sv as osv

    n, ops = tref.STATES[state]
    psi = osv.simulate(n, ops)
    pairs = tref.all_pairs(n)
    rhos = np.stack([OE.partial_trace_sv(psi, a, b) for a, b in pairs])
    fit, counts = tref.tomography(rhos, tref.SHOTS, tref.SEED)
    assert (counts.sum(axis=2) == tref.SHOTS).all()
    other, _ = tref.tomography(rhos, tref.SHOTS, tref.SEED + 1)
    lb = tref.concurrence_lower_bounds(rhos, tref.SHOTS, tref.SEED)
    worst = {}
    for r, f, g, b in zip(rhos, fit, other, lb):
        for method in OE.METHODS:
            worst[method] = max(worst.get(method, 0.0), abs(OE.measure(method, f) - tref.exact_measure(method, r)))
        worst["entry"] = max(worst.get("entry", 0.0), np.max(np.abs(f - r)))
        worst["draws"] = max(worst.get("draws", 0.0), np.max(np.abs(f - g)))
        worst["bound"] = max(worst.get("bound", 0.0), b - OE.concurrence(r) ** 2)
    print(state, {k: round(v * np.sqrt(tref.SHOTS), 2) for k, v in worst.items()}, "(x 1 / sqrt(shots))")
    assert not np.isnan(list(worst.values())).any() and max(worst.values()) < tref.MARGIN
