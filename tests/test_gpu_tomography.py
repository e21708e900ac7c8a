"""Shot-based pair tomography on MI355X (csrc/tomo.hip): each routine against its numpy restatement
(tomography_ref.py), the marginal route against the rotated circuit, the device mode of the sampling
backend end to end, device against circuits mode, and an ISL compile on the sampling backend."""
import numpy as np
import pytest

import sampling_ref as sref
import tomography_ref as tref
from conftest import to_circuit
from oracle import entanglement as OE
from oracle import sv as osv

pytestmark = pytest.mark.gpu

BRICK = sref.brickwork(4, 4, 21)
SEED = 2 ** 40 + 3


def _device(engine, n, ops):
    from adaptaqc_amd.circuit import device_ops
    from adaptaqc_amd.device import DeviceMPS, DeviceSV

    d = DeviceSV(n) if engine == "sv" else DeviceMPS(n, 8, 1e-16, None)
    d.apply(device_ops(to_circuit(n, ops)))
    return d


@pytest.fixture(scope="module")
def brick_rdms():
    """RDMs of every pair of the 4-qubit brickwork from both engines (computed once, read only)."""
    out = {e: _device(e, 4, BRICK).pair_rdms(tref.all_pairs(4)) for e in ("sv", "mps")}
    for r in out.values():
        r.setflags(write=False)
    return out


@pytest.mark.parametrize("engine", ["sv", "mps"])
def test_probabilities_match_restatement(engine, brick_rdms):
    from adaptaqc_amd.device import concurrence_bound_probs, pair_tomo_probs

    rdms = brick_rdms[engine]
    got = pair_tomo_probs(rdms)
    assert got.shape == (6, 9, 4) and (got >= 0).all()
    np.testing.assert_allclose(got, tref.pair_tomo_probs(rdms), atol=1e-13, rtol=0)
    np.testing.assert_allclose(got.sum(axis=2), 1.0, atol=1e-12)
    np.testing.assert_allclose(concurrence_bound_probs(rdms), tref.concurrence_bound_probs(rdms), atol=1e-13, rtol=0)


@pytest.mark.parametrize("engine", ["sv", "mps"])
def test_probabilities_match_the_rotated_circuit(engine, brick_rdms):
    """Pair (0, 2), settings XY and ZX (hi letter first): the exact outcome probabilities of the
    circuit with the basis rotations appended, from the oracle's statevector."""
    from adaptaqc_amd.device import pair_tomo_probs

    probs = pair_tomo_probs(brick_rdms[engine])[tref.all_pairs(4).index((0, 2))]
    rot = {"X": lambda q: [("h", (q,), ())], "Y": lambda q: [("sdg", (q,), ()), ("h", (q,), ())], "Z": lambda q: []}
    for hi_letter, lo_letter in ("XY", "ZX"):
        s = 3 * "XYZ".index(hi_letter) + "XYZ".index(lo_letter)
        p = np.abs(osv.simulate(4, BRICK + rot[lo_letter](0) + rot[hi_letter](2))) ** 2
        k = np.arange(16)
        want = [p[((k >> 2) & 1 == o >> 1) & ((k & 1) == (o & 1))].sum() for o in range(4)]
        np.testing.assert_allclose(probs[s], want, atol=1e-12, rtol=0)


def _job_probs(njobs, K, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.0, 1.0, (njobs, K))
    p[rng.uniform(size=p.shape) < 0.2] = 0.0  # some outcomes impossible
    p[:, rng.integers(K)] += 0.1              # no all-zero row
    return p * rng.uniform(0.5, 1.0, (njobs, 1))  # rows need not sum to 1


@pytest.mark.parametrize("K", [2, 3, 4, 16])
@pytest.mark.parametrize("njobs", [1, 9, 37])
def test_multinomial_counts_are_the_restatements(K, njobs):
    from adaptaqc_amd.device import multinomial_counts

    p = _job_probs(njobs, K, 100 * K + njobs)
    for shots in (1, 63, 64, 65, 1000, 8192):
        want = tref.multinomial_counts(p, shots, seed=SEED, run=3)
        got = multinomial_counts(p, shots, SEED, 3)
        assert got.dtype == np.int64 and got.shape == (njobs, K)
        assert np.array_equal(got, want), (shots, np.abs(got - want).max())
        assert (got.sum(axis=1) == shots).all()
        assert np.array_equal(multinomial_counts(p, shots, SEED, 3), got)  # identical across calls
        u = sref.uniforms(SEED, 3, shots, njobs)
        assert np.array_equal(multinomial_counts(p, shots, 0, 0, u=u), want)  # supplied uniforms


def test_multinomial_counts_over_more_than_one_chunk():
    """Above 65536 shots a job is drawn by several workgroups whose partial counts are summed."""
    from adaptaqc_amd.device import multinomial_counts

    p = _job_probs(9, 4, 1)
    for shots in (65536, 65537, 140000):
        got = multinomial_counts(p, shots, 77, 1)
        assert np.array_equal(got, tref.multinomial_counts(p, shots, seed=77, run=1))
        assert (got.sum(axis=1) == shots).all()


def test_multinomial_edge_rule_and_errors():
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.device import multinomial_counts

    p = np.array([[0, 0.25, 0.25, 0.5, 0]])
    for u, k in ((0.0, 1), (0.25, 2), (np.nextafter(1.0, 0.0), 3)):
        got = multinomial_counts(p, 1, 0, 0, u=np.array([[u]]))
        assert got.tolist() == [[int(j == k) for j in range(5)]], (u, got)
    got = multinomial_counts(p, 4096, 9, 0)
    assert got[0, 0] == 0 and got[0, 4] == 0 and got.sum() == 4096
    with pytest.raises(AqcError, match="-1"):  # an all-zero row
        multinomial_counts(np.array([[0.5, 0.5, 0, 0], [0, 0, 0, 0]]), 10, 1)
    for bad in (np.array([[0.5, -0.1]]), np.array([[0.5, np.nan]]), np.ones((1, 17)), np.ones((1, 1))):
        with pytest.raises(AqcError, match="-1"):
            multinomial_counts(bad, 10, 1)
    with pytest.raises(AqcError, match="-1"):
        multinomial_counts(p, 0, 1)
    with pytest.raises(AqcError, match="-1"):
        multinomial_counts(p, 2, 1, u=np.array([[0.5], [1.0]]))


def _bell_rdm():
    bell = np.array([1, 0, 0, 1]) / np.sqrt(2)
    return np.outer(bell, bell.conj())


def test_fit_matches_restatement(brick_rdms):
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.device import tomo_fit

    tables = [tref.tomography(brick_rdms["sv"], shots, 3)[1] for shots in (8192, 64)]
    bell64 = tref.tomography(_bell_rdm()[None], 64, 1)[1]  # hand-made: a Bell pair at 64 shots
    one_outcome = np.tile([64, 0, 0, 0], (1, 9, 1))       # and every setting reading ++
    for t in (bell64, one_outcome):  # their linear inversions are not positive semidefinite
        assert np.linalg.eigvalsh(tref.linear_inversion(t)[0]).min() < -1e-3
    counts = np.concatenate(tables + [bell64, one_outcome])
    got = tomo_fit(counts)
    want = tref.tomo_fit(counts)
    assert got.shape == (14, 4, 4)
    np.testing.assert_allclose(got, want, atol=1e-10, rtol=0)
    for r in got:
        assert np.array_equal(r, r.conj().T)
        assert abs(np.trace(r).real - 1) < 1e-12
        assert np.linalg.eigvalsh(r).min() >= -1e-12
    bad = counts[:2].copy()
    bad[1, 4] = 0
    with pytest.raises(AqcError, match="-1"):  # a setting without counts
        tomo_fit(bad)


def _backend(engine, mode="device"):
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator

    method = "statevector" if engine == "sv" else "matrix_product_state"
    return QiskitSamplingBackend(SamplingSimulator(method=method, seed=11), tomography=mode)


@pytest.mark.parametrize("engine", ["sv", "mps"])
@pytest.mark.parametrize("state", list(tref.STATES))
def test_device_mode_end_to_end(engine, state):
    """Seeded device mode against the restatement chain on the device's own RDMs (the tolerance
    test_gpu_ent.py uses for the measures) and against the exact values (10 / sqrt(shots), which
    test_tomography_host.py confirms for the restatement on these states and this seed)."""
    from adaptaqc_amd.device import EM_METHOD_CODES

    n, ops = tref.STATES[state]
    qc = to_circuit(n, ops)
    for q in range(n):  # the trailing measures of the sampling backend's circuits are ignored
        qc.measure(q, q)
    pairs = tref.all_pairs(n)
    be = _backend(engine)
    kwargs = {"shots": tref.SHOTS, "seed_simulator": tref.SEED}
    rdms = be.simulator._state(qc).pair_rdms(pairs)
    psi = osv.simulate(n, ops)
    exact = np.stack([OE.partial_trace_sv(psi, a, b) for a, b in pairs])
    np.testing.assert_allclose(rdms, exact, atol=1e-11)
    fit_ref, _ = tref.tomography(rdms, tref.SHOTS, tref.SEED, 0)
    for method in EM_METHOD_CODES:
        rho, got = be.pair_tomography(qc, pairs, kwargs, method)
        np.testing.assert_allclose(rho, fit_ref, atol=1e-10, rtol=0)
        want = [OE.measure(method, r) for r in fit_ref]
        print(state, engine, method, np.abs(got - want).max())
        np.testing.assert_allclose(got, want, atol=1e-7, rtol=0)
        truth = np.array([tref.exact_measure(method, r) for r in exact])
        assert np.max(np.abs(got - truth)) < tref.MARGIN
    lb = be.concurrence_lower_bounds(qc, pairs, kwargs)
    np.testing.assert_allclose(lb, tref.concurrence_lower_bounds(rdms, tref.SHOTS, tref.SEED, 0), atol=1e-12, rtol=0)
    c2 = np.array([OE.concurrence(r) ** 2 for r in exact])
    assert (lb <= c2 + tref.MARGIN).all()
    assert be.simulator.runs == 0  # seed_simulator: the run counter is not used
    be.pair_tomography(qc, pairs, {"shots": 64})
    assert be.simulator.runs == 1  # unseeded: it advances once per sweep


def test_public_functions_on_the_sampling_backend():
    from adaptaqc_amd.utils import entanglement_measures as em

    n, ops = tref.STATES["bell_in_3"]
    qc = to_circuit(n, ops)
    be = _backend("sv")
    kwargs = {"shots": tref.SHOTS, "seed_simulator": tref.SEED}
    rho = em.perform_quantum_tomography(qc, 2, 0, be.simulator, None, kwargs)
    assert rho.shape == (4, 4) and np.max(np.abs(rho - _bell_rdm())) < tref.MARGIN
    c = em.calculate_entanglement_measure(em.EM_TOMOGRAPHY_CONCURRENCE, qc, 0, 2, be, None, kwargs)
    assert abs(c - 1) < tref.MARGIN
    lb = em.calculate_entanglement_measure(em.EM_OBSERVABLE_CONCURRENCE_LOWER_BOUND, qc, 0, 2, be, None, kwargs)
    assert lb == em.measure_concurrence_lower_bound(qc, 0, 2, be, None, kwargs)
    # a pure pair: the bound is C^2 = 1 = 8 p - 4 q at p = q = 1 / 4; five standard deviations of
    # 8 f - 4 g for two binomial shares: 5 sqrt(64 p (1 - p) + 16 q (1 - q)) / sqrt(shots)
    five_sigma = 5 * np.sqrt(64 * 3 / 16 + 16 * 3 / 16) / np.sqrt(tref.SHOTS)
    assert abs(lb - 1) < five_sigma
    assert abs(em.measure_concurrence_lower_bound(qc, 2, 0, be, None, kwargs) - 1) < five_sigma
    with pytest.raises(ValueError):
        em.calculate_entanglement_measure("nope", qc, 0, 1, be)


def test_device_mode_against_circuits_mode():
    """One pair of a 3-qubit state: the rho fitted to counts drawn from the RDM and the rho fitted to
    the counts of the nine rotated circuits (independent streams) differ by less than
    10 / sqrt(shots) per entry; so do the two lower bounds (two-copy circuits on 6 qubits)."""
    n, ops = 3, sref.brickwork(3, 3, 8)
    qc = to_circuit(n, ops)
    kwargs = {"shots": tref.SHOTS, "seed_simulator": 3}
    dev, cir = _backend("sv", "device"), _backend("sv", "circuits")
    a, _ = dev.pair_tomography(qc, [(0, 2)], kwargs)
    b, _ = cir.pair_tomography(qc, [(0, 2)], dict(kwargs, seed_simulator=4))
    print("device vs circuits: max entry difference", np.abs(a - b).max(), "margin", tref.MARGIN)
    assert np.max(np.abs(a - b)) < tref.MARGIN
    la = dev.concurrence_lower_bounds(qc, [(2, 0)], kwargs)
    lb = cir.concurrence_lower_bounds(qc, [(2, 0)], dict(kwargs, seed_simulator=4))
    # 8 f - 4 g of binomial shares: standard deviation below sqrt(8^2 + 4^2) * 0.5 / sqrt(shots) each
    assert abs(la[0] - lb[0]) < 5 * np.sqrt(2) * np.sqrt(80) * 0.5 / np.sqrt(tref.SHOTS)


def test_isl_compile_with_sampling_backend():
    """ISL on the shot backend (the reference's two defaults together), on the 3-qubit target and by
    the criterion of test_gpu_sampling.py: exact overlap > 1 - sufficient_cost - 5 / sqrt(shots)."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend
    from adaptaqc_amd.circuit import device_ops
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig
    from adaptaqc_amd.utils.constants import DEFAULT_SUFFICIENT_COST

    shots = 10000
    target_ops = [("ry", (0,), (0.9,)), ("cx", (0, 1), ()), ("rx", (2,), (0.4,)), ("cx", (1, 2), ()), ("rz", (1,), (0.3,))]
    target = to_circuit(3, target_ops)
    comp = AdaptCompiler(target, backend=QiskitSamplingBackend(tomography="device"),
                         adapt_config=AdaptConfig(method="ISL"),
                         execute_kwargs={"shots": shots, "seed_simulator": 7})
    result = comp.compile()
    psi_t = osv.simulate(3, target_ops)
    psi_c = np.zeros(8, dtype=complex)
    psi_c[0] = 1
    for m, q in device_ops(result.circuit):
        psi_c = osv.apply_matrix(psi_c, 3, q, m)
    overlap = abs(np.vdot(psi_t, psi_c)) ** 2
    print("exact overlap", overlap, "layers", len(result.qubit_pair_history))
    assert overlap > 1 - DEFAULT_SUFFICIENT_COST - 5 / np.sqrt(shots)
    history = result.entanglement_measures_history
    assert len(history) == len(result.qubit_pair_history) >= 1
    assert all(isinstance(h, list) and len(h) == len(comp.coupling_map) for h in history)
    assert "ISL" in result.method_history
