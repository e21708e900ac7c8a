"""Shot sampling on MI355X: the device samplers against their numpy restatements (sampling_ref.py),
their distribution against the oracle's |psi|^2, and the sampling backend built on them."""
import numpy as np
import pytest

import sampling_ref as ref
from conftest import FakeCompiler, to_circuit
from oracle import sv as osv

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 3


def _sv_ops(n):
    if n == 1:
        return [("rx", (0,), (0.7,)), ("rz", (0,), (1.1,))]
    return ref.brickwork(n, 4, 100 + n)


def _device_sv(n, ops):
    from adaptaqc_amd.circuit import device_ops
    from adaptaqc_amd.device import DeviceSV

    d = DeviceSV(n)
    d.apply(device_ops(to_circuit(n, ops)))
    return d


def _device_mps(n, ops, cap, max_chi=None):
    from adaptaqc_amd.circuit import device_ops
    from adaptaqc_amd.device import DeviceMPS

    d = DeviceMPS(n, cap, 1e-16, max_chi)
    d.apply(device_ops(to_circuit(n, ops)))
    return d


def test_uniforms_match_philox_restatement():
    from adaptaqc_amd.device import sample_uniforms

    got = sample_uniforms(SEED, 5, 1000, 7)
    want = ref.uniforms(SEED, 5, 1000, 7)
    assert got.shape == (1000, 7)
    assert np.array_equal(got, want)
    assert got.min() >= 0.0 and got.max() < 1.0


@pytest.mark.parametrize("n", [1, 3, 13])
@pytest.mark.parametrize("shots", [1, 100, 4097])
def test_statevector_sampler_matches_inverse_cdf(n, shots):
    """Outcome per shot = smallest k with C_k > u P on the device's own amplitudes; the same
    outcomes with u passed in and with u drawn on the device from (seed, run)."""
    d = _device_sv(n, _sv_ops(n))
    psi = d.get()
    run = 3
    u = ref.uniforms(SEED + n, run, shots, 1)[:, 0]
    want, near = ref.sv_sample(psi, u)
    # the seed was chosen so that the oracle's state shows no shot at a CDF boundary
    assert not ref.sv_sample(osv.simulate(n, _sv_ops(n)), u)[1].any()
    assert near.sum() <= 2
    for got in (d.sample(shots, SEED + n, run, u=u), d.sample(shots, SEED + n, run)):
        assert got.dtype == np.uint64 and got.shape == (shots,)
        got = got.astype(np.int64)
        bad = np.flatnonzero(got != want)
        for j in bad:
            assert near[j] and got[j] in ref.sv_neighbours(psi, want[j]), (j, got[j], want[j])
    np.testing.assert_array_equal(d.get(), psi)  # the state is not modified


def _ghz_ops(n):
    return [("h", (0,), ())] + [("cx", (q, q + 1), ()) for q in range(n - 1)]


MPS_CASES = {
    "n2": dict(n=2, ops=[("h", (0,), ()), ("cx", (0, 1), ()), ("ry", (1,), (0.3,))], cap=4, max_chi=None, shots=4097),
    "n12_truncated_cap64": dict(n=12, ops=ref.brickwork(12, 8, 7), cap=64, max_chi=8, shots=200),
    "ghz70": dict(n=70, ops=_ghz_ops(70), cap=4, max_chi=None, shots=130),
    "n16_cap256": dict(n=16, ops=ref.brickwork(16, 8, 11), cap=256, max_chi=None, shots=100),
}


@pytest.mark.parametrize("case", list(MPS_CASES))
def test_mps_sampler_matches_per_site_rule(case):
    c = MPS_CASES[case]
    n, shots = c["n"], c["shots"]
    d = _device_mps(n, c["ops"], c["cap"], c["max_chi"])
    tensors = d.preprocessed()
    if case == "n12_truncated_cap64":
        assert max(t.shape[2] for t in tensors) == 8
        assert abs(ref.right_environments(tensors)[0][0, 0].real - 1.0) > 1e-6  # truncated: norm != 1
    if case == "n16_cap256":
        assert max(t.shape[2] for t in tensors) > 8
    before = d.overlap_zero()
    run = 2
    u = ref.uniforms(SEED, run, shots, n)
    want, near = ref.mps_sample(tensors, u)
    assert near.sum() <= 2
    keep = ~near
    for got in (d.sample(shots, SEED, run, u=u), d.sample(shots, SEED, run)):
        assert got.dtype == np.uint64 and got.shape == (shots, (n + 63) // 64)
        bits = ref.unpack_bits(got, n)
        np.testing.assert_array_equal(bits[keep], want[keep])
        if n % 64:  # no bits past qubit n - 1
            assert not (got[:, -1] >> np.uint64(n % 64)).any()
        if case == "ghz70":
            s = bits.sum(axis=1)
            assert set(np.unique(s)) <= {0, n} and 0 < (s == n).sum() < shots
    after = d.overlap_zero()
    assert after == before  # 0 ulp: the state is not modified
    for a, b in zip(d.preprocessed(), tensors):
        np.testing.assert_array_equal(a, b)


def test_distribution_chi_square_both_samplers():
    """65536 shots of a 10-qubit brickwork state against the oracle's |psi|^2: Pearson chi-square
    below dof + 6 sqrt(2 dof) (six standard deviations of the chi-square distribution)."""
    from adaptaqc_amd.device import counts_from_samples

    n, shots = 10, 65536
    ops = ref.brickwork(n, 6, 5)
    probs = np.abs(osv.simulate(n, ops)) ** 2
    for d in (_device_sv(n, ops), _device_mps(n, ops, 32)):
        s = d.sample(shots, 12345, 0)
        idx = s.reshape(shots).astype(np.int64)
        stat, dof = ref.chi_square(np.bincount(idx, minlength=2 ** n), probs, shots)
        print(type(d).__name__, "chi2", stat, "dof", dof)
        assert dof > 100
        assert stat < dof + 6 * np.sqrt(2 * dof)
        counts = counts_from_samples(s, n)
        assert sum(counts.values()) == shots
        k = int(np.argmax(probs))
        assert counts[format(k, f"0{n}b")] == int((idx == k).sum())


def test_x_on_qubit_0_gives_001_on_both():
    from adaptaqc_amd.device import counts_from_samples

    ops = [("x", (0,), ())]
    for d in (_device_sv(3, ops), _device_mps(3, ops, 4)):
        assert counts_from_samples(d.sample(1000, 1), 3) == {"001": 1000}


def test_sv_state_unchanged_after_sampling():
    d = _device_sv(13, _sv_ops(13))
    before = d.amp0()
    d.sample(500, 9)
    assert d.amp0() == before


def test_argument_errors():
    from adaptaqc_amd._lib import AqcError

    sv = _device_sv(3, _sv_ops(3))
    mps = _device_mps(3, _sv_ops(3), 4)
    for d, shape in ((sv, (4,)), (mps, (4, 3))):
        with pytest.raises(AqcError, match="-1"):
            d.sample(0, 1)
        for badv in (1.0, -1e-9, np.nan):
            u = np.full(shape, 0.5)
            u.flat[-1] = badv
            with pytest.raises(AqcError, match="-1"):
                d.sample(4, 1, u=u)


def test_pending_capacity_flag_is_a_state_error():
    """Work queued without a flag read (apply_batch(wait=False)) that overflows the bond capacity:
    the sampler reports it as aqc_mps_overlap_zero does (AQC_ERR_STATE)."""
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.circuit import device_ops
    from adaptaqc_amd.device import apply_batch

    d = _device_mps(6, [], 2)
    apply_batch([d], [device_ops(to_circuit(6, ref.brickwork(6, 6, 1)))], sort=True, wait=False)
    with pytest.raises(AqcError, match="capacity"):
        d.sample(10, 1)


def _cost_table_circuits():
    from adaptaqc_amd.circuit import QuantumCircuit

    zero = QuantumCircuit(4)
    neel = QuantumCircuit(4)
    neel.x([0, 2])
    ghz = QuantumCircuit(4)
    ghz.h(0)
    for i in range(3):
        ghz.cx(0, i + 1)
    had = QuantumCircuit(4)
    had.h([0, 1, 2, 3])
    return [zero, neel, ghz, had], [0, 0, 1, 0.5, 0.5, 0.5, 15 / 16, 0.5]


@pytest.mark.parametrize("method", ["statevector", "matrix_product_state"])
def test_sampling_backend_cost_table(method):
    """The reference's cost-table states (test_approximate_compiler.py:114-150) through
    QiskitSamplingBackend: each cost is a binomial mean (standard deviation <= 0.5 / sqrt(shots)),
    so 5 / sqrt(shots) is ten standard deviations."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator

    shots = 8192
    circuits, exact = _cost_table_circuits()
    be = QiskitSamplingBackend(SamplingSimulator(method=method, seed=11))
    got = []
    for c in circuits:
        comp = FakeCompiler(c)
        comp.execute_kwargs = {"shots": shots}
        comp.total_num_qubits = 4
        comp.general_initial_state = False
        got += [be.evaluate_global_cost(comp), be.evaluate_local_cost(comp)]
        assert len(c.data) == len(comp.full_circuit.data)  # the local cost removed its measures
    assert np.max(np.abs(np.array(got) - exact)) < 5 / np.sqrt(shots)
    z = be.measure_qubit_expectation_values(comp)  # |++++>
    assert len(z) == 4 and np.max(np.abs(z)) < 5 / np.sqrt(shots)


def test_same_seed_simulator_gives_identical_counts():
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator

    qc = to_circuit(5, ref.brickwork(5, 4, 2))
    sim = SamplingSimulator()
    a = sim.run(qc, shots=2000, seed_simulator=7).result().get_counts()
    b = sim.run(qc, shots=2000, seed_simulator=7).result().get_counts()
    c = sim.run(qc, shots=2000).result().get_counts()
    e = sim.run(qc, shots=2000).result().get_counts()
    assert a == b and sum(a.values()) == 2000
    assert c != e  # unseeded runs advance the run counter


def test_compile_with_sampling_backend():
    """The reference's own criterion (test_adapt_compiler.py:60-68): the compiled circuit's exact
    overlap with the target exceeds 1 - sufficient_cost - 5 / sqrt(shots)."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig
    from adaptaqc_amd.utils.constants import DEFAULT_SUFFICIENT_COST

    shots = 10000
    target_ops = [("ry", (0,), (0.9,)), ("cx", (0, 1), ()), ("rx", (2,), (0.4,)), ("cx", (1, 2), ()), ("rz", (1,), (0.3,))]
    target = to_circuit(3, target_ops)
    comp = AdaptCompiler(target, backend=QiskitSamplingBackend(), adapt_config=AdaptConfig(method="expectation"),
                         execute_kwargs={"shots": shots, "seed_simulator": 7})
    result = comp.compile()
    from adaptaqc_amd.circuit import device_ops

    psi_t = osv.simulate(3, target_ops)
    psi_c = np.zeros(8, dtype=complex)
    psi_c[0] = 1
    for m, q in device_ops(result.circuit):
        psi_c = osv.apply_matrix(psi_c, 3, q, m)
    overlap = abs(np.vdot(psi_t, psi_c)) ** 2
    print("exact overlap", overlap)
    assert overlap > 1 - DEFAULT_SUFFICIENT_COST - 5 / np.sqrt(shots)
    with pytest.raises(NotImplementedError):
        AdaptCompiler(target, backend=QiskitSamplingBackend(), adapt_config=AdaptConfig(method="ISL"))
