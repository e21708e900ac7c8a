"""Host side of shot sampling (no GPU): the Philox restatement, counts formatting, the sampling
backend's cost arithmetic on a stub simulator, compiler defaults, circuit measures and pickling."""
import pickle

import numpy as np
import pytest

import sampling_ref as ref
from conftest import FakeCompiler


def test_philox_known_answers():
    vectors = [
        ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
         "d16cfe09 94fdcceb 5001e420 24126ea1"),
    ]
    for ctr, key, want in vectors:
        assert " ".join(f"{int(x):08x}" for x in ref.philox4x32_10(ctr, key)) == want


def test_uniform_formula_and_counter_layout():
    u = ref.uniforms(2 ** 40 + 3, 5, 4, 3)
    assert u.shape == (4, 3) and (u >= 0).all() and (u < 1).all()
    x = ref.philox4x32_10((2, 0, 1, 5), (3, 2 ** 8))  # shot 2, site 1, run 5; seed 2^40 + 3
    want = ((int(x[0]) >> 5) * 2 ** 26 + (int(x[1]) >> 6)) * 2.0 ** -53
    assert u[2, 1] == want
    assert len(np.unique(ref.uniforms(1, 0, 64, 8))) == 512
    assert not np.array_equal(ref.uniforms(1, 0, 8, 2), ref.uniforms(1, 1, 8, 2))


def test_inverse_cdf_restatement():
    psi = np.sqrt(np.array([0.0, 0.25, 0.0, 0.5, 0.25, 0.0, 0.0, 0.0]))
    k, near = ref.sv_sample(psi, np.array([0.01, 0.2, 0.26, 0.74, 0.76, 0.999999]))
    assert list(k) == [1, 1, 3, 3, 4, 4] and not near.any()
    assert ref.sv_sample(psi, np.array([0.25 + 1e-14]))[1].all()
    assert ref.sv_neighbours(psi, 3) == (1, 4)


def test_mps_restatement_on_a_bell_pair():
    s = np.sqrt(0.5)
    a0 = np.zeros((2, 1, 2), dtype=complex)
    a0[0, 0, 0] = a0[1, 0, 1] = s
    a1 = np.zeros((2, 2, 1), dtype=complex)
    a1[0, 0, 0] = a1[1, 1, 0] = 1
    bits, near = ref.mps_sample([a0, a1], np.array([[0.2, 0.9], [0.7, 0.1], [0.5 + 1e-12, 0.3]]))
    assert bits.tolist() == [[0, 0], [1, 1], [1, 1]]
    assert near.tolist() == [False, False, True]


def test_counts_from_samples_bit_order():
    from adaptaqc_amd.device import counts_from_samples

    assert counts_from_samples(np.array([1], dtype=np.uint64), 3) == {"001": 1}
    assert counts_from_samples(np.array([4, 1, 4], dtype=np.uint64), 3) == {"100": 2, "001": 1}
    # 70 qubits in two words: qubits 0, 63 (word 0) and 64, 69 (word 1)
    w = np.array([[1 | (1 << 63), 1 | (1 << 5)], [0, 0], [1 | (1 << 63), 1 | (1 << 5)]], dtype=np.uint64)
    key = "".join("1" if q in (0, 63, 64, 69) else "0" for q in range(69, -1, -1))
    assert counts_from_samples(w, 70) == {key: 2, "0" * 70: 1}
    # clbits: qubit 69 -> clbit 0, qubit 1 -> clbit 2; clbit 1 is never written and reads 0
    assert counts_from_samples(w, 70, {69: 0, 1: 2}) == {"001": 2, "000": 1}
    assert counts_from_samples(np.array([2, 3], dtype=np.uint64), 2, {1: 0}) == {"1": 2}


class StubSimulator:
    """The ``run`` contract of SamplingSimulator with fixed counts; records its calls."""

    def __init__(self, counts):
        self.counts = counts
        self.calls = []

    def run(self, circuit, **kwargs):
        from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingJob, SamplingResult

        measures = [(i.qubits[0], i.clbits[0]) for i in circuit.data if i.operation.name == "measure"]
        self.calls.append((measures, kwargs))
        c = self.counts(measures) if callable(self.counts) else self.counts
        return SamplingJob(SamplingResult(c))


def _fake(n, general=False, soften=False, shots=100):
    from adaptaqc_amd.circuit import QuantumCircuit

    comp = FakeCompiler(QuantumCircuit(2 * n if general else n), soften=soften)
    comp.total_num_qubits = n
    comp.general_initial_state = general
    comp.execute_kwargs = {"shots": shots}
    return comp


def test_backend_global_cost_from_counts():
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend

    be = QiskitSamplingBackend(StubSimulator({"000": 60, "001": 30, "110": 10}))
    assert be.evaluate_global_cost(_fake(3)) == pytest.approx(0.4)
    assert be.simulator.calls[-1][1] == {"shots": 100}
    # no shot read all zeros: the key is missing and the cost is 1
    assert QiskitSamplingBackend(StubSimulator({"01": 7, "11": 3})).evaluate_global_cost(_fake(2)) == 1
    # general initial state: the register (and the all-zero key) doubles
    be = QiskitSamplingBackend(StubSimulator({"0000": 25, "0100": 75}))
    assert be.evaluate_global_cost(_fake(2, general=True)) == pytest.approx(0.75)
    assert QiskitSamplingBackend(StubSimulator({"00": 25, "01": 75})).evaluate_global_cost(_fake(2, general=True)) == 1
    with pytest.raises(NotImplementedError):
        be.evaluate_global_cost(_fake(2, soften=True))


def test_backend_local_cost_measures_each_qubit_and_cleans_up():
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend

    zero_share = {0: 1.0, 1: 0.5, 2: 0.0}

    def counts(measures):
        (q, c), = measures
        assert c == 0
        z = int(100 * zero_share[q])
        return {k: v for k, v in (("0", z), ("1", 100 - z)) if v}

    be = QiskitSamplingBackend(StubSimulator(counts))
    comp = _fake(3)
    comp.full_circuit.h(0)
    assert be.evaluate_local_cost(comp) == pytest.approx(0.5)
    assert [m for m, _ in be.simulator.calls] == [[(0, 0)], [(1, 0)], [(2, 0)]]
    assert len(comp.full_circuit.data) == 1
    # general initial state: qubit i into clbit 0, its partner i + n into clbit 1, key "00"
    be = QiskitSamplingBackend(StubSimulator(lambda m: {"00": 20, "10": 80} if m[0][0] == 0 else {"00": 100}))
    comp = _fake(2, general=True)
    assert be.evaluate_local_cost(comp) == pytest.approx(0.4)
    assert [m for m, _ in be.simulator.calls] == [[(0, 0), (2, 1)], [(1, 0), (3, 1)]]
    assert len(comp.full_circuit.data) == 0


def test_backend_expectation_values_from_counts():
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend

    # bit 0 is the rightmost character: qubit 0 always 1, qubit 1 half, qubit 2 always 0
    be = QiskitSamplingBackend(StubSimulator({"001": 50, "011": 50}))
    assert be.measure_qubit_expectation_values(_fake(3)) == [-1.0, 0.0, 1.0]


def test_default_backends_and_shots():
    from adaptaqc_amd.backends import AerSVBackend
    from adaptaqc_amd.backends.python_default_backends import QASM_SIM
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.circuit import QuantumCircuit
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig

    assert isinstance(QASM_SIM, QiskitSamplingBackend) and isinstance(QASM_SIM.simulator, SamplingSimulator)
    qc = QuantumCircuit(3)
    qc.h(0)
    qc.cx(0, 1)
    cfg = AdaptConfig(method="expectation")
    sampling = AdaptCompiler(qc, backend=QiskitSamplingBackend(StubSimulator({})), adapt_config=cfg)
    assert sampling.execute_kwargs["shots"] == 8192
    assert AdaptCompiler(qc, backend=AerSVBackend(), adapt_config=cfg).execute_kwargs["shots"] == 1
    assert AdaptCompiler(qc, backend=QiskitSamplingBackend(StubSimulator({})), adapt_config=cfg,
                         execute_kwargs={"shots": 77}).execute_kwargs["shots"] == 77
    # the global cost reads every qubit: trailing measures q -> q, counted on the right-hand side
    tail = sampling.full_circuit.data[-3:]
    assert [(i.operation.name, i.qubits, i.clbits) for i in tail] == [("measure", (q,), (q,)) for q in range(3)]
    assert sampling.rhs_gate_count == 3 and sampling.full_circuit.num_clbits == 3
    assert sampling.variational_circuit_range() == (2, 2)
    local = AdaptCompiler(qc, backend=QiskitSamplingBackend(StubSimulator({})), adapt_config=cfg, optimise_local_cost=True)
    assert local.rhs_gate_count == 0 and "measure" not in local.full_circuit.count_ops()
    sv = AdaptCompiler(qc, backend=AerSVBackend(), adapt_config=cfg)
    assert "measure" not in sv.full_circuit.count_ops()
    with pytest.raises(NotImplementedError):
        AdaptCompiler(qc, backend=QiskitSamplingBackend(StubSimulator({})), adapt_config=AdaptConfig(method="ISL"))
    with pytest.raises(ValueError):
        AdaptCompiler(qc, backend=QiskitSamplingBackend(StubSimulator({})),
                      adapt_config=AdaptConfig(method="general_gradient"))


def test_circuit_measure_and_num_clbits():
    from adaptaqc_amd.circuit import QuantumCircuit, device_ops, qasm2_dumps

    qc = QuantumCircuit(3)
    assert qc.num_clbits == 0
    qc.x(0)
    qc.measure(0, 0)
    assert qc.num_clbits == 1
    qc.measure(2, 4)
    assert qc.num_clbits == 5
    ins = qc.data[-1]
    assert (ins.operation.name, ins.qubits, ins.clbits) == ("measure", (2,), (4,))
    assert len(device_ops(qc)) == 1  # measures are not device ops
    cp = qc.copy()
    assert cp.num_clbits == 5 and cp.data[-1].clbits == (4,)
    assert "creg c[5];" in qasm2_dumps(qc) and "measure q[2] -> c[4];" in qasm2_dumps(qc)
    with pytest.raises(IndexError):
        qc.measure(3, 0)
    del qc.data[-1]
    assert len(qc.data) == 2


def test_measures_must_be_terminal():
    from adaptaqc_amd.backends.qiskit_sampling_backend import terminal_measurements
    from adaptaqc_amd.circuit import QuantumCircuit

    qc = QuantumCircuit(2)
    qc.h(0)
    assert terminal_measurements(qc) is None
    qc.measure(0, 1)
    qc.x(1)  # another qubit: fine
    assert terminal_measurements(qc) == {0: 1}
    qc.cx(1, 0)
    with pytest.raises(NotImplementedError):
        terminal_measurements(qc)


def test_simulator_and_backend_pickle_without_device_state():
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator

    sim = SamplingSimulator(method="matrix_product_state", seed=5, max_chi=16)
    sim._last = (3, "statevector", b"", object())  # stands for a device state: never pickled
    sim.runs = 4
    be = pickle.loads(pickle.dumps(QiskitSamplingBackend(sim)))
    assert be.simulator._last is None
    assert (be.simulator.seed, be.simulator.runs) == (5, 4)
    assert be.simulator.options.method == "matrix_product_state"
    assert be.simulator.options.matrix_product_state_max_bond_dimension == 16
    assert SamplingSimulator().seed != SamplingSimulator().seed
    auto = SamplingSimulator()
    assert (auto._method(26), auto._method(27)) == ("statevector", "matrix_product_state")
    assert be.simulator._method(3) == "matrix_product_state"
    with pytest.raises(ValueError):
        SamplingSimulator(method="density_matrix")
