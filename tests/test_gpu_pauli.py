"""Pauli-string expectation values on MI355X: the statevector and MPS kernels against numpy
restatements applied to the device's own state (only the contraction is compared: 1e-11, the bound
of z_all_batch against a contraction of the same tensors), against the existing device paths
(z_all, pair_rdms), and the host API built on them."""
import numpy as np
import pytest

import sampling_ref as ref
from conftest import to_circuit
from oracle import sv as osv
from sv_readers_ref import sv_pauli_ref

pytestmark = pytest.mark.gpu

ATOL = 1e-11
PAULI = {
    "I": np.eye(2, dtype=complex),
    "X": np.array([[0, 1], [1, 0]], dtype=complex),
    "Y": np.array([[0, -1j], [1j, 0]], dtype=complex),
    "Z": np.array([[1, 0], [0, -1]], dtype=complex),
}


# ---- numpy restatements (the statevector one is sv_readers_ref.sv_pauli_ref) ---------------------
def mps_pauli_ref(tensors, label):
    """Transfer-matrix contraction over the whole chain: E <- sum_{s,t} P[s][t] A_s^H E A_t."""
    E = np.ones((1, 1), dtype=complex)
    for q, A in enumerate(tensors):
        P = PAULI[label[len(label) - 1 - q]]
        En = np.zeros((A.shape[2], A.shape[2]), dtype=complex)
        for s in range(2):
            for t in range(2):
                if P[s, t] != 0:
                    En += P[s, t] * (A[s].conj().T @ E @ A[t])
        E = En
    return float(E[0, 0].real)


def label_of(n, ops):
    chars = ["I"] * n
    for q, p in ops.items():
        chars[n - 1 - q] = p
    return "".join(chars)


def random_labels(n, count, seed):
    rng = np.random.default_rng(seed)
    out = ["I" * n, "".join(rng.choice(list("XYZ"), n))]  # all-identity and full-weight
    while len(out) < count:
        out.append("".join(rng.choice(list("IXYZ"), n)))
    return out


# ---- states ------------------------------------------------------------------------------------
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


def _ghz_ops(n):
    return [("h", (0,), ())] + [("cx", (q, q + 1), ()) for q in range(n - 1)]


MPS_CASES = {
    "n2": dict(n=2, ops=[("h", (0,), ()), ("cx", (0, 1), ()), ("ry", (1,), (0.3,))], cap=4, max_chi=None),
    "n12_truncated_cap64": dict(n=12, ops=ref.brickwork(12, 8, 7), cap=64, max_chi=8),
    "ghz70": dict(n=70, ops=_ghz_ops(70), cap=4, max_chi=None),
    "n16_cap256": dict(n=16, ops=ref.brickwork(16, 8, 11), cap=256, max_chi=None),
}
_STATES = {}


def mps_case(case):
    """(device state, its preprocessed tensors), built once per case; tests do not modify them."""
    if case not in _STATES:
        c = MPS_CASES[case]
        d = _device_mps(c["n"], c["ops"], c["cap"], c["max_chi"])
        _STATES[case] = (d, d.preprocessed())
    return _STATES[case]


def mps_labels(case):
    n = MPS_CASES[case]["n"]
    if n == 2:
        return [a + b for a in "IXYZ" for b in "IXYZ"]
    mid = n // 2
    out = ["I" * n]
    for p in "XYZ":  # support 1: first site, last site, interior
        out += [label_of(n, {0: p}), label_of(n, {n - 1: p}), label_of(n, {mid: p})]
    # support 2 at both ends and inside; longer supports from site 0, to site n - 1, interior
    out += [label_of(n, {0: "X", 1: "Y"}), label_of(n, {n - 2: "Z", n - 1: "X"}), label_of(n, {mid: "Y", mid + 1: "Y"})]
    out += [label_of(n, {0: "Z", mid: "X"}), label_of(n, {mid: "Y", n - 1: "Z"}), label_of(n, {1: "X", 3: "Z", n - 2: "Y"})]
    out += [label_of(n, {0: "Z", n - 1: "Z"})]
    out += random_labels(n, 4, 1000 + n)[1:]  # full weight (support n) and three random strings
    return out


# ---- statevector -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 13])
def test_statevector_terms_match_dense_application(n):
    d = _device_sv(n, _sv_ops(n))
    psi = d.get()
    labels = [label_of(n, {q: p}) for q in range(n) for p in "XYZ"]
    labels += random_labels(n, 40, 7 + n)
    labels.append(label_of(n, {n - 1: "Y"}))  # the only non-identity qubit is n - 1
    got = d.pauli_expect(labels)
    want = np.array([sv_pauli_ref(psi, l) for l in labels])
    print("sv n", n, "max abs err", np.max(np.abs(got - want)))
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
    assert abs(got[labels.index("I" * n)] - np.vdot(psi, psi).real) < ATOL
    again = d.pauli_expect(labels)
    assert np.array_equal(got, again)  # bit-identical: fixed summation order, no atomics
    np.testing.assert_array_equal(d.get(), psi)  # the state is not modified
    # code arrays and masks are the same call
    from adaptaqc_amd import paulis

    codes = paulis.terms_to_codes(labels, n)
    assert np.array_equal(d.pauli_expect(codes), got)
    assert np.array_equal(d.pauli_expect_masks(*paulis.codes_to_masks(codes)), got)


# ---- MPS ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(MPS_CASES))
def test_mps_terms_match_transfer_matrix_contraction(case):
    d, tensors = mps_case(case)
    n = d.n
    labels = mps_labels(case)
    if case == "n16_cap256":
        assert max(t.shape[2] for t in tensors) > 8 and len(labels) >= 12
    before = d.overlap_zero()
    got = d.pauli_expect(labels)
    want = np.array([mps_pauli_ref(tensors, l) for l in labels])
    print(case, "max abs err", np.max(np.abs(got - want)))
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
    if case == "n12_truncated_cap64":
        assert max(t.shape[2] for t in tensors) == 8
        norm = ref.right_environments(tensors)[0][0, 0].real
        assert abs(norm - 1.0) > 1e-6  # truncated: norm != 1
        assert abs(got[labels.index("I" * n)] - norm) < ATOL  # <psi|P|psi> is not divided by <psi|psi>
    if case == "ghz70":
        exact = {"X" * 70: 1.0, label_of(70, {0: "Z", 69: "Z"}): 1.0, label_of(70, {0: "Z"}): 0.0,
                 "X" * 69 + "Y": 0.0, "X" * 68 + "YY": -1.0}
        vals = d.pauli_expect(list(exact))
        np.testing.assert_allclose(vals, list(exact.values()), rtol=0, atol=ATOL)
        np.testing.assert_allclose(vals, [mps_pauli_ref(tensors, l) for l in exact], rtol=0, atol=ATOL)
    # the state is not modified
    assert d.overlap_zero() == before  # 0 ulp
    for a, b in zip(d.preprocessed(), tensors):
        np.testing.assert_array_equal(a, b)


def test_single_z_terms_equal_z_all():
    for case in ("n12_truncated_cap64", "n16_cap256"):
        d, _ = mps_case(case)
        n = d.n
        got = d.pauli_expect([label_of(n, {q: "Z"}) for q in range(n)])
        np.testing.assert_allclose(got, d.z_all(), rtol=0, atol=ATOL)


def test_two_site_terms_equal_pair_rdm_traces():
    """All nine P_a (x) P_b on three pairs against Tr(rho_ab P_hi (x) P_lo): the RDM's row index is
    2 bit(max) + bit(min) whichever order the pair is given in."""
    d, _ = mps_case("n16_cap256")
    n = d.n
    pairs = [(0, 1), (5, 11), (15, 3)]
    rdms = d.pair_rdms(pairs)
    swapped = d.pair_rdms([(b, a) for a, b in pairs])
    np.testing.assert_allclose(swapped, rdms, rtol=0, atol=ATOL)
    labels, want = [], []
    for (a, b), rho in zip(pairs, rdms):
        for pa in "XYZ":
            for pb in "XYZ":
                labels.append(label_of(n, {a: pa, b: pb}))
                hi, lo = (pb, pa) if b > a else (pa, pb)
                want.append(np.trace(rho @ np.kron(PAULI[hi], PAULI[lo])).real)
    got = d.pauli_expect(labels)
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)


def test_batch_equals_single_calls_and_mixed_capacities_raise():
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.device import pauli_expect_batch

    n = 9
    states = [_device_mps(n, ref.brickwork(n, 5, 20 + s), 16) for s in range(3)]
    labels = mps_labels_for(n)
    got = pauli_expect_batch(states, labels)
    assert got.shape == (3, len(labels))
    for s, d in enumerate(states):
        assert np.array_equal(got[s], d.pauli_expect(labels))
        np.testing.assert_allclose(got[s], [mps_pauli_ref(d.preprocessed(), l) for l in labels], rtol=0, atol=ATOL)
    other = _device_mps(n, ref.brickwork(n, 2, 3), 8)
    with pytest.raises(AqcError, match="-1"):
        pauli_expect_batch(states[:2] + [other], labels)
    assert pauli_expect_batch([], labels).shape == (0, 0)


def mps_labels_for(n):
    mid = n // 2
    return ["I" * n, label_of(n, {0: "X"}), label_of(n, {n - 1: "Y"}), label_of(n, {mid: "Z", mid + 1: "X"}),
            label_of(n, {0: "Y", n - 1: "Y"})] + random_labels(n, 5, 77)[1:]


def test_mps_expectation_x_and_y():
    from adaptaqc_amd.mps_operations import mps_expectation

    d, tensors = mps_case("n12_truncated_cap64")
    n = d.n
    for op in "XYI":
        for q in (0, 5, n - 1):
            want = mps_pauli_ref(tensors, label_of(n, {q: op}))
            assert abs(mps_expectation(d, op, q) - want) < ATOL
    assert abs(mps_expectation(d, "Z", 5) - mps_pauli_ref(tensors, label_of(n, {5: "Z"}))) < ATOL
    with pytest.raises(ValueError):
        mps_expectation(d, "W", 0)


def test_argument_errors():
    from adaptaqc_amd import _lib
    from adaptaqc_amd._lib import AqcError

    sv = _device_sv(3, _sv_ops(3))
    mps, _ = mps_case("n2")
    with pytest.raises(ValueError):
        mps.pauli_expect(np.array([[0, 4]], dtype=np.uint8))
    codes = np.array([[0, 4]], dtype=np.uint8)  # past the Python check: the library's own
    out = np.zeros(1)
    assert _lib.lib().aqc_mps_pauli_expect(mps.h, _lib.ptr(codes), 1, _lib.ptr(out)) == -1
    with pytest.raises(AqcError, match="-1"):
        sv.pauli_expect_masks([1 << 3], [0])
    with pytest.raises(AqcError, match="-1"):
        sv.pauli_expect_masks([0], [1 << 40])
    with pytest.raises(ValueError):
        sv.pauli_expect(["XX"])
    assert sv.pauli_expect([]).shape == (0,)
    assert mps.pauli_expect([]).shape == (0,)


def test_pending_capacity_flag_is_a_state_error():
    """Work queued without a flag read (apply_batch(wait=False)) that overflows the bond capacity is
    reported as aqc_mps_overlap_zero reports it (AQC_ERR_STATE)."""
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.circuit import device_ops
    from adaptaqc_amd.device import apply_batch

    d = _device_mps(6, [], 2)
    apply_batch([d], [device_ops(to_circuit(6, ref.brickwork(6, 6, 1)))], sort=True, wait=False)
    with pytest.raises(AqcError, match="capacity"):
        d.pauli_expect(["IIIIIZ"])


# ---- host API ----------------------------------------------------------------------------------
HOST_N, HOST_OPS = 6, ref.brickwork(6, 4, 31)


def _host_exact():
    from adaptaqc_amd.utils.hamiltonians import heisenberg_hamiltonian

    ham = heisenberg_hamiltonian(HOST_N, 1, 1, 1, 0.5, 0.5, 0.5)
    psi = osv.simulate(HOST_N, HOST_OPS)
    terms = {l: sv_pauli_ref(psi, l) for l in ham}
    return ham, terms, sum(ham[l] * terms[l] for l in ham)


def test_heisenberg_energy_on_sv_and_mps_backends():
    from adaptaqc_amd.backends.aer_mps_backend import AerMPSBackend
    from adaptaqc_amd.backends.aer_sv_backend import AerSVBackend
    from adaptaqc_amd.utils.circuit_operations import expectation_value_of_pauli_operator

    ham, _, energy = _host_exact()
    assert len(ham) == 5 * 3 + 6 * 3
    qc = to_circuit(HOST_N, HOST_OPS)
    before = len(qc.data)
    for backend in (AerSVBackend(), AerMPSBackend()):
        got = expectation_value_of_pauli_operator(qc, ham, backend)
        print(type(backend).__name__, got, energy)
        assert abs(got - energy) < 1e-10
        shifted = dict(ham)
        shifted["I" * HOST_N] = 0.75  # the identity term contributes its coefficient
        assert abs(expectation_value_of_pauli_operator(qc, shifted, backend) - (energy + 0.75)) < 1e-10
    assert len(qc.data) == before


@pytest.mark.parametrize("method", ["statevector", "matrix_product_state"])
def test_heisenberg_energy_on_sampling_backend(method):
    """Each term is a mean of +-1 outcomes (variance <= 1): 5 / sqrt(shots) is five standard
    deviations at least."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.utils.circuit_operations import (expectation_value_of_pauli_operator,
                                                       expectation_values_of_pauli_terms)

    shots = 8192
    ham, terms, _ = _host_exact()
    qc = to_circuit(HOST_N, HOST_OPS)
    before = len(qc.data)
    be = QiskitSamplingBackend(SamplingSimulator(method=method, seed=11))
    kw = {"shots": shots, "seed_simulator": 5}
    labels = list(ham)
    est = expectation_values_of_pauli_terms(qc, labels, be, execute_kwargs=kw)
    err = np.abs(est - np.array([terms[l] for l in labels]))
    print(method, "max term error", err.max(), "bound", 5 / np.sqrt(shots))
    assert err.max() < 5 / np.sqrt(shots)
    e1 = expectation_value_of_pauli_operator(qc, ham, be, execute_kwargs=kw)
    e2 = expectation_value_of_pauli_operator(qc, ham, be, execute_kwargs=kw)
    assert e1 == e2  # the same seed_simulator: identical counts
    assert e1 == sum(ham[l] * float(v) for l, v in zip(labels, est))
    assert len(qc.data) == before and getattr(qc, "num_clbits", 0) == 0
