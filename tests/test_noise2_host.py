"""Host side of correlated two-qubit errors: QuantumError.two_qubit, depolarizing_error(p, 2), two-letter
pauli_error labels, NoiseModel.channels, the Kraus groups of trajectory_program and the MPS refusals.
No GPU needed."""
import numpy as np
import pytest

import trajectory2_ref as t2ref
from adaptaqc_amd import _lib, noise
from adaptaqc_amd.circuit import QuantumCircuit

X = np.array([[0, 1], [1, 0]], dtype=complex)
Y = np.array([[0, -1j], [1j, 0]], dtype=complex)


def _channel(err, rho):
    return sum(k @ rho @ k.conj().T for k in err.kraus)


def _random_rho(dim, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim))
    rho = a @ a.conj().T
    return rho / np.trace(rho)


def test_two_qubit_validation():
    ks = t2ref.collective_decay(0.3)
    err = noise.QuantumError.two_qubit(ks)
    assert err.num_qubits == 2 and err.pair is None and len(err.kraus) == 2
    assert all(k.shape == (4, 4) and k.dtype == complex for k in err.kraus)
    assert not err.is_identity()
    assert abs(err.no_jump_weight() - (3 + 0.7) / 4) < 1e-15  # Tr(K0^dag K0) / 4
    assert noise.QuantumError.two_qubit([np.eye(4)]).is_identity()
    assert noise.QuantumError.two_qubit([0.6 * np.eye(4), 0.8j * np.eye(4)]).is_identity()
    assert len(noise.QuantumError.two_qubit(t2ref.random_channel()).kraus) == 3
    with pytest.raises(ValueError):
        noise.QuantumError.two_qubit([ks[0]])  # incomplete
    with pytest.raises(ValueError):
        noise.QuantumError.two_qubit([0.9 * np.eye(4)])
    with pytest.raises(ValueError):
        noise.QuantumError.two_qubit([np.eye(4) / np.sqrt(17)] * 17)
    with pytest.raises(ValueError):
        noise.QuantumError.two_qubit([])
    with pytest.raises(ValueError):
        noise.QuantumError.two_qubit([np.eye(2)])
    with pytest.raises(ValueError):
        noise.QuantumError.two_qubit([np.eye(4), np.zeros((2, 2))])
    for bad in (np.nan, np.inf):
        k = np.eye(4, dtype=complex)
        k[1, 2] = bad
        with pytest.raises(ValueError):
            noise.QuantumError.two_qubit([k])
    with pytest.raises(NotImplementedError):
        noise.QuantumError([np.eye(4)])  # the constructor keeps refusing 4x4 matrices
    one = noise.amplitude_damping_error(0.1)
    for call in (lambda: err.expand(one), lambda: err.tensor(one), lambda: one.expand(err), lambda: one.tensor(err)):
        with pytest.raises(NotImplementedError):
            call()


def test_two_qubit_depolarizing_map():
    rho = _random_rho(4, 3)
    for p in (0.05, 0.5, 1.0, 16 / 15):
        err = noise.depolarizing_error(p, 2)
        assert err.num_qubits == 2 and len(err.kraus) == 16
        np.testing.assert_allclose(_channel(err, rho), (1 - p) * rho + p * np.eye(4) / 4, atol=1e-14, rtol=0)
        # the identity comes first: operator 0 is the no-jump operator, of weight 1 - 15 p / 16
        k0 = err.kraus[0]
        assert np.max(np.abs(k0 - k0[0, 0] * np.eye(4))) == 0
        assert abs(abs(k0[0, 0]) ** 2 - (1 - 15 * p / 16)) < 1e-15
        assert abs(err.no_jump_weight() - (1 - 15 * p / 16)) < 1e-15
    zero = noise.depolarizing_error(0.0, 2)
    assert zero.is_identity()
    np.testing.assert_allclose(_channel(zero, rho), rho, atol=1e-15, rtol=0)
    for bad in (-1e-3, 16 / 15 + 1e-9, np.nan):
        with pytest.raises(ValueError):
            noise.depolarizing_error(bad, 2)
    with pytest.raises(ValueError):
        noise.depolarizing_error(0.1, 3)
    # the one-qubit form is what it was, by position and by keyword
    assert len(noise.depolarizing_error(0.1).kraus) == 4 and noise.depolarizing_error(0.1, num_qubits=1).num_qubits == 1


def test_two_letter_pauli_labels():
    """The rightmost letter acts on the gate's first listed qubit: "XY" puts X on the second listed one."""
    err = noise.pauli_error([("XY", 1.0)])
    assert err.num_qubits == 2 and len(err.kraus) == 1
    first = np.array([0.8, 0.6j])          # the first listed qubit: the low bit of the matrix index
    second = np.array([0.6, -0.8])
    psi = np.kron(second, first)
    np.testing.assert_allclose(err.kraus[0] @ psi, np.kron(X @ second, Y @ first), atol=1e-15)
    mix = noise.pauli_error([("II", 0.5), ("ZX", 0.25), ("II", 0.125), ("YI", 0.125)])
    assert len(mix.kraus) == 3  # equal labels merge
    rho = _random_rho(4, 5)
    zx, yi = np.kron(np.diag([1.0, -1.0]), X), np.kron(Y, np.eye(2))
    want = 0.625 * rho + 0.25 * zx @ rho @ zx.conj().T + 0.125 * yi @ rho @ yi.conj().T
    np.testing.assert_allclose(_channel(mix, rho), want, atol=1e-15)
    assert noise.pauli_error([("II", 1.0)]).is_identity()
    with pytest.raises(ValueError):
        noise.pauli_error([("II", 0.5), ("X", 0.5)])  # mixed lengths
    with pytest.raises(ValueError):
        noise.pauli_error([("IQ", 1.0)])
    with pytest.raises(ValueError):
        noise.pauli_error([("XX", 0.5)])
    with pytest.raises(ValueError):
        noise.pauli_error([("XX", 1.5), ("II", -0.5)])
    with pytest.raises(ValueError):
        noise.pauli_error([("XYZ", 1.0)])


def test_channels_of_a_correlated_error():
    nm = noise.NoiseModel()
    dep = noise.depolarizing_error(0.05, 2)
    local = noise.QuantumError.two_qubit(t2ref.collective_decay(0.3))
    one = noise.amplitude_damping_error(0.1)
    nm.add_all_qubit_quantum_error(dep, ["cx", "x"])
    nm.add_all_qubit_quantum_error(one, "h")
    nm.add_quantum_error(local, "cx", [2, 0])
    nm.add_all_qubit_quantum_error(noise.depolarizing_error(0.0, 2), "cz")
    assert nm.channels("cx", (0, 1)) == [((0, 1), dep)]
    assert nm.channels("cx", (1, 0)) == [((1, 0), dep)]  # the gate's listed order
    assert nm.channels("cx", (2, 0)) == [((2, 0), local)] and nm.channels("cx", (0, 2)) == [((0, 2), dep)]
    assert nm.channels("h", (1,)) == [(1, one)]  # one-qubit entries keep their form
    assert nm.channels("cz", (0, 1)) == []  # an identity channel
    with pytest.raises(ValueError):
        nm.channels("x", (0,))  # a two-qubit error on a one-qubit instruction
    with pytest.raises(NotImplementedError):
        nm.add_all_qubit_quantum_error(dep, "cx")  # two errors on one instruction


def test_trajectory_program_groups():
    one = noise.amplitude_damping_error(0.1)
    dep = noise.depolarizing_error(0.05, 2)
    decay = noise.QuantumError.two_qubit(t2ref.collective_decay(0.3))
    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(one, "h")
    nm.add_all_qubit_quantum_error(dep, "cx")
    nm.add_quantum_error(decay, "cx", [0, 1])
    nm.add_all_qubit_quantum_error(noise.depolarizing_error(0.0, 2), "cz")  # identity: no rows
    qc = QuantumCircuit(3)
    qc.h(1)
    qc.cx(2, 0)
    qc.cz(0, 1)
    qc.cx(0, 1)
    qc.h(0)
    rows, n_events, measured = noise.trajectory_program(qc, nm)
    assert measured is None and n_events == 4 and len(rows) == 2 + 1 + 16 + 1 + 1 + 2 + 2
    assert noise.count_events(rows) == 4 and noise.has_correlated_rows(rows) and t2ref.n_events(rows) == 4
    got = [(int(r["flags"]) & 0xFF, int(r["nq"]), int(r["q0"]), int(r["q1"])) for r in rows]
    assert got[:3] == [(0, 1, 1, 0), (1, 1, 1, 2), (0, 2, 2, 0)]        # h(1), its error, cx(2, 0)
    assert got[3:19] == [(_lib.OP_KRAUS2, 2, 2, 0)] * 16                  # the depolarizing group on (2, 0)
    assert [int(f) for f in rows["flags"][3:19]] == [3 | (k << 8) | (16 << 16) for k in range(16)]
    assert got[19:21] == [(0, 2, 0, 1), (0, 2, 0, 1)]                     # cz (identity error), cx(0, 1)
    assert [int(f) for f in rows["flags"][21:23]] == [3 | (2 << 16), 3 | (1 << 8) | (2 << 16)]
    assert got[21:23] == [(3, 2, 0, 1)] * 2 and got[23:] == [(0, 1, 0, 0), (1, 1, 0, 2)]
    for k in range(16):
        np.testing.assert_array_equal(rows["m"][3 + k].view(np.complex128).reshape(4, 4), dep.kraus[k])
    np.testing.assert_array_equal(rows["m"][22].view(np.complex128).reshape(4, 4), decay.kraus[1])
    # events in program order: h's row, the group of 16, the group of 2, h's row
    steps = [(len(m), qs) for m, qs, ev in t2ref.events(rows) if ev]
    assert steps == [(2, (1,)), (16, (2, 0)), (2, (0, 1)), (2, (0,))]
    # the restatement's density matrix: the depolarizing map by hand on the pair (2, 0)
    rho = t2ref.density_matrix(3, rows)
    assert abs(np.trace(rho) - 1) < 1e-12 and np.max(np.abs(rho - rho.conj().T)) < 1e-12
    # an identity channel alone: gate rows only
    only = noise.NoiseModel()
    only.add_all_qubit_quantum_error(noise.depolarizing_error(0.0, 2), ["cx", "cz"])
    r0, e0, _ = noise.trajectory_program(qc, only)
    assert e0 == 0 and len(r0) == 5 and not r0["flags"].any()


def test_restatement_density_matrix_is_the_channel():
    """cx(1, 0) then depolarizing on (1, 0), from a product state: (1 - p) rho + p I/4 (x) rest."""
    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(noise.depolarizing_error(0.4, 2), "cx")
    qc = QuantumCircuit(2)
    qc.ry(0.7, 1)
    qc.cx(1, 0)
    rows, n_events, _ = noise.trajectory_program(qc, nm)
    assert n_events == 1
    clean = t2ref.density_matrix(2, noise.trajectory_program(qc, None)[0])
    np.testing.assert_allclose(t2ref.density_matrix(2, rows), 0.6 * clean + 0.4 * np.eye(4) / 4, atol=1e-14)
    # the restatement's trajectories average to it: every branch by hand for u on a grid
    u = np.stack([np.linspace(0.001, 0.999, 400), np.full(400, 0.5)], axis=1)
    _, choices, _ = t2ref.trajectories(2, rows, u)
    assert choices.max() <= 15 and np.count_nonzero(choices[:, 0] == 0) == round(400 * (1 - 15 * 0.4 / 16))


def test_mps_routes_refuse_correlated_errors():
    from adaptaqc_amd import device
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator

    qc, rows, n_events = t2ref.program(3, 1, "a")
    nm = t2ref.model("a")
    match = "correlated.*24 qubits"
    with pytest.raises(NotImplementedError, match=match):
        SamplingSimulator(method="matrix_product_state", mps_trajectories=True).run(qc, shots=10, noise_model=nm)
    be = QiskitSamplingBackend(SamplingSimulator(method="matrix_product_state", mps_trajectories=True),
                               tomography="device", trajectory_tomography=True)
    with pytest.raises(NotImplementedError, match=match):
        be.pair_tomography(qc, [(0, 1)], {"shots": 10, "noise_model": nm})
    wide = QuantumCircuit(26)
    wide.cx(0, 25)
    with pytest.raises(NotImplementedError, match=match):
        SamplingSimulator(mps_trajectories=True).run(wide, shots=10, noise_model=nm)
    effects = noise.readout_effects(3, None)
    with pytest.raises(NotImplementedError, match=match):
        device.mps_trajectory_sample(3, rows, n_events, 4, 1)
    with pytest.raises(NotImplementedError, match=match):
        device.mps_trajectory_pair_tomography(3, rows, n_events, [(0, 1)], effects, 4, 1)
    with pytest.raises(NotImplementedError, match=match):
        device.mps_trajectory_plan(3, rows)


def test_mps_entry_points_answer_err_arg():
    """The C entry points of the MPS engine refuse the new row kind on the host (AQC_ERR_ARG = -1)."""
    import ctypes

    _, rows, _ = t2ref.program(3, 1, "b")
    rows = np.ascontiguousarray(rows)
    lib = _lib.load()  # (does not touch the GPU)
    counts = np.zeros(7, dtype=np.int32)
    assert lib.aqc_mps_traj_plan(3, _lib.ptr(rows), len(rows), _lib.ptr(counts), None, 0) == -1
    assert lib.aqc_mps_traj_tomo_plan(3, _lib.ptr(rows), len(rows), _lib.ptr(counts), None, 0) == -1
    out = np.zeros((4, 1), dtype=np.uint64)
    rc = lib.aqc_mps_traj_sample(3, 8, 1e-16, 0, _lib.ptr(rows), len(rows), 4, ctypes.c_uint64(1), ctypes.c_uint64(0),
                                 None, _lib.ptr(out), None)
    assert rc == -1
    pairs = np.array([0, 1], dtype=np.int32)
    eff = np.ascontiguousarray(noise.readout_effects(3, None))
    tables = np.zeros((1, 9, 4), dtype=np.int64)
    rc = lib.aqc_mps_traj_pair_tomo(3, 8, 1e-16, 0, _lib.ptr(rows), len(rows), _lib.ptr(pairs), 1, _lib.ptr(eff), 4,
                                    ctypes.c_uint64(1), ctypes.c_uint64(0), None, _lib.ptr(tables), None)
    assert rc == -1


def _malformed_programs():
    """(label, rows): the program of ops(3, 1) under model (b), whose groups hold 2 rows, broken one way each."""
    _, rows, _ = t2ref.program(3, 1, "b")
    g = int(np.flatnonzero((rows["flags"] & 0xFFFF) == _lib.OP_KRAUS2)[0])  # a group's first row
    assert int(rows["flags"][g]) == 3 | (2 << 16) and int(rows["flags"][g + 1]) == 3 | (1 << 8) | (2 << 16)
    dep = t2ref.program(3, 1, "a")[1]
    d = int(np.flatnonzero((dep["flags"] & 0xFFFF) == _lib.OP_KRAUS2)[0])
    out = []

    def case(label, base, edit):
        bad = base.copy()
        bad = edit(bad)
        out.append((label, np.ascontiguousarray(bad)))

    def swap(r):
        r[[d + 1, d + 2]] = r[[d + 2, d + 1]]
        return r

    def setf(field, i, value):
        def edit(r):
            r[field][i] = value
            return r
        return edit

    def setm(i, e, value):
        def edit(r):
            r["m"][i, e] = value
            return r
        return edit

    case("k out of order", dep, swap)
    case("a group without its first row", rows, lambda r: np.delete(r, g))
    case("a group cut short by a gate", rows, lambda r: np.delete(r, g + 1))
    case("a group cut short by the program's end", dep, lambda r: r[: d + 9])
    case("k repeated", rows, setf("flags", g + 1, 3 | (2 << 16)))
    case("nk = 0", rows, lambda r: setf("flags", g + 1, 3 | (1 << 8))(setf("flags", g, 3)(r)))
    case("nk = 17", dep, lambda r: np.concatenate([r[:d], np.repeat(r[d: d + 1], 17), r[d + 16:]]))
    case("nk differs inside the group", rows, setf("flags", g + 1, 3 | (1 << 8) | (3 << 16)))
    case("qubits differ inside the group", rows, lambda r: setf("q1", g + 1, int(r["q0"][g]))(
        setf("q0", g + 1, int(r["q1"][g]))(r)))
    case("q0 = q1", rows, lambda r: setf("q1", g + 1, int(r["q0"][g]))(setf("q1", g, int(r["q0"][g]))(r)))
    case("a qubit out of range", rows, lambda r: setf("q1", g + 1, 3)(setf("q1", g, 3)(r)))
    case("a negative qubit", rows, lambda r: setf("q0", g + 1, -1)(setf("q0", g, -1)(r)))
    case("nq = 1", rows, setf("nq", g, 1))
    case("bits above nk", rows, setf("flags", g, 3 | (2 << 16) | (1 << 24)))
    case("a NaN entry", rows, setm(g + 1, 5, np.nan))
    case("an infinite entry", rows, setm(g, 0, np.inf))
    case("sum K^dag K off the identity", rows, setm(g, 0, 1.0 + 1e-8))
    # nk = 17 needs its flags rewritten to a consistent group of 17
    label, r17 = out[6]
    r17["flags"][d: d + 17] = 3 | (np.arange(17) << 8) | (17 << 16)
    r17["m"][d: d + 17] *= np.sqrt(16 / 17)
    return out


MALFORMED = _malformed_programs()


@pytest.mark.parametrize("label,rows", MALFORMED, ids=[label for label, _ in MALFORMED])
def test_malformed_groups_answer_err_arg_on_the_host(label, rows):
    """build_rows runs before any device call: the C entry points answer AQC_ERR_ARG without a GPU."""
    import ctypes

    lib = _lib.load()  # (does not touch the GPU)
    out = np.zeros(4, dtype=np.uint64)
    rc = lib.aqc_sv_traj_sample(3, _lib.ptr(rows), len(rows), 4, ctypes.c_uint64(1), ctypes.c_uint64(0), None,
                                _lib.ptr(out), None)
    assert rc == -1, label
    pairs = np.array([0, 1], dtype=np.int32)
    eff = np.ascontiguousarray(noise.readout_effects(3, None))
    tables = np.zeros((1, 9, 4), dtype=np.int64)
    rc = lib.aqc_sv_traj_pair_tomo(3, _lib.ptr(rows), len(rows), _lib.ptr(pairs), 1, _lib.ptr(eff), 4,
                                   ctypes.c_uint64(1), ctypes.c_uint64(0), None, _lib.ptr(tables), None)
    assert rc == -1, label


@pytest.mark.gpu
def test_malformed_groups_through_the_device_wrapper():
    """The same programs through device.trajectory_sample (which selects the device first); the library
    still runs the well-formed program afterwards."""
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.device import trajectory_sample

    for label, rows in MALFORMED:
        with pytest.raises(AqcError, match="-1"):
            trajectory_sample(3, rows, noise.count_events(rows), 4, 1)
    _, rows, n_events = t2ref.program(3, 1, "b")
    assert trajectory_sample(3, rows, n_events, 4, 1).shape == (4,)
