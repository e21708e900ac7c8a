"""The references of sv_readers_ref.py pinned on the host against explicit dense operators, and the
side conditions of the shared sampling inputs, so that test_gpu_sv_readers.py can be trusted without
a GPU."""
import numpy as np
import pytest

import sampling_ref
import sv_readers_ref as R
from oracle.entanglement import partial_trace_sv


def _kron_on(n, q, m):
    """kron(I, m on qubit q, I) on n qubits (qubit 0 = least significant bit)."""
    return np.kron(np.kron(np.eye(2 ** (n - 1 - q)), m), np.eye(2 ** q))


def _one_qubit_rdm(psi, n, q):
    m = np.asarray(psi).reshape(2 ** (n - 1 - q), 2, 2 ** q)
    return np.einsum("hal,hbl->ab", m, m.conj())


@pytest.mark.parametrize("q", [0, 1, 2])
def test_transition_ref_is_the_explicit_matrix_element(q):
    n = 3
    bra, ket = R.random_state(n, 1000 + n), R.random_state(n, 2000 + n)
    T = R.transition_ref(bra, ket, n, q)
    for a in range(2):
        for b in range(2):
            e = np.zeros((2, 2))
            e[a, b] = 1.0  # |a><b|
            assert abs(T[a, b] - np.vdot(bra, _kron_on(n, q, e) @ ket)) < 1e-15
    v = R.random_unitary(40 + q)
    want = np.vdot(bra, _kron_on(n, q, v) @ ket)
    assert abs(np.sum(v * T) - want) < 1e-15
    assert abs(np.vdot(bra, R.apply_1q(ket, n, q, v)) - want) < 1e-15
    arbitrary = np.array([[0.3, -1.2j], [2.0 + 1j, 0.0]])  # any 2 x 2, not only unitaries
    assert abs(np.sum(arbitrary * T) - np.vdot(bra, _kron_on(n, q, arbitrary) @ ket)) < 1e-15


@pytest.mark.parametrize("n", [1, 3, 6])
def test_transition_ref_of_a_state_with_itself_is_the_transposed_rdm(n):
    psi = R.random_state(n, 1000 + n)
    for q in range(n):
        T = R.transition_ref(psi, psi, n, q)
        np.testing.assert_allclose(T, _one_qubit_rdm(psi, n, q).T, rtol=0, atol=1e-15)
        assert abs(np.trace(T) - 1.0) < 1e-15
        if n >= 2:  # and the one-qubit RDM is the pair RDM with the partner traced out
            other = (q + 1) % n
            rho = partial_trace_sv(psi, q, other).reshape(2, 2, 2, 2)  # [hi, lo, hi', lo']
            one = np.einsum("hlhm->lm", rho) if q < other else np.einsum("hlgl->hg", rho)
            np.testing.assert_allclose(T, one.T, rtol=0, atol=1e-15)


def test_z_ref_against_explicit_operators():
    n = 4
    psi = R.random_state(n, 1000 + n)
    want = [np.vdot(psi, _kron_on(n, q, np.diag([1.0, -1.0])) @ psi).real for q in range(n)]
    np.testing.assert_allclose(R.z_ref(psi, n), want, rtol=0, atol=1e-15)
    assert np.array_equal(R.z_ref(R.basis_state(n, 2 ** n - 1), n), -np.ones(n))
    assert np.array_equal(R.z_ref(R.basis_state(n, 0), n), np.ones(n))
    assert np.array_equal(R.z_ref(R.basis_state(1, 1), 1), [-1.0])


def test_sv_pauli_ref_against_explicit_operators():
    n = 3
    psi = R.random_state(n, 1000 + n)
    mats = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0])}
    for label in ("III", "IIX", "YII", "XYZ", "ZZY", "YYY"):
        op = np.ones((1, 1))
        for c in label:  # rightmost character = qubit 0
            op = np.kron(op, mats[c])
        assert abs(R.sv_pauli_ref(psi, label) - np.vdot(psi, op @ psi).real) < 1e-15
    # mask bits above 12: single Z and X terms against z_ref and apply_1q
    n = 14
    psi = R.random_state(n, 1000 + n)
    z = R.z_ref(psi, n)
    x = np.array([[0.0, 1.0], [1.0, 0.0]])
    for q in (0, 12, 13):
        label = "I" * (n - 1 - q) + "{}" + "I" * q
        assert abs(R.sv_pauli_ref(psi, label.format("Z")) - z[q]) < 1e-14
        assert abs(R.sv_pauli_ref(psi, label.format("X")) - np.vdot(psi, R.apply_1q(psi, n, q, x)).real) < 1e-14
    zz = np.vdot(psi, R.apply_1q(R.apply_1q(psi, n, 13, np.diag([1.0, -1.0])), n, 5, np.diag([1.0, -1.0]))).real
    assert abs(R.sv_pauli_ref(psi, "Z" + "I" * 7 + "Z" + "I" * 5) - zz) < 1e-14


def test_sparse_sample_ref_equals_the_dense_rule():
    n = 10
    rng = np.random.default_rng(10)
    idx = rng.choice(2 ** n, 40, replace=False)  # unsorted on purpose
    amps = rng.standard_normal(40) + 1j * rng.standard_normal(40)
    psi = R.embed(n, idx, amps)
    u = np.concatenate([R.philox_u(n, 2000), [0.0, 1.0 - 2.0 ** -53]])
    want, near = sampling_ref.sv_sample(psi, u)
    got, near_sparse = R.sparse_sample_ref(idx, amps, u)
    assert np.array_equal(got, want)
    assert not near[:2000].any() and not near_sparse[:2000].any()  # (the two edge u are boundaries)
    assert got[-2] == idx.min() and got[-1] == idx.max()
    for k in (int(idx.min()), int(idx.max()), int(np.sort(idx)[7])):
        assert R.sparse_neighbours(idx, amps, k) == sampling_ref.sv_neighbours(psi, k)


@pytest.mark.parametrize("name", [c["name"] for c in R.SAMPLING_CASES])
def test_sampling_cases_side_conditions(name):
    case, idx, amps, u, want, near = R.sampling_case(name)
    n, shots = case["n"], case["shots"]
    assert u.shape == (shots,) and u.min() >= 0.0 and u.max() < 1.0
    assert np.array_equal(u, sampling_ref.uniforms(2 ** 40 + 3 + n, 3, shots, 1)[:, 0])
    assert len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < 2 ** n
    assert abs(np.linalg.norm(amps) - 1.0) < 1e-14
    assert near.sum() <= 2  # the cap of test_gpu_sampling.py, from the reference alone
    assert np.isin(want, idx).all()
    tiles = np.unique(want // R.TILE)
    if case["dense"]:
        assert len(idx) == 2 ** n and shots == 4097
        assert len(tiles) == max(1, 2 ** n // R.TILE)  # every tile is drawn from
    elif n == 16:  # the dense rule on the embedded vector gives the same outcomes
        dense_want, dense_near = sampling_ref.sv_sample(R.embed(n, idx, amps), u)
        assert np.array_equal(dense_want, want) and np.array_equal(dense_near, near)
    if name == "inside_tile_9":
        assert list(tiles) == [9] and len(np.unique(want)) > 25
    if name == "tiles_1_and_14":
        assert list(tiles) == [1, 14]
        p = np.abs(amps) ** 2
        assert abs(p[idx // R.TILE == 1].sum() - 0.5) < 1e-15 and abs(p[idx // R.TILE == 14].sum() - 0.5) < 1e-15
        assert 0.4 < np.mean(want // R.TILE == 14) < 0.6
    if name == "sparse25":
        # outcomes in both 4096-tile chunks of the tile scan, in a few hundred distinct tiles
        assert shots == 4097 and len(idx) == 300
        assert set(np.unique(tiles // 4096)) == {0, 1} and len(tiles) > 200


def test_exact_tie_inputs_are_exact_in_double():
    """The uniform state 2^-8 at n = 16: probabilities and prefix sums are dyadic, so u = k / 2^16
    lies on a CDF boundary exactly and the rule (smallest k with C_k > u P) gives k itself."""
    n = 16
    psi = np.full(2 ** n, 2.0 ** -8, dtype=complex)
    ks = np.array([0, 1, 4095, 4096, 4097, 65535])
    u = np.concatenate([ks / 2.0 ** 16, [0.0, 1.0 - 2.0 ** -53]])
    c = np.cumsum(np.abs(psi) ** 2)
    assert np.array_equal(c, np.arange(1, 2 ** n + 1) / 2.0 ** n) and c[-1] == 1.0
    want, _ = sampling_ref.sv_sample(psi, u)
    assert list(want) == list(ks) + [0, 65535]
