"""Host side of the ground-state path: the x-mask grouping aqc_sv_pauli_apply does, mps_from_vector and
the refusals of calculate_ground_state that need no device."""
import numpy as np
import pytest

import pauli_apply_ref as ref
from adaptaqc_amd import paulis
from adaptaqc_amd.mps_operations import check_mps, mps_from_vector
from adaptaqc_amd.utils.hamiltonians import calculate_ground_state, heisenberg_hamiltonian


# ---- grouping ----------------------------------------------------------------------------------
def test_group_order_and_term_order():
    #        x     z     c
    terms = [(0b011, 0b000, 1.0), (0b000, 0b001, 2.0), (0b011, 0b100, 3.0), (0b110, 0b000, 4.0),
             (0b000, 0b110, 5.0), (0b011, 0b000, 6.0)]
    x, z, c = zip(*terms)
    groups = paulis.group_by_xmask(x, z, c)
    assert [g[0] for g in groups] == [0b011, 0b000, 0b110]  # first appearance
    assert groups[0][1] == [(0b000, 1.0), (0b100, 3.0), (0b000, 6.0)]  # input order; equal terms are not merged
    assert groups[1][1] == [(0b001, 2.0), (0b110, 5.0)]
    assert groups[2][1] == [(0b000, 4.0)]


def test_group_y_phases():
    c = 0.5 - 0.25j
    for ny, want in ((1, 1j * c), (2, -c), (3, -1j * c)):
        m = (1 << ny) - 1
        (x, members), = paulis.group_by_xmask([m], [m], [c])
        assert x == m and members == [(m, want)]
    # an X and a Z on different qubits have no phase
    (x, members), = paulis.group_by_xmask([0b01], [0b10], [c])
    assert members == [(0b10, c)]


def test_group_identity_term():
    groups = paulis.group_by_xmask([0, 0b1, 0], [0, 0, 0b1], [0.75, 1.0, 2.0])
    assert groups[0] == (0, [(0, 0.75), (0b1, 2.0)])  # the offset sits in the diagonal group


def test_group_heisenberg_chain_count():
    n = 8
    ham = heisenberg_hamiltonian(n, -1.0, -1.0, -1.0)
    assert len(ham) == 3 * (n - 1)
    x, z, c = paulis.operator_to_masks(ham, n)
    groups = paulis.group_by_xmask(x, z, c)
    # XX and YY of a bond share their x mask; every ZZ is in the diagonal group
    assert len(groups) == (n - 1) + 1
    assert sorted(len(m) for _, m in groups) == [2] * (n - 1) + [n - 1]
    periodic = heisenberg_hamiltonian(n, -1.0, -1.0, -1.0, hz=0.5, periodic_bc=True)
    xp, zp, cp = paulis.operator_to_masks(periodic, n)
    assert len(paulis.group_by_xmask(xp, zp, cp)) == n + 1


def test_grouped_sum_is_the_operator():
    """The grouping evaluated as the kernel does, against the term-by-term restatement."""
    rng = np.random.default_rng(3)
    n = 5
    labels = ["".join(rng.choice(list("IXYZ"), n)) for _ in range(30)]
    op = {s: complex(rng.normal(), rng.normal()) for s in labels}
    psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    x, z, c = paulis.operator_to_masks(op, n)
    out = np.zeros_like(psi)
    for j in range(1 << n):
        for xg, members in paulis.group_by_xmask(x, z, c):
            k = j ^ xg
            out[j] += sum(-cp if bin(k & zt).count("1") & 1 else cp for zt, cp in members) * psi[k]
    want = ref.apply_operator(op, psi)
    assert np.max(np.abs(out - want)) <= 1e-12 * ref.weight(op) * np.max(np.abs(psi))


def test_operator_to_masks_forms():
    x, z, c = paulis.operator_to_masks({"XY": 2.0, "IZ": -1j}, 2)
    assert list(x) == [0b11, 0] and list(z) == [0b01, 0b01] and list(c) == [2.0, -1j]
    x2, z2, c2 = paulis.operator_to_masks((["XY", "IZ"], [2.0, -1j]), 2)
    assert list(x2) == list(x) and list(z2) == list(z) and list(c2) == list(c)
    with pytest.raises(ValueError):
        paulis.operator_to_masks((["XY", "IZ"], [2.0]), 2)
    assert ref.label_masks("XY") == (0b11, 0b01)


def test_restatement_dense_matrix_agrees_with_its_apply():
    """The reference's two routes agree, and a known matrix comes out: XX + YY + ZZ on two qubits."""
    h = ref.dense_hamiltonian({"XX": 1.0, "YY": 1.0, "ZZ": 1.0}, 2)
    assert np.array_equal(h, np.array([[1, 0, 0, 0], [0, -1, 2, 0], [0, 2, -1, 0], [0, 0, 0, 1]], dtype=complex))
    rng = np.random.default_rng(8)
    op = {"XIZY": 0.5, "IYYI": -1.5 + 0.5j, "ZZII": 2.0, "IIII": 0.25}
    psi = rng.normal(size=16) + 1j * rng.normal(size=16)
    assert np.max(np.abs(ref.dense_hamiltonian(op, 4) @ psi - ref.apply_operator(op, psi))) <= 1e-14 * ref.weight(op) * 4
    # Y on qubit 0 of two: Y|00> = i|01>
    assert np.array_equal(ref.apply_operator({"IY": 1.0}, np.array([1, 0, 0, 0])), np.array([0, 1j, 0, 0]))


# ---- mps_from_vector ---------------------------------------------------------------------------
def _contract(gam, lam):
    """Dense vector of an Aer-format MPS, index bit q = qubit q, in numpy."""
    n = len(gam)
    out = np.zeros(1 << n, dtype=complex)
    for idx in range(1 << n):
        m = np.ones((1, 1), dtype=complex)
        for q in range(n):
            m = m @ gam[q][(idx >> q) & 1]
            if q < n - 1:
                m = m * lam[q][None, :]
        out[idx] = m[0, 0]
    return out


def test_mps_from_vector_roundtrip():
    rng = np.random.default_rng(11)
    n = 6
    psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    psi /= np.linalg.norm(psi)
    gam, lam = mps_from_vector(psi)
    assert check_mps((gam, lam))
    assert [len(s) for s in lam] == [2, 4, 8, 4, 2]
    assert all(np.all(np.diff(s) <= 0) for s in lam)
    assert np.max(np.abs(_contract(gam, lam) - psi)) <= 1e-12
    # Vidal form: sum_s (Gamma^s lam)^H ... left-normalised sites lam_{q-1} Gamma_q
    for q in range(n - 1):
        left = np.ones(1) if q == 0 else lam[q - 1]
        a = np.concatenate([left[:, None] * gam[q][0], left[:, None] * gam[q][1]], axis=0)
        assert np.max(np.abs(a.conj().T @ a - np.eye(a.shape[1]))) <= 1e-12


def test_mps_from_vector_product_and_ghz():
    n = 5
    rng = np.random.default_rng(5)
    qubits = [rng.normal(size=2) + 1j * rng.normal(size=2) for _ in range(n)]
    prod = np.ones(1, dtype=complex)
    for v in qubits:  # qubit 0 fastest
        prod = np.kron(v / np.linalg.norm(v), prod)
    gam, lam = mps_from_vector(prod)
    assert [len(s) for s in lam] == [1] * (n - 1)
    assert np.max(np.abs(_contract(gam, lam) - prod)) <= 1e-12
    ghz = np.zeros(1 << n, dtype=complex)
    ghz[0] = ghz[-1] = 2 ** -0.5
    gam, lam = mps_from_vector(ghz)
    assert [len(s) for s in lam] == [2] * (n - 1)
    assert all(np.allclose(s, [2 ** -0.5, 2 ** -0.5], atol=1e-14) for s in lam)
    assert check_mps((gam, lam))
    assert np.max(np.abs(_contract(gam, lam) - ghz)) <= 1e-12


def test_mps_from_vector_max_chi_and_threshold():
    rng = np.random.default_rng(12)
    n = 6
    psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    psi /= np.linalg.norm(psi)
    gam, lam = mps_from_vector(psi, max_chi=3)
    assert [len(s) for s in lam] == [2, 3, 3, 3, 2]
    assert check_mps((gam, lam))
    assert all(a.shape == b.shape for a, b in gam)
    approx = _contract(gam, lam)
    assert 0.3 < abs(np.vdot(psi, approx)) <= 1.0 + 1e-12  # a truncation, still close to the state
    # a threshold above every lambda^2 but the first leaves bond 1
    gam, lam = mps_from_vector(psi, trunc_thr=0.99)
    assert [len(s) for s in lam] == [1] * (n - 1)
    with pytest.raises(ValueError):
        mps_from_vector(np.ones(6))
    with pytest.raises(ValueError):
        mps_from_vector(psi, max_chi=0)
    # one qubit: no bonds
    gam, lam = mps_from_vector(np.array([0.6, 0.8j]))
    assert lam == [] and gam[0][0].shape == (1, 1) and abs(gam[0][1][0, 0] - 0.8j) < 1e-15


# ---- refusals that need no device --------------------------------------------------------------
@pytest.mark.parametrize("ham, word", [
    ({}, "non-empty"),
    ({"XX": 1.0, "Z": 0.5}, "same length"),
    ({"XX": 1.0 + 0.5j}, "imaginary"),
    ({"XX": float("nan")}, "finite"),
    ([("XX", 1.0)], "non-empty"),
])
def test_calculate_ground_state_refusals(ham, word):
    with pytest.raises(ValueError, match=word):
        calculate_ground_state(ham)


def test_calculate_ground_state_bad_letter_and_options():
    with pytest.raises(ValueError, match="unknown Pauli letter"):
        calculate_ground_state({"XQ": 1.0})
    with pytest.raises(ValueError, match="tol > 0"):
        calculate_ground_state({"XX": 1.0}, tol=0.0)
    with pytest.raises(ValueError, match="max_iterations"):
        calculate_ground_state({"XX": 1.0}, max_iterations=0)
