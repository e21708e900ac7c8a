"""The DMRG bond plan (aqc_mps_dmrg_plan, no GPU), calculate_ground_state_mps's argument checks, and the
numpy restatement's own consistency (tests/dmrg_ref.py)."""
import numpy as np
import pytest

import dmrg_ref
import pauli_apply_ref as ref

CLOSED_L, CLOSED_R, LOCAL, OPEN, IDENT = range(5)
LH, RH, LOC, OPN = range(4)


def _label(n, ops):
    chars = ["I"] * n
    for q, p in ops:
        chars[n - 1 - q] = p
    return "".join(chars)


def _chain_with_fields(n):
    """XX, YY, ZZ on every neighbour pair (in that order, pair by pair), then Z on every site."""
    ham = {}
    for i in range(n - 1):
        for p in "XYZ":
            ham[_label(n, [(i, p), (i + 1, p)])] = 1.0
    for i in range(n):
        ham[_label(n, [(i, "Z")])] = 0.5
    return ham


def test_plan_heisenberg_chain_with_fields():
    """n = 6: term 3 i + k is the k-th letter on the pair (i, i + 1), term 15 + i the field on site i."""
    from adaptaqc_amd.device import dmrg_plan

    n = 6
    plan = dmrg_plan(n, _chain_with_fields(n), chi_cap=8)
    # per bond: records, closed-left terms, closed-right terms, local terms, open records, stored left
    # environments of open terms (the pair (b - 1, b) crosses cut b), stored right ones (the pair (b + 1, b + 2))
    want_bonds = [
        [5, 0, 13, 5, 3, 0, 3],  # local: the pair (0, 1), Z_0, Z_1; open: the pair (1, 2); the rest closed right
        [9, 1, 9, 5, 6, 3, 3],   # closed left: Z_0; open: the pairs (0, 1) and (2, 3)
        [9, 5, 5, 5, 6, 3, 3],   # closed left: the pair (0, 1), Z_0, Z_1; closed right: the pair (4, 5), Z_4, Z_5
        [9, 9, 1, 5, 6, 3, 3],
        [5, 13, 0, 5, 3, 3, 0],
    ]
    assert plan["bonds"].tolist() == want_bonds
    assert plan["records"].shape == (37, 4) and plan["max_records"] == 9 and plan["identities"] == 0
    # bond 2 in full: LH, RH, the local matrix, then the open terms in input order with their flags
    rows = plan["records"][plan["records"][:, 0] == 2][:, 1:].tolist()
    assert rows == [[LH, -1, 1], [RH, -1, 2], [LOC, -1, 0],
                    [OPN, 3, 1], [OPN, 4, 1], [OPN, 5, 1],      # the pair (1, 2): a stored left environment
                    [OPN, 9, 2], [OPN, 10, 2], [OPN, 11, 2]]   # the pair (3, 4): a stored right one
    # bond 0 has no LH and bond n - 2 no RH
    assert plan["records"][plan["records"][:, 0] == 0][:, 1].tolist() == [RH, LOC, OPN, OPN, OPN]
    assert plan["records"][plan["records"][:, 0] == 4][:, 1].tolist() == [LH, LOC, OPN, OPN, OPN]
    # classes at bond 2: pairs (0,1) closed left, (1,2) open, (2,3) local, (3,4) open, (4,5) closed right;
    # fields 0, 1 closed left, 2, 3 local, 4, 5 closed right
    want = [CLOSED_L] * 3 + [OPEN] * 3 + [LOCAL] * 3 + [OPEN] * 3 + [CLOSED_R] * 3 + \
           [CLOSED_L, CLOSED_L, LOCAL, LOCAL, CLOSED_R, CLOSED_R]
    assert plan["classes"][2].tolist() == want
    # stored matrices: per cut 1 .. n - 1 and per side the closed sum and the 3 crossing terms
    assert plan["env_matrices"] == 2 * (n - 1) * 4
    assert plan["env_bytes"] == plan["env_matrices"] * 8 * 8 * 16
    assert plan["record_limit"] >= 9 and plan["byte_budget"] > plan["env_bytes"] + plan["scratch_bytes"]


def _class_by_definition(lo, hi, b):
    if lo is None:
        return IDENT
    if hi < b:
        return CLOSED_L
    if lo > b + 1:
        return CLOSED_R
    if b <= lo and hi <= b + 1:
        return LOCAL
    return OPEN


def test_plan_long_range_three_body_identity_and_end_terms():
    from adaptaqc_amd.device import dmrg_plan

    n = 6
    terms = [(_label(n, [(0, "X"), (5, "X")]), 0.3, 0, 5),
             (_label(n, [(1, "Y"), (2, "Y"), (4, "Y")]), -0.7, 1, 4),
             ("I" * n, 1.25, None, None),
             (_label(n, [(0, "Z")]), 0.5, 0, 0),
             (_label(n, [(5, "X")]), -0.4, 5, 5)]
    ham = {t[0]: t[1] for t in terms}
    plan = dmrg_plan(n, ham, chi_cap=4)
    assert plan["identities"] == 1
    for b in range(n - 1):
        want = [_class_by_definition(lo, hi, b) for _, _, lo, hi in terms]
        assert plan["classes"][b].tolist() == want, b
    # X0 X5 is open at every bond; Y1 Y2 Y4 from bond 0 (its first site is b + 1) to bond 4
    assert plan["classes"][:, 0].tolist() == [OPEN] * 5
    assert plan["classes"][:, 1].tolist() == [OPEN, OPEN, OPEN, OPEN, OPEN]
    assert plan["classes"][:, 3].tolist() == [LOCAL, CLOSED_L, CLOSED_L, CLOSED_L, CLOSED_L]
    assert plan["classes"][:, 4].tolist() == [CLOSED_R, CLOSED_R, CLOSED_R, CLOSED_R, LOCAL]
    # flags: bond 0, X0 X5 starts at the bond (no left environment, a right one); Y1 Y2 Y4 likewise
    rows = plan["records"][plan["records"][:, 0] == 0][:, 1:].tolist()
    assert rows == [[RH, -1, 2], [LOC, -1, 0], [OPN, 0, 2], [OPN, 1, 2]]
    # bond 3 (sites 3, 4): both open terms have a left environment, X0 X5 a right one too
    rows = plan["records"][plan["records"][:, 0] == 3][:, 1:].tolist()
    assert rows == [[LH, -1, 1], [RH, -1, 2], [OPN, 0, 3], [OPN, 1, 1]]
    # crossing terms per cut 1 .. 5: X0 X5 all, Y1 Y2 Y4 cuts 2, 3, 4
    assert plan["env_matrices"] == 2 * sum(1 + k for k in (1, 2, 2, 2, 1))


def test_plan_refusals_name_their_numbers():
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.device import dmrg_plan

    n = 6
    small = dmrg_plan(n, _chain_with_fields(n), chi_cap=8)
    limit, budget = small["record_limit"], small["byte_budget"]
    # every pair of 80 qubits with three letters: 3 * 40 * 40 terms cross the middle bond
    m = 80
    dense = {_label(m, [(i, p), (j, p)]): 1.0 for i in range(m) for j in range(i + 1, m) for p in "XYZ"}
    assert 3 * 39 * 39 > limit
    with pytest.raises(AqcError, match=rf"bond \d+ has \d+ records, above the limit of {limit}"):
        dmrg_plan(m, dense, chi_cap=4)
    # a 100-site chain at capacity 1024: 2 * 99 * 4 matrices of 16 MiB
    assert 2 * 99 * 4 * 1024 * 1024 * 16 > budget
    with pytest.raises(AqcError, match=rf"need \d+ bytes at capacity 1024, above the budget of {budget}"):
        dmrg_plan(100, _chain_with_fields(100), chi_cap=1024)
    with pytest.raises(AqcError, match="n must be in 2"):
        dmrg_plan(1, {"Z": 1.0})
    with pytest.raises(AqcError, match="krylov_dim"):
        dmrg_plan(n, _chain_with_fields(n), krylov_dim=17)
    with pytest.raises(ValueError, match="characters for 6 qubits"):
        dmrg_plan(n, {"ZZ": 1.0})
    with pytest.raises(ValueError, match="real coefficients"):
        dmrg_plan(n, {"ZZIIII": 1.0j})


def test_ground_state_mps_argument_checks():
    """Every refusal comes before the device is touched."""
    from adaptaqc_amd.utils import hamiltonians as H

    ham = H.heisenberg_hamiltonian(4, -1.0, -1.0, -1.0)
    with pytest.raises(ValueError, match="at least 2 qubits"):
        H.calculate_ground_state_mps({"Z": 1.0})
    with pytest.raises(ValueError, match="non-empty"):
        H.calculate_ground_state_mps({})
    with pytest.raises(ValueError, match="same length"):
        H.calculate_ground_state_mps({"ZZ": 1.0, "Z": 1.0})
    with pytest.raises(ValueError, match="imaginary part"):
        H.calculate_ground_state_mps({"ZZ": 1.0j})
    for kw in (dict(tol=0.0), dict(max_sweeps=0), dict(max_chi=0), dict(threshold=-1.0)):
        with pytest.raises(ValueError, match="tol > 0"):
            H.calculate_ground_state_mps(ham, **kw)
    for k in (1, 17):
        with pytest.raises(ValueError, match="krylov_dim"):
            H.calculate_ground_state_mps(ham, krylov_dim=k)
    with pytest.raises(ValueError, match="not both"):
        H.calculate_ground_state_mps(ham, initial_circuit=object(), initial_mps=([], []))


def test_squared_operator_matches_dense():
    from adaptaqc_amd import paulis
    from adaptaqc_amd.utils import hamiltonians as H

    n = 5
    ham = H.heisenberg_hamiltonian(n, -1.0, 0.5, 0.25, hx=0.3, hz=-0.2)
    ham["I" * n] = 0.75
    ham[_label(n, [(0, "X"), (2, "Y"), (4, "Z")])] = 0.4
    labels = list(ham)
    codes, coeffs = H._squared_operator(paulis.terms_to_codes(labels, n), np.array([ham[s] for s in labels]))
    sq = {paulis.codes_to_label(c): v for c, v in zip(codes, coeffs)}
    dense = ref.dense_hamiltonian(ham, n)
    assert np.max(np.abs(ref.dense_hamiltonian(sq, n) - dense @ dense)) <= 1e-12 * ref.weight(ham) ** 2


def test_restatement_projection_equals_term_formula():
    """P^dag H P from the dense H equals the per-term environment formula on a random canonical MPS."""
    n = 8
    rng = np.random.default_rng(5)
    psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    psi /= np.linalg.norm(psi)
    mps = dmrg_ref.vidal_from_vector(psi)
    assert np.max(np.abs(dmrg_ref.to_vector(mps) - psi)) <= 1e-13
    ham = _chain_with_fields(n)
    ham[_label(n, [(0, "X"), (5, "X")])] = 0.3
    ham[_label(n, [(1, "Y"), (2, "Y"), (4, "Y")])] = -0.7
    ham["I" * n] = 1.25
    scale = ref.weight(ham)
    for b in (0, 3, n - 2):
        dense, p = dmrg_ref.heff_dense(ham, mps, b)
        assert np.max(np.abs(p.conj().T @ p - np.eye(p.shape[1]))) <= 1e-12  # the bases are orthonormal
        dim = dense.shape[0]
        dense = dense - dmrg_ref.shift(ham) * np.eye(dim)
        cols = np.stack([dmrg_ref.heff_terms(ham, mps, b, np.eye(dim)[:, k]) for k in range(dim)], axis=1)
        err = np.max(np.abs(cols - dense))
        print(f"bond {b}: dim {dim}, max |P^dag H P - per-term| = {err:.3e}")
        assert err <= 1e-12 * scale


def test_restatement_dmrg_reaches_the_ground_state():
    from adaptaqc_amd.utils.hamiltonians import heisenberg_hamiltonian

    n = 6
    ham = heisenberg_hamiltonian(n, -1.0, -1.0, -1.0)
    vals, _ = ref.spectrum(ham, n)
    energy, mps, info = dmrg_ref.dmrg(ham, n, tol=1e-9, krylov_dim=4)
    print("restatement: E - lambda0", energy - vals[0], info["sweeps"], "sweeps", info["breakdowns"], "breakdowns")
    assert abs(energy - vals[0]) <= 1e-10 * ref.weight(ham)
    assert abs(np.linalg.norm(dmrg_ref.to_vector(mps)) - 1) <= 1e-12
