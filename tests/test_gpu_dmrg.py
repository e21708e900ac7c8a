"""Two-site DMRG on the MPS engine (dmrg.hip) on MI355X: the effective Hamiltonian against the numpy
restatement (tests/dmrg_ref.py: P^dag H P from the dense H, and the per-term environment formula), one
sweep's Ritz values, calculate_ground_state_mps against numpy's spectra, the statevector solver and its
own restatement, and a ground state compiled end to end.

Bounds.  An output element of H_eff x is a sum over at most 2 chi + records products of magnitude
<= S |x|_2 (environment norms are at most 1), so its rounding is about (2 chi + records) 2^-53 S |x|_2, 2e-14 at
chi = 80: the bound 1e-12 S |x|_2 leaves a factor 50.  The ground states run at tol = 1e-9; every case first
asserts, on numpy's spectrum and the restatement alone, that its gap exceeds 100 tol S and that the
restatement itself lands within 0.1 tol S of the ground level."""
import functools

import numpy as np
import pytest

import dmrg_ref
import pauli_apply_ref as ref

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _label(n, ops):
    chars = ["I"] * n
    for q, p in ops:
        chars[n - 1 - q] = p
    return "".join(chars)


def _operator(n):
    """The Heisenberg chain with fields, a long-range term, a three-body term and the identity."""
    from adaptaqc_amd.utils.hamiltonians import heisenberg_hamiltonian

    ham = heisenberg_hamiltonian(n, -1.0, 0.5, 0.25, hx=0.3, hz=-0.2)
    if n >= 6:
        ham[_label(n, [(0, "X"), (5, "X")])] = 0.3
        ham[_label(n, [(1, "Y"), (2, "Y"), (4, "Y")])] = -0.7
    ham["I" * n] = 1.25
    return ham


def _random_unitary(rng):
    q, r = np.linalg.qr(rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4)))
    return q * (np.diag(r) / np.abs(np.diag(r)))[None, :]


@functools.lru_cache(maxsize=None)
def _brickwork(n, cap, max_chi, seed):
    """(DeviceMPS, its Aer-format tensors) of 2 n layers of random two-qubit gates: every bond is full."""
    from adaptaqc_amd.device import DeviceMPS

    rng = np.random.default_rng(seed)
    mps = DeviceMPS(n, cap, 1e-16, max_chi)
    ops = []
    for layer in range(2 * n):
        for q in range(layer % 2, n - 1, 2):
            ops.append((_random_unitary(rng), (q, q + 1)))
    mps.apply(ops)
    return mps, mps.to_aer()


def _vector(dim, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=dim) + 1j * rng.normal(size=dim)


@pytest.mark.parametrize("n,bonds", [(2, [0]), (6, [0, 2, 4]), (10, [0, 3, 4, 5, 8])])
def test_heff_apply_matches_projection_and_term_formula(n, bonds):
    """Bond 0 (chi_l = 1), bond n - 2 (chi_r = 1), the middle bond of n = 6 (4 x 4, below one MFMA tile) and of
    n = 10 (16 x 16, the 32 of the middle lambda inside theta) with its neighbours (8 x 32 and 32 x 8); the
    untruncated brickwork state is canonical at every bond."""
    from adaptaqc_amd.device import DeviceDMRG

    mps, aer = _brickwork(n, 1 << (n // 2), None, 10 + n)
    ham = _operator(n)
    scale = ref.weight(ham)
    dm = DeviceDMRG(mps, ham)
    dims = mps.dims()
    for b in bonds:
        dim = 4 * int(dims[b]) * int(dims[b + 2])
        x, z = _vector(dim, 100 + b), _vector(dim, 200 + b)
        y = dm.heff_apply(b, x)
        dense, _ = dmrg_ref.heff_dense(ham, aer, b)
        want_dense = dense @ x - dmrg_ref.shift(ham) * x
        want_terms = dmrg_ref.heff_terms(ham, aer, b, x)
        bound = 1e-12 * scale * np.linalg.norm(x)
        e1, e2 = np.max(np.abs(y - want_dense)), np.max(np.abs(y - want_terms))
        print(f"n={n} bond {b} dims {dims[b]} x {dims[b + 2]}: vs P^dag H P {e1:.3e}, vs per-term {e2:.3e}, bound {bound:.3e}")
        assert np.linalg.norm(want_terms) > 0
        assert e1 <= bound and e2 <= bound
        assert np.array_equal(dm.heff_apply(b, x).view(np.uint64), y.view(np.uint64))  # the same bits
        hz = dm.heff_apply(b, z)
        herm = abs(np.vdot(x, hz) - np.conj(np.vdot(z, y)))
        assert herm <= 1e-12 * scale * np.linalg.norm(x) * np.linalg.norm(z)
    if n >= 6:
        assert int(dims[n // 2]) == 1 << (n // 2)
    dm.close()


def test_heff_apply_wide_bond_crosses_the_gemm_block():
    """n = 14 at max_chi = 80: the middle lambda has 80 entries, so the bonds next to the middle one are 32 x 80 and
    80 x 32 -- past the 64-wide GEMM block and no multiple of 16 -- and the middle one 64 x 64; against the per-term
    formula on the same (truncated) tensors."""
    from adaptaqc_amd.device import DeviceDMRG

    n = 14
    mps, aer = _brickwork(n, 80, 80, 77)
    ham = _operator(n)
    scale = ref.weight(ham)
    dm = DeviceDMRG(mps, ham)
    dims = mps.dims()
    b = n // 2 - 1
    assert int(dims[b]) == 64 and int(dims[b + 1]) == 80 and int(dims[b + 2]) == 64
    for bond in (b - 1, b, b + 1):  # (chi_l, chi_r) = (32, 80), (64, 64) and (80, 32)
        dim = 4 * int(dims[bond]) * int(dims[bond + 2])
        x = _vector(dim, 300 + bond)
        y = dm.heff_apply(bond, x)
        want = dmrg_ref.heff_terms(ham, aer, bond, x)
        err, bound = np.max(np.abs(y - want)), 1e-12 * scale * np.linalg.norm(x)
        print(f"n={n} bond {bond} dims {dims[bond]} x {dims[bond + 2]}: vs per-term {err:.3e}, bound {bound:.3e}")
        assert err <= bound
        assert np.array_equal(dm.heff_apply(bond, x).view(np.uint64), y.view(np.uint64))
    dm.close()


def test_heff_apply_80_by_80():
    """A bond with 80 on both sides: n = 16 at max_chi = 80, bond 7 (dims[7] = dims[9] = 80)."""
    from adaptaqc_amd.device import DeviceDMRG

    n = 16
    mps, aer = _brickwork(n, 80, 80, 78)
    ham = _operator(n)
    dm = DeviceDMRG(mps, ham)
    dims = mps.dims()
    bond = 7
    assert int(dims[bond]) == 80 and int(dims[bond + 2]) == 80
    x = _vector(4 * 80 * 80, 5)
    y = dm.heff_apply(bond, x)
    want = dmrg_ref.heff_terms(ham, aer, bond, x)
    err, bound = np.max(np.abs(y - want)), 1e-12 * ref.weight(ham) * np.linalg.norm(x)
    print(f"n={n} bond {bond} 80 x 80: vs per-term {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    dm.close()


# ---- ground states -----------------------------------------------------------------------------
HAMILTONIANS = {
    "antiferromagnet n=2": (2, dict(jx=-1.0, jy=-1.0, jz=-1.0)),
    "transverse-field Ising n=8": (8, dict(jx=0.0, jz=1.0, hx=0.7)),
    "ferromagnet n=4": (4, dict(jx=1.0, jy=1.0, jz=1.0)),
    "antiferromagnet n=6": (6, dict(jx=-1.0, jy=-1.0, jz=-1.0)),
    "open antiferromagnet n=10": (10, dict(jx=-1.0, jy=-1.0, jz=-1.0)),
}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(n, ham, S, eigenvalues, ground-space basis, gap) from numpy's eigh, with the input conditions
    asserted on numpy and the restatement alone."""
    from adaptaqc_amd.utils.hamiltonians import heisenberg_hamiltonian

    n, kw = HAMILTONIANS[name]
    ham = heisenberg_hamiltonian(n, **kw)
    scale = ref.weight(ham)
    vals, vecs = ref.spectrum(ham, n)
    ground = vals <= vals[0] + 1e-10 * scale
    gap = float(vals[np.count_nonzero(ground)] - vals[0])
    assert gap > 100 * TOL * scale
    e_ref, _, info = dmrg_ref.dmrg(ham, n, max_chi=1 << (n // 2), tol=TOL)
    print(f"{name}: restatement E - lambda0 {e_ref - vals[0]:.3e} in {info['sweeps']} sweeps")
    assert e_ref - vals[0] <= 0.1 * TOL * scale
    return n, ham, scale, vals, vecs[:, ground], gap


def _solve_and_check(name, degeneracy, **kw):
    from adaptaqc_amd.mps_operations import mps_to_vector
    from adaptaqc_amd.utils import hamiltonians

    n, ham, scale, vals, ground, gap = _reference(name)
    assert ground.shape[1] == degeneracy
    energy, mps = hamiltonians.calculate_ground_state_mps(ham, max_chi=1 << (n // 2), tol=TOL, **kw)
    run = hamiltonians.last_run_mps
    psi = np.asarray(mps_to_vector(mps))
    print(f"{name}: E {energy!r} lambda0 {vals[0]!r} E - lambda0 {energy - vals[0]:.3e} sweeps {run.sweeps} "
          f"max bond {run.max_bond} breakdowns {run.breakdowns} of {run.updates} variance {run.variance:.3e}")
    assert run.energy == energy and run.scale == scale and run.sweeps == len(run.energies)
    assert -1e-12 * scale <= energy - vals[0] <= TOL * scale
    assert abs(np.linalg.norm(psi) - 1.0) <= 1e-12
    hpsi = ref.apply_operator(ham, psi)
    e_np = float(np.vdot(psi, hpsi).real)
    assert abs(energy - e_np) <= 1e-11 * scale
    var = max(float(np.vdot(hpsi, hpsi).real) - e_np * e_np, 0.0)
    sigma = np.sqrt(var)
    inside = float(np.sum(np.abs(ground.conj().T @ psi) ** 2))
    print(f"{name}: 1 - |P psi|^2 = {1 - inside:.3e}, bound {var / (gap - sigma) ** 2 + 1e-12:.3e}")
    assert sigma < gap and 1 - inside <= var / (gap - sigma) ** 2 + 1e-12
    return energy, psi, run


def test_ground_state_two_qubit_singlet_breaks_down():
    energy, psi, run = _solve_and_check("antiferromagnet n=2", 1)
    assert abs(energy + 3.0) <= 1e-12 * 3.0
    singlet = np.array([0, 1, -1, 0]) / np.sqrt(2)
    assert 1 - abs(np.vdot(singlet, psi)) ** 2 <= 1e-12
    # four dimensions and six Krylov steps: every update ends on the breakdown rule
    assert run.updates == 2 * run.sweeps and run.breakdowns == run.updates


def test_ground_state_transverse_field_ising():
    _solve_and_check("transverse-field Ising n=8", 1)


def test_ground_state_degenerate_ferromagnet():
    energy, _, _ = _solve_and_check("ferromagnet n=4", 5)
    assert abs(energy + 3.0) <= 1e-9 * 9.0


def test_ground_state_six_qubits_breaks_down_at_the_chain_ends():
    """krylov_dim = 16: an end bond has at most 4 * 1 * 4 = 16 dimensions, so each of its four updates a sweep
    (bond 0 first and last, bond n - 2 twice in the middle) exhausts its space and ends on the breakdown rule."""
    _, _, run = _solve_and_check("antiferromagnet n=6", 1, krylov_dim=16)
    assert run.breakdowns >= 4 * run.sweeps


def test_ground_state_open_chain_ten_qubits():
    _solve_and_check("open antiferromagnet n=10", 1)


def test_one_sweep_lowers_the_energy_bond_by_bond():
    from adaptaqc_amd.device import DeviceDMRG, DeviceMPS

    name = "transverse-field Ising n=8"
    n, ham, scale, vals, _, _ = _reference(name)
    mps = DeviceMPS(n, 16, 1e-16, 16)
    gam, lam = dmrg_ref.product_state(n, 0)
    mps.load_aer((gam, lam))
    dm = DeviceDMRG(mps, ham)
    ritz = dm.sweep()
    print("Ritz values", ritz - vals[0])
    assert ritz.shape == (2 * (n - 1),)
    assert np.all(np.diff(ritz) <= 1e-12 * scale)
    assert np.all(ritz >= vals[0] - 1e-12 * scale)
    assert ritz[-1] < ritz[0] - 0.1  # and it does go down
    dm.close()
    mps.close()


@functools.lru_cache(maxsize=None)
def _truncated_reference(chi):
    n, ham, _, vals, _, _ = _reference("open antiferromagnet n=10")
    e_ref, _, _ = dmrg_ref.dmrg(ham, n, max_chi=chi, tol=TOL)
    return e_ref - vals[0]


@pytest.mark.parametrize("chi", [8, 16])
def test_truncated_ground_state(chi):
    from adaptaqc_amd.mps_operations import mps_to_vector
    from adaptaqc_amd.utils import hamiltonians

    n, ham, scale, vals, ground, _ = _reference("open antiferromagnet n=10")
    lam0, lam1 = vals[0], vals[ground.shape[1]]
    energy, mps = hamiltonians.calculate_ground_state_mps(ham, max_chi=chi, tol=TOL)
    run = hamiltonians.last_run_mps
    psi = np.asarray(mps_to_vector(mps))
    psi = psi / np.linalg.norm(psi)
    hpsi = ref.apply_operator(ham, psi)
    e_np = float(np.vdot(psi, hpsi).real)
    var = float(np.vdot(hpsi, hpsi).real) - e_np * e_np
    print(f"chi {chi}: E - lambda0 {energy - lam0:.3e} (restatement {_truncated_reference(chi):.3e}), sigma^2 {var:.3e} "
          f"(reported {run.variance:.3e}), Temple bound {var / (lam1 - energy):.3e}, sweeps {run.sweeps}")
    assert run.max_bond == chi
    assert energy >= lam0 - 1e-12 * scale
    assert energy < lam1
    assert energy - lam0 <= var / (lam1 - energy)
    assert abs(run.variance - var) <= 1e-11 * scale ** 2


def test_against_the_statevector_solver_sixteen_qubits():
    from adaptaqc_amd.device import DeviceMPS
    from adaptaqc_amd.utils import hamiltonians

    n = 16
    ham = hamiltonians.heisenberg_hamiltonian(n, -1.0, -1.0, -1.0)
    scale = ref.weight(ham)
    e_lanczos, _ = hamiltonians.calculate_ground_state(ham, tol=TOL)
    e_dmrg, mps = hamiltonians.calculate_ground_state_mps(ham, max_chi=64, tol=TOL, return_device=True)
    run = hamiltonians.last_run_mps
    print(f"n=16: E_dmrg - E_lanczos {e_dmrg - e_lanczos:.3e}, sweeps {run.sweeps}, max bond {run.max_bond}, "
          f"variance {run.variance:.3e}")
    assert isinstance(mps, DeviceMPS)
    assert e_dmrg >= e_lanczos - 1e-9 * scale
    labels = list(ham)
    again = float(np.dot([ham[s] for s in labels], mps.pauli_expect(labels)))
    assert abs(again - e_dmrg) <= 1e-10 * scale
    mps.close()


def test_same_seed_same_bits_other_seed_other_state():
    from adaptaqc_amd.utils import hamiltonians

    _, ham, _, _, _, _ = _reference("transverse-field Ising n=8")
    e1, (g1, l1) = hamiltonians.calculate_ground_state_mps(ham, max_chi=16, tol=TOL, seed=3)
    first = hamiltonians.last_run_mps
    e2, (g2, l2) = hamiltonians.calculate_ground_state_mps(ham, max_chi=16, tol=TOL, seed=3)
    assert e1 == e2 and hamiltonians.last_run_mps == first
    for (a0, a1), (b0, b1) in zip(g1, g2):
        assert np.array_equal(a0.view(np.uint64), b0.view(np.uint64)) and np.array_equal(a1.view(np.uint64), b1.view(np.uint64))
    for a, b in zip(l1, l2):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    _, (g3, _) = hamiltonians.calculate_ground_state_mps(ham, max_chi=16, tol=TOL, seed=4)
    assert any(a[0].shape != b[0].shape or not np.array_equal(a[0], b[0]) for a, b in zip(g1, g3))


def test_warm_start_and_unconverged():
    from adaptaqc_amd.utils import hamiltonians

    _, ham, scale, _, _, _ = _reference("transverse-field Ising n=8")
    e1, mps = hamiltonians.calculate_ground_state_mps(ham, max_chi=16, tol=TOL)
    e2, _ = hamiltonians.calculate_ground_state_mps(ham, max_chi=16, tol=TOL, initial_mps=mps)
    print("warm start: sweeps", hamiltonians.last_run_mps.sweeps, "E2 - E1", e2 - e1)
    assert hamiltonians.last_run_mps.sweeps <= 2
    assert e2 <= e1 + 1e-12 * scale
    hamiltonians.last_run_mps = None
    with pytest.raises(RuntimeError, match="still changed"):
        hamiltonians.calculate_ground_state_mps(ham, max_chi=16, tol=TOL, max_sweeps=1)
    assert hamiltonians.last_run_mps.sweeps == 1 and len(hamiltonians.last_run_mps.energies) == 1


def test_initial_circuit_start():
    from adaptaqc_amd.circuit import QuantumCircuit
    from adaptaqc_amd.utils import hamiltonians

    n, ham, scale, vals, _, _ = _reference("antiferromagnet n=6")
    qc = QuantumCircuit(n)
    for q in range(n):
        qc.ry(0.3 + 0.4 * q, q)
    for q in range(n - 1):
        qc.cx(q, q + 1)
    energy, _ = hamiltonians.calculate_ground_state_mps(ham, max_chi=8, tol=TOL, initial_circuit=qc)
    assert -1e-12 * scale <= energy - vals[0] <= TOL * scale


def test_compile_an_mps_ground_state_end_to_end():
    """Hamiltonian -> DMRG ground state (an MPS) -> compile -> energy of the compiled circuit; the
    assertions of test_compile_a_ground_state_end_to_end, with no mps_from_vector in the path."""
    from adaptaqc_amd.backends import AerMPSBackend
    from adaptaqc_amd.backends.aer_sv_backend import AerSVBackend
    from adaptaqc_amd.circuit import device_ops
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig
    from adaptaqc_amd.device import DeviceSV
    from adaptaqc_amd.mps_operations import check_mps, mps_to_vector
    from adaptaqc_amd.utils import hamiltonians
    from adaptaqc_amd.utils.circuit_operations import expectation_value_of_pauli_operator

    n, ham, scale, vals, _, _ = _reference("antiferromagnet n=6")
    e0, target = hamiltonians.calculate_ground_state_mps(ham, max_chi=8, tol=TOL)
    assert check_mps(target)
    gs = np.asarray(mps_to_vector(target))
    comp = AdaptCompiler(target=target, backend=AerMPSBackend(), adapt_config=AdaptConfig(max_layers=4))
    first = comp.evaluate_cost()
    print("first cost", first, "1 - |<0|gs>|^2", 1 - abs(gs[0]) ** 2)
    assert abs(first - (1 - abs(gs[0]) ** 2)) <= 1e-8
    res = comp.compile()
    sol, ground = DeviceSV(n), DeviceSV(n)
    sol.apply(device_ops(res.circuit))
    ground.set(gs)
    overlap = abs(ground.dot(sol)) ** 2
    print("overlap", res.overlap, "recomputed", overlap)
    assert abs(res.overlap - overlap) <= 1e-8
    energy = expectation_value_of_pauli_operator(res.circuit, ham, AerSVBackend())
    print("energy", energy, "E0", e0, "bound", e0 + (1 - overlap) * (vals[-1] - e0))
    assert e0 - 1e-10 * scale <= energy <= e0 + (1 - overlap) * (vals[-1] - e0) + 1e-8 * scale


def test_refusals_leave_the_state_as_it_was():
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.device import DeviceDMRG, DeviceMPS

    n = 6
    ham = _operator(n)
    mps = DeviceMPS(n, 8, 1e-16, 8)
    mps.load_aer(dmrg_ref.product_state(n, 1))
    rng = np.random.default_rng(9)
    mps.apply([(_random_unitary(rng), (q, q + 1)) for q in range(n - 1)])
    before = mps.to_aer()

    def unchanged():
        now = mps.to_aer()
        return all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(before[0], now[0])) and \
            all(np.array_equal(a, b) for a, b in zip(before[1], now[1]))

    for k in (1, 17):
        with pytest.raises(AqcError, match="krylov_dim must be in 2 .. 16"):
            DeviceDMRG(mps, ham, krylov_dim=k)
    with pytest.raises(ValueError, match="characters for 6 qubits"):
        DeviceDMRG(mps, {"ZZ": 1.0})
    with pytest.raises(ValueError, match="real coefficients"):
        DeviceDMRG(mps, {"ZZIIII": 1.0j})
    assert unchanged()
    dm = DeviceDMRG(mps, ham)
    assert unchanged()
    mps.apply([(_random_unitary(rng), (2, 3))])
    before = mps.to_aer()
    with pytest.raises(AqcError, match="changed outside this DMRG handle"):
        dm.sweep()
    with pytest.raises(AqcError, match="changed outside this DMRG handle"):
        dm.heff_apply(0, np.ones(4 * int(mps.dims()[2]), dtype=complex))
    assert unchanged()
    dm.close()
    fresh = DeviceDMRG(mps, ham)  # and a new handle on the changed state is taken
    assert fresh.sweep().shape == (2 * (n - 1),)
    fresh.close()
    mps.close()
