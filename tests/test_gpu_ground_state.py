"""Device Lanczos ground states on MI355X: aqc_sv_pauli_apply / aqc_sv_dot / aqc_sv_axpby against the numpy
restatement (pauli_apply_ref), calculate_ground_state against numpy's spectra, and a ground state
compiled end to end.

Bounds.  An output amplitude of the apply is a sum of at most T products, so its rounding is about
(T + 2) 2^-53 S max|psi| with S = sum_t |c_t| (3e-14 S max|psi| at T = 300): the entrywise bound
1e-12 S max|psi| leaves a factor 30.  The ground states run at tol = 1e-9, four orders above that
floor; every case first asserts, on numpy's spectrum alone, that its gap exceeds 100 tol S."""
import functools

import numpy as np
import pytest

import pauli_apply_ref as ref

pytestmark = pytest.mark.gpu

TOL = 1e-9
CHUNK_WORDS = 768  # 16-byte table words of one staged chunk: a group is 1 + 2 terms words
GROUP_TERMS = 383  # terms of one record


def _state(n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)


def _random_terms(n, nterms, nx, seed, complex_coeffs=False, diagonal=False):
    """nterms terms over nx distinct x masks (x = 0 only when diagonal), random z masks."""
    rng = np.random.default_rng(seed)
    dim = 1 << n
    xs = np.zeros(1, dtype=np.uint64) if diagonal else rng.choice(dim, size=nx, replace=False).astype(np.uint64)
    x = xs[rng.integers(0, len(xs), nterms)]
    x[: len(xs)] = xs  # every mask occurs
    z = rng.integers(0, dim, nterms).astype(np.uint64)
    c = rng.normal(size=nterms) + (1j * rng.normal(size=nterms) if complex_coeffs else 0)
    return x, z, c.astype(np.complex128)


def _label_terms(op, n):
    from adaptaqc_amd import paulis

    return paulis.operator_to_masks(op, n)


def _cases(n):
    """name -> ((x, z, c), timer family that must run)."""
    from adaptaqc_amd.utils.hamiltonians import heisenberg_hamiltonian

    top = n - 1
    one = "sv_pauli_apply"
    cases = {}
    for p in "XYZ":
        cases[f"single {p} on qubit {top}"] = (_label_terms({p + "I" * top: 0.7}, n), one)
    cases["identity alone"] = (_label_terms({"I" * n: -1.25}, n), one)
    cases["diagonal only"] = (_random_terms(n, 7, 1, 40 + n, diagonal=True), one)
    cases["complex coefficients"] = (_random_terms(n, 6, min(3, 1 << n), 50 + n, complex_coeffs=True), one)
    if n >= 3:
        cases["Y on three qubits"] = (_label_terms({"Y" + "I" * (n - 3) + "YY": 1.5}, n), one)
        cases["40 terms over 5 x masks"] = (_random_terms(n, 40, 5, 60 + n), one)
        cases["periodic Heisenberg chain"] = (
            _label_terms(heisenberg_hamiltonian(n, -1.0, 0.5, 0.25, hz=0.3, periodic_bc=True), n), one)
    if n >= 9:
        # 300 groups of one term: 900 words, two chunks; 400 diagonal terms: two records of one group
        cases["more groups than a chunk"] = (_random_terms(n, 300, 300, 70 + n), "sv_pauli_apply_chunks")
        cases["a group longer than a record"] = (_random_terms(n, 400, 1, 80 + n, diagonal=True),
                                                 "sv_pauli_apply_chunks")
    return cases


def _run_apply(n, terms, psi, family):
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import DeviceSV

    x, z, c = terms
    a, b = DeviceSV(n), DeviceSV(n)
    a.set(psi)
    _lib.timing_enable(True)
    _lib.timing_reset()
    try:
        a.pauli_apply_masks(x, z, c, b)
        ran = {f: _lib.timing_query(f)["launches"] for f in ("sv_pauli_apply", "sv_pauli_apply_chunks")}
    finally:
        _lib.timing_enable(False)
    assert ran[family] == 1 and sum(ran.values()) == 1, ran
    assert np.array_equal(a.get(), psi)  # the input is not changed
    return b.get()


@pytest.mark.parametrize("n", [1, 5, 6, 9, 13])
def test_pauli_apply_matches_restatement(n):
    """n = 1, 5: fewer amplitudes than a wave; 6: one wave; 9: two workgroups; 13: 32 workgroups."""
    psi = _state(n, n)
    cases = _cases(n)
    assert ("more groups than a chunk" in cases) == (n >= 9)
    assert 300 * 3 > CHUNK_WORDS and 400 > GROUP_TERMS
    for name, (terms, family) in cases.items():
        got = _run_apply(n, terms, psi, family)
        want = ref.apply_masks(*terms, psi)
        bound = 1e-12 * float(np.sum(np.abs(terms[2]))) * np.max(np.abs(psi))
        err = np.max(np.abs(got - want))
        print(f"n={n} {name}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, name
        assert np.max(np.abs(want)) > 0


def test_pauli_apply_grid_stride():
    """The grid is bounded at 2048 workgroups of 256 threads: from 2^20 amplitudes a thread owns more
    than one, on the one-chunk path and on the chunked one (which restages per amplitude)."""
    n = 20
    psi = _state(n, 20)
    for terms, family in ((_random_terms(n, 12, 4, 21, complex_coeffs=True), "sv_pauli_apply"),
                          (_random_terms(n, 258, 258, 22), "sv_pauli_apply_chunks")):
        got = _run_apply(n, terms, psi, family)
        # the restatement on a slice of the outputs spread over the whole index range and on the last block
        idx = np.concatenate([np.arange(0, 1 << n, 4099), np.arange((1 << n) - 300, 1 << n)]).astype(np.uint64)
        want = np.zeros(len(idx), dtype=complex)
        for x, z, c in zip(*terms):
            k = idx ^ x
            par = np.array([bin(int(v)).count("1") & 1 for v in (k & z)])
            want += c * (1, 1j, -1, -1j)[bin(int(x & z)).count("1") & 3] * np.where(par, -1.0, 1.0) * psi[k.astype(np.int64)]
        bound = 1e-12 * float(np.sum(np.abs(terms[2]))) * np.max(np.abs(psi))
        err = np.max(np.abs(got[idx.astype(np.int64)] - want))
        print(f"n={n} {family}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound


def test_pauli_apply_label_forms_and_expectation_cross_check():
    """No dense oracle at n = 20: Re <psi|H psi> from apply and dot equals sum_t c_t <P_t> from
    aqc_sv_pauli_expect on the same open Heisenberg chain, to 1e-11 S."""
    from adaptaqc_amd.device import DeviceSV
    from adaptaqc_amd.utils.hamiltonians import heisenberg_hamiltonian

    n = 20
    ham = heisenberg_hamiltonian(n, -1.0, -1.0, -1.0)
    psi = _state(n, 7)
    psi /= np.linalg.norm(psi)
    a, b = DeviceSV(n), DeviceSV(n)
    a.set(psi)
    a.pauli_apply(ham, b)
    via_apply = a.dot(b)
    labels = list(ham)
    via_expect = float(np.dot([ham[s] for s in labels], a.pauli_expect(labels)))
    print("Re <psi|H psi>", via_apply.real, "sum c <P>", via_expect, "Im", via_apply.imag)
    assert abs(via_apply.real - via_expect) <= 1e-11 * ref.weight(ham)
    assert abs(via_apply.imag) <= 1e-11 * ref.weight(ham)  # H is Hermitian
    # (terms, coeffs) is the same operator
    c = DeviceSV(n)
    a.pauli_apply((labels, [ham[s] for s in labels]), c)
    assert np.array_equal(b.get(), c.get())


def test_pauli_apply_repeats_bit_for_bit_and_zero_terms():
    from adaptaqc_amd.device import DeviceSV

    n = 13
    psi = _state(n, 31)
    terms = _random_terms(n, 300, 300, 32, complex_coeffs=True)
    a, b, c = DeviceSV(n), DeviceSV(n), DeviceSV(n)
    a.set(psi)
    a.pauli_apply_masks(*terms, b)
    a.pauli_apply_masks(*terms, c)
    first = b.get()
    assert np.array_equal(first.view(np.uint64), c.get().view(np.uint64))
    a.pauli_apply_masks(*terms, b)  # into a buffer that holds an old result
    assert np.array_equal(first.view(np.uint64), b.get().view(np.uint64))
    a.pauli_apply_masks([], [], [], b)
    assert np.array_equal(b.get(), np.zeros(1 << n))
    # from 14 qubits a new state's reset is deferred: both sides of the apply in that condition
    m = 14
    fresh, out = DeviceSV(m), DeviceSV(m)
    fresh.pauli_apply({"I" * (m - 1) + "X": 2.0}, out)
    want = np.zeros(1 << m, dtype=complex)
    want[1] = 2.0
    assert np.array_equal(out.get(), want)
    assert fresh.amp0() == 1.0


def test_pauli_apply_refusals_leave_out_untouched():
    from adaptaqc_amd import _lib
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.device import DeviceSV

    n = 5
    psi, old = _state(n, 1), _state(n, 2)
    a, out, other = DeviceSV(n), DeviceSV(n), DeviceSV(n + 1)
    a.set(psi)
    out.set(old)
    x, z, c = _random_terms(n, 4, 2, 3)
    lib = _lib.lib()
    err_arg = -1

    def raw(h_in, h_out, nterms):
        return lib.aqc_sv_pauli_apply(h_in, h_out, _lib.ptr(x), _lib.ptr(z), _lib.ptr(c), nterms)

    assert raw(None, out.h, 4) == err_arg and b"null handle" in lib.aqc_last_error()
    assert raw(a.h, None, 4) == err_arg and b"null handle" in lib.aqc_last_error()
    assert raw(a.h, out.h, (1 << 20) + 1) == err_arg and b"nterms" in lib.aqc_last_error()
    assert raw(a.h, out.h, -1) == err_arg and b"nterms" in lib.aqc_last_error()
    with pytest.raises(AqcError, match="different states"):
        out.pauli_apply_masks(x, z, c, out)
    with pytest.raises(AqcError, match="different qubit counts"):
        other.pauli_apply_masks(x, z, c, out)
    for bad in ((x | np.uint64(1 << n), z), (x, z | np.uint64(1 << (n + 3)))):
        with pytest.raises(AqcError, match="mask bit at or above n"):
            a.pauli_apply_masks(bad[0], bad[1], c, out)
    for value in (np.nan, np.inf, 1j * np.inf):
        cc = c.copy()
        cc[2] = value
        with pytest.raises(AqcError, match="not finite"):
            a.pauli_apply_masks(x, z, cc, out)
    assert np.array_equal(out.get(), old)
    assert np.array_equal(a.get(), psi)
    a.pauli_apply_masks(x, z, c, out)  # and the same arguments unspoilt are taken
    assert np.max(np.abs(out.get() - ref.apply_masks(x, z, c, psi))) <= 1e-12 * np.sum(np.abs(c)) * np.max(np.abs(psi))


@pytest.mark.parametrize("n", [1, 6, 9, 13])
def test_dot_and_axpby(n):
    """n = 9: a thread sums two amplitudes; n = 13: two workgroups' partials."""
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.device import DeviceSV

    u, v = _state(n, 100 + n), _state(n, 200 + n)
    a, b = DeviceSV(n), DeviceSV(n)
    a.set(u)
    b.set(v)
    got = a.dot(b)
    bound = 1e-13 * np.linalg.norm(u) * np.linalg.norm(v)
    print(f"n={n} dot error {abs(got - np.vdot(u, v)):.3e}, bound {bound:.3e}")
    assert abs(got - np.vdot(u, v)) <= bound
    assert got == a.dot(b)  # the same bits
    assert abs(a.dot(a) - np.vdot(u, u)) <= 1e-13 * np.linalg.norm(u) ** 2
    assert abs(b.dot(a) - np.conj(np.vdot(u, v))) <= bound
    big = max(np.max(np.abs(u)), np.max(np.abs(v)))
    alpha, beta = 0.75 - 1.5j, -0.3 + 0.2j
    a.axpby(alpha, b, beta)
    want = alpha * u + beta * v
    err = np.max(np.abs(a.get() - want))
    print(f"n={n} axpby error {err:.3e}, bound {1e-14 * (abs(alpha) + abs(beta)) * big:.3e}")
    assert err <= 1e-14 * (abs(alpha) + abs(beta)) * big
    assert np.array_equal(b.get(), v)
    # a pure scale, with no x and with an x that is not read
    a.set(u)
    a.axpby(alpha)
    assert np.max(np.abs(a.get() - alpha * u)) <= 1e-14 * abs(alpha) * big
    scaled = a.get()
    a.set(u)
    a.axpby(alpha, b, 0.0)
    assert np.array_equal(a.get(), scaled)
    a.axpby(2.0, b, 1.0)
    assert np.max(np.abs(a.get() - (2.0 * scaled + v))) <= 1e-14 * 3.0 * max(big, np.max(np.abs(scaled)))
    # refusals leave y as it is
    a.set(u)
    with pytest.raises(AqcError, match="different states"):
        a.axpby(1.0, a, 1.0)
    with pytest.raises(AqcError, match="null x"):
        a.axpby(1.0, None, 1.0)
    with pytest.raises(AqcError, match="not finite"):
        a.axpby(np.nan, b, 1.0)
    with pytest.raises(AqcError, match="different qubit counts"):
        a.axpby(1.0, DeviceSV(n + 1), 1.0)
    with pytest.raises(AqcError, match="different qubit counts"):
        a.dot(DeviceSV(n + 1))
    assert np.array_equal(a.get(), u)


# ---- ground states -----------------------------------------------------------------------------
def _heisenberg(n, **kw):
    from adaptaqc_amd.utils.hamiltonians import heisenberg_hamiltonian

    return heisenberg_hamiltonian(n, **kw)


HAMILTONIANS = {
    "antiferromagnet n=2": (2, dict(jx=-1.0, jy=-1.0, jz=-1.0)),
    "transverse-field Ising n=8": (8, dict(jx=0.0, jz=1.0, hx=0.7)),
    "ferromagnet n=4": (4, dict(jx=1.0, jy=1.0, jz=1.0)),
    "antiferromagnet n=6": (6, dict(jx=-1.0, jy=-1.0, jz=-1.0)),
    "open antiferromagnet n=10": (10, dict(jx=-1.0, jy=-1.0, jz=-1.0)),
}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(n, ham, S, eigenvalues, ground-space basis, gap) from numpy's eigh; the ground space is the
    eigenvalues within 1e-10 S of the lowest."""
    n, kw = HAMILTONIANS[name]
    ham = _heisenberg(n, **kw)
    scale = ref.weight(ham)
    vals, vecs = ref.spectrum(ham, n)
    ground = vals <= vals[0] + 1e-10 * scale
    gap = float(vals[np.count_nonzero(ground)] - vals[0])
    assert gap > 100 * TOL * scale  # a condition on the inputs, from the reference alone
    return n, ham, scale, vals, vecs[:, ground], gap


def _solve_and_check(name, degeneracy, **kw):
    from adaptaqc_amd.utils import hamiltonians

    n, ham, scale, vals, ground, gap = _reference(name)
    assert ground.shape[1] == degeneracy
    energy, psi = hamiltonians.calculate_ground_state(ham, tol=TOL, **kw)
    run = hamiltonians.last_run
    print(f"{name}: E {energy!r} lambda0 {vals[0]!r} r {run.residual:.3e} tol S {TOL * scale:.3e} gap {gap:.4f} "
          f"steps {run.iterations} restarts {run.restarts}")
    assert psi.shape == (1 << n,) and psi.dtype == np.complex128
    assert abs(np.linalg.norm(psi) - 1.0) <= 1e-13  # (the norm's own sum rounds at 2^-53 log2(2^n))
    assert run.energy == energy and run.scale == scale
    r = run.residual
    assert r <= TOL * scale
    # the residual is the state's own: numpy on the returned vector
    assert abs(np.linalg.norm(ref.apply_operator(ham, psi) - energy * psi) - r) <= 1e-12 * scale
    assert -1e-12 * scale <= energy - vals[0] <= TOL * scale
    inside = float(np.sum(np.abs(ground.conj().T @ psi) ** 2))
    print(f"{name}: 1 - |P psi|^2 = {1 - inside:.3e}, bound {(r / (gap - r)) ** 2 + 1e-12:.3e}")
    assert 1 - inside <= (r / (gap - r)) ** 2 + 1e-12  # the sin(theta) bound
    return energy, psi, run


def test_ground_state_two_qubit_singlet():
    energy, psi, _ = _solve_and_check("antiferromagnet n=2", 1)
    assert abs(energy + 3.0) <= 1e-9 * 3.0
    singlet = np.array([0, 1, -1, 0]) / np.sqrt(2)
    assert 1 - abs(np.vdot(singlet, psi)) ** 2 <= 1e-12


def test_ground_state_transverse_field_ising():
    _solve_and_check("transverse-field Ising n=8", 1)


def test_ground_state_degenerate_ferromagnet():
    energy, _, _ = _solve_and_check("ferromagnet n=4", 5)
    assert abs(energy + 3.0) <= 1e-9 * 9.0


def test_ground_state_open_chain_ten_qubits():
    _solve_and_check("open antiferromagnet n=10", 1)


def test_ground_state_restarts():
    """Twelve steps a run do not reach tol: the restarts from the Ritz vector do."""
    _, _, run = _solve_and_check("antiferromagnet n=6", 1, max_iterations=12, max_restarts=60)
    assert run.restarts >= 1 and run.iterations > 12


def test_ground_state_same_seed_same_bits_and_device_result():
    from adaptaqc_amd.device import DeviceSV
    from adaptaqc_amd.utils import hamiltonians

    _, ham, _, _, _, _ = _reference("transverse-field Ising n=8")
    e1, p1 = hamiltonians.calculate_ground_state(ham, tol=TOL, seed=3)
    first = hamiltonians.last_run
    e2, p2 = hamiltonians.calculate_ground_state(ham, tol=TOL, seed=3)
    assert e1 == e2 and np.array_equal(p1.view(np.uint64), p2.view(np.uint64))
    assert hamiltonians.last_run == first
    e3, dev = hamiltonians.calculate_ground_state(ham, tol=TOL, seed=3, return_device=True)
    assert isinstance(dev, DeviceSV) and e3 == e1
    assert np.array_equal(dev.get().view(np.uint64), p1.view(np.uint64))
    _, p4 = hamiltonians.calculate_ground_state(ham, tol=TOL, seed=4)
    assert not np.array_equal(p4, p1)  # another start vector


def test_ground_state_unconverged_raises():
    from adaptaqc_amd.utils import hamiltonians

    _, ham, scale, _, _, _ = _reference("transverse-field Ising n=8")
    with pytest.raises(RuntimeError, match="residual"):
        hamiltonians.calculate_ground_state(ham, tol=TOL, max_iterations=3, max_restarts=0)
    assert hamiltonians.last_run.residual > TOL * scale and hamiltonians.last_run.iterations == 3


# ---- end to end --------------------------------------------------------------------------------
def test_compile_a_ground_state_end_to_end():
    """Hamiltonian -> ground state -> MPS target -> compile -> energy of the compiled circuit.  No
    convergence threshold: the compiler's numbers are recomputed from the ground state."""
    from adaptaqc_amd.backends import AerMPSBackend
    from adaptaqc_amd.backends.aer_sv_backend import AerSVBackend
    from adaptaqc_amd.circuit import device_ops
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig
    from adaptaqc_amd.device import DeviceSV
    from adaptaqc_amd.mps_operations import check_mps, mps_from_vector
    from adaptaqc_amd.utils import hamiltonians
    from adaptaqc_amd.utils.circuit_operations import expectation_value_of_pauli_operator

    n, ham, scale, vals, _, _ = _reference("antiferromagnet n=6")
    e0, gs = hamiltonians.calculate_ground_state(ham, tol=TOL)
    target = mps_from_vector(gs)
    assert check_mps(target)
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
