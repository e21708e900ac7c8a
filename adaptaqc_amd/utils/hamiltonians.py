# (C) Copyright IBM 2025.
#
# This code is licensed under the Apache License, Version 2.0. You may
# obtain a copy of this license in the LICENSE.txt file in the root directory
# of this source tree or at http://www.apache.org/licenses/LICENSE-2.0.
#
# Any modifications or derivative works of this code must retain this
# copyright notice, and modified files need to carry a notice indicating
# that they have been altered from the originals.
#
# Modified for adaptaqc_amd: this file restates the reference file named in its docstring
# (qiskit-community/adapt-aqc) on top of the MI355X engine (libaqchip); it has been altered
# from the original.

"""Model Hamiltonians as Pauli-label dicts (reference adaptaqc/utils/hamiltonians.py).

The reference builds OpenFermion ``QubitOperator``s and converts them with
``convert_qubit_op_to_pauli_dict``; here ``heisenberg_hamiltonian`` returns the ``{label: real
coefficient}`` dict that ``expectation_value_of_pauli_operator`` takes directly (labels in qiskit
order: the rightmost character is qubit 0).  The Anderson model (hamiltonians.py:42-77) needs
OpenFermion's Jordan-Wigner transform and is not provided.

``calculate_ground_state`` (hamiltonians.py:80-85, there OpenFermion's sparse eigensolver on the
host) is a Lanczos iteration on device statevectors: the operator apply, the inner products and
the vector updates are libaqchip kernels (csrc/sv_linalg.hip); the host holds the tridiagonal.

``calculate_ground_state_mps`` has no counterpart in the reference: above a statevector's reach the ground
state is found as a matrix-product state by two-site DMRG on the MPS engine (csrc/dmrg.hip), and returned
in the Aer format the compiler takes as a target.
"""
import math
from dataclasses import dataclass

import numpy as np


@dataclass
class GroundStateRun:
    """What the last ``calculate_ground_state`` call did (``last_run``)."""
    energy: float       # <psi|H|psi> of the returned state
    residual: float     # r = |H psi - E psi|, measured on the device
    scale: float        # S = sum_t |c_t|; the call converged to r <= tol * S
    iterations: int     # Lanczos steps (operator applies of the first passes), all restarts together
    restarts: int       # restarts taken after the first run


last_run = None


def _label(n, ops):
    chars = ["I"] * n
    for q, p in ops:
        chars[n - 1 - q] = p
    return "".join(chars)


def heisenberg_hamiltonian(n=4, jx=1.0, jy=0.0, jz=0.0, hx=0.0, hy=0.0, hz=0.0, periodic_bc=False):
    """hamiltonians.py:21-39:
    H = -sum_over_nn(j_x*X_i*X_(i+1) + j_y*Y_i*Y_(i+1) + j_z*Z_i*Z_(i+1)) - sum(h_x*X_i + h_y*Y_i + h_z*Z_i).

    Terms with a zero coefficient are left out (the reference keeps them in its QubitOperator
    until OpenFermion's own simplification); coefficients of a label that occurs twice (the n = 2
    periodic chain) add."""
    n = int(n)
    ham = {}

    def add(label, coeff):
        if coeff == 0:
            return
        ham[label] = ham.get(label, 0.0) + float(coeff)

    for i in range(n if periodic_bc else n - 1):
        j = 0 if (i == n - 1 and periodic_bc) else i + 1
        for p, c in (("X", jx), ("Y", jy), ("Z", jz)):
            add(_label(n, [(i, p), (j, p)]), -c)
    for i in range(n):
        for p, c in (("X", hx), ("Y", hy), ("Z", hz)):
            add(_label(n, [(i, p)]), -c)
    return ham


def _checked_hamiltonian(hamiltonian):
    """(n, xmask, zmask, real coefficients as complex128, S) of a label dict, or ValueError."""
    from .. import paulis

    if not isinstance(hamiltonian, dict) or len(hamiltonian) == 0:
        raise ValueError("calculate_ground_state: the Hamiltonian must be a non-empty {label: coefficient} dict")
    labels = list(hamiltonian.keys())
    n = len(labels[0]) if isinstance(labels[0], str) else 0
    if n < 1 or any(not isinstance(s, str) or len(s) != n for s in labels):
        raise ValueError("calculate_ground_state: every label must be a string of the same length (one letter a qubit)")
    coeffs = np.asarray([complex(v) for v in hamiltonian.values()], dtype=np.complex128)
    if not np.all(np.isfinite(coeffs.real)) or not np.all(np.isfinite(coeffs.imag)):
        raise ValueError("calculate_ground_state: a coefficient is not finite")
    if np.any(coeffs.imag != 0):
        bad = labels[int(np.flatnonzero(coeffs.imag != 0)[0])]
        raise ValueError(f"calculate_ground_state: the coefficient of {bad!r} has an imaginary part; a Hamiltonian "
                         f"(a Hermitian Pauli sum) has real coefficients")
    x, z, c = paulis.operator_to_masks((labels, coeffs), n)
    return n, x, z, c, float(np.sum(np.abs(coeffs)))


def _lowest_ritz(alphas, betas):
    """Lowest eigenpair (theta, s) of the symmetric tridiagonal with diagonal alphas, off-diagonal betas."""
    if len(alphas) == 1:
        return float(alphas[0]), np.ones(1)
    from scipy.linalg import eigh_tridiagonal

    w, v = eigh_tridiagonal(np.asarray(alphas), np.asarray(betas), select="i", select_range=(0, 0),
                            lapack_driver="stemr")
    return float(w[0]), v[:, 0]


def calculate_ground_state(hamiltonian, tol=1e-9, max_iterations=300, max_restarts=5, seed=0, return_device=False):
    """hamiltonians.py:80-85: ``(gs_energy, gs_wf)`` of a Hamiltonian, here the ``{label: real
    coefficient}`` dict ``heisenberg_hamiltonian`` returns (the reference takes a QubitOperator).

    ``gs_wf`` is a normalised complex128 array of 2^n amplitudes whose index bit q is qubit q, this
    package's convention everywhere.  The reference's vector comes from OpenFermion's sparse operator,
    where qubit 0 is the MOST significant bit of the index: reverse the bits of the index to compare.
    With ``return_device`` the state is returned as the ``DeviceSV`` that holds it.

    Lanczos with the three-term recurrence on device vectors, no stored basis.  The start vector is a
    complex Gaussian vector fixed by ``seed`` (complex, so that it has weight in every symmetry sector
    of a real Hamiltonian).  After each step the lowest Ritz pair (theta, s) of the tridiagonal is solved
    on the host, and the run stops at |beta_m s_m| <= tol S, S = sum_t |c_t|, or after ``max_iterations``
    steps.  The Ritz vector is formed by running the recurrence a second time from the same start
    vector (the kernels sum in a fixed order, so the vectors repeat bit for bit).  Then the residual
    r = |H psi - E psi| is measured on the device; while r > tol S the iteration restarts from psi, at most
    ``max_restarts`` times -- this is what answers the recurrence's loss of orthogonality.

    The returned state has r <= tol S, or the call raises ``RuntimeError`` naming r: an unconverged state is
    never returned.  At a degenerate ground level the state is some vector of the ground space.
    ``last_run`` keeps r, the steps and the restarts of the last call.  Four state-sized device buffers."""
    global last_run
    n, x, z, c, scale = _checked_hamiltonian(hamiltonian)
    tol, max_iterations, max_restarts = float(tol), int(max_iterations), int(max_restarts)
    if not tol > 0 or max_iterations < 1 or max_restarts < 0:
        raise ValueError("calculate_ground_state: tol > 0, max_iterations >= 1 and max_restarts >= 0")
    from ..device import DeviceSV

    dim = 1 << n
    steps = min(max_iterations, dim)
    psi, v_prev, v, w = (DeviceSV(n) for _ in range(4))
    rng = np.random.default_rng(seed)
    psi.set(rng.standard_normal(dim) + 1j * rng.standard_normal(dim))
    psi.axpby(1.0 / math.sqrt(psi.dot(psi).real))
    bound = tol * scale
    iterations = 0
    for restart in range(max_restarts + 1):
        # first pass: alpha, beta and the Ritz pair; psi holds the start vector
        v.copy_from(psi)
        alphas, betas = [], []
        while True:
            j = len(alphas)
            v.pauli_apply_masks(x, z, c, w)
            alphas.append(v.dot(w).real)
            w.axpby(1.0, v, -alphas[j])
            if j > 0:
                w.axpby(1.0, v_prev, -betas[j - 1])
            beta = math.sqrt(max(w.dot(w).real, 0.0))
            _, s = _lowest_ritz(alphas, betas)
            if beta * abs(s[-1]) <= bound or j + 1 == steps:
                break
            betas.append(beta)
            v_prev, v, w = v, w, v_prev
            v.axpby(1.0 / beta)
        iterations += len(alphas)
        # second pass: the same vectors again, psi <- sum_j s_j v_j
        v.copy_from(psi)
        psi.axpby(s[0])
        for j in range(len(alphas) - 1):
            v.pauli_apply_masks(x, z, c, w)
            w.axpby(1.0, v, -alphas[j])
            if j > 0:
                w.axpby(1.0, v_prev, -betas[j - 1])
            v_prev, v, w = v, w, v_prev
            v.axpby(1.0 / betas[j])
            psi.axpby(1.0, v, s[j + 1])
        psi.axpby(1.0 / math.sqrt(psi.dot(psi).real))
        # the true residual
        psi.pauli_apply_masks(x, z, c, w)
        energy = psi.dot(w).real
        w.axpby(1.0, psi, -energy)
        residual = math.sqrt(max(w.dot(w).real, 0.0))
        last_run = GroundStateRun(energy=energy, residual=residual, scale=scale, iterations=iterations, restarts=restart)
        if residual <= bound:
            break
    for buf in (v_prev, v, w):
        buf.close()
    if not residual <= bound:
        psi.close()
        raise RuntimeError(f"calculate_ground_state: residual |H psi - E psi| = {residual:.3e} above tol * S = {bound:.3e} "
                           f"after {iterations} Lanczos steps and {max_restarts} restarts")
    if return_device:
        return energy, psi
    out = psi.get()
    psi.close()
    return energy, out


# ---- matrix-product ground states: two-site DMRG on the MPS engine --------------------------------------
@dataclass
class GroundStateMPSRun:
    """What the last ``calculate_ground_state_mps`` call did (``last_run_mps``)."""
    energy: float      # sum_t c_t <P_t> of the returned state
    energies: list     # the same after every sweep
    sweeps: int
    max_bond: int      # the largest bond dimension of the returned state
    scale: float       # S = sum_t |c_t|; the call converged to |E - E_prev| <= tol * S
    variance: float    # sigma^2 = <H^2> - E^2, resolved to about 1e-11 S^2 (see calculate_ground_state_mps)
    breakdowns: int    # bond updates whose Lanczos iteration ended early (aqc_dmrg_stats)
    updates: int       # bond updates


last_run_mps = None


def _squared_operator(codes, coeffs):
    """H^2 of H = sum_t c_t P_t as (codes, real coefficients), its label products formed on the host:
    with P = i^{|x & z|} X^x Z^z, P_a P_b = i^{ny_a + ny_b - ny_ab} (-1)^{|z_a & x_b|} P_ab.  Products of
    the same string are added; the anticommuting pairs cancel, and what is left is real."""
    x = (codes == 1) | (codes == 2)
    z = (codes == 3) | (codes == 2)
    ny = np.sum(x & z, axis=1)
    total = {}
    for a in range(len(codes)):
        xa = x[a][None, :] ^ x
        za = z[a][None, :] ^ z
        k = (ny[a] + ny - np.sum(xa & za, axis=1) + 2 * np.sum(z[a][None, :] & x, axis=1)) % 4
        prod = np.where(xa & za, 2, np.where(xa, 1, np.where(za, 3, 0))).astype(np.uint8)
        w = coeffs[a] * coeffs * np.array([1, 1j, -1, -1j])[k]
        for b in range(len(codes)):
            key = prod[b].tobytes()
            total[key] = total.get(key, 0.0) + w[b]
    keys = [k for k, v in total.items() if v.real != 0.0]
    out = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(len(keys), codes.shape[1])
    return np.ascontiguousarray(out), np.array([total[k].real for k in keys])


def calculate_ground_state_mps(hamiltonian, max_chi=64, threshold=1e-16, tol=1e-9, max_sweeps=30, krylov_dim=6, seed=0,
                               initial_circuit=None, initial_mps=None, return_device=False):
    """``(energy, mps)``: the ground state of a ``{label: real coefficient}`` Hamiltonian as a
    matrix-product state, by two-site DMRG (density-matrix renormalisation group) on the MPS engine --
    ``calculate_ground_state`` beyond a statevector's reach.  ``mps`` is the Aer-format MPS
    (``DeviceMPS.to_aer()``) that ``AdaptCompiler(target=...)`` takes directly; with ``return_device`` it is
    the ``DeviceMPS`` that holds it.

    The start state is, by default, a product state with ``ry`` / ``rz`` angles drawn from ``seed`` on every
    qubit -- it has weight in every S_z sector, and a two-site update cannot leave a symmetry sector that
    the start lacks; otherwise ``initial_circuit`` run on the engine, or the Aer-format ``initial_mps``.
    A sweep updates the bonds 0 .. n - 2 left to right, then back (``DeviceDMRG.sweep``): each update is a
    Lanczos iteration of ``krylov_dim`` steps on the bond's effective Hamiltonian and the engine's SVD
    with the truncation (``max_chi``, ``threshold``).  After every sweep the energy is the state's own,
    E = sum_t c_t <P_t> from ``pauli_expect`` (truncation moves it off the last Ritz value), and the call
    stops at |E - E_prev| <= tol S, S = sum_t |c_t|.  If that has not happened after ``max_sweeps`` the call
    raises ``RuntimeError`` naming the last change: an unconverged state is never returned.

    ``last_run_mps`` keeps the energies, the sweeps, the largest bond and the variance sigma^2 = <H^2> - E^2
    (the label products of H^2 formed on the host, read by one ``pauli_expect`` call).  sigma^2 is resolved
    only to about 1e-11 S^2 -- the per-term accuracy of the MPS Pauli reader times sum |c_a c_b| -- so it is
    a report, not a stopping rule.  Labels are limited to 64 qubits by ``_checked_hamiltonian``."""
    global last_run_mps
    n, _, _, c, scale = _checked_hamiltonian(hamiltonian)
    if n < 2:
        raise ValueError("calculate_ground_state_mps: a two-site update needs at least 2 qubits")
    tol, max_sweeps, max_chi, krylov_dim = float(tol), int(max_sweeps), int(max_chi), int(krylov_dim)
    if not tol > 0 or max_sweeps < 1 or max_chi < 1 or not float(threshold) >= 0:
        raise ValueError("calculate_ground_state_mps: tol > 0, max_sweeps >= 1, max_chi >= 1 and threshold >= 0")
    if not 2 <= krylov_dim <= 16:
        raise ValueError("calculate_ground_state_mps: krylov_dim must be in 2 .. 16")
    if initial_circuit is not None and initial_mps is not None:
        raise ValueError("calculate_ground_state_mps: give initial_circuit or initial_mps, not both")
    from .. import paulis
    from ..device import DeviceDMRG, DeviceMPS

    labels = list(hamiltonian.keys())
    coeffs = c.real.copy()
    codes = paulis.terms_to_codes(labels, n)
    cap = min(max_chi, 1 << (n // 2), 1024)
    if initial_mps is not None:
        gam, _ = initial_mps
        if len(gam) != n:
            raise ValueError(f"calculate_ground_state_mps: initial_mps has {len(gam)} sites for {n} qubits")
        cap = max(cap, max(int(np.asarray(g[0]).shape[1]) for g in gam))
    mps = DeviceMPS(n, cap, float(threshold), max_chi)
    try:
        if initial_mps is not None:
            mps.load_aer(initial_mps)
        elif initial_circuit is not None:
            from ..circuit import device_ops

            if initial_circuit.num_qubits != n:
                raise ValueError(f"calculate_ground_state_mps: initial_circuit has {initial_circuit.num_qubits} qubits for {n}")
            mps.apply(device_ops(initial_circuit))
        else:
            rng = np.random.default_rng(seed)
            ops = []
            for q in range(n):
                t, p = rng.uniform(0.0, math.pi), rng.uniform(0.0, 2.0 * math.pi)
                ry = np.array([[math.cos(t / 2), -math.sin(t / 2)], [math.sin(t / 2), math.cos(t / 2)]], dtype=complex)
                rz = np.diag([np.exp(-0.5j * p), np.exp(0.5j * p)])
                ops.append((rz @ ry, (q,)))
            mps.apply(ops)
        dm = DeviceDMRG(mps, (codes, coeffs), krylov_dim)
        try:
            energies = []
            change = math.inf
            for _ in range(max_sweeps):
                dm.sweep()
                energies.append(float(np.dot(coeffs, mps.pauli_expect(codes))))
                if len(energies) > 1:
                    change = abs(energies[-1] - energies[-2])
                    if change <= tol * scale:
                        break
            energy = energies[-1]
            sq_codes, sq_coeffs = _squared_operator(codes, coeffs)
            variance = float(np.dot(sq_coeffs, mps.pauli_expect(sq_codes))) - energy * energy
            stats = dm.stats()
        finally:
            dm.close()
        last_run_mps = GroundStateMPSRun(energy=energy, energies=energies, sweeps=len(energies),
                                         max_bond=int(mps.dims().max()), scale=scale, variance=variance,
                                         breakdowns=stats["breakdowns"], updates=stats["updates"])
        if not change <= tol * scale:
            raise RuntimeError(f"calculate_ground_state_mps: the energy still changed by {change:.3e}, above tol * S = "
                               f"{tol * scale:.3e}, in the last of {max_sweeps} sweeps")
    except BaseException:
        mps.close()
        raise
    if return_device:
        return energy, mps
    out = mps.to_aer()
    mps.close()
    return energy, out
