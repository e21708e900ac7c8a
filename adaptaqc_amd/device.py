"""Owning Python wrappers around libaqchip handles (device-resident statevector / MPS)."""
import ctypes

import numpy as np

from . import _lib


class DeviceSV:
    """2^n complex128 amplitudes resident in HBM (Aer statevector_simulator state)."""

    def __init__(self, n):
        self._l = _lib.lib()
        self.n = int(n)
        h = ctypes.c_void_p()
        _lib.check(self._l.aqc_sv_create(self.n, ctypes.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self._l.aqc_sv_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self):
        _lib.check(self._l.aqc_sv_reset(self.h))

    def copy_from(self, other):
        _lib.check(self._l.aqc_sv_copy(self.h, other.h))

    def apply(self, ops):
        if len(ops) == 0:
            return
        arr = ops if isinstance(ops, np.ndarray) else _lib.ops_array(ops)
        _lib.check(self._l.aqc_sv_apply(self.h, _lib.ptr(arr), len(arr)))

    def amp0(self):
        re, im = ctypes.c_double(), ctypes.c_double()
        _lib.check(self._l.aqc_sv_amp0(self.h, ctypes.byref(re), ctypes.byref(im)))
        return complex(re.value, im.value)

    def z_all(self):
        out = np.zeros(self.n)
        _lib.check(self._l.aqc_sv_z_all(self.h, _lib.dptr(out)))
        return out

    def transition(self, ket, q):
        """2x2 T[a][b] = <self| (|a><b|)_q |ket> (cached Rotoselect / Rotosolve)."""
        out = np.zeros(4, dtype=np.complex128)
        _lib.check(self._l.aqc_sv_transition(self.h, ket.h, int(q), _lib.ptr(out)))
        return out.reshape(2, 2)

    def pair_rdms(self, pairs):
        """4x4 reduced density matrices of qubit pairs (entanglement_measures.py:326-340)."""
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1))
        out = np.zeros(len(pairs) // 2 * 16, dtype=np.complex128)
        if len(pairs):
            _lib.check(self._l.aqc_sv_pair_rdms(self.h, _lib.ptr(pairs), len(pairs) // 2, _lib.ptr(out)))
        return out.reshape(-1, 4, 4)

    def sample(self, shots, seed, run=0, u=None):
        """``shots`` measurement outcomes of all qubits (aqc_sv_sample): uint64[shots] basis
        indices (bit q = qubit q).  ``u``: shots uniforms in [0, 1) used instead of the generator's."""
        shots = int(shots)
        out = np.zeros(max(shots, 0), dtype=np.uint64)
        up = _uniforms_arg(u, (shots,))
        _lib.check(self._l.aqc_sv_sample(self.h, shots, _u64(seed), _u64(run), _lib.ptr(up), _lib.ptr(out)))
        return out

    def pauli_expect(self, terms):
        """Re <psi|P_t|psi> of every Pauli string in one launch (aqc_sv_pauli_expect).  ``terms``: a
        list of qiskit labels (rightmost character = qubit 0) or an (nterms, n) uint8 code array
        (0 I, 1 X, 2 Y, 3 Z; column q = qubit q)."""
        from . import paulis

        x, z = paulis.codes_to_masks(paulis.terms_to_codes(terms, self.n))
        return self.pauli_expect_masks(x, z)

    def pauli_expect_masks(self, xmask, zmask):
        """The same from bit masks (bit q = qubit q; a qubit in both masks is Y)."""
        x = np.ascontiguousarray(xmask, dtype=np.uint64).reshape(-1)
        z = np.ascontiguousarray(zmask, dtype=np.uint64).reshape(-1)
        if len(x) != len(z):
            raise ValueError("pauli_expect_masks: one x and one z mask per term")
        out = np.zeros(len(x))
        _lib.check(self._l.aqc_sv_pauli_expect(self.h, _lib.ptr(x), _lib.ptr(z), len(x), _lib.ptr(out)))
        return out

    def pauli_apply(self, operator, out):
        """out <- sum_t c_t P_t self (aqc_sv_pauli_apply); self is not changed.  ``operator``: a
        ``{label: coefficient}`` dict (qiskit labels, rightmost character = qubit 0) or ``(terms,
        coeffs)`` with terms as ``pauli_expect`` takes them.  ``out``: another DeviceSV on as many qubits."""
        from . import paulis

        x, z, c = paulis.operator_to_masks(operator, self.n)
        return self.pauli_apply_masks(x, z, c, out)

    def pauli_apply_masks(self, xmask, zmask, coeffs, out):
        """The same from bit masks and complex coefficients."""
        x = np.ascontiguousarray(xmask, dtype=np.uint64).reshape(-1)
        z = np.ascontiguousarray(zmask, dtype=np.uint64).reshape(-1)
        c = np.ascontiguousarray(coeffs, dtype=np.complex128).reshape(-1)
        if not len(x) == len(z) == len(c):
            raise ValueError("pauli_apply_masks: one x mask, z mask and coefficient per term")
        _lib.check(self._l.aqc_sv_pauli_apply(self.h, out.h if out is not None else None, _lib.ptr(x), _lib.ptr(z),
                                              _lib.ptr(c), len(x)))
        return out

    def dot(self, other):
        """<self|other> = sum_k conj(self_k) other_k, summed in a fixed order (aqc_sv_dot)."""
        out = np.zeros(2)
        _lib.check(self._l.aqc_sv_dot(self.h, other.h if other is not None else None, _lib.dptr(out)))
        return complex(out[0], out[1])

    def axpby(self, a, x=None, b=0.0):
        """self <- a self + b x (aqc_sv_axpby); with b = 0, x may be None: a pure scale."""
        a, b = complex(a), complex(b)
        _lib.check(self._l.aqc_sv_axpby(self.h, a.real, a.imag, x.h if x is not None else None, b.real, b.imag))

    def get(self):
        out = np.zeros(2 ** self.n, dtype=np.complex128)
        _lib.check(self._l.aqc_sv_get(self.h, _lib.ptr(out)))
        return out

    def set(self, psi):
        psi = np.ascontiguousarray(psi, dtype=np.complex128)
        _lib.check(self._l.aqc_sv_set(self.h, _lib.ptr(psi)))


class DeviceDM:
    """The density matrix of n <= 13 qubits resident in HBM (csrc/dm.hip): 4^n complex128, entry (r, c) at
    r + (c << n).  What Aer's ``method="density_matrix"`` holds: one deterministic evolution of a noisy
    program gives the exact cost, RDMs, Pauli values and outcome distribution that the trajectory
    samplers estimate from shots."""

    MAX_QUBITS = 13

    def __init__(self, n):
        self._l = _lib.lib()
        self.n = int(n)
        h = ctypes.c_void_p()
        _lib.check(self._l.aqc_dm_create(self.n, ctypes.byref(h)))
        self.h = h
        self._diag = None  # the diagonal as a DeviceSV, made on first use
        self._diag_valid = False

    def close(self):
        if getattr(self, "_diag", None) is not None:
            self._diag.close()
            self._diag = None
        if getattr(self, "h", None) is not None and self.h.value:
            self._l.aqc_dm_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self):
        """rho = |0...0><0...0|."""
        self._diag_valid = False
        _lib.check(self._l.aqc_dm_reset(self.h))

    def run(self, rows):
        """Evolves rho by the program ``rows`` (noise.trajectory_program; aqc_dm_apply): gate rows as
        U rho U^dag, Kraus rows and groups as sum_k K_k rho K_k^dag.  Returns when it is done."""
        rows = np.ascontiguousarray(rows, dtype=_lib.OP_DTYPE)
        self._diag_valid = False
        _lib.check(self._l.aqc_dm_apply(self.h, _lib.ptr(rows) if len(rows) else None, len(rows)))

    def run_adjoint(self, rows):
        """X <- Lambda^dag(X) for the map Lambda of ``run(rows)`` (aqc_dm_apply_adjoint): the program in
        reverse, gate rows as U^dag X U, Kraus rows and groups as sum_k K_k^dag X K_k -- an observable
        pushed backwards through the program.  Tr(X^H Lambda(rho)) = Tr(Lambda^dag(X)^H rho)."""
        rows = np.ascontiguousarray(rows, dtype=_lib.OP_DTYPE)
        self._diag_valid = False
        _lib.check(self._l.aqc_dm_apply_adjoint(self.h, _lib.ptr(rows) if len(rows) else None, len(rows)))

    def get(self):
        """rho as a [2^n, 2^n] complex array (index bit q = qubit q)."""
        dim = 2 ** self.n
        out = np.zeros(dim * dim, dtype=np.complex128)
        _lib.check(self._l.aqc_dm_get(self.h, _lib.ptr(out)))
        return np.ascontiguousarray(out.reshape(dim, dim).T)  # entry (r, c) at r + (c << n)

    def set(self, x):
        """Uploads a [2^n, 2^n] complex array with ``get``'s convention: any matrix, Hermitian or not."""
        dim = 2 ** self.n
        x = np.asarray(x, dtype=np.complex128)
        if x.shape != (dim, dim):
            raise ValueError(f"set: the matrix must have shape {(dim, dim)}")
        flat = np.ascontiguousarray(x.T).reshape(-1)
        self._diag_valid = False
        _lib.check(self._l.aqc_dm_set(self.h, _lib.ptr(flat)))

    def set_diag(self, d):
        """The matrix diag(d) from 2^n real entries (aqc_dm_set_diag)."""
        d = np.ascontiguousarray(d, dtype=np.float64).reshape(-1)
        if len(d) != 2 ** self.n:
            raise ValueError(f"set_diag: {2 ** self.n} diagonal entries expected")
        self._diag_valid = False
        _lib.check(self._l.aqc_dm_set_diag(self.h, _lib.dptr(d)))

    def copy_from(self, other):
        """self <- other on the device (aqc_dm_copy; the same qubit count)."""
        self._diag_valid = False
        _lib.check(self._l.aqc_dm_copy(self.h, other.h))

    def transition(self, ket, q):
        """The [4, 4] complex T[j', j] = sum_o conj(self[j', o]) ket[j, o] (aqc_dm_transition): j = r_q +
        2 c_q the local index of qubit ``q``, o every other index bit.  For a superoperator S on qubit q
        (``noise.candidate_superoperator``), Tr(self^H (S_q (x) id)(ket)) = sum(S * T): with self an
        observable pulled back through the gates after a one-qubit gate and ``ket`` the state before it,
        one scan of both prices every candidate for that gate.  Fixed summation order."""
        out = np.zeros(16, dtype=np.complex128)
        _lib.check(self._l.aqc_dm_transition(self.h, ket.h, int(q), _lib.ptr(out)))
        return out.reshape(4, 4)

    def inner(self, other):
        """Tr(self^H other), the Hilbert-Schmidt inner product (the trace of ``transition(other, 0)``).
        For density matrices ``rho.inner(rho)`` is the purity Tr rho^2 and ``rho.inner(sigma)`` the state
        overlap Tr(rho sigma) (real up to rounding)."""
        return complex(np.trace(self.transition(other, 0)))

    def _trace0(self):
        out = np.zeros(2)
        _lib.check(self._l.aqc_dm_trace0(self.h, _lib.dptr(out)))
        return out

    def prob0(self):
        """Re rho_00: the probability of reading all zeros (not divided by the trace)."""
        return float(self._trace0()[0])

    def trace(self):
        return float(self._trace0()[1])

    def _diagonal(self):
        """The DeviceSV holding sqrt(rho_kk) (aqc_dm_diag_sv): the statevector readers serve it."""
        if self._diag is None:
            self._diag = DeviceSV(self.n)
        if not self._diag_valid:
            _lib.check(self._l.aqc_dm_diag_sv(self.h, self._diag.h))
            self._diag_valid = True
        return self._diag

    def probabilities(self):
        """float64 [2^n]: max(0, Re rho_kk)."""
        return self._diagonal().get().real ** 2

    def sample(self, shots, seed, run=0, u=None):
        """``shots`` outcomes of all qubits drawn from the diagonal by aqc_sv_sample's rule: uint64[shots]
        basis indices.  ``u`` as ``DeviceSV.sample``."""
        return self._diagonal().sample(shots, seed, run, u)

    def z_all(self):
        """<Z_q> of every qubit from the diagonal (not divided by the trace)."""
        return self._diagonal().z_all()

    def pauli_expect(self, terms, effects=None):
        """Re Tr(M_t rho) of every term (aqc_dm_pauli_expect).  ``terms``: qiskit labels (rightmost
        character = qubit 0) or an (nterms, n) uint8 code array, none all-identity.  ``effects`` None: M_t
        is the Pauli string; else the [n, 3, 2, 4] POVM effects of noise.readout_effects and M_t the
        parity operator of the noisy readout of term t."""
        from . import paulis

        codes = paulis.terms_to_codes(terms, self.n)
        out = np.zeros(len(codes))
        if len(codes) == 0:
            return out
        eff = None
        if effects is not None:
            eff = np.ascontiguousarray(effects, dtype=np.float64)
            if eff.shape != (self.n, 3, 2, 4):
                raise ValueError(f"pauli_expect: effects must have shape {(self.n, 3, 2, 4)}")
        _lib.check(self._l.aqc_dm_pauli_expect(self.h, _lib.ptr(codes), len(codes), _lib.ptr(eff), _lib.ptr(out)))
        return out

    def pair_rdms(self, pairs):
        """4x4 reduced density matrices of qubit pairs, conventions of ``DeviceSV.pair_rdms``."""
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1))
        out = np.zeros(len(pairs) // 2 * 16, dtype=np.complex128)
        if len(pairs):
            _lib.check(self._l.aqc_dm_pair_rdms(self.h, _lib.ptr(pairs), len(pairs) // 2, _lib.ptr(out)))
        return out.reshape(-1, 4, 4)

    def pair_envs(self, pairs, effects=None):
        """complex [npairs, 4, 4]: every pair's environment R = Tr_rest((1 (x) E_rest) rho)
        (aqc_dm_pair_envs), index 2 bit_hi + bit_lo as ``pair_rdms``.  ``effects``: float64 [n, 4], qubit
        q's Hermitian effect as (E00, E11, Re E01, Im E01) (``noise.terminal_effects``; a pair's own
        entries are ignored), or None for identity effects, which give the RDMs.  For any channel L on
        the pair, Tr(((x) E_q) (L (x) id)(rho)) = Tr((E_hi (x) E_lo) L(R))."""
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1))
        eff = None
        if effects is not None:
            eff = np.ascontiguousarray(effects, dtype=np.float64)
            if eff.shape != (self.n, 4):
                raise ValueError(f"pair_envs: effects must have shape {(self.n, 4)}")
        out = np.zeros(len(pairs) // 2 * 16, dtype=np.complex128)
        if len(pairs):
            _lib.check(self._l.aqc_dm_pair_envs(self.h, _lib.ptr(pairs), len(pairs) // 2, _lib.ptr(eff), _lib.ptr(out)))
        return out.reshape(-1, 4, 4)

    def pair_transitions(self, ket, pairs):
        """complex [npairs, 16, 16]: ``transition`` for pairs (aqc_dm_pair_transitions), T[j', j] =
        sum_o conj(self[j', o]) ket[j, o] at the pair's local index j = (r_lo + 2 r_hi) + 4 (c_lo + 2 c_hi) --
        ``noise.layer_superoperator``'s index, lo / hi the pair's smaller / larger qubit in whatever order it
        is listed.  For a two-qubit superoperator S on the pair, Tr(self^H (S (x) id)(ket)) = sum(S * T): with
        self a cost observable pulled back through everything behind a candidate layer and ``ket`` the state
        in front of it, one call prices every candidate on every pair.  Fixed summation order."""
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1))
        out = np.zeros(len(pairs) // 2 * 256, dtype=np.complex128)
        if len(pairs):
            _lib.check(self._l.aqc_dm_pair_transitions(self.h, ket.h, _lib.ptr(pairs), len(pairs) // 2, _lib.ptr(out)))
        return out.reshape(-1, 16, 16)


def dm_pair_transitions_split(n, npairs=1):
    """The workgroups ``DeviceDM.pair_transitions`` spreads one pair over, for ``npairs`` pairs of ``n``
    qubits (aqc_dm_pair_transitions_plan; no GPU)."""
    split = ctypes.c_int()
    _lib.check(_lib.load().aqc_dm_pair_transitions_plan(int(n), int(npairs), ctypes.byref(split)))
    return int(split.value)


DM_PLAN_COUNTS = ("segments", "steps", "rows", "tile_bits")


def dm_plan(n, rows, return_steps=False, adjoint=False):
    """The plan of ``DeviceDM.run`` (aqc_dm_plan; no GPU): a dict of the counts named in DM_PLAN_COUNTS
    (segments = launches), and with ``return_steps`` also the steps in execution order as a
    DM_STEP_DTYPE array (kind 0: a unitary step, U in ``m``; kind 1: a superoperator step, S in ``m``;
    see include/aqc_hip.h).  ``adjoint``: the plan of ``DeviceDM.run_adjoint`` (aqc_dm_plan_adjoint)."""
    rows = np.ascontiguousarray(rows, dtype=_lib.OP_DTYPE)
    counts = np.zeros(4, dtype=np.int32)
    prog = _lib.ptr(rows) if len(rows) else None
    entry = _lib.load().aqc_dm_plan_adjoint if adjoint else _lib.load().aqc_dm_plan
    _lib.check(entry(int(n), prog, len(rows), _lib.ptr(counts), None, 0))
    named = dict(zip(DM_PLAN_COUNTS, (int(c) for c in counts)))
    if not return_steps:
        return named
    steps = np.zeros(int(counts[1]), dtype=_lib.DM_STEP_DTYPE)
    _lib.check(entry(int(n), prog, len(rows), _lib.ptr(counts), _lib.ptr(steps) if len(steps) else None, len(steps)))
    return named, steps


class DeviceMPS:
    """Vidal-form MPS resident in HBM with Aer MPS-simulator semantics."""

    def __init__(self, n, chi_cap, threshold=1e-16, max_chi=None):
        self._l = _lib.lib()
        self.n = int(n)
        self.chi_cap = int(chi_cap)
        h = ctypes.c_void_p()
        _lib.check(
            self._l.aqc_mps_create(self.n, self.chi_cap, float(threshold), int(max_chi or 0), ctypes.byref(h))
        )
        self.h = h

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self._l.aqc_mps_destroy(self.h)
            self.h = None

    __del__ = close

    # -- state transfer --------------------------------------------------------------
    def set_truncation(self, threshold, max_chi):
        _lib.check(self._l.aqc_mps_set_truncation(self.h, float(threshold), int(max_chi or 0)))

    def load_aer(self, qiskit_mps):
        gam, lam = qiskit_mps
        if len(gam) != self.n:
            raise ValueError("MPS length mismatch")
        dims = [1]
        for a, _ in gam:
            dims.append(np.asarray(a).shape[1])
        dims = np.asarray(dims, dtype=np.int32)
        if dims.max() > self.chi_cap:
            raise ValueError(f"MPS bond dimension {dims.max()} exceeds chi_cap {self.chi_cap}")
        g = np.concatenate(
            [np.stack([np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)]).reshape(-1) for a, b in gam]
        )
        l = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in lam]) if len(lam) else np.zeros(1)
        g = np.ascontiguousarray(g)
        l = np.ascontiguousarray(l)
        _lib.check(self._l.aqc_mps_set_vidal(self.h, _lib.ptr(dims), _lib.ptr(g), _lib.ptr(l)))

    def dims(self):
        d = np.zeros(self.n + 1, dtype=np.int32)
        _lib.check(self._l.aqc_mps_get_dims(self.h, _lib.ptr(d)))
        return d

    def to_aer(self):
        """save_matrix_product_state: sorted qubits, Aer format."""
        d = np.zeros(self.n + 1, dtype=np.int32)
        _lib.check(self._l.aqc_mps_get_vidal(self.h, _lib.ptr(d), None, None))
        ng = int(sum(2 * d[i] * d[i + 1] for i in range(self.n)))
        nl = int(sum(d[1:self.n]))
        g = np.zeros(ng, dtype=np.complex128)
        l = np.zeros(max(nl, 1), dtype=np.float64)
        _lib.check(self._l.aqc_mps_get_vidal(self.h, _lib.ptr(d), _lib.ptr(g), _lib.ptr(l)))
        gam, lam = [], []
        off = 0
        for i in range(self.n):
            a, b = int(d[i]), int(d[i + 1])
            t = g[off: off + 2 * a * b].reshape(2, a, b)
            gam.append((t[0].copy(), t[1].copy()))
            off += 2 * a * b
        off = 0
        for bnd in range(1, self.n):
            k = int(d[bnd])
            lam.append(l[off: off + k].copy())
            off += k
        return gam, lam

    def preprocessed(self):
        """aqc_research ``_preprocess_mps`` form: list of (2, chi_l, chi_r) arrays."""
        gam, lam = self.to_aer()
        out = []
        for i, (a, b) in enumerate(gam):
            t = np.stack([a, b])
            if i < self.n - 1:
                t = t * lam[i][None, None, :]
            out.append(t)
        return out

    def copy_from(self, other):
        _lib.check(self._l.aqc_mps_copy(self.h, other.h))

    # -- gates and measurements ------------------------------------------------------
    def apply(self, ops):
        if len(ops) == 0:
            return
        arr = ops if isinstance(ops, np.ndarray) else _lib.ops_array(ops)
        _lib.check(self._l.aqc_mps_apply(self.h, _lib.ptr(arr), len(arr)))

    def sort(self):
        _lib.check(self._l.aqc_mps_sort(self.h))

    def overlap_zero(self):
        """``mps_dot(psi, zero_mps)`` = <psi|0...0>."""
        re, im = ctypes.c_double(), ctypes.c_double()
        _lib.check(self._l.aqc_mps_overlap_zero(self.h, ctypes.byref(re), ctypes.byref(im)))
        return complex(re.value, im.value)

    def dot(self, other):
        """<self|other> (conjugates self)."""
        re, im = ctypes.c_double(), ctypes.c_double()
        _lib.check(self._l.aqc_mps_dot(self.h, other.h, ctypes.byref(re), ctypes.byref(im)))
        return complex(re.value, im.value)

    def z_all(self):
        out = np.zeros(self.n)
        _lib.check(self._l.aqc_mps_z_all(self.h, _lib.ptr(out)))
        return out

    def amps_hw1(self):
        out = np.zeros(2 * self.n)
        _lib.check(self._l.aqc_mps_amps_hw1(self.h, _lib.ptr(out)))
        return out[0::2] + 1j * out[1::2]

    def sample(self, shots, seed, run=0, u=None):
        """``shots`` measurement outcomes of all qubits (aqc_mps_sample): uint64[shots, words],
        bit q % 64 of word q // 64 = outcome of qubit q.  ``u``: [shots, n] uniforms in [0, 1) used
        instead of the generator's."""
        shots = int(shots)
        out = np.zeros((max(shots, 0), (self.n + 63) // 64), dtype=np.uint64)
        up = _uniforms_arg(u, (shots, self.n))
        _lib.check(self._l.aqc_mps_sample(self.h, shots, _u64(seed), _u64(run), _lib.ptr(up), _lib.ptr(out)))
        return out

    def pauli_expect(self, terms):
        """<psi|P_t|psi> of every Pauli string (aqc_mps_pauli_expect), not divided by <psi|psi> (the
        convention of z_all).  ``terms``: qiskit labels (rightmost character = qubit 0) or an
        (nterms, n) uint8 code array (0 I, 1 X, 2 Y, 3 Z; column q = qubit q)."""
        from . import paulis

        codes = paulis.terms_to_codes(terms, self.n)
        out = np.zeros(len(codes))
        _lib.check(self._l.aqc_mps_pauli_expect(self.h, _lib.ptr(codes), len(codes), _lib.ptr(out)))
        return out

    def product_fit(self, svec=None, min_sweeps=10, max_sweeps=50, tol=1e-12):
        """Best product-state approximation (aqc_mps_product_fit): returns (svec (n, 2), fidelity,
        sweeps).  svec None starts from the chi = 1 truncation of the canonical form."""
        guess = svec is None
        s = np.zeros((self.n, 2), dtype=np.complex128) if guess else np.array(svec, dtype=np.complex128)
        s = np.ascontiguousarray(s.reshape(self.n, 2))
        fid = ctypes.c_double()
        sw = ctypes.c_int()
        _lib.check(self._l.aqc_mps_product_fit(self.h, _lib.ptr(s), int(guess), int(min_sweeps), int(max_sweeps),
                                               float(tol), ctypes.byref(fid), ctypes.byref(sw)))
        return s, fid.value, sw.value

    def pair_rdms(self, pairs):
        """4x4 RDMs of qubit pairs by environment chains (aqc_research partial_trace semantics)."""
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1))
        out = np.zeros(len(pairs) // 2 * 16, dtype=np.complex128)
        if len(pairs):
            _lib.check(self._l.aqc_mps_pair_rdms(self.h, _lib.ptr(pairs), len(pairs) // 2, _lib.ptr(out)))
        return out.reshape(-1, 4, 4)


def _dmrg_operator(operator, n):
    """(codes (nterms, n) uint8, real coefficients float64) of a Pauli sum in the forms
    ``DeviceSV.pauli_apply`` takes; a Hamiltonian's coefficients are real."""
    from . import paulis

    if isinstance(operator, dict):
        terms, coeffs = list(operator.keys()), list(operator.values())
    else:
        terms, coeffs = operator
    codes = paulis.terms_to_codes(terms, n)
    coeffs = np.asarray(coeffs, dtype=np.complex128).reshape(-1)
    if len(coeffs) != len(codes):
        raise ValueError(f"a Pauli sum needs one coefficient per term: {len(codes)} terms, {len(coeffs)} coefficients")
    if np.any(coeffs.imag != 0):
        raise ValueError("a Hamiltonian (a Hermitian Pauli sum) has real coefficients")
    return codes, np.ascontiguousarray(coeffs.real, dtype=np.float64)


DMRG_CLASSES = ("closed left", "closed right", "local", "open", "identity")
DMRG_RECORD_KINDS = ("LH", "RH", "local", "open")


def dmrg_plan(n, operator, chi_cap=64, krylov_dim=6):
    """The bond plan of a two-site DMRG of ``operator`` on n qubits (aqc_mps_dmrg_plan; no GPU): a dict
    with the totals (``total_records``, ``max_records``, ``env_matrices``, ``env_bytes`` and
    ``scratch_bytes`` at ``chi_cap``, ``record_limit``, ``byte_budget``, ``identities``), ``bonds`` (per
    bond: records, closed-left, closed-right and local terms, open records, stored left and right
    environments of open terms), ``records`` (rows of bond, kind, term, flags; kinds ``DMRG_RECORD_KINDS``,
    flag bit 0 / 1: a stored left / right environment) and ``classes`` ((n - 1, nterms), indices into
    ``DMRG_CLASSES``).  Raises ``AqcError`` naming the numbers when a bond has more records than the
    limit or environments and scratch exceed the byte budget."""
    n = int(n)
    if n < 1:
        raise ValueError("dmrg_plan: n >= 1")
    codes, coeffs = _dmrg_operator(operator, n)
    l = _lib.load()
    totals = np.zeros(8, dtype=np.int64)
    bonds = np.zeros((max(n - 1, 0), 7), dtype=np.int32)
    classes = np.zeros((max(n - 1, 0), len(codes)), dtype=np.uint8)
    args = (n, _lib.ptr(codes), _lib.ptr(coeffs), len(codes), int(chi_cap), int(krylov_dim), _lib.ptr(totals))
    _lib.check(l.aqc_mps_dmrg_plan(*args, _lib.ptr(bonds), None, 0, _lib.ptr(classes)))
    records = np.zeros((int(totals[0]), 4), dtype=np.int32)
    _lib.check(l.aqc_mps_dmrg_plan(*args, None, _lib.ptr(records) if len(records) else None, len(records), None))
    names = ("total_records", "max_records", "env_matrices", "env_bytes", "scratch_bytes", "record_limit", "byte_budget",
             "identities")
    out = {k: int(v) for k, v in zip(names, totals)}
    out.update(bonds=bonds, records=records, classes=classes)
    return out


class DeviceDMRG:
    """Two-site DMRG of a Pauli sum on a ``DeviceMPS`` (aqc_dmrg_*): the environments, the Krylov scratch
    and the record tables.  The MPS is not owned and must outlive the handle; after any change of it that
    is not one of this handle's sweeps, every call is refused."""

    def __init__(self, mps, operator, krylov_dim=6):
        self._l = _lib.lib()
        self.mps = mps
        self.n = mps.n
        codes, coeffs = _dmrg_operator(operator, self.n)
        h = ctypes.c_void_p()
        _lib.check(self._l.aqc_dmrg_create(mps.h, _lib.ptr(codes), _lib.ptr(coeffs), len(codes), int(krylov_dim),
                                           ctypes.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self._l.aqc_dmrg_destroy(self.h)
            self.h = None

    __del__ = close

    def sweep(self):
        """One sweep (left to right, then back): the 2 (n - 1) Ritz values in update order."""
        out = np.zeros(2 * (self.n - 1))
        _lib.check(self._l.aqc_dmrg_sweep(self.h, _lib.ptr(out)))
        return out

    def heff_apply(self, bond, x):
        """y = H_eff x at ``bond`` with the environments of the state as it stands (test hook,
        aqc_dmrg_heff_apply); x in theta's layout, 4 dims[bond] dims[bond + 2] complex numbers."""
        bond = int(bond)
        d = self.mps.dims()
        if not 0 <= bond < self.n - 1:
            raise ValueError("heff_apply: bond outside 0 .. n - 2")
        x = np.ascontiguousarray(x, dtype=np.complex128).reshape(-1)
        if len(x) != 4 * int(d[bond]) * int(d[bond + 2]):
            raise ValueError(f"heff_apply: x needs {4 * int(d[bond]) * int(d[bond + 2])} amplitudes, got {len(x)}")
        y = np.zeros_like(x)
        _lib.check(self._l.aqc_dmrg_heff_apply(self.h, bond, _lib.ptr(x), _lib.ptr(y)))
        return y

    def stats(self):
        """{"breakdowns": bond updates whose Lanczos iteration ended early, "updates": bond updates}."""
        out = np.zeros(2, dtype=np.int64)
        _lib.check(self._l.aqc_dmrg_stats(self.h, _lib.ptr(out)))
        return {"breakdowns": int(out[0]), "updates": int(out[1])}


def _u64(x):
    return ctypes.c_uint64(int(x) & 0xFFFFFFFFFFFFFFFF)


def _uniforms_arg(u, shape):
    if u is None:
        return None
    u = np.ascontiguousarray(u, dtype=np.float64)
    if u.shape != tuple(shape):
        raise ValueError(f"sample: u must have shape {tuple(shape)}")
    return u


def sample_uniforms(seed, run, shots, nper):
    """The uniforms the samplers draw for (seed, run): [shots, nper] (aqc_sample_uniforms)."""
    out = np.zeros((int(shots), int(nper)))
    _lib.check(_lib.lib().aqc_sample_uniforms(_u64(seed), _u64(run), int(shots), int(nper), _lib.ptr(out)))
    return out


def _count_events(rows):
    """The events of a trajectory program: its one-qubit Kraus rows plus its correlated groups."""
    from .noise import count_events

    return count_events(rows)


def _refuse_correlated_rows(rows, what):
    from .noise import _CORRELATED_ON_MPS, has_correlated_rows

    if has_correlated_rows(rows):
        raise NotImplementedError(f"{what}: {_CORRELATED_ON_MPS}")


class _correlated_mode:
    """The MPS trajectory engine's process-wide switch for correlated groups (aqc_mps_traj_set_correlated)
    around one call: ``correlated`` False / 0 leaves it alone (the refusal stands), True / 1 runs groups,
    2 runs every group on the general path.  0 is restored on exit."""

    def __init__(self, correlated):
        self.mode = int(correlated)
        if self.mode not in (0, 1, 2):
            raise ValueError("correlated must be False, True (1) or 2")

    def __enter__(self):
        if self.mode:
            _lib.check(_lib.load().aqc_mps_traj_set_correlated(self.mode))
        return self

    def __exit__(self, *exc):
        if self.mode:
            _lib.load().aqc_mps_traj_set_correlated(0)
        return False


def _check_mps_rows(rows, n_events, correlated, what):
    """The refusal of correlated groups unless ``correlated``, and n_events against the program."""
    if not int(correlated):
        _refuse_correlated_rows(rows, what)
        found = int(np.count_nonzero(rows["flags"] == _lib.OP_KRAUS1))
    else:
        found = _count_events(rows)
    if found != n_events:
        raise ValueError(f"{what}: n_events does not match the program's Kraus rows")


def trajectory_sample(n, rows, n_events, shots, seed, run=0, u=None, return_choices=False):
    """``shots`` noisy shots as quantum trajectories (aqc_sv_traj_sample): uint64[shots] basis indices
    (bit q = qubit q) of the program ``rows`` (noise.trajectory_program) on n qubits, whose events
    (one-qubit Kraus rows and correlated two-qubit groups) number ``n_events``.  ``u``: [shots,
    n_events + 1] uniforms in [0, 1) used instead of the generator's (event e in column e, the final
    draw last).  With ``return_choices`` also the uint8[shots, n_events] Kraus operator (0 .. 15 for a
    correlated group) chosen at every event."""
    shots, n_events = int(shots), int(n_events)
    rows = np.ascontiguousarray(rows, dtype=_lib.OP_DTYPE)
    if _count_events(rows) != n_events:
        raise ValueError("trajectory_sample: n_events does not match the program's Kraus rows")
    out = np.zeros(max(shots, 0), dtype=np.uint64)
    up = _uniforms_arg(u, (shots, n_events + 1))
    choices = np.zeros((max(shots, 0), n_events), dtype=np.uint8) if return_choices else None
    _lib.check(_lib.lib().aqc_sv_traj_sample(int(n), _lib.ptr(rows) if len(rows) else None, len(rows), shots, _u64(seed),
                                             _u64(run), _lib.ptr(up), _lib.ptr(out),
                                             _lib.ptr(choices) if return_choices and n_events else None))
    return (out, choices) if return_choices else out


def trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, seed, run=0, u=None, return_outcomes=False):
    """Noisy tomography counts of every pair in one launch (aqc_sv_traj_pair_tomo): int64 [npairs, 9, 4],
    ``shots`` per Pauli setting, of the program ``rows`` (noise.trajectory_program of the circuit without
    its classical operations) whose Kraus rows number ``n_events``, measured with the POVM ``effects``
    [n, 3, 2, 4] (noise.readout_effects).  9 ``shots`` trajectories run; trajectory t = 9 i + s serves
    setting s = 3 b_hi + b_lo of every pair.  ``u``: [9 shots, n_events + npairs] uniforms in [0, 1) used
    instead of the generator's (events first, then pairs).  With ``return_outcomes`` also the uint8
    [9 shots, npairs] outcome o = 2 o_hi + o_lo every trajectory drew for every pair."""
    n, shots, n_events = int(n), int(shots), int(n_events)
    rows = np.ascontiguousarray(rows, dtype=_lib.OP_DTYPE)
    if _count_events(rows) != n_events:
        raise ValueError("trajectory_pair_tomography: n_events does not match the program's Kraus rows")
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    npairs = len(pr)
    eff = np.ascontiguousarray(effects, dtype=np.float64)
    if eff.shape != (n, 3, 2, 4):
        raise ValueError(f"trajectory_pair_tomography: effects must have shape {(n, 3, 2, 4)}")
    ntraj = 9 * max(shots, 0)
    up = _uniforms_arg(u, (ntraj, n_events + npairs))
    counts = np.zeros((npairs, 9, 4), dtype=np.int64)
    outcomes = np.zeros((ntraj, npairs), dtype=np.uint8) if return_outcomes else None
    _lib.check(_lib.lib().aqc_sv_traj_pair_tomo(n, _lib.ptr(rows) if len(rows) else None, len(rows),
                                                _lib.ptr(pr) if npairs else None, npairs, _lib.ptr(eff), shots,
                                                _u64(seed), _u64(run), _lib.ptr(up), _lib.ptr(counts),
                                                _lib.ptr(outcomes) if return_outcomes and npairs else None))
    return (counts, outcomes) if return_outcomes else counts


def trajectory_pauli_counts(n, rows, n_events, terms, effects, shots, seed, run=0, u=None, return_values=False,
                            return_outcomes=False):
    """The noisy Pauli readout of every term in one launch (aqc_sv_traj_pauli_counts): int64 [nterms], the
    number of +1 parities among ``shots`` trajectories of the program ``rows`` (noise.trajectory_program
    of the circuit without its classical operations, ``n_events`` events), every trajectory drawing one
    +-1 outcome per term from its own state under the POVM ``effects`` [n, 3, 2, 4]
    (noise.readout_effects).  ``terms``: qiskit labels (rightmost character = qubit 0) or an
    (nterms, n) uint8 code array; no all-identity term.  The estimate of a term is
    (2 plus - shots) / shots.  ``u``: [shots, n_events + nterms] uniforms in [0, 1) used instead of the
    generator's (events first, then terms).  With ``return_values`` also the float64 [shots, nterms]
    Re <psi_t|M_j|psi_t> before clamping, with ``return_outcomes`` the uint8 [shots, nterms] outcomes
    (1 = parity -1); the result is then the tuple (plus[, values][, outcomes])."""
    from . import paulis

    n, shots, n_events = int(n), int(shots), int(n_events)
    rows = np.ascontiguousarray(rows, dtype=_lib.OP_DTYPE)
    if _count_events(rows) != n_events:
        raise ValueError("trajectory_pauli_counts: n_events does not match the program's Kraus rows")
    codes = paulis.terms_to_codes(terms, n)
    nterms = len(codes)
    eff = np.ascontiguousarray(effects, dtype=np.float64)
    if eff.shape != (n, 3, 2, 4):
        raise ValueError(f"trajectory_pauli_counts: effects must have shape {(n, 3, 2, 4)}")
    up = _uniforms_arg(u, (shots, n_events + nterms))
    plus = np.zeros(nterms, dtype=np.int64)
    values = np.zeros((max(shots, 0), nterms)) if return_values else None
    outcomes = np.zeros((max(shots, 0), nterms), dtype=np.uint8) if return_outcomes else None
    _lib.check(_lib.lib().aqc_sv_traj_pauli_counts(n, _lib.ptr(rows) if len(rows) else None, len(rows),
                                                   _lib.ptr(codes) if nterms else None, nterms, _lib.ptr(eff), shots,
                                                   _u64(seed), _u64(run), _lib.ptr(up), _lib.ptr(plus),
                                                   _lib.ptr(values) if return_values and nterms else None,
                                                   _lib.ptr(outcomes) if return_outcomes and nterms else None))
    out = (plus,) + ((values,) if return_values else ()) + ((outcomes,) if return_outcomes else ())
    return out if len(out) > 1 else plus


def mps_trajectory_sample(n, rows, n_events, shots, seed, run=0, u=None, return_choices=False, chi_cap=64,
                          threshold=1e-16, max_chi=None, correlated=False):
    """``shots`` noisy shots as quantum trajectories on the MPS engine (aqc_mps_traj_sample):
    uint64[shots, (n + 63) // 64] outcome words (bit q % 64 of word q // 64 = qubit q, DeviceMPS.sample's
    format) of the program ``rows`` (noise.trajectory_program) on n qubits, whose Kraus rows number
    ``n_events``.  Every trajectory is an MPS of capacity ``chi_cap`` truncated by (``threshold``,
    ``max_chi``); one that outgrows the capacity raises the capacity AqcError.  ``u``: [shots,
    n_events + n] uniforms in [0, 1) used instead of the generator's (event e in column e, qubit q's
    measurement in column n_events + q).  With ``return_choices`` also the uint8[shots, n_events] Kraus
    operator chosen at every event.  ``correlated``: False refuses a program with correlated two-qubit
    groups; True (or 1) runs them, one event each (choices 0 .. 15), a product-unitary group such as
    ``depolarizing_error(p, 2)`` as one-site unitaries and any other as a two-site update whose operator is
    chosen on the device; 2 sends every group down that general path (a second route to the same outcomes)."""
    shots, n_events, n = int(shots), int(n_events), int(n)
    rows = np.ascontiguousarray(rows, dtype=_lib.OP_DTYPE)
    _check_mps_rows(rows, n_events, correlated, "mps_trajectory_sample")
    out = np.zeros((max(shots, 0), (max(n, 1) + 63) // 64), dtype=np.uint64)
    up = _uniforms_arg(u, (shots, n_events + n))
    choices = np.zeros((max(shots, 0), n_events), dtype=np.uint8) if return_choices else None
    with _correlated_mode(correlated):
        _lib.check(_lib.lib().aqc_mps_traj_sample(n, int(chi_cap), float(threshold), int(max_chi or 0),
                                                  _lib.ptr(rows) if len(rows) else None, len(rows), shots, _u64(seed),
                                                  _u64(run), _lib.ptr(up), _lib.ptr(out),
                                                  _lib.ptr(choices) if return_choices and n_events else None))
    return (out, choices) if return_choices else out


def mps_trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, seed, run=0, u=None, return_outcomes=False,
                                   chi_cap=64, threshold=1e-16, max_chi=None, correlated=False):
    """``trajectory_pair_tomography`` on the MPS engine (aqc_mps_traj_pair_tomo): the same arguments, the
    same int64 [npairs, 9, 4] counts and, with ``return_outcomes``, uint8 [9 shots, npairs] outcomes.
    Every one of the 9 ``shots`` trajectories is an MPS of capacity ``chi_cap`` truncated by
    (``threshold``, ``max_chi``), run through ``mps_trajectory_sample``'s schedule without its
    measurement sweep and read out pair by pair from its RDMs; one that outgrows the capacity raises
    the capacity AqcError.  ``correlated``: as ``mps_trajectory_sample``."""
    n, shots, n_events = int(n), int(shots), int(n_events)
    rows = np.ascontiguousarray(rows, dtype=_lib.OP_DTYPE)
    _check_mps_rows(rows, n_events, correlated, "mps_trajectory_pair_tomography")
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    npairs = len(pr)
    eff = np.ascontiguousarray(effects, dtype=np.float64)
    if eff.shape != (n, 3, 2, 4):
        raise ValueError(f"mps_trajectory_pair_tomography: effects must have shape {(n, 3, 2, 4)}")
    ntraj = 9 * max(shots, 0)
    up = _uniforms_arg(u, (ntraj, n_events + npairs))
    counts = np.zeros((npairs, 9, 4), dtype=np.int64)
    outcomes = np.zeros((ntraj, npairs), dtype=np.uint8) if return_outcomes else None
    with _correlated_mode(correlated):
        _lib.check(_lib.lib().aqc_mps_traj_pair_tomo(n, int(chi_cap), float(threshold), int(max_chi or 0),
                                                     _lib.ptr(rows) if len(rows) else None, len(rows),
                                                     _lib.ptr(pr) if npairs else None, npairs, _lib.ptr(eff), shots,
                                                     _u64(seed), _u64(run), _lib.ptr(up), _lib.ptr(counts),
                                                     _lib.ptr(outcomes) if return_outcomes and npairs else None))
    return (counts, outcomes) if return_outcomes else counts


def mps_trajectory_pauli_counts(n, rows, n_events, terms, effects, shots, seed, run=0, u=None, return_values=False,
                                return_norms=False, return_outcomes=False, chi_cap=64, threshold=1e-16, max_chi=None,
                                correlated=False):
    """``trajectory_pauli_counts`` on the MPS engine (aqc_mps_traj_pauli_counts): the same arguments and
    the same int64 [nterms] count of +1 parities, with no limit on the general factors of a term.  Every
    one of the ``shots`` trajectories is an MPS of capacity ``chi_cap`` truncated by (``threshold``,
    ``max_chi``), run through ``mps_trajectory_pair_tomography``'s schedule and read out for every term
    by a transfer chain over the term's support; one that outgrows the capacity raises the capacity
    AqcError.  With ``return_values`` also the float64 [shots, nterms] v = Re <psi_t|M_j|psi_t>, with
    ``return_norms`` the float64 [shots] w = <psi_t|psi_t> (below 1 for a truncated trajectory; the draw
    uses p+- = (w +- v) / 2, so nothing is renormalised), with ``return_outcomes`` the uint8
    [shots, nterms] outcomes (1 = parity -1); the result is then the tuple
    (plus[, values][, norms][, outcomes]).  ``correlated``: as ``mps_trajectory_sample``."""
    from . import paulis

    n, shots, n_events = int(n), int(shots), int(n_events)
    rows = np.ascontiguousarray(rows, dtype=_lib.OP_DTYPE)
    _check_mps_rows(rows, n_events, correlated, "mps_trajectory_pauli_counts")
    codes = paulis.terms_to_codes(terms, n)
    nterms = len(codes)
    eff = np.ascontiguousarray(effects, dtype=np.float64)
    if eff.shape != (n, 3, 2, 4):
        raise ValueError(f"mps_trajectory_pauli_counts: effects must have shape {(n, 3, 2, 4)}")
    up = _uniforms_arg(u, (shots, n_events + nterms))
    plus = np.zeros(nterms, dtype=np.int64)
    values = np.zeros((max(shots, 0), nterms)) if return_values else None
    norms = np.zeros(max(shots, 0)) if return_norms else None
    outcomes = np.zeros((max(shots, 0), nterms), dtype=np.uint8) if return_outcomes else None
    with _correlated_mode(correlated):
        _lib.check(_lib.lib().aqc_mps_traj_pauli_counts(n, int(chi_cap), float(threshold), int(max_chi or 0),
                                                        _lib.ptr(rows) if len(rows) else None, len(rows),
                                                        _lib.ptr(codes) if nterms else None, nterms, _lib.ptr(eff), shots,
                                                        _u64(seed), _u64(run), _lib.ptr(up), _lib.ptr(plus),
                                                        _lib.ptr(values) if return_values and nterms else None,
                                                        _lib.ptr(norms) if return_norms and shots > 0 else None,
                                                        _lib.ptr(outcomes) if return_outcomes and nterms else None))
    out = ((plus,) + ((values,) if return_values else ()) + ((norms,) if return_norms else ())
           + ((outcomes,) if return_outcomes else ()))
    return out if len(out) > 1 else plus


MPS_TRAJECTORY_COUNTS = ("gate_updates", "swap_updates", "centre_moves", "one_site_rows", "kraus_rows",
                         "measure_rows", "rows")


def mps_trajectory_plan(n, rows, return_schedule=False, measure=True, correlated=False):
    """The site-level schedule every shot of ``mps_trajectory_sample`` runs (aqc_mps_traj_plan; no GPU):
    a dict of the row counts named in MPS_TRAJECTORY_COUNTS (a two-site update is a gate, swap or
    centre-move row), and with ``return_schedule`` also the rows themselves as an OP_DTYPE array
    (``q0`` the site; flags 0 unitary, ``flags & 0xff == OP_KRAUS1`` a Kraus row with its event index
    in ``flags >> 8``, OP_MEASURE1 the measurement of qubit ``q1``; see include/aqc_hip.h).
    ``measure=False``: the schedule of ``mps_trajectory_pair_tomography`` (aqc_mps_traj_tomo_plan), which
    ends with the sort, before the measurement sweep.
    ``correlated`` (as ``mps_trajectory_sample``): a group's event then appears as nk consecutive rows with
    ``flags == OP_KRAUS2 | k << 8 | nk << 16``, bit 24 added for a product-unitary group, ``q0 < q1`` the
    two sites and ``m`` the folded operator in site order; "kraus_rows" counts a group once."""
    rows = np.ascontiguousarray(rows, dtype=_lib.OP_DTYPE)
    if not int(correlated):
        _refuse_correlated_rows(rows, "mps_trajectory_plan")
    counts = np.zeros(7, dtype=np.int32)
    prog = _lib.ptr(rows) if len(rows) else None
    entry = _lib.load().aqc_mps_traj_plan if measure else _lib.load().aqc_mps_traj_tomo_plan
    with _correlated_mode(correlated):
        _lib.check(entry(int(n), prog, len(rows), _lib.ptr(counts), None, 0))
        named = dict(zip(MPS_TRAJECTORY_COUNTS, (int(c) for c in counts)))
        if not return_schedule:
            return named
        sched = np.zeros(int(counts[6]), dtype=_lib.OP_DTYPE)
        _lib.check(entry(int(n), prog, len(rows), _lib.ptr(counts), _lib.ptr(sched), len(sched)))
    return named, sched


def counts_from_samples(samples, n, clbit_of_qubit=None):
    """Counts dict of qiskit bitstrings (highest bit leftmost) from sampler output: uint64[shots]
    basis indices (n <= 64) or uint64[shots, words] packed words.  ``clbit_of_qubit``: {qubit:
    clbit}; the keys then run over the clbits max(clbit) .. 0, an unwritten clbit reading 0;
    None: the keys run over all n qubits."""
    s = np.asarray(samples, dtype=np.uint64)
    if s.ndim == 1:
        s = s.reshape(-1, 1)
    if s.shape[1] * 64 < n:
        raise ValueError("counts_from_samples: too few words for n qubits")
    if clbit_of_qubit is None:
        width = int(n)
        cols = s[:, : (width + 63) // 64]
        if width % 64:
            cols = cols.copy()
            cols[:, -1] &= np.uint64((1 << (width % 64)) - 1)
    else:
        width = max(clbit_of_qubit.values()) + 1 if clbit_of_qubit else 0
        cols = np.zeros((s.shape[0], max(1, (width + 63) // 64)), dtype=np.uint64)
        for q, c in clbit_of_qubit.items():
            if not 0 <= q < n:
                raise ValueError("counts_from_samples: measured qubit out of range")
            bit = (s[:, q // 64] >> np.uint64(q % 64)) & np.uint64(1)
            mask = ~(np.uint64(1) << np.uint64(c % 64))
            cols[:, c // 64] = (cols[:, c // 64] & mask) | (bit << np.uint64(c % 64))  # (a later measure overwrites)
    if s.shape[0] == 0:
        return {}
    vals, cnt = np.unique(np.ascontiguousarray(cols), axis=0, return_counts=True)
    out = {}
    for v, c in zip(vals, cnt):
        x = 0
        for w in range(len(v) - 1, -1, -1):
            x = (x << 64) | int(v[w])
        out[format(x, f"0{max(width, 1)}b")[-max(width, 1):]] = int(c)
    return out


def _handles(states):
    arr = (ctypes.c_void_p * len(states))(*[s.h.value for s in states])
    return arr


class OpsBatch:
    """Per-state op lists marshalled once for the C ABI: the pointer array and the counts that
    apply_batch would otherwise rebuild from the Python list on every call (1-2 ms for 1024 lists,
    mostly ``ndarray.ctypes``).  It holds references to its arrays, so their contents may be
    rewritten in place between calls (new angles) and the batch stays valid; replacing an array
    needs a new OpsBatch."""

    def __init__(self, ops_lists):
        self.arrays = [np.ascontiguousarray(o) if isinstance(o, np.ndarray) else _lib.ops_array(o)
                       for o in ops_lists]
        self.ptrs = (ctypes.c_void_p * len(self.arrays))(*[a.ctypes.data if len(a) else 0 for a in self.arrays])
        self.counts = np.asarray([len(a) for a in self.arrays], dtype=np.int32)

    def __len__(self):
        return len(self.arrays)


def apply_batch(states, ops_lists, sort=False, wait=True):
    """Apply per-state op lists (one batched launch sequence, or one fused chain per state); with
    sort=True every state also returns to sorted qubit order in the same schedule (an evaluation's
    replay + save).  ops_lists: a list of op lists / ops arrays, or an OpsBatch.  wait=False
    returns once the work is queued; call check_batch(states) before trusting the states (their
    error flags are read there)."""
    if not states:
        return
    l = _lib.lib()
    batch = ops_lists if isinstance(ops_lists, OpsBatch) else OpsBatch(ops_lists)
    if len(batch) != len(states):
        raise ValueError("apply_batch: one op list per state")
    fn = l.aqc_mps_apply_sort_batch if sort else l.aqc_mps_apply_batch
    if not wait:
        fn = l.aqc_mps_apply_sort_batch_async if sort else l.aqc_mps_apply_batch_async
    _lib.check(fn(_handles(states), len(states), batch.ptrs, _lib.ptr(batch.counts)))


def check_batch(states):
    """Wait for the states' queued work and raise on their error flags (after apply_batch(...,
    wait=False))."""
    if states:
        _lib.check(_lib.lib().aqc_mps_check_batch(_handles(states), len(states)))


EM_METHOD_CODES = {"concurrence": 0, "eof": 1, "negativity": 2, "log_negativity": 3}


def entanglement_measures(rdms, method):
    """Entanglement measure of each 4x4 density matrix on the device (aqc_entanglement_measures)."""
    code = EM_METHOD_CODES[method]
    r = np.ascontiguousarray(np.asarray(rdms, dtype=np.complex128).reshape(-1, 16))
    out = np.zeros(len(r))
    if len(r):
        _lib.check(_lib.lib().aqc_entanglement_measures(_lib.ptr(r), len(r), code, _lib.ptr(out), 0))
    return out


# -- shot-based pair tomography (csrc/tomo.hip) -----------------------------------------------------
# Conventions (include/aqc_hip.h): pair (a, b) as hi = max, lo = min; RDM index 2 bit_hi + bit_lo;
# basis codes 0 X, 1 Y, 2 Z; setting s = 3 b_hi + b_lo; outcome o = 2 o_hi + o_lo, 0 the +1 eigenstate.
def _rdm_rows(rdms):
    return np.ascontiguousarray(np.asarray(rdms, dtype=np.complex128).reshape(-1, 16))


def pair_tomo_probs(rdms):
    """[npairs, 9, 4] outcome probabilities of the nine two-qubit Pauli settings of each 4x4 RDM
    (aqc_pair_tomo_probs): max(0, <v|rho|v>), not renormalised."""
    r = _rdm_rows(rdms)
    out = np.zeros((len(r), 9, 4))
    if len(r):
        _lib.check(_lib.lib().aqc_pair_tomo_probs(_lib.ptr(r), len(r), _lib.ptr(out), 0))
    return out


def concurrence_bound_probs(rdms):
    """[npairs, 3]: P("1111"), P("0011"), P("1100") of the three two-copy circuits of the observable
    concurrence bound (aqc_concurrence_bound_probs); "0011" belongs to the pair's lower qubit."""
    r = _rdm_rows(rdms)
    out = np.zeros((len(r), 3))
    if len(r):
        _lib.check(_lib.lib().aqc_concurrence_bound_probs(_lib.ptr(r), len(r), _lib.ptr(out), 0))
    return out


def multinomial_counts(probs, shots, seed, run=0, u=None):
    """int64[njobs, K] counts of ``shots`` draws from each row of ``probs`` [njobs, K], 2 <= K <= 16
    (aqc_multinomial_counts).  Job j's shot t uses the uniform of (seed, run, t, j), or ``u[t, j]``
    when ``u`` [shots, njobs] is given.  Rows need not sum to 1; an all-zero row is an error."""
    p = np.ascontiguousarray(np.asarray(probs, dtype=np.float64))
    if p.ndim != 2:
        raise ValueError("multinomial_counts: probs must be [njobs, K]")
    njobs, k = p.shape
    shots = int(shots)
    up = _uniforms_arg(u, (shots, njobs))
    out = np.zeros((njobs, k), dtype=np.int64)
    _lib.check(_lib.lib().aqc_multinomial_counts(_lib.ptr(p), njobs, k, shots, _u64(seed), _u64(run), _lib.ptr(up),
                                                 _lib.ptr(out)))
    return out


def tomo_fit(counts):
    """[npairs, 4, 4] density matrices fitted to count tables [npairs, 9, 4] (aqc_tomo_fit): linear
    inversion, positive-semidefinite rescaling of the eigenvalues, trace 1."""
    c = np.ascontiguousarray(np.asarray(counts, dtype=np.int64).reshape(-1, 36))
    out = np.zeros((len(c), 4, 4), dtype=np.complex128)
    if len(c):
        _lib.check(_lib.lib().aqc_tomo_fit(_lib.ptr(c), len(c), _lib.ptr(out), 0))
    return out


def pair_tomography(rdms, shots, seed, run=0, method=None, timings=None):
    """Tomography of every pair as one launch chain on device buffers: probabilities of the nine
    settings -> ``shots`` draws per setting (job index pair 9 + s) -> fit -> measure.  Returns
    (rho [npairs, 4, 4], measures [npairs] or None when ``method`` is None).  ``timings``: a dict
    that receives the wall-clock seconds of each stage (every stage ends on a stream
    synchronisation)."""
    import time

    import torch

    r = _rdm_rows(rdms)
    npairs = len(r)
    if npairs == 0:
        return np.zeros((0, 4, 4), dtype=np.complex128), (None if method is None else np.zeros(0))
    l = _lib.lib()
    dev = torch.device("cuda", _lib.device_index())
    drdm = torch.from_numpy(r.view(np.float64)).to(dev)
    probs = torch.empty(npairs * 36, dtype=torch.float64, device=dev)
    counts = torch.empty(npairs * 36, dtype=torch.int64, device=dev)
    rho = torch.empty(npairs * 32, dtype=torch.float64, device=dev)
    meas = torch.empty(npairs, dtype=torch.float64, device=dev)
    # (the library's stream waits for the upload queued on torch's; each call below returns after
    # its own stream synchronisation, so torch's reads afterwards need no further ordering)
    _lib.check(l.aqc_stream_wait(ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def stage(name, call):
        t0 = time.perf_counter()
        _lib.check(call())
        if timings is not None:
            timings[name] = timings.get(name, 0.0) + time.perf_counter() - t0

    stage("probs", lambda: l.aqc_pair_tomo_probs(p(drdm), npairs, p(probs), 1))
    stage("counts", lambda: l.aqc_multinomial_counts(p(probs), npairs * 9, 4, int(shots), _u64(seed), _u64(run), None,
                                                     p(counts)))
    stage("fit", lambda: l.aqc_tomo_fit(p(counts), npairs, p(rho), 1))
    if method is not None:
        code = EM_METHOD_CODES[method]
        stage("measure", lambda: l.aqc_entanglement_measures(p(rho), npairs, code, p(meas), 1))
    out = rho.cpu().numpy().view(np.complex128).reshape(npairs, 4, 4)
    return out, (meas.cpu().numpy() if method is not None else None)


def concurrence_lower_bounds(rdms, shots, seed, run=0, swap=None):
    """The observable concurrence lower bound max(8 f_pmpm - 4 f_ipm, 8 f_pmpm - 4 f_pmi) of every
    pair from three binomial jobs a pair (K = 2, job index pair 3 + c; c = 0 pmpm, 1 pmi, 2 ipm).
    ``swap[pair]``: qubit_1 is the pair's higher qubit (pmi and ipm change places)."""
    pr = concurrence_bound_probs(rdms)
    if len(pr) == 0:
        return np.zeros(0)
    if swap is not None:
        sw = np.asarray(swap, dtype=bool)
        pr[sw] = pr[sw][:, [0, 2, 1]]
    jobs = np.stack([pr.reshape(-1), 1.0 - pr.reshape(-1)], axis=1)
    f = multinomial_counts(jobs, shots, seed, run)[:, 0].reshape(-1, 3) / float(shots)
    return np.maximum(8 * f[:, 0] - 4 * f[:, 2], 8 * f[:, 0] - 4 * f[:, 1])


def copy_batch(dst, src):
    """dst[s] <- src[s] for every state in one launch (per-evaluation reload of a cached MPS)."""
    if len(dst) != len(src):
        raise ValueError("copy_batch: dst and src differ in length")
    if not dst:
        return
    _lib.check(_lib.lib().aqc_mps_copy_batch(_handles(dst), _handles(src), len(dst)))


def overlap_zero_batch(states):
    l = _lib.lib()
    out = np.zeros(2 * len(states))
    _lib.check(l.aqc_mps_overlap_zero_batch(_handles(states), len(states), _lib.ptr(out)))
    return out[0::2] + 1j * out[1::2]


def z_all_batch(states):
    """<Z_i> of every state (rows), one set of launches (aqc_mps_z_all_batch)."""
    if not states:
        return np.zeros((0, 0))
    n = states[0].n
    out = np.zeros(len(states) * n)
    _lib.check(_lib.lib().aqc_mps_z_all_batch(_handles(states), len(states), _lib.ptr(out)))
    return out.reshape(len(states), n)


def pauli_expect_batch(states, terms):
    """<psi_s|P_t|psi_s> as rows per state, one set of launches for every (term, state)
    (aqc_mps_pauli_expect_batch); the states need the same n and capacity.  ``terms`` as
    DeviceMPS.pauli_expect."""
    from . import paulis

    if not states:
        return np.zeros((0, 0))
    codes = paulis.terms_to_codes(terms, states[0].n)
    out = np.zeros(len(states) * len(codes))
    _lib.check(_lib.lib().aqc_mps_pauli_expect_batch(_handles(states), len(states), _lib.ptr(codes), len(codes),
                                                     _lib.ptr(out)))
    return out.reshape(len(states), len(codes))


def z_sum_batch(base, states):
    """sum_i <Z_i> of every state (aqc_mps_z_sum_batch): states copied from ``base`` (unchanged
    since) contract only the sites they rewrote, against environments cached on ``base``."""
    out = np.zeros(len(states))
    if states:
        _lib.check(_lib.lib().aqc_mps_z_sum_batch(base.h, _handles(states), len(states), _lib.ptr(out)))
    return out


def zero_hw1_batch(base, states, amps=False):
    """(<psi|0..0> per state, and with ``amps`` the amplitudes <e_i|psi> as rows) through
    aqc_mps_zero_hw1_batch: states copied from ``base`` (unchanged since) contract only the sites
    they rewrote, against rows cached on ``base``."""
    ns = len(states)
    ov = np.zeros(2 * ns)
    a = np.zeros(2 * ns * (states[0].n if ns else 0)) if amps else None
    if ns:
        _lib.check(_lib.lib().aqc_mps_zero_hw1_batch(base.h, _handles(states), ns, _lib.ptr(ov),
                                                     _lib.ptr(a) if amps else None))
    ovc = ov[0::2] + 1j * ov[1::2]
    if not amps:
        return ovc, None
    return ovc, (a[0::2] + 1j * a[1::2]).reshape(ns, -1)


def amps_hw1_batch(states):
    """Amplitudes <e_i|psi> of every state (rows, complex), one set of launches
    (aqc_mps_amps_hw1_batch)."""
    if not states:
        return np.zeros((0, 0), dtype=complex)
    n = states[0].n
    out = np.zeros(2 * len(states) * n)
    _lib.check(_lib.lib().aqc_mps_amps_hw1_batch(_handles(states), len(states), _lib.ptr(out)))
    return (out[0::2] + 1j * out[1::2]).reshape(len(states), n)


def pair_grads_batch(states, svec, pairs, u0, gens, degs, out=None):
    """Per-state gradient norms for every pair; ``out`` may be a device pointer (int): then the call
    returns once the work is queued and is ordered both ways against torch's current stream -- the
    sweep waits for the torch work queued before it (aqc_stream_wait: a fill of ``out``, the
    previous step's reads of it), and torch's stream waits for the sweep (aqc_stream_join), so
    torch ops on ``out`` (the all-gather, the arg-max) see the scores."""
    l = _lib.lib()
    svec = np.ascontiguousarray(np.asarray(svec, dtype=np.complex128).reshape(-1))
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1))
    u0 = np.ascontiguousarray(np.asarray(u0, dtype=np.complex128).reshape(16))
    gens = np.ascontiguousarray(np.asarray(gens, dtype=np.complex128).reshape(-1))
    degs = np.ascontiguousarray(np.asarray(degs, dtype=np.float64).reshape(-1))
    npairs = len(pairs) // 2
    ngen = len(degs)
    if out is None:
        host = np.zeros((len(states), npairs))
        outp, is_dev = _lib.ptr(host), 0
    else:
        import torch

        host, outp, is_dev = None, ctypes.c_void_p(int(out)), 1
        _lib.check(l.aqc_stream_wait(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    _lib.check(
        l.aqc_pair_grads_batch(
            _handles(states), len(states), _lib.ptr(svec), _lib.ptr(pairs), npairs, _lib.ptr(u0),
            _lib.ptr(gens) if ngen else None, _lib.ptr(degs) if ngen else None, ngen, outp, is_dev,
        )
    )
    if is_dev:
        import torch

        _lib.check(l.aqc_stream_join(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return host


def argmax_rows(scores, prio):
    """Per-row np.argmax(scores * prio) (first maximum) of a device score matrix on libaqchip's
    kernel (aqc_argmax_scaled_batch), ordered both ways against torch's current stream like a
    device-output sweep.  scores: [S, ld] float64 CUDA tensor (the first len(prio) columns are
    scored), prio: [count] float64 CUDA tensor.  Returns ([S] int64 index, [S] float64 score)."""
    import torch

    l = _lib.lib()
    S, ld = scores.shape
    count = prio.shape[0]
    if not (scores.is_cuda and prio.is_cuda and scores.dtype == torch.float64 and prio.dtype == torch.float64
            and scores.is_contiguous() and prio.is_contiguous() and count <= ld):
        raise ValueError("argmax_rows: contiguous float64 CUDA tensors with len(prio) <= scores.shape[1]")
    out = torch.empty((2, S), dtype=torch.float64, device=scores.device)
    cur = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(l.aqc_stream_wait(cur))
    _lib.check(l.aqc_argmax_scaled_batch(ctypes.c_void_p(scores.data_ptr()), ld, ctypes.c_void_p(prio.data_ptr()),
                                         count, S, ctypes.c_void_p(out.data_ptr())))
    _lib.check(l.aqc_stream_join(cur))
    return out[0].to(torch.int64), out[1]
