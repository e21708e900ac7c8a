"""GPU implementations of the ``aqc_research.mps_operations`` helpers the reference calls.

Call sites: aer_mps_backend.py:49-93, gradients.py:60-110, approximate_compiler.py:133-135,198,
adapt_compiler.py:1129.  Every function computes on the device through libaqchip; host numpy
is used only to marshal MPS tensors in and out (Aer format / preprocessed lists).
"""
from __future__ import annotations

import numpy as np

from .circuit import QuantumCircuit, device_ops_array, mps_payload
from .device import DeviceMPS

MAX_CHI_CAP = 1024


def check_mps(obj) -> bool:
    """True for an Aer-format MPS ``(list[(G0, G1)], list[lambda])`` (constants.py:17)."""
    try:
        gam, lam = obj
        if not isinstance(gam, (list, tuple)) or not isinstance(lam, (list, tuple)):
            return False
        if len(lam) != len(gam) - 1:
            return False
        for g in gam:
            if len(g) != 2 or np.asarray(g[0]).ndim != 2:
                return False
        return True
    except (TypeError, ValueError):
        return False


def _preprocess_mps(qiskit_mps):
    """Gamma_i diag(lambda_i) for i < n-1 -> list of (2, chi_l, chi_r) arrays."""
    gam, lam = qiskit_mps
    out = []
    for i, (a, b) in enumerate(gam):
        t = np.stack([np.asarray(a, dtype=complex), np.asarray(b, dtype=complex)])
        if i < len(gam) - 1:
            t = t * np.asarray(lam[i])[None, None, :]
        out.append(t)
    return out


# Unbounded runs (max_chi None, the reference default) grow their capacity on demand, as Aer's MPS
# grows its bonds: a replay starts at the smallest power of two >= 64 that holds the loaded MPS and
# whatever an earlier replay on as many qubits needed, and a capacity overflow re-runs it at twice
# the capacity (up to min(MAX_CHI_CAP, 2^(n/2))).  Until round 4 they took that upper bound at once,
# and every kernel whose work follows the capacity -- the candidate sweep's cap x cap transfer
# matrices, whole-state copies -- paid for 512 at bond 64 (~100 ms per sweep, 0.4 ms at 64).
# The learned capacities (n -> capacity) belong to a simulator -- the backend's MPSSimulator, whose
# compiler resets them at the start of each compile (one process-wide table made every
# later compile on n qubits start at the largest capacity any earlier run had needed); calls without
# a simulator share the module table below.
_UNBOUNDED_CAP = {}


def learned_capacities(sim=None) -> dict:
    """The n -> capacity table of unbounded replays driven by ``sim`` (created on first use)."""
    if sim is None:
        return _UNBOUNDED_CAP
    table = getattr(sim, "aqc_learned_cap", None)
    if table is None:
        table = {}
        try:
            sim.aqc_learned_cap = table
        except AttributeError:  # (a simulator object that takes no attributes: the shared table)
            return _UNBOUNDED_CAP
    return table


def _full_cap(n):
    return min(MAX_CHI_CAP, 2 ** (n // 2))


def chi_cap_for(n, max_chi, loaded_max=1, learned=None):
    if max_chi:
        cap = int(max_chi)
    else:
        table = _UNBOUNDED_CAP if learned is None else learned
        full = _full_cap(n)
        want = max(table.get(n, 0), int(loaded_max), min(64, full))
        cap = 1
        while cap < want:
            cap <<= 1
        cap = min(cap, full)
    cap = max(cap, int(loaded_max), 1)
    if cap > MAX_CHI_CAP:
        raise NotImplementedError(f"bond dimension {cap} exceeds the supported maximum {MAX_CHI_CAP}")
    return cap


def is_capacity_error(e) -> bool:
    return "capacity (chi_cap) exceeded" in str(e)


def grow_capacity(n, max_chi, cap, learned=None) -> bool:
    """After a capacity overflow at ``cap``: raise the unbounded capacity for n qubits to 2 cap in
    ``learned`` (default: the module table; chi_cap_for returns it from now on); False when the run
    is bounded or already at the limit."""
    if max_chi or cap >= _full_cap(n):
        return False
    table = _UNBOUNDED_CAP if learned is None else learned
    table[n] = max(table.get(n, 0), min(2 * cap, _full_cap(n)))
    return True


def apply_checked(state: DeviceMPS, ops):
    """state.apply(ops), re-raising a bond-capacity overflow with the remedy: an unbounded run
    (max_chi None, the reference default) is capped at MAX_CHI_CAP on the device, where Aer's MPS
    would keep growing."""
    from ._lib import AqcError

    try:
        state.apply(ops)
    except AqcError as e:
        if "capacity" in str(e):
            raise AqcError(f"{e} -- this MPS needs a bond dimension above chi_cap = {state.chi_cap} (the device "
                           f"engine supports at most {MAX_CHI_CAP}); set max_chi (mps_sim_with_args(max_chi=...)) "
                           f"to truncate as Aer's matrix_product_state_max_bond_dimension does") from e
        raise


def _sim_options(sim):
    if sim is None:
        return 1e-16, None
    o = sim.options
    return o.matrix_product_state_truncation_threshold, o.matrix_product_state_max_bond_dimension


def device_mps_from_circuit(circuit: QuantumCircuit, sim=None, trunc_thr=None, out: DeviceMPS | None = None):
    """Run ``circuit`` (optionally led by set_matrix_product_state) on the device MPS engine."""
    thr, max_chi = _sim_options(sim)
    if trunc_thr is not None:
        thr = trunc_thr
    n = circuit.num_qubits
    start = 0
    loaded = None
    if len(circuit.data) and circuit.data[0].operation.name == "set_matrix_product_state":
        loaded = mps_payload(circuit.data[0].operation)
        start = 1
    lmax = max(np.asarray(a).shape[1] for a, _ in loaded[0]) if loaded is not None else 1
    ops = device_ops_array(circuit, start)
    learned = learned_capacities(sim)
    while True:
        cap = chi_cap_for(n, max_chi, lmax, learned)
        if out is None or out.n != n or out.chi_cap < cap:
            out = DeviceMPS(n, cap, thr, max_chi)
        else:
            out.set_truncation(thr, max_chi)
        if loaded is not None:
            out.load_aer(loaded)
        else:
            out.load_aer(zero_aer_mps(n))
        try:
            apply_checked(out, ops)
            break
        except Exception as e:  # an unbounded run outgrew its capacity: again at twice the capacity
            if not (is_capacity_error(e) and grow_capacity(n, max_chi, out.chi_cap, learned)):
                raise
    out.sort()
    return out


def zero_aer_mps(n):
    g = (np.array([[1.0 + 0j]]), np.array([[0.0 + 0j]]))
    return [tuple(x.copy() for x in g) for _ in range(n)], [np.ones(1) for _ in range(n - 1)]


def mps_from_circuit(circuit: QuantumCircuit, return_preprocessed=False, sim=None, trunc_thr=None,
                     print_log_data=False):
    """aqc_research ``mps_from_circuit``: Aer tuple, or the preprocessed list if requested."""
    d = device_mps_from_circuit(circuit, sim, trunc_thr)
    return d.preprocessed() if return_preprocessed else d.to_aer()


def _as_device(mps, already_preprocessed, like: DeviceMPS | None = None):
    if isinstance(mps, DeviceMPS):
        return mps
    if isinstance(mps, DevicePreprocessedMPS):
        return mps.device
    if not already_preprocessed and check_mps(mps):
        aer = mps
    else:
        # preprocessed list: load as Gammas with unit lambdas (A_i = Gamma_i * 1)
        aer = ([(np.asarray(t[0]), np.asarray(t[1])) for t in mps], [np.ones(np.asarray(t).shape[2]) for t in mps[:-1]])
    n = len(aer[0])
    lmax = max(np.asarray(a).shape[1] for a, _ in aer[0])
    cap = like.chi_cap if like is not None and like.chi_cap >= lmax else chi_cap_for(n, None, lmax)
    d = DeviceMPS(n, cap)
    d.load_aer(aer)
    return d


def _is_zero_state(mps, pre):
    """Host MPS equal to |0...0> (every site a (2,1,1) tensor [1, 0]).  Device-backed states
    answer False: the check is only a fast path, and the general dot gives the same value."""
    if isinstance(mps, (DeviceMPS, DevicePreprocessedMPS)):
        return False
    try:
        sites = mps if pre else _preprocess_mps(mps)
        return all(np.shape(t) == (2, 1, 1) and t[0, 0, 0] == 1 and t[1, 0, 0] == 0 for t in sites)
    except (TypeError, ValueError, IndexError):
        return False


def _to_aer_like(mps, pre):
    if isinstance(mps, DevicePreprocessedMPS):
        return mps.device.to_aer(), False
    if isinstance(mps, DeviceMPS):
        return mps.to_aer(), False
    return mps, pre


def mps_dot(a, b, already_preprocessed=False):
    """<a|b>, conjugating ``a`` (pinned by test_gradients.py:39-73)."""
    if _is_zero_state(b, already_preprocessed):
        return _as_device(a, already_preprocessed).overlap_zero()
    if _is_zero_state(a, already_preprocessed):
        return np.conj(_as_device(b, already_preprocessed).overlap_zero())
    da = _as_device(a, already_preprocessed)
    db = _as_device(b, already_preprocessed)
    if da.chi_cap != db.chi_cap:
        big = max(da.chi_cap, db.chi_cap)
        if da.chi_cap != big:
            src, pre = _to_aer_like(a, already_preprocessed)
            da = _as_device(src, pre, db)
        else:
            src, pre = _to_aer_like(b, already_preprocessed)
            db = _as_device(src, pre, da)
    return da.dot(db)


def mps_expectation(mps, operator, qubit, already_preprocessed=False):
    d = _as_device(mps, already_preprocessed)
    if operator == "Z":
        return float(d.z_all()[qubit])
    if operator not in ("I", "X", "Y"):
        raise ValueError(f"mps_expectation: operator must be one of I, X, Y, Z, got {operator!r}")
    if not 0 <= int(qubit) < d.n:
        raise ValueError(f"mps_expectation: qubit {qubit} out of range for {d.n} qubits")
    from .paulis import CODES

    codes = np.zeros((1, d.n), dtype=np.uint8)
    codes[0, int(qubit)] = CODES[operator]
    return float(d.pauli_expect(codes)[0])


def extract_amplitude(mps, index, already_preprocessed=False):
    d = _as_device(mps, already_preprocessed)
    n = d.n
    if index == 0:
        return np.conj(d.overlap_zero())
    if index & (index - 1) == 0:
        i = int(index).bit_length() - 1
        return complex(d.amps_hw1()[i])
    basis = zero_aer_mps(n)
    for q in range(n):
        if (index >> q) & 1:
            basis[0][q] = (np.array([[0.0 + 0j]]), np.array([[1.0 + 0j]]))
    bd = DeviceMPS(n, d.chi_cap)
    bd.load_aer(basis)
    return bd.dot(d)


class DevicePreprocessedMPS(list):
    """A preprocessed MPS (list of (2, chi_l, chi_r) host arrays, what the reference's
    ``AerMPSBackend.evaluate_circuit`` returns, aer_mps_backend.py:76-78) that also carries a device
    snapshot of the same state.  ``partial_trace`` and the other helpers here use the snapshot
    instead of uploading the host tensors again; the host arrays are fetched lazily."""

    def __init__(self, device: DeviceMPS):
        super().__init__()
        self._device = device
        self._filled = False
        self._rdms = None

    def _fill(self):
        if not self._filled:
            self._filled = True
            super().extend(self._device.preprocessed())

    # every read of the list contents goes through _fill
    def __len__(self):
        return self._device.n

    def __getitem__(self, i):
        self._fill()
        return super().__getitem__(i)

    def __iter__(self):
        self._fill()
        return super().__iter__()

    def __reduce__(self):  # pickles (checkpoints) as the plain host list
        self._fill()
        return (list, (list(super().__iter__()),))

    @property
    def device(self) -> DeviceMPS:
        return self._device

    def all_pair_rdms(self):
        """{(a, b): 4x4} for every a < b, computed in one batched device sweep and memoised."""
        if self._rdms is None:
            n = self._device.n
            pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
            r = self._device.pair_rdms(pairs) if pairs else np.zeros((0, 4, 4), complex)
            self._rdms = {p: r[k] for k, p in enumerate(pairs)}
        return self._rdms

    def pair_rdms(self, pairs):
        return self._device.pair_rdms(pairs)


def _filling(name):
    """list method ``name`` run on the filled storage (C-level list methods read the internal
    array directly, which is empty until the first fill)."""
    base = getattr(list, name)

    def method(self, *args, **kwargs):
        self._fill()
        return base(self, *args, **kwargs)

    method.__name__ = name
    method.__doc__ = base.__doc__
    return method


for _name in ("copy", "__eq__", "__ne__", "__lt__", "__le__", "__gt__", "__ge__", "__reversed__", "__add__",
              "__mul__", "__rmul__", "__contains__", "index", "count", "__repr__", "append", "extend", "insert",
              "pop", "remove", "sort", "reverse", "__setitem__", "__delitem__", "__iadd__", "__imul__", "clear"):
    setattr(DevicePreprocessedMPS, _name, _filling(_name))
del _name


def _dpm_radd(self, other):  # [..] + mps: Python tries a subclass's reflected method first
    self._fill()
    return list(other) + list(super(DevicePreprocessedMPS, self).__iter__())


DevicePreprocessedMPS.__radd__ = _dpm_radd

# partial_trace on a host list: every pair's RDM from one device sweep, kept for the following
# calls on the same list (the reference's ISL loop calls it once per pair).  Keyed on the list and
# the identities of its site tensors (a site replaced in place starts a new sweep; tensors mutated
# in place are not detected); the device copy of the state is released as soon as the RDMs are
# read back.
_pt_cache = {"obj": None, "sites": None, "rdms": None}


def partial_trace(mps, qubits, already_preprocessed=False):
    """aqc_research ``partial_trace(mps, [q1, q2], already_preprocessed)``: the 4x4 reduced density
    matrix of two qubits (row index 2*bit(max) + bit(min), as qiskit's partial trace orders the
    kept qubits), called per coupling-map pair by the reference's ISL sweep
    (entanglement_measures.py:76-79, adapt_compiler.py:964-974).  The first call on a state computes
    every pair's RDM in one device sweep (aqc_mps_pair_rdms); the following calls on the same state
    are lookups."""
    q = [int(x) for x in qubits]
    if len(q) != 2 or q[0] == q[1]:
        raise ValueError("partial_trace keeps exactly two distinct qubits")
    key = (min(q), max(q))
    if isinstance(mps, DevicePreprocessedMPS):
        return mps.all_pair_rdms()[key].copy()
    sites = _site_objects(mps)
    old = _pt_cache["sites"]
    if (_pt_cache["obj"] is not mps or sites is None or old is None or len(old) != len(sites)
            or any(a is not b for a, b in zip(old, sites))):
        dev = _as_device(mps, already_preprocessed)
        n = dev.n
        pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
        r = dev.pair_rdms(pairs)
        del dev
        _pt_cache.update(obj=mps, sites=sites, rdms={p: r[k] for k, p in enumerate(pairs)})
    return _pt_cache["rdms"][key].copy()


def _site_objects(mps):
    """The objects a host MPS holds (a preprocessed list of site tensors, or Aer's (gammas,
    lambdas) pair), held by the cache and compared by identity: replacing any of them invalidates
    the partial-trace cache."""
    try:
        if isinstance(mps, tuple) and len(mps) == 2:
            return tuple(x for part in mps for x in part)
        return tuple(mps)
    except TypeError:
        return None


def mps_to_vector(mps, already_preprocessed=False):
    """Dense statevector of a (small) MPS, evaluated amplitude by amplitude on the device."""
    d = _as_device(mps, already_preprocessed)
    return np.array([extract_amplitude(d, i) for i in range(2 ** d.n)])


def mps_from_vector(psi, trunc_thr=1e-16, max_chi=None):
    """Aer-format MPS ``(gam, lam)`` of a dense statevector (index bit q = qubit q; site q = qubit q,
    the convention ``mps_to_vector`` inverts), by successive SVDs on the host.  A format conversion
    at the ingestion boundary, like ``DeviceMPS.load_aer``: it runs once, to make a state such as
    ``calculate_ground_state``'s a compile target, and sits on no evaluation path.

    Vidal form, psi = Gamma_0 lam_0 Gamma_1 ... lam_{n-2} Gamma_{n-1}: every bond's lambdas descend,
    those with lambda^2 <= ``trunc_thr`` are dropped (the largest is always kept) and at most
    ``max_chi`` are kept.  The kept lambdas are not rescaled: a truncated result has the norm of what
    was kept."""
    psi = np.asarray(psi, dtype=np.complex128).reshape(-1)
    n = int(psi.size).bit_length() - 1
    if n < 1 or psi.size != 1 << n:
        raise ValueError(f"mps_from_vector: the vector needs 2^n entries with n >= 1, got {psi.size}")
    if max_chi is not None and int(max_chi) < 1:
        raise ValueError("mps_from_vector: max_chi must be at least 1")
    # axis q of the tensor = qubit q (the dense index has qubit n-1 as its slowest bit)
    rest = psi.reshape((2,) * n).transpose(tuple(range(n - 1, -1, -1))).reshape(1, -1)
    gam, lam = [], []
    prev = np.ones(1)
    for _ in range(n - 1):
        chi_l = rest.shape[0]
        u, s, vh = np.linalg.svd(rest.reshape(chi_l * 2, -1), full_matrices=False)
        keep = max(1, int(np.count_nonzero(s * s > trunc_thr)))
        if max_chi is not None:
            keep = min(keep, int(max_chi))
        u, s, vh = u[:, :keep], s[:keep], vh[:keep]
        g = u.reshape(chi_l, 2, keep) / prev[:, None, None]
        gam.append((np.ascontiguousarray(g[:, 0, :]), np.ascontiguousarray(g[:, 1, :])))
        lam.append(s.copy())
        rest = s[:, None] * vh
        prev = s
    g = rest.reshape(rest.shape[0], 2, 1) / prev[:, None, None]
    gam.append((np.ascontiguousarray(g[:, 0, :]), np.ascontiguousarray(g[:, 1, :])))
    return gam, lam
