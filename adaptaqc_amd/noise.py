"""Noise models for the shot backend: one-qubit Kraus channels, products of two of them, and correlated
two-qubit Kraus sets (``QuantumError.two_qubit``, ``depolarizing_error(p, 2)``, two-letter
``pauli_error`` labels) attached to instruction names, and the flat program the device's trajectory samplers run (csrc/traj.hip, aqc_sv_traj_sample, on a statevector;
csrc/mps_traj.hip, aqc_mps_traj_sample, on an MPS), and the POVM effects of a noisy Pauli-basis
readout for noisy pair tomography (``readout_effects``, aqc_sv_traj_pair_tomo / aqc_mps_traj_pair_tomo)
and for the noisy Pauli readout of every term of an operator from each trajectory
(aqc_sv_traj_pauli_counts on statevector trajectories, aqc_mps_traj_pauli_counts on MPS trajectories;
``SamplingSimulator.pauli_counts``, the MPS engine with ``mps_pauli_readout=True``).

Stands in for the parts of ``qiskit_aer.noise`` that the reference uses
(``execute_kwargs={'noise_model': NoiseModel, 'shots': ...}``, approximate_compiler.py:93;
``thermal_relaxation_error`` and ``NoiseModel`` in circuit_operations_running.py:72-109).  A noisy
shot is one quantum trajectory: after every gate that carries an error, one Kraus operator of each
affected qubit's channel is drawn with probability |K_k psi|^2 and applied.  The law of the counts is
that of the channel; the individual trajectories depend on the Kraus decomposition chosen here.

A correlated error follows a two-qubit gate as one event: one of its 1-16 4x4 operators is drawn with
probability |K_k psi|^2 and applied to both qubits (matrix index 2 b(second listed qubit) + b(first
listed qubit), a two-qubit gate row's and Aer's convention).  It runs on the statevector trajectory
engine (up to 24 qubits), and on the MPS trajectory engine where the caller opts in
(``SamplingSimulator(..., mps_trajectories=True, mps_correlated=True)``, ``correlated=True`` on the
``device.mps_trajectory_*`` wrappers); without the opt-in the MPS routes refuse it by name.  There a
product-unitary error (every operator a scalar times a product of two unitaries: every Pauli channel,
``depolarizing_error(p, 2)``) costs two one-site updates and no SVD; any other is a two-site update whose
operator is chosen on the device from the pair's reduced density matrix.

The same flat program also runs exactly: up to 13 qubits the density-matrix engine (csrc/dm.hip,
``device.DeviceDM``, ``backends.DensityMatrixSimulator`` / ``DensityMatrixBackend``) evolves rho by it --
a gate row as U rho U^dag, a Kraus row or group as sum_k K_k rho K_k^dag -- and reads the cost, the RDMs,
the Pauli values (with ``readout_effects``) and the outcome distribution off rho with no shot noise.

Out of scope: two errors on one instruction, readout-error matrices, reset, errors on gates of three or
more qubits.
"""
import numpy as np

_TOL = 1e-9
_CORRELATED_ON_MPS = ("correlated two-qubit errors run on the statevector trajectory engine (at most 24 qubits) "
                      "unless the MPS trajectory engine is told to take them: build the simulator with "
                      "mps_trajectories=True, mps_correlated=True, or pass correlated=True to the "
                      "device.mps_trajectory_* call")
_PAULIS = {
    "I": np.eye(2, dtype=complex),
    "X": np.array([[0, 1], [1, 0]], dtype=complex),
    "Y": np.array([[0, -1j], [1j, 0]], dtype=complex),
    "Z": np.diag([1.0 + 0j, -1.0]),
}


class QuantumError:
    """A one-qubit channel held as 1-4 Kraus matrices, a two-qubit product of two such channels
    (``expand`` / ``tensor``), or a correlated two-qubit channel of 1-16 4x4 Kraus matrices
    (``two_qubit``).  ``kraus``: a list of 2x2 complex matrices with sum K^dag K = I within 1e-9."""

    def __init__(self, kraus):
        mats = [np.array(k, dtype=complex) for k in kraus]
        if mats and all(m.shape == (4, 4) for m in mats):
            raise NotImplementedError("QuantumError(kraus) takes one-qubit matrices: build a correlated two-qubit "
                                      "error with QuantumError.two_qubit(kraus), a product error with expand() / "
                                      "tensor()")
        if not 1 <= len(mats) <= 4 or any(m.shape != (2, 2) for m in mats):
            raise ValueError("QuantumError: 1 to 4 Kraus matrices of shape 2x2")
        total = sum(m.conj().T @ m for m in mats)
        if not np.all(np.isfinite(total)) or np.max(np.abs(total - np.eye(2))) > _TOL:
            raise ValueError("QuantumError: sum K^dag K is not the identity")
        self.kraus = mats
        self.pair = None  # (channel of the gate's first listed qubit, of its second)
        self._identity = all(np.max(np.abs(k - np.trace(k) / 2 * np.eye(2))) <= 1e-12 for k in mats)

    @classmethod
    def two_qubit(cls, kraus):
        """A correlated two-qubit channel: 1 to 16 complex 4x4 matrices with sum K^dag K = I within 1e-9,
        matrix index 2 b(second listed qubit) + b(first listed qubit) of the gate it follows."""
        mats = [np.array(k, dtype=complex) for k in kraus]
        if not 1 <= len(mats) <= 16 or any(m.shape != (4, 4) for m in mats):
            raise ValueError("QuantumError.two_qubit: 1 to 16 Kraus matrices of shape 4x4")
        if not all(np.all(np.isfinite(m)) for m in mats):
            raise ValueError("QuantumError.two_qubit: a matrix entry is not finite")
        if np.max(np.abs(sum(m.conj().T @ m for m in mats) - np.eye(4))) > _TOL:
            raise ValueError("QuantumError.two_qubit: sum K^dag K is not the identity")
        e = cls.__new__(cls)
        e.kraus = mats
        e.pair = None
        e._identity = all(np.max(np.abs(k - np.trace(k) / 4 * np.eye(4))) <= 1e-12 for k in mats)
        return e

    @classmethod
    def _product(cls, first, second):
        if first.num_qubits != 1 or second.num_qubits != 1:
            raise NotImplementedError("only products of two one-qubit errors are supported")
        e = cls.__new__(cls)
        e.kraus = None
        e.pair = (first, second)
        e._identity = first._identity and second._identity
        return e

    @property
    def correlated(self):
        """True for a two-qubit channel held as 4x4 Kraus matrices (``two_qubit``)."""
        return self.pair is None and self.kraus[0].shape == (4, 4)

    @property
    def num_qubits(self):
        return 2 if self.pair is not None or self.correlated else 1

    def expand(self, other):
        """The two-qubit product error with ``self`` on the gate's first listed qubit."""
        return QuantumError._product(self, other)

    def tensor(self, other):
        """The two-qubit product error with ``self`` on the gate's second listed qubit."""
        return QuantumError._product(other, self)

    def is_identity(self):
        """True when the channel is the identity map: every Kraus matrix a multiple of I."""
        return self._identity

    def no_jump_weight(self):
        """Tr(K_0^dag K_0) / 2 (the product over both qubits for a product error; Tr(K_0^dag K_0) / 4
        for a correlated one)."""
        if self.pair is not None:
            return self.pair[0].no_jump_weight() * self.pair[1].no_jump_weight()
        return float(np.trace(self.kraus[0].conj().T @ self.kraus[0]).real / len(self.kraus[0]))

    def __repr__(self):
        if self.pair is not None:
            return f"QuantumError(product of {self.pair[0]!r} and {self.pair[1]!r})"
        if self.correlated:
            return f"QuantumError({len(self.kraus)} Kraus, 2 qubits, correlated)"
        return f"QuantumError({len(self.kraus)} Kraus, 1 qubit)"


def thermal_relaxation_error(t1, t2, time):
    """Relaxation towards |0> (excited-state population 0) for ``time``: with gamma = 1 - e^(-time/t1),
    e2 = e^(-time/t2) and lambda = 1 - gamma - e2^2, K0 = diag(1, e2), K1 = sqrt(gamma) |0><1|,
    K2 = sqrt(lambda) |1><1|.  The map is rho11 -> e^(-time/t1) rho11, rho01 -> e^(-time/t2) rho01 --
    Aer's thermal_relaxation_error for every t2 <= 2 t1."""
    t1, t2, time = float(t1), float(t2), float(time)
    if not (t1 > 0 and t2 > 0):
        raise ValueError("thermal_relaxation_error: t1 and t2 must be positive")
    if not time >= 0:
        raise ValueError("thermal_relaxation_error: time must not be negative")
    if t2 > 2 * t1:
        raise ValueError("thermal_relaxation_error: t2 must not exceed 2 t1")
    gamma = -np.expm1(-time / t1)
    e2 = np.exp(-time / t2)
    lam = max(0.0, 1.0 - gamma - e2 * e2)
    return QuantumError([np.diag([1.0, e2]), np.sqrt(gamma) * np.array([[0, 1], [0, 0]]),
                         np.sqrt(lam) * np.diag([0.0, 1.0])])


def amplitude_damping_error(gamma):
    gamma = float(gamma)
    if not 0 <= gamma <= 1:
        raise ValueError("amplitude_damping_error: gamma must lie in [0, 1]")
    return QuantumError([np.diag([1.0, np.sqrt(1 - gamma)]), np.sqrt(gamma) * np.array([[0, 1], [0, 0]])])


def phase_damping_error(lam):
    lam = float(lam)
    if not 0 <= lam <= 1:
        raise ValueError("phase_damping_error: lam must lie in [0, 1]")
    return QuantumError([np.diag([1.0, np.sqrt(1 - lam)]), np.sqrt(lam) * np.diag([0.0, 1.0])])


def pauli_error(terms):
    """[(label, probability), ...] over the one-qubit labels I, X, Y, Z, or over two-letter labels
    (all of length 2: a correlated two-qubit error, the rightmost letter on the gate's first listed
    qubit); the probabilities sum to 1."""
    terms = list(terms)
    width = {len(label) if isinstance(label, str) else 0 for label, _ in terms}
    if width == {2}:
        return _pauli_error2(terms)
    if len(width) > 1 and width <= {1, 2}:
        raise ValueError("pauli_error: labels of one length, 1 or 2")
    probs = {}
    for label, p in terms:
        if label not in _PAULIS:
            raise ValueError("pauli_error: one-qubit labels I, X, Y, Z")
        if not p >= 0:
            raise ValueError("pauli_error: probabilities must not be negative")
        probs[label] = probs.get(label, 0.0) + float(p)
    if not probs or abs(sum(probs.values()) - 1) > _TOL:
        raise ValueError("pauli_error: probabilities must sum to 1")
    return QuantumError([np.sqrt(p) * _PAULIS[label] for label, p in probs.items()])


def _pauli_error2(terms):
    probs = {}
    for label, p in terms:
        if label[0] not in _PAULIS or label[1] not in _PAULIS:
            raise ValueError("pauli_error: two-qubit labels of the letters I, X, Y, Z")
        if not p >= 0:
            raise ValueError("pauli_error: probabilities must not be negative")
        probs[label] = probs.get(label, 0.0) + float(p)
    if abs(sum(probs.values()) - 1) > _TOL:
        raise ValueError("pauli_error: probabilities must sum to 1")
    # the left letter is the second listed qubit, the high bit of the matrix index
    return QuantumError.two_qubit([np.sqrt(p) * np.kron(_PAULIS[label[0]], _PAULIS[label[1]])
                                   for label, p in probs.items()])


def depolarizing_error(p, num_qubits=1):
    """rho -> (1 - p) rho + p I / 2 on one qubit (0 <= p <= 4/3), as Aer parametrises it.  With
    ``num_qubits=2`` the correlated rho -> (1 - p) rho + p I / 4 on two qubits (0 <= p <= 16/15): the
    sixteen two-qubit Paulis, II first with weight 1 - 15 p / 16, p / 16 each for the others."""
    p = float(p)
    if num_qubits == 2:
        if not 0 <= p <= 16 / 15:
            raise ValueError("depolarizing_error: p must lie in [0, 16/15] on two qubits")
        rest = [a + b for a in "IXYZ" for b in "IXYZ"][1:]
        return pauli_error([("II", max(0.0, 1 - 15 * p / 16))] + [(label, p / 16) for label in rest])
    if num_qubits != 1:
        raise ValueError("depolarizing_error: num_qubits must be 1 or 2")
    if not 0 <= p <= 4 / 3:
        raise ValueError("depolarizing_error: p must lie in [0, 4/3]")
    return pauli_error([("I", 1 - 3 * p / 4), ("X", p / 4), ("Y", p / 4), ("Z", p / 4)])


def _names(instructions):
    names = [instructions] if isinstance(instructions, str) else list(instructions)
    if not names or not all(isinstance(n, str) for n in names):
        raise ValueError("instructions: a name or a list of names")
    return names


class NoiseModel:
    """Errors looked up by instruction name (and qubits).  A gate with no error attached is noiseless;
    a one-qubit error attached to a two-qubit instruction acts on both its qubits."""

    def __init__(self):
        self._all = {}    # name -> QuantumError
        self._local = {}  # (name, qubits) -> QuantumError

    def add_all_qubit_quantum_error(self, error, instructions):
        self._add(self._all, error, _names(instructions))

    def add_quantum_error(self, error, instructions, qubits):
        qubits = tuple(int(q) for q in qubits)
        self._add(self._local, error, [(n, qubits) for n in _names(instructions)])

    @staticmethod
    def _add(table, error, keys):
        if not isinstance(error, QuantumError):
            raise TypeError("expected a QuantumError")
        for key in keys:
            if key in table:
                raise NotImplementedError(f"{key} already carries an error: composing errors is not supported")
            table[key] = error

    def instructions(self):
        """{name: error} of the all-qubit errors."""
        return dict(self._all)

    def channels(self, name, qubits):
        """The channels that follow instruction ``name`` on ``qubits``: one-qubit channels as
        [(qubit, error)] in the gate's qubit order, a correlated error on a two-qubit instruction as the
        single entry [((qa, qb), error)] with the qubits in the gate's listed order (identity channels
        left out); [] for a noiseless instruction."""
        qubits = tuple(int(q) for q in qubits)
        error = self._local.get((name, qubits), self._all.get(name))
        if error is None:
            return []
        if len(qubits) > 2:
            raise NotImplementedError(f"an error on the {len(qubits)}-qubit gate {name!r} is not supported")
        if error.num_qubits == 1:
            per_qubit = [error] * len(qubits)
        elif len(qubits) == 2 and error.correlated:
            return [] if error.is_identity() else [(qubits, error)]
        elif len(qubits) == 2:
            per_qubit = list(error.pair)
        else:
            raise ValueError(f"a two-qubit error is attached to the one-qubit instruction {name!r}")
        return [(q, e) for q, e in zip(qubits, per_qubit) if not e.is_identity()]

    def __repr__(self):
        return f"NoiseModel(all-qubit: {sorted(self._all)}, local: {sorted(self._local)})"


def kraus_row(error, qubit):
    """One aqc_op_t Kraus row (flags AQC_OP_KRAUS1): q0 the qubit, q1 the number of operators,
    m[8k .. 8k+7] the k-th 2x2 matrix."""
    from . import _lib

    row = np.zeros(1, dtype=_lib.OP_DTYPE)
    row["nq"], row["q0"], row["q1"], row["flags"] = 1, int(qubit), len(error.kraus), _lib.OP_KRAUS1
    row["m"][0, : 8 * len(error.kraus)] = np.stack(error.kraus).reshape(-1).view(np.float64)
    return row


def kraus2_rows(error, qubits):
    """The group of aqc_op_t rows of a correlated error (flags AQC_OP_KRAUS2 | k << 8 | nk << 16): row k
    holds the 4x4 operator K_k in m, q0 and q1 the gate's qubits in listed order."""
    from . import _lib

    nk = len(error.kraus)
    rows = np.zeros(nk, dtype=_lib.OP_DTYPE)
    rows["nq"], rows["q0"], rows["q1"] = 2, int(qubits[0]), int(qubits[1])
    rows["flags"] = _lib.OP_KRAUS2 | (np.arange(nk) << 8) | (nk << 16)
    rows["m"] = np.stack(error.kraus).reshape(nk, 16).view(np.float64)
    return rows


def has_correlated_rows(rows):
    """True when the program holds a correlated two-qubit Kraus group (AQC_OP_KRAUS2 rows)."""
    from . import _lib

    return bool(np.any((np.asarray(rows["flags"]) & 0xFF) == _lib.OP_KRAUS2))


def count_events(rows):
    """The events of a program: its one-qubit Kraus rows plus its correlated groups (their first rows)."""
    from . import _lib

    flags = np.asarray(rows["flags"])
    return int(np.count_nonzero(flags == _lib.OP_KRAUS1) + np.count_nonzero((flags & 0xFFFF) == _lib.OP_KRAUS2))


_H = np.array([[1, 1], [1, -1]], dtype=complex) / np.sqrt(2)
_SDG = np.diag([1.0 + 0j, -1j])


def readout_effects(n, noise_model):
    """float64 [n, 3, 2, 4]: the POVM effects of a noisy Pauli-basis measurement of every qubit, as
    aqc_sv_traj_pair_tomo and aqc_mps_traj_pair_tomo take them -- entry [q, b, o] holds (E00, E11, Re E01, Im E01) of the
    Hermitian 2x2 effect of qubit q, basis b (0 X, 1 Y, 2 Z), outcome o (0 the +1 eigenstate).

    The reference measures basis Y by appending ``sdg``, ``h``, ``measure`` (X: ``h``, ``measure``;
    Z: ``measure``), and under a noise model each of them carries the error attached to it on
    ``(q,)``.  All are one-qubit operations on the measured qubit, so they fold into
    E = Sdg^dag A_sdg( H^dag A_h( A_meas(|o><o|) ) H ) Sdg, with A_x(E) = sum_k K_k^dag E K_k the adjoint
    of the channel ``noise_model.channels(x, (q,))`` (H / A_h for X and Y only, Sdg / A_sdg for Y only).
    ``None`` or a model without these errors gives the projectors onto the Pauli eigenvectors."""

    def adjoint(name, q, e):
        if noise_model is None:
            return e
        for _, error in noise_model.channels(name, (q,)):
            e = sum(k.conj().T @ e @ k for k in error.kraus)
        return e

    out = np.zeros((int(n), 3, 2, 4))
    for q in range(int(n)):
        for b in range(3):
            for o in range(2):
                e = np.zeros((2, 2), dtype=complex)
                e[o, o] = 1.0
                e = adjoint("measure", q, e)
                if b < 2:
                    e = _H.conj().T @ adjoint("h", q, e) @ _H
                if b == 1:
                    e = _SDG.conj().T @ adjoint("sdg", q, e) @ _SDG
                out[q, b, o] = (e[0, 0].real, e[1, 1].real, e[0, 1].real, e[0, 1].imag)
    return out


def candidate_superoperator(matrix, name, qubit, noise_model):
    """The 4x4 superoperator S of the one-qubit gate ``matrix`` followed by the channels that
    ``noise_model`` attaches to instruction ``name`` on ``(qubit,)``: S[r' + 2 c', r + 2 c] =
    sum_k (K_k V)[r', r] conj((K_k V)[c', c]), the local index of the density-matrix engine's steps
    (``DeviceDM.transition``).  ``noise_model`` None, or a noiseless instruction: the lifted gate."""
    v = np.asarray(matrix, dtype=complex).reshape(2, 2)
    s = np.kron(v.conj(), v)
    if noise_model is not None:
        for _, error in noise_model.channels(name, (int(qubit),)):
            s = sum(np.kron(k.conj(), k) for k in error.kraus) @ s
    return s


def _pair_frame(matrix, qubits, lo):
    """A 2x2 operator on one of a pair's qubits, or a 4x4 one on both (index 2 b(second listed) + b(first
    listed)), as a 4x4 matrix at the pair's index 2 bit_hi + bit_lo."""
    m = np.asarray(matrix, dtype=complex)
    if m.shape == (2, 2):
        return np.kron(np.eye(2), m) if qubits[0] == lo else np.kron(m, np.eye(2))
    if qubits[0] == lo:
        return m
    swap = [0, 2, 1, 3]
    return m[np.ix_(swap, swap)]


def layer_superoperator(circuit, qubits, noise_model):
    """The 16x16 superoperator of the two-qubit ``circuit`` placed on ``qubits`` (its qubit 0 on
    ``qubits[0]``): its gates composed with every channel that ``noise_model.channels(name, qubits)``
    attaches to them, in ``trajectory_program``'s order (a gate, then its errors in the gate's qubit order,
    or its one correlated error).  Index (2 r_hi + r_lo) + 4 (2 c_hi + c_lo) with lo / hi the smaller /
    larger of ``qubits``: x <- S x on R.reshape(-1, order="F") of a pair environment
    (``DeviceDM.pair_envs``).  ``noise_model`` None: the lifted unitary."""
    from .circuit import decompose, qubit_indices

    qubits = (int(qubits[0]), int(qubits[1]))
    if qubits[0] == qubits[1]:
        raise ValueError("layer_superoperator: two different qubits")
    lo = min(qubits)

    def lifted(mats, qs):
        return sum(np.kron(f.conj(), f) for f in (_pair_frame(k, qs, lo) for k in mats))

    s = np.eye(16, dtype=complex)
    for ins in circuit.data:
        name = ins.operation.name
        if name in ("barrier", "id", "delay"):
            continue
        if name == "measure":
            raise ValueError("layer_superoperator: a circuit of gates, without measures")
        qs = tuple(qubits[i] for i in qubit_indices(circuit, ins))
        for matrix, q in decompose(ins, qs):
            s = lifted([matrix], q) @ s
        if noise_model is not None:
            for q, error in noise_model.channels(name, qs):
                s = lifted(error.kraus, q if error.correlated else (q,)) @ s
    return s


def terminal_effects(n, rhs_instructions, circuit, noise_model):
    """float64 [n, 4]: per qubit (E00, E11, Re E01, Im E01) of the effect that reading 0 on it has in front
    of ``rhs_instructions`` (instructions of ``circuit``: what a compiler keeps to the right of its
    variational range): |0><0| pulled back through the adjoint of the error on ``measure`` and then, last
    instruction first, through every gate and the error attached to it.  Every instruction must act on one
    qubit (measures, barriers, ``id`` and ``delay`` aside): a starting circuit with an entangling gate
    leaves no product of effects and raises NotImplementedError.  ``DeviceDM.pair_envs`` takes the result."""
    from .circuit import op_matrix, qubit_indices

    def adjoint(name, q, e):
        if noise_model is None:
            return e
        for _, error in noise_model.channels(name, (q,)):
            e = sum(k.conj().T @ e @ k for k in error.kraus)
        return e

    n = int(n)
    eff = []
    for q in range(n):
        e = np.zeros((2, 2), dtype=complex)
        e[0, 0] = 1.0
        eff.append(adjoint("measure", q, e))
    for ins in reversed(list(rhs_instructions)):
        name = ins.operation.name
        if name in ("barrier", "id", "delay", "measure"):
            continue
        qs = qubit_indices(circuit, ins)
        if len(qs) != 1:
            raise NotImplementedError(
                f"terminal_effects: the {len(qs)}-qubit gate {name!r} after the variational range leaves no product "
                "of one-qubit effects: the noise-aware general_gradient needs a starting_circuit of one-qubit "
                "gates (or none)")
        u = np.asarray(op_matrix(ins.operation), dtype=complex)
        eff[qs[0]] = u.conj().T @ adjoint(name, qs[0], eff[qs[0]]) @ u
    return np.array([(e[0, 0].real, e[1, 1].real, e[0, 1].real, e[0, 1].imag) for e in eff])


def trajectory_program(circuit, noise_model):
    """(rows, n_events, measured): the flat program of aqc_sv_traj_sample for ``circuit`` under
    ``noise_model``.  Each gate of ``device_ops(circuit)`` is a gate row; after a gate that carries an
    error one Kraus row follows per affected qubit, in the gate's qubit order, or, for a correlated
    error, one group of nk consecutive rows (``kraus2_rows``); an error attached to "measure" gives one
    Kraus row per measure instruction, in circuit order, after all gates.  Identity channels emit no
    row.  Event e numbers the one-qubit Kraus rows and the groups in program order.  ``measured``:
    {qubit: clbit}, or None for a circuit without measures (which must be terminal)."""
    from . import _lib
    from .backends.qiskit_sampling_backend import terminal_measurements
    from .circuit import decompose, qubit_indices

    measured = terminal_measurements(circuit)
    # the program as a list of slots: a gate piece (matrix, qubits), or a channel (error, qubit);
    # the gate rows are then converted in one ops_array call and each error's row written once
    slots, tail = [], []
    for ins in circuit.data:
        name = ins.operation.name
        if name == "set_matrix_product_state":
            raise ValueError("trajectory_program: a circuit that starts from an MPS cannot run as trajectories")
        if name in ("barrier", "id", "delay"):
            continue
        qs = qubit_indices(circuit, ins)
        channels = noise_model.channels(name, qs) if noise_model is not None else []
        if name == "measure":
            tail += [(e, q) for q, e in channels]
            continue
        slots += list(decompose(ins, qs))
        slots += [(e, q) for q, e in channels]
    slots += tail
    is_kraus = np.fromiter((isinstance(s[0], QuantumError) for s in slots), dtype=bool, count=len(slots))
    # a correlated channel takes one row per operator: first[i] = the first row of slot i
    width = np.fromiter((len(s[0].kraus) if k and s[0].correlated else 1 for s, k in zip(slots, is_kraus)),
                        dtype=np.int64, count=len(slots))
    first = np.cumsum(width) - width
    rows = np.zeros(int(width.sum()), dtype=_lib.OP_DTYPE)
    if len(slots) and not is_kraus.all():
        rows[first[~is_kraus]] = _lib.ops_array([s for s, k in zip(slots, is_kraus) if not k])
    by_error = {}
    for i in np.flatnonzero(is_kraus):
        by_error.setdefault(id(slots[i][0]), []).append(i)
    for slot_ids in by_error.values():
        error = slots[slot_ids[0]][0]
        if error.correlated:
            group = kraus2_rows(error, (0, 1))
            for i in slot_ids:
                rows[first[i]: first[i] + len(group)] = group
                rows["q0"][first[i]: first[i] + len(group)] = slots[i][1][0]
                rows["q1"][first[i]: first[i] + len(group)] = slots[i][1][1]
        else:
            rows[first[slot_ids]] = kraus_row(error, 0)[0]
            rows["q0"][first[slot_ids]] = [slots[i][1] for i in slot_ids]
    return rows, int(is_kraus.sum()), measured
