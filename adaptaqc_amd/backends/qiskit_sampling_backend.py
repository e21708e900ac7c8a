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

"""Shot-sampling backend on MI355X: drop-in for adaptaqc/backends/qiskit_sampling_backend.py:20-108.

Costs are estimated from measurement counts, as the reference estimates them from Aer's
``qasm_simulator``.  Here the counts come from ``SamplingSimulator``: the circuit is simulated on the
device (statevector or MPS) and the shots are drawn there by libaqchip's samplers
(aqc_sv_sample / aqc_mps_sample); only the outcomes come back to the host.  Any object with the
same ``run(circuit, shots=..., **kwargs).result().get_counts()`` contract can stand in for it.
"""
import os
from types import SimpleNamespace

import numpy as np

from .aqc_backend import AQCBackend

_SKIP = ("barrier", "id", "delay")


class SamplingJob:
    """What ``SamplingSimulator.run`` returns: the shots are drawn by the time it exists."""

    def __init__(self, result):
        self._result = result

    def result(self):
        return self._result

    def status(self):
        return "DONE"


class SamplingResult:
    def __init__(self, counts):
        self._counts = counts

    def get_counts(self, experiment=None):
        return dict(self._counts)


def _bit_index(circuit, b):
    if isinstance(b, (int, np.integer)):
        return int(b)
    return int(circuit.find_bit(b).index)


def terminal_measurements(circuit):
    """{qubit: clbit} of the circuit's measure instructions, or None when it has none.  They must be
    terminal: a gate after a measure on the same qubit is a mid-circuit measurement, which the
    pure-state simulation does not run."""
    from ..circuit import qubit_indices

    measured = {}
    for ins in circuit.data:
        name = ins.operation.name
        qs = qubit_indices(circuit, ins) if name != "set_matrix_product_state" else ()
        if name == "measure":
            measured[qs[0]] = _bit_index(circuit, ins.clbits[0])
        elif name not in _SKIP and any(q in measured for q in qs):
            raise NotImplementedError("a gate after a measure on the same qubit (mid-circuit measurement) is not "
                                      "supported: measurements must be terminal")
    return measured or None


class SamplingSimulator:
    """Stand-in for Aer's ``qasm_simulator`` handle held as ``backend.simulator``.

    ``run(circuit, shots=1024, seed_simulator=None, noise_model=None)`` simulates the circuit's gates
    on the device and draws ``shots`` outcomes of its measurements there; ``result().get_counts()`` gives qiskit's
    counts dict (bitstrings over the classical bits, highest leftmost; over all qubits for a circuit
    without measure instructions).  ``method``: "statevector", "matrix_product_state", or
    "automatic" (statevector up to 26 qubits, MPS above).

    The simulated state is kept, keyed by the gate list (measures are not part of the key), so the
    reference's local cost -- n runs that differ only in the measured qubit
    (qiskit_sampling_backend.py:46-76) -- simulates once and samples n times.

    With ``seed_simulator`` the shots depend on that seed alone (identical calls give identical
    counts, as with Aer); without it the seed is drawn at construction (or is ``seed``) and every
    run advances a run counter, so repeated runs are independent.

    ``mps_trajectories``: a noise model runs as statevector trajectories (at most MAX_NOISY_QUBITS
    qubits) unless this is True; then method "matrix_product_state", and "automatic" above
    MAX_NOISY_QUBITS, run it as MPS trajectories (aqc_mps_traj_sample) under the simulator's
    truncation options.  Opt-in, because an MPS trajectory costs about three two-site SVDs per noisy
    gate: every Kraus operator has to meet the orthogonality centre.  The same flag and the same rule
    (``_trajectory_engine``) put QiskitSamplingBackend's noisy pair tomography on the MPS engine.

    ``mps_pauli_readout`` (needs ``mps_trajectories``): the same rule puts the noisy Pauli readout of
    ``pauli_counts`` on the MPS engine (aqc_mps_traj_pauli_counts: every term read from each trajectory
    by a transfer chain over its support); without it ``pauli_counts`` refuses a noise model there.
    Opt-in like the other two.

    ``mps_correlated`` (needs ``mps_trajectories``): the MPS trajectory engine then takes noise models with
    correlated two-qubit errors (``depolarizing_error(p, 2)``, ``QuantumError.two_qubit``, two-letter
    ``pauli_error`` labels) for shots, noisy pair tomography and the noisy Pauli readout; without it those
    routes refuse such a model by name."""

    name = "hip_sampling_simulator"
    METHODS = ("automatic", "statevector", "matrix_product_state")
    MAX_NOISY_QUBITS = 24  # aqc_sv_traj_sample's limit

    def __init__(self, method="automatic", seed=None, mps_truncation_threshold=1e-16, max_chi=None,
                 mps_trajectories=False, mps_pauli_readout=False, mps_correlated=False):
        if method not in self.METHODS:
            raise ValueError(f"method must be one of {self.METHODS}")
        if mps_pauli_readout and not mps_trajectories:
            raise ValueError("mps_pauli_readout=True needs mps_trajectories=True")
        if mps_correlated and not mps_trajectories:
            raise ValueError("mps_correlated=True needs mps_trajectories=True")
        self.options = SimpleNamespace(method=method, matrix_product_state_truncation_threshold=mps_truncation_threshold,
                                       matrix_product_state_max_bond_dimension=max_chi)
        self.seed = int(seed) if seed is not None else int(np.random.SeedSequence().generate_state(2, np.uint32).view(np.uint64)[0])
        self.runs = 0
        self.mps_trajectories = bool(mps_trajectories)
        self.mps_pauli_readout = bool(mps_pauli_readout)
        self.mps_correlated = bool(mps_correlated)
        self._last = None  # (n, method, ops bytes, device state)

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_last"] = None
        d.pop("aqc_learned_cap", None)
        return d

    def __repr__(self):
        return f"SamplingSimulator(hip, gfx950, method={self.options.method!r})"

    def _method(self, n):
        m = self.options.method
        if m == "automatic":
            return "statevector" if n <= 26 else "matrix_product_state"
        return m

    def _state(self, circuit):
        from ..circuit import device_ops_array
        from ..device import DeviceSV
        from ..mps_operations import device_mps_from_circuit

        n = circuit.num_qubits
        method = self._method(n)
        key = device_ops_array(circuit).tobytes()
        if self._last is not None and self._last[:3] == (n, method, key):
            return self._last[3]
        if method == "statevector":
            dev = DeviceSV(n)
            dev.apply(device_ops_array(circuit))
        else:
            dev = device_mps_from_circuit(circuit, sim=self)
        self._last = (n, method, key, dev)
        return dev

    def _trajectory_engine(self, n):
        """The engine a noise model's trajectories of n qubits ask for: "matrix_product_state" for that
        method and for "automatic" above MAX_NOISY_QUBITS, else "statevector".  Shots and pair
        tomography both decide by it; whether the engine may run (``mps_trajectories``, the statevector
        limit) is the caller's to check, each with its own message."""
        method = self.options.method
        if method == "matrix_product_state" or (method == "automatic" and n > self.MAX_NOISY_QUBITS):
            return "matrix_product_state"
        return "statevector"

    def _noisy_program(self, circuit, noise_model):
        """(rows, n_events, engine) of the circuit's trajectories under ``noise_model``, or None when no
        Kraus row comes of it (no model, an empty or all-identity one): the noiseless path then."""
        from ..noise import trajectory_program

        if noise_model is None:
            return None
        rows, n_events, _ = trajectory_program(circuit, noise_model)
        if n_events == 0:
            return None
        n = circuit.num_qubits
        if self._trajectory_engine(n) == "matrix_product_state":
            if not self.mps_trajectories:
                raise NotImplementedError(
                    "a noise model runs as statevector trajectories (method 'statevector', or 'automatic' up to "
                    f"{self.MAX_NOISY_QUBITS} qubits) unless the simulator is built with mps_trajectories=True, "
                    "which runs it as MPS trajectories")
            self._refuse_correlated_on_mps(rows)
            return rows, n_events, "matrix_product_state"
        if n > self.MAX_NOISY_QUBITS:
            raise NotImplementedError(
                f"statevector trajectories stop at {self.MAX_NOISY_QUBITS} qubits: use method 'automatic' or "
                "'matrix_product_state' with mps_trajectories=True")
        return rows, n_events, "statevector"

    def _correlated(self):
        """Whether the MPS trajectory engine takes correlated groups (absent in an old pickle: no)."""
        return bool(getattr(self, "mps_correlated", False))

    def _correlated_kw(self):
        """The keyword that switches the device wrappers' MPS engine to correlated groups, when set."""
        return {"correlated": True} if self._correlated() else {}

    def _refuse_correlated_on_mps(self, rows):
        """A program with a correlated two-qubit Kraus group runs on the MPS trajectory engine only with
        ``mps_correlated``."""
        from ..noise import _CORRELATED_ON_MPS, has_correlated_rows

        if not self._correlated() and has_correlated_rows(rows):
            raise NotImplementedError(f"noise_model: {_CORRELATED_ON_MPS}")

    def _at_learned_capacity(self, n, call):
        """``call(chi_cap=, threshold=, max_chi=)`` -- a batch of MPS trajectories of n qubits -- at the
        capacity of chi_cap_for under the simulator's truncation options; a capacity overflow grows the
        learned capacity and runs the call again: the same trajectories, their uniforms being counters."""
        from .._lib import AqcError
        from ..mps_operations import chi_cap_for, grow_capacity, is_capacity_error, learned_capacities

        thr = self.options.matrix_product_state_truncation_threshold
        max_chi = self.options.matrix_product_state_max_bond_dimension
        learned = learned_capacities(self)
        while True:
            cap = chi_cap_for(n, max_chi, 1, learned)
            try:
                return call(chi_cap=cap, threshold=thr, max_chi=max_chi)
            except AqcError as e:
                if not (is_capacity_error(e) and grow_capacity(n, max_chi, cap, learned)):
                    raise

    def _mps_trajectories(self, n, rows, n_events, shots, seed, run):
        """The shots as MPS trajectories (aqc_mps_traj_sample) at the learned capacity."""
        from ..device import mps_trajectory_sample

        return self._at_learned_capacity(
            n, lambda **cap: mps_trajectory_sample(n, rows, n_events, shots, seed, run,
                                                   **self._correlated_kw(), **cap))

    def run(self, circuit, shots=1024, seed_simulator=None, noise_model=None, **ignored):
        """``noise_model`` (adaptaqc_amd.noise.NoiseModel): every shot is then one quantum trajectory on
        the device (aqc_sv_traj_sample, or aqc_mps_traj_sample with ``mps_trajectories``), the errors
        following the gates they are attached to."""
        from ..device import counts_from_samples, trajectory_sample

        measured = terminal_measurements(circuit)
        noisy = self._noisy_program(circuit, noise_model)
        dev = self._state(circuit) if noisy is None else None
        if seed_simulator is not None:
            seed, run = int(seed_simulator), 0
        else:
            seed, run = self.seed, self.runs
            self.runs += 1
        if noisy is None:
            samples = dev.sample(int(shots), seed, run)
        elif noisy[2] == "statevector":
            samples = trajectory_sample(circuit.num_qubits, noisy[0], noisy[1], int(shots), seed, run)
        else:
            samples = self._mps_trajectories(circuit.num_qubits, noisy[0], noisy[1], int(shots), seed, run)
        counts = counts_from_samples(samples, circuit.num_qubits, measured)
        if measured is not None:  # keys over every classical bit: an unmeasured one reads 0
            width = max(int(getattr(circuit, "num_clbits", 0) or 0), max(measured.values()) + 1)
            counts = {k.rjust(width, "0"): v for k, v in counts.items()}
        return SamplingJob(SamplingResult(counts))

    def _noisy_pauli_program(self, circuit, noise_model):
        """(rows, n_events, effects, engine) of the noisy Pauli readout, or None when ``noise_model`` has
        no effective error on the circuit or on the readout (one simulation and binomial draws then).
        The engine follows ``_trajectory_engine``; the MPS one needs ``mps_pauli_readout``."""
        from ..noise import readout_effects, trajectory_program

        if noise_model is None:
            return None
        n = circuit.num_qubits
        rows, n_events, _ = trajectory_program(without_classical_operations(circuit), noise_model)
        readout = any(noise_model.channels(name, (q,)) for name in ("sdg", "h", "measure") for q in range(n))
        if n_events == 0 and not readout:
            return None
        if self._trajectory_engine(n) == "matrix_product_state":
            if not getattr(self, "mps_pauli_readout", False):
                raise NotImplementedError("the Pauli readout of MPS trajectories is not built into this simulator: "
                                          "pauli_terms='device' under a noise model runs statevector trajectories "
                                          "(method 'statevector', or 'automatic' up to "
                                          f"{self.MAX_NOISY_QUBITS} qubits) unless the simulator is built with "
                                          "mps_trajectories=True, mps_pauli_readout=True")
            self._refuse_correlated_on_mps(rows)
            return rows, n_events, readout_effects(n, noise_model), "matrix_product_state"
        if n > self.MAX_NOISY_QUBITS:
            raise NotImplementedError(f"statevector trajectories stop at {self.MAX_NOISY_QUBITS} qubits: use method "
                                      "'automatic' or 'matrix_product_state' with mps_trajectories=True, "
                                      "mps_pauli_readout=True")
        return rows, n_events, readout_effects(n, noise_model), "statevector"

    def pauli_counts(self, circuit, labels, shots=1024, seed_simulator=None, noise_model=None):
        """int64 [len(labels)]: for every Pauli label (qiskit order, none all-identity) the number of +1
        parities among ``shots`` shots of the reference's rotated and measured copy of ``circuit`` --
        without building the copies.  The estimate of <P> is (2 plus - shots) / shots.

        Under a ``noise_model`` with an effective error, ``shots`` trajectories of the circuit (without
        its classical operations) run once and every one draws a +-1 outcome per term
        (aqc_sv_traj_pauli_counts), the errors on the appended ``sdg`` / ``h`` / ``measure`` folded into
        POVM effects (noise.readout_effects): each term's count has the law of its own noisy circuit;
        different terms share trajectories and are correlated.  With ``mps_pauli_readout`` the MPS
        engine takes them where ``_trajectory_engine`` says so (aqc_mps_traj_pauli_counts, at the learned
        capacity: an overflow grows it and runs the same trajectories again).
        Otherwise the circuit is simulated once (the cached state of ``run``), every term is taken by
        ``pauli_expect`` and its count is one binomial draw on the device (aqc_multinomial_counts).
        Seed and run counter as ``run``: one call advances the counter once."""
        from ..device import mps_trajectory_pauli_counts, multinomial_counts, trajectory_pauli_counts
        from ..paulis import terms_to_codes

        n = circuit.num_qubits
        shots = int(shots)
        codes = terms_to_codes(list(labels), n)
        if len(codes) == 0:
            return np.zeros(0, dtype=np.int64)
        if not codes.any(axis=1).all():
            raise ValueError("pauli_counts: an all-identity label has the value 1 and is not measured")
        noisy = self._noisy_pauli_program(circuit, noise_model)
        dev = self._state(circuit) if noisy is None else None
        if seed_simulator is not None:
            seed, run = int(seed_simulator), 0
        else:
            seed, run = self.seed, self.runs
            self.runs += 1
        if noisy is not None:
            rows, n_events, effects, engine = noisy
            if engine == "statevector":
                return trajectory_pauli_counts(n, rows, n_events, codes, effects, shots, seed, run)
            return self._at_learned_capacity(
                n, lambda **cap: mps_trajectory_pauli_counts(n, rows, n_events, codes, effects, shots, seed, run,
                                                             **self._correlated_kw(), **cap))
        ev = dev.pauli_expect(np.concatenate([codes, np.zeros((1, n), dtype=np.uint8)]))
        v, w = ev[:-1], ev[-1]  # w = <psi|psi>: below 1 for a truncated MPS
        probs = np.stack([np.maximum(0.0, (w + v) / 2), np.maximum(0.0, (w - v) / 2)], axis=1)
        return multinomial_counts(probs, shots, seed, run)[:, 0]


def without_classical_operations(circuit):
    """A copy of ``circuit`` without its measure instructions and classical bits (the reference's
    co.remove_classical_operations, on a copy)."""
    qc = circuit.copy()
    qc.data = [ins for ins in qc.data if ins.operation.name != "measure"]
    qc.num_clbits = 0
    return qc


def tomography_counts_from_circuits(circuit, qubit_1, qubit_2, simulator, execute_kwargs=None):
    """The reference's route to a pair's tomography data (entanglement_measures.py:101-135): nine
    copies of ``circuit`` (without its classical operations), each with the basis rotations of one
    two-qubit Pauli setting and ``measure(lo -> 0, hi -> 1)``, run through
    ``simulator.run(copy, **execute_kwargs).result().get_counts()``.  Returns the int64 [9, 4]
    table: row s = 3 b_hi + b_lo (0 X, 1 Y, 2 Z), column o = 2 o_hi + o_lo (the clbits' values; 0 is
    the +1 eigenstate).  Bits left of clbit 1 in a key are ignored.  ``circuit`` is not modified."""
    from ..utils.circuit_operations import add_pauli_measurement_rotations

    lo, hi = sorted((int(qubit_1), int(qubit_2)))
    if lo == hi:
        raise ValueError("tomography needs two different qubits")
    n = circuit.num_qubits
    base = without_classical_operations(circuit)
    kwargs = dict(execute_kwargs or {})
    table = np.zeros((9, 4), dtype=np.int64)
    for s in range(9):
        label = ["I"] * n
        label[n - 1 - hi] = "XYZ"[s // 3]
        label[n - 1 - lo] = "XYZ"[s % 3]
        rotated = base.copy()
        add_pauli_measurement_rotations(rotated, "".join(label))
        rotated.measure(lo, 0)
        rotated.measure(hi, 1)
        counts = simulator.run(rotated, **kwargs).result().get_counts()
        for key, c in counts.items():
            bits = key.replace(" ", "").rjust(2, "0")
            table[s, 2 * int(bits[-2]) + int(bits[-1])] += int(c)
    return table


def concurrence_bound_counts_from_circuits(circuit, qubit_1, qubit_2, simulator, execute_kwargs=None):
    """The three two-copy circuits of entanglement_measures.py:170-245 on 2 n qubits: the
    antisymmetric-subspace projector measurement (cx, h, measure) on (qubit_1, n + qubit_1) into
    clbits 0, 1 and / or on (qubit_2, n + qubit_2) into clbits 2, 3.  Returns the shares
    (f_pmpm, f_pmi, f_ipm) of the keys "1111", "0011", "1100"."""
    from ..circuit import QuantumCircuit
    from ..utils.circuit_operations import add_to_circuit

    n = circuit.num_qubits
    base = without_classical_operations(circuit)
    two = QuantumCircuit(2 * n)
    add_to_circuit(two, base, qubit_subset=list(range(n)))
    add_to_circuit(two, base, qubit_subset=list(range(n, 2 * n)))
    kwargs = dict(execute_kwargs or {})

    def projector(qc, q, c0):
        qc.cx(q, n + q)
        qc.h(q)
        qc.measure(q, c0)
        qc.measure(n + q, c0 + 1)

    shares = []
    for on_1, on_2, key in ((True, True, "1111"), (True, False, "0011"), (False, True, "1100")):
        qc = two.copy()
        if on_1:
            projector(qc, int(qubit_1), 0)
        if on_2:
            projector(qc, int(qubit_2), 2)
        counts = simulator.run(qc, **kwargs).result().get_counts()
        counts = {k.replace(" ", "").rjust(4, "0")[-4:]: v for k, v in counts.items()}
        shares.append(_share(counts, key))
    return tuple(shares)


class QiskitSamplingBackend(AQCBackend):
    """``tomography``: how pair entanglement is measured from shots (the ISL method needs it).

    * ``None``: not at all -- ISL with this backend raises at the compiler's construction;
    * ``"circuits"``: the reference's route, for any simulator that honours the
      ``run().result().get_counts()`` contract: nine rotated circuits per pair;
    * ``"device"`` (needs a ``SamplingSimulator``): the state is simulated once, the RDMs of all pairs
      are taken on the device, and every setting's counts are drawn from the probabilities the RDM
      fixes (csrc/tomo.hip) -- the law of the counts is that of the nine circuits.

    A ``noise_model`` in the compiler's ``execute_kwargs`` reaches ``SamplingSimulator.run`` with every
    cost, <Z> and ``"circuits"`` tomography evaluation; ``"device"`` tomography is pure-state and
    raises when it is given one, unless ``trajectory_tomography`` is set.

    ``trajectory_tomography`` (needs ``tomography="device"``): under a noise model with an effective
    error, ``pair_tomography`` runs 9 x shots quantum trajectories of the circuit and reads every pair
    out of each (aqc_sv_traj_pair_tomo): trajectory 9 i + s serves Pauli setting s of every pair, the
    errors the model attaches to the appended ``sdg`` / ``h`` / ``measure`` folded into POVM effects
    (noise.readout_effects).  A pair's nine tables have the law of the reference's nine noisy circuits;
    tables of different pairs share trajectories and are correlated, which the per-pair fit never
    sees.  Opt-in, because the sweep costs 9 x shots trajectories.  Statevector trajectories up to 24
    qubits.  With a simulator built with ``mps_trajectories=True``, method "matrix_product_state", and
    "automatic" above 24 qubits, run the trajectories on the MPS engine instead
    (aqc_mps_traj_pair_tomo: every pair read from the trajectory's RDMs), at the simulator's learned
    capacity as its noisy shots do.  The concurrence lower bound stays noiseless-only.

    ``pauli_terms``: how ``expectation_values_of_pauli_terms`` (and so
    ``expectation_value_of_pauli_operator``) measures the terms of an operator with this backend.

    * ``None``: the reference's route -- one rotated and measured copy of the circuit per term through
      ``simulator.run``; under a noise model every copy is a full trajectory run;
    * ``"device"`` (needs a simulator with ``pauli_counts``, i.e. a ``SamplingSimulator``): all terms
      from one ``SamplingSimulator.pauli_counts`` call -- under a noise model ``shots`` trajectories,
      each read out for every term (aqc_sv_traj_pauli_counts).  A term's estimate has the law of the
      reference's circuit for that term; different terms share trajectories and are correlated.
      Statevector trajectories up to 24 qubits; with a simulator built with ``mps_trajectories=True,
      mps_pauli_readout=True``, method "matrix_product_state", and "automatic" above 24 qubits, run MPS
      trajectories instead (aqc_mps_traj_pauli_counts: every term read from each trajectory by a transfer
      chain over its support, any number of general factors a term).
    """

    TOMOGRAPHY_MODES = (None, "circuits", "device")
    PAULI_TERMS_MODES = (None, "device")

    def __init__(self, simulator=None, tomography=None, trajectory_tomography=False, pauli_terms=None):
        if tomography not in self.TOMOGRAPHY_MODES:
            raise ValueError(f"tomography must be one of {self.TOMOGRAPHY_MODES}")
        if pauli_terms not in self.PAULI_TERMS_MODES:
            raise ValueError(f"pauli_terms must be one of {self.PAULI_TERMS_MODES}")
        if trajectory_tomography and tomography != "device":
            raise TypeError("trajectory_tomography=True needs tomography='device'")
        self.simulator = simulator if simulator is not None else SamplingSimulator()
        if tomography == "device" and not isinstance(self.simulator, SamplingSimulator):
            raise TypeError("tomography='device' needs a SamplingSimulator (its cached device state); "
                            "use tomography='circuits' with other simulators")
        if pauli_terms == "device" and not callable(getattr(self.simulator, "pauli_counts", None)):
            raise TypeError("pauli_terms='device' needs a simulator with pauli_counts (a SamplingSimulator); "
                            "leave pauli_terms=None with other simulators")
        self.tomography = tomography
        self.trajectory_tomography = bool(trajectory_tomography)
        self.pauli_terms = pauli_terms

    # -- pair tomography ---------------------------------------------------------------
    def _require_tomography(self):
        if self.tomography is None:
            raise NotImplementedError("this QiskitSamplingBackend was built without tomography: pass "
                                      "tomography='device' or 'circuits'")

    def _require_noiseless_device_route(self, kwargs, what="pair tomography"):
        if self.tomography == "device" and kwargs.get("noise_model") is not None:
            if what == "pair tomography":
                hint = ("build the backend with trajectory_tomography=True (9 x shots noisy trajectories per "
                        "sweep), or use tomography='circuits'")
            else:
                hint = "use tomography='circuits'"
            raise NotImplementedError(f"tomography='device' takes the pairs' RDMs from the pure state and cannot "
                                      f"honour a noise_model for {what}: {hint}")

    def _noisy_tomography_program(self, circuit, noise_model):
        """(rows, n_events, effects, engine) of the noisy device route, or None when ``noise_model`` has
        no effective error on the circuit or on the readout (the pure-state route then)."""
        from ..noise import readout_effects, trajectory_program

        if noise_model is None:
            return None
        n = circuit.num_qubits
        base = without_classical_operations(circuit)
        rows, n_events, _ = trajectory_program(base, noise_model)
        readout = any(noise_model.channels(name, (q,)) for name in ("sdg", "h", "measure") for q in range(n))
        if n_events == 0 and not readout:
            return None
        sim = self.simulator
        method = sim.options.method
        if sim._trajectory_engine(n) == "matrix_product_state" and sim.mps_trajectories:
            sim._refuse_correlated_on_mps(rows)
            return rows, n_events, readout_effects(n, noise_model), "matrix_product_state"
        if method == "matrix_product_state":
            raise NotImplementedError("trajectory_tomography runs statevector trajectories: a noise_model with "
                                      "method 'matrix_product_state' is not supported unless the simulator is "
                                      "built with mps_trajectories=True, which runs it as MPS trajectories")
        if n > sim.MAX_NOISY_QUBITS:
            raise NotImplementedError(f"trajectory_tomography runs statevector trajectories, which stop at "
                                      f"{sim.MAX_NOISY_QUBITS} qubits (method {method!r}, {n} qubits): use method "
                                      "'automatic' or 'matrix_product_state' with a simulator built with "
                                      "mps_trajectories=True")
        return rows, n_events, readout_effects(n, noise_model), "statevector"

    def _noisy_counts(self, n, noisy, pairs, shots, seed, run):
        """The int64 [npairs, 9, 4] tables of the noisy device route on the engine ``noisy`` names."""
        from ..device import mps_trajectory_pair_tomography, trajectory_pair_tomography

        rows, n_events, effects, engine = noisy
        if engine == "statevector":
            return trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, seed, run)
        return self.simulator._at_learned_capacity(
            n, lambda **cap: mps_trajectory_pair_tomography(n, rows, n_events, pairs, effects, shots, seed, run,
                                                            **self.simulator._correlated_kw(), **cap))

    def _seed_and_run(self, kwargs):
        """(seed, run) of one device sweep: ``seed_simulator`` alone when given, else the
        simulator's seed and its run counter, which advances once per sweep."""
        if kwargs.get("seed_simulator") is not None:
            return int(kwargs["seed_simulator"]), 0
        seed, run = self.simulator.seed, self.simulator.runs
        self.simulator.runs += 1
        return seed, run

    def pair_tomography(self, circuit, pairs, execute_kwargs=None, measure=None):
        """(rho [npairs, 4, 4], measures [npairs] or None) of the state ``circuit`` prepares, from
        ``execute_kwargs["shots"]`` shots per Pauli setting.  ``measure``: a name of
        device.EM_METHOD_CODES.  RDM index 2 bit_hi + bit_lo with hi the pair's larger qubit."""
        from ..device import entanglement_measures, pair_tomography, tomo_fit

        self._require_tomography()
        kwargs = dict(execute_kwargs or {})
        if not self.trajectory_tomography:
            self._require_noiseless_device_route(kwargs)
        pairs = [(int(a), int(b)) for a, b in pairs]
        noisy = self._noisy_tomography_program(circuit, kwargs.get("noise_model")) if self.trajectory_tomography else None
        if noisy is not None:
            if not pairs:
                return np.zeros((0, 4, 4), dtype=complex), (None if measure is None else np.zeros(0))
            seed, run = self._seed_and_run(kwargs)
            counts = self._noisy_counts(circuit.num_qubits, noisy, pairs, int(kwargs.get("shots", 1024)), seed, run)
            rho = tomo_fit(counts)
            return rho, (None if measure is None else entanglement_measures(rho, measure))
        if self.tomography == "device":
            dev = self.simulator._state(circuit)  # (measures are not part of the cached state's key)
            rdms = dev.pair_rdms(pairs)
            seed, run = self._seed_and_run(kwargs)
            return pair_tomography(rdms, int(kwargs.get("shots", 1024)), seed, run, measure)
        tables = [tomography_counts_from_circuits(circuit, a, b, self.simulator, kwargs) for a, b in pairs]
        rho = tomo_fit(np.stack(tables)) if tables else np.zeros((0, 4, 4), dtype=complex)
        return rho, (None if measure is None else entanglement_measures(rho, measure))

    def concurrence_lower_bounds(self, circuit, pairs, execute_kwargs=None):
        """The observable concurrence lower bound of every pair (entanglement_measures.py:138-250)."""
        from ..device import concurrence_lower_bounds

        self._require_tomography()
        kwargs = dict(execute_kwargs or {})
        self._require_noiseless_device_route(kwargs, "the concurrence lower bound (its two-copy circuits)")
        pairs = [(int(a), int(b)) for a, b in pairs]
        if self.tomography == "device":
            dev = self.simulator._state(circuit)
            rdms = dev.pair_rdms(pairs)
            seed, run = self._seed_and_run(kwargs)
            return concurrence_lower_bounds(rdms, int(kwargs.get("shots", 1024)), seed, run,
                                            swap=[a > b for a, b in pairs])
        out = []
        for a, b in pairs:
            pmpm, pmi, ipm = concurrence_bound_counts_from_circuits(circuit, a, b, self.simulator, kwargs)
            out.append(max(8 * pmpm - 4 * ipm, 8 * pmpm - 4 * pmi))
        return np.asarray(out, dtype=float)

    def evaluate_global_cost(self, compiler):
        """qiskit_sampling_backend.py:24-44: 1 - (share of shots that read all zeros)."""
        if compiler.soften_global_cost:
            raise NotImplementedError("soften_global_cost is currently only implemented for AerMPSBackend")
        counts = self.evaluate_circuit(compiler)
        width = compiler.total_num_qubits * (2 if compiler.general_initial_state else 1)
        return 1 - _share(counts, "0" * width)

    def evaluate_local_cost(self, compiler):
        """qiskit_sampling_backend.py:46-76: per qubit (with its partner under general_initial_state),
        measure, run, remove the measure; the cost is the mean share of shots not reading zero."""
        n = compiler.total_num_qubits
        circuit = compiler.full_circuit
        qubit_costs = np.zeros(n)
        for i in range(n):
            qubits = (i, i + n) if compiler.general_initial_state else (i,)
            for clbit, q in enumerate(qubits):
                circuit.measure(q, clbit)
            try:
                counts = self.evaluate_circuit(compiler)
            finally:
                del circuit.data[-len(qubits):]
            qubit_costs[i] = 1 - _share(counts, "0" * len(qubits))
        return np.mean(qubit_costs)

    def evaluate_circuit(self, compiler):
        # Don't parallelise shots if ADAPT-AQC is already being run in parallel (reference :79-81);
        # backend_options (method / max_parallel_experiments) are Aer's and have no meaning here.
        _ = os.environ["QISKIT_IN_PARALLEL"] == "TRUE"
        job = self.simulator.run(compiler.full_circuit, **compiler.execute_kwargs)
        return job.result().get_counts()

    def measure_qubit_expectation_values(self, compiler):
        """qiskit_sampling_backend.py:91-108: <Z_i> = (shots reading 0 - shots reading 1) / shots of
        bit i (bit 0 is the rightmost character)."""
        counts = self.evaluate_circuit(compiler)
        keys = list(counts)
        width = len(keys[0])
        total = sum(counts.values())
        out = []
        for i in range(width):
            pos = width - 1 - i
            out.append(sum((1 if k[pos] == "0" else -1) * counts[k] for k in keys) / total)
        return out


def _share(counts, key):
    """counts[key] / shots; a key no shot produced is absent from the dict (share 0)."""
    total = sum(counts.values())
    return counts.get(key, 0) / total
