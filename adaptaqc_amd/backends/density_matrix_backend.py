"""Exact noisy simulation on MI355X: the density-matrix engine (csrc/dm.hip) as a simulator handle and
as a compiler backend.

What ``QiskitSamplingBackend`` estimates from shots under ``execute_kwargs["noise_model"]`` -- every
shot one quantum trajectory -- the density matrix gives exactly: one deterministic evolution of rho by
the same flat program (``noise.trajectory_program``) yields the noisy cost 1 - rho_00, every qubit's
<Z>, every pair's reduced density matrix, every Pauli term and the whole outcome distribution.  Up to
``MAX_QUBITS`` = 13 qubits (4^13 complex128 is 1 GiB); above that the trajectory engines
(``SamplingSimulator``: statevector trajectories to 24 qubits, MPS trajectories beyond) are the route.

* ``DensityMatrixSimulator``: a stand-in for an Aer simulator handle with ``method="density_matrix"``,
  with ``SamplingSimulator``'s ``run`` / ``pauli_counts`` contracts: the shots are drawn from the exact
  distribution, so ``QiskitSamplingBackend(DensityMatrixSimulator(), ...)`` works as it is.
* ``DensityMatrixBackend``: an ``AQCBackend`` without shots -- the expectation of the sampling
  backend's costs, and ISL from the exact mixed RDMs (``pair_rdms``).
"""
import numpy as np

from .aqc_backend import AQCBackend
from .qiskit_sampling_backend import (SamplingJob, SamplingResult, terminal_measurements,
                                      without_classical_operations)

MAX_QUBITS = 13  # aqc_dm_create's limit


def _refuse_width(n, who):
    if n > MAX_QUBITS:
        raise NotImplementedError(
            f"{who}: the density matrix stops at {MAX_QUBITS} qubits ({n} asked for): run a noise model on the "
            "trajectory engines instead -- SamplingSimulator (statevector trajectories up to 24 qubits, MPS "
            "trajectories with mps_trajectories=True above)")


class _Evolved:
    """rho after a program, kept on the device and keyed by the program's bytes."""

    def __init__(self):
        self._last = None  # (n, program bytes, DeviceDM)

    def state(self, n, rows):
        from ..device import DeviceDM

        key = rows.tobytes()
        if self._last is not None and self._last[:2] == (n, key):
            return self._last[2]
        dev = self._last[2] if self._last is not None and self._last[0] == n else None
        self._last = None
        if dev is None:
            dev = DeviceDM(n)
        else:
            dev.reset()
        dev.run(rows)
        self._last = (n, key, dev)
        return dev


class DensityMatrixSimulator:
    """Stand-in for an Aer simulator handle with ``method="density_matrix"``.

    ``run(circuit, shots=1024, seed_simulator=None, noise_model=None)`` evolves rho once by the circuit's
    program under ``noise_model`` (cached, keyed by the program's bytes) and draws ``shots`` outcomes of
    its measurements from the diagonal on the device; ``result().get_counts()`` follows
    ``SamplingSimulator.run``: keys over the classical bits (highest leftmost; over all qubits without
    measure instructions), an unmeasured bit reads 0, and with ``seed_simulator`` the shots depend on
    that seed alone, else on the simulator's seed and a run counter that every call advances."""

    name = "hip_density_matrix_simulator"
    MAX_QUBITS = MAX_QUBITS

    def __init__(self, seed=None):
        self.seed = int(seed) if seed is not None else int(np.random.SeedSequence().generate_state(2, np.uint32).view(np.uint64)[0])
        self.runs = 0
        self._evolved = _Evolved()

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_evolved"] = _Evolved()
        return d

    def __repr__(self):
        return "DensityMatrixSimulator(hip, gfx950)"

    def _state(self, circuit, noise_model):
        from ..noise import trajectory_program

        n = circuit.num_qubits
        _refuse_width(n, "DensityMatrixSimulator")
        rows, _, _ = trajectory_program(circuit, noise_model)
        return self._evolved.state(n, rows)

    def _seed_and_run(self, seed_simulator):
        if seed_simulator is not None:
            return int(seed_simulator), 0
        seed, run = self.seed, self.runs
        self.runs += 1
        return seed, run

    def run(self, circuit, shots=1024, seed_simulator=None, noise_model=None, **ignored):
        from ..device import counts_from_samples

        measured = terminal_measurements(circuit)
        dev = self._state(circuit, noise_model)
        seed, run = self._seed_and_run(seed_simulator)
        samples = dev.sample(int(shots), seed, run)
        counts = counts_from_samples(samples, circuit.num_qubits, measured)
        if measured is not None:  # keys over every classical bit: an unmeasured one reads 0
            width = max(int(getattr(circuit, "num_clbits", 0) or 0), max(measured.values()) + 1)
            counts = {k.rjust(width, "0"): v for k, v in counts.items()}
        return SamplingJob(SamplingResult(counts))

    def _values(self, circuit, codes, noise_model):
        """Tr(M_t rho) / Tr rho of the noisy readout of every term: the circuit without its classical
        operations, the errors on the appended ``sdg`` / ``h`` / ``measure`` as POVM effects."""
        from ..noise import readout_effects

        n = circuit.num_qubits
        dev = self._state(without_classical_operations(circuit), noise_model)
        effects = readout_effects(n, noise_model) if noise_model is not None else None
        return dev.pauli_expect(codes, effects) / dev.trace()

    def pauli_values(self, circuit, labels, noise_model=None):
        """float64 [len(labels)]: the exact expectation of the +-1 parity that the reference's rotated and
        measured copy of ``circuit`` reads for every Pauli label (qiskit order) under ``noise_model`` --
        what ``pauli_counts`` estimates; without a model, <P>.  An all-identity label gives 1."""
        from ..paulis import terms_to_codes

        codes = terms_to_codes(list(labels), circuit.num_qubits)
        out = np.ones(len(codes))
        live = codes.any(axis=1) if len(codes) else np.zeros(0, dtype=bool)
        if live.any():
            out[live] = self._values(circuit, np.ascontiguousarray(codes[live]), noise_model)
        return out

    def pauli_counts(self, circuit, labels, shots=1024, seed_simulator=None, noise_model=None):
        """int64 [len(labels)]: ``SamplingSimulator.pauli_counts``'s contract -- for every label (none
        all-identity) the number of +1 parities among ``shots`` shots.  The value of every term is exact
        (``pauli_values``); its count is one binomial draw on the device (aqc_multinomial_counts), so
        different terms are independent.  Seed and run counter as ``run``."""
        from ..device import multinomial_counts
        from ..paulis import terms_to_codes

        shots = int(shots)
        codes = terms_to_codes(list(labels), circuit.num_qubits)
        if len(codes) == 0:
            return np.zeros(0, dtype=np.int64)
        if not codes.any(axis=1).all():
            raise ValueError("pauli_counts: an all-identity label has the value 1 and is not measured")
        v = self._values(circuit, codes, noise_model)
        seed, run = self._seed_and_run(seed_simulator)
        probs = np.stack([np.maximum(0.0, (1 + v) / 2), np.maximum(0.0, (1 - v) / 2)], axis=1)
        return multinomial_counts(probs, shots, seed, run)[:, 0]


class DensityMatrixBackend(AQCBackend):
    """The exact expectation of what ``QiskitSamplingBackend`` estimates under the same
    ``execute_kwargs["noise_model"]``, with no shots.

    The program is ``noise.trajectory_program`` of a copy of ``compiler.full_circuit`` with a terminal
    measure on every qubit, so the errors attached to ``measure`` are in it, as they are in the sampling
    backend's cost; the compiler's circuit is untouched.  rho is evolved once per program and kept.

    ``AdaptConfig(method="general_gradient")`` scores the pairs by the gradient of the noisy cost in the new
    layer's angles: ``general_gradients`` reads one 4x4 environment per pair off rho in front of the layer
    (``pair_environments``, aqc_dm_pair_envs) and prices every shifted candidate, with its errors, on the
    host (``gradients.noisy_grads_from_envs``).  The starting circuit must be a product of one-qubit gates.

    ``heisenberg_sweep=True`` (opt-in): Rotosolve / Rotoselect cycles on the global or the local cost read
    every candidate of a gate off one 4x4 transition matrix between the forward-evolved prefix state and
    the observable pulled back through the suffix (``cached_rotations.DMHeisenbergSweep``) instead of
    evolving rho through the whole circuit per candidate; the costs are the same numbers up to rounding.
    ``checkpoint_bytes`` bounds the device memory of the pulled-back observables kept per cycle (16 x 4^n
    bytes each, at least one)."""

    MAX_QUBITS = MAX_QUBITS
    # (defaults for a backend restored from a checkpoint written before these existed)
    heisenberg_sweep = False
    checkpoint_bytes = 8 << 30
    _sweep = (0, ())
    pair_transitions = False
    gradient_cost = "global"
    _observables = None
    backward_passes = 0

    def __init__(self, heisenberg_sweep=False, checkpoint_bytes=8 << 30, pair_transitions=False,
                 gradient_cost="global"):
        if not (isinstance(pair_transitions, bool) or pair_transitions == "always"):
            raise ValueError(f"DensityMatrixBackend: pair_transitions must be False, True or 'always', not "
                             f"{pair_transitions!r}")
        if gradient_cost not in ("global", "local", "compiler"):
            raise ValueError(f"DensityMatrixBackend: gradient_cost must be 'global', 'local' or 'compiler', not "
                             f"{gradient_cost!r}")
        self._evolved = _Evolved()
        self._evolved_left = _Evolved()  # rho in front of a candidate layer (pair_environments)
        self.heisenberg_sweep = bool(heisenberg_sweep)
        self.checkpoint_bytes = int(checkpoint_bytes)
        self._sweep = (0, [])
        self.pair_transitions = pair_transitions
        self.gradient_cost = gradient_cost
        self._observables = {}    # cost kind -> (key, DeviceDM): the observable pulled back through the right-hand side
        self.backward_passes = 0  # the run_adjoint passes that made them
        if gradient_cost == "local":
            self._refuse_local_without_transitions()

    def _refuse_local_without_transitions(self):
        if not self.pair_transitions:
            raise ValueError("DensityMatrixBackend: gradient_cost='local' needs pair_transitions=True (or 'always'): "
                             "the environments route reads the global cost only")

    # checkpoints pickle the whole compiler including its backend
    def __getstate__(self):
        return {"_evolved": _Evolved(), "_evolved_left": _Evolved(), "heisenberg_sweep": self.heisenberg_sweep,
                "checkpoint_bytes": self.checkpoint_bytes, "_sweep": (0, []),
                "pair_transitions": self.pair_transitions, "gradient_cost": self.gradient_cost,
                "_observables": {}, "backward_passes": 0}

    def sweep_states(self, n, count):
        """``count`` device matrices of n qubits for the Heisenberg sweep, kept from cycle to cycle."""
        from ..device import DeviceDM

        if self._sweep[0] != n:
            for dev in self._sweep[1]:
                dev.close()
            self._sweep = (n, [])
        states = self._sweep[1]
        while len(states) < count:
            states.append(DeviceDM(n))
        return states[:count]

    @staticmethod
    def _refuse_options(compiler):
        if getattr(compiler, "soften_global_cost", False):
            raise NotImplementedError("soften_global_cost is currently only implemented for AerMPSBackend")
        if getattr(compiler, "general_initial_state", False):
            raise NotImplementedError("DensityMatrixBackend does not support general_initial_state (its 2 n-qubit "
                                      "circuit): use QiskitSamplingBackend")

    def _run(self, compiler):
        from ..noise import trajectory_program

        self._refuse_options(compiler)
        n = compiler.full_circuit.num_qubits
        _refuse_width(n, "DensityMatrixBackend")
        qc = without_classical_operations(compiler.full_circuit)
        for q in range(n):
            qc.measure(q, q)
        rows, _, _ = trajectory_program(qc, (getattr(compiler, "execute_kwargs", None) or {}).get("noise_model"))
        return self._evolved.state(n, rows)

    def evaluate_global_cost(self, compiler):
        """1 - rho_00 / Tr rho: the expectation of the sampling backend's 1 - count("0...0") / shots."""
        dev = self._run(compiler)
        return 1 - dev.prob0() / dev.trace()

    def evaluate_local_cost(self, compiler):
        """The mean over the qubits of P(the qubit reads 1)."""
        return float(0.5 * (1 - np.mean(self.measure_qubit_expectation_values(compiler))))

    def measure_qubit_expectation_values(self, compiler):
        dev = self._run(compiler)
        trace = dev.trace()
        return [float(z / trace) for z in dev.z_all()]

    def evaluate_circuit(self, compiler):
        """The outcome probabilities as a dict in the counts key format (all qubits, highest leftmost);
        outcomes of probability 0 are left out."""
        dev = self._run(compiler)
        n = compiler.full_circuit.num_qubits
        p = dev.probabilities() / dev.trace()
        return {format(int(k), f"0{n}b"): float(p[k]) for k in np.flatnonzero(p > 0)}

    def pair_rdms(self, compiler, pairs):
        """The exact 4x4 mixed RDM of every pair (index 2 bit_hi + bit_lo), divided by Tr rho: the ISL
        sweep's input (``pair_entanglement_measures``)."""
        dev = self._run(compiler)
        return dev.pair_rdms(pairs) / dev.trace()

    def pair_environments(self, compiler, pairs):
        """(envs, trace, effects) for the noise-aware general gradient: rho evolved by the program of
        ``full_circuit[:variational_circuit_range()[1]]`` (no measures; kept in a cache of its own, so the
        cost's rho stays), Tr rho, the [n, 4] effects of reading all zeros pulled back through the
        compiler's right-hand side and the error on ``measure`` (``noise.terminal_effects``), and complex
        [len(pairs), 4, 4] environments of ``pairs`` (``DeviceDM.pair_envs``; not divided by the trace).
        A candidate layer goes exactly between the two: its noisy cost is linear in the pair's R."""
        from ..noise import terminal_effects

        n, full, end, noise_model = self._layer_context(compiler)
        effects = terminal_effects(n, full.data[end:], full, noise_model)  # (refuses before any device work)
        dev = self._left_state(n, full, end, noise_model)
        return dev.pair_envs(pairs, effects), dev.trace(), effects

    def _layer_context(self, compiler):
        """(n, full_circuit, the end of the variational range, the noise model), after the backend's refusals."""
        self._refuse_options(compiler)
        full = compiler.full_circuit
        n = full.num_qubits
        _refuse_width(n, "DensityMatrixBackend")
        noise_model = (getattr(compiler, "execute_kwargs", None) or {}).get("noise_model")
        return n, full, compiler.variational_circuit_range()[1], noise_model

    def _left_state(self, n, full, end, noise_model):
        """rho in front of a candidate layer: evolved by the program of ``full[:end]``, kept in a cache of its own."""
        from ..noise import trajectory_program
        from ..utils import circuit_operations as co

        left = without_classical_operations(co.extract_inner_circuit(full, (0, end)))
        rows, _, _ = trajectory_program(left, noise_model)
        if getattr(self, "_evolved_left", None) is None:  # (a backend restored from an older checkpoint)
            self._evolved_left = _Evolved()
        return self._evolved_left.state(n, rows)

    def _pulled_back_observable(self, n, full, end, noise_model, cost):
        """M = Lambda^dag(O) on the device: the observable of ``cost`` pulled back through the program of
        ``full[end:]`` and the errors on every qubit's measure.  It depends on the right-hand side, the noise
        model and the cost alone: kept per cost, keyed by the program's bytes, so a compile makes one backward
        pass (``backward_passes`` counts them)."""
        from ..device import DeviceDM
        from ..utils.cached_rotations import load_cost_observable, noisy_rows

        rows = noisy_rows(full, end, len(full.data), noise_model, measures=True)
        key = (n, rows.tobytes())
        if self._observables is None:  # (a backend restored from an older checkpoint)
            self._observables = {}
        held = self._observables.get(cost)
        if held is not None and held[0] == key:
            return held[1]
        dev = held[1] if held is not None and held[0][0] == n else DeviceDM(n)
        self._observables.pop(cost, None)
        load_cost_observable(dev, cost)
        dev.run_adjoint(rows)
        self.backward_passes += 1
        self._observables[cost] = (key, dev)
        return dev

    def pair_transition_matrices(self, compiler, pairs, cost="global"):
        """(T, trace): complex [len(pairs), 16, 16] transition matrices of ``pairs`` between M, the observable
        of ``cost`` ("global": |0...0><0...0|, "local": diag(popcount / n)) pulled back through everything behind
        the variational range, and rho in front of a candidate layer (``pair_environments``'s cached state);
        Tr rho.  A two-qubit circuit with superoperator S (``noise.layer_superoperator``) placed there has
        Tr(O rho_final) / Tr rho = Re sum(S * T) / trace: the local cost, or 1 minus the global cost."""
        if cost not in ("global", "local"):
            raise ValueError("pair_transition_matrices: cost must be 'global' or 'local'")
        n, full, end, noise_model = self._layer_context(compiler)
        rho = self._left_state(n, full, end, noise_model)
        obs = self._pulled_back_observable(n, full, end, noise_model, cost)
        return obs.pair_transitions(rho, pairs), rho.trace()

    def candidate_layer_costs(self, compiler, pair, circuits, cost="global"):
        """The exact noisy ``cost`` of every two-qubit circuit of ``circuits`` placed on ``pair`` (its qubit 0 on
        ``pair[0]``) at the end of the variational range, errors included: one reader call, then 16x16 host
        arithmetic per circuit -- rho is not evolved."""
        from ..noise import layer_superoperator

        pair = (int(pair[0]), int(pair[1]))
        noise_model = (getattr(compiler, "execute_kwargs", None) or {}).get("noise_model")
        trans, trace = self.pair_transition_matrices(compiler, [pair], cost)
        vals = [float(np.sum(layer_superoperator(qc, pair, noise_model) * trans[0]).real / trace) for qc in circuits]
        return [1.0 - v for v in vals] if cost == "global" else vals

    def _gradient_kind(self, compiler):
        """The cost whose gradient ``general_gradients`` takes."""
        kind = self.gradient_cost
        if kind == "compiler":
            kind = "local" if getattr(compiler, "optimise_local_cost", False) else "global"
        if kind == "local":
            self._refuse_local_without_transitions()
        return kind

    @staticmethod
    def _product_right_hand_side(compiler):
        """Whether every gate behind the variational range acts on one qubit (``terminal_effects`` applies)."""
        from ..circuit import qubit_indices

        full = compiler.full_circuit
        end = compiler.variational_circuit_range()[1]
        return all(len(qubit_indices(full, ins)) == 1 for ins in full.data[end:]
                   if ins.operation.name not in ("barrier", "id", "delay", "measure"))

    def general_gradients(self, compiler):
        """The noise-aware general gradient of every pair of ``compiler.coupling_map``: from the pairs'
        environments (``gradients.noisy_general_grad_of_pairs``), or with ``pair_transitions`` from their
        transition matrices (``gradients.noisy_transition_grad_of_pairs``) when the right-hand side entangles,
        the gradient is the local cost's, or ``pair_transitions="always"``."""
        from ..utils.gradients import noisy_general_grad_of_pairs, noisy_transition_grad_of_pairs

        kind = self._gradient_kind(compiler)
        mode = self.pair_transitions
        if mode == "always" or (mode and (kind == "local" or not self._product_right_hand_side(compiler))):
            return noisy_transition_grad_of_pairs(compiler, kind)
        return noisy_general_grad_of_pairs(compiler)
