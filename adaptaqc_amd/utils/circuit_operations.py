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

"""Circuit surgery helpers used by the compilers (reference utils/circuit_operations/*).

Host-only list manipulation on ``adaptaqc_amd.circuit.QuantumCircuit``; no simulation here
except ``calculate_overlap_between_circuits`` (device statevector engine) and the Pauli-operator
expectation values, which run on the given backend's device engine.
"""
import numpy as np

from ..circuit import CircuitInstruction, Operation, QuantumCircuit

SUPPORTED_1Q_GATES = ["rx", "ry", "rz"]
SUPPORTED_2Q_GATES = ["cx", "cz"]
MINIMUM_ROTATION_ANGLE = 1e-3


def create_1q_gate(gate_name, angle):
    if gate_name not in SUPPORTED_1Q_GATES:
        raise ValueError(f"Unsupported gate {gate_name}")
    return Operation(gate_name, 1, [angle], label=gate_name)


def is_supported_1q_gate(gate):
    if not isinstance(gate, Operation):
        return False
    name = gate.label if gate.label is not None else gate.name
    if "@" in name:
        return False
    return name.split("#")[0] in SUPPORTED_1Q_GATES


def add_gate(circuit, gate, gate_index=None, qubit_indexes=None):
    if gate_index is None:
        gate_index = len(circuit.data)
    circuit.data.insert(gate_index, CircuitInstruction(gate, qubit_indexes or []))


def replace_1q_gate(circuit, gate_index, gate_name, angle):
    """circuit_operations_basic.py:70-110."""
    if gate_name is None:
        return
    qargs = circuit.data[gate_index].qubits
    circuit.data[gate_index] = CircuitInstruction(create_1q_gate(gate_name, angle), qargs)


def add_dressed_cnot(circuit, control, target, thinly_dressed=False, gate_index=None, v1=True, v2=True, v3=True,
                     v4=True):
    """circuit_operations_basic.py:135-189: rz (ry rz) on each qubit, cx, again."""
    if gate_index is None:
        gate_index = len(circuit.data)

    def rot(q, loc):
        add_gate(circuit, create_1q_gate("rz", 0), loc, [q])
        loc += 1
        if not thinly_dressed:
            add_gate(circuit, create_1q_gate("ry", 0), loc, [q])
            add_gate(circuit, create_1q_gate("rz", 0), loc + 1, [q])
            loc += 2
        return loc

    if v1:
        gate_index = rot(control, gate_index)
    if v2:
        gate_index = rot(target, gate_index)
    add_gate(circuit, Operation("cx", 2), gate_index, [control, target])
    gate_index += 1
    if v3:
        gate_index = rot(control, gate_index)
    if v4:
        rot(target, gate_index)


def add_to_circuit(original, to_add, location=None, qubit_subset=None):
    """Insert ``to_add``'s gates at ``location`` (qubit i of to_add -> qubit_subset[i])."""
    if location is None:
        location = len(original.data)
    # a dict maps only the qubits the gates use (the general-initial-state circuit has 2n qubits,
    # its variational gates act on the first n)
    mapping = (lambda q: q) if qubit_subset is None else (lambda q: qubit_subset[q])
    for k, ins in enumerate(to_add.data):
        op = ins.operation.copy()
        if op.label is None and op.name in SUPPORTED_1Q_GATES:
            op.label = op.name
        original.data.insert(location + k, CircuitInstruction(op, [mapping(q) for q in ins.qubits]))


def extract_inner_circuit(circuit, gate_range):
    inner = QuantumCircuit(circuit.num_qubits)
    inner.data = [circuit.data[i] for i in range(*gate_range)]
    return inner


def remove_inner_circuit(circuit, gate_range):
    del circuit.data[gate_range[0]:gate_range[1]]


def replace_inner_circuit(circuit, replacement, gate_range):
    remove_inner_circuit(circuit, gate_range)
    if replacement is not None and len(replacement.data) > 0:
        add_to_circuit(circuit, replacement, gate_range[0])


def circuit_by_inverting_circuit(circuit):
    """circuit_operations_full_circuit.py:364-382 (labels kept, rotation angles negated)."""
    out = QuantumCircuit(circuit.num_qubits)
    for ins in reversed(circuit.data):
        op = ins.operation
        if op.label in SUPPORTED_1Q_GATES:
            inv = op.copy()
            inv.params[0] *= -1
        else:
            inv = op.inverse()
            inv.label = op.label
        out.data.append(CircuitInstruction(inv, ins.qubits))
    return out


def find_num_gates(circuit, gate_range=None):
    """(num_2q_gates, num_1q_gates) over ``gate_range``."""
    if circuit is None:
        return 0, 0
    if gate_range is None:
        gate_range = (0, len(circuit.data))
    n2 = n1 = 0
    for i in range(*gate_range):
        ins = circuit.data[i]
        if ins.operation.name in ("set_matrix_product_state", "barrier", "measure"):
            continue
        if len(ins.qubits) >= 2:
            n2 += 1
        elif len(ins.qubits) == 1:
            n1 += 1
    return n2, n1


def find_angles_in_circuit(circuit, gate_range=None):
    if gate_range is None:
        gate_range = (0, len(circuit.data))
    return [circuit.data[i].operation.params[0] for i in range(*gate_range)
            if is_supported_1q_gate(circuit.data[i].operation)]


def update_angles_in_circuit(circuit, angles, gate_range=None):
    if gate_range is None:
        gate_range = (0, len(circuit.data))
    k = 0
    for i in range(*gate_range):
        op = circuit.data[i].operation
        if is_supported_1q_gate(op):
            op.params[0] = float(angles[k])
            k += 1


def zyz_angles(u):
    """(theta, phi, lam) with u = e^{i g} Rz(phi) Ry(theta) Rz(lam) (OneQubitEulerDecomposer)."""
    u = np.asarray(u, dtype=complex)
    det = np.linalg.det(u)
    v = u / np.sqrt(det)
    theta = 2 * np.arctan2(abs(v[1, 0]), abs(v[0, 0]))
    phiplam = 2 * np.angle(v[1, 1])
    phimlam = 2 * np.angle(v[1, 0])
    return theta, (phiplam + phimlam) / 2, (phiplam - phimlam) / 2


def _prev_on_qubit(circuit, gi):
    req = set(circuit.data[gi].qubits)
    i = gi - 1
    while i >= 0:
        if req & set(circuit.data[i].qubits):
            return circuit.data[i].operation, i
        i -= 1
    return None, None


def remove_unnecessary_1q_gates_from_circuit(circuit, remove_zero_gates=True, remove_small_gates=False,
                                             gate_range=None, min_rotation_angle=MINIMUM_ROTATION_ANGLE):
    """circuit_operations_optimisation.py:73-164."""
    if gate_range is None:
        gate_range = (0, len(circuit.data))
    to_remove, dealt = [], []
    for gi in range(gate_range[1] - 1, gate_range[0] - 1, -1):
        gate = circuit.data[gi].operation
        if gi in to_remove or gi in dealt or not is_supported_1q_gate(gate):
            continue
        if (remove_zero_gates and gate.params[0] == 0) or (
                remove_small_gates and abs(gate.params[0]) < min_rotation_angle):
            to_remove.append(gi)
            continue
        matrix = gate.to_matrix()
        idxs = [gi]
        pg, pi = _prev_on_qubit(circuit, gi)
        while pg is not None and is_supported_1q_gate(pg) and pi >= gate_range[0]:
            if (remove_zero_gates and pg.params[0] == 0) or (
                    remove_small_gates and abs(pg.params[0]) < min_rotation_angle):
                to_remove.append(pi)
            else:
                idxs.append(pi)
                matrix = matrix @ pg.to_matrix()
            pg, pi = _prev_on_qubit(circuit, pi)
        if len(idxs) > 3:
            theta, phi, lam = zyz_angles(matrix)
            replace_1q_gate(circuit, idxs[0], "rz", phi)
            replace_1q_gate(circuit, idxs[1], "ry", theta)
            replace_1q_gate(circuit, idxs[2], "rz", lam)
            dealt += [idxs[1], idxs[2]]
            to_remove += idxs[3:]
        else:
            dealt += idxs
    for i in sorted(set(to_remove), reverse=True):
        del circuit.data[i]


def remove_unnecessary_2q_gates_from_circuit(circuit, gate_range=None):
    """circuit_operations_optimisation.py:167-204."""
    if gate_range is None:
        gate_range = (0, len(circuit.data))
    to_remove, dealt = [], []
    for gi in range(gate_range[1] - 1, gate_range[0] - 1, -1):
        ins = circuit.data[gi]
        if ins.operation.name not in ("cx", "cy", "cz") or gi in to_remove or gi in dealt:
            continue
        pg, pi = _prev_on_qubit(circuit, gi)
        if pg is None or pg.name != ins.operation.name or pi < gate_range[0]:
            continue
        if pi in to_remove or pi in dealt:
            continue
        if circuit.data[pi].qubits == ins.qubits:
            to_remove += [gi, pi]
    for i in sorted(to_remove, reverse=True):
        del circuit.data[i]


def remove_unnecessary_gates_from_circuit(circuit, remove_zero_gates=True, remove_small_gates=False,
                                          gate_range=None):
    """circuit_operations_optimisation.py:30-70: alternate 1q merging and 2q cancellation."""
    gate_range = [0, len(circuit.data)] if gate_range is None else list(gate_range)
    last = len(circuit.data)
    i = 0
    while True:
        if i == 0:
            remove_unnecessary_1q_gates_from_circuit(circuit, remove_zero_gates, remove_small_gates, gate_range)
            i = 1
        else:
            remove_unnecessary_2q_gates_from_circuit(circuit, gate_range)
            i = 0
        new = len(circuit.data)
        if new != last:
            gate_range[1] -= last - new
            last = new
        elif i == 0:
            return


def add_pauli_measurement_rotations(circuit, pauli_label):
    """The basis rotations of circuit_operations_pauli_ops.py:52-62 appended to ``circuit``: X is
    measured after H, Y after S^dagger then H (label in qiskit order: rightmost character = qubit 0)."""
    from ..paulis import label_to_codes

    for q, c in enumerate(label_to_codes(pauli_label, circuit.num_qubits)):
        if c == 2:
            circuit.sdg(q)
        if c in (1, 2):
            circuit.h(q)
    return circuit


def expectation_values_of_pauli_terms(circuit, labels, backend, backend_options=None, execute_kwargs=None):
    """<circuit|P_label|circuit> for every label (qiskit order), as an array; an all-identity label
    gives 1, as the reference counts it (circuit_operations_pauli_ops.py:83-85).

    * ``AerSVBackend``: the circuit is simulated once on the device and every term is evaluated by
      one aqc_sv_pauli_expect launch;
    * ``AerMPSBackend``: one replay under the backend simulator's truncation options, then one
      aqc_mps_pauli_expect call for all terms (the value is <psi|P|psi> of the possibly truncated
      state, not divided by <psi|psi>);
    * ``QiskitSamplingBackend``: per term a copy of the circuit with the reference's basis rotations
      and a measure on every qubit, counts from ``backend.simulator.run(copy, **execute_kwargs)``
      (``shots``, ``seed_simulator``), then the parity average.  A backend built with
      ``pauli_terms="device"`` hands all non-identity terms to one
      ``backend.simulator.pauli_counts`` call instead (under a noise model: ``shots`` trajectories,
      each read out for every term -- statevector trajectories, or MPS trajectories on a simulator built
      with ``mps_trajectories=True, mps_pauli_readout=True``); a term's value is
      (2 plus - shots) / shots.

    ``circuit`` is not modified (its own measure instructions are ignored); ``backend_options`` are
    Aer's and have no meaning here."""
    from ..backends.aer_mps_backend import AerMPSBackend
    from ..backends.aer_sv_backend import AerSVBackend
    from ..backends.qiskit_sampling_backend import QiskitSamplingBackend
    from ..circuit import device_ops_array
    from ..device import DeviceSV
    from ..paulis import terms_to_codes
    from .utilityfunctions import expectation_value_of_pauli_observable

    n = circuit.num_qubits
    labels = list(labels)
    codes = terms_to_codes(labels, n)  # (validates every label before any device work)
    out = np.ones(len(labels))
    todo = [t for t in range(len(labels)) if codes[t].any()]
    if not todo:
        return out
    if isinstance(backend, AerSVBackend):
        state = DeviceSV(n)
        state.apply(device_ops_array(circuit))
        out[todo] = state.pauli_expect(codes[todo])
    elif isinstance(backend, AerMPSBackend):
        out[todo] = backend.device_state(circuit).pauli_expect(codes[todo])
    elif isinstance(backend, QiskitSamplingBackend):
        kwargs = dict(execute_kwargs or {})
        if getattr(backend, "pauli_terms", None) == "device":
            shots = int(kwargs.get("shots", 1024))
            plus = backend.simulator.pauli_counts(circuit, [labels[t] for t in todo], shots=shots,
                                                  seed_simulator=kwargs.get("seed_simulator"),
                                                  noise_model=kwargs.get("noise_model"))
            out[todo] = (2.0 * np.asarray(plus, dtype=float) - shots) / shots
            return out
        for t in todo:
            rotated = circuit.copy()
            rotated.data = [ins for ins in rotated.data if ins.operation.name != "measure"]
            add_pauli_measurement_rotations(rotated, labels[t])
            for q in range(n):
                rotated.measure(q, q)
            counts = backend.simulator.run(rotated, **kwargs).result().get_counts()
            out[t] = expectation_value_of_pauli_observable(counts, labels[t])
    else:
        raise TypeError(f"expectation_values_of_pauli_terms: unsupported backend {type(backend).__name__}")
    return out


def expectation_value_of_pauli_operator(circuit, operator, backend, backend_options=None, execute_kwargs=None):
    """circuit_operations_pauli_ops.py:71-103: sum_label operator[label] <circuit|P_label|circuit> for
    a ``{label: real coefficient}`` dict (qiskit order), an all-identity label contributing its
    coefficient; the terms through ``expectation_values_of_pauli_terms`` (one simulation for all of
    them on the statevector and MPS backends, where the reference runs one circuit per term)."""
    labels = list(operator.keys())
    evs = expectation_values_of_pauli_terms(circuit, labels, backend, backend_options, execute_kwargs)
    value = 0.0
    for label, ev in zip(labels, evs):
        value += operator[label] * float(ev)
    return value


# instruction names of this IR by the pulse they stand for, with the reference's times in ns
# (circuit_operations_running.py:73-79)
NOISE_INSTRUCTION_TIMES = (
    (0, ("u1", "p", "rz", "z", "s", "sdg", "t", "tdg")),  # virtual Z
    (50, ("u2", "h", "sx", "sxdg")),                      # one X90 pulse
    (100, ("u3", "u", "rx", "ry", "x", "y")),             # two X90 pulses
    (300, ("cx",)),                                       # on both qubits
    (1000, ("reset", "measure")),
)


def create_noisemodel(t1, t2, log_fidelities=True):
    """circuit_operations_running.py:72-109: thermal relaxation after every instruction, with the
    reference's instruction times (0 / 50 / 100 / 300 / 1000 / 1000 ns for u1 / u2 / u3 / cx / reset /
    measure) and its scaling of the time constants (t1 and t2 are multiplied by 1e6 and then compared
    with those times).

    The reference attaches the errors to u1 / u2 / u3 / cx / reset / measure and relies on the
    transpiler to bring every circuit to those names.  There is no transpiler here, so the errors are
    also attached to this IR's names for the same pulses (NOISE_INSTRUCTION_TIMES): time 0 (virtual
    Z) for p, rz, z, s, sdg, t, tdg; 50 ns for h, sx, sxdg; 100 ns for u, rx, ry, x, y.  Any other
    gate (cz, swap, unitary, ...) stays noiseless, as a gate without an error does in Aer.

    The "fidelity" logged per instruction is the no-jump weight Tr(K_0^dag K_0) / 2."""
    import logging

    from ..noise import NoiseModel, thermal_relaxation_error

    t1 = t1 * 1e6
    t2 = t2 * 1e6
    model = NoiseModel()
    for time, names in NOISE_INSTRUCTION_TIMES:
        error = thermal_relaxation_error(t1, t2, time)
        if names == ("cx",):
            error = error.expand(thermal_relaxation_error(t1, t2, time))
        model.add_all_qubit_quantum_error(error, list(names))
    if log_fidelities:
        logger = logging.getLogger(__name__)
        logger.info("Noise model fidelities:")
        for name, error in model.instructions().items():
            logger.info(f"['{name}']: {error.no_jump_weight()}")
    return model


def zero_noise_extrapolate(circuit, measurement_function, num_points=10, rng=None):
    """circuit_operations_running.py:112-139: for each probability in linspace(0, 1, num_points) every
    cx gets a ``cx cx`` pair inserted in front of it with that probability, ``measurement_function()``
    is called and ``circuit.data`` is restored; then intercept + amp e^(-x / decay) is fitted to the
    values and the fit at x = -0.5 is returned.  When the fit fails, ``measurement_function()``.
    ``rng``: a numpy Generator (default: numpy's global generator, as in the reference)."""
    import logging

    from scipy.optimize import curve_fit

    draw = rng.random if rng is not None else np.random.random
    calculated_values = []
    probabilities = np.linspace(0, 1, num_points)
    for prob in probabilities:
        original = circuit.data
        circuit.data = list(original)
        try:
            for i in range(len(original) - 1, -1, -1):
                ins = original[i]
                if ins.operation.name == "cx" and draw() < prob:
                    circuit.data.insert(i, ins)
                    circuit.data.insert(i, ins)
            calculated_values.append(measurement_function())
        finally:
            circuit.data = original

    def exp_decay(x, intercept, amp, decay_rate):
        return intercept + amp * np.exp(-1 * x / decay_rate)

    try:
        popt, _ = curve_fit(exp_decay, probabilities, calculated_values, [0, calculated_values[0], 1])
        return exp_decay(-0.5, *popt)
    except RuntimeError as e:
        logging.getLogger(__name__).warning(f"Failed to zero-noise-extrapolate. Error was {e}")
        return measurement_function()


def calculate_overlap_between_circuits(circuit1, circuit2):
    """|<0|U1^dag U2|0>|^2 = |<psi1|psi2>|^2, evaluated on the device statevector engine."""
    from ..circuit import device_ops
    from ..device import DeviceSV

    d = DeviceSV(circuit1.num_qubits)
    d.apply(device_ops(circuit2) + device_ops(circuit1.inverse()))
    return float(abs(d.amp0()) ** 2)
