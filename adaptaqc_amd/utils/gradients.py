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

"""Candidate-pair gradients on MI355X: drop-in for adaptaqc/utils/gradients.py:23-224.

``general_grad_of_pairs`` keeps the reference signature and return value (list of floats, one
per coupling-map pair) but evaluates every pair's generator overlaps in one device sweep over
|psi> (libaqchip ``aqc_pair_grads``) instead of 1 + Npairs * (Ngen + [U0 != I]) Aer runs.
Starting circuits made of 1-qubit gates give the product state |s> the sweep needs; a starting
circuit with entangling gates takes the per-(pair, generator) device MPS route instead.
"""
from typing import List, Tuple

import numpy as np

from .. import gates as G
from ..circuit import QuantumCircuit, op_matrix, qubit_indices
from ..device import DeviceMPS, pair_grads_batch
from ..mps_operations import device_mps_from_circuit
from .utilityfunctions import get_distinct_items_and_degeneracies

PARAMETERISED = ("rx", "ry", "rz")


def circuit_unitary(qc: QuantumCircuit) -> np.ndarray:
    """Unitary of a small circuit (little-endian over its qubits)."""
    n = qc.num_qubits
    u = np.eye(2 ** n, dtype=complex)
    for ins in qc.data:
        if ins.operation.name in ("barrier", "id"):
            continue
        full = _embed(op_matrix(ins.operation), qubit_indices(qc, ins), n)
        u = full @ u
    return u


def _embed(m, qubits, n):
    k = len(qubits)
    dim = 2 ** n
    out = np.zeros((dim, dim), dtype=complex)
    for col in range(dim):
        sub_in = 0
        for i, q in enumerate(qubits):
            sub_in |= ((col >> q) & 1) << i
        rest = col
        for q in qubits:
            rest &= ~(1 << q)
        for sub_out in range(2 ** k):
            row = rest
            for i, q in enumerate(qubits):
                row |= ((sub_out >> i) & 1) << q
            out[row, col] += m[sub_out, sub_in]
    return out


def product_state_vectors(n, starting_circuit):
    """Per-qubit 2-vectors of |s> = starting_circuit|0..0>, or None if it entangles."""
    s = np.zeros((n, 2), dtype=complex)
    s[:, 0] = 1.0
    if starting_circuit is None:
        return s
    for ins in starting_circuit.data:
        if ins.operation.name in ("barrier", "id"):
            continue
        if len(ins.qubits) != 1:
            return None
        q = qubit_indices(starting_circuit, ins)[0]
        s[q] = op_matrix(ins.operation) @ s[q]
    return s


def general_grad_of_pairs(
    circuit: QuantumCircuit,
    inverse_zero_ansatz: QuantumCircuit,
    generators: List[QuantumCircuit],
    degeneracies: List[int],
    coupling_map: List[Tuple],
    starting_circuit=None,
    backend=None,
    comm=None,
):
    """Euclidean norm over the layer's generators of dC/dtheta at theta=0, for every pair.

    g_ct = sqrt(sum_k deg_k * (-Im(<s|G_k|psi> <psi|U0^dag|s>))^2)  (gradients.py:23-124).
    ``generators`` are the circuits of G_k^dag and ``inverse_zero_ansatz`` that of U0^dag, as
    in the reference (adapt_compiler.py:213-216).

    ``comm`` (not in the reference; None = one process): the ranks of one node share the sweep --
    every rank replays |psi> on its own GPU (deterministic, the same on every rank), scores the
    pairs whose first qubit it owns, and one all-gather of the float64 scores returns the whole
    list on every rank (sharding.sharded_pair_scores; ``TorchComm`` over RCCL / gloo, or
    ``comm.RcclComm`` through the C ABI).
    """
    from ..sharding import sharded_pair_scores

    if backend is None:
        from ..backends.python_default_backends import MPS_SIM as backend
    # the device MPS backend replays from its cached device copy of the target payload (the same
    # data load_aer would upload again: ~3.5 ms of host marshalling and copy per layer at 50 qubits,
    # chi = 64), into its work state; other backends build a fresh state
    replay = getattr(backend, "device_state", None)
    psi = replay(circuit) if replay is not None else device_mps_from_circuit(circuit.copy(), sim=backend.simulator)
    n = circuit.num_qubits
    return sharded_pair_scores(
        lambda pairs: grads_for_state(psi, n, inverse_zero_ansatz, generators, degeneracies, pairs,
                                      starting_circuit, backend),
        coupling_map, n, comm)


def layer_operators(inverse_zero_ansatz, generators):
    u0 = circuit_unitary(inverse_zero_ansatz).conj().T
    gmats = [circuit_unitary(g).conj().T for g in generators]
    return u0, gmats


def grads_for_state(psi: DeviceMPS, n, inverse_zero_ansatz, generators, degeneracies, coupling_map,
                    starting_circuit=None, backend=None):
    if len(coupling_map) == 0:
        return []
    u0, gmats = layer_operators(inverse_zero_ansatz, generators)
    svec = product_state_vectors(n, starting_circuit)
    if svec is not None:
        gens = np.stack(gmats) if gmats else np.zeros((0, 4, 4), dtype=complex)
        out = pair_grads_batch([psi], svec, coupling_map, u0, gens, np.asarray(degeneracies, dtype=float))
        return [float(x) for x in out[0]]
    return _grads_entangled_start(psi, n, inverse_zero_ansatz, generators, degeneracies, coupling_map,
                                  starting_circuit, backend)


def _grads_entangled_start(psi, n, inverse_zero_ansatz, generators, degeneracies, coupling_map,
                           starting_circuit, backend):
    """Reference structure (gradients.py:81-122) with every MPS build and dot on the device."""
    sim = backend.simulator if backend is not None else None
    resolves_to_id = np.allclose(circuit_unitary(inverse_zero_ansatz), np.eye(4))
    if resolves_to_id:
        s = device_mps_from_circuit(starting_circuit.copy(), sim=sim)
        zero_overlap = psi.dot(s)
    out = []
    for control, target in coupling_map:
        if not resolves_to_id:
            st = device_mps_from_circuit(starting_circuit.compose(inverse_zero_ansatz, [control, target]), sim=sim)
            zero_overlap = psi.dot(st)
        g = 0.0
        for gen, deg in zip(generators, degeneracies):
            st = device_mps_from_circuit(starting_circuit.compose(gen, [control, target]), sim=sim)
            ov = st.dot(psi)
            gg = -1 * np.imag(ov * zero_overlap)
            g += (gg ** 2) * deg
        out.append(float(np.sqrt(g)))
    return out


def remove_unnecessary_2q_gates_from_circuit(circuit: QuantumCircuit):
    """Cancel adjacent identical CX/CY/CZ pairs (circuit_operations_optimisation.py:167-204)."""
    data = circuit.data
    to_remove, dealt = [], []
    for gi in range(len(data) - 1, -1, -1):
        ins = data[gi]
        if ins.operation.name not in ("cx", "cy", "cz") or gi in to_remove or gi in dealt:
            continue
        req = set(ins.qubits)
        pi = gi - 1
        while pi >= 0 and not (req & set(data[pi].qubits)):
            pi -= 1
        if pi < 0 or data[pi].operation.name != ins.operation.name:
            continue
        if pi in to_remove or pi in dealt:
            continue
        if data[pi].qubits == ins.qubits:
            to_remove += [gi, pi]
    for i in sorted(to_remove, reverse=True):
        del data[i]


def get_generators_and_degeneracies(ansatz: QuantumCircuit, rotoselect: bool = False, inverse: bool = False):
    """gradients.py:127-170."""
    gens = []
    for i, ins in enumerate(ansatz.data):
        if ins.operation.name in PARAMETERISED:
            for op in (PARAMETERISED if rotoselect else (ins.operation.name,)):
                g = get_generator(ansatz, i, op)
                gens.append(g.inverse() if inverse else g)
    return get_distinct_items_and_degeneracies(gens)


def get_generator(ansatz: QuantumCircuit, index: int, op: str):
    """gradients.py:173-224."""
    if op not in PARAMETERISED:
        raise ValueError("op must be one of rx, ry or rz")
    gen = QuantumCircuit(2)
    for i, ins in enumerate(ansatz.data):
        name = ins.operation.name
        if name not in ("rx", "ry", "rz", "cx"):
            raise ValueError("Circuit must only contain rx, ry, rz and cx gates")
        if i == index:
            getattr(gen, {"rx": "x", "ry": "y", "rz": "z"}[op])(ins.qubits[0])
        if name == "cx":
            gen.cx(*ins.qubits)
    remove_unnecessary_2q_gates_from_circuit(gen)
    return gen


def shifted_layers(layer: QuantumCircuit, rotoselect: bool, shift: float):
    """The candidate circuits L_{i,op}(shift): ``layer`` with every rotation at angle 0 under its own name and
    rotation i replaced by op(shift), for every rotation i and every op in rx, ry, rz (only i's own name
    without ``rotoselect``), in ``get_generators_and_degeneracies``'s order."""
    from ..circuit import CircuitInstruction
    from .circuit_operations import create_1q_gate

    for ins in layer.data:
        if ins.operation.name not in PARAMETERISED + ("cx",):
            raise ValueError("Circuit must only contain rx, ry, rz and cx gates")
    zero = QuantumCircuit(2)
    for ins in layer.data:
        name = ins.operation.name
        op = create_1q_gate(name, 0.0) if name in PARAMETERISED else ins.operation.copy()
        zero.data.append(CircuitInstruction(op, list(ins.qubits)))
    out = []
    for i, ins in enumerate(layer.data):
        if ins.operation.name not in PARAMETERISED:
            continue
        for op in (PARAMETERISED if rotoselect else (ins.operation.name,)):
            qc = QuantumCircuit(2)
            qc.data = list(zero.data)
            qc.data[i] = CircuitInstruction(create_1q_gate(op, float(shift)), list(ins.qubits))
            out.append(qc)
    return out


def _shifted_half_differences(layer, noise_model, rotoselect):
    """half(c, t) -> complex [candidates, 16, 16]: [S(L_{i,op}(+pi/2)) - S(L_{i,op}(-pi/2))] / 2 of every shifted
    candidate of ``layer`` on the ordered pair (c, t) under ``noise_model`` (``noise.layer_superoperator``'s
    index), in ``shifted_layers``'s order; what the noise-aware gradients of every kind share.  Without errors
    attached to particular qubits the maps depend on the pair's orientation alone and are made once each."""
    from ..noise import layer_superoperator

    plus = shifted_layers(layer, rotoselect, np.pi / 2)
    minus = shifted_layers(layer, rotoselect, -np.pi / 2)
    local = noise_model is not None and bool(getattr(noise_model, "_local", None))
    cache = {}

    def half_differences(c, t):
        key = (c, t) if local else c < t
        if key not in cache:
            cache[key] = np.stack([(layer_superoperator(p, (c, t), noise_model)
                                    - layer_superoperator(m, (c, t), noise_model)) / 2
                                   for p, m in zip(plus, minus)]) if plus else np.zeros((0, 16, 16), dtype=complex)
        return cache[key]

    return half_differences


def _pair_gradient_norms(coupling_map, per_pair, value_of):
    """sqrt(sum_{i,op} g^2) per ordered pair: ``value_of((c, t), the pair's entry of per_pair)`` gives the
    g_{i,op} of one pair."""
    out = []
    for (c, t), data in zip(coupling_map, per_pair):
        g = value_of((int(c), int(t)), data)
        out.append(float(np.sqrt(np.sum(g * g))))
    return out


def noisy_grads_from_envs(envs, trace, effects, layer, coupling_map, noise_model, rotoselect):
    """The noise-aware general gradient of every ordered pair (c, t) of ``coupling_map`` from the pairs'
    environments (host only).

    ``envs``: complex [len(coupling_map), 4, 4], R of each pair at the index 2 bit_hi + bit_lo
    (``DeviceDM.pair_envs``; not divided by the trace); ``trace``: Tr rho; ``effects``: [n, 4] as
    ``noise.terminal_effects``.  With S the superoperator of a candidate circuit on (c, t) under
    ``noise_model`` (``noise.layer_superoperator``), C = 1 - Re Tr((E_hi (x) E_lo) S(R)) / Tr rho, and
    g_{i,op} = [C(L_{i,op}(+pi/2)) - C(L_{i,op}(-pi/2))] / 2 is dC/dtheta at 0 exactly (C is a + b cos theta +
    c sin theta in one rotation angle whatever fixed channels follow).  Returns sqrt(sum_{i,op} g^2) per
    pair; with ``noise_model`` None that is the reference's sqrt(sum_k deg_k g_k^2)."""
    envs = np.asarray(envs, dtype=complex).reshape(-1, 4, 4)
    effects = np.asarray(effects, dtype=float)
    if len(envs) != len(coupling_map):
        raise ValueError("noisy_grads_from_envs: one environment per pair of the coupling map")
    half_differences = _shifted_half_differences(layer, noise_model, rotoselect)

    def matrix(e):
        return np.array([[e[0], e[2] + 1j * e[3]], [e[2] - 1j * e[3], e[1]]])

    def value_of(pair, env):
        lo, hi = min(pair), max(pair)
        evec = np.kron(matrix(effects[hi]), matrix(effects[lo])).reshape(-1)  # Tr(E X) = evec . vec(X)
        return -np.real(half_differences(*pair) @ env.reshape(-1, order="F") @ evec) / trace

    return _pair_gradient_norms(coupling_map, envs, value_of)


def noisy_grads_from_transitions(trans, trace, layer, coupling_map, noise_model, rotoselect, sign):
    """``noisy_grads_from_envs``'s gradients from the pairs' transition matrices (host only): for any
    right-hand side and either cost.

    ``trans``: complex [len(coupling_map), 16, 16], T of each pair between the cost observable pulled back
    through everything behind the layer and the state in front of it (``DeviceDM.pair_transitions``); ``trace``:
    Tr rho.  A candidate circuit on (c, t) with superoperator S costs C = ``sign`` Re sum(S * T) / Tr rho plus a
    constant: ``sign`` -1 for the global cost (1 minus that value), +1 for the local cost (the value itself).
    g_{i,op} = [C(L_{i,op}(+pi/2)) - C(L_{i,op}(-pi/2))] / 2, sqrt(sum_{i,op} g^2) per pair, as
    ``noisy_grads_from_envs``."""
    trans = np.asarray(trans, dtype=complex).reshape(-1, 16, 16)
    if len(trans) != len(coupling_map):
        raise ValueError("noisy_grads_from_transitions: one transition matrix per pair of the coupling map")
    half_differences = _shifted_half_differences(layer, noise_model, rotoselect)

    def value_of(pair, t):
        return float(sign) * np.real(np.sum(half_differences(*pair) * t, axis=(1, 2))) / trace

    return _pair_gradient_norms(coupling_map, trans, value_of)


def noisy_general_grad_of_pairs(compiler):
    """The noise-aware general gradient of every pair of ``compiler.coupling_map`` on a
    ``DensityMatrixBackend``: one reader over the evolved rho (``pair_environments``: one
    ``DeviceDM.pair_envs`` call over the unordered pairs) and host arithmetic per candidate
    (``noisy_grads_from_envs``); a pair listed in both orientations shares its environment."""
    cmap = [(int(c), int(t)) for c, t in compiler.coupling_map]
    if not cmap:
        return []
    unordered = sorted({(min(c, t), max(c, t)) for c, t in cmap})
    envs, trace, effects = compiler.backend.pair_environments(compiler, unordered)
    where = {p: k for k, p in enumerate(unordered)}
    envs = np.stack([envs[where[(min(c, t), max(c, t))]] for c, t in cmap])
    noise_model = (getattr(compiler, "execute_kwargs", None) or {}).get("noise_model")
    return noisy_grads_from_envs(envs, trace, effects, compiler.layer_2q_gate, cmap, noise_model,
                                 compiler.use_rotoselect)


def noisy_transition_grad_of_pairs(compiler, cost="global"):
    """``noisy_general_grad_of_pairs`` for any right-hand side and either cost, on a ``DensityMatrixBackend``:
    one ``DeviceDM.pair_transitions`` call over the unordered pairs (``pair_transition_matrices``) and host
    arithmetic per candidate (``noisy_grads_from_transitions``)."""
    cmap = [(int(c), int(t)) for c, t in compiler.coupling_map]
    if not cmap:
        return []
    unordered = sorted({(min(c, t), max(c, t)) for c, t in cmap})
    trans, trace = compiler.backend.pair_transition_matrices(compiler, unordered, cost)
    where = {p: k for k, p in enumerate(unordered)}
    trans = np.stack([trans[where[(min(c, t), max(c, t))]] for c, t in cmap])
    noise_model = (getattr(compiler, "execute_kwargs", None) or {}).get("noise_model")
    return noisy_grads_from_transitions(trans, trace, compiler.layer_2q_gate, cmap, noise_model,
                                        compiler.use_rotoselect, -1.0 if cost == "global" else 1.0)


__all__ = [
    "general_grad_of_pairs",
    "noisy_grads_from_envs",
    "noisy_grads_from_transitions",
    "noisy_general_grad_of_pairs",
    "noisy_transition_grad_of_pairs",
    "get_generators_and_degeneracies",
    "get_generator",
    "circuit_unitary",
    "G",
]
