"""numpy restatements for the noise-aware general gradient's tests (aqc_dm_pair_envs, noise.layer_superoperator,
noise.terminal_effects, gradients.noisy_grads_from_envs).

- ``pair_env``: R = Tr_rest((1 (x) E_rest) rho) of a full matrix, entry by entry from its definition
  R[a, b] = Tr((|b><a|_pair (x) E_rest) rho), index 2 bit_hi + bit_lo;
- ``brute_force_gradients``: every shifted candidate layer inserted into the full circuit, the whole
  program evolved in numpy (trajectory2_ref.density_matrix), parameter shifts of the costs 1 - rho_00 / Tr rho;
- ``case``: the small circuits the host and the device tests share.
"""
import numpy as np

import dm_ref as dref
import sampling_ref as ref
import trajectory2_ref as t2ref
from conftest import to_circuit

ROT = ("rx", "ry", "rz")
# the compiler's default layer (a thinly dressed CNOT) and one with mixed names and a reversed cx
THIN = [("rz", (0,), (0.0,)), ("rz", (1,), (0.0,)), ("cx", (0, 1), ()), ("rz", (0,), (0.0,)), ("rz", (1,), (0.0,))]
MIXED = [("ry", (1,), (0.0,)), ("rx", (0,), (0.0,)), ("cx", (1, 0), ()), ("rz", (1,), (0.0,)), ("cx", (0, 1), ()),
         ("ry", (0,), (0.0,))]


def unpack(w):
    """The Hermitian 2x2 matrix of (E00, E11, Re E01, Im E01)."""
    z = w[2] + 1j * w[3]
    return np.array([[w[0], z], [np.conj(z), w[1]]], dtype=complex)


def pack(e):
    return np.array([e[0, 0].real, e[1, 1].real, e[0, 1].real, e[0, 1].imag])


def pair_env(rho, n, a, b, effects=None):
    """[4, 4]: R[x, y] = Tr((|y><x| on the pair (x) E on the rest) rho); ``effects`` [n, 4] or None
    (identity effects: the RDM)."""
    lo, hi = min(a, b), max(a, b)
    out = np.zeros((4, 4), dtype=complex)
    for x in range(4):
        for y in range(4):
            factors = []
            for q in range(n):
                if q in (lo, hi):
                    bit = 0 if q == lo else 1
                    f = np.zeros((2, 2), dtype=complex)
                    f[(y >> bit) & 1, (x >> bit) & 1] = 1.0
                else:
                    f = np.eye(2, dtype=complex) if effects is None else unpack(effects[q])
                factors.append(f)
            out[x, y] = np.trace(dref.kron_all(factors) @ rho)
    return out


def random_effects(n, seed, kind):
    """[n, 4] by kind: "diagonal" (with |0><0| on qubit n // 2), "mixed" (every other qubit with an
    off-diagonal) or "full" (every qubit with one)."""
    rng = np.random.default_rng(seed)
    eff = np.zeros((n, 4))
    eff[:, :2] = rng.uniform(0.1, 1.0, (n, 2))
    if kind == "diagonal":
        eff[n // 2] = (1.0, 0.0, 0.0, 0.0)
    else:
        off = rng.uniform(-0.3, 0.3, (n, 2))
        if kind == "mixed":
            off[::2] = 0.0
        eff[:, 2:] = off
    return eff


def with_measures(qc):
    out = qc.copy()
    for q in range(qc.num_qubits):
        out.measure(q, q)
    return out


def cost(n, ops, nm):
    """1 - rho_00 / Tr rho of the circuit of ``ops`` with a measure on every qubit, evolved in numpy."""
    from adaptaqc_amd.noise import trajectory_program

    rows, _, _ = trajectory_program(with_measures(to_circuit(n, ops)), nm)
    rho = t2ref.density_matrix(n, rows)
    return 1 - rho[0, 0].real / np.trace(rho).real


def placed(layer, c, t):
    return [(name, tuple((c, t)[q] for q in qs), p) for name, qs, p in layer]


def brute_force_gradients(n, left, right, layer, cmap, nm, rotoselect):
    """sqrt(sum_{i,op} g^2) per ordered pair, g = [C(+pi/2) - C(-pi/2)] / 2 of the costs of
    left + L_{i,op}(theta) on (c, t) + right under ``nm``, each from an evolution of its own."""
    out = []
    for c, t in cmap:
        total = 0.0
        for i, (name, qs, _) in enumerate(layer):
            if name not in ROT:
                continue
            for op in (ROT if rotoselect else (name,)):
                shifted = []
                for theta in (np.pi / 2, -np.pi / 2):
                    cand = list(layer)
                    cand[i] = (op, qs, (theta,))
                    shifted.append(cost(n, left + placed(cand, c, t) + right, nm))
                total += ((shifted[0] - shifted[1]) / 2) ** 2
        out.append(np.sqrt(total))
    return out


def model(local=True):
    """create_noisemodel's relaxation with a correlated depolarizing error on cx and, with ``local``, an
    amplitude damping attached to rz on qubit 1 and a product error to the cx on (0, 2) alone."""
    from adaptaqc_amd import noise
    from adaptaqc_amd.utils.circuit_operations import create_noisemodel

    nm = noise.NoiseModel()
    for name, error in create_noisemodel(50e-3, 70e-3, log_fidelities=False).instructions().items():
        if name != "cx":
            nm.add_all_qubit_quantum_error(error, name)
    nm.add_all_qubit_quantum_error(noise.depolarizing_error(0.04, 2), "cx")
    if local:
        nm.add_quantum_error(noise.amplitude_damping_error(0.15), "rz", (1,))
        nm.add_quantum_error(noise.phase_damping_error(0.2).expand(noise.amplitude_damping_error(0.1)), "cx", (0, 2))
    return nm


def case(n, start):
    """(left ops, right ops, starting ops or None): a seeded brickwork in front, and behind it the
    inverse of a product starting circuit (``start``) or nothing."""
    left = ref.brickwork(n, 2, 300 + n)
    if not start:
        return left, [], None
    rng = np.random.default_rng(400 + n)
    start_ops = []
    for q in range(n):
        start_ops += [("ry", (q,), (float(rng.uniform(-1, 1)),)), ("rz", (q,), (float(rng.uniform(-1, 1)),))]
    right = [(name, qs, (-p[0],)) for name, qs, p in reversed(start_ops)]
    return left, right, start_ops


def full_cmap(n):
    """Every unordered pair once, some of them control-above-target."""
    return [(a, b) if (a + b) % 3 else (b, a) for a in range(n) for b in range(a + 1, n)]
