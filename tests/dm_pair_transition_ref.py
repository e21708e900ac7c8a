"""numpy restatements for the pair-transition reader's tests (aqc_dm_pair_transitions,
gradients.noisy_grads_from_transitions, DensityMatrixBackend's two-matrix route).

- ``pair_transition``: T[j', j] = sum_o conj(A[j', o]) B[j, o] at the pair's local index
  j = (r_lo + 2 r_hi) + 4 (c_lo + 2 c_hi), from the definition by reshape and one matrix product;
- ``contract``: T summed over the partner's equal indices, one qubit's 4x4 ``dm_sweep_ref.transition``;
- ``local_cost`` / ``global_cost`` and ``brute_force_gradients``: every shifted candidate layer inserted into
  the full circuit, the whole program evolved in numpy, parameter shifts of either cost;
- ``observable`` / ``pulled_back``: the cost observables and M = Lambda^dag(O) through a right-hand side with the
  errors on its measures (``dm_sweep_ref.adjoint``);
- ``ENTANGLING_RIGHT``: a right-hand side with cx gates, what an entangling starting circuit leaves.
"""
import numpy as np

import dm_gradient_ref as gref
import dm_sweep_ref as sref
import trajectory2_ref as t2ref
from conftest import to_circuit


def local16(x, n, p, q):
    """X [2^n, 2^n] as [16, 4^(n-2)]: row j = (r_lo + 2 r_hi) + 4 (c_lo + 2 c_hi), lo / hi the smaller / larger
    of p and q, the other index bits along the columns."""
    lo, hi = min(p, q), max(p, q)
    t = np.asarray(x, dtype=complex).reshape((2,) * (2 * n))  # row bits n-1 .. 0, then column bits n-1 .. 0
    front = [2 * n - 1 - hi, 2 * n - 1 - lo, n - 1 - hi, n - 1 - lo]  # c_hi, c_lo, r_hi, r_lo
    return np.moveaxis(t, front, [0, 1, 2, 3]).reshape(16, -1)


def pair_transition(a, b, n, p, q):
    return local16(a, n, p, q).conj() @ local16(b, n, p, q).T


def contract(t, which):
    """[4, 4] at one qubit's index r + 2 c: the pair's T summed over the other qubit's equal indices
    (``which`` "lo" or "hi": the qubit kept)."""
    t8 = np.asarray(t).reshape((2,) * 8)  # c_hi', c_lo', r_hi', r_lo', c_hi, c_lo, r_hi, r_lo
    spec = "xaybxcyd->abcd" if which == "lo" else "axbycxdy->abcd"
    return np.einsum(spec, t8).reshape(4, 4)


def observable(n, cost):
    """O of a cost Tr(O rho) / Tr rho: |0...0><0...0| (1 minus the global cost) or diag(popcount / n) (the local)."""
    dim = 2 ** n
    if cost == "global":
        o = np.zeros((dim, dim), dtype=complex)
        o[0, 0] = 1.0
        return o
    return np.diag([bin(k).count("1") / n for k in range(dim)]).astype(complex)


def pulled_back(n, right_ops, nm, cost):
    """M: the observable pulled back through the program of ``right_ops`` and a measure on every qubit."""
    from adaptaqc_amd.noise import trajectory_program

    rows, _, _ = trajectory_program(gref.with_measures(to_circuit(n, right_ops)), nm)
    return sref.adjoint(n, rows, observable(n, cost))


def final_rho(n, ops, nm):
    from adaptaqc_amd.noise import trajectory_program

    rows, _, _ = trajectory_program(gref.with_measures(to_circuit(n, ops)), nm)
    return t2ref.density_matrix(n, rows)


def global_cost(n, ops, nm):
    rho = final_rho(n, ops, nm)
    return 1 - rho[0, 0].real / np.trace(rho).real


def local_cost(n, ops, nm):
    """The mean over the qubits of P(the qubit reads 1)."""
    rho = final_rho(n, ops, nm)
    pop = np.array([bin(k).count("1") for k in range(2 ** n)])
    return float(np.sum(pop * np.diag(rho).real) / n / np.trace(rho).real)


def brute_force_gradients(n, left, right, layer, cmap, nm, rotoselect, cost):
    """``dm_gradient_ref.brute_force_gradients`` for either cost (``cost``: ``global_cost`` or ``local_cost``)."""
    out = []
    for c, t in cmap:
        total = 0.0
        for i, (name, qs, _) in enumerate(layer):
            if name not in gref.ROT:
                continue
            for op in (gref.ROT if rotoselect else (name,)):
                shifted = []
                for theta in (np.pi / 2, -np.pi / 2):
                    cand = list(layer)
                    cand[i] = (op, qs, (theta,))
                    shifted.append(cost(n, left + gref.placed(cand, c, t) + right, nm))
                total += ((shifted[0] - shifted[1]) / 2) ** 2
        out.append(np.sqrt(total))
    return out


# the inverse of a starting circuit with entangling gates, on 3 and on 4 qubits
ENTANGLING_RIGHT = {
    3: [("cx", (0, 1), ()), ("ry", (1,), (0.7,)), ("rz", (2,), (-0.4,)), ("cx", (2, 1), ()), ("rx", (0,), (0.5,)),
        ("ry", (2,), (-0.9,))],
    4: [("cx", (0, 1), ()), ("ry", (1,), (0.7,)), ("cx", (3, 2), ()), ("rz", (2,), (-0.4,)), ("cx", (2, 1), ()),
        ("rx", (0,), (0.5,)), ("ry", (3,), (-0.9,))],
}


def entangling_start(n):
    """The starting circuit whose inverse ENTANGLING_RIGHT[n] is."""
    return [(name, qs, tuple(-x for x in p)) for name, qs, p in reversed(ENTANGLING_RIGHT[n])]
