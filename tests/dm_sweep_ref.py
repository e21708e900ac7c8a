"""numpy restatements for the Heisenberg-picture pieces of the density-matrix engine
(adaptaqc_amd/csrc/dm.hip: aqc_dm_apply_adjoint, aqc_dm_plan_adjoint, aqc_dm_transition).

- ``forward`` / ``adjoint``: program rows applied to an arbitrary matrix X [2^n, 2^n] -- a gate row as
  U X U^dag (adjoint: U^dag X U), a Kraus row or group as sum_k K_k X K_k^dag (adjoint: sum_k K_k^dag X K_k),
  the adjoint in reverse program order;
- ``replay_from``: plan steps applied to vec(X), as ``dm_ref.replay`` but from a start value;
- ``transition``: T[j', j] = sum_o conj(A[j', o]) B[j, o], j = r_q + 2 c_q, by reshape and einsum.
"""
import numpy as np

import dm_ref
import trajectory2_ref as t2ref
from trajectory_ref import apply


def _full(n, rows):
    """[[the 2^n x 2^n matrix of every operator] per event], program order."""
    eye = np.eye(2 ** n, dtype=complex)
    return [[apply(eye, n, m, qs).T for m in mats] for mats, qs, _ in t2ref.events(rows)]


def forward(n, rows, x):
    x = np.asarray(x, dtype=complex)
    for ops in _full(n, rows):
        x = sum(f @ x @ f.conj().T for f in ops)
    return x


def adjoint(n, rows, x):
    x = np.asarray(x, dtype=complex)
    for ops in reversed(_full(n, rows)):
        x = sum(f.conj().T @ x @ f for f in ops)
    return x


def replay_from(n, steps, x):
    """X [2^n, 2^n] after the plan steps (conventions of ``dm_ref.replay``)."""
    dim = 2 ** n
    vec = np.ascontiguousarray(np.asarray(x, dtype=complex).T).reshape(-1)  # index r + (c << n)
    for st in steps:
        nq = int(st["nq"])
        d = 2 ** nq
        m = np.asarray(st["m"], dtype=np.float64).view(np.complex128)
        axes = dm_ref._local_axes(n, st)
        t = np.moveaxis(vec.reshape((2,) * (2 * n)), axes, range(len(axes))).reshape(d * d, -1)
        if int(st["kind"]) == 0:  # X <- U X U^dag with X[r, c] = x[r + d c]
            u = m[: d * d].reshape(d, d)
            t = np.einsum("ar,crk,bc->bak", u, t.reshape(d, d, -1), u.conj()).reshape(d * d, -1)
        else:
            t = m[: d ** 4].reshape(d * d, d * d) @ t
        vec = np.moveaxis(t.reshape((2,) * len(axes) + (2,) * (2 * n - len(axes))), range(len(axes)), axes).reshape(-1)
    return np.ascontiguousarray(vec.reshape(dim, dim).T)


def local4(x, n, q):
    """X [2^n, 2^n] as [4, 4^(n-1)]: row j = r_q + 2 c_q, the other index bits along the columns."""
    t = np.asarray(x, dtype=complex).reshape((2,) * (2 * n))  # row bits n-1 .. 0, then column bits n-1 .. 0
    return np.moveaxis(t, [2 * n - 1 - q, n - 1 - q], [0, 1]).reshape(4, -1)


def transition(a, b, n, q):
    return np.einsum("po,jo->pj", local4(a, n, q).conj(), local4(b, n, q))


def random_matrix(n, seed):
    rng = np.random.default_rng(seed)
    dim = 2 ** n
    return rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim))
