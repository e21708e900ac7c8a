"""numpy references (complex128, no device code) for the statevector readers of adaptaqc_amd/csrc:
z_all, the one-qubit transition matrix, Pauli strings and the shot sampler, and the one list of
sampling inputs that the host test (test_sv_readers_ref_host.py) and the device test
(test_gpu_sv_readers.py) share.  Pair RDMs use oracle.entanglement.partial_trace_sv; the sampling
rule itself is sampling_ref.sv_sample.

Basis index k has bit q = qubit q (little-endian), as everywhere in the library."""
import numpy as np

import sampling_ref

SEED = 2 ** 40 + 3  # the sampling seed of test_gpu_sampling.py
RUN = 3
TILE = 4096  # amplitudes per sampler tile (sample.hip kTile)


# ---- states ------------------------------------------------------------------------------------
def random_state(n, seed):
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(2 ** n) + 1j * rng.standard_normal(2 ** n)
    psi /= np.linalg.norm(psi)
    return psi


def basis_state(n, k):
    psi = np.zeros(2 ** n, dtype=complex)
    psi[k] = 1.0
    return psi


def embed(n, support_idx, amps):
    """The dense vector with amps on support_idx and zeros elsewhere."""
    psi = np.zeros(2 ** n, dtype=complex)
    psi[np.asarray(support_idx)] = amps
    return psi


# ---- readers -----------------------------------------------------------------------------------
def z_ref(psi, n):
    """<Z_q> = p0 - p1 for q = 0 .. n - 1."""
    p = (np.abs(np.asarray(psi)) ** 2).reshape([2] * n)  # axis j <-> qubit n - 1 - j
    out = np.zeros(n)
    for q in range(n):
        m = p.sum(axis=tuple(j for j in range(n) if j != n - 1 - q))
        out[q] = m[0] - m[1]
    return out


def transition_ref(bra, ket, n, q):
    """T[a][b] = sum_rest conj(bra[rest, q = a]) ket[rest, q = b]."""
    shape = (2 ** (n - 1 - q), 2, 2 ** q)
    return np.einsum("hal,hbl->ab", np.conj(np.asarray(bra)).reshape(shape), np.asarray(ket).reshape(shape))


def apply_1q(psi, n, q, v):
    """V on qubit q of psi."""
    shape = (2 ** (n - 1 - q), 2, 2 ** q)
    return np.einsum("ab,hbl->hal", v, np.asarray(psi).reshape(shape)).reshape(-1)


def random_unitary(seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
    q, r = np.linalg.qr(z)
    return q * (np.diag(r) / np.abs(np.diag(r)))


def sv_pauli_ref(psi, label):
    """Re sum_k conj(psi[k ^ x]) i^ny (-1)^popcount(k & z) psi[k] with the label's masks."""
    x = z = ny = 0
    for q, c in enumerate(reversed(label)):
        if c in "XY":
            x |= 1 << q
        if c in "ZY":
            z |= 1 << q
        ny += c == "Y"
    k = np.arange(len(psi), dtype=np.int64)
    par = k & z
    for s in (32, 16, 8, 4, 2, 1):  # parity of the 64 bits by folding
        par ^= par >> s
    par &= 1
    return float(((1j) ** ny * np.sum(np.conj(psi[k ^ x]) * (1 - 2 * par) * psi[k])).real)


# ---- sampling ----------------------------------------------------------------------------------
def sparse_sample_ref(support_idx, amps, u):
    """(outcomes int64[shots], near bool[shots]) of a state that is zero off support_idx:
    sampling_ref.sv_sample on the support's amplitudes in index order, mapped back through
    support_idx (zero amplitudes add nothing to a prefix sum, so this is the dense rule)."""
    idx = np.asarray(support_idx, dtype=np.int64)
    order = np.argsort(idx)
    k, near = sampling_ref.sv_sample(np.asarray(amps)[order], u)
    return idx[order][k], near


def sparse_neighbours(support_idx, amps, k):
    """sampling_ref.sv_neighbours on the support: the supported outcomes next to k."""
    idx = np.asarray(support_idx, dtype=np.int64)
    order = np.argsort(idx)
    idx = idx[order]
    lo, hi = sampling_ref.sv_neighbours(np.asarray(amps)[order], int(np.searchsorted(idx, k)))
    return int(idx[lo]), int(idx[hi])


def philox_u(n, shots):
    return sampling_ref.uniforms(SEED + n, RUN, shots, 1)[:, 0]


def _normal_amps(rng, count):
    a = rng.standard_normal(count) + 1j * rng.standard_normal(count)
    return a / np.linalg.norm(a)


def _dense(n):
    return lambda: (np.arange(2 ** n), random_state(n, 1000 + n))


def _one_index(k):
    return lambda: (np.array([k]), np.array([1.0 + 0j]))


def _tile9():
    rng = np.random.default_rng(9)
    return 9 * TILE + rng.choice(TILE, 50, replace=False), _normal_amps(rng, 50)


def tiles_1_and_14():
    """30 seeded indices in tile 1 and 30 in tile 14, each tile with total weight 1/2."""
    rng = np.random.default_rng(114)
    idx = np.concatenate([1 * TILE + rng.choice(TILE, 30, replace=False), 14 * TILE + rng.choice(TILE, 30, replace=False)])
    amps = np.concatenate([_normal_amps(rng, 30), _normal_amps(rng, 30)]) / np.sqrt(2.0)
    return idx, amps


def support_n25():
    rng = np.random.default_rng(25)
    idx = rng.choice(2 ** 25, 300, replace=False)
    return idx, _normal_amps(rng, 300)


# name, n, state recipe () -> (support_idx, amps) (a dense state lists every index), shots, and the
# u recipe (n, shots) -> u.  Every case draws u from Philox at (SEED + n, RUN), so the device can
# draw the same numbers itself.
SAMPLING_CASES = [
    dict(name="dense12", n=12, state=_dense(12), dense=True, shots=4097, u=philox_u),  # 1 tile
    dict(name="dense14", n=14, state=_dense(14), dense=True, shots=4097, u=philox_u),  # 4 tiles
    dict(name="dense16", n=16, state=_dense(16), dense=True, shots=4097, u=philox_u),  # 16 tiles
    dict(name="dense20", n=20, state=_dense(20), dense=True, shots=4097, u=philox_u),  # 256 tiles
    dict(name="only_index_0", n=16, state=_one_index(0), dense=False, shots=100, u=philox_u),
    dict(name="only_last_index", n=16, state=_one_index(2 ** 16 - 1), dense=False, shots=100, u=philox_u),
    dict(name="inside_tile_9", n=16, state=_tile9, dense=False, shots=1000, u=philox_u),
    dict(name="tiles_1_and_14", n=16, state=tiles_1_and_14, dense=False, shots=1000, u=philox_u),
    # 8192 tiles: both 4096-tile chunks of the tile scan
    dict(name="sparse25", n=25, state=support_n25, dense=False, shots=4097, u=philox_u),
]
_REFS = {}


def sampling_case(name):
    """(case, support_idx, amps, u, want, near) of a SAMPLING_CASES entry, computed once; callers do
    not modify them."""
    if name not in _REFS:
        case = next(c for c in SAMPLING_CASES if c["name"] == name)
        idx, amps = case["state"]()
        u = case["u"](case["n"], case["shots"])
        want, near = sparse_sample_ref(idx, amps, u)
        _REFS[name] = (case, idx, amps, u, want, near)
    return _REFS[name]
