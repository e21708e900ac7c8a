"""Host side of the wide-bond reader tests: loaded states whose bonds reach into every workgroup's
column slice of the split environment chains (csrc/ent.hip), and the references they are read
against.  numpy and oracle/ only, no device code.

Above capacity 64 the environment chains split by output columns: workgroup w owns columns
w*CW .. w*CW+CW of every environment.  A state loaded with small bonds gives only slice 0 any
columns; the bond lists here give every slice a full bond, some slice other than 0 a partly filled
one, and the upper slices an empty one (cr - c0 < 0).  ragged_vidal_mps builds them in Vidal form
(what the gate updates need); left_canonical_mps builds the same bonds in a gauge that spreads the
weight evenly over the slices, which a Vidal state's descending Schmidt values do not.

References: the oracle's contractions (oracle.mps.mps_expectation_z / mps_dot / extract_amplitude,
oracle.entanglement.mps_rdm), the sampler's restatement (sampling_ref.mps_sample), the
transfer-matrix contraction of a Pauli string, and -- for n <= 21 -- the dense 2^n vector."""
import functools
import os

import numpy as np

from oracle import mps as M

# capacity -> (CW columns per workgroup, NW workgroups per chain): env_split_cols / env_split_nw in
# adaptaqc_amd/csrc/ent.hip (k_env_split<CW, NW>; the Z-sum chains k_zenv use the same table)
SLICES = {128: (32, 4), 256: (64, 4), 512: (128, 4), 1024: (64, 16)}

# One bond list per capacity (dims[k] = bond between sites k - 1 and k).  Every list reaches the
# capacity once (a full slice for every workgroup), has bonds that end strictly inside a slice above
# slice 0 (128: 100 -> 4 of 32 in slice 3, 70 -> 6 in slice 2; 256: 230, 200, 155, 130, 88, 70;
# 512: 450, 390, 270, 200, 155; 1024: 700 -> 60 of 64 in slice 10, 470, 400, 270, ...) and small
# bonds that leave the upper slices empty.  No bond sits close to min(2 * neighbour, 2^k): a nearly
# square unfolding has a tiny smallest singular value, and Gamma = A / lambda is then badly scaled.
DIMS = {
    128: [1, 2, 3, 5, 9, 16, 28, 50, 88, 128, 100, 70, 40, 22, 12, 7, 4, 2, 1],
    256: [1, 2, 3, 5, 9, 16, 28, 50, 88, 155, 230, 256, 200, 130, 70, 40, 22, 12, 7, 4, 2, 1],
    512: [1, 2, 3, 5, 9, 16, 28, 50, 88, 155, 270, 450, 512, 390, 200, 110, 60, 33, 18, 10, 6, 3, 2, 1],
    # (two wide bonds only, for the host time; 1024 and not 1000, or slice 15 would never be full;
    # the right tail mirrors the left start: with ... 560 290 150 80 43 23 12 7 4 2 1 the nearly
    # square last sites pushed the smallest Schmidt value of bond 1024 down to 2e-7)
    1024: [1, 2, 3, 5, 9, 16, 28, 50, 88, 155, 270, 470, 700, 1024, 700, 400, 220, 120, 65, 35, 19, 10, 5, 3, 2, 1],
}
SEEDS = (2100, 2200)  # first and second state of a capacity: seed = SEEDS[which] + cap
SCHMIDT_FLOOR = 1e-6  # lambda^2 stays far from the 1e-16 chop

# the sampler cases: (seed, run, shots) per capacity; 130 shots are three tiles, the last one short.
# Chosen on the host so that sampling_ref.mps_sample flags at most 2 shots as near a boundary.
SAMPLER = {256: (2 ** 40 + 11, 2, 130), 512: (2 ** 40 + 12, 2, 130), 1024: (2 ** 40 + 13, 2, 130)}

PAULI = {
    "I": np.eye(2, dtype=complex),
    "X": np.array([[0, 1], [1, 0]], dtype=complex),
    "Y": np.array([[0, -1j], [1j, 0]], dtype=complex),
    "Z": np.array([[1, 0], [0, -1]], dtype=complex),
}


def blas_threads():
    """numpy's BLAS on up to 16 threads for the wide QRs, SVDs and contractions (importing bench
    pins it to one for the CPU baseline's workers)."""
    from threadpoolctl import threadpool_limits

    return threadpool_limits(limits=min(16, os.cpu_count() or 1))


def ragged_vidal_mps(dims, seed):
    """Random normalised MPS with exactly the bonds ``dims`` (n + 1 entries, ends 1) in Vidal form
    (Aer tuple): complex-normal site tensors (2, dims[i], dims[i + 1]) through
    bench.vidal_from_tensors.  The bonds must be reachable (<= 2^k, <= 2^(n-k)) and of full rank
    (each at most twice its neighbours), or the canonical form would come out narrower."""
    import bench

    dims = [int(d) for d in dims]
    n = len(dims) - 1
    for k, d in enumerate(dims):
        assert 1 <= d <= min(2 ** k, 2 ** (n - k)), (k, d)
    for k in range(n):
        assert dims[k + 1] <= 2 * dims[k] and dims[k] <= 2 * dims[k + 1], (k, dims[k], dims[k + 1])
    rng = np.random.default_rng(seed)
    A = [rng.standard_normal((2, dims[i], dims[i + 1])) + 1j * rng.standard_normal((2, dims[i], dims[i + 1]))
         for i in range(n)]
    with blas_threads():
        return bench.vidal_from_tensors(A)


def left_canonical_mps(dims, seed):
    """The same kind of random state as ragged_vidal_mps, left in the left-canonical gauge with
    every lambda = 1 (Aer tuple; a valid input of the readers, which contract A = Gamma lambda as
    they find it, but not of the gate updates).  In Vidal form bond index k carries the weight
    lambda_k^2, and the top slice of a wide bond holds the smallest Schmidt values (1e-5 of the
    weight at 512, 1e-8 at 1024): a wrong top slice moves a Vidal state's <Z> by that much only.  Here the left
    environments are identities, the right ones dense, and the bond indices randomly permuted, so
    every slice carries about its share CW / cap of the weight in every result."""
    dims = [int(d) for d in dims]
    n = len(dims) - 1
    rng = np.random.default_rng(seed)
    A = [rng.standard_normal((2, dims[i], dims[i + 1])) + 1j * rng.standard_normal((2, dims[i], dims[i + 1]))
         for i in range(n)]
    with blas_threads():
        for i in range(n - 1):
            s, l, r = A[i].shape
            assert 2 * l >= r, (i, l, r)  # (an isometry: the bond keeps its width)
            q, rr = np.linalg.qr(A[i].transpose(1, 0, 2).reshape(l * s, r))
            # (QR orders the bond like Gram-Schmidt, heavy columns first: shuffle them over the slices)
            perm = rng.permutation(r)
            q, rr = q[:, perm], rr[perm, :]
            A[i] = q.reshape(l, s, r).transpose(1, 0, 2)
            A[i + 1] = rr @ A[i + 1]
    A[n - 1] /= np.linalg.norm(A[n - 1])
    return [(a[0].copy(), a[1].copy()) for a in A], [np.ones(dims[i]) for i in range(1, n)]


def slice_fill(dims, cap):
    """Per workgroup w of the split at ``cap``: the columns min(CW, d - w*CW) it owns of every
    bond d that reaches its slice (d > w*CW)."""
    cw, nw = SLICES[cap]
    return [[min(cw, d - w * cw) for d in dims if d > w * cw] for w in range(nw)]


def bonds_of(aer):
    gam, _ = aer
    return [1] + [np.asarray(a).shape[1] for a, _ in gam]


def min_schmidt(aer):
    return min(float(np.min(l)) for l in aer[1])


def widest(dims):
    """k of the widest bond: it lies between sites k - 1 and k."""
    return int(np.argmax(dims))


@functools.lru_cache(maxsize=None)
def _state(cap, which):
    return ragged_vidal_mps(DIMS[cap], SEEDS[which] + cap)


def state(cap, which=0):
    """The Aer tuple of DIMS[cap] with seed SEEDS[which] + cap, built once per process; read-only."""
    return _state(int(cap), int(which))


@functools.lru_cache(maxsize=None)
def flat_state(cap):
    """left_canonical_mps of DIMS[cap], built once per process; read-only."""
    return left_canonical_mps(DIMS[cap], 2300 + cap)


def preprocessed(aer):
    return M.MPS.from_aer(aer).preprocessed()


def dense(aer):
    """The 2^n vector of an Aer tuple (qubit 0 the lowest bit of the index); n <= 21."""
    gam, lam = aer
    assert len(gam) <= 21
    v = np.ones((1, 1), dtype=complex)  # [index, bond]
    for i, (g0, g1) in enumerate(gam):
        a = np.stack([g0, g1])
        if i < len(gam) - 1:
            a = a * np.asarray(lam[i])[None, None, :]
        v = np.einsum("xl,slr->sxr", v, a).reshape(-1, a.shape[2])  # the new site is the high bit
    return v[:, 0]


def dense_z(psi):
    """<Z_i> of every qubit of a dense vector."""
    n = int(round(np.log2(len(psi))))
    p = np.abs(np.asarray(psi)) ** 2
    idx = np.arange(len(p))
    return np.array([np.sum(p * (1.0 - 2.0 * ((idx >> q) & 1))) for q in range(n)])


def oracle_z(pre):
    """The oracle's <Z_i> of every site (a full contraction each)."""
    with blas_threads():
        return np.array([M.mps_expectation_z(pre, i) for i in range(len(pre))])


def oracle_rdms(pre, pairs):
    from oracle import entanglement as OE

    with blas_threads():
        return np.array([OE.mps_rdm(pre, a, b) for a, b in pairs])


def mps_pauli_ref(tensors, label):
    """Transfer-matrix contraction over the whole chain: E <- sum_{s,t} P[s][t] A_s^H E A_t (qiskit
    label: the rightmost character is qubit 0)."""
    E = np.ones((1, 1), dtype=complex)
    for q, A in enumerate(tensors):
        P = PAULI[label[len(label) - 1 - q]]
        En = np.zeros((A.shape[2], A.shape[2]), dtype=complex)
        for s in range(2):
            for t in range(2):
                if P[s, t] != 0:
                    En += P[s, t] * (A[s].conj().T @ E @ A[t])
        E = En
    return float(E[0, 0].real)


def label_of(n, ops):
    chars = ["I"] * n
    for q, p in ops.items():
        chars[n - 1 - q] = p
    return "".join(chars)


def wide_labels(n, k):
    """The label set of test_gpu_pauli.py::mps_labels with the interior site replaced by the two
    sites beside the widest bond (k - 1, k): supports that start or end there, from either end of
    the chain, across the bond, and the full-weight and random strings that run through it."""
    a, b = k - 1, k
    out = ["I" * n]
    for p in "XYZ":  # support 1 on each side of the wide bond
        out += [label_of(n, {a: p}), label_of(n, {b: p})]
    out += [label_of(n, {a: "Y", b: "Y"}), label_of(n, {a - 1: "X", a: "Z"}), label_of(n, {b: "Z", b + 1: "X"})]
    out += [label_of(n, {0: "Z", a: "X"}), label_of(n, {0: "X", b: "Y"}), label_of(n, {a: "Y", n - 1: "Z"}),
            label_of(n, {b: "X", n - 1: "Y"}), label_of(n, {1: "X", a: "Z", n - 2: "Y"})]
    out += [label_of(n, {0: "Z", n - 1: "Z"})]
    rng = np.random.default_rng(1000 + n)
    out.append("".join(rng.choice(list("XYZ"), n)))  # full weight
    out += ["".join(rng.choice(list("IXYZ"), n)) for _ in range(2)]
    return out


def rdm_pairs(n, k, three_lowers=False):
    """Pairs of the widest bond k (between sites k - 1 and k): the chain's two ends, left of the
    bond, across it (adjacent, and reversed at a distance), right of it.  Their lower qubits are
    0, k - 1 and k; without ``three_lowers`` (each lower qubit runs a chain through every wide bond
    to its right: the 1024 budget) also k - 3 and k + 1."""
    pairs = [(0, n - 1), (0, 2), (k - 1, k), (k + 3, k - 1), (k, k + 2)]
    if not three_lowers:
        pairs += [(k - 3, k - 2), (k - 3, k + 2), (k + 1, n - 1)]
    return pairs
