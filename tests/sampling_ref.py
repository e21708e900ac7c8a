"""numpy restatements of the shot samplers (adaptaqc_amd/csrc/sample.hip), for the sampling tests.

- Philox4x32-10 and the uniform of a counter (include/aqc_hip.h, shot sampling);
- the statevector rule: smallest k whose inclusive prefix sum of |psi_k|^2 exceeds u * total, with
  an np.longdouble cumulative sum;
- the per-site MPS rule on preprocessed tensors A_i (2, chi_l, chi_r) and their right environments.
"""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint32 words (arrays broadcast), key: two.  Returns the four output words."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in counter]
    k = [np.asarray(x, dtype=np.uint64) & _MASK for x in key]
    c = list(np.broadcast_arrays(*c))
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + _W0) & _MASK, (k[1] + _W1) & _MASK]
    return c


def uniforms(seed, run, shots, nper):
    """[shots, nper] uniforms of (seed, run): counter (shot lo, shot hi, site, run)."""
    seed, run = int(seed), int(run)
    shot = np.arange(shots, dtype=np.uint64)[:, None]
    site = np.arange(nper, dtype=np.uint64)[None, :]
    x = philox4x32_10((shot & _MASK, shot >> _S32, site, np.uint64(run & 0xFFFFFFFF)),
                      (np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)))
    hi = (x[0] >> np.uint64(5)).astype(np.float64)
    lo = (x[1] >> np.uint64(6)).astype(np.float64)
    return (hi * 67108864.0 + lo) * (1.0 / 9007199254740992.0)


def sv_sample(psi, u):
    """(outcomes int64[shots], near bool[shots]): the inverse-CDF rule; near marks shots whose u lies
    within 1e-12 of a CDF boundary C_k / P."""
    p = (np.abs(np.asarray(psi)) ** 2).astype(np.longdouble)
    c = np.cumsum(p)
    total = c[-1]
    t = np.asarray(u, dtype=np.longdouble) * total
    k = np.searchsorted(c, t, side="right")  # smallest k with c[k] > t
    nz = np.flatnonzero(p > 0)
    k = np.where(k >= len(p), nz[-1], k)
    cdf = (c / total).astype(np.float64)
    j = np.clip(np.searchsorted(cdf, u), 1, len(cdf) - 1)
    near = np.minimum(np.abs(cdf[j] - u), np.abs(cdf[j - 1] - u)) < 1e-12
    return k.astype(np.int64), near


def sv_neighbours(psi, k):
    """The outcomes with nonzero probability next to k (below, above); k itself where none."""
    nz = np.flatnonzero(np.abs(np.asarray(psi)) ** 2 > 0)
    i = np.searchsorted(nz, k)
    return int(nz[max(i - 1, 0)]), int(nz[min(i + 1, len(nz) - 1)])


def right_environments(tensors):
    """R_i = sum_s A_i^s R_{i+1} A_i^s dag, R_n = [[1]]; list of n + 1 matrices."""
    n = len(tensors)
    envs = [None] * (n + 1)
    envs[n] = np.ones((1, 1), dtype=complex)
    for i in range(n - 1, -1, -1):
        a = np.asarray(tensors[i], dtype=complex)
        envs[i] = sum(a[s] @ envs[i + 1] @ a[s].conj().T for s in range(2))
    return envs


def mps_sample(tensors, u):
    """(bits uint8[shots, n], near bool[shots]): per site w_s = v A^s, p_s = Re(w_s R w_s dag), bit = 1
    iff u (p_0 + p_1) >= p_0, v = w_bit / sqrt(p_bit); near marks shots with
    |u (p_0 + p_1) - p_0| < 1e-10 (p_0 + p_1) at some site."""
    u = np.asarray(u, dtype=np.float64)
    shots, n = u.shape
    envs = right_environments(tensors)
    v = np.ones((shots, 1), dtype=complex)
    bits = np.zeros((shots, n), dtype=np.uint8)
    near = np.zeros(shots, dtype=bool)
    for i in range(n):
        a = np.asarray(tensors[i], dtype=complex)
        w = [v @ a[s] for s in range(2)]
        p = [np.einsum("ij,jk,ik->i", w[s], envs[i + 1], w[s].conj()).real for s in range(2)]
        tot = p[0] + p[1]
        x = u[:, i] * tot
        bit = x >= p[0]
        near |= np.abs(x - p[0]) < 1e-10 * tot
        bits[:, i] = bit
        pb = np.where(bit, p[1], p[0])
        v = np.where(bit[:, None], w[1], w[0]) / np.sqrt(pb)[:, None]
    return bits, near


def unpack_bits(words, n):
    """uint64[shots, words] -> uint8[shots, n] (bit q % 64 of word q // 64 = qubit q)."""
    w = np.asarray(words, dtype=np.uint64)
    q = np.arange(n)
    return ((w[:, q // 64] >> (q % 64).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)


def brickwork(n, depth, seed):
    """Seeded brickwork ops [(name, qubits, params)]: a layer of random rx / ry / rz, then cx on
    alternating neighbours."""
    rng = np.random.default_rng(seed)
    ops = []
    for layer in range(depth):
        for q in range(n):
            ops.append((["rx", "ry", "rz"][rng.integers(3)], (q,), (rng.uniform(-np.pi, np.pi),)))
        for q in range(layer % 2, n - 1, 2):
            ops.append(("cx", (q, q + 1), ()))
    return ops


def chi_square(counts, probs, shots):
    """(statistic, dof) of Pearson's chi-square of observed counts (array over outcomes) against
    probabilities, merging bins with expectation < 5 (in order of increasing expectation)."""
    exp = np.asarray(probs, dtype=float) * shots
    obs = np.asarray(counts, dtype=float)
    order = np.argsort(exp)
    exp, obs = exp[order], obs[order]
    e_bins, o_bins = [], []
    ce = co = 0.0
    for e, o in zip(exp, obs):
        ce += e
        co += o
        if ce >= 5:
            e_bins.append(ce)
            o_bins.append(co)
            ce = co = 0.0
    if ce > 0 and e_bins:
        e_bins[-1] += ce
        o_bins[-1] += co
    e_bins, o_bins = np.array(e_bins), np.array(o_bins)
    return float(np.sum((o_bins - e_bins) ** 2 / e_bins)), len(e_bins) - 1
