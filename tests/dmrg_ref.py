"""numpy restatement of the two-site DMRG of dmrg.hip, for the DMRG tests.  Nothing here uses the package
or the GPU.

An MPS is the Aer-format pair (list of (G0, G1), list of lambda) that ``DeviceMPS.to_aer()`` returns, in
Vidal form; ``forms`` gives A_i = lambda_i Gamma_i (left-orthonormal in a canonical state), B_i = Gamma_i
lambda_{i+1} (right-orthonormal; what ``DeviceMPS.preprocessed()`` returns) and the lambdas with the two
boundary ones.  At bond b (sites b, b + 1) a vector in theta's layout has the index
(s2 chi_r + r) 2 chi_l + s1 chi_l + l, i.e. the C-order shape (s2, r, s1, l).

  heff_dense     P^dag H P from the dense H and the isometry P of the two bases (n <= 10)
  heff_terms     the per-term environment formula: y = sum_t c_t (L_t x sigma_b x sigma_{b+1} x R_t) x with
                 E'[b'][k'] = sum_{s,t} P[s][t] conj(A_s[b][b']) E[b][k] A_t[k][k'] from the identity, and the
                 mirror image with B on the right
  dmrg           a plain two-site DMRG: dense SVD, numpy eigh of the Lanczos tridiagonal, the stop rule of
                 calculate_ground_state_mps
"""
import numpy as np

import pauli_apply_ref as ref

PAULI = {
    "I": np.eye(2, dtype=complex),
    "X": np.array([[0, 1], [1, 0]], dtype=complex),
    "Y": np.array([[0, -1j], [1j, 0]], dtype=complex),
    "Z": np.diag([1.0 + 0j, -1.0]),
}
EPS = 2.220446049250313e-16
BREAKDOWN = 256.0  # Lanczos breakdown at beta <= BREAKDOWN eps S, as dmrg.hip


def forms(mps):
    gam, lam = mps
    n = len(gam)
    lams = [np.ones(1)] + [np.asarray(x, dtype=float) for x in lam] + [np.ones(1)]
    G = [np.stack([np.asarray(a, dtype=complex), np.asarray(b, dtype=complex)]) for a, b in gam]
    A = [lams[i][None, :, None] * G[i] for i in range(n)]
    B = [G[i] * lams[i + 1][None, None, :] for i in range(n)]
    return A, B, lams


def vidal_from_vector(psi):
    """The canonical Vidal form of a state vector (index bit q = qubit q), no truncation."""
    psi = np.asarray(psi, dtype=complex)
    n = int(np.log2(psi.size))
    gam, lam = [], []
    rest = psi.reshape(1, -1)  # (chi, remaining index), qubit i the lowest remaining bit
    prev = np.ones(1)
    for i in range(n - 1):
        chi = rest.shape[0]
        m = rest.reshape(chi, -1, 2).transpose(0, 2, 1).reshape(chi * 2, -1)  # rows (chi, s_i)
        u, s, vh = np.linalg.svd(m, full_matrices=False)
        keep = s > 1e-14 * s[0]
        u, s, vh = u[:, keep], s[keep], vh[keep]
        a = u.reshape(chi, 2, -1).transpose(1, 0, 2)  # A_i[s][l][r]
        g = a / prev[None, :, None]
        gam.append((g[0], g[1]))
        lam.append(s)
        prev = s
        rest = s[:, None] * vh
    a = rest.reshape(rest.shape[0], 2, 1).transpose(1, 0, 2)
    g = a / prev[None, :, None]
    gam.append((g[0], g[1]))
    return gam, lam


def to_vector(mps):
    _, B, _ = forms(mps)
    m = np.ones((1, 1), dtype=complex)  # (index of the sites so far, chi)
    for b in B:
        m = np.einsum("ok,skj->soj", m, b).reshape(-1, b.shape[2])
    return m[:, 0]


def term_list(operator, n):
    """[(c, [letter of qubit 0, ...])] of a {label: coefficient} dict."""
    out = []
    for label, c in operator.items():
        assert len(label) == n
        out.append((complex(c).real, list(reversed(label))))
    return out


def _left_basis(A, b):
    m = np.ones((1, 1), dtype=complex)
    for i in range(b):
        m = np.einsum("ok,skj->soj", m, A[i]).reshape(-1, A[i].shape[2])
    return m  # (2^b, chi_l)


def _right_basis(B, b):
    n = len(B)
    m = np.ones((1, 1), dtype=complex)
    for i in range(n - 1, b + 1, -1):
        m = np.einsum("skj,oj->osk", B[i], m).reshape(-1, B[i].shape[1])
    return m  # (2^(n-b-2), chi_r)


def heff_dense(operator, mps, b):
    """P^dag H P at bond b as a (4 chi_l chi_r)^2 matrix in theta's layout, and the isometry P."""
    A, B, _ = forms(mps)
    n = len(A)
    pl, pr = _left_basis(A, b), _right_basis(B, b)
    eye = np.eye(2)
    p = np.einsum("Rr,ab,cd,Ll->RacLbrdl", pr, eye, eye, pl).reshape(1 << n, -1)
    h = ref.dense_hamiltonian(operator, n)
    return p.conj().T @ h @ p, p


def _step_left(E, A, P):
    return np.einsum("st,sbc,bk,tkj->cj", P, A.conj(), E, A, optimize=True)


def _step_right(E, B, P):
    # E[b][k] (bra, ket) of the sites to the right
    return np.einsum("st,sbc,tkj,cj->bk", P, B.conj(), B, E, optimize=True)


def term_environments(letters, A, B, b):
    """(L, R) of one Pauli string at bond b: L[bra][ket] over the sites < b, R[bra][ket] over the sites > b + 1."""
    L = np.ones((1, 1), dtype=complex)
    for i in range(b):
        L = _step_left(L, A[i], PAULI[letters[i]])
    R = np.ones((1, 1), dtype=complex)
    for i in range(len(A) - 1, b + 1, -1):
        R = _step_right(R, B[i], PAULI[letters[i]])
    return L, R


def bond_operator(operator, mps, b):
    """x -> H_eff x at bond b by the per-term formula (the environments are built once); x in theta's layout."""
    A, B, _ = forms(mps)
    n = len(A)
    chl, chr_ = A[b].shape[1], B[b + 1].shape[2]
    parts = []
    for c, letters in term_list(operator, n):
        if all(ch == "I" for ch in letters):
            continue  # the constant is kept outside H_eff
        L, R = term_environments(letters, A, B, b)
        parts.append((c, PAULI[letters[b + 1]], R, PAULI[letters[b]], L))

    def apply(x):
        xt = np.asarray(x, dtype=complex).reshape(2, chr_, 2, chl)
        y = np.zeros_like(xt)
        for c, p2, R, p1, L in parts:
            y += c * np.einsum("ab,rq,cd,lk,bqdk->arcl", p2, R, p1, L, xt, optimize=True)
        return y.reshape(-1)

    return apply


def heff_terms(operator, mps, b, x):
    """y = H_eff x by the per-term formula; x in theta's layout."""
    return bond_operator(operator, mps, b)(x)


def shift(operator):
    return sum(complex(c).real for label, c in operator.items() if set(label) == {"I"})


def lanczos_lowest(apply, v0, k, thresh):
    """(Ritz value, Ritz vector, breakdown) of k Lanczos steps with full reorthogonalisation from v0."""
    dim = v0.size
    V = [v0 / np.linalg.norm(v0)]
    alphas, betas = [], []
    brk = False
    for j in range(k):
        w = apply(V[j])
        alpha = 0.0
        for _ in range(2):
            for i in range(j, -1, -1):
                h = np.vdot(V[i], w)
                w = w - h * V[i]
                if i == j:
                    alpha += h.real
        alphas.append(alpha)
        beta = np.linalg.norm(w)
        if not beta > thresh or j + 1 >= dim:
            brk = True
            break
        if j + 1 == k:
            break
        betas.append(beta)
        V.append(w / beta)
    m = len(alphas)
    T = np.diag(alphas) + np.diag(betas[: m - 1], 1) + np.diag(betas[: m - 1], -1)
    vals, vecs = np.linalg.eigh(T)
    y = sum(vecs[i, 0] * V[i] for i in range(m))
    return float(vals[0]), y / np.linalg.norm(y), brk


def truncation_rank(s, max_chi, threshold):
    """Aer's reduce_zeros on descending singular values: chop sigma^2 <= 1e-16, the cap, then drop the
    smallest while the dropped sum of squares stays below the threshold."""
    s2 = s * s
    k = max(int(np.count_nonzero(s2 > 1e-16)), 1)
    if max_chi:
        k = min(k, max_chi)
    tail = 0.0
    while k > 1 and tail + s2[k - 1] < threshold:
        tail += s2[k - 1]
        k -= 1
    return k


def energy_of(operator, mps):
    psi = to_vector(mps)
    return float(np.vdot(psi, ref.apply_operator(operator, psi)).real / np.vdot(psi, psi).real)


def product_state(n, seed):
    """The seeded product start of calculate_ground_state_mps."""
    rng = np.random.default_rng(seed)
    gam = []
    for _ in range(n):
        t, p = rng.uniform(0.0, np.pi), rng.uniform(0.0, 2.0 * np.pi)
        v = np.array([np.exp(-0.5j * p) * np.cos(t / 2), np.exp(0.5j * p) * np.sin(t / 2)])
        gam.append((v[0].reshape(1, 1), v[1].reshape(1, 1)))
    return gam, [np.ones(1) for _ in range(n - 1)]


def dmrg(operator, n, max_chi=64, threshold=1e-16, tol=1e-9, max_sweeps=30, krylov_dim=6, seed=0):
    """(energy, mps, info) of a plain two-site DMRG from the seeded product state."""
    scale = ref.weight(operator)
    gam, lam = product_state(n, seed)
    G = [np.stack([a, b]) for a, b in gam]
    lams = [np.ones(1)] + [np.asarray(x) for x in lam] + [np.ones(1)]
    energies, ritz, breakdowns = [], [], 0

    def current():
        return [(g[0], g[1]) for g in G], lams[1:-1]

    def update(b):
        nonlocal breakdowns
        mps = current()
        chl, chr_ = G[b].shape[1], G[b + 1].shape[2]
        a = lams[b][None, :, None] * G[b] * lams[b + 1][None, None, :]
        c = G[b + 1] * lams[b + 2][None, None, :]
        theta = np.einsum("slm,tmr->trsl", a, c).reshape(-1)  # (s2, r, s1, l)
        val, vec, brk = lanczos_lowest(bond_operator(operator, mps, b), theta, krylov_dim,
                                       BREAKDOWN * EPS * scale)
        breakdowns += brk
        ritz.append(val + shift(operator))
        m = vec.reshape(2, chr_, 2, chl).transpose(2, 3, 0, 1).reshape(2 * chl, 2 * chr_)  # rows (s1, l), cols (s2, r)
        u, s, vh = np.linalg.svd(m, full_matrices=False)
        k = truncation_rank(s, max_chi, threshold)
        u, s, vh = u[:, :k], s[:k], vh[:k]
        s = s / np.linalg.norm(s)
        lams[b + 1] = s
        G[b] = u.reshape(2, chl, k) / lams[b][None, :, None]
        G[b + 1] = vh.reshape(k, 2, chr_).transpose(1, 0, 2) / lams[b + 2][None, None, :]

    change = np.inf
    for _ in range(max_sweeps):
        for b in range(n - 1):
            update(b)
        for b in range(n - 2, -1, -1):
            update(b)
        energies.append(energy_of(operator, current()))
        if len(energies) > 1:
            change = abs(energies[-1] - energies[-2])
            if change <= tol * scale:
                break
    info = dict(energies=energies, sweeps=len(energies), ritz=ritz, breakdowns=breakdowns, change=change,
                max_bond=max(len(x) for x in lams))
    return energies[-1], current(), info
