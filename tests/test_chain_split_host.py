"""The index conventions of the chain's LDS split (chain epilogue 3: split_lds_body in mps.hip, the
tail of s6_back in svd_gram.h), restated in numpy lane by lane and compared with the formulas of
split_copy_body and the split GEMM, Gamma_copied = W / (sigma lambda) and Gamma_gemm = theta W /
(sigma^2 lambda) with W = V Sigma, in both orientations.

The restatement keeps what the kernel does to the indices: theta' column-major with leading dimension
M, V in the swizzled 128 x 64 LDS layout (kVlPos) written from S6's accumulator layout, the three
reciprocal vectors with zeros for the d != 0 guard, two 16 x 16 tiles per wave over the whole
contraction, three real products per complex one (3M), V on the A side in the orientation that
conjugates it, and the accumulator's (row lk + 4 q, column li) mapping of the 16 x 16 x 4 FP64 MFMA.
No GPU is needed.
"""
import numpy as np
import pytest

CAP = 64


def _pos(row, col):
    return row * 64 + (col ^ (row & 15))


def _mfma(a, b, acc):
    """v_mfma_f64_16x16x4: lane (li, lk) = lane & 15, lane >> 4 holds A[m = li][k = lk] and
    B[k = lk][n = li]; its accumulator element q is D[lk + 4 q][li]."""
    A = a.reshape(4, 16).T          # [m][k]
    B = b.reshape(4, 16)            # [k][n]
    D = A @ B
    lane = np.arange(64)
    li, lk = lane & 15, lane >> 4
    for q in range(4):
        acc[q] += D[lk + 4 * q, li]


def _s6_leave_in_lds(V, sigma, ll, lr, C, K, chl, chr):
    """What s6_back writes on the LDS route: V from the accumulator layout (wave (nt, mg): column 16 nt
    + li, rows 32 mg + 16 t + lk + 4 q; zero past C rows and K columns) and the reciprocals."""
    Vl = np.full(128 * 64, np.nan + 0j)
    Vp = np.zeros((128, 64), dtype=complex)
    Vp[:C, :K] = V
    lane = np.arange(64)
    li, lk = lane & 15, lane >> 4
    for wave in range(16):
        nt, mg = wave & 3, wave >> 2
        for t in range(2):
            for q in range(4):
                row, col = 32 * mg + 16 * t + lk + 4 * q, 16 * nt + li
                Vl[_pos(row, col)] = Vp[row, col]
    assert not np.isnan(Vl).any()   # the whole 128 x 64 is written
    rcp = np.zeros(192)
    for o in range(64):
        x = [sigma[o] if o < K else 0.0, ll[o] if o < chl else 0.0, lr[o] if o < chr else 0.0]
        for a in range(3):
            rcp[64 * a + o] = 1.0 / x[a] if x[a] != 0.0 else 0.0
    return Vl, rcp


def _split_lds(th, Vl, rcp, chl, chr, k):
    """split_lds_body: returns (Gp', Gq') as [2][CAP][CAP] arrays (zeros where nothing is written)."""
    M, N = 2 * chl, 2 * chr
    TR = M >= N
    C = N if TR else M
    gp = np.zeros((2, CAP, CAP), dtype=complex)
    gq = np.zeros((2, CAP, CAP), dtype=complex)
    if TR:
        for e in range(N * k):
            cc, kk = e % N, e // N
            s2 = int(cc >= chr)
            r = cc - s2 * chr
            f = rcp[128 + r] if rcp[kk] != 0.0 else 0.0
            gq[s2, kk, r] = np.conj(Vl[_pos(cc, kk)]) * f
    else:
        for e in range(M * k):
            kk, R = e % k, e // k
            s1 = int(R >= chl)
            l = R - s1 * chl
            f = rcp[64 + l] if rcp[kk] != 0.0 else 0.0
            gp[s1, l, kk] = Vl[_pos(R, kk)] * f
    lane = np.arange(64)
    li, lk = lane & 15, lane >> 4
    outer = M if TR else N
    for wave in range(16):
        rt, ct = wave >> 1, 2 * (wave & 1)
        if 16 * rt >= outer:
            continue
        m = 16 * rt + li
        p = [[np.zeros((4, 64)) for _ in range(2)] for _ in range(3)]
        for s in range((C + 3) >> 2):
            kc = 4 * s + lk
            ok = (m < outer) & (kc < C)
            idx = np.where(ok, kc * M + m if TR else m * M + kc, 0)
            t = np.where(ok, th[idx], 0.0)
            for u in range(2):
                v = Vl[_pos(kc, 16 * (ct + u) + li)]
                if TR:
                    _mfma(t.real, v.real, p[0][u])
                    _mfma(t.imag, v.imag, p[1][u])
                    _mfma(t.real + t.imag, v.real + v.imag, p[2][u])
                else:
                    _mfma(v.real, t.real, p[0][u])
                    _mfma(v.imag, t.imag, p[1][u])
                    _mfma(v.real - v.imag, t.real + t.imag, p[2][u])
        for u in range(2):
            for q in range(4):
                p1, p2, p3 = p[0][u][q], p[1][u][q], p[2][u][q]
                re = p1 - p2 if TR else p1 + p2
                im = p3 - p1 - p2 if TR else p3 - p1 + p2
                kq = 16 * (ct + u) + (li if TR else lk + 4 * q)
                o = 16 * rt + (lk + 4 * q if TR else li)
                ch = chl if TR else chr
                for x in range(64):
                    if kq[x] < k and o[x] < outer:
                        s = int(o[x] >= ch)
                        b = o[x] - s * ch
                        f1, f2 = rcp[kq[x]], rcp[(64 if TR else 128) + b]
                        g = complex(re[x] * f1 * f2, im[x] * f1 * f2)
                        if TR:
                            gp[s, b, kq[x]] = g
                        else:
                            gq[s, kq[x], b] = g
    return gp, gq


def _reference(theta, V, sigma, ll, lr, chl, chr, k):
    """split_copy_body's and the split GEMM's formulas on W = V Sigma, with their d != 0 guards."""
    M, N = 2 * chl, 2 * chr
    TR = M >= N
    W = V * sigma[None, :]          # W[:, kk]: column kk
    gp = np.zeros((2, CAP, CAP), dtype=complex)
    gq = np.zeros((2, CAP, CAP), dtype=complex)

    def div(x, d):
        return x / d if d != 0.0 else 0.0

    U = theta @ W if TR else W.conj().T @ theta   # (M x K) or (K x N)
    for kk in range(k):
        for s in range(2):
            for l in range(chl):
                gp[s, l, kk] = (div(U[s * chl + l, kk], sigma[kk] ** 2 * ll[l]) if TR
                                else div(W[s * chl + l, kk], sigma[kk] * ll[l]))
            for r in range(chr):
                gq[s, kk, r] = (div(np.conj(W[s * chr + r, kk]), sigma[kk] * lr[r]) if TR
                                else div(U[kk, s * chr + r], sigma[kk] ** 2 * lr[r]))
    return gp, gq


# (chl, chr, Gram kept count K, rank rule's kept count k): the full update, both rectangular ones, a
# tail-rule cut below 64, sides that are no multiple of the tiles, a square one below the capacity
SHAPES = [(64, 64, 64, 64), (16, 64, 32, 32), (64, 16, 32, 32), (64, 64, 64, 37), (5, 3, 6, 5), (3, 5, 6, 6),
          (33, 64, 64, 64), (24, 24, 48, 41)]


@pytest.mark.parametrize("chl,chr,K,k", SHAPES)
@pytest.mark.parametrize("zeros", [False, True])
def test_lds_split_matches_the_split_formulas(chl, chr, K, k, zeros):
    rng = np.random.default_rng(1000 * chl + 10 * chr + k)
    M, N = 2 * chl, 2 * chr
    C = min(M, N)
    assert k <= K <= min(C, 64)
    theta = (rng.standard_normal((M, N)) + 1j * rng.standard_normal((M, N))) / np.sqrt(M * N)
    q, _ = np.linalg.qr(rng.standard_normal((C, C)) + 1j * rng.standard_normal((C, C)))
    V = q[:, :K]
    sigma = np.sort(rng.uniform(0.05, 1.0, K))[::-1].copy()
    ll, lr = rng.uniform(0.1, 1.0, chl), rng.uniform(0.1, 1.0, chr)
    if zeros:  # the d != 0 guards: a zero lambda on either side and a zero sigma inside the kept ones
        ll[chl // 2] = 0.0
        lr[chr // 3] = 0.0
        sigma[k - 1] = 0.0
    th = theta.T.reshape(-1).copy()   # theta[R][c] = th[c * M + R]
    Vl, rcp = _s6_leave_in_lds(V, sigma, ll, lr, C, K, chl, chr)
    gp, gq = _split_lds(th, Vl, rcp, chl, chr, k)
    rp, rq = _reference(theta, V, sigma, ll, lr, chl, chr, k)
    # one 3M product over C <= 128 terms and two scalings against one product and a division: a few
    # C eps |theta| |V| / (sigma lambda) in absolute terms
    scale = max(np.abs(rp).max(), np.abs(rq).max())
    tol = 8 * C * 2.0 ** -53 * scale / min(sigma[sigma > 0].min(), 1.0)
    assert np.abs(gp - rp).max() <= tol, (np.abs(gp - rp).max(), tol)
    assert np.abs(gq - rq).max() <= tol, (np.abs(gq - rq).max(), tol)
    assert np.abs(rp).max() > 0 and np.abs(rq).max() > 0
