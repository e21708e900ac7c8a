// Two-site DMRG ground states of a Pauli sum H = sum_t c_t P_t on the MPS engine.
//
// The state is the engine's Vidal MPS in sorted qubit order.  At bond b (sites b, b + 1) the two-site
// theta that k_theta forms (mps.hip) is the wavefunction in the basis (left Schmidt vectors) x s1 x s2 x
// (right Schmidt vectors); the left basis is built from A_i = lambda_i Gamma_i (left-orthonormal), the
// right one from B_i = Gamma_i lambda_{i+1} (right-orthonormal).  A sweep keeps that gauge by itself: the
// split leaves site b as U and site b + 1 as V^H of the SVD, so the identity's environments are the
// identity and are not stored.
//
// Cuts.  Cut p lies between the sites p - 1 and p.  A term with support lo..hi crosses cut p when
// lo < p <= hi.  Per cut the handle stores, on each side, one matrix for the closed sum (left: every
// term with hi < p, times c_t, summed: LH_p; right: every term with lo >= p: RH_p) and one per crossing
// term (slot 1 + its place among the cut's crossing terms, input order).  Left environments are
// [bra][ket], right ones [ket][bra] (so that both act on theta as plain products), row stride cap.
//
//   k_dmrg_env     one step of every environment of a cut through one site, all of them in one launch
//                  (workgroups over output matrices x 64-column blocks), as k_pauli_chain's site step:
//                  T = E [A_0 | A_1], E' = sum_t c_t A_sigma(t)^H T_t, on the FP64 matrix cores.  The closed
//                  sum's job adds its items (the old sum with P = 1, then the terms that close at this
//                  site, times c_t, in input order) into one output: each element has one owner thread,
//                  which adds in item order.  No atomics.
//   k_heff_stage1  W_r = L_r (G_r x), per (record, s1' s2' block, 64 x 64 tile): the record's 4 x 4 matrix G
//                  (a Pauli pair times c_t, the dense local matrix h_b, or 1) mixes the four (s1, s2)
//                  blocks of x as the GEMM's operand is read.
//   k_heff_stage2  y = sum_r W_r R_r, per (block, tile): the records in record order, one owner an element.
//   k_lz_*         a Lanczos iteration of fixed Krylov dimension on theta, with every scalar on the device:
//                  init (v_0 = theta / |theta|), step (two modified Gram-Schmidt passes against the whole
//                  stored basis, alpha, beta, the breakdown test), solve (one wave: cyclic Jacobi on the
//                  k x k tridiagonal), combine (the lowest Ritz vector, normalised, over theta).  On
//                  breakdown -- beta_j <= kBreakdown eps S, or j + 1 = 4 chi_l chi_r -- a device flag turns
//                  the remaining launches into no-ops.  Every sum runs in a fixed order.
//
// The sweep is a list of kind-6 device ops handed to run_waves (mps.hip), which calls launch_heff between
// k_theta and the wave's SVD and launch_dmrg_env behind the split: the engine's SVD, truncation,
// renormalisation and split serve the update unchanged, and nothing waits on the host between bonds (up
// to 2 chi = 128; the larger SVD classes synchronise once per update themselves).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "aqc_gemm.h"
#include "mps_internal.h"

using aqc::cplx;

namespace {

constexpr int kGemmT = aqc::kGemmThreads;
constexpr int kLzT = 1024;            // the vector kernels: one workgroup
constexpr int kMaxKrylov = 16;
constexpr int kMaxRecords = 4096;     // records of one bond
constexpr long long kMaxBytes = 8ll << 30;  // environments and scratch of one handle
constexpr double kBreakdown = 256.0;  // Lanczos breakdown: beta <= kBreakdown eps S
constexpr double kEps = 2.220446049250313e-16;

// ---- the bond plan (host only) -----------------------------------------------------------------
struct Term {
  int lo, hi;  // support; lo = -1: the identity
  double c;
};

struct Rec {
  int kind;   // 0: LH, 1: RH, 2: the local 4 x 4 matrix, 3: an open term
  int term;   // kind 3: the term, else -1
  int flags;  // bit 0: a stored left environment, bit 1: a stored right one
};

struct Plan {
  int n = 0;
  std::vector<Term> terms;
  std::vector<std::vector<int>> cross;  // [p], p = 0 .. n: the terms with lo < p <= hi, input order
  std::vector<std::vector<Rec>> recs;   // [b], b = 0 .. n - 2
  std::vector<int> closed_l, closed_r, local;  // per bond: the numbers of terms
  double shift = 0.0, scale = 0.0;
  int identities = 0, max_recs = 0, max_cross = 0;
  long long total_recs = 0, env_mats = 0;

  int slot(int p, int t) const {  // of crossing term t at cut p
    const std::vector<int>& v = cross[p];
    return 1 + (int)(std::lower_bound(v.begin(), v.end(), t) - v.begin());
  }
  // 0 closed left, 1 closed right, 2 local, 3 open, 4 identity
  int cls(int b, int t) const {
    const Term& T = terms[t];
    if (T.lo < 0) return 4;
    if (T.hi < b) return 0;
    if (T.lo > b + 1) return 1;
    if (b <= T.lo && T.hi <= b + 1) return 2;
    return 3;
  }
};

int build_plan(int n, const uint8_t* codes, const double* coeffs, int nterms, Plan& P, const char* who) {
  P.n = n;
  P.terms.resize(nterms);
  P.cross.assign(n + 1, {});
  for (int t = 0; t < nterms; ++t) {
    int lo = -1, hi = -1;
    for (int q = 0; q < n; ++q) {
      const uint8_t c = codes[(size_t)t * n + q];
      if (c > 3) {
        aqc::set_error(std::string(who) + ": codes must be 0 (I), 1 (X), 2 (Y) or 3 (Z)");
        return AQC_ERR_ARG;
      }
      if (c) {
        if (lo < 0) lo = q;
        hi = q;
      }
    }
    if (!std::isfinite(coeffs[t])) {
      aqc::set_error(std::string(who) + ": a coefficient is not finite");
      return AQC_ERR_ARG;
    }
    P.terms[t] = {lo, hi, coeffs[t]};
    P.scale += std::fabs(coeffs[t]);
    if (lo < 0) {
      P.shift += coeffs[t];
      ++P.identities;
    }
    for (int p = lo + 1; lo >= 0 && p <= hi; ++p) P.cross[p].push_back(t);
  }
  P.recs.assign(n - 1, {});
  P.closed_l.assign(n - 1, 0);
  P.closed_r.assign(n - 1, 0);
  P.local.assign(n - 1, 0);
  for (int b = 0; b + 1 < n; ++b) {
    std::vector<Rec> open;
    for (int t = 0; t < nterms; ++t) {
      const int c = P.cls(b, t);
      if (c == 0) ++P.closed_l[b];
      else if (c == 1) ++P.closed_r[b];
      else if (c == 2) ++P.local[b];
      else if (c == 3) open.push_back({3, t, (P.terms[t].lo < b ? 1 : 0) | (P.terms[t].hi > b + 1 ? 2 : 0)});
    }
    std::vector<Rec>& r = P.recs[b];
    if (P.closed_l[b]) r.push_back({0, -1, 1});
    if (P.closed_r[b]) r.push_back({1, -1, 2});
    if (P.local[b]) r.push_back({2, -1, 0});
    r.insert(r.end(), open.begin(), open.end());
    P.max_recs = std::max(P.max_recs, (int)r.size());
    P.total_recs += (long long)r.size();
  }
  for (int p = 1; p < n; ++p) {
    P.env_mats += 2 * (1 + (long long)P.cross[p].size());
    P.max_cross = std::max(P.max_cross, (int)P.cross[p].size());
  }
  return AQC_OK;
}

long long env_bytes(const Plan& P, int cap) { return P.env_mats * (long long)cap * cap * (long long)sizeof(cplx); }
// W of every record, the Krylov basis, the environment steps' T panels
long long scratch_bytes(const Plan& P, int cap, int kdim) {
  const long long cc = (long long)cap * cap * (long long)sizeof(cplx), ncb = (cap + 63) / 64;
  return (long long)std::max(P.max_recs, 1) * 4 * cc + (long long)(kdim + 1) * 4 * cc +
         (long long)(1 + P.max_cross) * ncb * cap * 128 * (long long)sizeof(cplx);
}

int check_limits(const Plan& P, int cap, int kdim, const char* who) {
  for (int b = 0; b + 1 < P.n; ++b)
    if ((int)P.recs[b].size() > kMaxRecords) {
      aqc::set_error(std::string(who) + ": bond " + std::to_string(b) + " has " + std::to_string(P.recs[b].size()) +
                     " records, above the limit of " + std::to_string(kMaxRecords));
      return AQC_ERR_ARG;
    }
  const long long need = env_bytes(P, cap) + scratch_bytes(P, cap, kdim);
  if (need > kMaxBytes) {
    aqc::set_error(std::string(who) + ": environments and scratch need " + std::to_string(need) + " bytes at capacity " +
                   std::to_string(cap) + ", above the budget of " + std::to_string(kMaxBytes));
    return AQC_ERR_ARG;
  }
  return AQC_OK;
}

// ---- device tables -----------------------------------------------------------------------------
struct EnvItem {
  const cplx* src;  // the environment the step starts from; null: the identity
  int pauli, pad;
  double coef;
};

struct EnvJob {
  cplx* out;
  int first, count;  // its items
};

struct HeffRec {
  const cplx* L;   // [bra][ket], null: the identity
  const cplx* Rt;  // [ket][bra], null: the identity
  cplx G[16];      // row 2 s1' + s2' (out), column 2 s1 + s2 (in); c_t folded in
};

struct LzState {
  double alpha[kMaxKrylov], beta[kMaxKrylov + 1], s[kMaxKrylov];
  double ritz;
  int m, done, brk, pad;
};

struct EnvArgs {
  const EnvJob* jobs;
  const EnvItem* items;
  const cplx* gam;    // the site's Gamma
  const double* lam;  // left step: lambda left of the site; right step: lambda right of it
  const int* dims;    // &dims[site]
  cplx* ws;           // per workgroup cap x 128: the T panel
  int cap, right;
};

struct HeffArgs {
  const HeffRec* recs;
  const int* dims;  // &dims[b]: chi_l, chi_m, chi_r
  const cplx* x;
  cplx* y;
  cplx* W;  // per record 4 cap^2, theta's layout
  const LzState* st;
  int nrec, cap;
};

struct LzArgs {
  cplx* V;  // kdim + 1 vectors of 4 cap^2
  cplx* theta;
  const int* dims;
  LzState* st;
  double* energies;
  long long* counters;  // [0] breakdowns, [1] bonds solved
  size_t vstride;
  double thresh;
  int kdim, slot;
};

// P[sigma(t)][t] = c_t:  I (t, 1, 1)  X (1 - t, 1, 1)  Y (1 - t, i, -i)  Z (t, 1, -1)
__host__ __device__ inline void pauli_cols(int p, bool& flip, cplx& c0, cplx& c1) {
  flip = p == 1 || p == 2;
  c0 = p == 2 ? aqc::cmk(0, 1) : aqc::cmk(1, 0);
  c1 = p == 2 ? aqc::cmk(0, -1) : p == 3 ? aqc::cmk(-1, 0) : aqc::cmk(1, 0);
}

// Left step through site i (A_t = lambda_i Gamma_t, output chi_r x chi_r [bra][ket]):
//   T[b][t][k'] = sum_k E[b][k] A_t[k][k'],  E'[b'][k'] = sum_{t, b} c_t conj(A_sigma(t)[b][b']) T[b][t][k'].
// Right step (B_t = Gamma_t lambda_{i+1}, output chi_l x chi_l [ket][bra]):
//   T[k'][s][b] = sum_b' R[k'][b'] conj(B_s[b][b']),  R'[k][b] = sum_{t, k'} c_t B_t[k][k'] T[k'][sigma(t)][b].
// blockIdx.x = job * ncb + (64-column block of the output)
__global__ __launch_bounds__(kGemmT) void k_dmrg_env(const EnvArgs a) {
  __shared__ aqc::GemmLds lds;
  const int cap = a.cap, ncb = (cap + 63) / 64;
  const int job = blockIdx.x / ncb, c0 = (blockIdx.x % ncb) * 64;
  const EnvJob J = a.jobs[job];
  const int cl = a.dims[0], cr = a.dims[1];
  const int dout = a.right ? cl : cr, din = a.right ? cr : cl;
  if (c0 >= dout) return;
  const int bw = min(64, dout - c0);
  const bool right = a.right != 0;
  const size_t cc = (size_t)cap * cap;
  const cplx* g = a.gam;
  const double* lam = a.lam;
  cplx* T = a.ws + (size_t)blockIdx.x * cap * 128;
  if (J.count == 0) {
    for (int e = threadIdx.x; e < dout * bw; e += kGemmT) J.out[(size_t)(e / bw) * cap + c0 + e % bw] = aqc::cmk(0, 0);
    return;
  }
  for (int it = 0; it < J.count; ++it) {
    const EnvItem I = a.items[J.first + it];
    const cplx* src = I.src;
    bool flip;
    cplx c[2];
    pauli_cols(I.pauli, flip, c[0], c[1]);
    c[0] = aqc::cscale(c[0], I.coef);
    c[1] = aqc::cscale(c[1], I.coef);
    aqc::block_cgemm<true, false, false>(
        din, 2 * bw, din,
        [&](int r, int k) { return src ? aqc::ldg(src + (size_t)r * cap + k) : aqc::cmk(r == k ? 1.0 : 0.0, 0.0); },
        [&](int k, int col) {
          const int t = col >= bw ? 1 : 0, o = c0 + col - t * bw;
          if (!right) return aqc::cscale(aqc::ldg(g + t * cc + (size_t)k * cap + o), aqc::ldg(lam + k));
          return aqc::cconj(aqc::cscale(aqc::ldg(g + t * cc + (size_t)o * cap + k), aqc::ldg(lam + k)));
        },
        [&](int r, int col, cplx v) { T[(size_t)r * 128 + col] = v; }, lds);
    __syncthreads();
    const bool first = it == 0;
    aqc::block_cgemm<false, false, false>(
        dout, bw, 2 * din,
        [&](int r, int kk) {
          const int t = kk >= din ? 1 : 0, q = kk - t * din;
          if (!right) {
            const int s = flip ? 1 - t : t;
            return aqc::cmul(c[t], aqc::cconj(aqc::cscale(aqc::ldg(g + s * cc + (size_t)q * cap + r), aqc::ldg(lam + q))));
          }
          return aqc::cmul(c[t], aqc::cscale(aqc::ldg(g + t * cc + (size_t)r * cap + q), aqc::ldg(lam + q)));
        },
        [&](int kk, int col) {
          const int t = kk >= din ? 1 : 0, q = kk - t * din;
          const int blk = right ? (flip ? 1 - t : t) : t;
          return T[(size_t)q * 128 + blk * bw + col];
        },
        [&](int r, int col, cplx v) {
          cplx* o = J.out + (size_t)r * cap + c0 + col;
          *o = first ? v : aqc::cadd(*o, v);
        },
        lds);
    __syncthreads();
  }
}

// theta's layout: block o = 2 s1 + s2, element (l, r)
__device__ __forceinline__ size_t th_idx(int o, int l, int r, int chl, int chr) {
  return (size_t)((o & 1) * chr + r) * (2 * chl) + (size_t)(o >> 1) * chl + l;
}

// blockIdx.x = (rec * 4 + o) * tiles + tile
__global__ __launch_bounds__(kGemmT) void k_heff_stage1(const HeffArgs a) {
  __shared__ aqc::GemmLds lds;
  if (a.st->done) return;
  const int cap = a.cap, tl = (cap + 63) / 64, tiles = tl * tl;
  const int rec = blockIdx.x / (4 * tiles), o = (blockIdx.x / tiles) & 3, tile = blockIdx.x % tiles;
  const int chl = a.dims[0], chr = a.dims[2];
  const int bi = (tile / tl) * 64, bj = (tile % tl) * 64;
  if (bi >= chl || bj >= chr) return;
  const int mt = min(64, chl - bi), nt = min(64, chr - bj);
  const HeffRec& R = a.recs[rec];
  cplx G[4];
  bool nz[4];
#pragma unroll
  for (int in = 0; in < 4; ++in) {
    G[in] = R.G[o * 4 + in];
    nz[in] = G[in].x != 0.0 || G[in].y != 0.0;
  }
  const cplx* x = a.x;
  auto mix = [&](int l, int r) {
    cplx v = aqc::cmk(0, 0);
#pragma unroll
    for (int in = 0; in < 4; ++in)
      if (nz[in]) v = aqc::cfma(G[in], aqc::ldg(x + th_idx(in, l, r, chl, chr)), v);
    return v;
  };
  cplx* W = a.W + (size_t)rec * 4 * cap * cap;
  const cplx* L = R.L;
  if (!L) {
    for (int e = threadIdx.x; e < mt * nt; e += kGemmT) {
      const int l = bi + e % mt, r = bj + e / mt;
      W[th_idx(o, l, r, chl, chr)] = mix(l, r);
    }
    return;
  }
  aqc::block_cgemm<true, false, false>(
      mt, nt, chl, [&](int r, int k) { return aqc::ldg(L + (size_t)(bi + r) * cap + k); },
      [&](int k, int col) { return mix(k, bj + col); },
      [&](int r, int col, cplx v) { W[th_idx(o, bi + r, bj + col, chl, chr)] = v; }, lds);
}

// blockIdx.x = o * tiles + tile
__global__ __launch_bounds__(kGemmT) void k_heff_stage2(const HeffArgs a) {
  __shared__ aqc::GemmLds lds;
  if (a.st->done) return;
  const int cap = a.cap, tl = (cap + 63) / 64, tiles = tl * tl;
  const int o = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int chl = a.dims[0], chr = a.dims[2];
  const int bi = (tile / tl) * 64, bj = (tile % tl) * 64;
  if (bi >= chl || bj >= chr) return;
  const int mt = min(64, chl - bi), nt = min(64, chr - bj);
  cplx* y = a.y;
  if (a.nrec == 0)
    for (int e = threadIdx.x; e < mt * nt; e += kGemmT) y[th_idx(o, bi + e % mt, bj + e / mt, chl, chr)] = aqc::cmk(0, 0);
  for (int rec = 0; rec < a.nrec; ++rec) {
    const cplx* W = a.W + (size_t)rec * 4 * cap * cap;
    const cplx* Rt = a.recs[rec].Rt;
    const bool first = rec == 0;
    if (!Rt) {
      for (int e = threadIdx.x; e < mt * nt; e += kGemmT) {
        const size_t i = th_idx(o, bi + e % mt, bj + e / mt, chl, chr);
        y[i] = first ? W[i] : aqc::cadd(y[i], W[i]);
      }
    } else {
      aqc::block_cgemm<false, false, false>(
          mt, nt, chr, [&](int r, int k) { return W[th_idx(o, bi + r, k, chl, chr)]; },
          [&](int k, int col) { return aqc::ldg(Rt + (size_t)k * cap + bj + col); },
          [&](int r, int col, cplx v) {
            const size_t i = th_idx(o, bi + r, bj + col, chl, chr);
            y[i] = first ? v : aqc::cadd(y[i], v);
          },
          lds);
    }
    __syncthreads();  // the next record's owner of an element may be another thread
  }
}

// ---- Lanczos on theta: one workgroup of 1024 threads, every sum in a fixed order --------------------
// lane tree, then the 16 waves in order; the result in every thread
__device__ __forceinline__ double block_sum1024(double v, double* red) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < kLzT / 64; ++w) s += red[w];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(kLzT) void k_lz_init(const LzArgs a) {
  __shared__ double red[kLzT / 64];
  const int dim = 4 * a.dims[0] * a.dims[2];
  double acc = 0.0;
  for (int e = threadIdx.x; e < dim; e += kLzT) acc += aqc::cnorm2(a.theta[e]);
  const double nrm = sqrt(block_sum1024(acc, red));
  const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;
  for (int e = threadIdx.x; e < dim; e += kLzT) a.V[e] = aqc::cscale(a.theta[e], inv);
  if (threadIdx.x == 0) {
    a.st->m = 0;
    a.st->done = 0;
    a.st->brk = 0;
  }
}

// step j: w = V[j + 1] holds H v_j
__global__ __launch_bounds__(kLzT) void k_lz_step(const LzArgs a, int j) {
  __shared__ double red[kLzT / 64];
  const int done = a.st->done;
  __syncthreads();
  if (done) return;
  const int dim = 4 * a.dims[0] * a.dims[2];
  cplx* w = a.V + (size_t)(j + 1) * a.vstride;
  double alpha = 0.0;
  for (int pass = 0; pass < 2; ++pass)
    for (int i = j; i >= 0; --i) {
      const cplx* v = a.V + (size_t)i * a.vstride;
      double hr = 0.0, hi = 0.0;
      for (int e = threadIdx.x; e < dim; e += kLzT) {
        const cplx p = aqc::cconjmul(v[e], w[e]);
        hr += p.x;
        hi += p.y;
      }
      hr = block_sum1024(hr, red);
      hi = block_sum1024(hi, red);
      const cplx h = aqc::cmk(-hr, -hi);
      for (int e = threadIdx.x; e < dim; e += kLzT) w[e] = aqc::cfma(h, v[e], w[e]);  // (a thread's own elements)
      if (i == j) alpha += hr;
    }
  double acc = 0.0;
  for (int e = threadIdx.x; e < dim; e += kLzT) acc += aqc::cnorm2(w[e]);
  const double beta = sqrt(block_sum1024(acc, red));
  const bool brk = !(beta > a.thresh) || j + 1 >= dim;
  const bool last = brk || j + 1 == a.kdim;
  if (threadIdx.x == 0) {
    a.st->alpha[j] = alpha;
    a.st->beta[j + 1] = beta;
    a.st->m = j + 1;
    if (last) a.st->done = 1;
    if (brk) a.st->brk = 1;
  }
  if (!last) {
    const double inv = 1.0 / beta;
    for (int e = threadIdx.x; e < dim; e += kLzT) w[e] = aqc::cscale(w[e], inv);
  }
}

// One wave: the m x m tridiagonal (alpha, beta) by cyclic Jacobi, A' = J^T A J with lane i owning row and
// column entry i of each rotation; the lowest eigenpair to st->ritz, st->s.
__global__ __launch_bounds__(64) void k_lz_solve(const LzArgs a) {
  __shared__ double A[kMaxKrylov][kMaxKrylov + 1], Z[kMaxKrylov][kMaxKrylov + 1];
  LzState* st = a.st;
  const int m = st->m, i = threadIdx.x;
  if (i < kMaxKrylov)
    for (int c = 0; c < kMaxKrylov; ++c) {
      A[i][c] = 0.0;
      Z[i][c] = i == c ? 1.0 : 0.0;
    }
  __syncthreads();
  if (i < m) {
    A[i][i] = st->alpha[i];
    if (i + 1 < m) A[i][i + 1] = A[i + 1][i] = st->beta[i + 1];
  }
  __syncthreads();
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0, dia = 0.0;
    for (int p = 0; p < m; ++p)
      for (int q = 0; q < m; ++q) (p == q ? dia : off) += A[p][q] * A[p][q];
    if (!(off > 1e-32 * dia)) break;  // (every lane reads the same values)
    for (int p = 0; p + 1 < m; ++p)
      for (int q = p + 1; q < m; ++q) {
        const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
        __syncthreads();
        if (fabs(apq) <= 1e-300) continue;
        const double tau = (aqq - app) / (2.0 * apq);
        const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
        if (i < m) {
          const double x = A[i][p], y = A[i][q];
          A[i][p] = c * x - s * y;
          A[i][q] = s * x + c * y;
          const double u = Z[i][p], v = Z[i][q];
          Z[i][p] = c * u - s * v;
          Z[i][q] = s * u + c * v;
        }
        __syncthreads();
        if (i < m) {
          const double x = A[p][i], y = A[q][i];
          A[p][i] = c * x - s * y;
          A[q][i] = s * x + c * y;
        }
        __syncthreads();
      }
  }
  if (i == 0) {
    int best = 0;
    for (int k = 1; k < m; ++k)
      if (A[k][k] < A[best][best]) best = k;
    double nn = 0.0;
    for (int k = 0; k < m; ++k) nn += Z[k][best] * Z[k][best];
    const double inv = 1.0 / sqrt(nn);
    for (int k = 0; k < m; ++k) st->s[k] = Z[k][best] * inv;
    st->ritz = A[best][best];
    a.energies[a.slot] = A[best][best];
    a.counters[0] += st->brk;
    a.counters[1] += 1;
  }
}

__global__ __launch_bounds__(kLzT) void k_lz_combine(const LzArgs a) {
  __shared__ double red[kLzT / 64];
  const int dim = 4 * a.dims[0] * a.dims[2], m = a.st->m;
  double acc = 0.0;
  for (int e = threadIdx.x; e < dim; e += kLzT) {
    cplx v = aqc::cmk(0, 0);
    for (int k = 0; k < m; ++k) v = aqc::cadd(v, aqc::cscale(a.V[(size_t)k * a.vstride + e], a.st->s[k]));
    a.theta[e] = v;
    acc += aqc::cnorm2(v);
  }
  const double nrm = sqrt(block_sum1024(acc, red));
  const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;
  for (int e = threadIdx.x; e < dim; e += kLzT) a.theta[e] = aqc::cscale(a.theta[e], inv);
}

size_t al256(size_t b) { return aqc::up256(b); }

}  // namespace

struct aqc_dmrg_s {
  aqc_mps_s* mps = nullptr;
  unsigned long long uid = 0, version = 0;
  int n = 0, cap = 0, kdim = 0;
  Plan plan;
  std::vector<uint8_t> codes;
  char* block = nullptr;
  cplx *envL = nullptr, *envR = nullptr, *W = nullptr, *V = nullptr, *ws = nullptr;
  LzState* st = nullptr;
  double* energies = nullptr;
  long long* counters = nullptr;
  HeffRec* recs = nullptr;
  EnvJob* jobs = nullptr;
  EnvItem* items = nullptr;
  std::vector<long long> lmat, rmat;       // first matrix of cut p on each side
  std::vector<int> rec0;                    // first record of bond b
  std::vector<std::pair<int, int>> lstep, rstep;  // per site: (first job, jobs) of the step through it
  bool gauged = false, right_ready = false;

  cplx* L(int p, int slot) const { return envL + (size_t)(lmat[p] + slot) * cap * cap; }
  cplx* R(int p, int slot) const { return envR + (size_t)(rmat[p] + slot) * cap * cap; }
};

namespace {

// G[2 s1' + s2'][2 s1 + s2] += c P1[s1'][s1] P2[s2'][s2]
void add_pair(cplx* G, int p1, int p2, double c) {
  bool f1, f2;
  cplx a[2], b[2];
  pauli_cols(p1, f1, a[0], a[1]);
  pauli_cols(p2, f2, b[0], b[1]);
  for (int t1 = 0; t1 < 2; ++t1)
    for (int t2 = 0; t2 < 2; ++t2) {
      const int s1 = f1 ? 1 - t1 : t1, s2 = f2 ? 1 - t2 : t2;
      cplx& g = G[(2 * s1 + s2) * 4 + 2 * t1 + t2];
      g = aqc::cadd(g, aqc::cscale(aqc::hmul(a[t1], b[t2]), c));
    }
}

int build_tables(aqc_dmrg_s* d) {
  const Plan& P = d->plan;
  const int n = d->n, cap = d->cap;
  const uint8_t* codes = d->codes.data();
  const size_t cc = (size_t)cap * cap * sizeof(cplx);
  d->lmat.assign(n + 1, 0);
  d->rmat.assign(n + 1, 0);
  long long m = 0;
  for (int p = 1; p < n; ++p) {
    d->lmat[p] = d->rmat[p] = m;
    m += 1 + (long long)P.cross[p].size();
  }
  // the carve
  const size_t ncb = (cap + 63) / 64;
  const size_t b_env = al256((size_t)m * cc), b_W = al256((size_t)std::max(P.max_recs, 1) * 4 * cc);
  const size_t b_V = al256((size_t)(d->kdim + 1) * 4 * cc);
  const size_t b_ws = al256((size_t)(1 + P.max_cross) * ncb * cap * 128 * sizeof(cplx));
  const size_t b_st = al256(sizeof(LzState)), b_en = al256((size_t)2 * (n - 1) * sizeof(double)), b_ct = 256;
  std::vector<HeffRec> recs;
  std::vector<EnvJob> jobs;
  std::vector<EnvItem> items;
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    const size_t o = off;
    off += bytes;
    return o;
  };
  const size_t o_L = carve(b_env), o_R = carve(b_env), o_W = carve(b_W), o_V = carve(b_V), o_ws = carve(b_ws);
  const size_t o_st = carve(b_st), o_en = carve(b_en), o_ct = carve(b_ct);
  // (pointers into the block are needed to fill the tables: size them first)
  size_t nrec = 0, njob = 0, nitem = 0;
  for (int b = 0; b + 1 < n; ++b) nrec += P.recs[b].size();
  for (int p = 1; p < n; ++p) njob += 2 * (1 + P.cross[p].size());
  nitem = 2 * ((size_t)P.terms.size() + (size_t)n) + njob;
  const size_t o_rec = carve(al256(std::max<size_t>(nrec, 1) * sizeof(HeffRec)));
  const size_t o_job = carve(al256(std::max<size_t>(njob, 1) * sizeof(EnvJob)));
  const size_t o_item = carve(al256(nitem * sizeof(EnvItem)));
  d->block = (char*)aqc::dev_alloc(off);
  if (!d->block) {
    aqc::set_error("aqc_dmrg_create: out of device memory");
    return AQC_ERR_NOMEM;
  }
  d->envL = (cplx*)(d->block + o_L);
  d->envR = (cplx*)(d->block + o_R);
  d->W = (cplx*)(d->block + o_W);
  d->V = (cplx*)(d->block + o_V);
  d->ws = (cplx*)(d->block + o_ws);
  d->st = (LzState*)(d->block + o_st);
  d->energies = (double*)(d->block + o_en);
  d->counters = (long long*)(d->block + o_ct);
  d->recs = (HeffRec*)(d->block + o_rec);
  d->jobs = (EnvJob*)(d->block + o_job);
  d->items = (EnvItem*)(d->block + o_item);
  // H_eff records
  d->rec0.assign(n, 0);
  for (int b = 0; b + 1 < n; ++b) {
    d->rec0[b] = (int)recs.size();
    for (const Rec& r : P.recs[b]) {
      HeffRec h;
      std::memset(&h, 0, sizeof(h));
      if (r.kind == 0) {
        h.L = d->L(b, 0);
        add_pair(h.G, 0, 0, 1.0);
      } else if (r.kind == 1) {
        h.Rt = d->R(b + 2, 0);
        add_pair(h.G, 0, 0, 1.0);
      } else if (r.kind == 2) {
        for (size_t t = 0; t < P.terms.size(); ++t)
          if (P.cls(b, (int)t) == 2) add_pair(h.G, codes[t * n + b], codes[t * n + b + 1], P.terms[t].c);
      } else {
        const int t = r.term;
        if (r.flags & 1) h.L = d->L(b, P.slot(b, t));
        if (r.flags & 2) h.Rt = d->R(b + 2, P.slot(b + 2, t));
        add_pair(h.G, codes[(size_t)t * n + b], codes[(size_t)t * n + b + 1], P.terms[t].c);
      }
      recs.push_back(h);
    }
  }
  d->rec0[n - 1] = (int)recs.size();
  // terms that end / start at a site, input order
  std::vector<std::vector<int>> ends(n), starts(n);
  for (size_t t = 0; t < P.terms.size(); ++t)
    if (P.terms[t].lo >= 0) {
      ends[P.terms[t].hi].push_back((int)t);
      starts[P.terms[t].lo].push_back((int)t);
    }
  d->lstep.assign(n, {0, 0});
  d->rstep.assign(n, {0, 0});
  // left steps: cut p -> cut p + 1 through site p
  for (int p = 0; p + 1 < n; ++p) {
    const int j0 = (int)jobs.size();
    auto src = [&](int t) -> const cplx* { return P.terms[t].lo < p ? d->L(p, P.slot(p, t)) : nullptr; };
    EnvJob J{d->L(p + 1, 0), (int)items.size(), 0};
    if (p >= 1) items.push_back({d->L(p, 0), 0, 0, 1.0});
    for (int t : ends[p]) items.push_back({src(t), codes[(size_t)t * n + p], 0, P.terms[t].c});
    J.count = (int)items.size() - J.first;
    jobs.push_back(J);
    for (size_t k = 0; k < P.cross[p + 1].size(); ++k) {
      const int t = P.cross[p + 1][k];
      jobs.push_back({d->L(p + 1, 1 + (int)k), (int)items.size(), 1});
      items.push_back({src(t), codes[(size_t)t * n + p], 0, 1.0});
    }
    d->lstep[p] = {j0, (int)jobs.size() - j0};
  }
  // right steps: cut p + 1 -> cut p through site p
  for (int p = n - 1; p >= 1; --p) {
    const int j0 = (int)jobs.size();
    auto src = [&](int t) -> const cplx* { return P.terms[t].hi > p ? d->R(p + 1, P.slot(p + 1, t)) : nullptr; };
    EnvJob J{d->R(p, 0), (int)items.size(), 0};
    if (p + 1 <= n - 1) items.push_back({d->R(p + 1, 0), 0, 0, 1.0});
    for (int t : starts[p]) items.push_back({src(t), codes[(size_t)t * n + p], 0, P.terms[t].c});
    J.count = (int)items.size() - J.first;
    jobs.push_back(J);
    for (size_t k = 0; k < P.cross[p].size(); ++k) {
      const int t = P.cross[p][k];
      jobs.push_back({d->R(p, 1 + (int)k), (int)items.size(), 1});
      items.push_back({src(t), codes[(size_t)t * n + p], 0, 1.0});
    }
    d->rstep[p] = {j0, (int)jobs.size() - j0};
  }
  if (recs.size() > nrec || jobs.size() > njob || items.size() > nitem) {
    aqc::set_error("aqc_dmrg_create: internal table sizes");
    return AQC_ERR_STATE;
  }
  hipStream_t st = aqc::mps_stream();
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  if (!recs.empty()) AQC_HIP_CHECK(hipMemcpy(d->recs, recs.data(), recs.size() * sizeof(HeffRec), hipMemcpyHostToDevice));
  if (!jobs.empty()) AQC_HIP_CHECK(hipMemcpy(d->jobs, jobs.data(), jobs.size() * sizeof(EnvJob), hipMemcpyHostToDevice));
  if (!items.empty()) AQC_HIP_CHECK(hipMemcpy(d->items, items.data(), items.size() * sizeof(EnvItem), hipMemcpyHostToDevice));
  AQC_HIP_CHECK(hipMemset(d->st, 0, sizeof(LzState)));
  AQC_HIP_CHECK(hipMemset(d->energies, 0, (size_t)2 * (n - 1) * sizeof(double)));
  AQC_HIP_CHECK(hipMemset(d->counters, 0, 256));
  return AQC_OK;
}

// the step of every environment through `site`: left (cut site -> site + 1) or right (site + 1 -> site)
int launch_env(aqc_dmrg_s* d, bool right, int site, hipStream_t st) {
  const std::pair<int, int> s = right ? d->rstep[site] : d->lstep[site];
  if (s.second == 0) return AQC_OK;
  const aqc::MpsDev& m = d->mps->d;
  EnvArgs a;
  std::memset(&a, 0, sizeof(a));
  a.jobs = d->jobs + s.first;
  a.items = d->items;
  a.gam = m.site(site);
  a.lam = right ? m.bond(site + 1) : m.bond(site);
  a.dims = m.dims + site;
  a.ws = d->ws;
  a.cap = d->cap;
  a.right = right ? 1 : 0;
  const int ncb = (d->cap + 63) / 64;
  const std::vector<int>& ub = d->mps->ub;
  const double cl = ub[site], cr = ub[site + 1], din = right ? cr : cl, dout = right ? cl : cr;
  // per item T = E [A_0 | A_1] and E' = sum_t A^H T_t: 8 flops a complex multiply-add
  const double flops = (double)s.second * 8.0 * (2.0 * din * din * dout + 2.0 * din * dout * dout);
  aqc::KernelTimer::begin(st, "dmrg_env", (double)s.second * 16.0 * (din * din + dout * dout + 2.0 * cl * cr), flops);
  hipLaunchKernelGGL(k_dmrg_env, dim3(s.second * ncb), dim3(kGemmT), 0, st, a);
  aqc::KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  return AQC_OK;
}

int launch_apply(aqc_dmrg_s* d, int bond, const cplx* x, cplx* y, hipStream_t st) {
  HeffArgs a;
  std::memset(&a, 0, sizeof(a));
  a.recs = d->recs + d->rec0[bond];
  a.nrec = d->rec0[bond + 1] - d->rec0[bond];
  a.dims = d->mps->d.dims + bond;
  a.x = x;
  a.y = y;
  a.W = d->W;
  a.st = d->st;
  a.cap = d->cap;
  const int tl = (d->cap + 63) / 64, tiles = tl * tl;
  const std::vector<int>& ub = d->mps->ub;
  const double cl = ub[bond], cr = ub[bond + 2];
  double flops = 0.0;
  for (const Rec& r : d->plan.recs[bond])
    flops += 4.0 * 8.0 * ((r.flags & 1 ? cl * cl * cr : 0.0) + (r.flags & 2 ? cl * cr * cr : 0.0));
  // x once per record, W written and read, the environments, y
  const double bytes = 16.0 * ((double)a.nrec * (12.0 * cl * cr + cl * cl + cr * cr) + 4.0 * cl * cr);
  aqc::KernelTimer::begin(st, "dmrg_heff", bytes, flops);
  if (a.nrec) hipLaunchKernelGGL(k_heff_stage1, dim3(a.nrec * 4 * tiles), dim3(kGemmT), 0, st, a);
  hipLaunchKernelGGL(k_heff_stage2, dim3(4 * tiles), dim3(kGemmT), 0, st, a);
  aqc::KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  return AQC_OK;
}

int check_handle(aqc_dmrg_s* d, const char* who) {
  if (!d || !d->mps) {
    aqc::set_error(std::string(who) + ": null handle");
    return AQC_ERR_ARG;
  }
  if (d->mps->uid != d->uid || d->mps->version != d->version) {
    aqc::set_error(std::string(who) + ": the MPS was changed outside this DMRG handle (create a new one)");
    return AQC_ERR_STATE;
  }
  return AQC_OK;
}

aqc::DevOp identity_update(int kind, int b) {
  aqc::DevOp op = aqc::DevOp();
  op.kind = kind;
  op.p = b;
  for (int e = 0; e < 4; ++e) op.m[e * 4 + e] = aqc::hc(1, 0);
  return op;
}

}  // namespace

// ---- the hooks run_waves calls (mps.hip) ---------------------------------------------------------
int aqc::launch_heff(const DevOp& op, aqc_dmrg_s* d, hipStream_t st) {
  const int b = op.p;
  LzArgs a;
  std::memset(&a, 0, sizeof(a));
  a.V = d->V;
  a.theta = d->mps->d.theta;
  a.dims = d->mps->d.dims + b;
  a.st = d->st;
  a.energies = d->energies;
  a.counters = d->counters;
  a.vstride = (size_t)4 * d->cap * d->cap;
  a.thresh = kBreakdown * kEps * d->plan.scale;
  a.kdim = d->kdim;
  a.slot = op.slot;
  const double dim = 4.0 * d->mps->ub[b] * d->mps->ub[b + 2];
  aqc::KernelTimer::begin(st, "dmrg_krylov", 32.0 * dim, 4.0 * dim);
  hipLaunchKernelGGL(k_lz_init, dim3(1), dim3(kLzT), 0, st, a);
  aqc::KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  for (int j = 0; j < d->kdim; ++j) {
    if (int rc = launch_apply(d, b, a.V + (size_t)j * a.vstride, a.V + (size_t)(j + 1) * a.vstride, st)) return rc;
    // two Gram-Schmidt passes against j + 1 vectors: a dot and an update each
    aqc::KernelTimer::begin(st, "dmrg_krylov", 2.0 * (j + 1) * 80.0 * dim, 2.0 * (j + 1) * 16.0 * dim);
    hipLaunchKernelGGL(k_lz_step, dim3(1), dim3(kLzT), 0, st, a, j);
    aqc::KernelTimer::end(st);
    AQC_CHECK_LAUNCH();
  }
  aqc::KernelTimer::begin(st, "dmrg_krylov", 16.0 * dim * (d->kdim + 2), 4.0 * dim * d->kdim);
  hipLaunchKernelGGL(k_lz_solve, dim3(1), dim3(64), 0, st, a);
  hipLaunchKernelGGL(k_lz_combine, dim3(1), dim3(kLzT), 0, st, a);
  aqc::KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  return AQC_OK;
}

int aqc::launch_dmrg_env(const DevOp& op, aqc_dmrg_s* d, hipStream_t st) {
  // left -> right (grp 0): the left environments of cut p + 1 from the new site p;
  // right -> left: the right environments of cut p + 1 from the new site p + 1
  return op.grp == 0 ? launch_env(d, false, op.p, st) : launch_env(d, true, op.p + 1, st);
}

extern "C" {

int aqc_mps_dmrg_plan(int n, const uint8_t* codes, const double* coeffs, int nterms, int chi_cap, int krylov_dim,
                      int64_t* totals, int* bonds, int* records, int records_cap, uint8_t* classes) {
  AQC_REQUIRE(n >= 2 && n <= 4096, "aqc_mps_dmrg_plan: n must be in 2 .. 4096 (a two-site update needs two sites)");
  AQC_REQUIRE(nterms >= 1 && nterms <= (1 << 20) && codes && coeffs, "aqc_mps_dmrg_plan: nterms outside 1 .. 2^20, or null terms");
  AQC_REQUIRE(chi_cap >= 1 && chi_cap <= aqc::kMaxCap, "aqc_mps_dmrg_plan: chi_cap must be in [1, 1024]");
  AQC_REQUIRE(krylov_dim >= 2 && krylov_dim <= kMaxKrylov, "aqc_mps_dmrg_plan: krylov_dim must be in 2 .. 16");
  AQC_REQUIRE(totals, "aqc_mps_dmrg_plan: null totals");
  Plan P;
  if (int rc = build_plan(n, codes, coeffs, nterms, P, "aqc_mps_dmrg_plan")) return rc;
  if (int rc = check_limits(P, chi_cap, krylov_dim, "aqc_mps_dmrg_plan")) return rc;
  totals[0] = P.total_recs;
  totals[1] = P.max_recs;
  totals[2] = P.env_mats;
  totals[3] = env_bytes(P, chi_cap);
  totals[4] = scratch_bytes(P, chi_cap, krylov_dim);
  totals[5] = kMaxRecords;
  totals[6] = kMaxBytes;
  totals[7] = P.identities;
  if (bonds)
    for (int b = 0; b + 1 < n; ++b) {
      int* o = bonds + 7 * b;
      int open = 0;
      for (const Rec& r : P.recs[b]) open += r.kind == 3;
      o[0] = (int)P.recs[b].size();
      o[1] = P.closed_l[b];
      o[2] = P.closed_r[b];
      o[3] = P.local[b];
      o[4] = open;
      o[5] = b >= 1 ? (int)P.cross[b].size() : 0;          // stored left environments of open terms
      o[6] = b + 2 <= n - 1 ? (int)P.cross[b + 2].size() : 0;  // stored right ones
    }
  if (records) {
    AQC_REQUIRE((long long)records_cap >= P.total_recs, "aqc_mps_dmrg_plan: records_cap below totals[0]");
    size_t k = 0;
    for (int b = 0; b + 1 < n; ++b)
      for (const Rec& r : P.recs[b]) {
        records[4 * k] = b;
        records[4 * k + 1] = r.kind;
        records[4 * k + 2] = r.term;
        records[4 * k + 3] = r.flags;
        ++k;
      }
  }
  if (classes)
    for (int b = 0; b + 1 < n; ++b)
      for (int t = 0; t < nterms; ++t) classes[(size_t)b * nterms + t] = (uint8_t)P.cls(b, t);
  return AQC_OK;
}

int aqc_dmrg_create(aqc_mps_t mps, const uint8_t* codes, const double* coeffs, int nterms, int krylov_dim,
                    aqc_dmrg_t* out) {
  AQC_REQUIRE(mps && out, "aqc_dmrg_create: null handle");
  AQC_REQUIRE(mps->d.n >= 2, "aqc_dmrg_create: a two-site update needs n >= 2");
  AQC_REQUIRE(nterms >= 1 && nterms <= (1 << 20) && codes && coeffs, "aqc_dmrg_create: nterms outside 1 .. 2^20, or null terms");
  AQC_REQUIRE(krylov_dim >= 2 && krylov_dim <= kMaxKrylov, "aqc_dmrg_create: krylov_dim must be in 2 .. 16");
  auto* d = new aqc_dmrg_s();
  d->mps = mps;
  d->n = mps->d.n;
  d->cap = mps->d.cap;
  d->kdim = krylov_dim;
  int rc = build_plan(d->n, codes, coeffs, nterms, d->plan, "aqc_dmrg_create");
  if (rc == AQC_OK) rc = check_limits(d->plan, d->cap, krylov_dim, "aqc_dmrg_create");
  if (rc == AQC_OK) {
    d->codes.assign(codes, codes + (size_t)nterms * d->n);
    rc = build_tables(d);
  }
  if (rc != AQC_OK) {
    aqc::dev_free(d->block);
    delete d;
    return rc;
  }
  d->uid = mps->uid;
  d->version = mps->version;
  *out = d;
  return AQC_OK;
}

int aqc_dmrg_destroy(aqc_dmrg_t d) {
  if (!d) return AQC_OK;
  (void)hipStreamSynchronize(aqc::mps_stream());
  aqc::dev_free(d->block);
  delete d;
  return AQC_OK;
}

// One sweep: bonds 0 .. n - 2 left to right, then back.  out: 2 (n - 1) Ritz values in that order, the
// identity terms' constant added.
int aqc_dmrg_sweep(aqc_dmrg_t d, double* out) {
  if (int rc = check_handle(d, "aqc_dmrg_sweep")) return rc;
  AQC_REQUIRE(out, "aqc_dmrg_sweep: null out");
  aqc_mps_t h = d->mps;
  const int n = d->n;
  if (int rc = aqc_mps_sort(h)) return rc;
  hipStream_t st = aqc::mps_stream();
  std::vector<std::vector<aqc::DevOp>> lists(1);
  if (!d->gauged) {
    // identity updates in both directions: every site left of the centre becomes U, every site right of
    // it V^H of an SVD, whatever gauge the state arrived in
    for (int b = 0; b + 1 < n; ++b) lists[0].push_back(identity_update(2, b));
    for (int b = n - 2; b >= 0; --b) lists[0].push_back(identity_update(2, b));
    if (int rc = aqc::run_waves(&h, 1, lists)) return rc;
    lists[0].clear();
    d->gauged = true;
    d->right_ready = false;
  }
  if (!d->right_ready)
    for (int p = n - 1; p >= 2; --p)
      if (int rc = launch_env(d, true, p, st)) return rc;
  int slot = 0;
  for (int dir = 0; dir < 2; ++dir)
    for (int k = 0; k + 1 < n; ++k) {
      aqc::DevOp op = identity_update(6, dir == 0 ? k : n - 2 - k);
      op.grp = dir;
      op.slot = slot++;
      lists[0].push_back(op);
    }
  int rc = aqc::run_waves(&h, 1, lists, nullptr, d);
  d->version = h->version;
  if (rc != AQC_OK) return rc;
  AQC_HIP_CHECK(hipMemcpyAsync(out, d->energies, (size_t)slot * sizeof(double), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  for (int k = 0; k < slot; ++k) out[k] += d->plan.shift;
  d->right_ready = true;
  return aqc_mps_check_batch(&h, 1);
}

int aqc_dmrg_stats(aqc_dmrg_t d, int64_t* out) {
  AQC_REQUIRE(d && out, "aqc_dmrg_stats: null argument");
  long long c[2];
  hipStream_t st = aqc::mps_stream();
  AQC_HIP_CHECK(hipMemcpyAsync(c, d->counters, sizeof(c), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  out[0] = c[0];
  out[1] = c[1];
  return AQC_OK;
}

int aqc_dmrg_heff_apply(aqc_dmrg_t d, int bond, const double* x, double* y) {
  if (int rc = check_handle(d, "aqc_dmrg_heff_apply")) return rc;
  AQC_REQUIRE(x && y && x != y, "aqc_dmrg_heff_apply: null or aliased vectors");
  AQC_REQUIRE(bond >= 0 && bond + 1 < d->n, "aqc_dmrg_heff_apply: bond outside 0 .. n - 2");
  aqc_mps_t h = d->mps;
  if (int rc = aqc_mps_sort(h)) return rc;
  if (int rc = aqc_mps_check_batch(&h, 1)) return rc;
  if (h->version != d->version) {  // (the sort moved qubits)
    aqc::set_error("aqc_dmrg_heff_apply: the MPS is not in sorted qubit order (sort it before creating the handle)");
    return AQC_ERR_STATE;
  }
  hipStream_t st = aqc::mps_stream();
  int dims[3];
  AQC_HIP_CHECK(hipMemcpyAsync(dims, h->d.dims + bond, sizeof(dims), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  const size_t dim = (size_t)4 * dims[0] * dims[2];
  for (int p = 0; p < bond; ++p)
    if (int rc = launch_env(d, false, p, st)) return rc;
  for (int p = d->n - 1; p >= bond + 2; --p)
    if (int rc = launch_env(d, true, p, st)) return rc;
  d->right_ready = false;
  cplx* vx = d->V;
  cplx* vy = d->V + (size_t)4 * d->cap * d->cap;
  AQC_HIP_CHECK(hipMemsetAsync(d->st, 0, sizeof(LzState), st));
  AQC_HIP_CHECK(hipMemcpyAsync(vx, x, dim * sizeof(cplx), hipMemcpyHostToDevice, st));
  if (int rc = launch_apply(d, bond, vx, vy, st)) return rc;
  AQC_HIP_CHECK(hipMemcpyAsync(y, vy, dim * sizeof(cplx), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  return AQC_OK;
}

}  // extern "C"
