// Pauli-string expectation values <psi| P |psi> on the device, for the statevector and for the MPS.
// Replaces adaptaqc/utils/circuit_operations_pauli_ops.py:60-100 (expectation_value_of_pauli_operator),
// which simulates one rotated copy of the circuit per term: here the state is simulated once and every
// term is contracted against it.
//
// Statevector: P = i^{popcount(x & z)} X^x Z^z (a qubit in both masks is Y), so
//   <P> = i^{ny} sum_k conj(psi[k ^ x]) (-1)^{popcount(k & z)} psi[k].
// k_sv_pauli runs one grid over (blocks, terms): threads grid-stride over k, sum within the wave and
// the block in a fixed order and write one partial per (term, block); k_sv_pauli_sum adds each term's
// partials in index order.  No atomics: the same state gives the same bits.  Per term the state is
// read twice (psi[k] and psi[k ^ x]): 32 * 2^n bytes, from the L2 / MALL for all but the first term
// while the state fits there.
//
// MPS (sorted qubits, A_i^s = Gamma_i^s lambda_{i+1}, no canonical form assumed, <psi|P|psi> not
// divided by <psi|psi>): with the identity environments L_b (bra x ket) and R_b (ket x bra) of
// ent.hip's chains, a term with support lo..hi (first and last non-identity site) is
//   E = L_lo;  for i = lo..hi:  E'[b'][k'] = sum_{s,t} P_i[s][t] conj(A_s[b][b']) E[b][k] A_t[k][k'];
//   <P> = Re sum E[b][k] R_{hi+1}[k][b].
// A Pauli has one non-zero entry per column (s = sigma(t), value c_t), so a site is two GEMMs on the
// FP64 matrix cores (aqc::block_cgemm): T = E [A_0 | A_1] (chi_l x 2 chi_r, contraction chi_l), then
// E' = sum_t c_t A_{sigma(t)}^H T_t (chi_r x chi_r, contraction over the stacked (t, b) of length
// 2 chi_l): 4 chi^3 complex multiply-adds (32 chi^3 flops) a site.  k_pauli_chain gives each
// (term, state) to one 256-thread workgroup, which needs nothing from any other workgroup: no
// counters, no hand-offs, so nothing in it can wait.  E and T (3 cap^2 complex) are the workgroup's slice of a global workspace
// (196 KB at capacity 64: L2-resident); the grid is bounded so that the workspace stays within
// kWsBytes, and a workgroup walks the items wg, wg + grid, ... .  Terms are issued by decreasing
// support so that the long chains start first.  At capacity 1024 a single-workgroup chain of
// 1024 x 2048 x 1024 GEMMs is slow (one CU's matrix cores) but correct.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "aqc_gemm.h"
#include "mps_internal.h"

using aqc::cplx;

namespace {

constexpr int kThreads = 256;
constexpr size_t kWsBytes = (size_t)512 << 20;  // bound of the chain kernel's E / T workspace
constexpr int kMaxWg = 2048;                    // and of its grid (8 workgroups a CU)
constexpr int kMaxTermsPerLaunch = 32768;       // gridDim.y of the statevector kernel

// sum over the block in a fixed order (lane tree, then the four waves in order); the result in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) { return aqc::block_sum256(v, red); }

// ---- statevector -------------------------------------------------------------------------------
// blockIdx.y: term, blockIdx.x: block of the term; partial[term * gridDim.x + blockIdx.x]
__global__ __launch_bounds__(kThreads) void k_sv_pauli(const cplx* __restrict__ state, uint64_t dim,
                                                       const uint64_t* __restrict__ xmask,
                                                       const uint64_t* __restrict__ zmask,
                                                       double* __restrict__ partial) {
  __shared__ double red[4];
  const uint64_t x = xmask[blockIdx.y], z = zmask[blockIdx.y];
  const int ny = __popcll(x & z) & 3;
  double ar = 0.0, ai = 0.0;
  for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < dim; k += (uint64_t)gridDim.x * kThreads) {
    const cplx v = aqc::cconjmul(aqc::ldg(state + (k ^ x)), aqc::ldg(state + k));
    if (__popcll(k & z) & 1) {
      ar -= v.x;
      ai -= v.y;
    } else {
      ar += v.x;
      ai += v.y;
    }
  }
  // Re(i^ny (ar + i ai))
  const double mine = ny == 0 ? ar : ny == 1 ? -ai : ny == 2 ? -ar : ai;
  const double s = block_sum(mine, red);
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

__global__ void k_sv_pauli_sum(const double* __restrict__ partial, int nblk, int nterms, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nterms) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partial[(size_t)t * nblk + b];
  out[t] = s;
}

// ---- MPS ---------------------------------------------------------------------------------------
struct PauliState {
  const cplx* gam;
  const double* lam;
  const int* dims;
  const cplx* Lenv;  // (n+1) cap^2: L_b at b cap^2 [bra][ket], row stride cap (b = 0 .. n-1)
  const cplx* Renv;  // (n+1) cap^2: R_b at b cap^2 [ket][bra], row stride cap (b = 1 .. n)
};

struct PauliJob {
  const PauliState* states;
  const uint8_t* codes;  // nterms x n
  const int* terms;      // per issued term: lo, hi, index of the term in codes / out
  int n, cap, nterms, ns;
  cplx* ws;     // per workgroup 3 cap^2: E (cap x cap), T (cap x 2 cap)
  double* out;  // ns x nterms
};

__global__ __launch_bounds__(kThreads) void k_pauli_chain(const PauliJob j) {
  __shared__ aqc::GemmLds lds;
  __shared__ double red[4];
  const int n = j.n, cap = j.cap;
  const size_t cc = (size_t)cap * cap;
  cplx* E = j.ws + (size_t)blockIdx.x * 3 * cc;
  cplx* T = E + cc;
  const int items = j.nterms * j.ns;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int it = item / j.ns, st = item % j.ns;
    const int lo = j.terms[3 * it], hi = j.terms[3 * it + 1], term = j.terms[3 * it + 2];
    const PauliState& S = j.states[st];
    const uint8_t* code = j.codes + (size_t)term * n;
    const cplx* cur = S.Lenv + (size_t)lo * cc;
    for (int i = lo; i <= hi; ++i) {
      const int cl = S.dims[i], cr = S.dims[i + 1];
      const cplx* g = S.gam + (size_t)i * 2 * cc;
      const double* lam = S.lam + (size_t)(i + 1) * cap;
      // T[b][t cap + k'] = sum_k E[b][k] A_t[k][k']
      aqc::block_cgemm<true, false, true>(
          cl, 2 * cr, cl, [&](int r, int k) { return cur[(size_t)r * cap + k]; },
          [&](int k, int c) {
            const int t = c >= cr ? 1 : 0, rr = c - t * cr;
            return aqc::cscale(aqc::ldg(g + (size_t)t * cc + (size_t)k * cap + rr), aqc::ldg(lam + rr));
          },
          [&](int r, int c, cplx v) { T[(size_t)r * 2 * cap + (c >= cr ? cap + c - cr : c)] = v; }, lds);
      __syncthreads();
      // P[sigma(t)][t] = c_t:  I (t, 1, 1)  X (1 - t, 1, 1)  Y (1 - t, i, -i)  Z (t, 1, -1)
      const int p = code[i];
      const bool flip = p == 1 || p == 2;
      const cplx c0 = p == 2 ? aqc::cmk(0, 1) : aqc::cmk(1, 0);
      const cplx c1 = p == 2 ? aqc::cmk(0, -1) : p == 3 ? aqc::cmk(-1, 0) : aqc::cmk(1, 0);
      // E'[b'][k'] = sum_{(t, b)} c_t conj(A_sigma(t)[b][b']) T[b][t cap + k']
      aqc::block_cgemm<false, false, true>(
          cr, cr, 2 * cl,
          [&](int r, int kk) {
            const int t = kk >= cl ? 1 : 0, b = kk - t * cl, s = flip ? 1 - t : t;
            const cplx a = aqc::cscale(aqc::ldg(g + (size_t)s * cc + (size_t)b * cap + r), aqc::ldg(lam + r));
            return aqc::cmul(t ? c1 : c0, aqc::cconj(a));
          },
          [&](int kk, int c) {
            const int t = kk >= cl ? 1 : 0, b = kk - t * cl;
            return T[(size_t)b * 2 * cap + (size_t)t * cap + c];
          },
          [&](int r, int c, cplx v) { E[(size_t)r * cap + c] = v; }, lds);
      __syncthreads();
      cur = E;
    }
    const int d = S.dims[hi + 1];
    const cplx* R = S.Renv + (size_t)(hi + 1) * cc;
    double acc = 0.0;
    for (int e = threadIdx.x; e < d * d; e += kThreads) {
      const int b = e / d, k = e % d;
      const cplx u = cur[(size_t)b * cap + k], v = aqc::ldg(R + (size_t)k * cap + b);
      acc += fma(u.x, v.x, -u.y * v.y);
    }
    const double s = block_sum(acc, red);  // (its barriers also fence E before the next item's stores)
    if (threadIdx.x == 0) j.out[(size_t)st * j.nterms + term] = s;
  }
}

// per-device grow-only scratch of the statevector path (masks, partials, results)
aqc::PerDevice<aqc::DevScratch> g_scr;
using aqc::up256;

int mps_pauli(aqc_mps_t* hs, int ns, const uint8_t* codes, int nterms, double* out, const char* who) {
  if (!(hs && ns >= 1 && nterms >= 0 && ((codes && out) || nterms == 0))) {
    aqc::set_error(std::string(who) + ": bad arguments");
    return AQC_ERR_ARG;
  }
  for (int s = 0; s < ns; ++s)
    if (!hs[s] || hs[s]->d.n != hs[0]->d.n || hs[s]->d.cap != hs[0]->d.cap) {
      aqc::set_error(std::string(who) + ": all states need the same n and capacity");
      return AQC_ERR_ARG;
    }
  if (nterms == 0) return AQC_OK;
  const int n = hs[0]->d.n, cap = hs[0]->d.cap;
  if ((size_t)nterms * ns > (size_t)1 << 30) {
    aqc::set_error(std::string(who) + ": more than 2^30 (term, state) pairs");
    return AQC_ERR_ARG;
  }
  // supports; the all-identity term runs site 0 with the identity (L_0, one step, R_1)
  std::vector<int> terms(3 * (size_t)nterms);
  {
    std::vector<int> lo(nterms), hi(nterms), order(nterms);
    for (int t = 0; t < nterms; ++t) {
      int a = -1, b = -1;
      for (int q = 0; q < n; ++q) {
        const uint8_t c = codes[(size_t)t * n + q];
        if (c > 3) {
          aqc::set_error(std::string(who) + ": codes must be 0 (I), 1 (X), 2 (Y) or 3 (Z)");
          return AQC_ERR_ARG;
        }
        if (c) {
          if (a < 0) a = q;
          b = q;
        }
      }
      lo[t] = a < 0 ? 0 : a;
      hi[t] = a < 0 ? 0 : b;
    }
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return hi[a] - lo[a] > hi[b] - lo[b]; });
    for (int k = 0; k < nterms; ++k) {
      terms[3 * k] = lo[order[k]];
      terms[3 * k + 1] = hi[order[k]];
      terms[3 * k + 2] = order[k];
    }
  }
  int rc = aqc_mps_sort_batch(hs, ns);  // qubits back in site order, as measurements do
  if (rc != AQC_OK) return rc;
  rc = aqc_mps_check_batch(hs, ns);  // pending capacity / SVD flags of queued work: AQC_ERR_STATE
  if (rc != AQC_OK) return rc;
  const size_t cc = (size_t)cap * cap;
  const size_t per_wg = 3 * cc * sizeof(cplx);
  const size_t items = (size_t)nterms * ns;
  const int nwg = (int)std::max<size_t>(1, std::min<size_t>({items, (size_t)kMaxWg, kWsBytes / per_wg}));
  const size_t sb = up256((size_t)ns * sizeof(PauliState)), cb = up256((size_t)nterms * n);
  const size_t tb = up256(terms.size() * sizeof(int)), ob = up256(items * sizeof(double));
  const cplx* lenv = nullptr;
  size_t stride = 0;
  void* extra = nullptr;
  hipStream_t st = nullptr;
  rc = aqc::mps_envs_batch(hs, ns, sb + cb + tb + ob + (size_t)nwg * per_wg, "pauli_env", &lenv, &stride, &extra, &st);
  if (rc != AQC_OK) return rc;
  char* base = (char*)extra;
  std::vector<PauliState> states(ns);
  for (int s = 0; s < ns; ++s) {
    states[s].gam = hs[s]->d.gam;
    states[s].lam = hs[s]->d.lam;
    states[s].dims = hs[s]->d.dims;
    states[s].Lenv = lenv + (size_t)s * stride;
    states[s].Renv = states[s].Lenv + (size_t)(n + 1) * cc;
  }
  PauliJob j;
  std::memset(&j, 0, sizeof(j));
  j.states = (const PauliState*)base;
  j.codes = (const uint8_t*)(base + sb);
  j.terms = (const int*)(base + sb + cb);
  j.n = n;
  j.cap = cap;
  j.nterms = nterms;
  j.ns = ns;
  j.out = (double*)(base + sb + cb + tb);
  j.ws = (cplx*)(base + sb + cb + tb + ob);
  AQC_HIP_CHECK(hipMemcpyAsync(base, states.data(), (size_t)ns * sizeof(PauliState), hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemcpyAsync(base + sb, codes, (size_t)nterms * n, hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemcpyAsync(base + sb + cb, terms.data(), terms.size() * sizeof(int), hipMemcpyHostToDevice, st));
  double steps = 0.0;
  for (int k = 0; k < nterms; ++k) steps += (double)(terms[3 * k + 1] - terms[3 * k] + 1);
  aqc::KernelTimer::begin(st, "pauli_chain", 0.0, (double)ns * steps * 4.0 * 8.0 * (double)cc * cap);
  hipLaunchKernelGGL(k_pauli_chain, dim3(nwg), dim3(kThreads), 0, st, j);
  aqc::KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipMemcpyAsync(out, j.out, items * sizeof(double), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  return AQC_OK;
}

}  // namespace

extern "C" {

int aqc_sv_pauli_expect(aqc_sv_t h, const uint64_t* xmask, const uint64_t* zmask, int nterms, double* out) {
  AQC_REQUIRE(h && nterms >= 0 && ((xmask && zmask && out) || nterms == 0), "aqc_sv_pauli_expect: bad arguments");
  const cplx* state = nullptr;
  int n = 0;
  hipStream_t st = nullptr;
  if (int rc = aqc::sv_view(h, &state, &n, &st)) return rc;
  const uint64_t valid = n >= 64 ? ~0ull : (1ull << n) - 1;
  for (int t = 0; t < nterms; ++t)
    AQC_REQUIRE(((xmask[t] | zmask[t]) & ~valid) == 0, "aqc_sv_pauli_expect: a mask bit at or above n");
  if (nterms == 0) return AQC_OK;
  const uint64_t dim = 1ull << n;
  const int nblk = (int)std::min<uint64_t>(256, std::max<uint64_t>(1, dim / 4096));
  const size_t mb = up256((size_t)nterms * sizeof(uint64_t)), ob = up256((size_t)nterms * sizeof(double));
  const size_t pb = up256((size_t)nterms * nblk * sizeof(double));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  aqc::DevScratch& sc = g_scr.here();
  if (int rc = sc.ensure(2 * mb + pb + ob)) return rc;
  char* buf = sc.dev;
  uint64_t* dx = (uint64_t*)buf;
  uint64_t* dz = (uint64_t*)(buf + mb);
  double* partial = (double*)(buf + 2 * mb);
  double* dout = (double*)(buf + 2 * mb + pb);
  AQC_HIP_CHECK(hipMemcpyAsync(dx, xmask, (size_t)nterms * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemcpyAsync(dz, zmask, (size_t)nterms * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  aqc::KernelTimer::begin(st, "sv_pauli", 32.0 * (double)dim * nterms, 8.0 * (double)dim * nterms);
  for (int t0 = 0; t0 < nterms; t0 += kMaxTermsPerLaunch) {
    const int m = std::min(kMaxTermsPerLaunch, nterms - t0);
    hipLaunchKernelGGL(k_sv_pauli, dim3(nblk, m), dim3(kThreads), 0, st, state, dim, (const uint64_t*)(dx + t0),
                       (const uint64_t*)(dz + t0), partial + (size_t)t0 * nblk);
    AQC_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_sv_pauli_sum, dim3((nterms + 255) / 256), dim3(256), 0, st, (const double*)partial, nblk, nterms,
                     dout);
  aqc::KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipMemcpyAsync(out, dout, (size_t)nterms * sizeof(double), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  return AQC_OK;
}

int aqc_mps_pauli_expect(aqc_mps_t h, const uint8_t* codes, int nterms, double* out) {
  AQC_REQUIRE(h, "aqc_mps_pauli_expect: null handle");
  return mps_pauli(&h, 1, codes, nterms, out, "aqc_mps_pauli_expect");
}

int aqc_mps_pauli_expect_batch(aqc_mps_t* hs, int nstates, const uint8_t* codes, int nterms, double* out) {
  return mps_pauli(hs, nstates, codes, nterms, out, "aqc_mps_pauli_expect_batch");
}

}  // extern "C"
