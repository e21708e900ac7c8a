// ISL entanglement sweep: two-qubit reduced density matrices for every coupling-map pair and the
// 4x4 entanglement measures.  Replaces adaptaqc/compilers/adapt/adapt_compiler.py:955-976
// (_get_all_qubit_pair_entanglement_measures), whose loop calls
// entanglement_measures.py:39-98 (calculate_entanglement_measure) once per pair: a full SV
// partial trace (:326-340) or aqc_research.mps_operations.partial_trace per pair, then
// concurrence / EoF / negativity / log-negativity (:245-306) on the 4x4 result.
//
// MPS (preprocessed A_i = Gamma_i lambda_{i+1}, sorted qubits), no canonical form assumed:
//   L_{i+1} = sum_s A_i^{s dag} L_i A_i^s          (bra x ket, L_0 = 1)      k_rdm_env
//   R_i     = sum_s A_i^s R_{i+1} A_i^{s dag}      (ket x bra, R_n = 1)      k_rdm_env
//   P_b[s][sb] = A_b^s R_{b+1} A_b^{sb dag}                                   k_rdm_P
//   per first qubit a and bra/ket index pair (sb, s) of site a:               k_rdm_chain
//     E = A_a^{sb dag} L_a A_a^s;  for b > a:  rho_ab[(s, s_b), (sb, sb_b)] = Tr(E P_b[s_b][sb_b]),
//     E <- sum_t A_b^{t dag} E A_b^t
// Work per state: sum_a (n-1-a) transfer steps of 3 matrices x 4 chi^3 complex MACs, against
// the reference's n(n-1)/2 independent contractions.  Row index of a 4x4 RDM: 2*bit(b) + bit(a)
// for a < b (qiskit partial_trace convention: remaining qubits ascending, little-endian).
#include <algorithm>
#include <cstring>
#include <vector>

#include "aqc_gemm.h"
#include "herm4.h"
#include "mps_internal.h"

using aqc::cplx;

namespace {

constexpr int kT = aqc::kGemmThreads;
// the GEMMs of the environment chains fetch the next k tile's operands while the matrix cores run
// on the current one: a chain's steps are dependent, so each tile's global round trip was exposed
#ifndef AQC_ENV_PF
#define AQC_ENV_PF 1
#endif
constexpr bool kEnvPf = AQC_ENV_PF != 0;

struct RdmJob {
  const cplx* gam;
  const double* lam;
  const int* dims;
  int n;
  int cap;
  cplx* Lenv;   // (n+1) cap^2
  cplx* Renv;   // (n+1) cap^2
  cplx* tmpL;   // cap x 2cap
  cplx* tmpR;   // 2cap x cap
  cplx* P;      // n x 3 cap^2
  cplx* U;      // n x 3 cap^2
  cplx* chain;  // na x 3 x 4 cap^2
  cplx* rho;    // n x n x 16
};

__device__ __forceinline__ cplx aval(const RdmJob& j, int i, int s, int l, int r) {
  const size_t cc = (size_t)j.cap * j.cap;
  return aqc::cscale(j.gam[(size_t)i * 2 * cc + (size_t)s * cc + (size_t)l * j.cap + r], j.lam[(size_t)(i + 1) * j.cap + r]);
}

// blockIdx.x: 0 left / 1 right environments, blockIdx.y: state
__global__ __launch_bounds__(kT) void k_rdm_env(const RdmJob* __restrict__ jobs) {
  const RdmJob& j = jobs[blockIdx.y];
  __shared__ aqc::GemmLds lds;
  const int n = j.n, cap = j.cap;
  const size_t cc = (size_t)cap * cap;
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) j.Lenv[0] = aqc::cmk(1, 0);
    __syncthreads();
    for (int i = 0; i + 1 < n; ++i) {
      const int cl = j.dims[i], cr = j.dims[i + 1];
      const cplx* L = j.Lenv + (size_t)i * cc;
      cplx* T = j.tmpL;  // T[l][t*cap + r] = (L A^t)[l][r]
      aqc::block_cgemm<true, false, kEnvPf>(
          cl, 2 * cap, cl, [&](int r, int k) { return L[(size_t)r * cap + k]; },
          [&](int k, int c) { const int t = c / cap, r = c % cap; return r < cr ? aval(j, i, t, k, r) : aqc::cmk(0, 0); },
          [&](int r, int c, cplx v) { T[(size_t)r * 2 * cap + c] = v; }, lds);
      __syncthreads();
      cplx* Ln = j.Lenv + (size_t)(i + 1) * cc;
      aqc::block_cgemm<false, false, kEnvPf>(
          cr, cr, 2 * cl,
          [&](int r, int kk) { const int t = kk / cl, k = kk % cl; return aqc::cconj(aval(j, i, t, k, r)); },
          [&](int kk, int c) { const int t = kk / cl, k = kk % cl; return T[(size_t)k * 2 * cap + t * cap + c]; },
          [&](int r, int c, cplx v) { Ln[(size_t)r * cap + c] = v; }, lds);
      __syncthreads();
    }
  } else {
    if (threadIdx.x == 0) j.Renv[(size_t)n * cc] = aqc::cmk(1, 0);
    __syncthreads();
    for (int i = n - 1; i >= 1; --i) {
      const int cl = j.dims[i], cr = j.dims[i + 1];
      const cplx* R = j.Renv + (size_t)(i + 1) * cc;
      cplx* T = j.tmpR;  // T[t*cap + l][r] = (A^t R)[l][r]
      aqc::block_cgemm<true, false, kEnvPf>(
          2 * cap, cr, cr,
          [&](int rr, int k) { const int t = rr / cap, l = rr % cap; return l < cl ? aval(j, i, t, l, k) : aqc::cmk(0, 0); },
          [&](int k, int c) { return R[(size_t)k * cap + c]; }, [&](int rr, int c, cplx v) { T[(size_t)rr * cap + c] = v; },
          lds);
      __syncthreads();
      cplx* Rn = j.Renv + (size_t)i * cc;
      aqc::block_cgemm<true, true, kEnvPf>(
          cl, cl, 2 * cr,
          [&](int l, int kk) { const int t = kk / cr, k = kk % cr; return T[(size_t)(t * cap + l) * cap + k]; },
          [&](int kk, int c) { const int t = kk / cr, k = kk % cr; return aqc::cconj(aval(j, i, t, c, k)); },
          [&](int l, int c, cplx v) { Rn[(size_t)l * cap + c] = v; }, lds);
      __syncthreads();
    }
  }
}

// ---- environments over four workgroups per chain ---------------------------------------------
// k_rdm_env runs a chain (left or right, one state) in one workgroup: its n - 1 steps are dependent
// and each is ~1 M complex MACs at 2 chi = 128, so one CU's matrix cores bound it (~27 us a step at
// peak, 55 us measured: ~2.7 ms for a 50-site state).  Here kEnvNW workgroups share a chain by
// output columns: workgroup w owns columns c0 = w CW .. c0 + CW of every environment and computes
//   left:  T = L_i A_i^t[:, cols] (cl x 2 CW, both t),  L_{i+1}[:, cols] = sum_t A_i^{t dag} T_t
//   right: T = R_{i+1} conj(A_i^t[cols, :])^T,         R_i[:, cols]     = sum_t A_i^t T_t
// -- its own columns need only its own T, so a step has no exchange inside it.  Between steps the
// chain's workgroups hand the new environment over as gram_big.hip's column exchange does (sc1
// stores, s_waitcnt vmcnt(0), a barrier, one agent-scope counter add, one lane polling the counter;
// the next step reads the environment with sc1 loads).  Spins are bounded: a timeout sets *err and
// the host reports it.  The GEMMs keep each wave on 16 output rows and all of a block's (<= 64)
// columns, so a 16-column chunk wastes no MFMAs (block_cgemm's 64 x 64 blocks would waste 3/4).
constexpr int kEnvNW = 4;
constexpr int kEnvKT = 32;
struct NarrowLds {
  cplx As[kEnvKT][65];
  cplx Bs[kEnvKT][65];
};

typedef __attribute__((address_space(1))) double env_gdbl;
__device__ __forceinline__ void env_st(cplx* p, cplx v) {
  env_gdbl* q = (env_gdbl*)(double*)p;
  __hip_atomic_store(q, v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(q + 1, v.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ cplx env_ld(const cplx* p) {
  env_gdbl* q = (env_gdbl*)(double*)p;
  return aqc::cmk(__hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                  __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// C[i][j] = sum_k a(i, k) b(k, j) for i < m, j < n: blocks of 64 rows x NB columns, wave w on rows
// 16 w .. 16 w + 15 and all NB / 16 column tiles (v_mfma_f64_16x16x4_f64, a complex product as four
// real MFMAs); k in LDS tiles of kEnvKT with the next tile's operands fetched into registers while
// the matrix cores run.  AK / BK: consecutive threads walk k in a's / b's fetch (a source contiguous
// along k).  Ends on a barrier.
template <int NB, bool AK, bool BK, typename FA, typename FB, typename FS>
__device__ __forceinline__ void narrow_cgemm(int m, int n, int k, FA a, FB b, FS store, NarrowLds& lds) {
  constexpr int NT = NB / 16, EA = kEnvKT * 64 / kT, EB = kEnvKT * NB / kT;
  static_assert(NB % 16 == 0 && NB <= 64 && EB >= 1, "narrow_cgemm block width");
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  for (int bi = 0; bi < m; bi += 64) {
    for (int bj = 0; bj < n; bj += NB) {
      aqc::d4_t cr[NT], ci[NT];
#pragma unroll
      for (int c = 0; c < NT; ++c) cr[c] = aqc::d4_t{0, 0, 0, 0}, ci[c] = aqc::d4_t{0, 0, 0, 0};
      cplx pa[EA], pb[EB];
      auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < EA; ++q) {
          const int e = tid + q * kT, ka = AK ? e % kEnvKT : e / 64, ia = AK ? e / kEnvKT : e % 64;
          pa[q] = (bi + ia < m && k0 + ka < k) ? a(bi + ia, k0 + ka) : aqc::cmk(0, 0);
        }
#pragma unroll
        for (int q = 0; q < EB; ++q) {
          const int e = tid + q * kT, kb = BK ? e % kEnvKT : e / NB, ib = BK ? e / kEnvKT : e % NB;
          pb[q] = (bj + ib < n && k0 + kb < k) ? b(k0 + kb, bj + ib) : aqc::cmk(0, 0);
        }
      };
      fetch(0);
      for (int k0 = 0; k0 < k; k0 += kEnvKT) {
#pragma unroll
        for (int q = 0; q < EA; ++q) {
          const int e = tid + q * kT, ka = AK ? e % kEnvKT : e / 64, ia = AK ? e / kEnvKT : e % 64;
          lds.As[ka][ia] = pa[q];
        }
#pragma unroll
        for (int q = 0; q < EB; ++q) {
          const int e = tid + q * kT, kb = BK ? e % kEnvKT : e / NB, ib = BK ? e / kEnvKT : e % NB;
          lds.Bs[kb][ib] = pb[q];
        }
        __syncthreads();
        if (k0 + kEnvKT < k) fetch(k0 + kEnvKT);
#pragma unroll
        for (int ks = 0; ks < kEnvKT / 4; ++ks) {
          const int kk = 4 * ks + lk;
          const cplx av = lds.As[kk][16 * wave + li];
#pragma unroll
          for (int c = 0; c < NT; ++c) {
            const cplx bv = lds.Bs[kk][16 * c + li];
            cr[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, bv.x, cr[c], 0, 0, 0);
            cr[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(-av.y, bv.y, cr[c], 0, 0, 0);
            ci[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, bv.y, ci[c], 0, 0, 0);
            ci[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, bv.x, ci[c], 0, 0, 0);
          }
        }
        __syncthreads();
      }
#pragma unroll
      for (int c = 0; c < NT; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = bi + 16 * wave + lk + 4 * q, jj = bj + 16 * c + li;
          if (i < m && jj < n) store(i, jj, aqc::cmk(cr[c][q], ci[c][q]));
        }
    }
  }
}

// shader-clock ticks of workgroup (0, 0, 0)'s steps (aqc_env_ticks): T, the new environment's
// columns, the hand-off; then the steps counted
__device__ unsigned long long g_env_ticks[4];

// grid (2 states rounded up to 8, NW), kT threads; CW = cap / NW output columns per workgroup (NW =
// kEnvNW = 4 up to capacity 512; 16 workgroups of 64 columns at capacity 1024).  Counters:
// cnt[32 (2 state + dir)] (zeroed by the host).
template <int CW, int NW = kEnvNW>
__global__ __launch_bounds__(kT) void k_env_split(const RdmJob* __restrict__ jobs, unsigned* __restrict__ cnt,
                                                  int* __restrict__ err, unsigned long long spin, int nchains) {
  constexpr int NB1 = 2 * CW < 64 ? 2 * CW : 64, NB2 = CW < 64 ? CW : 64;
  // (grid as k_env64's: a chain's workgroups on one XCD)
  const int chain = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
  if (chain >= nchains) return;
  const int dir = chain & 1;
  const RdmJob& j = jobs[chain >> 1];
  unsigned* ctr = cnt + 32 * chain;
  __shared__ NarrowLds lds;
  __shared__ int s_abort;
  const int n = j.n, cap = j.cap;
  const size_t cc = (size_t)cap * cap;
  const int c0 = w * CW;
  cplx* Tw = (dir == 0 ? j.tmpL : j.tmpR) + (size_t)w * cap * 2 * CW;
  if (tid == 0) {
    s_abort = 0;
    if (w == 0) {  // the boundary environments, for the kernels after this one
      if (dir == 0) j.Lenv[0] = aqc::cmk(1, 0);
      else j.Renv[(size_t)n * cc] = aqc::cmk(1, 0);
    }
  }
  const bool tk = tid == 0 && chain == 0 && w == 0;
  unsigned long long t_last = tk ? __builtin_amdgcn_s_memtime() : 0ull, acc[3] = {0, 0, 0};
  auto tick = [&](int ph) {
    if (tk) {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      acc[ph] += t - t_last;
      t_last = t;
    }
  };
  for (int step = 0; step < n - 1; ++step) {
    if (dir == 0) {
      const int i = step, cl = j.dims[i], cr = j.dims[i + 1];
      const cplx* L = j.Lenv + (size_t)i * cc;
      narrow_cgemm<NB1, true, false>(
          cl, 2 * CW, cl, [&](int l, int k) { return i == 0 ? aqc::cmk(1, 0) : env_ld(L + (size_t)l * cap + k); },
          [&](int k, int c2) {
            const int t = c2 / CW, c = c0 + c2 % CW;
            return c < cr ? aval(j, i, t, k, c) : aqc::cmk(0, 0);
          },
          [&](int l, int c2, cplx v) { Tw[(size_t)l * 2 * CW + c2] = v; }, lds);
      __syncthreads();
      tick(0);
      cplx* Ln = j.Lenv + (size_t)(i + 1) * cc;
      narrow_cgemm<NB2, false, false>(
          cr, min(CW, cr - c0), 2 * cl,
          [&](int r, int kk) { const int t = kk / cl, k = kk % cl; return aqc::cconj(aval(j, i, t, k, r)); },
          [&](int kk, int c) { const int t = kk / cl, k = kk % cl; return Tw[(size_t)k * 2 * CW + t * CW + c]; },
          [&](int r, int c, cplx v) { env_st(Ln + (size_t)r * cap + c0 + c, v); }, lds);
    } else {
      const int i = n - 1 - step, cl = j.dims[i], cr = j.dims[i + 1];
      const cplx* R = j.Renv + (size_t)(i + 1) * cc;
      // T[k][t CW + c] = sum_k' R[k][k'] conj(A_t[c0 + c][k'])
      narrow_cgemm<NB1, true, true>(
          cr, 2 * CW, cr, [&](int k, int k2) { return i == n - 1 ? aqc::cmk(1, 0) : env_ld(R + (size_t)k * cap + k2); },
          [&](int k2, int c2) {
            const int t = c2 / CW, c = c0 + c2 % CW;
            return c < cl ? aqc::cconj(aval(j, i, t, c, k2)) : aqc::cmk(0, 0);
          },
          [&](int k, int c2, cplx v) { Tw[(size_t)k * 2 * CW + c2] = v; }, lds);
      __syncthreads();
      tick(0);
      cplx* Rn = j.Renv + (size_t)i * cc;
      // R_i[l][c0 + c] = sum_{t, k} A_t[l][k] T[k][t CW + c]
      narrow_cgemm<NB2, true, false>(
          cl, min(CW, cl - c0), 2 * cr,
          [&](int l, int kk) { const int t = kk / cr, k = kk % cr; return aval(j, i, t, l, k); },
          [&](int kk, int c) { const int t = kk / cr, k = kk % cr; return Tw[(size_t)k * 2 * CW + t * CW + c]; },
          [&](int l, int c, cplx v) { env_st(Rn + (size_t)l * cap + c0 + c, v); }, lds);
    }
    tick(1);
    // hand-off: every workgroup's columns of the new environment stored before the count
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned target = (unsigned)NW * (unsigned)(step + 1);
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(1);
        if (__builtin_amdgcn_s_memrealtime() - t0 > spin) {
          s_abort = 1;
          atomicOr(err, 1);
          break;
        }
      }
    }
    __syncthreads();
    tick(2);
    if (s_abort) return;
  }
  if (tk) {
    for (int ph = 0; ph < 3; ++ph) atomicAdd(&g_env_ticks[ph], acc[ph]);
    atomicAdd(&g_env_ticks[3], (unsigned long long)(n - 1));
  }
}

// ---- the chains at capacity 64 (chi = 64: the local-cost and entanglement workloads) -----------
// k_env_split's steps are latency-bound, not matrix-core-bound (tools/env_probe.py: ~56 K ticks a
// step against ~16 K of MFMA issue): every 32-deep k tile goes through the LDS behind two barriers
// with its global fetch one tile ahead, and the site operands are fetched after the hand-off.  Here
// (same split: four workgroups per chain, workgroup w owns output columns 16 w .. 16 w + 15, four
// waves of 16 rows each) the operands stay resident for the whole step:
//   - the site operands of step s + 1 do not depend on the environment: they are fetched while
//     step s's hand-off is polled -- GEMM 2's A fragments into registers (32 complex a lane), GEMM
//     1's B (the site's 16 columns, both physical indices) staged through registers into the LDS;
//   - after the hand-off only the environment fragments are on the path (16 complex a lane, sc1);
//   - GEMM 1 runs its whole contraction from registers and the LDS without a barrier, T goes to the
//     LDS (one barrier), GEMM 2 reads it from there;
//   - complex products in 3M form: P1 = ar br, P2 = ai bi, P3 = (ar + ai)(br + bi), Re = P1 - P2,
//     Im = P3 - P1 - P2 (three real MFMAs instead of four).
// Unified over the directions: E (ke x ke: L_i, or R_{i+1}) is GEMM 1's A operand,
//   T[l][16 t + c]   = sum_k E[l][k] B1[k][16 t + c],   B1 = A_t[k][c0 + c] (left) or conj(A_t[c0 + c][k]) (right)
//   out[r][c0 + c]   = sum_{t, k} A2[r][t, k] T[k][16 t + c],  A2 = conj(A_t[k][r]) (left) or A_t[r][k] (right)
// with out = L_{i+1} (m2 = dims[i + 1]) or R_i (m2 = dims[i]).
// Measured (tools/env_probe.py, 7 fifty-qubit states): 1.40 -> 1.28 ms per z_all call (1.12 with
// a chain's workgroups on one XCD, below; 1.05 with the hand-off traffic as 16-byte sc1 buffer
// accesses: T 20.5 K -> 17.4 K ticks); per step
// GEMM 2 36 K -> 7 K ticks (at its MFMA issue), GEMM 1 20 K, the hand-off 4 K -> 26 K: it now
// carries the operand prefetch (160 KB a workgroup), which no ordering tried hid behind the poll
// (wave 0 fetching after the poll: 1.67 ms, profiles/r5_env_chain_ab.json).
typedef unsigned env_u4 __attribute__((ext_vector_type(4)));
struct Env64Lds {
  cplx B1[64][33];
  cplx Ts[64][33];
};

__device__ __forceinline__ void mfma3(aqc::d4_t& p1, aqc::d4_t& p2, aqc::d4_t& p3, cplx a, cplx b) {
  p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, p1, 0, 0, 0);
  p2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.y, p2, 0, 0, 0);
  p3 = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x + a.y, b.x + b.y, p3, 0, 0, 0);
}

// grid (2 states rounded up to 8, 4), 256 threads; cap == 64.  Counters as k_env_split's.
__global__ __launch_bounds__(256) void k_env64(const RdmJob* __restrict__ jobs, unsigned* __restrict__ cnt,
                                               int* __restrict__ err, unsigned long long spin, int nchains) {
  constexpr int cap = 64;
  constexpr size_t cc = 64 * 64;
  // grid (chains rounded up to 8, 4): the chain's four workgroups at linear ids chain + 8 m w, on
  // one XCD under the dispatcher's round-robin placement, so that the three after the first find
  // the site's operands in that XCD's L2 (placement is a speed matter only: the hand-off stays
  // agent-scope).  Measured: the hand-off 26.7 K -> 17.6 K ticks a step, z_all 1.29 -> 1.12 ms.
  const int chain = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
  if (chain >= nchains) return;  // (the padding: whole workgroups)
  const int st = chain >> 1, dir = chain & 1;
  const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const RdmJob& j = jobs[st];
  unsigned* ctr = cnt + 32 * (2 * st + dir);
  __shared__ Env64Lds lds;
  __shared__ int s_abort;
  const int n = j.n, c0 = 16 * w, r0 = 16 * wave;
  if (tid == 0) {
    s_abort = 0;
    if (w == 0) {
      if (dir == 0) j.Lenv[0] = aqc::cmk(1, 0);
      else j.Renv[(size_t)n * cc] = aqc::cmk(1, 0);
    }
  }
  const bool tk = tid == 0 && chain == 0 && w == 0;
  unsigned long long t_last = tk ? __builtin_amdgcn_s_memtime() : 0ull, acc[3] = {0, 0, 0};
  auto tick = [&](int ph) {
    if (tk) {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      acc[ph] += t - t_last;
      t_last = t;
    }
  };
  // step s: site i, ke = the environment's dimension (both GEMMs' contraction), m2 = the output's
  auto site = [&](int s, int& i, int& ke, int& m2) {
    i = dir == 0 ? s : n - 1 - s;
    ke = dir == 0 ? j.dims[i] : j.dims[i + 1];
    m2 = dir == 0 ? j.dims[i + 1] : j.dims[i];
  };
  cplx b1[8], a2[2][16];
  auto fetch_site = [&](int s) {
    int i, ke, m2;
    site(s, i, ke, m2);
    const cplx* g = j.gam + (size_t)i * 2 * cc;
    const double* lam = j.lam + (size_t)(i + 1) * cap;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = tid + 256 * q;
      if (dir == 0) {  // B1[k][16 t + c] = A_t[k][c0 + c]: c fastest (256-byte runs)
        const int c = e & 15, t = (e >> 4) & 1, k = e >> 5, col = c0 + c;
        b1[q] = (k < ke && col < m2) ? aqc::cscale(g[t * cc + k * cap + col], lam[col]) : aqc::cmk(0, 0);
      } else {  // conj(A_t[c0 + c][k]): k fastest
        const int k = e & 63, t = (e >> 6) & 1, c = e >> 7, row = c0 + c;
        b1[q] = (k < ke && row < m2) ? aqc::cconj(aqc::cscale(g[t * cc + row * cap + k], lam[k])) : aqc::cmk(0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        const int r = r0 + li, k = 4 * ks + lk;
        cplx v = aqc::cmk(0, 0);
        if (r < m2 && k < ke)
          v = dir == 0 ? aqc::cconj(aqc::cscale(g[t * cc + k * cap + r], lam[r])) : aqc::cscale(g[t * cc + r * cap + k], lam[k]);
        a2[t][ks] = v;
      }
  };
  fetch_site(0);
  for (int step = 0; step < n - 1; ++step) {
    int i, ke, m2;
    site(step, i, ke, m2);
    const int nks = (ke + 3) >> 2;  // 4-deep k steps holding the contraction
    // B1 into the LDS (its previous contents were last read before the previous step's T barrier)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = tid + 256 * q;
      if (dir == 0) lds.B1[e >> 5][16 * ((e >> 4) & 1) + (e & 15)] = b1[q];
      else lds.B1[e & 63][16 * ((e >> 6) & 1) + (e >> 7)] = b1[q];
    }
    // the environment's fragments: E[r0 + li][4 ks + lk]
    // (16-byte agent-coherent loads: a buffer load with sc1, aux = 16 -- half the instructions of two
    // 8-byte atomic loads; the hand-off's counter orders them)
    cplx ef[16];
    const cplx* E = dir == 0 ? j.Lenv + (size_t)i * cc : j.Renv + (size_t)(i + 1) * cc;
    const auto re = aqc::make_rsrc(E, (unsigned)(cc * sizeof(cplx)));
    const bool first = step == 0;  // E = [[1]] (ke = 1)
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const int r = r0 + li, k = 4 * ks + lk;
      ef[ks] = (r < ke && k < ke)
                   ? (first ? aqc::cmk(1, 0)
                            : __builtin_bit_cast(cplx, __builtin_amdgcn_raw_buffer_load_b128(re, (unsigned)(r * cap + k) * 16u, 0u, 16)))
                   : aqc::cmk(0, 0);
    }
    __syncthreads();
    // ---- GEMM 1: T = E B1 (this wave's 16 rows, both t)
    {
      aqc::d4_t p1[2], p2[2], p3[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) p1[t] = p2[t] = p3[t] = aqc::d4_t{0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        if (ks < nks) {
#pragma unroll
          for (int t = 0; t < 2; ++t) mfma3(p1[t], p2[t], p3[t], ef[ks], lds.B1[4 * ks + lk][16 * t + li]);
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          lds.Ts[r0 + lk + 4 * q][16 * t + li] = aqc::cmk(p1[t][q] - p2[t][q], p3[t][q] - p1[t][q] - p2[t][q]);
    }
    __syncthreads();
    tick(0);
    // ---- GEMM 2: out[r][c0 + c] = sum_{t, k} A2[r][t, k] T[k][16 t + c]
    {
      aqc::d4_t p1 = aqc::d4_t{0, 0, 0, 0}, p2 = p1, p3 = p1;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int ks = 0; ks < 16; ++ks)
          if (ks < nks) mfma3(p1, p2, p3, a2[t][ks], lds.Ts[4 * ks + lk][16 * t + li]);
      cplx* out = dir == 0 ? j.Lenv + (size_t)(i + 1) * cc : j.Renv + (size_t)i * cc;
      const auto ro = aqc::make_rsrc(out, (unsigned)(cc * sizeof(cplx)));
      const int col = c0 + li;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = r0 + lk + 4 * q;
        if (r < m2 && col < m2)
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(env_u4, aqc::cmk(p1[q] - p2[q], p3[q] - p1[q] - p2[q])), ro,
                                                 (unsigned)(r * cap + col) * 16u, 0u, 16);
      }
    }
    tick(1);
    // hand-off: this workgroup's columns stored before the count; the next step's site operands are
    // fetched while thread 0 polls
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (step + 1 < n - 1) fetch_site(step + 1);
    if (tid == 0) {
      const unsigned target = 4u * (unsigned)(step + 1);
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(1);
        if (__builtin_amdgcn_s_memrealtime() - t0 > spin) {
          s_abort = 1;
          atomicOr(err, 1);
          break;
        }
      }
    }
    __syncthreads();
    tick(2);
    if (s_abort) return;
  }
  if (tk) {
    for (int ph = 0; ph < 3; ++ph) atomicAdd(&g_env_ticks[ph], acc[ph]);
    atomicAdd(&g_env_ticks[3], (unsigned long long)(n - 1));
  }
}

// ---- the sum of every <Z_i> through a window (the local cost's candidates, round 6) -----------
// The local cost (aer_mps_backend.py:72-74, 80-86) needs only sum_i <Z_i>.  That sum is the
// expectation of the bond-2 operator sum_i Z_i, whose environments are pairs: from the left
//   L_{i+1} = sum_s A_s^dag L_i A_s,   LZ_{i+1} = sum_s A_s^dag (LZ_i + z_s L_i) A_s    (z = +1, -1)
// (LZ_b: one Z somewhere left of bond b), from the right likewise, and sum_i <Z_i> = Tr(LZ_b R_b) +
// Tr(L_b RZ_b) at any bond b.  A Rotoselect candidate is a copy of the prefix state rewritten only
// on sites lo..hi (its gate, the suffix and the final sort: the handle's reload bookkeeping), so its
// sum needs the prefix's pairs at bonds lo and hi + 1 (cached on the prefix handle and extended as
// it changes) and its own chains through lo..hi only (from both ends, meeting in the middle:
// Tr(LZ R) + Tr(L RZ) holds at any bond) -- instead of both full chains per
// candidate.  A step is k_env_split's with the environment rows doubled: GEMM 1 takes [E; EZ]
// (2 ke rows) against the site's columns, GEMM 2 writes E' to output columns [0, cw) and EZ' to
// [cw, 2 cw), reading T_E for the first and T_EZ + z_t T_E for the second.
struct ZJob {
  const cplx* gam;
  const double* lam;
  const int* dims;
  int cap;
  int dir;          // 0: left, sites first, first + 1, ...; 1: right, sites first, first - 1, ...
  int first;
  int nsteps;
  const cplx* ein;  // the pair (E, EZ) at the starting bond (2 cap^2)
  cplx* eout;       // step s's pair at eout + (dir ? -s : s) 2 cap^2
  cplx* tmp;        // NW x 2 cap x 2 cw
};

// grid (chains, NW), kT threads; cw = cap / NW output columns of each environment per workgroup.
// Counters and the bounded hand-off as k_env_split's.
template <int NB, int NW>
__global__ __launch_bounds__(kT) void k_zenv(const ZJob* __restrict__ jobs, unsigned* __restrict__ cnt,
                                             int* __restrict__ err, unsigned long long spin, int nchains, int cw) {
  const int chain = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
  if (chain >= nchains) return;
  const ZJob& j = jobs[chain];
  unsigned* ctr = cnt + 32 * chain;
  __shared__ NarrowLds lds;
  __shared__ int s_abort;
  const int cap = j.cap, dir = j.dir;
  const size_t cc = (size_t)cap * cap;
  const int c0 = w * cw, ldt = 2 * cw;
  cplx* Tw = j.tmp + (size_t)w * 2 * cap * ldt;
  if (tid == 0) s_abort = 0;
  for (int s = 0; s < j.nsteps; ++s) {
    const int i = dir == 0 ? j.first + s : j.first - s;
    const cplx* E = s == 0 ? j.ein : j.eout + (ptrdiff_t)(dir ? 1 - s : s - 1) * 2 * (ptrdiff_t)cc;
    cplx* O = j.eout + (ptrdiff_t)(dir ? -s : s) * 2 * (ptrdiff_t)cc;
    const int ke = dir == 0 ? j.dims[i] : j.dims[i + 1];
    const int m2 = dir == 0 ? j.dims[i + 1] : j.dims[i];
    const cplx* g = j.gam + (size_t)i * 2 * cc;
    const double* lam = j.lam + (size_t)(i + 1) * cap;
    auto site = [&](int t, int l, int r) {  // A_t[l][r] = Gamma_t[l][r] lambda_{i+1}[r]
      return aqc::cscale(g[t * cc + (size_t)l * cap + r], lam[r]);
    };
    auto ea = [&](int l, int k) { return env_ld(E + (l < ke ? 0 : cc) + (size_t)(l < ke ? l : l - ke) * cap + k); };
    auto ts = [&](int l, int c2, cplx v) { Tw[(size_t)l * ldt + c2] = v; };
    if (dir == 0)  // T[l][t cw + c] = sum_k [E; EZ][l][k] A_t[k][c0 + c]
      narrow_cgemm<NB, true, false>(
          2 * ke, ldt, ke, ea,
          [&](int k, int c2) { const int t = c2 / cw, c = c0 + c2 % cw; return c < m2 ? site(t, k, c) : aqc::cmk(0, 0); }, ts,
          lds);
    else  // T[k][t cw + c] = sum_k' [R; RZ][k][k'] conj(A_t[c0 + c][k'])
      narrow_cgemm<NB, true, true>(
          2 * ke, ldt, ke, ea,
          [&](int k2, int c2) {
            const int t = c2 / cw, c = c0 + c2 % cw;
            return c < m2 ? aqc::cconj(site(t, c, k2)) : aqc::cmk(0, 0);
          },
          ts, lds);
    __syncthreads();
    // GEMM 2 over 2 cw output columns: [0, cw) the environment, [cw, 2 cw) its Z partner
    auto tb = [&](int kk, int c2) {
      const int t = kk / ke, k = kk % ke, zc = c2 < cw ? c2 : c2 - cw, col = t * cw + zc;
      if (c0 + zc >= m2) return aqc::cmk(0, 0);
      const cplx te = Tw[(size_t)k * ldt + col];
      if (c2 < cw) return te;
      const cplx tz = Tw[(size_t)(ke + k) * ldt + col];
      return t == 0 ? aqc::cadd(tz, te) : aqc::csub(tz, te);
    };
    auto os = [&](int r, int c2, cplx v) {
      const int zc = c2 < cw ? c2 : c2 - cw;
      if (c0 + zc < m2) env_st(O + (c2 < cw ? 0 : cc) + (size_t)r * cap + c0 + zc, v);
    };
    if (dir == 0)  // L'[r][c0 + c] = sum_{t, k} conj(A_t[k][r]) T[k][t cw + c]
      narrow_cgemm<NB, false, false>(
          m2, ldt, 2 * ke, [&](int r, int kk) { return aqc::cconj(site(kk / ke, kk % ke, r)); }, tb, os, lds);
    else  // R'[l][c0 + c] = sum_{t, k} A_t[l][k] T[k][t cw + c]
      narrow_cgemm<NB, true, false>(
          m2, ldt, 2 * ke, [&](int l, int kk) { return site(kk / ke, l, kk % ke); }, tb, os, lds);
    // hand-off (k_env_split's)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned target = (unsigned)NW * (unsigned)(s + 1);
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(1);
        if (__builtin_amdgcn_s_memrealtime() - t0 > spin) {
          s_abort = 1;
          atomicOr(err, 1);
          break;
        }
      }
    }
    __syncthreads();
    if (s_abort) return;
  }
}

// out[s] = Re Tr(LZ R) + Re Tr(L RZ) for the pairs (L, LZ) at lp and (R, RZ) at rp, of bond
// dimension dims[bond]; L[b][k] is bra x ket, R[k][b] ket x bra.  grid (states), kT threads.
struct ZSumJob {
  const cplx* lp;
  const cplx* rp;
  const int* dims;
  int bond;
  int cap;
};
__global__ __launch_bounds__(kT) void k_zsum(const ZSumJob* __restrict__ jobs, double* __restrict__ out) {
  const ZSumJob& j = jobs[blockIdx.x];
  const int d = j.dims[j.bond], cap = j.cap;
  const size_t cc = (size_t)cap * cap;
  double acc = 0.0;
  for (int e = threadIdx.x; e < d * d; e += kT) {
    const int b = e / d, k = e % d;  // L[b][k] R[k][b]
    const cplx l = aqc::ldg(j.lp + (size_t)b * cap + k), lz = aqc::ldg(j.lp + cc + (size_t)b * cap + k);
    const cplx r = aqc::ldg(j.rp + (size_t)k * cap + b), rz = aqc::ldg(j.rp + cc + (size_t)k * cap + b);
    acc = fma(lz.x, r.x, fma(-lz.y, r.y, acc));
    acc = fma(l.x, rz.x, fma(-l.y, rz.y, acc));
  }
  __shared__ double red[kT];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int k = kT / 2; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// the boundary pairs of a fresh cache: L_0 = [[1]], R_n = [[1]] (LZ_0 = RZ_n = 0 from the memset)
__global__ void k_zenv_init(cplx* l0, cplx* rn) {
  if (threadIdx.x == 0) {
    l0[0] = aqc::cmk(1, 0);
    rn[0] = aqc::cmk(1, 0);
  }
}

// P_b[s][sb] = A_b^s R_{b+1} A_b^{sb dag}, stored transposed (j.P holds P^T: the traces against it,
// Tr(E P) in the pair chains and Tr(L P) in k_rdm_ztrace, then read both operands along rows);
// m = 0: (0,0), 1: (0,1), 2: (1,1).  grid (n, 3 or 2, states);
// with two m, the diagonal pair (0,0), (1,1) only (single-site <Z>).  first_site: site 0 too (pair
// RDMs never need it: it is never the second qubit of a pair)
__global__ __launch_bounds__(kT) void k_rdm_P(const RdmJob* __restrict__ jobs, int first_site) {
  const RdmJob& j = jobs[blockIdx.z];
  __shared__ aqc::GemmLds lds;
  const int b = blockIdx.x, m = gridDim.y == 2 ? 2 * (int)blockIdx.y : (int)blockIdx.y;
  if (b == 0 && !first_site) return;
  const int s = m == 2 ? 1 : 0, sb = m == 0 ? 0 : 1;
  const int cap = j.cap;
  const size_t cc = (size_t)cap * cap;
  const int cl = j.dims[b], cr = j.dims[b + 1];
  const cplx* R = j.Renv + (size_t)(b + 1) * cc;
  cplx* U = j.U + ((size_t)b * 3 + m) * cc;
  cplx* P = j.P + ((size_t)b * 3 + m) * cc;
  aqc::block_cgemm<true, false, kEnvPf>(
      cl, cr, cr, [&](int l, int k) { return aval(j, b, s, l, k); }, [&](int k, int c) { return R[(size_t)k * cap + c]; },
      [&](int l, int c, cplx v) { U[(size_t)l * cap + c] = v; }, lds);
  __syncthreads();
  aqc::block_cgemm<true, true, kEnvPf>(
      cl, cl, cr, [&](int l, int k) { return U[(size_t)l * cap + k]; },
      [&](int k, int c) { return aqc::cconj(aval(j, b, sb, c, k)); }, [&](int l, int c, cplx v) { P[(size_t)c * cap + l] = v; },
      lds);
}

// grid (3 bra/ket combos of site a, first qubits, states)
__global__ __launch_bounds__(kT) void k_rdm_chain(const RdmJob* __restrict__ jobs, const int* __restrict__ alist,
                                                  int ns) {
  // (from 8 states up, a state's chains -- which read the same P_b and site tensors -- on one
  // XCD; below, over the state's share of the XCDs: aqc_internal.h xcd_job_block; block = 3 ai + m)
  int st, blk;
  if (!aqc::xcd_job_block(ns, st, blk, true)) return;
  const RdmJob& j = jobs[st];
  __shared__ aqc::GemmLds lds;
  __shared__ double red[8][kT / 64];
  const int m = blk % 3, ai = blk / 3, a = alist[ai];
  const int sb = m == 2 ? 1 : 0, s = m == 0 ? 0 : 1;  // E[sb][s]: bra index sb, ket index s
  const int n = j.n, cap = j.cap, tid = threadIdx.x;
  const size_t cc = (size_t)cap * cap;
  cplx* base = j.chain + ((size_t)ai * 3 + m) * 4 * cc;
  cplx* Eb[2] = {base, base + cc};
  cplx* T = base + 2 * cc;  // cap x 2cap
  {
    const int cl = j.dims[a], cr = j.dims[a + 1];
    const cplx* L = j.Lenv + (size_t)a * cc;
    aqc::block_cgemm<true, false, kEnvPf>(
        cl, cr, cl, [&](int r, int k) { return L[(size_t)r * cap + k]; }, [&](int k, int c) { return aval(j, a, s, k, c); },
        [&](int r, int c, cplx v) { T[(size_t)r * 2 * cap + c] = v; }, lds);
    __syncthreads();
    cplx* E = Eb[0];
    aqc::block_cgemm<false, false, kEnvPf>(
        cr, cr, cl, [&](int r, int k) { return aqc::cconj(aval(j, a, sb, k, r)); },
        [&](int k, int c) { return T[(size_t)k * 2 * cap + c]; }, [&](int r, int c, cplx v) { E[(size_t)r * cap + c] = v; },
        lds);
    __syncthreads();
  }
  int cur = 0;
  for (int b = a + 1; b < n; ++b) {
    const int cl = j.dims[b], cr = j.dims[b + 1];
    const cplx* E = Eb[cur];
    // closing: v[s_b][sb_b] = sum_{ij} E[i][j] P_b[s_b][sb_b][j][i], with P[1][0] = P[0][1]^dag
    // (j.P holds P^T: E and three of the four operands read along rows)
    const cplx* P00 = j.P + ((size_t)b * 3 + 0) * cc;
    const cplx* P01 = j.P + ((size_t)b * 3 + 1) * cc;
    const cplx* P11 = j.P + ((size_t)b * 3 + 2) * cc;
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int e = tid; e < cl * cl; e += kT) {
      const int i = e / cl, jj = e % cl;
      const cplx ev = E[(size_t)i * cap + jj];
      const cplx p00 = P00[(size_t)i * cap + jj], p01 = P01[(size_t)i * cap + jj], p11 = P11[(size_t)i * cap + jj];
      const cplx p10 = aqc::cconj(P01[(size_t)jj * cap + i]);
      const cplx v00 = aqc::cmul(ev, p00), v01 = aqc::cmul(ev, p01), v10 = aqc::cmul(ev, p10), v11 = aqc::cmul(ev, p11);
      acc[0] += v00.x, acc[1] += v00.y, acc[2] += v01.x, acc[3] += v01.y;
      acc[4] += v10.x, acc[5] += v10.y, acc[6] += v11.x, acc[7] += v11.y;
    }
    // wave sums (DPP rows, then readlane), the waves' partials through the LDS
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const double w = aqc::row_sum16(acc[q]);
      double t = 0.0;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        t += __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(w), 16 * rr),
                              __builtin_amdgcn_readlane(__double2loint(w), 16 * rr));
      if ((tid & 63) == 0) red[q][tid >> 6] = t;
    }
    __syncthreads();
    if (tid < 4) {
      const int sbk = tid >> 1, sbb = tid & 1;  // ket / bra index of site b
      double re = 0.0, im = 0.0;
#pragma unroll
      for (int w = 0; w < kT / 64; ++w) re += red[2 * tid][w], im += red[2 * tid + 1][w];
      const cplx v = aqc::cmk(re, im);
      cplx* rho = j.rho + ((size_t)a * n + b) * 16;
      rho[(2 * sbk + s) * 4 + (2 * sbb + sb)] = v;
      if (m == 1) rho[(2 * sbb + sb) * 4 + (2 * sbk + s)] = aqc::cconj(v);  // the (sb=1, s=0) block
    }
    __syncthreads();
    if (b + 1 >= n) break;
    // transfer through site b: E' = sum_t A_b^{t dag} E A_b^t
    aqc::block_cgemm<true, false, kEnvPf>(
        cl, 2 * cap, cl, [&](int r, int k) { return E[(size_t)r * cap + k]; },
        [&](int k, int c) { const int t = c / cap, r = c % cap; return r < cr ? aval(j, b, t, k, r) : aqc::cmk(0, 0); },
        [&](int r, int c, cplx v) { T[(size_t)r * 2 * cap + c] = v; }, lds);
    __syncthreads();
    cplx* En = Eb[cur ^ 1];
    aqc::block_cgemm<false, false, kEnvPf>(
        cr, cr, 2 * cl,
        [&](int r, int kk) { const int t = kk / cl, k = kk % cl; return aqc::cconj(aval(j, b, t, k, r)); },
        [&](int kk, int c) { const int t = kk / cl, k = kk % cl; return T[(size_t)k * 2 * cap + t * cap + c]; },
        [&](int r, int c, cplx v) { En[(size_t)r * cap + c] = v; }, lds);
    __syncthreads();
    cur ^= 1;
  }
}

// requested pairs (c, t) -> rho of (min, max); grid over pairs x states
// <Z_b> = rho_b[0][0] - rho_b[1][1], rho_b[s][sb] = Tr(L_b P_b[s][sb]) (the single-site RDM of the
// same environments).  grid (n, states)
__global__ __launch_bounds__(kT) void k_rdm_ztrace(const RdmJob* __restrict__ jobs, double* __restrict__ out) {
  const RdmJob& j = jobs[blockIdx.y];
  const int b = blockIdx.x, cap = j.cap;
  const size_t cc = (size_t)cap * cap;
  const int cl = j.dims[b];
  const cplx* L = j.Lenv + (size_t)b * cc;
  const cplx* P0 = j.P + ((size_t)b * 3 + 0) * cc;
  const cplx* P1 = j.P + ((size_t)b * 3 + 2) * cc;
  __shared__ double red[kT];
  double acc = 0.0;
  for (int e = threadIdx.x; e < cl * cl; e += kT) {
    const int c = e % cl, cp = e / cl;  // L[cp][c] P[c][cp] (j.P holds P^T: both along rows)
    const cplx l = L[(size_t)cp * cap + c];
    const cplx d = aqc::csub(P0[(size_t)cp * cap + c], P1[(size_t)cp * cap + c]);
    acc = fma(l.x, d.x, fma(-l.y, d.y, acc));
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int k = kT / 2; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[(size_t)blockIdx.y * j.n + b] = red[0];
}

__global__ void k_rdm_gather(const RdmJob* __restrict__ jobs, const int* __restrict__ pairs, int npairs,
                             cplx* __restrict__ out) {
  const RdmJob& j = jobs[blockIdx.y];
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < npairs * 16; e += gridDim.x * blockDim.x) {
    const int p = e / 16, q = e % 16;
    const int a = min(pairs[2 * p], pairs[2 * p + 1]), b = max(pairs[2 * p], pairs[2 * p + 1]);
    out[((size_t)blockIdx.y * npairs + p) * 16 + q] = j.rho[((size_t)a * j.n + b) * 16 + q];
  }
}

// ---- 4x4 entanglement measures (the Hermitian eigensolver: herm4.h) ---------------------------
using aqc::herm4_eig;

__device__ double concurrence4(const cplx rho[4][4]) {
  // eig(rho rho~) = eig(S rho~ S), S = sqrt(rho) (Hermitian PSD): same non-zero spectrum, and the
  // Hermitian form keeps the eigenvalues real (the reference's eig path returns 0 when they are not)
  cplx H[4][4], V[4][4];
  double d[4];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) H[r][c] = rho[r][c];
  herm4_eig(H, d, V, true);
  cplx S[4][4];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      cplx acc = aqc::cmk(0, 0);
      for (int k = 0; k < 4; ++k)
        acc = aqc::cfma(aqc::cscale(V[r][k], sqrt(fmax(d[k], 0.0))), aqc::cconj(V[c][k]), acc);
      S[r][c] = acc;
    }
  const double y[4] = {-1.0, 1.0, 1.0, -1.0};  // sigma_y (x) sigma_y is anti-diagonal (-1, 1, 1, -1)
  cplx Rt[4][4], X[4][4];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) Rt[r][c] = aqc::cscale(aqc::cconj(rho[3 - r][3 - c]), y[r] * y[c]);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      cplx acc = aqc::cmk(0, 0);
      for (int k = 0; k < 4; ++k) acc = aqc::cfma(S[r][k], Rt[k][c], acc);
      X[r][c] = acc;
    }
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      cplx acc = aqc::cmk(0, 0);
      for (int k = 0; k < 4; ++k) acc = aqc::cfma(X[r][k], S[k][c], acc);
      H[r][c] = acc;
    }
  for (int r = 0; r < 4; ++r) {  // symmetrise rounding
    H[r][r].y = 0.0;
    for (int c = r + 1; c < 4; ++c) {
      const cplx m = aqc::cscale(aqc::cadd(H[r][c], aqc::cconj(H[c][r])), 0.5);
      H[r][c] = m;
      H[c][r] = aqc::cconj(m);
    }
  }
  herm4_eig(H, d, V, false);
  double l[4];
  for (int k = 0; k < 4; ++k) l[k] = sqrt(fmax(d[k], 0.0));
  for (int x = 0; x < 4; ++x)  // sort descending
    for (int z = x + 1; z < 4; ++z)
      if (l[z] > l[x]) {
        const double t = l[x];
        l[x] = l[z];
        l[z] = t;
      }
  return fmax(0.0, l[0] - l[1] - l[2] - l[3]);
}

__device__ double trace_norm_pt(const cplx rho[4][4]) {
  // partial transpose w.r.t. the first (high) subsystem (entanglement_measures.py:343-356);
  // Hermitian, so its trace norm is the sum of |eigenvalues|
  cplx H[4][4], V[4][4];
  double d[4];
  for (int ja = 0; ja < 2; ++ja)
    for (int ka = 0; ka < 2; ++ka)
      for (int jb = 0; jb < 2; ++jb)
        for (int kb = 0; kb < 2; ++kb) H[ka * 2 + jb][ja * 2 + kb] = rho[ja * 2 + jb][ka * 2 + kb];
  herm4_eig(H, d, V, false);
  return fabs(d[0]) + fabs(d[1]) + fabs(d[2]) + fabs(d[3]);
}

// method: 0 concurrence, 1 EoF, 2 negativity, 3 log-negativity
__global__ void k_ent_measure(const cplx* __restrict__ rdms, int count, int method, double* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= count) return;
  cplx rho[4][4];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) rho[r][c] = rdms[(size_t)p * 16 + r * 4 + c];
  double v = 0.0;
  if (method == 0 || method == 1) {
    const double c = concurrence4(rho);
    if (method == 0) {
      v = c;
    } else if (c != 0.0) {
      // entanglement_measures.py:263-275 (1 - c^2 clamped at 0: C rounds to 1 + O(eps) on Bell pairs)
      const double x = 0.5 * (1.0 + sqrt(fmax(0.0, 1.0 - c * c)));
      v = (x >= 1.0) ? 0.0 : -x * log2(x) - (1.0 - x) * log2(1.0 - x);
    }
  } else {
    const double tn = trace_norm_pt(rho);
    v = method == 2 ? (tn - 1.0) / 2.0 : log2(tn);
  }
  out[p] = v;
}

aqc::PerDevice<aqc::DevScratch> g_rbuf;  // jobs, environments and results of every entry point here

// Counter / error words behind the jobs of an environment launch: 32 words per chain, one error word.
size_t env_sync_bytes(int ns) { return aqc::up256(((size_t)ns * 2 * 32 + 32) * sizeof(unsigned)); }

// Output columns per workgroup of the split environment chains for a capacity, or 0 where the
// chains run one workgroup each (k_rdm_env).  Each split kernel's slices of tmpL / tmpR are sized for
// exactly cap = kEnvNW x CW (cap = 192, 320, 384, 448 once fell to k_env_split<128> and its
// slices ran past the 2 cap^2 scratch), so only these four capacities take them.
int env_split_cols(int cap) {
  switch (cap) {
    case 64: return 16;
    case 128: return 32;
    case 256: return 64;
    case 512: return 128;
    case 1024: return 64;  // (16 workgroups per chain: env_split_nw)
    default: return 0;
  }
}
// workgroups per chain of the split kernels
int env_split_nw(int cap) { return cap == 1024 ? 16 : kEnvNW; }

// environment launches that timed out on a hand-off and were re-run by k_rdm_env (aqc_env_fallbacks)
unsigned long long g_env_fallbacks = 0;
int g_env_single = 0;  // aqc_env_set_single: every chain on one workgroup
constexpr unsigned long long kEnvSpin = 200000000ull;  // s_memrealtime (100 MHz): 2 s
unsigned long long g_env_spin = kEnvSpin;  // aqc_env_set_spin_limit (0: any unsatisfied wait times out)

// The left / right environments of every state: kEnvNW workgroups per chain where the capacity
// is one of env_split_cols' (k_env64 at capacity 64, k_env_split above), else -- or with single --
// k_rdm_env; states in rounds small enough that every chain's workgroups are resident together.
// sync: env_sync_bytes(ns) of device memory.
int launch_envs(RdmJob* djobs, int ns, int cap, hipStream_t st, void* sync, bool single = false) {
  const int cw = (single || g_env_single) ? 0 : env_split_cols(cap);
  if (cw == 0) {
    hipLaunchKernelGGL(k_rdm_env, dim3(2, ns), dim3(kT), 0, st, djobs);
    AQC_CHECK_LAUNCH();
    return AQC_OK;
  }
  unsigned* cnt = (unsigned*)sync;
  int* err = (int*)(cnt + (size_t)ns * 2 * 32);
  AQC_HIP_CHECK(hipMemsetAsync(sync, 0, env_sync_bytes(ns), st));
  const unsigned long long kSpin = g_env_spin;
  const int nw = env_split_nw(cap);
  // 28 states x 2 chains x 4 workgroups (224, one per CU: ~400 VGPRs a lane) leave room; as many
  // workgroups in a round at 16 per chain
  const int kRound = std::max(1, 224 / (2 * nw));
  for (int s0 = 0; s0 < ns; s0 += kRound) {
    const int m = std::min(kRound, ns - s0);
    const dim3 xg((2 * m + 7) / 8 * 8, nw);  // (chains padded to 8, workgroup: one XCD per chain)
    RdmJob* jb = djobs + s0;
    unsigned* cb = cnt + (size_t)s0 * 2 * 32;
    switch (nw == kEnvNW ? cw : -cw) {
      case -64: hipLaunchKernelGGL((k_env_split<64, 16>), xg, dim3(kT), 0, st, jb, cb, err, kSpin, 2 * m); break;
      case 16: hipLaunchKernelGGL(k_env64, xg, dim3(256), 0, st, jb, cb, err, kSpin, 2 * m); break;
      case 32: hipLaunchKernelGGL(k_env_split<32>, xg, dim3(kT), 0, st, jb, cb, err, kSpin, 2 * m); break;
      case 64: hipLaunchKernelGGL(k_env_split<64>, xg, dim3(kT), 0, st, jb, cb, err, kSpin, 2 * m); break;
      case 128: hipLaunchKernelGGL(k_env_split<128>, xg, dim3(kT), 0, st, jb, cb, err, kSpin, 2 * m); break;
      default: aqc::set_error("launch_envs: no split environment kernel for this capacity"); return AQC_ERR_ARG;
    }
    AQC_CHECK_LAUNCH();
  }
  return AQC_OK;
}

// After the stream synchronised: did a split chain's hand-off time out (its workgroups were not all
// resident together, e.g. while other streams' kernels held CUs)?  *timed_out = true: the caller
// re-runs the call with single-workgroup chains (k_rdm_env, no co-residency needed) -- a scheduling
// condition, not a failure of the evaluation; gram_big declines to the block Jacobi the same way.
int env_timed_out(void* sync, int ns, int cap, bool& timed_out) {
  timed_out = false;
  if (g_env_single || env_split_cols(cap) == 0) return AQC_OK;
  int e = 0;
  AQC_HIP_CHECK(hipMemcpy(&e, (int*)((unsigned*)sync + (size_t)ns * 2 * 32), sizeof(int), hipMemcpyDeviceToHost));
  if (e != 0) {
    timed_out = true;
    ++g_env_fallbacks;
  }
  return AQC_OK;
}

// The Z-sum chains (k_zenv): the split of launch_envs (env_split_cols / env_split_nw), or one
// workgroup per chain (single, or a capacity without a split); rounds of <= 224 workgroups so that
// a chain's workgroups are resident together.  cnt: 32 words per chain, zeroed by the caller.
int launch_zenv(const ZJob* dj, int nch, int cap, hipStream_t st, unsigned* cnt, int* err, bool single) {
  const bool one = single || g_env_single || env_split_cols(cap) == 0;
  const int nw = one ? 1 : env_split_nw(cap), cw = cap / nw;
  const int kRound = std::max(1, 224 / nw);
  const unsigned long long spin = g_env_spin;
  for (int c0 = 0; c0 < nch; c0 += kRound) {
    const int m = std::min(kRound, nch - c0);
    const dim3 g((m + 7) / 8 * 8, nw);  // (a chain's workgroups on one XCD, as launch_envs)
    const ZJob* jb = dj + c0;
    unsigned* cb = cnt + (size_t)c0 * 32;
    if (nw == 1) hipLaunchKernelGGL((k_zenv<64, 1>), g, dim3(kT), 0, st, jb, cb, err, spin, m, cw);
    else if (nw == 16) hipLaunchKernelGGL((k_zenv<64, 16>), g, dim3(kT), 0, st, jb, cb, err, spin, m, cw);
    else if (cw == 16) hipLaunchKernelGGL((k_zenv<32, kEnvNW>), g, dim3(kT), 0, st, jb, cb, err, spin, m, cw);
    else hipLaunchKernelGGL((k_zenv<64, kEnvNW>), g, dim3(kT), 0, st, jb, cb, err, spin, m, cw);
    AQC_CHECK_LAUNCH();
  }
  return AQC_OK;
}

}  // namespace

// The environment chains of aqc_mps_z_all_batch for one state, left in the per-device buffer for a
// caller in another translation unit (the MPS sampler): see mps_internal.h.
int aqc::mps_right_envs(aqc_mps_s* h, size_t extra_bytes, const cplx** renv, void** extra, hipStream_t* stream) {
  const int n = h->d.n, cap = h->d.cap;
  const size_t cc = (size_t)cap * cap;
  const size_t per_state = (2 * (size_t)(n + 1) * cc + 4 * cc) * sizeof(cplx);
  const size_t jb = aqc::up256(sizeof(RdmJob));
  hipStream_t st = aqc::mps_stream();
  aqc::DevScratch& rb = g_rbuf.here();
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  const size_t sb = env_sync_bytes(1);
  int rc = rb.ensure(jb + per_state + sb + extra_bytes + 1024);
  if (rc != AQC_OK) return rc;
  char* base = rb.dev;
  RdmJob* djobs = (RdmJob*)base;
  cplx* work = (cplx*)(base + jb);
  void* dsync = base + jb + per_state;
  RdmJob j;
  std::memset(&j, 0, sizeof(j));
  j.gam = h->d.gam;
  j.lam = h->d.lam;
  j.dims = h->d.dims;
  j.n = n;
  j.cap = cap;
  j.Lenv = work;
  j.Renv = work + (size_t)(n + 1) * cc;
  j.tmpL = j.Renv + (size_t)(n + 1) * cc;
  j.tmpR = j.tmpL + 2 * cc;
  AQC_HIP_CHECK(hipMemcpyAsync(djobs, &j, sizeof(RdmJob), hipMemcpyHostToDevice, st));
  const double c3 = (double)cap * cap * cap;
  for (int attempt = 0;; ++attempt) {  // attempt 1: the split chains timed out, single-workgroup chains
    aqc::KernelTimer::begin(st, "sample_env", 0.0, 2.0 * n * 4.0 * c3 * 8.0);
    rc = launch_envs(djobs, 1, cap, st, dsync, attempt > 0);
    aqc::KernelTimer::end(st);
    if (rc != AQC_OK) return rc;
    AQC_HIP_CHECK(hipStreamSynchronize(st));
    bool again = false;
    if (attempt == 0) {
      rc = env_timed_out(dsync, 1, cap, again);
      if (rc != AQC_OK) return rc;
    }
    if (!again) break;
  }
  *renv = j.Renv;
  *extra = base + jb + per_state + sb;
  *stream = st;
  return AQC_OK;
}

// The same chains for a batch of states of one n and capacity, handing out both sides (the Pauli
// chains of pauli.hip): see mps_internal.h.
int aqc::mps_envs_batch(aqc_mps_s** hs, int ns, size_t extra_bytes, const char* family, const cplx** lenv,
                        size_t* state_stride, void** extra, hipStream_t* stream) {
  const int n = hs[0]->d.n, cap = hs[0]->d.cap;
  const size_t cc = (size_t)cap * cap;
  const size_t per_state = (2 * (size_t)(n + 1) * cc + 4 * cc) * sizeof(cplx);
  const size_t jb = aqc::up256((size_t)ns * sizeof(RdmJob));
  hipStream_t st = aqc::mps_stream();
  aqc::DevScratch& rb = g_rbuf.here();
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  const size_t sb = env_sync_bytes(ns);
  int rc = rb.ensure(jb + (size_t)ns * per_state + sb + extra_bytes + 1024);
  if (rc != AQC_OK) return rc;
  char* base = rb.dev;
  RdmJob* djobs = (RdmJob*)base;
  cplx* work = (cplx*)(base + jb);
  void* dsync = base + jb + (size_t)ns * per_state;
  std::vector<RdmJob> jobs(ns);
  for (int s = 0; s < ns; ++s) {
    RdmJob& j = jobs[s];
    std::memset(&j, 0, sizeof(j));
    j.gam = hs[s]->d.gam;
    j.lam = hs[s]->d.lam;
    j.dims = hs[s]->d.dims;
    j.n = n;
    j.cap = cap;
    j.Lenv = work + (size_t)s * (per_state / sizeof(cplx));
    j.Renv = j.Lenv + (size_t)(n + 1) * cc;
    j.tmpL = j.Renv + (size_t)(n + 1) * cc;
    j.tmpR = j.tmpL + 2 * cc;
  }
  AQC_HIP_CHECK(hipMemcpyAsync(djobs, jobs.data(), (size_t)ns * sizeof(RdmJob), hipMemcpyHostToDevice, st));
  const double c3 = (double)cap * cap * cap;
  for (int attempt = 0;; ++attempt) {  // attempt 1: the split chains timed out, single-workgroup chains
    aqc::KernelTimer::begin(st, family, 0.0, ns * 2.0 * n * 4.0 * c3 * 8.0);
    rc = launch_envs(djobs, ns, cap, st, dsync, attempt > 0);
    aqc::KernelTimer::end(st);
    if (rc != AQC_OK) return rc;
    AQC_HIP_CHECK(hipStreamSynchronize(st));
    bool again = false;
    if (attempt == 0) {
      rc = env_timed_out(dsync, ns, cap, again);
      if (rc != AQC_OK) return rc;
    }
    if (!again) break;
  }
  *lenv = work;
  *state_stride = per_state / sizeof(cplx);
  *extra = base + jb + (size_t)ns * per_state + sb;
  *stream = st;
  return AQC_OK;
}

// What mps_envs_batch lays out per state (see mps_internal.h).
size_t aqc::env_state_bytes(int n, int cap) {
  const size_t cc = (size_t)cap * cap;
  return (2 * (size_t)(n + 1) * cc + 4 * cc) * sizeof(cplx);
}

// What aqc_mps_pair_rdms_batch lays out per state in the per-device buffer: both environment sides,
// the chains' scratch, P and U of every site, the chains of the `na` distinct lower qubits and the
// n x n table of 4x4 blocks (see mps_internal.h).
size_t aqc::pair_rdm_state_bytes(int n, int cap, int na) {
  const size_t cc = (size_t)cap * cap;
  return (2 * (size_t)(n + 1) * cc + 4 * cc + 6 * (size_t)n * cc + 12 * (size_t)na * cc + (size_t)n * n * 16) * sizeof(cplx);
}

extern "C" {

int aqc_mps_pair_rdms_batch(aqc_mps_t* hs, int ns, const int* pairs, int npairs, double* out, int out_is_device) {
  AQC_REQUIRE(hs && ns > 0 && pairs && out && npairs >= 0, "aqc_mps_pair_rdms_batch: bad arguments");
  const int n = hs[0]->d.n, cap = hs[0]->d.cap;
  for (int s = 0; s < ns; ++s)
    AQC_REQUIRE(hs[s] && hs[s]->d.n == n && hs[s]->d.cap == cap, "aqc_mps_pair_rdms_batch: all states need the same n and capacity");
  for (int p = 0; p < npairs; ++p) {
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    AQC_REQUIRE(a >= 0 && a < n && b >= 0 && b < n && a != b, "aqc_mps_pair_rdms_batch: bad pair");
  }
  if (npairs == 0) return AQC_OK;
  int rc = aqc_mps_sort_batch(hs, ns);  // qubits back in site order, as measurements do
  if (rc != AQC_OK) return rc;
  std::vector<int> alist;
  {
    std::vector<char> need(n, 0);
    for (int p = 0; p < npairs; ++p) need[std::min(pairs[2 * p], pairs[2 * p + 1])] = 1;
    for (int a = 0; a < n - 1; ++a)
      if (need[a]) alist.push_back(a);
  }
  const int na = (int)alist.size();
  const size_t cc = (size_t)cap * cap;
  const size_t per_state = aqc::pair_rdm_state_bytes(n, cap, na);
  const size_t jb = aqc::up256(ns * sizeof(RdmJob));
  const size_t pb = aqc::up256(2 * npairs * sizeof(int) + na * sizeof(int));
  const size_t ob = out_is_device ? 0 : (size_t)ns * npairs * 16 * sizeof(cplx);
  hipStream_t st = aqc::mps_stream();
  aqc::DevScratch& rb = g_rbuf.here();
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  const size_t sb = env_sync_bytes(ns);
  rc = rb.ensure(jb + pb + ob + ns * per_state + sb + 1024);
  if (rc != AQC_OK) return rc;
  char* base = rb.dev;
  RdmJob* djobs = (RdmJob*)base;
  void* dsync = base + jb + pb + ob + ns * per_state;
  int* dpairs = (int*)(base + jb);
  int* dalist = dpairs + 2 * npairs;
  cplx* dout = out_is_device ? (cplx*)out : (cplx*)(base + jb + pb);
  cplx* work = (cplx*)(base + jb + pb + ob);
  std::vector<RdmJob> jobs(ns);
  for (int s = 0; s < ns; ++s) {
    RdmJob& j = jobs[s];
    j.gam = hs[s]->d.gam;
    j.lam = hs[s]->d.lam;
    j.dims = hs[s]->d.dims;
    j.n = n;
    j.cap = cap;
    cplx* p = work + (size_t)s * (per_state / sizeof(cplx));
    j.Lenv = p;
    p += (size_t)(n + 1) * cc;
    j.Renv = p;
    p += (size_t)(n + 1) * cc;
    j.tmpL = p;
    p += 2 * cc;
    j.tmpR = p;
    p += 2 * cc;
    j.P = p;
    p += 3 * (size_t)n * cc;
    j.U = p;
    p += 3 * (size_t)n * cc;
    j.chain = p;
    p += 12 * (size_t)na * cc;
    j.rho = p;
  }
  AQC_HIP_CHECK(hipMemcpyAsync(djobs, jobs.data(), ns * sizeof(RdmJob), hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemcpyAsync(dpairs, pairs, 2 * npairs * sizeof(int), hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemcpyAsync(dalist, alist.data(), na * sizeof(int), hipMemcpyHostToDevice, st));
  const double c3 = (double)cap * cap * cap;
  double steps = 0.0;
  for (int a : alist) steps += (double)(n - 1 - a);
  for (int attempt = 0;; ++attempt) {  // attempt 1: the split chains timed out, single-workgroup chains
    aqc::KernelTimer::begin(st, "rdm_env", 0.0, ns * 2.0 * n * 4.0 * c3 * 8.0);
    rc = launch_envs(djobs, ns, cap, st, dsync, attempt > 0);
    aqc::KernelTimer::end(st);
    if (rc != AQC_OK) return rc;
    hipLaunchKernelGGL(k_rdm_P, dim3(n, 3, ns), dim3(kT), 0, st, djobs, 0);
    AQC_CHECK_LAUNCH();
    aqc::KernelTimer::begin(st, "rdm_chain", 0.0, ns * steps * 3.0 * 4.0 * c3 * 8.0);
    hipLaunchKernelGGL(k_rdm_chain, dim3(aqc::xcd_grid(3 * na, ns, true)), dim3(kT), 0, st, djobs, dalist, ns);
    aqc::KernelTimer::end(st);
    AQC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_rdm_gather, dim3((npairs * 16 + 255) / 256, ns), dim3(256), 0, st, djobs, dpairs, npairs, dout);
    AQC_CHECK_LAUNCH();
    if (!out_is_device)
      AQC_HIP_CHECK(hipMemcpyAsync(out, dout, (size_t)ns * npairs * 16 * sizeof(cplx), hipMemcpyDeviceToHost, st));
    AQC_HIP_CHECK(hipStreamSynchronize(st));
    bool again = false;
    if (attempt == 0) {
      rc = env_timed_out(dsync, ns, cap, again);
      if (rc != AQC_OK) return rc;
    }
    if (!again) return AQC_OK;
  }
}

int aqc_mps_z_all_batch(aqc_mps_t* hs, int ns, double* out) {
  AQC_REQUIRE(hs && ns >= 0 && (out || ns == 0), "aqc_mps_z_all_batch: bad arguments");
  if (ns == 0) return AQC_OK;
  const int n = hs[0]->d.n, cap = hs[0]->d.cap;
  for (int s = 0; s < ns; ++s)
    AQC_REQUIRE(hs[s] && hs[s]->d.n == n && hs[s]->d.cap == cap, "aqc_mps_z_all_batch: all states need the same n and capacity");
  int rc = aqc_mps_sort_batch(hs, ns);
  if (rc != AQC_OK) return rc;
  const size_t cc = (size_t)cap * cap;
  const size_t per_state = (2 * (size_t)(n + 1) * cc + 4 * cc + 6 * (size_t)n * cc) * sizeof(cplx);
  const size_t jb = aqc::up256(ns * sizeof(RdmJob));
  const size_t ob = aqc::up256((size_t)ns * n * sizeof(double));
  hipStream_t st = aqc::mps_stream();
  aqc::DevScratch& rb = g_rbuf.here();
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  const size_t sb = env_sync_bytes(ns);
  rc = rb.ensure(jb + ob + ns * per_state + sb + 1024);
  if (rc != AQC_OK) return rc;
  char* base = rb.dev;
  RdmJob* djobs = (RdmJob*)base;
  double* dout = (double*)(base + jb);
  void* dsync = base + jb + ob + ns * per_state;
  cplx* work = (cplx*)(base + jb + ob);
  std::vector<RdmJob> jobs(ns);
  for (int s = 0; s < ns; ++s) {
    RdmJob& j = jobs[s];
    std::memset(&j, 0, sizeof(j));
    j.gam = hs[s]->d.gam;
    j.lam = hs[s]->d.lam;
    j.dims = hs[s]->d.dims;
    j.n = n;
    j.cap = cap;
    cplx* p = work + (size_t)s * (per_state / sizeof(cplx));
    j.Lenv = p;
    p += (size_t)(n + 1) * cc;
    j.Renv = p;
    p += (size_t)(n + 1) * cc;
    j.tmpL = p;
    p += 2 * cc;
    j.tmpR = p;
    p += 2 * cc;
    j.P = p;
    p += 3 * (size_t)n * cc;
    j.U = p;
  }
  AQC_HIP_CHECK(hipMemcpyAsync(djobs, jobs.data(), ns * sizeof(RdmJob), hipMemcpyHostToDevice, st));
  const double c3 = (double)cap * cap * cap;
  for (int attempt = 0;; ++attempt) {  // attempt 1: the split chains timed out, single-workgroup chains
    aqc::KernelTimer::begin(st, "mps_zall", 0.0, ns * 2.0 * n * 4.0 * c3 * 8.0);
    rc = launch_envs(djobs, ns, cap, st, dsync, attempt > 0);
    if (rc != AQC_OK) return rc;
    hipLaunchKernelGGL(k_rdm_P, dim3(n, 2, ns), dim3(kT), 0, st, djobs, 1);
    AQC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_rdm_ztrace, dim3(n, ns), dim3(kT), 0, st, djobs, dout);
    aqc::KernelTimer::end(st);
    AQC_CHECK_LAUNCH();
    AQC_HIP_CHECK(hipMemcpyAsync(out, dout, (size_t)ns * n * sizeof(double), hipMemcpyDeviceToHost, st));
    AQC_HIP_CHECK(hipStreamSynchronize(st));
    bool again = false;
    if (attempt == 0) {
      rc = env_timed_out(dsync, ns, cap, again);
      if (rc != AQC_OK) return rc;
    }
    if (!again) return AQC_OK;
  }
}

/* sum_i <Z_i> of every state hs[s] (sorted first, as aqc_mps_z_all_batch does): a state copied
   from `base` (aqc_mps_copy / aqc_mps_copy_batch) while base has not changed since takes base's
   cached environment pairs outside the sites it has rewritten and runs its own chain through those
   only; any other state runs aqc_mps_z_all_batch and sums.  base is not modified (its cache is
   extended). */
int aqc_mps_z_sum_batch(aqc_mps_t base, aqc_mps_t* hs, int ns, double* out) {
  AQC_REQUIRE(base && hs && ns >= 0 && (out || ns == 0), "aqc_mps_z_sum_batch: bad arguments");
  if (ns == 0) return AQC_OK;
  const int n = base->d.n, cap = base->d.cap;
  for (int s = 0; s < ns; ++s)
    AQC_REQUIRE(hs[s] && hs[s] != base && hs[s]->d.n == n && hs[s]->d.cap == cap,
                "aqc_mps_z_sum_batch: every state needs base's n and capacity (and is not base)");
  int rc = aqc_mps_sort_batch(hs, ns);
  if (rc != AQC_OK) return rc;
  // windows: the sites each state rewrote since its copy from base (empty: site 0, any bond works)
  std::vector<int> win, lo(ns, -1), hi(ns, -1), fb;
  int need_l = 0, need_r = n;
  for (int s = 0; s < ns; ++s) {
    const aqc_mps_s* h = hs[s];
    if (h->synced_src != base->uid || h->synced_ver != base->version) {
      fb.push_back(s);
      continue;
    }
    lo[s] = h->dirty_hi >= h->dirty_lo ? h->dirty_lo : 0;
    hi[s] = h->dirty_hi >= h->dirty_lo ? h->dirty_hi : 0;
    need_l = std::max(need_l, lo[s]);
    need_r = std::min(need_r, hi[s] + 1);
    win.push_back(s);
  }
  const size_t cc = (size_t)cap * cap, pair = 2 * cc;
  hipStream_t st = aqc::mps_stream();
  if (!win.empty()) {
    if (!base->zenv) {
      base->zenv = (cplx*)aqc::dev_alloc(2 * (size_t)(n + 1) * pair * sizeof(cplx));
      AQC_REQUIRE(base->zenv, "aqc_mps_z_sum_batch: out of device memory");
      AQC_HIP_CHECK(hipMemsetAsync(base->zenv, 0, 2 * (size_t)(n + 1) * pair * sizeof(cplx), st));
      hipLaunchKernelGGL(k_zenv_init, dim3(1), dim3(64), 0, st, base->zenv, base->zenv + (size_t)(n + 1) * pair + (size_t)n * pair);
      AQC_CHECK_LAUNCH();
      base->zl = 0;
      base->zr = n;
    }
    cplx* ZL = base->zenv;
    cplx* ZR = base->zenv + (size_t)(n + 1) * pair;
    std::vector<ZJob> jobs;
    auto job = [&](aqc_mps_t h, int dir, int first, int nsteps, const cplx* ein, cplx* eout) {
      ZJob j;
      j.gam = h->d.gam;
      j.lam = h->d.lam;
      j.dims = h->d.dims;
      j.cap = cap;
      j.dir = dir;
      j.first = first;
      j.nsteps = nsteps;
      j.ein = ein;
      j.eout = eout;
      j.tmp = nullptr;
      jobs.push_back(j);
    };
    // launch 1: extend base's cache (left pairs to bond need_l, right pairs down to need_r)
    const int zl = base->zl, zr = base->zr;
    if (need_l > zl) job(base, 0, zl, need_l - zl, ZL + (size_t)zl * pair, ZL + (size_t)(zl + 1) * pair);
    if (need_r < zr) job(base, 1, zr - 1, zr - need_r, ZR + (size_t)zr * pair, ZR + (size_t)(zr - 1) * pair);
    const int nbase = (int)jobs.size();
    // launch 2: each state's window from both ends -- a left chain from base's pair at bond lo
    // through the first half, a right chain from base's pair at bond hi + 1 through the rest --
    // meeting at bond lo + nl
    size_t wsteps = 0;
    int nwin_ch = 0;
    for (int s : win) {
      const int w = hi[s] - lo[s] + 1, nl = (w + 1) / 2;
      wsteps += (size_t)w;
      nwin_ch += 1 + (w > nl ? 1 : 0);
    }
    const int nch = nbase + nwin_ch;
    const size_t jb = aqc::up256(nch * sizeof(ZJob));
    const size_t zb = aqc::up256(win.size() * sizeof(ZSumJob));
    const size_t ob = aqc::up256(win.size() * sizeof(double));
    const size_t sb = aqc::up256(((size_t)nch * 32 + 32) * sizeof(unsigned));
    const size_t tb = (size_t)nch * 4 * cc * sizeof(cplx);
    const size_t wb = wsteps * pair * sizeof(cplx);
    aqc::DevScratch& rb = g_rbuf.here();
    AQC_HIP_CHECK(hipStreamSynchronize(st));
    rc = rb.ensure(jb + zb + ob + sb + tb + wb + 1024);
    if (rc != AQC_OK) return rc;
    char* b = rb.dev;
    ZJob* dj = (ZJob*)b;
    ZSumJob* dz = (ZSumJob*)(b + jb);
    double* dout = (double*)(b + jb + zb);
    unsigned* cnt = (unsigned*)(b + jb + zb + ob);
    int* err = (int*)(cnt + (size_t)nch * 32);
    cplx* tmp = (cplx*)(b + jb + zb + ob + sb);
    cplx* wbuf = tmp + (size_t)nch * 4 * cc;
    std::vector<ZSumJob> sums;
    size_t woff = 0;
    for (int s : win) {
      const int w = hi[s] - lo[s] + 1, nl = (w + 1) / 2, ny = w - nl;
      cplx* el = wbuf + woff * pair;
      job(hs[s], 0, lo[s], nl, ZL + (size_t)lo[s] * pair, el);
      woff += (size_t)nl;
      ZSumJob z;
      z.lp = el + (size_t)(nl - 1) * pair;
      z.rp = ZR + (size_t)(hi[s] + 1) * pair;
      if (ny > 0) {  // (right chains store downwards: step k at er + (ny - 1 - k) pair)
        cplx* er = wbuf + woff * pair;
        job(hs[s], 1, hi[s], ny, ZR + (size_t)(hi[s] + 1) * pair, er + (size_t)(ny - 1) * pair);
        woff += (size_t)ny;
        z.rp = er;
      }
      z.dims = hs[s]->d.dims;
      z.bond = lo[s] + nl;
      z.cap = cap;
      sums.push_back(z);
    }
    for (int c = 0; c < nch; ++c) jobs[c].tmp = tmp + (size_t)c * 4 * cc;
    AQC_HIP_CHECK(hipMemcpyAsync(dj, jobs.data(), nch * sizeof(ZJob), hipMemcpyHostToDevice, st));
    AQC_HIP_CHECK(hipMemcpyAsync(dz, sums.data(), sums.size() * sizeof(ZSumJob), hipMemcpyHostToDevice, st));
    std::vector<double> res(win.size());
    for (int attempt = 0;; ++attempt) {  // attempt 1: a hand-off timed out, single-workgroup chains
      AQC_HIP_CHECK(hipMemsetAsync(cnt, 0, sb, st));
      aqc::KernelTimer::begin(st, "mps_zsum", 0.0, (double)(wsteps + (size_t)(need_l > zl ? need_l - zl : 0) + (size_t)(need_r < zr ? zr - need_r : 0)) * 2.0 * 8.0 * 4.0 * (double)cc * cap);
      if (nbase) {
        rc = launch_zenv(dj, nbase, cap, st, cnt, err, attempt > 0);
        if (rc != AQC_OK) return rc;
      }
      rc = launch_zenv(dj + nbase, nwin_ch, cap, st, cnt + (size_t)nbase * 32, err, attempt > 0);
      if (rc != AQC_OK) return rc;
      hipLaunchKernelGGL(k_zsum, dim3((unsigned)win.size()), dim3(kT), 0, st, dz, dout);
      aqc::KernelTimer::end(st);
      AQC_CHECK_LAUNCH();
      AQC_HIP_CHECK(hipMemcpyAsync(res.data(), dout, res.size() * sizeof(double), hipMemcpyDeviceToHost, st));
      AQC_HIP_CHECK(hipStreamSynchronize(st));
      int e = 0;
      AQC_HIP_CHECK(hipMemcpy(&e, err, sizeof(int), hipMemcpyDeviceToHost));
      if (e == 0) break;
      AQC_REQUIRE(attempt == 0, "aqc_mps_z_sum_batch: single-workgroup chains timed out");
      ++g_env_fallbacks;
    }
    base->zl = std::max(zl, need_l);
    base->zr = std::min(zr, need_r);
    for (size_t k = 0; k < win.size(); ++k) out[win[k]] = res[k];
  }
  if (!fb.empty()) {  // states not copied from base (or base changed since): the full chains
    std::vector<aqc_mps_t> fh;
    for (int s : fb) fh.push_back(hs[s]);
    std::vector<double> z((size_t)fb.size() * n);
    rc = aqc_mps_z_all_batch(fh.data(), (int)fh.size(), z.data());
    if (rc != AQC_OK) return rc;
    for (size_t k = 0; k < fb.size(); ++k) {
      double t = 0.0;
      for (int q = 0; q < n; ++q) t += z[k * n + q];
      out[fb[k]] = t;
    }
  }
  return AQC_OK;
}

/* Environment launches whose split chains timed out on a hand-off and were re-run with
   single-workgroup chains since the last call (then reset). */
int aqc_env_fallbacks(long long* out) {
  AQC_REQUIRE(out, "aqc_env_fallbacks: null argument");
  *out = (long long)g_env_fallbacks;
  g_env_fallbacks = 0;
  return AQC_OK;
}

/* Force single-workgroup environment chains (1) or the default per-capacity choice (0): the tests'
   reference for the split kernels. */
int aqc_env_set_single(int on) {
  AQC_REQUIRE(on == 0 || on == 1, "aqc_env_set_single: on must be 0 or 1");
  g_env_single = on;
  return AQC_OK;
}

/* Hand-off wait limit of the split environment chains in microseconds (< 0: the default, 2 s).
   0 makes any wait not already satisfied a timeout: the tests use it to exercise the re-run. */
int aqc_env_set_spin_limit(double us) {
  g_env_spin = us < 0 ? kEnvSpin : (unsigned long long)(us * 100.0);
  return AQC_OK;
}

int aqc_env_ticks(double* out) {
  AQC_REQUIRE(out, "aqc_env_ticks: null argument");
  unsigned long long t[4];
  AQC_HIP_CHECK(hipMemcpyFromSymbol(t, HIP_SYMBOL(g_env_ticks), sizeof(t)));
  for (int i = 0; i < 4; ++i) out[i] = (double)t[i];
  unsigned long long z[4] = {0, 0, 0, 0};
  AQC_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_env_ticks), z, sizeof(z)));
  return AQC_OK;
}

int aqc_mps_pair_rdms(aqc_mps_t h, const int* pairs, int npairs, double* out) {
  return aqc_mps_pair_rdms_batch(&h, 1, pairs, npairs, out, 0);
}

int aqc_entanglement_measures(const double* rdms, int count, int method, double* out, int on_device) {
  AQC_REQUIRE(rdms && out && count >= 0, "aqc_entanglement_measures: bad arguments");
  AQC_REQUIRE(method >= 0 && method <= 3, "aqc_entanglement_measures: method must be 0..3");
  if (count == 0) return AQC_OK;
  hipStream_t st = aqc::mps_stream();
  const cplx* drdm = (const cplx*)rdms;
  double* dout = out;
  void* tmp = nullptr;
  if (!on_device) {
    AQC_HIP_CHECK(hipMalloc(&tmp, (size_t)count * (16 * sizeof(cplx) + sizeof(double))));
    AQC_HIP_CHECK(hipMemcpyAsync(tmp, rdms, (size_t)count * 16 * sizeof(cplx), hipMemcpyHostToDevice, st));
    drdm = (const cplx*)tmp;
    dout = (double*)((char*)tmp + (size_t)count * 16 * sizeof(cplx));
  }
  hipLaunchKernelGGL(k_ent_measure, dim3((count + 63) / 64), dim3(64), 0, st, drdm, count, method, dout);
  AQC_CHECK_LAUNCH();
  if (!on_device) AQC_HIP_CHECK(hipMemcpyAsync(out, dout, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  if (tmp) hipFree(tmp);
  return AQC_OK;
}

}  // extern "C"
