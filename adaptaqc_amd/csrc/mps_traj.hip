// Noisy shot sampling on the MPS engine: quantum trajectories above the statevector's 24 qubits, what
// Aer's qasm_simulator does with method="matrix_product_state" under a NoiseModel.
//
// A shot is one trajectory of aqc_sv_traj_sample's program (traj.hip) on a Vidal MPS: the gate rows
// run as the engine's two-site updates (swap-left routing, run_waves in mps.hip), a Kraus row draws
// one operator of a one-qubit channel and applies it to the site, and the final measurement draws
// the qubits one by one.  A Kraus operator is not unitary, so it breaks the canonical form at every
// bond, and the one-site formula for the qubit's reduced density matrix,
//   rho[s][s'] = sum_{l,r} lambda_p[l]^2 lambda_{p+1}[r]^2 Gamma_p^s[l][r] conj(Gamma_p^s'[l][r]),
// holds only at the orthogonality centre.  The schedule therefore tracks the centre on the host, by
// two integers that depend on the program alone: every site < a is left-orthonormal (sum_s (lambda_j
// Gamma_j^s)^H (lambda_j Gamma_j^s) = I), every site > b right-orthonormal (sum_s (Gamma_j^s
// lambda_{j+1}) (Gamma_j^s lambda_{j+1})^H = I); canonical: a = n, b = -1.
//   two-site update on (p, p+1)   needs a >= p and b <= p+1 (theta's environments are identities, so
//                                 the SVD is the Schmidt decomposition and the truncation Aer's);
//                                 then a = a >= p+2 ? a : p+1 and b = b <= p-1 ? b : p
//   Kraus / measurement row on p  needs a >= p and b <= p; then a = b = p
//   general group on (p, p+1)     needs what a two-site update needs; then a = p + 1, b = p (the operator
//                                 is not unitary, so no site beyond the two keeps its property)
//   product-unitary group         one-site unitaries on two sites: needs nothing, changes nothing
//   centre moves                  identity-gate two-site updates: on (a, a+1) while a < p, on
//                                 (b-1, b) while b > the row's right site (b <= a always, so both
//                                 are legal)
// One-qubit unitaries keep both properties and stay deferred; a Kraus row on a qubit with a pending
// gate P absorbs it (K_k <- K_k P).  The final measurement: flush, sort, then for q = 0 .. n-1 a
// measurement row {|0><0|, |1><1|} on site q, each behind the centre move that brings it there.
//
// k_mps_kraus1: one 256-thread workgroup per (state, row).  Pass 1 strides over the site's
// dims[p] x dims[p+1] block for rho00, rho11, rho01, reduced in a fixed order (wave butterfly, then
// the four waves in index order through the LDS; no atomics: two calls return the same bits).
// p_k = Re Tr(K_k^dag K_k rho) and the choice follow aqc_sv_traj_sample's rule, a measurement row
// aqc_mps_sample's bit = [u (p0 + p1) >= p0].  Pass 2: Gamma^s <- sum_s' K_k[s][s'] / sqrt(p_k) Gamma^s'.
//
// Noisy pair tomography (aqc_mps_traj_pair_tomo): the same schedule without the measurement sweep
// (gate rows, Kraus rows at the centre, the flush and the sort), 9 nshots trajectories, trajectory t
// serving Pauli setting t % 9 of every pair.  A batch's states are then read out by the all-pair RDM
// sweep that assumes no canonical form (aqc_mps_pair_rdms_batch, ent.hip, into device memory), and
// k_mps_traj_pair_draw -- one thread per (state, pair) -- forms the four outcome probabilities from
// the RDM and the two qubits' POVM effects with the arithmetic of k_sv_traj's pair ending
// (pair_draw.h), draws one outcome and adds it to the integer count table on the device.
//
// The noisy Pauli readout (aqc_mps_traj_pauli_counts): the pair readout's schedule, nshots trajectories,
// every trajectory serving every term.  A noisy readout turns a term's letter on qubit q into the
// Hermitian 2x2 factor D_q = E+ - E- (an identity part beside the Pauli one), so the chain of pauli.hip
// is restated for a general factor per site: with A_i^s = Gamma_i^s lambda_{i+1} and the identity
// environments L_b, R_b of ent.hip's chains (no canonical form assumed), a term with support lo..hi is
//   E = L_lo;  for i = lo..hi:  E'[b'][k'] = sum_{s,t} D_i[s][t] conj(A_s[b][b']) E[b][k] A_t[k][k'];
//   v = Re sum E[b][k] R_{hi+1}[k][b].
// k_mps_traj_pauli_chain gives each (term, state) item to one 256-thread workgroup that needs nothing
// from any other (no counters, no hand-offs: nothing in it can wait) and walks the items wg, wg + grid,
// ...; a site is two aqc::block_cgemm products on the FP64 matrix cores, T = E [A_0 | A_1] (chi_l x
// 2 chi_r, contraction chi_l) and E' = sum_{(t,b)} (sum_s D[s][t] conj(A_s[b][b'])) T_t[b][k'] (chi_r x
// chi_r, contraction 2 chi_l): 4 chi^3 complex multiply-adds (32 chi^3 flops); E and both slices of Gamma
// read and T written by the first product, both slices per (t, b) and T read and E' written by the
// second (12 chi^2 complex of traffic, 2 chi^2 more than a Pauli letter's one slice per t), whatever D
// is -- a general factor costs the same at any number per term.  E and T
// (3 cap^2 complex) are the workgroup's slice of a bounded workspace.  One more item per state, the
// all-identity term on site 0, gives w = <psi|psi>.  k_mps_traj_pauli_draw -- one thread per (state,
// term) -- draws the parity from (v, w) and adds to the 64-bit table on the device.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "aqc_gemm.h"
#include "kraus_group.h"
#include "mps_internal.h"
#include "pair_draw.h"
#include "sample_rng.h"

using aqc::cplx;
using aqc::DevOp;
using aqc::KrausJob;
using aqc::Kraus2Group;
using aqc::Kraus2Job;
using aqc::Kraus2ProdJob;
using aqc::TwoSiteJob;
using aqc::TrajCtx;

namespace {

constexpr int kKT = 256;
constexpr int kMaxShots = 1 << 30;
constexpr int kMaxBatch = 256;
constexpr int kMaxPairs = 4096;
constexpr int kDT = 256;  // threads of k_mps_traj_pair_draw
constexpr int kReadoutStates = 16;  // states per RDM sweep of the pair readout
// device memory the batch's MPS handles may take together (each: the Gammas, n 2 cap^2 complex, and
// one two-site workspace per concurrent update of the widest wave)
constexpr size_t kBatchBudgetBytes = (size_t)4 << 30;
constexpr int kChunkRows = 64;  // schedule rows per run_waves call (bounds the job staging)
int g_forced_batch = 0;
int g_forced_readout = 0;  // aqc_mps_traj_set_readout_batch: states per sweep of the pair / Pauli readout
// aqc_mps_traj_set_correlated: 0 refuses correlated groups, 1 runs them, 2 runs every one as a general group
int g_correlated = 0;
constexpr int kK2T = 256;        // threads of the k_mps_kraus2_* kernels (but the one-wave pick)
constexpr int kRhoSlice = 1024;  // (l, r) positions of theta per workgroup of k_mps_kraus2_rho
constexpr int kApplyMaxBlocks = 64;
constexpr int kMaxTerms = 65536;
constexpr int kCT = 256;  // threads of k_mps_traj_pauli_chain
constexpr size_t kChainWsBytes = (size_t)512 << 20;  // bound of the chain kernel's E / T workspace
constexpr int kChainMaxWg = 2048;                    // and of its grid (8 workgroups a CU)
constexpr int kPauliReadoutStates = 128;             // states per sweep of the Pauli readout

__device__ __forceinline__ double wave_sum(double v) {
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ __launch_bounds__(kKT) void k_mps_kraus1(const KrausJob* __restrict__ jobs, const TrajCtx c) {
  __shared__ double red[kKT / 64][4];
  const KrausJob& j = jobs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cap = j.cap;
  const int cl = min(j.dims[0], cap), cr = min(j.dims[1], cap);
  const size_t half = (size_t)cap * cap;
  double r00 = 0.0, r11 = 0.0, rx = 0.0, ry = 0.0;  // rho01 = sum w a0 conj(a1)
  for (int e = tid; e < cl * cr; e += kKT) {
    const int l = e / cr, r = e - l * cr;
    const double wl = aqc::ldg(j.ll + l), wr = aqc::ldg(j.lr + r);
    const double w = (wl * wl) * (wr * wr);
    const size_t o = (size_t)l * cap + r;
    const cplx a0 = aqc::ldg(j.g + o), a1 = aqc::ldg(j.g + half + o);
    r00 = fma(w, aqc::cnorm2(a0), r00);
    r11 = fma(w, aqc::cnorm2(a1), r11);
    const cplx x = aqc::cmulc(a0, a1);
    rx = fma(w, x.x, rx);
    ry = fma(w, x.y, ry);
  }
  r00 = wave_sum(r00);
  r11 = wave_sum(r11);
  rx = wave_sum(rx);
  ry = wave_sum(ry);
  if (lane == 0) {
    red[wave][0] = r00;
    red[wave][1] = r11;
    red[wave][2] = rx;
    red[wave][3] = ry;
  }
  __syncthreads();
  // every thread takes the same sums in the same order, so all choose the same k
  r00 = r11 = rx = ry = 0.0;
  for (int w = 0; w < kKT / 64; ++w) {
    r00 += red[w][0];
    r11 += red[w][1];
    rx += red[w][2];
    ry += red[w][3];
  }
  const int local = j.shot - c.shot0;
  const int idx = j.meas ? c.nev + j.slot : j.slot;
  const double u = c.u ? aqc::ldg(c.u + (size_t)local * c.nper + idx)
                       : aqc::sample_uniform(c.seed, c.run, (uint64_t)j.shot, (uint32_t)idx);
  const int nk = j.nk;
  double pk[4], P = 0.0;
  for (int k = 0; k < 4; ++k) {
    pk[k] = 0.0;
    if (k < nk) {
      const double* w = j.w + 4 * k;
      pk[k] = fmax(0.0, w[0] * r00 + w[1] * r11 + 2.0 * (w[2] * rx + w[3] * ry));
      P += pk[k];
    }
  }
  const double target = u * P;
  int k = -1;
  if (j.meas) {
    k = target >= pk[0] ? 1 : 0;
  } else {
    int lastnz = 0;
    double cs = 0.0;
    for (int q = 0; q < 4; ++q) {
      if (q >= nk) break;
      cs += pk[q];
      if (pk[q] > 0.0) lastnz = q;
      if (k < 0 && cs > target) k = q;
    }
    if (k < 0) k = lastnz;
  }
  double psel = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (q == k) psel = pk[q];
  const double sc = psel > 0.0 ? 1.0 / sqrt(psel) : 0.0;
  const cplx* m = j.K + 4 * k;
  const cplx m00 = aqc::cscale(m[0], sc), m01 = aqc::cscale(m[1], sc);
  const cplx m10 = aqc::cscale(m[2], sc), m11 = aqc::cscale(m[3], sc);
  for (int e = tid; e < cl * cr; e += kKT) {
    const int l = e / cr, r = e - l * cr;
    const size_t o = (size_t)l * cap + r;
    const cplx a0 = aqc::ldg(j.g + o), a1 = aqc::ldg(j.g + half + o);
    aqc::stg(j.g + o, aqc::cfma(m01, a1, aqc::cmul(m00, a0)));
    aqc::stg(j.g + half + o, aqc::cfma(m11, a1, aqc::cmul(m10, a0)));
  }
  if (tid == 0) {
    if (j.meas) {
      // one state's rows are serial, so this workgroup alone touches the word now
      uint64_t* word = c.out + (size_t)local * c.words + (j.slot >> 6);
      if (k) *word = *word | ((uint64_t)1 << (j.slot & 63));
    } else if (c.choices) {
      c.choices[(size_t)local * c.nev + j.slot] = (uint8_t)k;
    }
  }
}

// ---- correlated two-qubit groups -------------------------------------------------------------
// A general group event acts on the theta of its two adjacent sites, formed by k_theta with G = I:
// theta_o[l][r] at theta[(s2 chr + r) M + s1 chl + l], o = 2 s1 + s2, M = 2 chl, carrying all three
// lambdas.  With the centre condition rho_{oo'} = sum_{l,r} theta_o[l][r] conj(theta_o'[l][r]).
__device__ __forceinline__ void theta_shape(const TwoSiteJob& j, int& chl, int& chr) {
  chl = min(j.dims[0], j.cap);
  chr = min(j.dims[2], j.cap);
}

__device__ __forceinline__ size_t theta_at(int o, int l, int r, int chl, int chr) {
  return (size_t)((o & 1) * chr + r) * (size_t)(2 * chl) + (size_t)((o >> 1) * chl + l);
}

// rho in slices of kRhoSlice positions: grid (slices, jobs).  Each workgroup adds its positions' 16
// reals (rho_ss, then (Re, Im) of rho_st for s < t in the order 01 02 03 12 13 23) in a fixed order --
// thread stride, wave butterfly, the waves in index order through the LDS -- and writes them to
// partial[job][slice]; a slice past theta's end writes zeros.  No atomics.  A flat group (constant
// weights) needs no rho: its workgroups return at once.
__global__ __launch_bounds__(kK2T) void k_mps_kraus2_rho(const TwoSiteJob* __restrict__ two,
                                                         const Kraus2Job* __restrict__ jobs, const TrajCtx c) {
  __shared__ double red[kK2T / 64][16];
  const Kraus2Job& e = jobs[blockIdx.y];
  if (c.groups[e.grp].flat) return;
  const TwoSiteJob& j = two[e.two];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int chl, chr;
  theta_shape(j, chl, chr);
  const int npos = chl * chr, pos0 = (int)blockIdx.x * kRhoSlice;
  double d[4] = {0.0, 0.0, 0.0, 0.0};  // rho_ss; rho_st = sum a_s conj(a_t), s < t
  double ox[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, oy[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int q = tid; q < kRhoSlice; q += kK2T) {
    const int pos = pos0 + q;
    if (pos >= npos) break;
    const int l = pos % chl, r = pos / chl;  // (l runs along theta's columns: consecutive addresses)
    cplx a[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) a[o] = aqc::ldg(j.theta + theta_at(o, l, r, chl, chr));
    int k = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      d[s] += aqc::cnorm2(a[s]);
#pragma unroll
      for (int t = s + 1; t < 4; ++t, ++k) {
        const cplx z = aqc::cmulc(a[s], a[t]);
        ox[k] += z.x;
        oy[k] += z.y;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) d[s] = wave_sum(d[s]);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    ox[k] = wave_sum(ox[k]);
    oy[k] = wave_sum(oy[k]);
  }
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < 4; ++s) red[wave][s] = d[s];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      red[wave][4 + 2 * k] = ox[k];
      red[wave][5 + 2 * k] = oy[k];
    }
  }
  __syncthreads();
  if (tid < 16) {
    double x = 0.0;
    for (int w = 0; w < kK2T / 64; ++w) x += red[w][tid];
    aqc::stg(c.k2_part + ((size_t)blockIdx.y * c.k2_slices + blockIdx.x) * 16 + tid, x);
  }
}

// The smallest k with C_k > u P, else the last k with p_k > 0 (aqc_sv_traj_sample's rule), from the nk
// clamped weights in pk: every thread that calls it takes the same sums in the same order.
__device__ __forceinline__ int kraus2_choose(const double* pk, int nk, double u, double& psel) {
  double P = 0.0;
  for (int q = 0; q < nk; ++q) P += pk[q];
  const double target = u * P;
  int k = -1, lastnz = 0;
  double cs = 0.0;
  for (int q = 0; q < nk; ++q) {
    const double pq = pk[q];
    cs += pq;
    if (pq > 0.0) lastnz = q;
    if (k < 0 && cs > target) k = q;
  }
  if (k < 0) k = lastnz;
  psel = pk[k];
  return k;
}

__device__ __forceinline__ double event_uniform(const TrajCtx& c, int shot, int slot) {
  return c.u ? aqc::ldg(c.u + (size_t)(shot - c.shot0) * c.nper + slot)
             : aqc::sample_uniform(c.seed, c.run, (uint64_t)shot, (uint32_t)slot);
}

// One wave per job: the slices summed in index order, p_k = max(0, sum W_k rho) (a flat group: its
// constant), the choice, the choice byte, and K_k / sqrt(p_k) into the job's slot.
__global__ __launch_bounds__(64) void k_mps_kraus2_pick(const Kraus2Job* __restrict__ jobs, const TrajCtx c) {
  __shared__ double rho[16], pkl[16];
  const Kraus2Job& e = jobs[blockIdx.x];
  const Kraus2Group& g = c.groups[e.grp];
  const int tid = threadIdx.x, nk = g.nk, flat = g.flat;
  if (!flat && tid < 16) {
    const double* part = c.k2_part + (size_t)blockIdx.x * c.k2_slices * 16 + tid;
    double x = 0.0;
    for (int s = 0; s < c.k2_slices; ++s) x += aqc::ldg(part + (size_t)s * 16);
    rho[tid] = x;
  }
  __syncthreads();
  if (tid < nk) {
    const double* w = g.W[tid];
    double p = aqc::ldg(w);
    if (!flat) {
      p = p * rho[0] + aqc::ldg(w + 1) * rho[1] + aqc::ldg(w + 2) * rho[2] + aqc::ldg(w + 3) * rho[3];
      double o = 0.0;
      for (int q = 4; q < 16; ++q) o += aqc::ldg(w + q) * rho[q];
      p += 2.0 * o;
    }
    pkl[tid] = fmax(0.0, p);
  }
  __syncthreads();
  double psel;
  const int k = kraus2_choose(pkl, nk, event_uniform(c, e.shot, e.slot), psel);
  const double sc = psel > 0.0 ? 1.0 / sqrt(psel) : 0.0;
  if (tid == 0 && c.choices) c.choices[(size_t)(e.shot - c.shot0) * c.nev + e.slot] = (uint8_t)k;
  if (tid < 16) aqc::stg(c.k2_sel + (size_t)blockIdx.x * 16 + tid, aqc::cscale(aqc::ldg(&g.K[k][tid]), sc));
}

// theta'_o = sum_i K[o][i] theta_i in place: grid (blocks, jobs), a position's four entries read and
// written by one thread, so no position waits for another.
__global__ __launch_bounds__(kK2T) void k_mps_kraus2_apply(const TwoSiteJob* __restrict__ two,
                                                           const Kraus2Job* __restrict__ jobs, const TrajCtx c) {
  __shared__ cplx m[16];
  const TwoSiteJob& j = two[jobs[blockIdx.y].two];
  if (threadIdx.x < 16) m[threadIdx.x] = aqc::ldg(c.k2_sel + (size_t)blockIdx.y * 16 + threadIdx.x);
  __syncthreads();
  int chl, chr;
  theta_shape(j, chl, chr);
  const int npos = chl * chr;
  for (int pos = (int)blockIdx.x * kK2T + (int)threadIdx.x; pos < npos; pos += (int)gridDim.x * kK2T) {
    const int l = pos % chl, r = pos / chl;
    cplx v[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) v[o] = aqc::ldg(j.theta + theta_at(o, l, r, chl, chr));
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      cplx acc = aqc::cmul(m[4 * o], v[0]);
      acc = aqc::cfma(m[4 * o + 1], v[1], acc);
      acc = aqc::cfma(m[4 * o + 2], v[2], acc);
      acc = aqc::cfma(m[4 * o + 3], v[3], acc);
      aqc::stg(j.theta + theta_at(o, l, r, chl, chr), acc);
    }
  }
}

// A product-unitary group's event: grid (blocks, jobs).  The weights are the table's constants, so every
// workgroup of a job takes the same k from the same arithmetic; then the chosen 2x2 unitary of each of
// the two sites on that site's Gamma (pass 2 of k_mps_kraus1, twice).  Workgroup 0 writes the choice.
__global__ __launch_bounds__(kK2T) void k_mps_kraus2_prod(const Kraus2ProdJob* __restrict__ jobs, const TrajCtx c) {
  const Kraus2ProdJob& j = jobs[blockIdx.y];
  const Kraus2Group& g = c.groups[j.grp];
  const int nk = g.nk;
  double pk[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) pk[q] = q < nk ? fmax(0.0, aqc::ldg(&g.W[q][0])) : 0.0;
  double P = 0.0;
#pragma unroll
  for (int q = 0; q < 16; ++q)
    if (q < nk) P += pk[q];
  const double target = event_uniform(c, j.shot, j.slot) * P;
  int k = -1, lastnz = 0;
  double cs = 0.0;
#pragma unroll
  for (int q = 0; q < 16; ++q)
    if (q < nk) {
      cs += pk[q];
      if (pk[q] > 0.0) lastnz = q;
      if (k < 0 && cs > target) k = q;
    }
  if (k < 0) k = lastnz;
  const int cap = j.cap;
  const size_t half = (size_t)cap * cap;
  const int stride = (int)gridDim.x * kK2T, first = (int)blockIdx.x * kK2T + (int)threadIdx.x;
#pragma unroll
  for (int site = 0; site < 2; ++site) {
    const int* dims = site ? j.dims1 : j.dims0;
    cplx* gam = site ? j.g1 : j.g0;
    const cplx* m = &g.K[k][4 * site];
    const cplx m00 = aqc::ldg(m), m01 = aqc::ldg(m + 1), m10 = aqc::ldg(m + 2), m11 = aqc::ldg(m + 3);
    const int cl = min(dims[0], cap), cr = min(dims[1], cap);
    for (int e = first; e < cl * cr; e += stride) {
      const int l = e / cr, r = e - l * cr;
      const size_t o = (size_t)l * cap + r;
      const cplx a0 = aqc::ldg(gam + o), a1 = aqc::ldg(gam + half + o);
      aqc::stg(gam + o, aqc::cfma(m01, a1, aqc::cmul(m00, a0)));
      aqc::stg(gam + half + o, aqc::cfma(m11, a1, aqc::cmul(m10, a0)));
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && c.choices)
    c.choices[(size_t)(j.shot - c.shot0) * c.nev + j.slot] = (uint8_t)k;
}

// The pair readout of nr states of a batch: state s of the sweep is trajectory traj0 + s, state
// local0 + s of the batch (the batch's uniforms and outcome bytes are indexed by that).
struct PairDrawJob {
  const cplx* rdm;             // [nr][npairs][16], row-major 4x4, index 2 bit_hi + bit_lo
  const int* pairs;            // 2 npairs
  const double* effects;       // [n][3][2][4]: (E00, E11, Re E01, Im E01)
  const double* u;             // null, or the batch's [state][nper]
  unsigned long long* counts;  // [npairs][9][4]
  uint8_t* outcomes;           // null, or the batch's [state][npairs]
  uint64_t seed, run;
  int traj0, local0, nr, npairs, nev, nper;
};

// One thread per (state, pair): no sum crosses a thread, so the order is fixed; the table takes
// integer atomics only.
__global__ __launch_bounds__(kDT) void k_mps_traj_pair_draw(const PairDrawJob j) {
  const int e = blockIdx.x * kDT + threadIdx.x;
  if (e >= j.nr * j.npairs) return;
  const int s = e / j.npairs, pj = e - s * j.npairs;
  const int t = j.traj0 + s, local = j.local0 + s, s9 = t % 9;
  const int qa = j.pairs[2 * pj], qb = j.pairs[2 * pj + 1];
  const int lo = qa < qb ? qa : qb, hi = qa < qb ? qb : qa;
  const cplx* rho = j.rdm + (size_t)e * 16;
  double d[4], ox[6], oy[6];  // rho_ss; rho_st, s < t
  int c = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    d[a] = aqc::ldg(rho + 5 * a).x;
#pragma unroll
    for (int b = a + 1; b < 4; ++b, ++c) {
      const cplx z = aqc::ldg(rho + 4 * a + b);
      ox[c] = z.x;
      oy[c] = z.y;
    }
  }
  const double* eh = j.effects + (size_t)((hi * 3 + s9 / 3) * 2) * 4;
  const double* el = j.effects + (size_t)((lo * 3 + s9 % 3) * 2) * 4;
  const double uu = j.u ? aqc::ldg(j.u + (size_t)local * j.nper + j.nev + pj)
                        : aqc::sample_uniform(j.seed, j.run, (uint64_t)t, (uint32_t)(j.nev + pj));
  const int k = aqc::pair_outcome(eh, el, d, ox, oy, uu);
  if (j.outcomes) j.outcomes[(size_t)local * j.npairs + pj] = (uint8_t)k;
  atomicAdd(j.counts + ((size_t)pj * 9 + s9) * 4 + k, 1ULL);
}

// ---- the Pauli readout -----------------------------------------------------------------------
struct ChainState {
  const cplx* gam;
  const double* lam;
  const int* dims;
  const cplx* Lenv;  // L_b at b cap^2 [bra][ket], row stride cap (b = 0 .. n-1)
  const cplx* Renv;  // R_b at b cap^2 [ket][bra], row stride cap (b = 1 .. n)
};

struct ChainJob {
  const ChainState* states;  // the sweep's nr states
  const uint8_t* codes;      // nterms x n
  const int* terms;          // per issued term: lo, hi, index (index nterms: the all-identity term, w)
  const double* dtab;        // [n][3][4]: (D00, D11, Re D01, Im D01) of qubit q under letter c at (3 q + c - 1) 4
  int n, cap, nterms, nr;
  cplx* ws;     // per workgroup 3 cap^2: E (cap x cap), T (cap x 2 cap)
  double* out;  // [nr][nterms + 1], the last column w
};

// sum over the block in a fixed order (lane tree, then the four waves in index order); the result in thread 0
__device__ __forceinline__ double chain_block_sum(double v, double* red) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(kCT) void k_mps_traj_pauli_chain(const ChainJob j) {
  __shared__ aqc::GemmLds lds;
  __shared__ double red[4];
  const int n = j.n, cap = j.cap, nout = j.nterms + 1;
  const size_t cc = (size_t)cap * cap;
  cplx* E = j.ws + (size_t)blockIdx.x * 3 * cc;
  cplx* T = E + cc;
  const int items = nout * j.nr;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int it = item / j.nr, st = item % j.nr;
    const int lo = j.terms[3 * it], hi = j.terms[3 * it + 1], term = j.terms[3 * it + 2];
    const ChainState& S = j.states[st];
    const uint8_t* code = term < j.nterms ? j.codes + (size_t)term * n : nullptr;
    const cplx* cur = S.Lenv + (size_t)lo * cc;
    for (int i = lo; i <= hi; ++i) {
      const int cl = min(S.dims[i], cap), cr = min(S.dims[i + 1], cap);
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
      // the site's factor: column t of D is (D00, conj(D01)) for t = 0 and (D01, D11) for t = 1
      const int p = code ? code[i] : 0;
      double d00 = 1.0, d11 = 1.0, dx = 0.0, dy = 0.0;
      if (p) {
        const double* d = j.dtab + (size_t)(3 * i + p - 1) * 4;
        d00 = aqc::ldg(d), d11 = aqc::ldg(d + 1), dx = aqc::ldg(d + 2), dy = aqc::ldg(d + 3);
      }
      // E'[b'][k'] = sum_{(t, b)} (sum_s D[s][t] conj(A_s[b][b'])) T[b][t cap + k']
      aqc::block_cgemm<false, false, true>(
          cr, cr, 2 * cl,
          [&](int r, int kk) {
            const int t = kk >= cl ? 1 : 0, b = kk - t * cl;
            const size_t o = (size_t)b * cap + r;
            const cplx a0 = aqc::cconj(aqc::ldg(g + o)), a1 = aqc::cconj(aqc::ldg(g + cc + o));
            const cplx c0 = t ? aqc::cmk(dx, dy) : aqc::cmk(d00, 0.0), c1 = t ? aqc::cmk(d11, 0.0) : aqc::cmk(dx, -dy);
            return aqc::cscale(aqc::cfma(c1, a1, aqc::cmul(c0, a0)), aqc::ldg(lam + r));
          },
          [&](int kk, int c) {
            const int t = kk >= cl ? 1 : 0, b = kk - t * cl;
            return T[(size_t)b * 2 * cap + (size_t)t * cap + c];
          },
          [&](int r, int c, cplx v) { E[(size_t)r * cap + c] = v; }, lds);
      __syncthreads();
      cur = E;
    }
    const int d = min(S.dims[hi + 1], cap);
    const cplx* R = S.Renv + (size_t)(hi + 1) * cc;
    double acc = 0.0;
    for (int e = threadIdx.x; e < d * d; e += kCT) {
      const int b = e / d, k = e % d;
      const cplx x = cur[(size_t)b * cap + k], y = aqc::ldg(R + (size_t)k * cap + b);
      acc += fma(x.x, y.x, -x.y * y.y);
    }
    const double s = chain_block_sum(acc, red);  // (its barriers also fence E before the next item's stores)
    if (threadIdx.x == 0) j.out[(size_t)st * nout + term] = s;
  }
}

// The draw of the sweep's nr states: state s of the sweep is trajectory traj0 + s, state local0 + s of
// the batch (the batch's uniforms and output rows are indexed by that).
struct PauliDrawJob {
  const double* vals;        // [nr][nterms + 1]: v of every term, then w
  const double* u;           // null, or the batch's [state][nper]
  unsigned long long* plus;  // [nterms]
  double* values;            // null, or the batch's [state][nterms]
  double* norms;             // null, or the batch's [state]
  uint8_t* outcomes;         // null, or the batch's [state][nterms]
  uint64_t seed, run;
  int traj0, local0, nr, nterms, nev, nper;
};

// One thread per (state, term): no sum crosses a thread; the table takes integer atomics only.
__global__ __launch_bounds__(kDT) void k_mps_traj_pauli_draw(const PauliDrawJob j) {
  const int e = blockIdx.x * kDT + threadIdx.x;
  if (e >= j.nr * j.nterms) return;
  const int s = e / j.nterms, tj = e - s * j.nterms;
  const int t = j.traj0 + s, local = j.local0 + s;
  const double v = j.vals[(size_t)s * (j.nterms + 1) + tj], w = j.vals[(size_t)s * (j.nterms + 1) + j.nterms];
  const double pp = fmax(0.0, 0.5 * (w + v)), pm = fmax(0.0, 0.5 * (w - v));
  const double uu = j.u ? aqc::ldg(j.u + (size_t)local * j.nper + j.nev + tj)
                        : aqc::sample_uniform(j.seed, j.run, (uint64_t)t, (uint32_t)(j.nev + tj));
  const int o = uu * (pp + pm) >= pp ? 1 : 0;
  if (j.values) j.values[(size_t)local * j.nterms + tj] = v;
  if (j.norms && tj == 0) j.norms[local] = w;
  if (j.outcomes) j.outcomes[(size_t)local * j.nterms + tj] = (uint8_t)o;
  if (!o) atomicAdd(j.plus + tj, 1ULL);
}

// ---- the site-level schedule -----------------------------------------------------------------
enum { tGate = 0, tSwap = 1, tMove = 2, tOne = 3, tKraus = 4, tMeas = 5 };

struct TrajSched {
  std::vector<DevOp> ops;
  std::vector<uint8_t> tag;
  std::vector<Kraus2Group> groups;  // the correlated groups, in program order (DevOp::grp)
  int nev = 0;
  int general = 0;  // group events on the general path
};

thread_local const char* t_entry = "aqc_mps_traj_sample";  // the entry point named in error messages

int fail(const std::string& msg) {
  aqc::set_error(std::string(t_entry) + ": " + msg);
  return AQC_ERR_ARG;
}

// the program's rows as aqc_sv_traj_sample checks them (traj.hip, build_rows)
int validate(int n, const aqc_op_t* prog, int nprog) {
  for (int i = 0; i < nprog; ++i) {
    const aqc_op_t& op = prog[i];
    if (op.flags == 0) {
      if (!(op.nq == 1 || op.nq == 2) || op.q0 < 0 || op.q0 >= n) return fail("gate row: bad qubits");
      if (op.nq == 2 && (op.q1 < 0 || op.q1 >= n || op.q1 == op.q0)) return fail("gate row: bad qubits");
    } else if (op.flags == AQC_OP_KRAUS1) {
      if (op.nq != 1 || op.q0 < 0 || op.q0 >= n || op.q1 < 1 || op.q1 > 4) return fail("malformed Kraus row");
      double s00 = 0.0, s11 = 0.0, sx = 0.0, sy = 0.0;
      for (int k = 0; k < op.q1; ++k) {
        const double* K = op.m + 8 * k;  // K00 K01 K10 K11 as (re, im)
        for (int e = 0; e < 8; ++e)
          if (!std::isfinite(K[e])) return fail("malformed Kraus row");
        s00 += K[0] * K[0] + K[1] * K[1] + K[4] * K[4] + K[5] * K[5];
        s11 += K[2] * K[2] + K[3] * K[3] + K[6] * K[6] + K[7] * K[7];
        sx += K[0] * K[2] + K[1] * K[3] + K[4] * K[6] + K[5] * K[7];
        sy += K[0] * K[3] - K[1] * K[2] + K[4] * K[7] - K[5] * K[6];
      }
      if (std::fabs(s00 - 1.0) > 1e-9 || std::fabs(s11 - 1.0) > 1e-9 || std::fabs(sx) > 1e-9 || std::fabs(sy) > 1e-9)
        return fail("Kraus row: sum K^dag K is not the identity");
    } else if (g_correlated != 0 && (op.flags & 0xff) == AQC_OP_KRAUS2) {
      // a correlated group, as aqc_sv_traj_sample checks it (kraus_group.h)
      if (const char* why = aqc::kraus2_first_row_error(op, n, nprog - i)) return fail(why);
      const int nk = (op.flags >> 16) & 0xff;
      double w[16][16];
      bool flat;
      if (const char* why = aqc::kraus2_group_error(prog + i, nk, w, &flat)) return fail(why);
      i += nk - 1;
    } else {
      return fail("unknown row flags");
    }
  }
  return AQC_OK;
}

cplx hdiv(cplx a, cplx b) {  // a / b on the host
  const double d = b.x * b.x + b.y * b.y;
  return aqc::hc((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}

// K (4x4, index 2 b1 + b0) = z B (x) A with A (on b0) and B (on b1) unitary, all within 1e-12: then A
// times z / |z| into A, B into B.  The zero operator qualifies (A = B = I; its weight is 0).
bool product_unitary(const double* m, cplx* A, cplx* B) {
  cplx K[16];
  int at = 0;
  double big = 0.0;
  for (int e = 0; e < 16; ++e) {
    K[e] = aqc::hc(m[2 * e], m[2 * e + 1]);
    const double v = K[e].x * K[e].x + K[e].y * K[e].y;
    if (v > big) big = v, at = e;
  }
  for (int e = 0; e < 4; ++e) A[e] = B[e] = aqc::hc(e == 0 || e == 3 ? 1 : 0, 0);
  if (std::sqrt(big) <= 1e-12) return true;
  const int r = at >> 2, c = at & 3, r1 = r >> 1, r0 = r & 1, c1 = c >> 1, c0 = c & 1;
  const cplx z = K[at];
  cplx A0[4], B0[4];  // z B[r1][c1] A and z A[r0][c0] B
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) {
      A0[2 * i + j] = K[(2 * r1 + i) * 4 + 2 * c1 + j];
      B0[2 * i + j] = K[(2 * i + r0) * 4 + 2 * j + c0];
    }
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j)
      for (int k = 0; k < 2; ++k)
        for (int l = 0; l < 2; ++l) {
          const cplx t = hdiv(aqc::hmul(B0[2 * i + j], A0[2 * k + l]), z), want = K[(2 * i + k) * 4 + 2 * j + l];
          if (std::hypot(t.x - want.x, t.y - want.y) > 1e-12) return false;
        }
  auto unit = [](cplx* U) {  // U / sqrt(alpha) where U^dag U = alpha I; false where it is not
    const double alpha = U[0].x * U[0].x + U[0].y * U[0].y + U[2].x * U[2].x + U[2].y * U[2].y;
    if (!(alpha > 0.0)) return -1.0;
    const double sc = 1.0 / std::sqrt(alpha);
    for (int e = 0; e < 4; ++e) U[e] = aqc::hc(U[e].x * sc, U[e].y * sc);
    const double n1 = U[1].x * U[1].x + U[1].y * U[1].y + U[3].x * U[3].x + U[3].y * U[3].y;
    // column 0 . column 1
    const double dx = U[0].x * U[1].x + U[0].y * U[1].y + U[2].x * U[3].x + U[2].y * U[3].y;
    const double dy = U[0].x * U[1].y - U[0].y * U[1].x + U[2].x * U[3].y - U[2].y * U[3].x;
    if (std::fabs(n1 - 1.0) > 1e-12 || std::fabs(dx) > 1e-12 || std::fabs(dy) > 1e-12) return -1.0;
    return alpha;
  };
  const double alpha = unit(A0), beta = unit(B0);
  if (alpha < 0.0 || beta < 0.0) return false;
  // K = B0 (x) A0 / z = (sqrt(alpha beta) / z) B (x) A: the scalar's phase is conj(z) / |z|
  const double az = std::sqrt(big);
  const cplx ph = aqc::hc(z.x / az, -z.y / az);
  for (int e = 0; e < 4; ++e) A[e] = aqc::hmul(ph, A0[e]), B[e] = B0[e];
  return true;
}

struct Planner {
  int n, a, b;  // every site < a left-orthonormal, every site > b right-orthonormal
  std::vector<int> order, loc;
  std::vector<DevOp> tmp;  // what the swap-left scheduler emits, before the centre moves go between
  aqc::Scheduler sc;
  TrajSched& out;

  Planner(int n_, TrajSched& dst) : n(n_), a(n_), b(-1), order(n_), loc(n_), sc(n_, order, loc, tmp), out(dst) {
    for (int i = 0; i < n; ++i) order[i] = loc[i] = i;
  }

  void push(const DevOp& d, int tag) {
    out.ops.push_back(d);
    out.tag.push_back((uint8_t)tag);
  }

  void update(const DevOp& d, int tag) {  // a two-site update whose precondition holds
    push(d, tag);
    const int p = d.p;
    if (a < p + 2) a = p + 1;
    if (b > p - 1) b = p;
  }

  void centre(int left, int right) {  // until a >= left and b <= right
    DevOp id = DevOp();
    id.kind = 2;
    for (int e = 0; e < 4; ++e) id.m[5 * e] = aqc::hc(1, 0);
    while (a < left) {
      id.p = a;
      update(id, tMove);
    }
    while (b > right) {
      id.p = b - 1;
      update(id, tMove);
    }
  }

  void drain(bool last_is_gate) {
    for (size_t i = 0; i < tmp.size(); ++i) {
      const DevOp& d = tmp[i];
      if (d.kind == 2) {
        centre(d.p, d.p + 1);
        update(d, last_is_gate && i + 1 == tmp.size() ? tGate : tSwap);
      } else {
        push(d, tOne);
      }
    }
    tmp.clear();
  }

  void row(int p, int nk, const cplx* K, int slot, int meas) {
    centre(p, p);
    DevOp d = DevOp();
    d.kind = 3;
    d.p = p;
    d.nk = nk;
    d.slot = slot;
    d.meas = meas;
    for (int e = 0; e < 4 * nk; ++e) d.m[e] = K[e];
    push(d, meas ? tMeas : tKraus);
    a = b = p;
  }

  // A correlated group on (q0, q1): one event.  Product-unitary (every K_k a scalar times A_k (x) B_k,
  // both unitary; not under mode 2): constant weights and one-site unitaries, which keep both
  // orthonormality properties -- one row on the two sites where the qubits sit, no routing, no centre
  // move, no SVD.  Otherwise a two-site update whose 4x4 operator is chosen on the device: routed and
  // folded like a gate (Scheduler::two), behind the centre moves of a two-site update; the split of
  // theta' is then a Schmidt decomposition, and the centre stands on the two sites (a = p + 1, b = p).
  void group(const aqc_op_t* ops, int nk) {
    const int q0 = ops[0].q0, q1 = ops[0].q1;
    double w[16][16];
    bool flat = true;
    aqc::kraus2_group_error(ops, nk, w, &flat);  // (validated: only the weights are wanted)
    Kraus2Group g;
    std::memset(&g, 0, sizeof(g));
    g.nk = nk;
    g.flat = flat ? 1 : 0;
    cplx A[16][4], B[16][4], Pa[4], Pb[4];
    bool product = flat && g_correlated != 2;
    for (int k = 0; k < nk && product; ++k) product = product_unitary(ops[k].m, A[k], B[k]);
    DevOp d = DevOp();
    d.nk = nk;
    d.slot = out.nev++;
    d.grp = (int)out.groups.size();
    if (product) {
      sc.pending(q0, q1, Pa, Pb);
      sc.has[q0] = sc.has[q1] = 0;
      for (int k = 0; k < nk; ++k) {
        aqc::mat2_mul(A[k], Pa, &g.K[k][0]);
        aqc::mat2_mul(B[k], Pb, &g.K[k][4]);
        g.W[k][0] = w[k][0];
      }
      d.kind = 5;
      d.p = loc[q0];
      d.p2 = loc[q1];
      push(d, tKraus);
    } else {
      const int low = sc.route(q0, q1);
      drain(false);
      sc.pending(q0, q1, Pa, Pb);
      sc.has[q0] = sc.has[q1] = 0;
      for (int k = 0; k < nk; ++k) {
        cplx M4[16];
        for (int e = 0; e < 16; ++e) M4[e] = aqc::hc(ops[k].m[2 * e], ops[k].m[2 * e + 1]);
        sc.fold_site_order(q0, low, M4, Pa, Pb, g.K[k]);
        aqc::kraus2_weights((const double*)g.K[k], g.W[k]);
        if (flat) g.W[k][0] = w[k][0];  // the constant weight by aqc_sv_traj_sample's own arithmetic
      }
      centre(low, low + 1);
      d.kind = 4;
      d.p = low;
      for (int e = 0; e < 4; ++e) d.m[5 * e] = aqc::hc(1, 0);
      // K_k is not unitary: the Schmidt values of every other bond change, so nothing beyond the two
      // sites keeps its property (a gate's update keeps a >= p + 2 and b <= p - 1); the split leaves
      // site p left- and site p + 1 right-orthonormal
      push(d, tKraus);
      a = low + 1;
      b = low;
      out.general += 1;
    }
    out.groups.push_back(g);
  }

  // measure: the sweep of measurement rows behind the sort (the sampler's ending; the pair readout
  // stops at the sorted state)
  void run(const aqc_op_t* prog, int nprog, bool measure) {
    for (int i = 0; i < nprog; ++i) {
      const aqc_op_t& op = prog[i];
      if (op.flags == AQC_OP_KRAUS1) {
        const int q = op.q0, nk = op.q1;
        cplx K[16];
        for (int e = 0; e < 4 * nk; ++e) K[e] = aqc::hc(op.m[2 * e], op.m[2 * e + 1]);
        if (sc.has[q]) {  // K_k <- K_k P: exact for any K (folding P into a later update is not)
          for (int k = 0; k < nk; ++k) aqc::mat2_mul(K + 4 * k, &sc.pend[4 * q], K + 4 * k);
          sc.has[q] = 0;
        }
        row(loc[q], nk, K, out.nev++, 0);
      } else if ((op.flags & 0xff) == AQC_OP_KRAUS2) {
        const int nk = (op.flags >> 16) & 0xff;
        group(prog + i, nk);
        i += nk - 1;
      } else if (op.nq == 1) {
        sc.one(op.q0, op.m);
      } else {
        sc.two(op.q0, op.q1, op.m);
        drain(true);
      }
    }
    sc.flush();
    drain(false);
    sc.sort();
    drain(false);
    if (!measure) return;
    cplx proj[8];
    for (int e = 0; e < 8; ++e) proj[e] = aqc::hc(e == 0 || e == 7 ? 1 : 0, 0);
    for (int q = 0; q < n; ++q) row(q, 2, proj, q, 1);
  }
};

int build_schedule(int n, const aqc_op_t* prog, int nprog, TrajSched& s, bool measure = true) {
  if (int rc = validate(n, prog, nprog)) return rc;
  Planner pl(n, s);
  pl.run(prog, nprog, measure);
  return AQC_OK;
}

// the most two-site updates of one wave, levelled as run_waves levels a chunk (mps.hip, level_ops)
int max_width(const DevOp* ops, size_t count, int n) {
  std::vector<int> last(n + 1, -1), per;
  int width = 1;
  for (size_t i = 0; i < count; ++i) {
    const DevOp& op = ops[i];
    int l;
    if (aqc::two_site(op)) {
      l = std::max(last[op.p], last[op.p + 1]) + 1;
      last[op.p] = last[op.p + 1] = l;
      if ((int)per.size() <= l) per.resize(l + 1, 0);
      width = std::max(width, ++per[l]);
    } else if (op.kind == 5) {
      l = std::max(last[op.p], last[op.p2]) + 1;
      last[op.p] = last[op.p2] = l;
    } else {
      l = last[op.p] + 1;
      last[op.p] = l;
    }
  }
  return width;
}

aqc::PerDevice<aqc::DevScratch> g_scr;
using aqc::up256;

struct Handles {
  std::vector<aqc_mps_t> h;
  ~Handles() {
    for (aqc_mps_t x : h) aqc_mps_destroy(x);
  }
  int create(int count, int n, int chi_cap, double threshold, int max_chi) {
    h.reserve(count);
    for (int s = 0; s < count; ++s) {
      aqc_mps_t x = nullptr;
      if (int rc = aqc_mps_create(n, chi_cap, threshold, max_chi, &x)) return rc;
      h.push_back(x);
    }
    return AQC_OK;
  }
};

// device bytes of one trajectory's handle while the schedule runs: the Gammas, and one two-site
// workspace per concurrent update of the widest wave of a chunk
int sched_width(const TrajSched& sch, int n) {
  const size_t nrows = sch.ops.size();
  int width = 1;
  for (size_t r0 = 0; r0 < nrows; r0 += kChunkRows)
    width = std::max(width, max_width(sch.ops.data() + r0, std::min<size_t>(kChunkRows, nrows - r0), n));
  return width;
}

size_t evolve_state_bytes(const TrajSched& sch, int n, size_t cap) {
  const int width = sched_width(sch, n);
  return ((size_t)n * 2 * cap * cap + (size_t)width * (4 * cap * cap + aqc::work_elems(cap))) * sizeof(cplx);
}

// What a call with correlated groups keeps on the device beside its states: the group table, and for the
// general events of one wave (at most one per two-site update of the widest wave and state) the partial
// sums of k_mps_kraus2_rho and the chosen operators.
struct K2Bufs {
  size_t gb = 0, pb = 0, sb = 0;
  int slices = 0, jobs = 0;
  size_t bytes() const { return gb + pb + sb; }
};

K2Bufs k2_bufs(const TrajSched& sch, int n, int B, int cap) {
  K2Bufs k;
  if (sch.groups.empty()) return k;
  k.gb = up256(sch.groups.size() * sizeof(Kraus2Group));
  if (sch.general == 0) return k;
  k.slices = (int)(((size_t)cap * cap + kRhoSlice - 1) / kRhoSlice);
  k.jobs = B * sched_width(sch, n);
  k.pb = up256((size_t)k.jobs * k.slices * 16 * sizeof(double));
  k.sb = up256((size_t)k.jobs * 16 * sizeof(cplx));
  return k;
}

// binds the buffers at `base` (k.bytes() of device memory) and queues the table's upload
int k2_bind(const TrajSched& sch, const K2Bufs& k, char* base, TrajCtx& ctx, hipStream_t st) {
  if (k.gb == 0) return AQC_OK;
  ctx.groups = (const Kraus2Group*)base;
  ctx.k2_part = k.pb ? (double*)(base + k.gb) : nullptr;
  ctx.k2_sel = k.sb ? (cplx*)(base + k.gb + k.pb) : nullptr;
  ctx.k2_slices = k.slices;
  ctx.k2_jobs = k.jobs;
  AQC_HIP_CHECK(hipMemcpyAsync(base, sch.groups.data(), sch.groups.size() * sizeof(Kraus2Group), hipMemcpyHostToDevice, st));
  return AQC_OK;
}

// The schedule's rows on nb states (state s carrying shot ctx.shot0 + s), chunk by chunk; then waits
// for the batch and reads its flags: a capacity overflow ends the call.
int run_rows(const TrajSched& sch, aqc_mps_t* hs, int nb, const TrajCtx& ctx, std::vector<std::vector<DevOp>>& lists) {
  const size_t nrows = sch.ops.size();
  for (size_t r0 = 0; r0 < nrows; r0 += kChunkRows) {
    const size_t r1 = std::min(nrows, r0 + kChunkRows);
    lists.assign(nb, std::vector<DevOp>(sch.ops.begin() + r0, sch.ops.begin() + r1));
    if (int rc = aqc::run_waves(hs, nb, lists, &ctx)) return rc;
  }
  return aqc_mps_check_batch(hs, nb);
}

// aqc_mps_traj_plan's output of a schedule: a row per DevOp, a group's event as its nk rows
void write_plan(const TrajSched& s, int* counts, aqc_op_t* sched, int sched_cap) {
  for (int c = 0; c < 7; ++c) counts[c] = 0;
  for (uint8_t t : s.tag) counts[t] += 1;
  size_t at = 0;
  auto next = [&]() -> aqc_op_t* {
    aqc_op_t* o = at < (size_t)sched_cap ? &sched[at] : nullptr;
    ++at;
    if (o) std::memset(o, 0, sizeof(*o));
    return o;
  };
  for (const DevOp& d : s.ops) {
    if (d.kind == 4 || d.kind == 5) {
      const Kraus2Group& g = s.groups[d.grp];
      const bool swapped = d.kind == 5 && d.p2 < d.p;  // the row's q0 is the lower site, s1 its index
      for (int k = 0; k < d.nk; ++k) {
        aqc_op_t* o = next();
        if (!o) continue;
        o->nq = 2;
        o->q0 = d.kind == 4 ? d.p : std::min(d.p, d.p2);
        o->q1 = d.kind == 4 ? d.p + 1 : std::max(d.p, d.p2);
        o->flags = AQC_OP_KRAUS2 | (k << 8) | (d.nk << 16) | (d.kind == 5 ? 1 << 24 : 0);
        if (d.kind == 4) {
          std::memcpy(o->m, g.K[k], 16 * sizeof(cplx));
        } else {  // sqrt(p_k) U_lower (x) U_upper, out 2 s1' + s2', in 2 s1 + s2
          const cplx* lo = &g.K[k][swapped ? 4 : 0];
          const cplx* hi = &g.K[k][swapped ? 0 : 4];
          const double sc = std::sqrt(std::max(0.0, g.W[k][0]));
          cplx* m = (cplx*)o->m;
          for (int so = 0; so < 4; ++so)
            for (int si = 0; si < 4; ++si) {
              const cplx t = aqc::hmul(lo[(so >> 1) * 2 + (si >> 1)], hi[(so & 1) * 2 + (si & 1)]);
              m[so * 4 + si] = aqc::hc(t.x * sc, t.y * sc);
            }
        }
      }
      continue;
    }
    aqc_op_t* o = next();
    if (!o) continue;
    o->q0 = d.p;
    if (d.kind == 2) {
      o->nq = 2;
      o->q1 = d.p + 1;
      std::memcpy(o->m, d.m, 16 * sizeof(cplx));
    } else if (d.kind == 1) {
      o->nq = 1;
      std::memcpy(o->m, d.m, 4 * sizeof(cplx));
    } else {
      o->nq = 1;
      o->q1 = d.meas ? d.slot : d.nk;
      o->flags = d.meas ? AQC_OP_MEASURE1 : (AQC_OP_KRAUS1 | (d.slot << 8));
      std::memcpy(o->m, d.m, 4 * (size_t)d.nk * sizeof(cplx));
    }
  }
  counts[6] = (int)at;
}

int plan(const char* entry, bool measure, int n, const aqc_op_t* prog, int nprog, int* counts, aqc_op_t* sched,
         int sched_cap) {
  t_entry = entry;
  if (!(counts && nprog >= 0 && (prog || nprog == 0) && sched_cap >= 0 && (sched || sched_cap == 0)))
    return fail("bad argument");
  if (!(n >= 1 && n <= 4096)) return fail("n must be in 1 .. 4096");
  TrajSched s;
  if (int rc = build_schedule(n, prog, nprog, s, measure)) return rc;
  write_plan(s, counts, sched, sched_cap);
  return AQC_OK;
}

}  // namespace

int aqc::launch_kraus(const KrausJob* jobs, int nj, const TrajCtx& ctx, hipStream_t st) {
  // each job: the site's two Gammas read twice and written once, the lambdas
  KernelTimer::begin(st, "mps_kraus1", 0.0, 0.0);
  hipLaunchKernelGGL(k_mps_kraus1, dim3(nj), dim3(kKT), 0, st, jobs, ctx);
  KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  return AQC_OK;
}

int aqc::launch_kraus2(const TwoSiteJob* two, const Kraus2Job* jobs, int nj, int cap_max, const TrajCtx& ctx,
                       hipStream_t st) {
  if (!(ctx.groups && ctx.k2_part && ctx.k2_sel) || nj > ctx.k2_jobs ||
      ((size_t)cap_max * cap_max + kRhoSlice - 1) / kRhoSlice > (size_t)ctx.k2_slices) {
    aqc::set_error("launch_kraus2: the trajectory context has no room for the wave's group events");
    return AQC_ERR_ARG;
  }
  const double pos = (double)cap_max * cap_max;
  // rho: theta read once; apply: read and written
  KernelTimer::begin(st, "mps_kraus2_rho", nj * pos * 4.0 * 16.0, nj * pos * 64.0);
  hipLaunchKernelGGL(k_mps_kraus2_rho, dim3(ctx.k2_slices, nj), dim3(kK2T), 0, st, two, jobs, ctx);
  KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_mps_kraus2_pick, dim3(nj), dim3(64), 0, st, jobs, ctx);
  AQC_CHECK_LAUNCH();
  const int blocks = (int)std::min<size_t>(kApplyMaxBlocks, ((size_t)cap_max * cap_max + kK2T - 1) / kK2T);
  KernelTimer::begin(st, "mps_kraus2_apply", nj * pos * 8.0 * 16.0, nj * pos * 128.0);
  hipLaunchKernelGGL(k_mps_kraus2_apply, dim3(blocks, nj), dim3(kK2T), 0, st, two, jobs, ctx);
  KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  return AQC_OK;
}

int aqc::launch_kraus2_prod(const Kraus2ProdJob* jobs, int nj, int cap_max, const TrajCtx& ctx, hipStream_t st) {
  if (!ctx.groups) {
    aqc::set_error("launch_kraus2_prod: the trajectory context has no group table");
    return AQC_ERR_ARG;
  }
  const int blocks = (int)std::min<size_t>(kApplyMaxBlocks, ((size_t)cap_max * cap_max + kK2T - 1) / kK2T);
  // each job: two sites' Gammas read and written
  KernelTimer::begin(st, "mps_kraus2_prod", nj * 8.0 * 16.0 * (double)cap_max * cap_max, 0.0);
  hipLaunchKernelGGL(k_mps_kraus2_prod, dim3(blocks, nj), dim3(kK2T), 0, st, jobs, ctx);
  KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  return AQC_OK;
}

extern "C" {

int aqc_mps_traj_set_correlated(int mode) {
  AQC_REQUIRE(mode >= 0 && mode <= 2, "aqc_mps_traj_set_correlated: 0 (refuse), 1 (run) or 2 (every group general)");
  g_correlated = mode;
  return AQC_OK;
}

int aqc_mps_traj_set_batch(int batch) {
  AQC_REQUIRE(batch >= 0 && batch <= 4096, "aqc_mps_traj_set_batch: 0 (default) or 1 .. 4096");
  g_forced_batch = batch;
  return AQC_OK;
}

int aqc_mps_traj_set_readout_batch(int batch) {
  AQC_REQUIRE(batch >= 0 && batch <= 4096, "aqc_mps_traj_set_readout_batch: 0 (default) or 1 .. 4096");
  g_forced_readout = batch;
  return AQC_OK;
}

int aqc_mps_traj_plan(int n, const aqc_op_t* prog, int nprog, int* counts, aqc_op_t* sched, int sched_cap) {
  return plan("aqc_mps_traj_plan", true, n, prog, nprog, counts, sched, sched_cap);
}

int aqc_mps_traj_tomo_plan(int n, const aqc_op_t* prog, int nprog, int* counts, aqc_op_t* sched, int sched_cap) {
  return plan("aqc_mps_traj_tomo_plan", false, n, prog, nprog, counts, sched, sched_cap);
}

int aqc_mps_traj_sample(int n, int chi_cap, double threshold, int max_chi, const aqc_op_t* prog, int nprog, int nshots,
                        uint64_t seed, uint64_t run, const double* u, uint64_t* out, uint8_t* choices) {
  t_entry = "aqc_mps_traj_sample";
  AQC_REQUIRE(out && nprog >= 0 && (prog || nprog == 0), "aqc_mps_traj_sample: null argument");
  AQC_REQUIRE(n >= 1 && n <= 4096, "aqc_mps_traj_sample: n must be in 1 .. 4096");
  AQC_REQUIRE(chi_cap >= 1 && chi_cap <= aqc::kMaxCap, "aqc_mps_traj_sample: chi_cap must be in [1, 1024]");
  AQC_REQUIRE(nshots >= 1 && nshots <= kMaxShots, "aqc_mps_traj_sample: nshots must be in 1 .. 2^30");
  TrajSched sch;
  if (int rc = build_schedule(n, prog, nprog, sch)) return rc;
  const int nev = sch.nev, nper = nev + n, words = (n + 63) / 64;
  if (u)
    for (size_t e = 0, nu = (size_t)nshots * nper; e < nu; ++e)
      if (!(u[e] >= 0.0 && u[e] < 1.0)) return fail("u must lie in [0, 1)");
  const bool want_choices = choices && nev > 0;
  // the batch: B trajectories as B handles
  const size_t per_state = evolve_state_bytes(sch, n, chi_cap);
  int B = (int)std::min<size_t>({(size_t)nshots, (size_t)kMaxBatch, std::max<size_t>(1, kBatchBudgetBytes / per_state)});
  if (g_forced_batch > 0) B = std::min(nshots, g_forced_batch);
  Handles hs;
  if (int rc = hs.create(B, n, chi_cap, threshold, max_chi)) return rc;
  hipStream_t st = aqc::mps_stream();
  const size_t ub = u ? up256((size_t)B * nper * sizeof(double)) : 0;
  const size_t ob = up256((size_t)B * words * sizeof(uint64_t));
  const size_t cb = want_choices ? up256((size_t)B * nev) : 0;
  const K2Bufs k2 = k2_bufs(sch, n, B, chi_cap);
  AQC_HIP_CHECK(hipStreamSynchronize(st));  // (the scratch may be regrown)
  aqc::DevScratch& scr = g_scr.here();
  if (int rc = scr.ensure(ub + ob + cb + k2.bytes())) return rc;
  TrajCtx ctx;
  std::memset(&ctx, 0, sizeof(ctx));
  ctx.seed = seed;
  ctx.run = run;
  ctx.u = u ? (const double*)scr.dev : nullptr;
  ctx.out = (uint64_t*)(scr.dev + ub);
  ctx.choices = want_choices ? (uint8_t*)(scr.dev + ub + ob) : nullptr;
  ctx.nev = nev;
  ctx.nper = nper;
  ctx.words = words;
  if (int rc = k2_bind(sch, k2, scr.dev + ub + ob + cb, ctx, st)) return rc;
  std::vector<std::vector<DevOp>> lists;
  for (int shot0 = 0; shot0 < nshots; shot0 += B) {
    const int nb = std::min(B, nshots - shot0);
    ctx.shot0 = shot0;
    if (shot0 > 0)
      for (int s = 0; s < nb; ++s)
        if (int rc = aqc::mps_reset_zero(hs.h[s])) return rc;
    AQC_HIP_CHECK(hipMemsetAsync(ctx.out, 0, (size_t)nb * words * sizeof(uint64_t), st));
    if (u)
      AQC_HIP_CHECK(hipMemcpyAsync(scr.dev, u + (size_t)shot0 * nper, (size_t)nb * nper * sizeof(double),
                                   hipMemcpyHostToDevice, st));
    if (int rc = run_rows(sch, hs.h.data(), nb, ctx, lists)) return rc;
    AQC_HIP_CHECK(hipMemcpyAsync(out + (size_t)shot0 * words, ctx.out, (size_t)nb * words * sizeof(uint64_t),
                                 hipMemcpyDeviceToHost, st));
    if (want_choices)
      AQC_HIP_CHECK(hipMemcpyAsync(choices + (size_t)shot0 * nev, ctx.choices, (size_t)nb * nev, hipMemcpyDeviceToHost, st));
    AQC_HIP_CHECK(hipStreamSynchronize(st));
  }
  return AQC_OK;
}

int aqc_mps_traj_pair_tomo(int n, int chi_cap, double threshold, int max_chi, const aqc_op_t* prog, int nprog,
                           const int* pairs, int npairs, const double* effects, int nshots, uint64_t seed, uint64_t run,
                           const double* u, int64_t* counts, uint8_t* outcomes) {
  t_entry = "aqc_mps_traj_pair_tomo";
  AQC_REQUIRE(counts && pairs && effects && nprog >= 0 && (prog || nprog == 0), "aqc_mps_traj_pair_tomo: null argument");
  AQC_REQUIRE(n >= 2 && n <= 4096, "aqc_mps_traj_pair_tomo: n must be in 2 .. 4096");
  AQC_REQUIRE(chi_cap >= 1 && chi_cap <= aqc::kMaxCap, "aqc_mps_traj_pair_tomo: chi_cap must be in [1, 1024]");
  AQC_REQUIRE(npairs >= 1 && npairs <= kMaxPairs, "aqc_mps_traj_pair_tomo: npairs must be in 1 .. 4096");
  AQC_REQUIRE(nshots >= 1 && nshots <= kMaxShots / 9, "aqc_mps_traj_pair_tomo: 9 nshots must be in 9 .. 2^30");
  int na = 0;  // distinct lower qubits: what the RDM sweep's workspace grows with
  {
    std::vector<char> lower(n, 0);
    for (int p = 0; p < npairs; ++p) {
      const int a = pairs[2 * p], b = pairs[2 * p + 1];
      if (a < 0 || a >= n || b < 0 || b >= n || a == b) return fail("a pair needs two different qubits in 0 .. n-1");
      na += !lower[std::min(a, b)];
      lower[std::min(a, b)] = 1;
    }
  }
  if (int rc = aqc::check_effects(n, effects, t_entry)) return rc;
  TrajSched sch;
  if (int rc = build_schedule(n, prog, nprog, sch, false)) return rc;
  const int ntraj = 9 * nshots;
  const int nev = sch.nev, nper = nev + npairs;
  if (u)
    for (size_t e = 0, nu = (size_t)ntraj * nper; e < nu; ++e)
      if (!(u[e] >= 0.0 && u[e] < 1.0)) return fail("u must lie in [0, 1)");
  // The batch: B trajectories run the schedule together as B handles and are read out R at a time,
  // B evolve + R readout within the budget (readout: the RDM sweep's workspace of one state and its
  // npairs 4x4 blocks).  A wave of the schedule holds one update per state, so the run time goes with
  // the number of batches; the sweep has a workgroup per (state, chain) and fills the chip with few
  // states: R stays small, at most half the budget, and B takes the rest.
  const size_t evolve = evolve_state_bytes(sch, n, chi_cap);
  const size_t readout = aqc::pair_rdm_state_bytes(n, chi_cap, na) + (size_t)npairs * 16 * sizeof(cplx);
  int R = (int)std::max<size_t>(1, std::min<size_t>({(size_t)kReadoutStates, (size_t)ntraj, kBatchBudgetBytes / 2 / readout}));
  const size_t left = kBatchBudgetBytes - std::min(kBatchBudgetBytes, (size_t)R * readout);
  int B = (int)std::min<size_t>({(size_t)ntraj, (size_t)kMaxBatch, std::max<size_t>(1, left / evolve)});
  if (g_forced_batch > 0) {  // what a forced batch leaves of the budget
    B = std::min(ntraj, g_forced_batch);
    const size_t held = std::min(kBatchBudgetBytes, (size_t)B * evolve);
    R = (int)std::max<size_t>(1, std::min<size_t>((size_t)R, (kBatchBudgetBytes - held) / readout));
  }
  R = std::min(R, B);
  if (g_forced_readout > 0) R = std::min(B, g_forced_readout);
  Handles hs;
  if (int rc = hs.create(B, n, chi_cap, threshold, max_chi)) return rc;
  hipStream_t st = aqc::mps_stream();
  const size_t ub = u ? up256((size_t)B * nper * sizeof(double)) : 0;
  const size_t qb = up256((size_t)npairs * 2 * sizeof(int));
  const size_t eb = up256((size_t)n * 24 * sizeof(double));
  const size_t tb = up256((size_t)npairs * 36 * sizeof(int64_t));
  const size_t ob = outcomes ? up256((size_t)B * npairs) : 0;
  const size_t rb = up256((size_t)R * npairs * 16 * sizeof(cplx));
  const K2Bufs k2 = k2_bufs(sch, n, B, chi_cap);
  AQC_HIP_CHECK(hipStreamSynchronize(st));  // (the scratch may be regrown)
  aqc::DevScratch& scr = g_scr.here();
  if (int rc = scr.ensure(ub + qb + eb + tb + ob + rb + k2.bytes())) return rc;
  char* buf = scr.dev;
  TrajCtx ctx;
  std::memset(&ctx, 0, sizeof(ctx));
  ctx.seed = seed;
  ctx.run = run;
  ctx.u = u ? (const double*)buf : nullptr;
  ctx.nev = nev;
  ctx.nper = nper;
  if (int rc = k2_bind(sch, k2, buf + ub + qb + eb + tb + ob + rb, ctx, st)) return rc;
  PairDrawJob dj;
  std::memset(&dj, 0, sizeof(dj));
  dj.u = ctx.u;
  dj.pairs = (const int*)(buf + ub);
  dj.effects = (const double*)(buf + ub + qb);
  dj.counts = (unsigned long long*)(buf + ub + qb + eb);
  dj.outcomes = outcomes ? (uint8_t*)(buf + ub + qb + eb + tb) : nullptr;
  dj.rdm = (const cplx*)(buf + ub + qb + eb + tb + ob);
  dj.seed = seed;
  dj.run = run;
  dj.npairs = npairs;
  dj.nev = nev;
  dj.nper = nper;
  AQC_HIP_CHECK(hipMemcpyAsync((void*)dj.pairs, pairs, (size_t)npairs * 2 * sizeof(int), hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemcpyAsync((void*)dj.effects, effects, (size_t)n * 24 * sizeof(double), hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemsetAsync(dj.counts, 0, (size_t)npairs * 36 * sizeof(int64_t), st));
  std::vector<std::vector<DevOp>> lists;
  for (int t0 = 0; t0 < ntraj; t0 += B) {
    const int nb = std::min(B, ntraj - t0);
    ctx.shot0 = t0;
    if (t0 > 0)
      for (int s = 0; s < nb; ++s)
        if (int rc = aqc::mps_reset_zero(hs.h[s])) return rc;
    if (u)
      AQC_HIP_CHECK(hipMemcpyAsync(buf, u + (size_t)t0 * nper, (size_t)nb * nper * sizeof(double), hipMemcpyHostToDevice, st));
    if (int rc = run_rows(sch, hs.h.data(), nb, ctx, lists)) return rc;
    for (int r0 = 0; r0 < nb; r0 += R) {
      const int nr = std::min(R, nb - r0);
      // every pair's RDM of the sweep's states, by full contraction (a Kraus row has broken Vidal form)
      if (int rc = aqc_mps_pair_rdms_batch(hs.h.data() + r0, nr, pairs, npairs, (double*)dj.rdm, 1)) return rc;
      dj.traj0 = t0 + r0;
      dj.local0 = r0;
      dj.nr = nr;
      // each thread: 16 complex of RDM and two effects read, one byte and one count written
      aqc::KernelTimer::begin(st, "mps_traj_pair_draw", (double)nr * npairs * (16.0 * 16 + 64 + 9), 0.0);
      hipLaunchKernelGGL(k_mps_traj_pair_draw, dim3((nr * npairs + kDT - 1) / kDT), dim3(kDT), 0, st, dj);
      aqc::KernelTimer::end(st);
      AQC_CHECK_LAUNCH();
    }
    if (outcomes)
      AQC_HIP_CHECK(hipMemcpyAsync(outcomes + (size_t)t0 * npairs, dj.outcomes, (size_t)nb * npairs, hipMemcpyDeviceToHost, st));
    AQC_HIP_CHECK(hipStreamSynchronize(st));  // the next batch overwrites the uniforms and the outcome bytes
  }
  // the table accumulated on the device across the batches
  AQC_HIP_CHECK(hipMemcpyAsync(counts, dj.counts, (size_t)npairs * 36 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  return AQC_OK;
}

int aqc_mps_traj_pauli_counts(int n, int chi_cap, double threshold, int max_chi, const aqc_op_t* prog, int nprog,
                              const uint8_t* codes, int nterms, const double* effects, int nshots, uint64_t seed,
                              uint64_t run, const double* u, int64_t* plus, double* values, double* norms,
                              uint8_t* outcomes) {
  t_entry = "aqc_mps_traj_pauli_counts";
  AQC_REQUIRE(plus && codes && effects && nprog >= 0 && (prog || nprog == 0), "aqc_mps_traj_pauli_counts: null argument");
  AQC_REQUIRE(n >= 1 && n <= 4096, "aqc_mps_traj_pauli_counts: n must be in 1 .. 4096");
  AQC_REQUIRE(chi_cap >= 1 && chi_cap <= aqc::kMaxCap, "aqc_mps_traj_pauli_counts: chi_cap must be in [1, 1024]");
  AQC_REQUIRE(nterms >= 1 && nterms <= kMaxTerms, "aqc_mps_traj_pauli_counts: nterms must be in 1 .. 65536");
  AQC_REQUIRE(nshots >= 1 && nshots <= kMaxShots, "aqc_mps_traj_pauli_counts: nshots must be in 1 .. 2^30");
  if (int rc = aqc::check_effects(n, effects, t_entry)) return rc;
  // supports, issued by decreasing length so that the long chains start first; last the all-identity
  // term on site 0 (L_0, one identity step, R_1): w
  const int nout = nterms + 1;
  std::vector<int> terms(3 * (size_t)nout);
  double steps = 1.0;
  {
    std::vector<int> lo(nterms), hi(nterms), order(nterms);
    for (int t = 0; t < nterms; ++t) {
      int a = -1, b = -1;
      for (int q = 0; q < n; ++q) {
        const uint8_t c = codes[(size_t)t * n + q];
        if (c > 3) return fail("a Pauli code must be 0 (I), 1 (X), 2 (Y) or 3 (Z)");
        if (c) {
          if (a < 0) a = q;
          b = q;
        }
      }
      if (a < 0) return fail("an all-identity term (its value is 1: the caller answers it)");
      lo[t] = a;
      hi[t] = b;
      steps += (double)(b - a + 1);
    }
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return hi[a] - lo[a] > hi[b] - lo[b]; });
    for (int k = 0; k < nterms; ++k) {
      terms[3 * k] = lo[order[k]];
      terms[3 * k + 1] = hi[order[k]];
      terms[3 * k + 2] = order[k];
    }
    terms[3 * nterms] = terms[3 * nterms + 1] = 0;
    terms[3 * nterms + 2] = nterms;
  }
  // D = E+ - E- of every (qubit, letter)
  std::vector<double> dtab((size_t)n * 12);
  for (size_t qb = 0; qb < (size_t)n * 3; ++qb)
    for (int e = 0; e < 4; ++e) dtab[qb * 4 + e] = effects[qb * 8 + e] - effects[qb * 8 + 4 + e];
  TrajSched sch;
  if (int rc = build_schedule(n, prog, nprog, sch, false)) return rc;
  const int nev = sch.nev, nper = nev + nterms;
  if (u)
    for (size_t e = 0, nu = (size_t)nshots * nper; e < nu; ++e)
      if (!(u[e] >= 0.0 && u[e] < 1.0)) return fail("u must lie in [0, 1)");
  // The batch: B trajectories run the schedule together and are read out R at a time, within the
  // budget less the chains' workspace.  The environments are two dependent n-step chains per state and
  // the Pauli chains one workgroup per (term, state), so a sweep wants many states: R up to 128 (of 16 /
  // 32 / 64 / 128 the fastest on 50 qubits and 297 terms, profiles/mps_trajectory_pauli.json), at most
  // half of what is left, and B takes the rest.
  const size_t cc = (size_t)chi_cap * chi_cap;
  const size_t per_wg = 3 * cc * sizeof(cplx);
  const size_t max_wg = std::max<size_t>(1, std::min<size_t>((size_t)kChainMaxWg, kChainWsBytes / per_wg));
  const size_t budget = kBatchBudgetBytes - max_wg * per_wg;
  const size_t evolve = evolve_state_bytes(sch, n, chi_cap);
  const size_t readout = aqc::env_state_bytes(n, chi_cap) + (size_t)nout * sizeof(double);
  int R = (int)std::max<size_t>(1, std::min<size_t>({(size_t)kPauliReadoutStates, (size_t)nshots, budget / 2 / readout}));
  const size_t left = budget - std::min(budget, (size_t)R * readout);
  int B = (int)std::min<size_t>({(size_t)nshots, (size_t)kMaxBatch, std::max<size_t>(1, left / evolve)});
  if (g_forced_batch > 0) {  // what a forced batch leaves of the budget
    B = std::min(nshots, g_forced_batch);
    const size_t held = std::min(budget, (size_t)B * evolve);
    R = (int)std::max<size_t>(1, std::min<size_t>((size_t)R, (budget - held) / readout));
  }
  R = std::min(R, B);
  if (g_forced_readout > 0) R = std::min(B, g_forced_readout);
  const int nwg = (int)std::min<size_t>(max_wg, (size_t)R * nout);
  Handles hs;
  if (int rc = hs.create(B, n, chi_cap, threshold, max_chi)) return rc;
  hipStream_t st = aqc::mps_stream();
  const size_t ub = u ? up256((size_t)B * nper * sizeof(double)) : 0;
  const size_t cb = up256((size_t)nterms * n);
  const size_t tb = up256(terms.size() * sizeof(int));
  const size_t db = up256(dtab.size() * sizeof(double));
  const size_t pb = up256((size_t)nterms * sizeof(int64_t));
  const size_t vb = values ? up256((size_t)B * nterms * sizeof(double)) : 0;
  const size_t nb8 = norms ? up256((size_t)B * sizeof(double)) : 0;
  const size_t ob = outcomes ? up256((size_t)B * nterms) : 0;
  const size_t sb = up256((size_t)R * sizeof(ChainState));
  const size_t rb = up256((size_t)R * nout * sizeof(double));
  const K2Bufs k2 = k2_bufs(sch, n, B, chi_cap);
  AQC_HIP_CHECK(hipStreamSynchronize(st));  // (the scratch may be regrown)
  aqc::DevScratch& scr = g_scr.here();
  if (int rc = scr.ensure(ub + cb + tb + db + pb + vb + nb8 + ob + sb + rb + up256((size_t)nwg * per_wg) + k2.bytes()))
    return rc;
  char* at = scr.dev;
  auto take = [&](size_t bytes) {
    char* p = at;
    at += bytes;
    return p;
  };
  TrajCtx ctx;
  std::memset(&ctx, 0, sizeof(ctx));
  ctx.seed = seed;
  ctx.run = run;
  ctx.u = u ? (const double*)take(ub) : nullptr;
  ctx.nev = nev;
  ctx.nper = nper;
  ChainJob cj;
  std::memset(&cj, 0, sizeof(cj));
  cj.codes = (const uint8_t*)take(cb);
  cj.terms = (const int*)take(tb);
  cj.dtab = (const double*)take(db);
  cj.n = n;
  cj.cap = chi_cap;
  cj.nterms = nterms;
  PauliDrawJob dj;
  std::memset(&dj, 0, sizeof(dj));
  dj.u = ctx.u;
  dj.plus = (unsigned long long*)take(pb);
  dj.values = values ? (double*)take(vb) : nullptr;
  dj.norms = norms ? (double*)take(nb8) : nullptr;
  dj.outcomes = outcomes ? (uint8_t*)take(ob) : nullptr;
  dj.seed = seed;
  dj.run = run;
  dj.nterms = nterms;
  dj.nev = nev;
  dj.nper = nper;
  cj.states = (const ChainState*)take(sb);
  cj.out = (double*)take(rb);
  cj.ws = (cplx*)take(up256((size_t)nwg * per_wg));
  dj.vals = cj.out;
  if (int rc = k2_bind(sch, k2, take(k2.bytes()), ctx, st)) return rc;
  AQC_HIP_CHECK(hipMemcpyAsync((void*)cj.codes, codes, (size_t)nterms * n, hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemcpyAsync((void*)cj.terms, terms.data(), terms.size() * sizeof(int), hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemcpyAsync((void*)cj.dtab, dtab.data(), dtab.size() * sizeof(double), hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemsetAsync(dj.plus, 0, (size_t)nterms * sizeof(int64_t), st));
  std::vector<std::vector<DevOp>> lists;
  std::vector<ChainState> states(R);
  for (int t0 = 0; t0 < nshots; t0 += B) {
    const int nb = std::min(B, nshots - t0);
    ctx.shot0 = t0;
    if (t0 > 0)
      for (int s = 0; s < nb; ++s)
        if (int rc = aqc::mps_reset_zero(hs.h[s])) return rc;
    if (u)
      AQC_HIP_CHECK(hipMemcpyAsync((void*)ctx.u, u + (size_t)t0 * nper, (size_t)nb * nper * sizeof(double),
                                   hipMemcpyHostToDevice, st));
    if (int rc = run_rows(sch, hs.h.data(), nb, ctx, lists)) return rc;
    for (int r0 = 0; r0 < nb; r0 += R) {
      const int nr = std::min(R, nb - r0);
      // both identity environments of the sweep's states (a Kraus row has broken Vidal form); the call
      // returns with the stream idle, so the host copy of the states is free to be rewritten
      const cplx* lenv = nullptr;
      size_t stride = 0;
      void* extra = nullptr;
      hipStream_t est = nullptr;
      if (int rc = aqc::mps_envs_batch(hs.h.data() + r0, nr, 0, "traj_pauli_env", &lenv, &stride, &extra, &est)) return rc;
      for (int s = 0; s < nr; ++s) {
        const aqc_mps_t h = hs.h[r0 + s];
        states[s].gam = h->d.gam;
        states[s].lam = h->d.lam;
        states[s].dims = h->d.dims;
        states[s].Lenv = lenv + (size_t)s * stride;
        states[s].Renv = states[s].Lenv + (size_t)(n + 1) * cc;
      }
      AQC_HIP_CHECK(hipMemcpyAsync((void*)cj.states, states.data(), (size_t)nr * sizeof(ChainState), hipMemcpyHostToDevice, st));
      cj.nr = nr;
      const size_t items = (size_t)nr * nout;
      // a site of a chain at capacity: 12 chi^2 complex moved, 4 chi^3 complex multiply-adds
      aqc::KernelTimer::begin(st, "mps_traj_pauli_chain", (double)nr * steps * 12.0 * 16.0 * (double)cc,
                              (double)nr * steps * 4.0 * 8.0 * (double)cc * chi_cap);
      hipLaunchKernelGGL(k_mps_traj_pauli_chain, dim3((unsigned)std::min<size_t>((size_t)nwg, items)), dim3(kCT), 0, st, cj);
      aqc::KernelTimer::end(st);
      AQC_CHECK_LAUNCH();
      dj.traj0 = t0 + r0;
      dj.local0 = r0;
      dj.nr = nr;
      // each thread: v, w and u read, a value, a byte and a count written
      aqc::KernelTimer::begin(st, "mps_traj_pauli_draw", (double)nr * nterms * (24.0 + 9.0 + 8.0), 0.0);
      hipLaunchKernelGGL(k_mps_traj_pauli_draw, dim3((nr * nterms + kDT - 1) / kDT), dim3(kDT), 0, st, dj);
      aqc::KernelTimer::end(st);
      AQC_CHECK_LAUNCH();
    }
    if (values)
      AQC_HIP_CHECK(hipMemcpyAsync(values + (size_t)t0 * nterms, dj.values, (size_t)nb * nterms * sizeof(double),
                                   hipMemcpyDeviceToHost, st));
    if (norms) AQC_HIP_CHECK(hipMemcpyAsync(norms + t0, dj.norms, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, st));
    if (outcomes)
      AQC_HIP_CHECK(hipMemcpyAsync(outcomes + (size_t)t0 * nterms, dj.outcomes, (size_t)nb * nterms, hipMemcpyDeviceToHost, st));
    AQC_HIP_CHECK(hipStreamSynchronize(st));  // the next batch overwrites the uniforms and the output rows
  }
  // the table accumulated on the device across the batches
  AQC_HIP_CHECK(hipMemcpyAsync(plus, dj.plus, (size_t)nterms * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  return AQC_OK;
}

}  // extern "C"
