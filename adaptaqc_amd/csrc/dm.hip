// Density-matrix engine: what Aer's method="density_matrix" does under a NoiseModel.  One deterministic
// evolution of rho gives the exact noisy cost 1 - rho_00, every pair's reduced density matrix, every
// Pauli term and the outcome distribution that the trajectory engines (traj.hip, mps_traj.hip) can only
// estimate from shots.
//
// Layout: rho of n <= 13 qubits as 4^n interleaved complex128, entry (r, c) at r + (c << n); r and c are
// little-endian in the qubits.  Bit q of the index is qubit q's row bit, bit n + q its column bit.
// n = 13 is 1 GiB: element indices fit 32 bits, byte offsets do not (size_t at every pointer).
//
// aqc_dm_apply takes aqc_sv_traj_sample's program unchanged: a gate row is rho <- U rho U^dag, a Kraus row
// or group rho <- sum_k K_k rho K_k^dag.  The host plans it in two stages (aqc_dm_plan shows the result):
//   steps     rows on the same one or two qubits fold into one step: a unitary step keeps U (X <- U X U^dag
//             on the 4 or 16 entries that share the other bits), any other is one superoperator S, 4x4 or
//             16x16, on those entries (local index j = r_q + 2 c_q, or (r_q0 + 2 r_q1) + 4 (c_q0 + 2 c_q1);
//             S[j', j] = sum_k K[r', r] conj(K[c', c])).  A row folds into the last step on its qubits when
//             that step covers them; a new two-qubit step also takes in the one-qubit steps that were last
//             on its qubits.  Everything in between acts on other qubits and commutes.  (A one-qubit
//             unitary step runs on the device as its lifted 4x4 S: 16 complex MACs either way.)
//   segments  sv.hip's greedy rule on the steps: a run of steps (reordered only across disjoint qubits)
//             whose qubit set has at most 6 qubits.  The tile is the row and column bits of those qubits,
//             padded with the lowest free qubits: 2 x 6 = 12 bits, 4096 entries, 64 KB of LDS.
// k_dm_segment: one launch per segment.  A workgroup gathers one tile, applies every step of the segment
// in LDS and writes the tile back; the step records (a 16-byte header and 16 or 256 complex words) are
// staged in LDS in chunks with vector loads and read as broadcasts.  For n <= 6 rho is one tile and a
// program is one launch.  A two-qubit superoperator step gives a thread 16 entries and a 16x16 complex
// matrix-vector product on the FP64 vector pipe (gfx950's FP64 matrix cores share its ceiling).
// No atomics and no uniforms anywhere: two calls give the same bits.
//
// Readers (fixed summation order: a thread's terms in index order, a wave butterfly, the waves in
// order): rho_00 and the trace, the diagonal as an n-qubit statevector sqrt(rho_kk) (the statevector
// readers then serve shots, <Z> and probabilities unchanged), Re Tr(M rho) of Pauli terms or of the
// parity operators of a noisy readout (traj.hip's folding into an x mask, a z mask, a scalar and general
// factors, here any number of them: a term reads 2^n 2^ng entries), and the pairs' 4x4 RDMs.
//
// Heisenberg picture (cached_rotations.DMHeisenbergSweep).  aqc_dm_apply_adjoint is X <- Lambda^dag(X): the
// forward plan backwards (segments and the steps inside them in reverse order, U^H for U, S^H for S) through
// the same k_dm_segment; aqc_dm_set, aqc_dm_set_diag and aqc_dm_copy load an observable and checkpoint it.
// k_dm_transition reads two matrices once each into T[j', j] = sum_o conj(A[j', o]) B[j, o] at one qubit's
// local index j = r_q + 2 c_q: Tr(A^H (S_q (x) id)(B)) = sum S[j', j] T[j', j] for any one-qubit
// superoperator S, so every candidate gate at a position, with its error, costs 16 host MACs.  It is the one
// reader spread over workgroups (a partial per workgroup, a second launch adds them in order).
//
// Pair environments (gradients.noisy_general_grad_of_pairs).  A candidate layer on a pair sits directly in
// front of a product measurement (|0><0| on every qubit pulled back through the errors on measure and a
// product starting circuit's inverse: one Hermitian 2x2 effect E_q per qubit), so its noisy cost is linear
// in R = Tr_rest((1 (x) E_rest) rho), the pair's 4x4 block with the other qubits' effects contracted in.
// k_dm_pair_envs reads every pair's R off rho in one launch (spread over workgroups like k_dm_transition,
// the weights prod E_q from two LDS tables); every generator, shift and error is 16x16 host arithmetic.
//
// Pair transitions (gradients.noisy_grads_from_transitions).  k_dm_transition's two-qubit version: for a pair,
// T[j', j] = sum_o conj(A[j', o]) B[j, o] at the pair's local index j = (r_lo + 2 r_hi) + 4 (c_lo + 2 c_hi), o the
// other 2n - 4 index bits, so Tr(A^H (S (x) id)(B)) = sum S[j', j] T[j', j] for any two-qubit superoperator S.
// With A an observable pulled back through any right-hand side and B the state in front of a candidate layer, it
// prices every candidate on the pair, whatever follows it and for either cost.  Per pair a 16 x 16 x 4^(n-2)
// complex GEMM: k_dm_pair_transitions runs it on the FP64 matrix cores (four real v_mfma_f64_16x16x4_f64 per
// four values of o), a wave on a contiguous run of o, a pair spread over workgroups like k_dm_pair_envs.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <vector>

#include "aqc_gemm.h"
#include "aqc_internal.h"
#include "kraus_group.h"
#include "pair_draw.h"

using aqc::cplx;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxQubits = 13;
constexpr int kSegQubits = 6;      // qubits of a tile: 2 x 6 index bits, 4096 entries, 64 KB
constexpr int kStageWords = 768;   // 16-byte words of step records staged at a time (12 KB)
constexpr int kMaxTerms = 65536;
constexpr int kMaxPairs = 4096;

enum { kUnitary = 0, kSuper = 1 };                // a step's kind in aqc_dm_step_t
enum { kRecS1 = 1, kRecU2 = 2, kRecS2 = 3 };      // a device record's kind
constexpr int kWordsBig = 1 + 256;  // a record: the header and 16 or 256 matrix words
static_assert(kWordsBig <= kStageWords, "the largest record fits the staging buffer");

struct DmSegArg {
  int32_t tq[kSegQubits];  // the tile's qubits, ascending
  int32_t word_off, nwords;
};

__device__ __forceinline__ uint32_t insert_zero(uint32_t v, int b) {
  return ((v >> b) << (b + 1)) | (v & ((1u << b) - 1u));
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// The sum of v over the workgroup in a fixed order, returned to every thread; red: one double per wave.
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();  // red is free again
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
  return s;
}

template <int KQ>
__global__ __launch_bounds__(kThreads) void k_dm_segment(cplx* __restrict__ rho, int n, const DmSegArg sa,
                                                         const double2* __restrict__ words) {
  constexpr int TB = 2 * KQ, TILE = 1 << TB;
  constexpr int kPer = TILE >= kThreads ? TILE / kThreads : 1;
  __shared__ cplx tile[TILE];
  __shared__ double2 stage[kStageWords];
  const int tid = threadIdx.x;
  int tb[TB];  // ascending global bit positions: the row bits, then the column bits
#pragma unroll
  for (int j = 0; j < KQ; ++j) {
    tb[j] = sa.tq[j];
    tb[KQ + j] = n + sa.tq[j];
  }
  uint32_t base = blockIdx.x;  // the block's bits scattered into the positions outside the tile
#pragma unroll
  for (int j = 0; j < TB; ++j) base = insert_zero(base, tb[j]);
  uint32_t gidx[kPer];
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const int x = tid + r * kThreads;
    uint32_t g = base;
#pragma unroll
    for (int j = 0; j < TB; ++j) g |= (uint32_t)((x >> j) & 1) << tb[j];
    gidx[r] = g;
    if (x < TILE) tile[x] = rho[(size_t)g];
  }
  int off = sa.word_off;
  const int end = sa.word_off + sa.nwords;
  while (off < end) {
    const int nst = min(kStageWords, end - off);
    __syncthreads();  // the previous chunk's last step has read its matrix
    for (int w = tid; w < nst; w += kThreads) stage[w] = words[(size_t)off + w];
    __syncthreads();
    int p = 0;
    while (p < nst) {
      const int4 hd = *reinterpret_cast<const int4*>(stage + p);  // kind, t0, t1, words (uniform)
      if (p + hd.w > nst) break;  // the record continues past the chunk: restaged from its start
      const cplx* m = reinterpret_cast<const cplx*>(stage + p + 1);
      __syncthreads();  // the previous step's tile writes
      if (hd.x == kRecS1) {
        const int t = hd.y;
        cplx s[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = m[e];
        for (int g = tid; g < (TILE >> 2); g += kThreads) {
          const int b = (int)insert_zero(insert_zero((uint32_t)g, t), KQ + t);
          int idx[4];
          cplx x[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            idx[j] = b | ((j & 1) << t) | ((j >> 1) << (KQ + t));
            x[j] = tile[idx[j]];
          }
#pragma unroll
          for (int o = 0; o < 4; ++o) {
            cplx acc = aqc::cmul(s[4 * o], x[0]);
            acc = aqc::cfma(s[4 * o + 1], x[1], acc);
            acc = aqc::cfma(s[4 * o + 2], x[2], acc);
            acc = aqc::cfma(s[4 * o + 3], x[3], acc);
            tile[idx[o]] = acc;
          }
        }
      } else if constexpr (KQ >= 2) {
        const int t0 = hd.y, t1 = hd.z;
        const int lo = t0 < t1 ? t0 : t1, hi = t0 < t1 ? t1 : t0;
        // local index J = (r0 + 2 r1) + 4 (c0 + 2 c1) of the 16 entries that share the other bits
        auto at = [&](int b, int J) {
          return b | ((J & 1) << t0) | (((J >> 1) & 1) << t1) | (((J >> 2) & 1) << (KQ + t0)) | ((J >> 3) << (KQ + t1));
        };
        for (int g = tid; g < (TILE >> 4); g += kThreads) {
          const int b = (int)insert_zero(insert_zero(insert_zero(insert_zero((uint32_t)g, lo), hi), KQ + lo), KQ + hi);
          cplx x[16];
#pragma unroll
          for (int J = 0; J < 16; ++J) x[J] = tile[at(b, J)];
          if (hd.x == kRecU2) {  // Y = U X U^dag, X[R][C] = x[R + 4 C]
            cplx u[16], t[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) u[e] = m[e];
#pragma unroll
            for (int R = 0; R < 4; ++R)
#pragma unroll
              for (int C = 0; C < 4; ++C) {
                cplx acc = aqc::cmul(u[4 * R], x[4 * C]);
                acc = aqc::cfma(u[4 * R + 1], x[1 + 4 * C], acc);
                acc = aqc::cfma(u[4 * R + 2], x[2 + 4 * C], acc);
                acc = aqc::cfma(u[4 * R + 3], x[3 + 4 * C], acc);
                t[R + 4 * C] = acc;
              }
#pragma unroll
            for (int C = 0; C < 4; ++C)
#pragma unroll
              for (int R = 0; R < 4; ++R) {  // sum_c T[R][c] conj(U[C][c])
                cplx acc = aqc::cmulc(t[R], u[4 * C]);
                acc = aqc::cfmac(u[4 * C + 1], t[R + 4], acc);
                acc = aqc::cfmac(u[4 * C + 2], t[R + 8], acc);
                acc = aqc::cfmac(u[4 * C + 3], t[R + 12], acc);
                tile[at(b, R + 4 * C)] = acc;
              }
          } else {  // kRecS2: 16 outputs of 16 complex MACs, the matrix rows read as LDS broadcasts
#pragma unroll 2
            for (int o = 0; o < 16; ++o) {
              const cplx* row = m + 16 * o;
              cplx acc = aqc::cmul(row[0], x[0]);
#pragma unroll
              for (int J = 1; J < 16; ++J) acc = aqc::cfma(row[J], x[J], acc);
              tile[at(b, o)] = acc;
            }
          }
        }
      }
      p += hd.w;
    }
    if (p == 0) break;  // (a record larger than the buffer: never planned)
    off += p;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const int x = tid + r * kThreads;
    if (x < TILE) rho[(size_t)gidx[r]] = tile[x];
  }
}

__global__ void k_dm_reset(cplx* __restrict__ rho, size_t total) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < total; i += (size_t)gridDim.x * blockDim.x) rho[i] = aqc::cmk(i == 0 ? 1.0 : 0.0, 0.0);
}

// rho = diag(d): the observable of a cost that is linear in the outcome distribution
__global__ void k_dm_set_diag(cplx* __restrict__ rho, int n, const double* __restrict__ d, size_t total) {
  const size_t mask = ((size_t)1 << n) - 1;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i & mask;
    rho[i] = aqc::cmk((i >> n) == r ? d[r] : 0.0, 0.0);
  }
}

// part[block][j' * 4 + j] = sum over the block's o of conj(A[j', o]) B[j, o]: j = r_q + 2 c_q the local
// index of qubit q, o the other 2n - 2 index bits.  Lanes take consecutive o, so a wave's loads are
// contiguous up to the one split that bit q makes in a lane run; a thread's terms add in index order,
// then the wave butterfly and the waves in order (1 or 4 of them).  k_dm_transition_sum adds the blocks
// in order.
__global__ __launch_bounds__(kThreads) void k_dm_transition(const cplx* __restrict__ A, const cplx* __restrict__ B,
                                                            int n, int q, double* __restrict__ part) {
  __shared__ double red[kThreads / 64][32];
  const uint32_t total = 1u << (2 * n - 2);
  double acc[32];
#pragma unroll
  for (int e = 0; e < 32; ++e) acc[e] = 0.0;
  for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < total; o += gridDim.x * blockDim.x) {
    const size_t base = insert_zero(insert_zero(o, q), n + q);
    cplx a[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t at = base | ((size_t)(j & 1) << q) | ((size_t)(j >> 1) << (n + q));
      a[j] = A[at];
      b[j] = B[at];
    }
#pragma unroll
    for (int jp = 0; jp < 4; ++jp)
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // conj(a) b
        acc[2 * (4 * jp + j)] += a[jp].x * b[j].x + a[jp].y * b[j].y;
        acc[2 * (4 * jp + j) + 1] += a[jp].x * b[j].y - a[jp].y * b[j].x;
      }
  }
#pragma unroll
  for (int e = 0; e < 32; ++e) acc[e] = wave_sum(acc[e]);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int e = 0; e < 32; ++e) red[threadIdx.x >> 6][e] = acc[e];
  __syncthreads();
  if (threadIdx.x < 32) {
    double s = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w][threadIdx.x];
    part[(size_t)blockIdx.x * 32 + threadIdx.x] = s;
  }
}

// out[e] = sum_b part[b][e], b ascending (one workgroup of 32 threads)
__global__ void k_dm_transition_sum(const double* __restrict__ part, int nblocks, double* __restrict__ out) {
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s += part[(size_t)b * 32 + threadIdx.x];
  out[threadIdx.x] = s;
}

// out[0] = Re rho_00, out[1] = Re Tr rho (one workgroup)
__global__ __launch_bounds__(kThreads) void k_dm_trace(const cplx* __restrict__ rho, int n, double* __restrict__ out) {
  __shared__ double red[kThreads / 64];
  const uint32_t dim = 1u << n;
  double s = 0.0;
  for (uint32_t k = threadIdx.x; k < dim; k += kThreads) s += rho[(size_t)k + ((size_t)k << n)].x;
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    out[0] = rho[0].x;
    out[1] = s;
  }
}

__global__ void k_dm_diag(const cplx* __restrict__ rho, int n, cplx* __restrict__ sv) {
  const uint32_t dim = 1u << n;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < dim) sv[k] = aqc::cmk(sqrt(fmax(0.0, rho[(size_t)k + ((size_t)k << n)].x)), 0.0);
}

// A term as the reader takes it: M = (cr + i ci) P (x) G as traj.hip's PauliTerm, with up to 13 general
// factors g[a] = (D00, D11, Re D01, Im D01) on qubits gq[a].
struct DmTerm {
  uint32_t x, z;
  int32_t ng, gq[kMaxQubits];
  int32_t pad;
  double cr, ci;
  double g[kMaxQubits][4];
};
static_assert(sizeof(DmTerm) % 8 == 0, "DmTerm layout");

// out[t] = Re Tr(M_t rho) = Re sum_k sum_l M[k, l] rho[l, k]: a workgroup per term, row k of M per thread
__global__ __launch_bounds__(kThreads) void k_dm_pauli(const cplx* __restrict__ rho, int n,
                                                       const DmTerm* __restrict__ terms, double* __restrict__ out) {
  __shared__ double red[kThreads / 64];
  const DmTerm& tm = terms[blockIdx.x];
  const uint32_t dim = 1u << n, x = tm.x, z = tm.z;
  const int ng = tm.ng;
  uint32_t gmask = 0;
  for (int f = 0; f < ng; ++f) gmask |= 1u << tm.gq[f];
  double sx = 0.0, sy = 0.0;
  for (uint32_t k = threadIdx.x; k < dim; k += kThreads) {
    const uint32_t lbase = (k ^ x) & ~gmask;
    const cplx* col = rho + ((size_t)k << n);
    cplx acc = aqc::cmk(0.0, 0.0);
    for (uint32_t a = 0; a < (1u << ng); ++a) {
      uint32_t l = lbase;
      cplx w = aqc::cmk(1.0, 0.0);
      for (int f = 0; f < ng; ++f) {
        const int q = tm.gq[f];
        const bool kb = (k >> q) & 1, ab = (a >> f) & 1;
        l |= (uint32_t)ab << q;
        const double* g = tm.g[f];  // D[k_f, a_f]; D10 = conj(D01)
        const cplx d = kb == ab ? aqc::cmk(kb ? g[1] : g[0], 0.0) : aqc::cmk(g[2], kb ? -g[3] : g[3]);
        w = aqc::cmul(w, d);
      }
      acc = aqc::cfma(w, col[l], acc);
    }
    const double sg = (__popc(k & z) & 1) ? -1.0 : 1.0;
    sx += sg * acc.x;
    sy += sg * acc.y;
  }
  sx = block_sum(sx, red);
  sy = block_sum(sy, red);
  if (threadIdx.x == 0) out[blockIdx.x] = tm.cr * sx - tm.ci * sy;
}

// out[p][a][b] = sum_rest rho[(a, rest), (b, rest)], index 2 bit_hi + bit_lo: a workgroup per pair
__global__ __launch_bounds__(kThreads) void k_dm_pair_rdms(const cplx* __restrict__ rho, int n,
                                                           const int* __restrict__ pairs, cplx* __restrict__ out) {
  __shared__ double red[kThreads / 64][32];
  const int p = blockIdx.x;
  const int lo = min(pairs[2 * p], pairs[2 * p + 1]), hi = max(pairs[2 * p], pairs[2 * p + 1]);
  const uint32_t rest = 1u << (n - 2);
  double acc[32];
#pragma unroll
  for (int e = 0; e < 32; ++e) acc[e] = 0.0;
  for (uint32_t r = threadIdx.x; r < rest; r += kThreads) {
    const uint32_t b = insert_zero(insert_zero(r, lo), hi);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const size_t colbase = (size_t)(b | ((uint32_t)(c & 1) << lo) | ((uint32_t)(c >> 1) << hi)) << n;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const cplx v = rho[colbase + (b | ((uint32_t)(a & 1) << lo) | ((uint32_t)(a >> 1) << hi))];
        acc[2 * (4 * a + c)] += v.x;
        acc[2 * (4 * a + c) + 1] += v.y;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 32; ++e) acc[e] = wave_sum(acc[e]);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int e = 0; e < 32; ++e) red[threadIdx.x >> 6][e] = acc[e];
  __syncthreads();
  if (threadIdx.x < 16) {
    double sx = 0.0, sy = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) {
      sx += red[w][2 * threadIdx.x];
      sy += red[w][2 * threadIdx.x + 1];
    }
    out[(size_t)p * 16 + threadIdx.x] = aqc::cmk(sx, sy);
  }
}

// ---- pair environments ---------------------------------------------------------------------------------
// R_p[a][b] = sum_{r, r'} rho[(a, r), (b, r')] prod_{q not in p} E_q[r'_q, r_q]: the pair's 4x4 block of rho
// with the other qubits' effects contracted in.  r is the rest index (the n - 2 other qubits' row bits in
// qubit order); r' differs from r only on the rest qubits whose effect has an off-diagonal (the mask gm in
// rest bits, ng of them), so an item is (r, a), a < 2^ng, and a pair has 2^(n-2+ng) items of 16 entries.
constexpr int kEnvMaxSplit = 256;  // workgroups of one pair

// the workgroups a pair's items are spread over: an item per thread until 256 workgroups share the pair
__host__ __device__ inline int env_split(int m, int ng) {
  const int bits = m + ng - 8;  // log2(items / 256)
  return bits <= 0 ? 1 : (bits >= 8 ? kEnvMaxSplit : 1 << bits);
}

// bit i of a to the position of the i-th set bit of mask
__device__ __forceinline__ uint32_t deposit(uint32_t a, uint32_t mask) {
  uint32_t out = 0;
  while (mask) {
    const uint32_t b = mask & (0u - mask);
    if (a & 1u) out |= b;
    a >>= 1;
    mask ^= b;
  }
  return out;
}

// E[rp, r] of an effect g = (E00, E11, Re E01, Im E01); E10 = conj(E01)
__device__ __forceinline__ cplx effect_at(const double* g, int rp, int r) {
  return rp == r ? aqc::cmk(r ? g[1] : g[0], 0.0) : aqc::cmk(g[2], rp ? -g[3] : g[3]);
}

// part[(p * gridDim.x + s) * 32 ..]: workgroup s's share of pair p as 16 (re, im), index 4 a + b.  The weight
// of an item is one product of two table entries: the rest bits split into a low half of hl = ceil(m / 2)
// bits and a high half, each with its table in the LDS at (r_half, r'_half), of which only the entries that
// can occur (2^(h + ng_half)) are filled.  Lanes take consecutive r: a wave's 16 loads are each contiguous
// up to the splits the pair's two bits make.  A thread's items add in index order, then the wave butterfly
// and the waves in order; k_dm_pair_envs_sum adds a pair's workgroups in order.
__global__ __launch_bounds__(kThreads) void k_dm_pair_envs(const cplx* __restrict__ rho, int n,
                                                           const int* __restrict__ pairs,
                                                           const double* __restrict__ eff, uint32_t offdiag,
                                                           double* __restrict__ part) {
  extern __shared__ double2 env_tab[];
  __shared__ double red[kThreads / 64][32];
  const int p = blockIdx.y;
  const int lo = min(pairs[2 * p], pairs[2 * p + 1]), hi = max(pairs[2 * p], pairs[2 * p + 1]);
  const int m = n - 2, hl = (m + 1) >> 1, hh = m - hl;
  // the qubit mask of the off-diagonals squeezed into rest bits
  const uint32_t below_hi = (1u << hi) - 1u, below_lo = (1u << lo) - 1u;
  uint32_t gm = ((offdiag >> (hi + 1)) << hi) | (offdiag & below_hi);
  gm = ((gm >> (lo + 1)) << lo) | (gm & below_lo);
  const int ng = __popc(gm);
  const int nsplit = env_split(m, ng);
  if ((int)blockIdx.x >= nsplit) return;  // (uniform: before any barrier)
  cplx* tlo = reinterpret_cast<cplx*>(env_tab);
  cplx* thi = tlo + ((size_t)1 << (2 * hl));
  for (int half = 0; half < 2; ++half) {
    const int h = half ? hh : hl, j0 = half ? hl : 0;
    const uint32_t hmask = (1u << h) - 1u, gmh = (gm >> j0) & hmask;
    cplx* tab = half ? thi : tlo;
    const uint32_t count = 1u << (h + __popc(gmh));
    for (uint32_t e = threadIdx.x; e < count; e += kThreads) {
      const uint32_t rh = e & hmask, rph = (rh & ~gmh) | deposit(e >> h, gmh);
      cplx w = aqc::cmk(1.0, 0.0);
      for (int j = 0; j < h; ++j) {
        int q = j0 + j;  // the rest bit's qubit: past the pair's two
        q += q >= lo;
        q += q >= hi;
        w = aqc::cmul(w, effect_at(eff + 4 * q, (rph >> j) & 1, (rh >> j) & 1));
      }
      tab[rh | (rph << h)] = w;
    }
  }
  __syncthreads();
  const uint32_t items = 1u << (m + ng), chunk = items / (uint32_t)nsplit;
  const uint32_t w0 = blockIdx.x * chunk, rmask = (1u << m) - 1u, lmask = (1u << hl) - 1u;
  double acc[32];
#pragma unroll
  for (int e = 0; e < 32; ++e) acc[e] = 0.0;
  for (uint32_t w = w0 + threadIdx.x; w < w0 + chunk; w += kThreads) {
    const uint32_t r = w & rmask, rp = (r & ~gm) | deposit(w >> m, gm);
    const cplx wt = aqc::cmul(tlo[(r & lmask) | ((rp & lmask) << hl)], thi[(r >> hl) | ((rp >> hl) << hh)]);
    const uint32_t brow = insert_zero(insert_zero(r, lo), hi), bcol = insert_zero(insert_zero(rp, lo), hi);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const size_t colbase = (size_t)(bcol | ((uint32_t)(c & 1) << lo) | ((uint32_t)(c >> 1) << hi)) << n;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const cplx v = rho[colbase + (brow | ((uint32_t)(a & 1) << lo) | ((uint32_t)(a >> 1) << hi))];
        acc[2 * (4 * a + c)] += wt.x * v.x - wt.y * v.y;
        acc[2 * (4 * a + c) + 1] += wt.x * v.y + wt.y * v.x;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 32; ++e) acc[e] = wave_sum(acc[e]);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int e = 0; e < 32; ++e) red[threadIdx.x >> 6][e] = acc[e];
  __syncthreads();
  if (threadIdx.x < 32) {
    double s = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) s += red[w][threadIdx.x];
    part[((size_t)p * gridDim.x + blockIdx.x) * 32 + threadIdx.x] = s;
  }
}

// out[p][e] = sum_s part[p][s][e] over the pair's own workgroups, s ascending (a workgroup of 32 per pair)
__global__ void k_dm_pair_envs_sum(const double* __restrict__ part, int n, const int* __restrict__ pairs,
                                   uint32_t offdiag, int stride, double* __restrict__ out) {
  const int p = blockIdx.x;
  const uint32_t own = (1u << pairs[2 * p]) | (1u << pairs[2 * p + 1]);
  const int nsplit = env_split(n - 2, __popc(offdiag & ~own));
  double s = 0.0;
  for (int b = 0; b < nsplit; ++b) s += part[((size_t)p * stride + b) * 32 + threadIdx.x];
  out[(size_t)p * 32 + threadIdx.x] = s;
}

// ---- pair transitions ----------------------------------------------------------------------------------
// T_p[j'][j] = sum_o conj(A[j', o]) B[j, o]: j = (r_lo + 2 r_hi) + 4 (c_lo + 2 c_hi) the pair's local index (index
// bits lo, hi, n + lo, n + hi), o the other 2n - 4 index bits in ascending order, K = 4^(n-2) values.
constexpr int kTransMaxSplit = 256;   // workgroups of one pair
constexpr int kTransUnroll = 4;       // MFMA steps (of 4 values of o) whose operands are requested together
constexpr int kTransMaxGroups = 8192; // workgroups of one launch that write a partial (4 KB each)

// the workgroups a pair's K values of o are spread over: 256 values (64 a wave) each until 256 workgroups
// share the pair; fewer when the pairs alone fill the device (the partials stay within 32 MB)
inline int trans_split(int n, int npairs) {
  const int bits = 2 * (n - 2) - 8;  // log2(K / 256)
  int split = bits <= 0 ? 1 : (bits >= 8 ? kTransMaxSplit : 1 << bits);
  while (split > 1 && (long long)split * npairs > kTransMaxGroups) split >>= 1;
  return split;
}

// part[(p * gridDim.x + s) * 256 + 16 j' + j]: workgroup s's share of pair p.  The workgroup's K / gridDim.x
// values of o go to its waves as contiguous runs (at least 4: with K < 16 only the first waves have work).  A
// step is one 16 x 16 x 4 product: lane l feeds (j' = l & 15, o = o0 + (l >> 4)) of A and the same entry of B (the
// MFMA's A operand is [m = l & 15][k = l >> 4], its B operand [k = l >> 4][n = l & 15]); Re T accumulates
// ar br + ai bi, Im T ar bi - ai br, as four real MFMAs into two accumulators.  A lane whose o is past the run's
// end feeds zeros.  A wave walks its run upwards, kTransUnroll steps (16 consecutive o) requested at once: for
// each of the 16 values of j the 16 entries are one contiguous run of index space wherever the pair's bits
// leave one (256 B when lo >= 4; with lo < 4 the run breaks at bit lo and the neighbouring j fill the gap), so
// every cache line a wave touches is used up by that iteration or the next and never revisited.
// The result tile holds T[(l >> 4) + 4 reg][l & 15]; the waves' tiles add in order in the LDS, and
// k_dm_pair_transitions_sum adds a pair's workgroups in order.
__global__ __launch_bounds__(kThreads) void k_dm_pair_transitions(const cplx* __restrict__ A,
                                                                  const cplx* __restrict__ B, int n,
                                                                  const int* __restrict__ pairs,
                                                                  cplx* __restrict__ part) {
  __shared__ double red[kThreads / 64][8][64];
  const int p = blockIdx.y;
  const int lo = min(pairs[2 * p], pairs[2 * p + 1]), hi = max(pairs[2 * p], pairs[2 * p + 1]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  const uint32_t K = 1u << (2 * n - 4), chunk = K / gridDim.x;  // (gridDim.x is a power of two <= K)
  const uint32_t run = max(4u, chunk / (uint32_t)(kThreads / 64));
  const uint32_t w0 = blockIdx.x * chunk;
  const uint32_t begin = min(w0 + (uint32_t)wave * run, w0 + chunk), end = min(begin + run, w0 + chunk);
  const uint32_t jbits = ((uint32_t)(li & 1) << lo) | ((uint32_t)((li >> 1) & 1) << hi) |
                         ((uint32_t)((li >> 2) & 1) << (n + lo)) | ((uint32_t)(li >> 3) << (n + hi));
  aqc::d4_t sr = {0, 0, 0, 0}, si = {0, 0, 0, 0};
  for (uint32_t o0 = begin; o0 < end; o0 += 4 * kTransUnroll) {  // (uniform per wave)
    cplx a[kTransUnroll], b[kTransUnroll];
#pragma unroll
    for (int s = 0; s < kTransUnroll; ++s) {
      const uint32_t o = o0 + 4 * s + lk;
      a[s] = b[s] = aqc::cmk(0.0, 0.0);
      if (o < end) {
        const size_t at = insert_zero(insert_zero(insert_zero(insert_zero(o, lo), hi), n + lo), n + hi) | jbits;
        a[s] = A[at];
        b[s] = B[at];
      }
    }
#pragma unroll
    for (int s = 0; s < kTransUnroll; ++s) {
      sr = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s].x, b[s].x, sr, 0, 0, 0);
      si = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s].x, b[s].y, si, 0, 0, 0);
      sr = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s].y, b[s].y, sr, 0, 0, 0);
      si = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[s].y, b[s].x, si, 0, 0, 0);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    red[wave][q][lane] = sr[q];
    red[wave][4 + q][lane] = si[q];
  }
  __syncthreads();
  const int e = threadIdx.x, jp = e >> 4, src = ((jp & 3) << 4) | (e & 15), reg = jp >> 2;
  double x = 0.0, y = 0.0;
  for (int w = 0; w < kThreads / 64; ++w) {
    x += red[w][reg][src];
    y += red[w][4 + reg][src];
  }
  part[((size_t)p * gridDim.x + blockIdx.x) * 256 + e] = aqc::cmk(x, y);
}

// out[p][e] = sum_s part[p][s][e], s ascending (a workgroup of 256 per pair)
__global__ void k_dm_pair_transitions_sum(const cplx* __restrict__ part, int split, cplx* __restrict__ out) {
  const int p = blockIdx.x;
  double x = 0.0, y = 0.0;
  for (int s = 0; s < split; ++s) {
    const cplx v = part[((size_t)p * split + s) * 256 + threadIdx.x];
    x += v.x;
    y += v.y;
  }
  out[(size_t)p * 256 + threadIdx.x] = aqc::cmk(x, y);
}

// ---- host planning -----------------------------------------------------------------------------------
typedef std::complex<double> hcx;
typedef std::vector<hcx> hmat;

thread_local const char* t_entry = "aqc_dm_apply";

int fail(const std::string& msg) {
  aqc::set_error(std::string(t_entry) + ": " + msg);
  return AQC_ERR_ARG;
}

// a program row or group: a gate (one operator) or a channel's Kraus operators on one or two qubits
struct Event {
  int nq, q0, q1, nk;
  bool gate;
  const double* m[16];
};

// The argument checks of aqc_sv_traj_sample's build_rows (traj.hip), in its words.
int parse_events(int n, const aqc_op_t* prog, int nprog, std::vector<Event>& evs) {
  evs.clear();
  for (int i = 0; i < nprog; ++i) {
    const aqc_op_t& op = prog[i];
    Event e;
    std::memset(&e, 0, sizeof(e));
    if (op.flags == 0) {
      if (!(op.nq == 1 || op.nq == 2) || op.q0 < 0 || op.q0 >= n) return fail("gate row: bad qubits");
      if (op.nq == 2 && (op.q1 < 0 || op.q1 >= n || op.q1 == op.q0)) return fail("gate row: bad qubits");
      for (int c = 0; c < (op.nq == 1 ? 8 : 32); ++c)
        if (!std::isfinite(op.m[c])) return fail("gate row: a matrix entry is not finite");
      e.nq = op.nq, e.q0 = op.q0, e.q1 = op.nq == 2 ? op.q1 : 0, e.nk = 1, e.gate = true;
      e.m[0] = op.m;
    } else if (op.flags == AQC_OP_KRAUS1) {
      if (op.nq != 1 || op.q0 < 0 || op.q0 >= n || op.q1 < 1 || op.q1 > 4) return fail("malformed Kraus row");
      double s00 = 0.0, s11 = 0.0, sx = 0.0, sy = 0.0;
      for (int k = 0; k < op.q1; ++k) {
        const double* K = op.m + 8 * k;  // K00 K01 K10 K11 as (re, im)
        for (int c = 0; c < 8; ++c)
          if (!std::isfinite(K[c])) return fail("malformed Kraus row");
        s00 += K[0] * K[0] + K[1] * K[1] + K[4] * K[4] + K[5] * K[5];
        s11 += K[2] * K[2] + K[3] * K[3] + K[6] * K[6] + K[7] * K[7];
        sx += K[0] * K[2] + K[1] * K[3] + K[4] * K[6] + K[5] * K[7];
        sy += K[0] * K[3] - K[1] * K[2] + K[4] * K[7] - K[5] * K[6];
        e.m[k] = K;
      }
      if (std::fabs(s00 - 1.0) > 1e-9 || std::fabs(s11 - 1.0) > 1e-9 || std::fabs(sx) > 1e-9 || std::fabs(sy) > 1e-9)
        return fail("Kraus row: sum K^dag K is not the identity");
      e.nq = 1, e.q0 = op.q0, e.nk = op.q1, e.gate = false;
    } else if ((op.flags & 0xff) == AQC_OP_KRAUS2) {
      const int nk = (op.flags >> 16) & 0xff;
      if (const char* why = aqc::kraus2_first_row_error(op, n, nprog - i)) return fail(why);
      double w[16][16];
      bool flat = true;
      if (const char* why = aqc::kraus2_group_error(prog + i, nk, w, &flat)) return fail(why);
      e.nq = 2, e.q0 = op.q0, e.q1 = op.q1, e.nk = nk, e.gate = false;
      for (int k = 0; k < nk; ++k) e.m[k] = prog[i + k].m;
      i += nk - 1;
    } else {
      return fail("unknown row flags");
    }
    evs.push_back(e);
  }
  return AQC_OK;
}

struct HStep {
  int nq = 1, q0 = 0, q1 = 0, seg = 0;
  bool unitary = true, dead = false;
  hmat U, S;  // d x d while unitary, else d^2 x d^2 (d = 2^nq), row-major
};

hmat identity(int d) {
  hmat m((size_t)d * d, hcx(0.0, 0.0));
  for (int i = 0; i < d; ++i) m[(size_t)i * d + i] = hcx(1.0, 0.0);
  return m;
}

hmat matmul(const hmat& a, const hmat& b, int d) {  // a b
  hmat c((size_t)d * d, hcx(0.0, 0.0));
  for (int i = 0; i < d; ++i)
    for (int k = 0; k < d; ++k) {
      const hcx aik = a[(size_t)i * d + k];
      if (aik == hcx(0.0, 0.0)) continue;
      for (int j = 0; j < d; ++j) c[(size_t)i * d + j] += aik * b[(size_t)k * d + j];
    }
  return c;
}

// S[r' + d c', r + d c] += K[r', r] conj(K[c', c])
void add_lift(const hmat& K, int d, hmat& S) {
  const int D = d * d;
  for (int cp = 0; cp < d; ++cp)
    for (int rp = 0; rp < d; ++rp)
      for (int c = 0; c < d; ++c)
        for (int r = 0; r < d; ++r) S[(size_t)(rp + d * cp) * D + (r + d * c)] += K[(size_t)rp * d + r] * std::conj(K[(size_t)cp * d + c]);
}

hmat lift(const hmat& K, int d) {
  hmat S((size_t)d * d * d * d, hcx(0.0, 0.0));
  add_lift(K, d, S);
  return S;
}

// a 2x2 operator on bit `pos` of the two-qubit index b0 + 2 b1
hmat embed_op(const hmat& a, int pos) {
  hmat m(16, hcx(0.0, 0.0));
  for (int ip = 0; ip < 4; ++ip)
    for (int i = 0; i < 4; ++i) {
      const int other = 1 - pos;
      if (((ip >> other) & 1) != ((i >> other) & 1)) continue;
      m[(size_t)ip * 4 + i] = a[(size_t)((ip >> pos) & 1) * 2 + ((i >> pos) & 1)];
    }
  return m;
}

// a one-qubit superoperator (index r + 2 c) on qubit `pos` of the two-qubit index (r0 + 2 r1) + 4 (c0 + 2 c1)
hmat embed_super(const hmat& s, int pos) {
  hmat m(256, hcx(0.0, 0.0));
  const int other = 1 - pos;
  for (int Jp = 0; Jp < 16; ++Jp)
    for (int J = 0; J < 16; ++J) {
      if (((Jp >> other) & 1) != ((J >> other) & 1) || ((Jp >> (2 + other)) & 1) != ((J >> (2 + other)) & 1)) continue;
      const int jp = ((Jp >> pos) & 1) + 2 * ((Jp >> (2 + pos)) & 1), j = ((J >> pos) & 1) + 2 * ((J >> (2 + pos)) & 1);
      m[(size_t)Jp * 16 + J] = s[(size_t)jp * 4 + j];
    }
  return m;
}

// operator k of event e as a d x d matrix in the frame of a step on (q0, q1)
hmat event_op(const Event& e, int k, const HStep& st) {
  const int de = 1 << e.nq;
  hmat a((size_t)de * de);
  for (int c = 0; c < de * de; ++c) a[c] = hcx(e.m[k][2 * c], e.m[k][2 * c + 1]);
  if (st.nq == 1) return a;
  if (e.nq == 1) return embed_op(a, e.q0 == st.q0 ? 0 : 1);
  if (e.q0 == st.q0) return a;
  hmat b(16);  // the event lists the qubits the other way round: exchange the index bits
  auto sw = [](int i) { return ((i & 1) << 1) | (i >> 1); };
  for (int ip = 0; ip < 4; ++ip)
    for (int i = 0; i < 4; ++i) b[(size_t)ip * 4 + i] = a[(size_t)sw(ip) * 4 + sw(i)];
  return b;
}

// step <- op o step, op given as a unitary (opU) or a superoperator (opS) in the step's frame
void compose(HStep& st, bool op_unitary, const hmat& opU, const hmat& opS) {
  const int d = 1 << st.nq;
  if (op_unitary && st.unitary) {
    st.U = matmul(opU, st.U, d);
    return;
  }
  if (st.unitary) {
    st.S = lift(st.U, d);
    st.unitary = false;
  }
  st.S = matmul(op_unitary ? lift(opU, d) : opS, st.S, d * d);
}

void fold_event(HStep& st, const Event& e) {
  const int d = 1 << st.nq;
  if (e.gate) {
    compose(st, true, event_op(e, 0, st), hmat());
    return;
  }
  hmat S((size_t)d * d * d * d, hcx(0.0, 0.0));
  for (int k = 0; k < e.nk; ++k) add_lift(event_op(e, k, st), d, S);
  compose(st, false, hmat(), S);
}

struct Plan {
  std::vector<HStep> steps;      // in execution order: by segment, then in the segment's order
  std::vector<DmSegArg> segs;
  std::vector<double> words;     // the device records, 2 doubles a word
  int kq = 1;
};

void push_record(std::vector<double>& words, int kind, int t0, int t1, const hmat& m, int nmat) {
  int32_t hd[4] = {kind, t0, t1, 1 + nmat};
  double w[2];
  std::memcpy(w, hd, sizeof(w));
  words.push_back(w[0]);
  words.push_back(w[1]);
  for (int c = 0; c < nmat; ++c) {
    words.push_back(m[c].real());
    words.push_back(m[c].imag());
  }
}

hmat dagger(const hmat& m, int d) {
  hmat o((size_t)d * d);
  for (int i = 0; i < d; ++i)
    for (int j = 0; j < d; ++j) o[(size_t)i * d + j] = std::conj(m[(size_t)j * d + i]);
  return o;
}

// adjoint: the plan of the adjoint map X <- Lambda^dag(X).  The forward plan's segments in reverse order,
// each segment's steps in reverse order, every U replaced by U^H and every S by S^H (the adjoint of x <- S x
// under Tr(A^H B) in the same local index); tiles and records are the forward plan's.
int build_plan(int n, const aqc_op_t* prog, int nprog, Plan& plan, bool adjoint = false) {
  std::vector<Event> evs;
  if (int rc = parse_events(n, prog, nprog, evs)) return rc;
  // ---- steps ----
  std::vector<HStep> steps;
  std::vector<int> last(n, -1);  // the last step on each qubit
  for (const Event& e : evs) {
    const int s = last[e.q0];
    const bool same = s >= 0 && (e.nq == 1 || last[e.q1] == s);
    if (same && (e.nq == 1 || steps[s].nq == 2)) {  // the step covers the event's qubits: fold
      fold_event(steps[s], e);
      continue;
    }
    HStep st;
    st.nq = e.nq, st.q0 = e.q0, st.q1 = e.nq == 2 ? e.q1 : 0;
    st.U = identity(1 << e.nq);
    if (e.nq == 2)
      for (int pos = 0; pos < 2; ++pos) {  // take in the one-qubit steps that were last on the two qubits
        const int o = last[pos == 0 ? e.q0 : e.q1];
        if (o < 0 || steps[o].nq != 1) continue;
        HStep& os = steps[o];
        if (os.unitary) compose(st, true, embed_op(os.U, pos), hmat());
        else compose(st, false, hmat(), embed_super(os.S, pos));
        os.dead = true;
      }
    fold_event(st, e);
    last[e.q0] = (int)steps.size();
    if (e.nq == 2) last[e.q1] = (int)steps.size();
    steps.push_back(std::move(st));
  }
  std::vector<HStep> live;
  for (HStep& st : steps)
    if (!st.dead) live.push_back(std::move(st));
  // ---- segments: sv.hip's greedy rule on the steps ----
  const int kq = std::min(n, kSegQubits);
  plan.kq = kq;
  const int ns = (int)live.size();
  std::vector<char> done(ns, 0);
  std::vector<uint32_t> seg_mask;
  std::vector<std::vector<int>> seg_steps;
  int remaining = ns, first = 0;
  while (remaining > 0) {
    while (first < ns && done[first]) ++first;
    uint32_t qmask = 0, blocked = 0;
    std::vector<int> mine;
    for (int i = first; i < ns; ++i) {
      if (done[i]) continue;
      uint32_t gm = 1u << live[i].q0;
      if (live[i].nq == 2) gm |= 1u << live[i].q1;
      if ((gm & blocked) || __builtin_popcount(qmask | gm) > kq) {
        blocked |= gm;
      } else {
        qmask |= gm;
        mine.push_back(i);
        done[i] = 1;
        --remaining;
      }
      if (__builtin_popcount(blocked) >= n) break;
    }
    for (int b = 0; b < n && __builtin_popcount(qmask) < kq; ++b) qmask |= 1u << b;  // the lowest free qubits
    seg_mask.push_back(qmask);
    seg_steps.push_back(std::move(mine));
  }
  if (adjoint) {
    std::reverse(seg_mask.begin(), seg_mask.end());
    std::reverse(seg_steps.begin(), seg_steps.end());
    for (std::vector<int>& mine : seg_steps) std::reverse(mine.begin(), mine.end());
    for (HStep& st : live) {
      const int d = 1 << st.nq;
      if (st.unitary) st.U = dagger(st.U, d);
      else st.S = dagger(st.S, d * d);
    }
  }
  std::vector<int> order;
  for (size_t seg = 0; seg < seg_steps.size(); ++seg) {
    DmSegArg sa;
    std::memset(&sa, 0, sizeof(sa));
    int local_of[32], cnt = 0;
    for (int b = 0; b < n; ++b)
      if ((seg_mask[seg] >> b) & 1u) {
        sa.tq[cnt] = b;
        local_of[b] = cnt++;
      }
    sa.word_off = (int)(plan.words.size() / 2);
    for (int i : seg_steps[seg]) {
      HStep& st = live[i];
      st.seg = (int)seg;
      if (st.nq == 1) push_record(plan.words, kRecS1, local_of[st.q0], 0, st.unitary ? lift(st.U, 2) : st.S, 16);
      else if (st.unitary) push_record(plan.words, kRecU2, local_of[st.q0], local_of[st.q1], st.U, 16);
      else push_record(plan.words, kRecS2, local_of[st.q0], local_of[st.q1], st.S, 256);
      order.push_back(i);
    }
    sa.nwords = (int)(plan.words.size() / 2) - sa.word_off;
    plan.segs.push_back(sa);
  }
  plan.steps.reserve(ns);
  for (int i : order) plan.steps.push_back(std::move(live[i]));
  return AQC_OK;
}

// The term records from the codes and, when not null, the effects (traj.hip's build_terms restated with
// no limit on the general factors): per qubit of the support D = E[q][c-1][0] - E[q][c-1][1], a multiple
// of a Pauli matrix within 1e-14 into the masks and the scalar, any other into the general factors.
int build_terms(int n, const uint8_t* codes, int nterms, const double* effects, std::vector<DmTerm>& terms) {
  constexpr double tol = 1e-14;
  static const double pauli_d[3][4] = {{0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, -1.0}, {1.0, -1.0, 0.0, 0.0}};
  terms.assign((size_t)nterms, DmTerm());
  for (int t = 0; t < nterms; ++t) {
    DmTerm& tm = terms[t];
    std::memset(&tm, 0, sizeof(tm));
    double scal = 1.0;
    int ny = 0, weight = 0;
    for (int q = 0; q < n; ++q) {
      const int c = codes[(size_t)t * n + q];
      if (c > 3) return fail("a Pauli code must be 0 (I), 1 (X), 2 (Y) or 3 (Z)");
      if (c == 0) continue;
      ++weight;
      double d[4];
      if (effects) {
        const double* e0 = effects + (size_t)((q * 3 + c - 1) * 2) * 4;
        for (int i = 0; i < 4; ++i) d[i] = e0[i] - e0[4 + i];
      } else {
        std::memcpy(d, pauli_d[c - 1], sizeof(d));
      }
      const bool diag0 = std::fabs(d[0]) <= tol && std::fabs(d[1]) <= tol;
      if (diag0 && std::fabs(d[3]) <= tol) {  // d[2] X
        scal *= d[2];
        tm.x |= 1u << q;
      } else if (diag0 && std::fabs(d[2]) <= tol) {  // -d[3] Y: Y01 = -i
        scal *= -d[3];
        tm.x |= 1u << q;
        tm.z |= 1u << q;
        ++ny;
      } else if (std::fabs(d[0] + d[1]) <= tol && std::fabs(d[2]) <= tol && std::fabs(d[3]) <= tol) {  // d[0] Z
        scal *= d[0];
        tm.z |= 1u << q;
      } else {
        tm.gq[tm.ng] = q;
        std::memcpy(tm.g[tm.ng], d, sizeof(d));
        ++tm.ng;
      }
    }
    if (weight == 0) return fail("an all-identity term (its value is Tr rho: the caller answers it)");
    static const double ph[4][2] = {{1.0, 0.0}, {0.0, -1.0}, {-1.0, 0.0}, {0.0, 1.0}};  // (-i)^ny
    tm.cr = scal * ph[ny & 3][0];
    tm.ci = scal * ph[ny & 3][1];
  }
  return AQC_OK;
}

}  // namespace

struct aqc_dm_s {
  int n = 0;
  cplx* rho = nullptr;
  hipStream_t stream = nullptr;
  char* d_buf = nullptr;  // grow-only: the plan's records, or a reader's arguments and results
  size_t buf_cap = 0;
};

namespace {

int dm_buf(aqc_dm_t h, size_t bytes, char** out) {
  if (bytes > h->buf_cap) {
    AQC_HIP_CHECK(hipStreamSynchronize(h->stream));
    if (h->d_buf) AQC_HIP_CHECK(hipFree(h->d_buf));
    h->d_buf = nullptr;
    h->buf_cap = 0;
    const size_t cap = std::max(aqc::up256(bytes), (size_t)1 << 16);
    AQC_HIP_CHECK(hipMalloc(&h->d_buf, cap));
    h->buf_cap = cap;
  }
  *out = h->d_buf;
  return AQC_OK;
}

template <int KQ>
void launch_segment(aqc_dm_t h, const DmSegArg& sa, const double2* words) {
  const unsigned grid = 1u << (2 * (h->n - KQ));
  hipLaunchKernelGGL(k_dm_segment<KQ>, dim3(grid), dim3(kThreads), 0, h->stream, h->rho, h->n, sa, words);
}

}  // namespace

extern "C" {

int aqc_dm_create(int n, aqc_dm_t* out) {
  AQC_REQUIRE(out != nullptr, "aqc_dm_create: null out");
  AQC_REQUIRE(n >= 1 && n <= kMaxQubits, "aqc_dm_create: n must be in 1 .. 13");
  auto* h = new aqc_dm_s();
  h->n = n;
  h->rho = (cplx*)aqc::dev_alloc(sizeof(cplx) << (2 * n));
  if (!h->rho) {
    delete h;
    aqc::set_error("aqc_dm_create: out of device memory for the density matrix");
    return AQC_ERR_NOMEM;
  }
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    aqc::dev_free(h->rho);
    delete h;
    aqc::set_error("aqc_dm_create: hipStreamCreateWithFlags failed");
    return AQC_ERR_HIP;
  }
  *out = h;
  return aqc_dm_reset(h);
}

int aqc_dm_destroy(aqc_dm_t h) {
  if (!h) return AQC_OK;
  if (h->stream) hipStreamSynchronize(h->stream);
  aqc::dev_free(h->rho);
  if (h->d_buf) hipFree(h->d_buf);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
  return AQC_OK;
}

int aqc_dm_reset(aqc_dm_t h) {
  AQC_REQUIRE(h, "aqc_dm_reset: null handle");
  const size_t total = (size_t)1 << (2 * h->n);
  const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(k_dm_reset, dim3(grid), dim3(256), 0, h->stream, h->rho, total);
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipStreamSynchronize(h->stream));
  return AQC_OK;
}

static int plan_out(const char* entry, bool adjoint, int n, const aqc_op_t* prog, int nprog, int* counts,
                    aqc_dm_step_t* steps, int cap) {
  t_entry = entry;
  if (!(counts && nprog >= 0 && (prog || nprog == 0) && (steps || cap == 0) && cap >= 0)) return fail("bad arguments");
  if (!(n >= 1 && n <= kMaxQubits)) return fail("n must be in 1 .. 13");
  Plan plan;
  if (int rc = build_plan(n, prog, nprog, plan, adjoint)) return rc;
  counts[0] = (int)plan.segs.size();
  counts[1] = (int)plan.steps.size();
  counts[2] = nprog;
  counts[3] = plan.segs.empty() ? 0 : 2 * plan.kq;
  for (int i = 0; steps && i < (int)plan.steps.size() && i < cap; ++i) {
    const HStep& st = plan.steps[i];
    aqc_dm_step_t& o = steps[i];
    std::memset(&o, 0, sizeof(o));
    o.kind = st.unitary ? kUnitary : kSuper;
    o.nq = st.nq, o.q0 = st.q0, o.q1 = st.q1, o.segment = st.seg;
    const hmat& m = st.unitary ? st.U : st.S;
    for (size_t c = 0; c < m.size(); ++c) {
      o.m[2 * c] = m[c].real();
      o.m[2 * c + 1] = m[c].imag();
    }
  }
  return AQC_OK;
}

int aqc_dm_plan(int n, const aqc_op_t* prog, int nprog, int* counts, aqc_dm_step_t* steps, int cap) {
  return plan_out("aqc_dm_plan", false, n, prog, nprog, counts, steps, cap);
}

int aqc_dm_plan_adjoint(int n, const aqc_op_t* prog, int nprog, int* counts, aqc_dm_step_t* steps, int cap) {
  return plan_out("aqc_dm_plan_adjoint", true, n, prog, nprog, counts, steps, cap);
}

static int run_program(aqc_dm_t h, const aqc_op_t* prog, int nprog, bool adjoint) {
  Plan plan;
  if (int rc = build_plan(h->n, prog, nprog, plan, adjoint)) return rc;
  if (plan.segs.empty()) return AQC_OK;
  char* buf = nullptr;
  const size_t wb = plan.words.size() * sizeof(double);
  if (int rc = dm_buf(h, wb, &buf)) return rc;
  AQC_HIP_CHECK(hipMemcpyAsync(buf, plan.words.data(), wb, hipMemcpyHostToDevice, h->stream));
  const double bytes = 32.0 * std::ldexp(1.0, 2 * h->n);
  for (const DmSegArg& sa : plan.segs) {
    aqc::KernelTimer::begin(h->stream, "dm_segment", bytes, 0.0);
    switch (plan.kq) {
      case 1: launch_segment<1>(h, sa, (const double2*)buf); break;
      case 2: launch_segment<2>(h, sa, (const double2*)buf); break;
      case 3: launch_segment<3>(h, sa, (const double2*)buf); break;
      case 4: launch_segment<4>(h, sa, (const double2*)buf); break;
      case 5: launch_segment<5>(h, sa, (const double2*)buf); break;
      default: launch_segment<6>(h, sa, (const double2*)buf); break;
    }
    aqc::KernelTimer::end(h->stream);
    AQC_CHECK_LAUNCH();
  }
  // (the plan's host copy goes out of scope here, and a fault belongs to this call)
  AQC_HIP_CHECK(hipStreamSynchronize(h->stream));
  return AQC_OK;
}

int aqc_dm_apply(aqc_dm_t h, const aqc_op_t* prog, int nprog) {
  t_entry = "aqc_dm_apply";
  AQC_REQUIRE(h && nprog >= 0 && (prog || nprog == 0), "aqc_dm_apply: null argument");
  return run_program(h, prog, nprog, false);
}

int aqc_dm_apply_adjoint(aqc_dm_t h, const aqc_op_t* prog, int nprog) {
  t_entry = "aqc_dm_apply_adjoint";
  AQC_REQUIRE(h && nprog >= 0 && (prog || nprog == 0), "aqc_dm_apply_adjoint: null argument");
  return run_program(h, prog, nprog, true);
}

int aqc_dm_copy(aqc_dm_t dst, aqc_dm_t src) {
  AQC_REQUIRE(dst && src, "aqc_dm_copy: null handle");
  AQC_REQUIRE(dst->n == src->n, "aqc_dm_copy: the two matrices have different qubit counts");
  if (dst == src) return AQC_OK;
  AQC_HIP_CHECK(hipMemcpyAsync(dst->rho, src->rho, sizeof(cplx) << (2 * dst->n), hipMemcpyDeviceToDevice, dst->stream));
  AQC_HIP_CHECK(hipStreamSynchronize(dst->stream));
  return AQC_OK;
}

int aqc_dm_set(aqc_dm_t h, const double* in) {
  AQC_REQUIRE(h && in, "aqc_dm_set: null argument");
  AQC_HIP_CHECK(hipMemcpyAsync(h->rho, in, sizeof(cplx) << (2 * h->n), hipMemcpyHostToDevice, h->stream));
  AQC_HIP_CHECK(hipStreamSynchronize(h->stream));
  return AQC_OK;
}

int aqc_dm_set_diag(aqc_dm_t h, const double* d) {
  AQC_REQUIRE(h && d, "aqc_dm_set_diag: null argument");
  const size_t db = sizeof(double) << h->n;
  char* buf = nullptr;
  if (int rc = dm_buf(h, db, &buf)) return rc;
  AQC_HIP_CHECK(hipMemcpyAsync(buf, d, db, hipMemcpyHostToDevice, h->stream));
  const size_t total = (size_t)1 << (2 * h->n);
  const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(k_dm_set_diag, dim3(grid), dim3(256), 0, h->stream, h->rho, h->n, (const double*)buf, total);
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipStreamSynchronize(h->stream));  // (d is read by the copy until here)
  return AQC_OK;
}

int aqc_dm_transition(aqc_dm_t a, aqc_dm_t b, int q, double* out) {
  AQC_REQUIRE(a && b && out, "aqc_dm_transition: null argument");
  AQC_REQUIRE(a->n == b->n, "aqc_dm_transition: the two matrices have different qubit counts");
  AQC_REQUIRE(q >= 0 && q < a->n, "aqc_dm_transition: qubit out of range");
  const int n = a->n;
  // one workgroup while a thread has at most one o (4^(n-1) <= 256); else one o per thread, in one-wave
  // workgroups until 256-thread ones cover the 256 CUs (n = 8: 256 waves), and at most 1024 workgroups
  const size_t total = (size_t)1 << (2 * n - 2);
  const int threads = total <= (size_t)kThreads || total / kThreads >= 256 ? kThreads : 64;
  const int nblocks = total <= (size_t)kThreads ? 1 : (int)std::min<size_t>(total / threads, 1024);
  const size_t pb = aqc::up256((size_t)nblocks * 32 * sizeof(double));
  char* buf = nullptr;
  if (int rc = dm_buf(a, pb + 32 * sizeof(double), &buf)) return rc;
  aqc::KernelTimer::begin(a->stream, "dm_transition", 32.0 * std::ldexp(1.0, 2 * n), 0.0);
  hipLaunchKernelGGL(k_dm_transition, dim3(nblocks), dim3(threads), 0, a->stream, a->rho, b->rho, n, q, (double*)buf);
  aqc::KernelTimer::end(a->stream);
  AQC_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_dm_transition_sum, dim3(1), dim3(32), 0, a->stream, (const double*)buf, nblocks,
                     (double*)(buf + pb));
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipMemcpyAsync(out, buf + pb, 32 * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  AQC_HIP_CHECK(hipStreamSynchronize(a->stream));
  return AQC_OK;
}

int aqc_dm_get(aqc_dm_t h, double* out) {
  AQC_REQUIRE(h && out, "aqc_dm_get: null argument");
  AQC_HIP_CHECK(hipMemcpyAsync(out, h->rho, sizeof(cplx) << (2 * h->n), hipMemcpyDeviceToHost, h->stream));
  AQC_HIP_CHECK(hipStreamSynchronize(h->stream));
  return AQC_OK;
}

int aqc_dm_trace0(aqc_dm_t h, double* out) {
  AQC_REQUIRE(h && out, "aqc_dm_trace0: null argument");
  char* buf = nullptr;
  if (int rc = dm_buf(h, 2 * sizeof(double), &buf)) return rc;
  hipLaunchKernelGGL(k_dm_trace, dim3(1), dim3(kThreads), 0, h->stream, h->rho, h->n, (double*)buf);
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipMemcpyAsync(out, buf, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  AQC_HIP_CHECK(hipStreamSynchronize(h->stream));
  return AQC_OK;
}

int aqc_dm_diag_sv(aqc_dm_t h, aqc_sv_t sv) {
  AQC_REQUIRE(h && sv, "aqc_dm_diag_sv: null argument");
  cplx* state = nullptr;
  const int n = h->n;
  hipStream_t sv_stream = nullptr;
  if (int rc = aqc::sv_overwrite(sv, n, &state, &sv_stream)) return rc;  // (AQC_ERR_ARG for another qubit count)
  AQC_HIP_CHECK(hipStreamSynchronize(sv_stream));  // nothing queued still reads the amplitudes
  const unsigned dim = 1u << n;
  hipLaunchKernelGGL(k_dm_diag, dim3((dim + 255) / 256), dim3(256), 0, h->stream, h->rho, n, state);
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipStreamSynchronize(h->stream));
  return AQC_OK;
}

int aqc_dm_pauli_expect(aqc_dm_t h, const uint8_t* codes, int nterms, const double* effects, double* out) {
  t_entry = "aqc_dm_pauli_expect";
  AQC_REQUIRE(h && codes && out, "aqc_dm_pauli_expect: null argument");
  AQC_REQUIRE(nterms >= 1 && nterms <= kMaxTerms, "aqc_dm_pauli_expect: nterms must be in 1 .. 65536");
  if (effects)
    if (int rc = aqc::check_effects(h->n, effects, t_entry)) return rc;
  std::vector<DmTerm> terms;
  if (int rc = build_terms(h->n, codes, nterms, effects, terms)) return rc;
  const size_t tb = aqc::up256((size_t)nterms * sizeof(DmTerm)), ob = (size_t)nterms * sizeof(double);
  char* buf = nullptr;
  if (int rc = dm_buf(h, tb + ob, &buf)) return rc;
  AQC_HIP_CHECK(hipMemcpyAsync(buf, terms.data(), (size_t)nterms * sizeof(DmTerm), hipMemcpyHostToDevice, h->stream));
  aqc::KernelTimer::begin(h->stream, "dm_pauli", 0.0, 0.0);
  hipLaunchKernelGGL(k_dm_pauli, dim3(nterms), dim3(kThreads), 0, h->stream, h->rho, h->n, (const DmTerm*)buf,
                     (double*)(buf + tb));
  aqc::KernelTimer::end(h->stream);
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipMemcpyAsync(out, buf + tb, ob, hipMemcpyDeviceToHost, h->stream));
  AQC_HIP_CHECK(hipStreamSynchronize(h->stream));  // (terms is read by the copy until here)
  return AQC_OK;
}

int aqc_dm_pair_rdms(aqc_dm_t h, const int* pairs, int npairs, double* out) {
  AQC_REQUIRE(h && pairs && out && npairs >= 0 && npairs <= kMaxPairs, "aqc_dm_pair_rdms: bad arguments");
  AQC_REQUIRE(h->n >= 2, "aqc_dm_pair_rdms: needs at least 2 qubits");
  for (int p = 0; p < npairs; ++p) {
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    AQC_REQUIRE(a >= 0 && a < h->n && b >= 0 && b < h->n && a != b, "aqc_dm_pair_rdms: bad pair");
  }
  if (npairs == 0) return AQC_OK;
  const size_t pb = aqc::up256((size_t)2 * npairs * sizeof(int)), ob = (size_t)npairs * 16 * sizeof(cplx);
  char* buf = nullptr;
  if (int rc = dm_buf(h, pb + ob, &buf)) return rc;
  AQC_HIP_CHECK(hipMemcpyAsync(buf, pairs, (size_t)2 * npairs * sizeof(int), hipMemcpyHostToDevice, h->stream));
  aqc::KernelTimer::begin(h->stream, "dm_pair_rdms", 0.0, 0.0);
  hipLaunchKernelGGL(k_dm_pair_rdms, dim3(npairs), dim3(kThreads), 0, h->stream, h->rho, h->n, (const int*)buf,
                     (cplx*)(buf + pb));
  aqc::KernelTimer::end(h->stream);
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipMemcpyAsync(out, buf + pb, ob, hipMemcpyDeviceToHost, h->stream));
  AQC_HIP_CHECK(hipStreamSynchronize(h->stream));
  return AQC_OK;
}

int aqc_dm_pair_envs(aqc_dm_t h, const int* pairs, int npairs, const double* effects, double* out) {
  AQC_REQUIRE(h && pairs && out && npairs >= 0 && npairs <= kMaxPairs, "aqc_dm_pair_envs: bad arguments");
  AQC_REQUIRE(h->n >= 2, "aqc_dm_pair_envs: needs at least 2 qubits");
  const int n = h->n, m = n - 2;
  for (int p = 0; p < npairs; ++p) {
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    AQC_REQUIRE(a >= 0 && a < n && b >= 0 && b < n && a != b, "aqc_dm_pair_envs: bad pair");
  }
  double eff[kMaxQubits][4];
  uint32_t offdiag = 0;  // the qubits whose effect has an off-diagonal
  for (int q = 0; q < n; ++q)
    for (int c = 0; c < 4; ++c) {
      eff[q][c] = effects ? effects[4 * q + c] : (c < 2 ? 1.0 : 0.0);
      AQC_REQUIRE(std::isfinite(eff[q][c]), "aqc_dm_pair_envs: an effect is not finite");
      if (c >= 2 && eff[q][c] != 0.0) offdiag |= 1u << q;
    }
  if (npairs == 0) return AQC_OK;
  int split = 1;  // the grid's: the largest of the pairs'
  double items = 0.0;
  for (int p = 0; p < npairs; ++p) {
    const int ng = __builtin_popcount(offdiag & ~((1u << pairs[2 * p]) | (1u << pairs[2 * p + 1])));
    split = std::max(split, env_split(m, ng));
    items += std::ldexp(1.0, m + ng);
  }
  const size_t pb = aqc::up256((size_t)2 * npairs * sizeof(int)), eb = aqc::up256(sizeof(eff));
  const size_t ob = aqc::up256((size_t)npairs * 16 * sizeof(cplx));
  const size_t qb = split > 1 ? (size_t)npairs * split * 32 * sizeof(double) : 0;
  char* buf = nullptr;
  if (int rc = dm_buf(h, pb + eb + ob + qb, &buf)) return rc;
  const int* d_pairs = (const int*)buf;
  const double* d_eff = (const double*)(buf + pb);
  double* d_out = (double*)(buf + pb + eb);
  double* d_part = split > 1 ? (double*)(buf + pb + eb + ob) : d_out;
  AQC_HIP_CHECK(hipMemcpyAsync(buf, pairs, (size_t)2 * npairs * sizeof(int), hipMemcpyHostToDevice, h->stream));
  AQC_HIP_CHECK(hipMemcpyAsync(buf + pb, eff, sizeof(eff), hipMemcpyHostToDevice, h->stream));
  // the two weight tables: 4^ceil(m / 2) + 4^floor(m / 2) complex words, 80 KB at 13 qubits
  const int hl = (m + 1) / 2, hh = m - hl;
  const size_t lds = (((size_t)1 << (2 * hl)) + ((size_t)1 << (2 * hh))) * sizeof(cplx);
  if (lds > 48 * 1024)
    AQC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_dm_pair_envs),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  aqc::KernelTimer::begin(h->stream, "dm_pair_envs", 256.0 * items, 136.0 * items);  // 16 + 1 complex MACs an item
  hipLaunchKernelGGL(k_dm_pair_envs, dim3(split, npairs), dim3(kThreads), lds, h->stream, h->rho, n, d_pairs, d_eff,
                     offdiag, d_part);
  aqc::KernelTimer::end(h->stream);
  AQC_CHECK_LAUNCH();
  if (split > 1) {
    hipLaunchKernelGGL(k_dm_pair_envs_sum, dim3(npairs), dim3(32), 0, h->stream, (const double*)d_part, n, d_pairs,
                       offdiag, split, d_out);
    AQC_CHECK_LAUNCH();
  }
  AQC_HIP_CHECK(hipMemcpyAsync(out, d_out, (size_t)npairs * 16 * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
  AQC_HIP_CHECK(hipStreamSynchronize(h->stream));  // (pairs and eff are read by the copies until here)
  return AQC_OK;
}

int aqc_dm_pair_transitions_plan(int n, int npairs, int* split) {
  AQC_REQUIRE(split != nullptr, "aqc_dm_pair_transitions_plan: null split");
  AQC_REQUIRE(n >= 2 && n <= kMaxQubits, "aqc_dm_pair_transitions_plan: n must be in 2 .. 13");
  AQC_REQUIRE(npairs >= 1 && npairs <= kMaxPairs, "aqc_dm_pair_transitions_plan: npairs must be in 1 .. 4096");
  *split = trans_split(n, npairs);
  return AQC_OK;
}

int aqc_dm_pair_transitions(aqc_dm_t a, aqc_dm_t b, const int* pairs, int npairs, double* out) {
  AQC_REQUIRE(a && b && pairs && out && npairs >= 0 && npairs <= kMaxPairs, "aqc_dm_pair_transitions: bad arguments");
  AQC_REQUIRE(a->n == b->n, "aqc_dm_pair_transitions: the two matrices have different qubit counts");
  AQC_REQUIRE(a->n >= 2, "aqc_dm_pair_transitions: needs at least 2 qubits");
  const int n = a->n;
  for (int p = 0; p < npairs; ++p) {
    const int x = pairs[2 * p], y = pairs[2 * p + 1];
    AQC_REQUIRE(x >= 0 && x < n && y >= 0 && y < n && x != y, "aqc_dm_pair_transitions: bad pair");
  }
  if (npairs == 0) return AQC_OK;
  const int split = trans_split(n, npairs);
  const size_t pb = aqc::up256((size_t)2 * npairs * sizeof(int)), ob = (size_t)npairs * 256 * sizeof(cplx);
  const size_t qb = split > 1 ? (size_t)npairs * split * 256 * sizeof(cplx) : 0;
  char* buf = nullptr;
  if (int rc = dm_buf(a, pb + ob + qb, &buf)) return rc;
  cplx* d_out = (cplx*)(buf + pb);
  cplx* d_part = split > 1 ? (cplx*)(buf + pb + ob) : d_out;
  AQC_HIP_CHECK(hipMemcpyAsync(buf, pairs, (size_t)2 * npairs * sizeof(int), hipMemcpyHostToDevice, a->stream));
  // a pair reads both matrices once (2 x 16 x 4^n bytes) for 256 complex MACs per value of o
  const double items = (double)npairs * std::ldexp(1.0, 2 * n - 4);
  aqc::KernelTimer::begin(a->stream, "dm_pair_transitions", 512.0 * items, 2048.0 * items);
  hipLaunchKernelGGL(k_dm_pair_transitions, dim3(split, npairs), dim3(kThreads), 0, a->stream, a->rho, b->rho, n,
                     (const int*)buf, d_part);
  aqc::KernelTimer::end(a->stream);
  AQC_CHECK_LAUNCH();
  if (split > 1) {
    hipLaunchKernelGGL(k_dm_pair_transitions_sum, dim3(npairs), dim3(256), 0, a->stream, (const cplx*)d_part, split,
                       d_out);
    AQC_CHECK_LAUNCH();
  }
  AQC_HIP_CHECK(hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, a->stream));
  AQC_HIP_CHECK(hipStreamSynchronize(a->stream));  // (pairs is read by the copy until here)
  return AQC_OK;
}

}  // extern "C"
