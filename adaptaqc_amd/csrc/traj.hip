// Noisy shot sampling by quantum trajectories: what Aer's qasm_simulator does under a NoiseModel
// (execute_kwargs={'noise_model': ..., 'shots': ...}, approximate_compiler.py:93).
//
// A shot is one trajectory: psi = |0...0>, the program's rows in order, then one draw of all
// qubits.  A gate row (flags 0) is a 1- or 2-qubit unitary.  A Kraus row (AQC_OP_KRAUS1) holds the
// 1..4 operators K_k of a one-qubit channel on q0: with p_k = |K_k psi|^2, in-order inclusive sums
// C_k and P = C_last, event e takes the smallest k with C_k > u_e P (where rounding leaves none, the
// last k with p_k > 0) and psi <- K_k psi / sqrt(p_k).  The final draw is aqc_sv_sample's rule with
// u_E.  u_e = sample_uniform(seed, run, shot, e): an outcome depends on (seed, run, shot) only.
// A correlated two-qubit channel (AQC_OP_KRAUS2) is a group of nk <= 16 consecutive rows, one 4x4
// operator each, on the qubits (q0, q1) of the gate it follows: one event with the same choice rule,
// the chosen operator applied to both qubits.
//
// k_sv_traj: one workgroup carries one trajectory from |0...0> to its outcome and loops over the
// shots wg, wg + grid, ...; no workgroup waits for another.  Up to 13 qubits the state lives in
// dynamic LDS (16 * 2^n bytes), beside a staged chunk of program rows (vector loads, as
// k_sv_segment stages its gates), the chunk's uniforms and a small reduction area; from 14 qubits
// the same row code runs on the workgroup's slice of a global workspace (slow, but correct).
//   gate row    the pair / quad pass of k_sv_segment
//   Kraus row   a reduction pass for the qubit's reduced density matrix (rho00, rho11, rho01:
//               summed per thread in pair order, over the wave by a butterfly, over the waves in
//               index order), p_k = Re Tr(K_k^dag K_k rho) with K_k^dag K_k multiplied on the host,
//               then an apply pass with K_k / sqrt(p_k)
//   Kraus group on its first row: where every K_k^dag K_k is a multiple of I (Pauli and other
//               mixed-unitary channels) p_k is that multiple and no pass reads the state; else one
//               reduction pass over the amplitude quadruples of (q0, q1) for the 4 real and 6
//               complex entries of the 4x4 reduced density matrix (same order: thread, wave
//               butterfly, waves in index order), p_k = max(0, Re Tr(K_k^dag K_k rho)).  The
//               weights and the chosen operator are read from the global program (uniform
//               addresses), never from the staged chunk, which a group may overrun; the chosen
//               K_k / sqrt(p_k) replaces the first row's matrix in LDS and the gate row's quad
//               pass applies it.  The group's other rows are skipped.
//   final draw  thread t sums its contiguous amplitudes in order, a wave scan, the wave totals
//               in order; the first thread whose inclusive sum exceeds u_E P walks its amplitudes
// No atomics anywhere: two calls return the same bits.
//
// Noisy pair tomography (aqc_sv_traj_pair_tomo) runs the same rows with another ending (the kernel's
// END parameter): trajectory t serves Pauli setting s = t % 9 of every pair.  Instead of the final
// draw, wave w takes pairs w, w + nwaves, ...: its lanes stride over the 2^(n-2) amplitude
// quadruples of the pair and sum the 4 real and 6 complex entries of the pure state's 4x4 RDM, a
// butterfly adds the lanes (no workgroup barrier, no LDS beside the state; the order depends on the
// wave width only), and lane 0 forms p_o = max(0, Re Tr[(E_hi (x) E_lo) rho]) from the two qubits'
// POVM effects of the setting and draws one outcome by the multinomial rule.  The count tables are
// integer sums (integer atomics): they do not depend on the launch shape either.
//
// The Pauli readout (aqc_sv_traj_pauli_counts) is a third ending: every trajectory serves every term.
// Wave w takes terms w, w + nwaves, ...: its lanes stride over the 2^n amplitudes k and sum
// conj(psi[k]) (M psi)[k] for the term's parity operator M, a product of one Hermitian 2x2 factor
// D_q = E_q[+] - E_q[-] per qubit of its support.  The host folds the factors that are a multiple of a
// Pauli into an x mask, a z mask and one complex scalar (one load per amplitude, whatever the weight)
// and keeps the others -- at most 4: relaxation on the readout gives them an identity part -- as
// general factors, 2^ng loads per amplitude.  A butterfly adds the lanes (no workgroup barrier, no LDS
// beside the state), lane 0 clamps p_+ = (1 + v) / 2, draws one +-1 outcome and counts it (integer
// atomics).  Term records are read from global memory at wave-uniform addresses.
//
// LDS layout: interleaved 16-byte complex amplitudes, as k_sv_segment's tile.  Split re / im arrays
// (8-byte accesses) measured 2-7% slower at 8, 10, 12 and 13 qubits, with equal counts
// (profiles/trajectory_layout_ab.json), and were removed.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "aqc_internal.h"
#include "kraus_group.h"
#include "pair_draw.h"
#include "sample_rng.h"

using aqc::cplx;

namespace {

constexpr int kMaxThreads = 512;
constexpr int kMaxWaves = kMaxThreads / 64;
constexpr int kChunk = 16;          // program rows staged in LDS at a time (16 x 416 B)
constexpr int kLdsMaxQubits = 13;   // 2^13 x 16 B = 128 KB of the CU's 160 KB
constexpr int kMaxQubits = 24;
constexpr int kMaxShots = 1 << 30;
constexpr int kMaxGlobalWgs = 256;  // global-workspace path: at most 256 workgroups and 512 MB
constexpr size_t kMaxGlobalBytes = (size_t)512 << 20;

enum { kGate1 = 0, kGate2 = 1, kKraus = 2, kKraus2 = 3 };
enum { kLds = 0, kGlobal = 1 };
// a trajectory's ending: the full-register draw, the pair readout, or the Pauli readout
enum { kEndDraw = 0, kEndPairs = 1, kEndPaulis = 2 };
constexpr int kMaxPairs = 4096;
constexpr int kMaxTerms = 65536;
constexpr int kMaxGeneral = 4;  // general (not Pauli-proportional) factors per term: 2^4 loads per amplitude

// A program row as the kernel reads it.  Gate: m = the 2x2 / 4x4 matrix.  Kraus: m[8k ..] = K_k,
// w[4k ..] = (M00, M11, Re M01, Im M01) of M = K_k^dag K_k, ev = the event index.  Kraus2 (one row per
// operator of a group): m = the 4x4 K_k, w = M = K_k^dag K_k as M00 M11 M22 M33, then (Re, Im) of M01
// M02 M03 M12 M13 M23; k = the row's place in its group; flat (first row): every M a multiple of I.
struct TrajRow {
  int32_t kind, q0, q1, nk, ev, k, flat, pad;
  double m[32];
  double w[16];
};
static_assert(sizeof(TrajRow) == 416 && sizeof(TrajRow) % sizeof(double2) == 0, "TrajRow layout");
constexpr int kRowWords = (int)(sizeof(TrajRow) / sizeof(double2));

// A term of the Pauli readout as the kernel reads it: M = (cr + i ci) P (x) G, with P the Pauli string
// whose entry (k, k ^ x) is (-1)^popcount(k & z) (X and Y qubits in x, Y and Z qubits in z; the scalars
// of the factors and (-i)^ny folded into cr + i ci), and G the product of ng general factors, factor a
// on qubit gq[a] as g[a] = (D00, D11, Re D01, Im D01).  The supports of P and G are disjoint.
struct PauliTerm {
  uint32_t x, z;
  int32_t ng, gq[kMaxGeneral], pad;
  double cr, ci;
  double g[kMaxGeneral][4];
};
static_assert(sizeof(PauliTerm) == 176, "PauliTerm layout");

struct TrajJob {
  const TrajRow* prog;
  int nprog, n, nshots, nev;
  const double* u;  // null, or nshots x ustride (nev + 1; nev + npairs for the pair readout)
  uint64_t seed, run;
  uint64_t* out;
  uint8_t* choices;  // null, or nshots x nev
  cplx* ws;          // kGlobal: 2^n amplitudes per workgroup
  int ustride;
  // kEndPairs (nshots then counts trajectories, trajectory t serving setting t % 9); kEndPaulis (every
  // trajectory serves every term) keeps its fields in the same storage, so TrajJob does not grow
  union {
    int npairs;
    int nterms;
  };
  union {
    const int* pairs;             // 2 npairs
    const PauliTerm* terms;
  };
  union {
    const double* effects;        // [n][3][2][4]: (E00, E11, Re E01, Im E01)
    double* values;               // null, or nshots x nterms: v before clamping
  };
  union {
    unsigned long long* counts;   // [npairs][9][4]
    unsigned long long* plus;     // [nterms]: the outcome-0 draws
  };
  uint8_t* outcomes;              // null, or nshots x npairs / nshots x nterms
};

// bytes of dynamic LDS beside the state
// The kernel is compiled twice (its K2 parameter): a program without a Kraus group runs the variant
// without the group code, whose registers and side area are what the one-qubit rows need.
constexpr int kRedWords = 16;  // doubles per wave in the reduction area with groups: their 4x4 RDM
constexpr size_t side_bytes(bool k2) {
  return kChunk * sizeof(TrajRow) + kChunk * sizeof(double) + kMaxWaves * (k2 ? kRedWords : 4) * sizeof(double) +
         kMaxWaves * sizeof(double) + (k2 ? (16 + kRedWords) * sizeof(double) : 0) + kMaxWaves * sizeof(int);
}
static_assert(((size_t)1 << kLdsMaxQubits) * sizeof(cplx) + side_bytes(true) <= (size_t)160 * 1024,
              "the largest LDS-resident state and the side area fit a CU's LDS");

template <int MODE>
struct Amps;
template <>
struct Amps<kLds> {
  cplx* a;
  __device__ __forceinline__ cplx ld(int i) const { return a[i]; }
  __device__ __forceinline__ void st(int i, cplx v) const { a[i] = v; }
};
template <>
struct Amps<kGlobal> {
  cplx* a;
  __device__ __forceinline__ cplx ld(int i) const { return aqc::ldg(a + i); }
  __device__ __forceinline__ void st(int i, cplx v) const { aqc::stg(a + i, v); }
};

__device__ __forceinline__ int insert_zero(int v, int b) { return ((v >> b) << (b + 1)) | (v & ((1 << b) - 1)); }

__device__ __forceinline__ double wave_sum(double v) {
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ double wave_scan(double v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const double t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

// One lane's share of sum_k conj(psi[k]) sign_z(k) sum_a (prod_f D_f[k_f, a_f]) psi[(k ^ x) with the bits
// of the NG general factors set to a], k = lane, lane + 64, ...; the a loop unrolls, 2^NG loads.
template <int MODE, int NG>
__device__ __forceinline__ void pauli_term_sum(const Amps<MODE>& psi, const PauliTerm& tm, int lane, int dim, double& sx,
                                               double& sy) {
  const int x = (int)tm.x, z = (int)tm.z;
  int q[NG > 0 ? NG : 1], gmask = 0;
  double g[NG > 0 ? NG : 1][4];
#pragma unroll
  for (int f = 0; f < NG; ++f) {
    q[f] = tm.gq[f];
    gmask |= 1 << q[f];
#pragma unroll
    for (int c = 0; c < 4; ++c) g[f][c] = tm.g[f][c];
  }
  for (int k = lane; k < dim; k += 64) {
    const int base = (k ^ x) & ~gmask;
    cplx row[NG > 0 ? NG : 1][2];  // row k_f of D_f
#pragma unroll
    for (int f = 0; f < NG; ++f) {
      const bool kb = (k >> q[f]) & 1;  // D = (D00, D11, Re D01, Im D01); D10 = conj(D01)
      row[f][0] = kb ? aqc::cmk(g[f][2], -g[f][3]) : aqc::cmk(g[f][0], 0.0);
      row[f][1] = kb ? aqc::cmk(g[f][1], 0.0) : aqc::cmk(g[f][2], g[f][3]);
    }
    cplx acc = aqc::cmk(0.0, 0.0);
#pragma unroll
    for (int a = 0; a < (1 << NG); ++a) {
      int idx = base;
      cplx w = aqc::cmk(1.0, 0.0);
#pragma unroll
      for (int f = NG - 1; f >= 0; --f) {  // (the high factors first: their products are shared between a's)
        idx |= ((a >> f) & 1) << q[f];
        w = f == NG - 1 ? row[f][(a >> f) & 1] : aqc::cmul(w, row[f][(a >> f) & 1]);
      }
      acc = NG == 0 ? psi.ld(idx) : aqc::cfma(w, psi.ld(idx), acc);
    }
    const cplx t = aqc::cmulc(acc, psi.ld(k));  // acc conj(psi[k])
    const double sg = (__popc(k & z) & 1) ? -1.0 : 1.0;
    sx += sg * t.x;
    sy += sg * t.y;
  }
}

template <int MODE, int END, bool K2>
__global__ __launch_bounds__(kMaxThreads) void k_sv_traj(const TrajJob j) {
  extern __shared__ double2 traj_lds[];
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nwaves = T >> 6;
  const int n = j.n, dim = 1 << n, half = dim >> 1, quarter = dim >> 2;
  const int lds_amps = MODE == kGlobal ? 0 : dim;
  Amps<MODE> psi;
  if constexpr (MODE == kLds) psi.a = (cplx*)traj_lds;
  else psi.a = j.ws + (size_t)blockIdx.x * dim;
  TrajRow* rows = (TrajRow*)(traj_lds + lds_amps);
  double* ul = (double*)(rows + kChunk);  // the chunk's uniforms
  double* red = ul + kChunk;              // [wave][4], with groups [wave][kRedWords]
  double* wtot = red + kMaxWaves * (K2 ? kRedWords : 4);  // [wave]
  double* pkl = wtot + kMaxWaves;         // K2 only, [16]: a Kraus group's weights p_k
  double* rho = pkl + 16;                 // K2 only, [kRedWords]: a Kraus group's reduced density matrix
  int* wlast = (int*)(K2 ? rho + kRedWords : pkl);  // [wave]
  const int nev = j.nev;

  for (int shot = blockIdx.x; shot < j.nshots; shot += gridDim.x) {
    for (int i = tid; i < dim; i += T) psi.st(i, aqc::cmk(i == 0 ? 1.0 : 0.0, 0.0));
    for (int c0 = 0; c0 < j.nprog; c0 += kChunk) {
      const int nc = min(kChunk, j.nprog - c0);
      __syncthreads();  // the previous chunk's last row has been applied
      for (int w = tid; w < nc * kRowWords; w += T)
        ((double2*)rows)[w] = reinterpret_cast<const double2*>(j.prog + c0)[w];
      // an event's uniform sits at its (first) row's place in the chunk
      if (tid < nc && (j.prog[c0 + tid].kind == kKraus || (K2 && j.prog[c0 + tid].kind == kKraus2 && j.prog[c0 + tid].k == 0))) {
        const int e = j.prog[c0 + tid].ev;
        ul[tid] = j.u ? j.u[(size_t)shot * j.ustride + e] : aqc::sample_uniform(j.seed, j.run, (uint64_t)shot, (uint32_t)e);
      }
      for (int gi = 0; gi < nc; ++gi) {
        const TrajRow& r = rows[gi];
        __syncthreads();
        const int kind = r.kind;
        if (K2 && kind == kKraus2) {
          if (r.k != 0) continue;  // the group was served on its first row
          const TrajRow* grp = j.prog + (c0 + gi);  // the group's rows in the global program
          const int nk = r.nk, flat = r.flat;
          if (!flat) {
            const int t0 = r.q0, t1 = r.q1;
            const int lo = t0 < t1 ? t0 : t1, hi = t0 < t1 ? t1 : t0;
            double d[4] = {0.0, 0.0, 0.0, 0.0};  // rho_ss; rho_st = sum a_s conj(a_t), s < t
            double ox[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, oy[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int p = tid; p < quarter; p += T) {
              const int b = insert_zero(insert_zero(p, lo), hi);
              cplx a[4];
#pragma unroll
              for (int s = 0; s < 4; ++s) a[s] = psi.ld(b | ((s & 1) << t0) | ((s >> 1) << t1));
              int c = 0;
#pragma unroll
              for (int s = 0; s < 4; ++s) {
                d[s] += aqc::cnorm2(a[s]);
#pragma unroll
                for (int t = s + 1; t < 4; ++t, ++c) {
                  const cplx z = aqc::cmulc(a[s], a[t]);
                  ox[c] += z.x;
                  oy[c] += z.y;
                }
              }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) d[s] = wave_sum(d[s]);
#pragma unroll
            for (int c = 0; c < 6; ++c) {
              ox[c] = wave_sum(ox[c]);
              oy[c] = wave_sum(oy[c]);
            }
            if (lane == 0) {
              double* rw = red + kRedWords * wave;
#pragma unroll
              for (int s = 0; s < 4; ++s) rw[s] = d[s];
#pragma unroll
              for (int c = 0; c < 6; ++c) {
                rw[4 + 2 * c] = ox[c];
                rw[5 + 2 * c] = oy[c];
              }
            }
            __syncthreads();
            if (tid < kRedWords) {  // entry tid of rho: the waves' sums in index order
              double x = 0.0;
              for (int wv = 0; wv < nwaves; ++wv) x += red[kRedWords * wv + tid];
              rho[tid] = x;
            }
            __syncthreads();
          }
          // thread q < nk: p_q = max(0, Re Tr(M_q rho)); a flat group's p_q is M_q[0][0] (rho has trace 1)
          if (tid < nk) {
            const double* w = grp[tid].w;
            double p = w[0];
            if (!flat) {
              p = w[0] * rho[0] + w[1] * rho[1] + w[2] * rho[2] + w[3] * rho[3];
              double o = 0.0;
#pragma unroll
              for (int e = 4; e < kRedWords; ++e) o += w[e] * rho[e];
              p += 2.0 * o;
            }
            pkl[tid] = fmax(0.0, p);
          }
          __syncthreads();
          // every thread takes the same weights in the same order, so all choose the same k
          double P = 0.0;
          for (int q = 0; q < nk; ++q) P += pkl[q];
          const double target = ul[gi] * P;
          int k = -1, lastnz = 0;
          double c = 0.0;
          for (int q = 0; q < nk; ++q) {
            const double pq = pkl[q];
            c += pq;
            if (pq > 0.0) lastnz = q;
            if (k < 0 && c > target) k = q;
          }
          if (k < 0) k = lastnz;
          const double psel = pkl[k];
          const double sc = psel > 0.0 ? 1.0 / sqrt(psel) : 0.0;
          if (tid == 0 && j.choices) j.choices[(size_t)shot * nev + r.ev] = (uint8_t)k;
          // the chosen operator, scaled, takes the place of K_0 in the staged row (restaged every shot)
          if (tid < 16) ((cplx*)rows[gi].m)[tid] = aqc::cscale(((const cplx*)grp[k].m)[tid], sc);
          __syncthreads();
        }
        if (kind == kGate2 || (K2 && kind == kKraus2)) {
          const int t0 = r.q0, t1 = r.q1;
          const int lo = t0 < t1 ? t0 : t1, hi = t0 < t1 ? t1 : t0;
          const cplx* m = (const cplx*)r.m;
          for (int p = tid; p < quarter; p += T) {
            const int b = insert_zero(insert_zero(p, lo), hi);
            int idx[4];
            cplx v[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              idx[s] = b | ((s & 1) << t0) | ((s >> 1) << t1);
              v[s] = psi.ld(idx[s]);
            }
#pragma unroll
            for (int o = 0; o < 4; ++o) {
              cplx acc = aqc::cmul(m[4 * o], v[0]);
              acc = aqc::cfma(m[4 * o + 1], v[1], acc);
              acc = aqc::cfma(m[4 * o + 2], v[2], acc);
              acc = aqc::cfma(m[4 * o + 3], v[3], acc);
              psi.st(idx[o], acc);
            }
          }
          continue;
        }
        const int t = r.q0;
        cplx m00, m01, m10, m11;
        if (kind == kGate1) {
          const cplx* m = (const cplx*)r.m;
          m00 = m[0], m01 = m[1], m10 = m[2], m11 = m[3];
        } else {
          double r00 = 0.0, r11 = 0.0, rx = 0.0, ry = 0.0;  // rho01 = sum a0 conj(a1)
          for (int p = tid; p < half; p += T) {
            const int i0 = insert_zero(p, t);
            const cplx a0 = psi.ld(i0), a1 = psi.ld(i0 | (1 << t));
            r00 += aqc::cnorm2(a0);
            r11 += aqc::cnorm2(a1);
            const cplx c = aqc::cmulc(a0, a1);
            rx += c.x;
            ry += c.y;
          }
          r00 = wave_sum(r00);
          r11 = wave_sum(r11);
          rx = wave_sum(rx);
          ry = wave_sum(ry);
          if (lane == 0) {
            red[4 * wave] = r00;
            red[4 * wave + 1] = r11;
            red[4 * wave + 2] = rx;
            red[4 * wave + 3] = ry;
          }
          __syncthreads();
          // every thread takes the same sums in the same order, so all choose the same k
          r00 = r11 = rx = ry = 0.0;
          for (int w = 0; w < nwaves; ++w) {
            r00 += red[4 * w];
            r11 += red[4 * w + 1];
            rx += red[4 * w + 2];
            ry += red[4 * w + 3];
          }
          const int nk = r.nk;
          double pk[4], P = 0.0;
          for (int k = 0; k < 4; ++k) {
            pk[k] = 0.0;
            if (k < nk) {
              const double* w = r.w + 4 * k;
              pk[k] = fmax(0.0, w[0] * r00 + w[1] * r11 + 2.0 * (w[2] * rx + w[3] * ry));
              P += pk[k];
            }
          }
          const double target = ul[gi] * P;
          int k = -1, lastnz = 0;
          double c = 0.0, psel = 0.0;
          for (int q = 0; q < 4; ++q) {
            if (q >= nk) break;
            c += pk[q];
            if (pk[q] > 0.0) lastnz = q;
            if (k < 0 && c > target) k = q;
          }
          if (k < 0) k = lastnz;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q == k) psel = pk[q];
          const double sc = psel > 0.0 ? 1.0 / sqrt(psel) : 0.0;
          const cplx* m = (const cplx*)r.m + 4 * k;
          m00 = aqc::cscale(m[0], sc), m01 = aqc::cscale(m[1], sc);
          m10 = aqc::cscale(m[2], sc), m11 = aqc::cscale(m[3], sc);
          if (tid == 0 && j.choices) j.choices[(size_t)shot * nev + r.ev] = (uint8_t)k;
        }
        for (int p = tid; p < half; p += T) {
          const int i0 = insert_zero(p, t), i1 = i0 | (1 << t);
          const cplx a0 = psi.ld(i0), a1 = psi.ld(i1);
          psi.st(i0, aqc::cfma(m01, a1, aqc::cmul(m00, a0)));
          psi.st(i1, aqc::cfma(m11, a1, aqc::cmul(m10, a0)));
        }
      }
    }
    __syncthreads();
    if constexpr (END == kEndPaulis) {
      // ---- the Pauli readout: a wave per term, every term from every trajectory ----
      for (int tj = wave; tj < j.nterms; tj += nwaves) {
        const PauliTerm& tm = j.terms[tj];  // (wave-uniform address)
        double sx = 0.0, sy = 0.0;
        switch (tm.ng) {  // (wave-uniform: the general factors' loops unroll per count)
          case 0: pauli_term_sum<MODE, 0>(psi, tm, lane, dim, sx, sy); break;
          case 1: pauli_term_sum<MODE, 1>(psi, tm, lane, dim, sx, sy); break;
          case 2: pauli_term_sum<MODE, 2>(psi, tm, lane, dim, sx, sy); break;
          case 3: pauli_term_sum<MODE, 3>(psi, tm, lane, dim, sx, sy); break;
          default: pauli_term_sum<MODE, 4>(psi, tm, lane, dim, sx, sy); break;
        }
        sx = wave_sum(sx);
        sy = wave_sum(sy);
        if (lane == 0) {
          const double v = tm.cr * sx - tm.ci * sy;
          const double pp = fmin(1.0, fmax(0.0, 0.5 * (1.0 + v)));
          const double uu = j.u ? j.u[(size_t)shot * j.ustride + nev + tj]
                                : aqc::sample_uniform(j.seed, j.run, (uint64_t)shot, (uint32_t)(nev + tj));
          const int o = uu >= pp ? 1 : 0;
          if (j.values) j.values[(size_t)shot * j.nterms + tj] = v;
          if (j.outcomes) j.outcomes[(size_t)shot * j.nterms + tj] = (uint8_t)o;
          if (!o) atomicAdd(j.plus + tj, 1ULL);
        }
      }
    } else if constexpr (END == kEndPairs) {
      // ---- the pair readout: a wave per pair, setting s = shot % 9 ----
      const int s9 = shot % 9;
      for (int pj = wave; pj < j.npairs; pj += nwaves) {
        const int qa = j.pairs[2 * pj], qb = j.pairs[2 * pj + 1];
        const int lo = qa < qb ? qa : qb, hi = qa < qb ? qb : qa;
        double d[4] = {0.0, 0.0, 0.0, 0.0};  // rho_ss
        double ox[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, oy[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // rho_st, s < t
        for (int p = lane; p < quarter; p += 64) {
          const int b = insert_zero(insert_zero(p, lo), hi);
          cplx a[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) a[s] = psi.ld(b | ((s & 1) << lo) | ((s >> 1) << hi));
          int c = 0;
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            d[s] += aqc::cnorm2(a[s]);
#pragma unroll
            for (int t = s + 1; t < 4; ++t, ++c) {
              const cplx z = aqc::cmulc(a[s], a[t]);  // a_s conj(a_t)
              ox[c] += z.x;
              oy[c] += z.y;
            }
          }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) d[s] = wave_sum(d[s]);
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          ox[c] = wave_sum(ox[c]);
          oy[c] = wave_sum(oy[c]);
        }
        if (lane == 0) {
          const double* eh = j.effects + (size_t)((hi * 3 + s9 / 3) * 2) * 4;
          const double* el = j.effects + (size_t)((lo * 3 + s9 % 3) * 2) * 4;
          const double uu = j.u ? j.u[(size_t)shot * j.ustride + nev + pj]
                                : aqc::sample_uniform(j.seed, j.run, (uint64_t)shot, (uint32_t)(nev + pj));
          const int k = aqc::pair_outcome(eh, el, d, ox, oy, uu);
          if (j.outcomes) j.outcomes[(size_t)shot * j.npairs + pj] = (uint8_t)k;
          atomicAdd(j.counts + ((size_t)pj * 9 + s9) * 4 + k, 1ULL);
        }
      }
    } else {
      // ---- the final draw ----
      const int cpt = dim >= T ? dim / T : 1;  // contiguous amplitudes per thread
      const int base = tid * cpt;
      double s = 0.0;
      int lastnz = -1;
      if (base < dim)
        for (int q = 0; q < cpt; ++q) {
          const double p = aqc::cnorm2(psi.ld(base + q));
          if (p > 0.0) lastnz = base + q;
          s += p;
        }
      const double scan = wave_scan(s, lane);
      int wl = lastnz;
      for (int d = 1; d < 64; d <<= 1) wl = max(wl, __shfl_xor(wl, d, 64));
      if (lane == 63) wtot[wave] = scan;
      if (lane == 0) wlast[wave] = wl;
      __syncthreads();
      double off = 0.0, P = 0.0;
      int last = -1;
      for (int w = 0; w < nwaves; ++w) {
        if (w == wave) off = P;
        P += wtot[w];
        last = max(last, wlast[w]);
      }
      const double uu = j.u ? j.u[(size_t)shot * (nev + 1) + nev]
                            : aqc::sample_uniform(j.seed, j.run, (uint64_t)shot, (uint32_t)nev);
      const double target = uu * P;
      if (!(target < P)) {  // rounding (or the zero vector): the last outcome with p > 0
        if (tid == 0) j.out[shot] = (uint64_t)(last < 0 ? 0 : last);
      } else {
        double prev = __shfl_up(scan, 1, 64);
        if (lane == 0) prev = 0.0;
        const double incl = off + scan, excl = off + prev;
        if (incl > target && !(excl > target)) {  // the first thread whose inclusive sum exceeds the target
          int idx = -1;
          double c = excl;
          for (int q = 0; q < cpt; ++q) {
            c += aqc::cnorm2(psi.ld(base + q));
            if (c > target) {
              idx = base + q;
              break;
            }
          }
          if (idx < 0) idx = lastnz < 0 ? base : lastnz;
          j.out[shot] = (uint64_t)idx;
        }
      }
    }
    __syncthreads();  // the draw has read the state before the next shot resets it
  }
}

aqc::PerDevice<aqc::DevScratch> g_scr;
using aqc::up256;

thread_local const char* t_entry = "aqc_sv_traj_sample";  // the entry point named in error messages

int fail(const std::string& msg) {
  aqc::set_error(std::string(t_entry) + ": " + msg);
  return AQC_ERR_ARG;
}

// the nk rows of a correlated group whose first row (k = 0, nk, qubits) has been checked: every row's
// flags and qubits, finite entries, M_k = K_k^dag K_k into w, sum M_k = I within 1e-9
int build_group(const aqc_op_t* ops, int nk, TrajRow* out, int ev) {
  double w[16][16];
  bool flat = true;
  if (const char* why = aqc::kraus2_group_error(ops, nk, w, &flat)) return fail(why);
  for (int k = 0; k < nk; ++k) {
    const aqc_op_t& op = ops[k];
    TrajRow& r = out[k];
    r.kind = kKraus2;
    r.q0 = op.q0;
    r.q1 = op.q1;
    r.nk = nk;
    r.ev = ev;
    r.k = k;
    std::memcpy(r.m, op.m, 32 * sizeof(double));
    std::memcpy(r.w, w[k], sizeof(r.w));
  }
  out[0].flat = flat ? 1 : 0;
  return AQC_OK;
}

// validates the program and writes its device rows; *nev = the number of events (Kraus rows and groups)
int build_rows(int n, const aqc_op_t* prog, int nprog, std::vector<TrajRow>& rows, int* nev) {
  rows.assign((size_t)nprog, TrajRow());
  int ev = 0;
  for (int i = 0; i < nprog; ++i) {
    const aqc_op_t& op = prog[i];
    TrajRow& r = rows[i];
    std::memset(&r, 0, sizeof(r));
    if (op.flags == 0) {
      if (!(op.nq == 1 || op.nq == 2) || op.q0 < 0 || op.q0 >= n) return fail("gate row: bad qubits");
      if (op.nq == 2 && (op.q1 < 0 || op.q1 >= n || op.q1 == op.q0)) return fail("gate row: bad qubits");
      r.kind = op.nq == 1 ? kGate1 : kGate2;
      r.q0 = op.q0;
      r.q1 = op.nq == 2 ? op.q1 : 0;
      std::memcpy(r.m, op.m, (op.nq == 1 ? 8 : 32) * sizeof(double));
    } else if (op.flags == AQC_OP_KRAUS1) {
      if (op.nq != 1 || op.q0 < 0 || op.q0 >= n || op.q1 < 1 || op.q1 > 4) return fail("malformed Kraus row");
      r.kind = kKraus;
      r.q0 = op.q0;
      r.nk = op.q1;
      r.ev = ev++;
      std::memcpy(r.m, op.m, 8 * (size_t)op.q1 * sizeof(double));
      double s00 = 0.0, s11 = 0.0, sx = 0.0, sy = 0.0;
      for (int k = 0; k < op.q1; ++k) {
        const double* K = op.m + 8 * k;  // K00 K01 K10 K11 as (re, im)
        for (int e = 0; e < 8; ++e)
          if (!std::isfinite(K[e])) return fail("malformed Kraus row");
        const double m00 = K[0] * K[0] + K[1] * K[1] + K[4] * K[4] + K[5] * K[5];
        const double m11 = K[2] * K[2] + K[3] * K[3] + K[6] * K[6] + K[7] * K[7];
        // M01 = conj(K00) K01 + conj(K10) K11
        const double mx = K[0] * K[2] + K[1] * K[3] + K[4] * K[6] + K[5] * K[7];
        const double my = K[0] * K[3] - K[1] * K[2] + K[4] * K[7] - K[5] * K[6];
        r.w[4 * k] = m00, r.w[4 * k + 1] = m11, r.w[4 * k + 2] = mx, r.w[4 * k + 3] = my;
        s00 += m00, s11 += m11, sx += mx, sy += my;
      }
      if (std::fabs(s00 - 1.0) > 1e-9 || std::fabs(s11 - 1.0) > 1e-9 || std::fabs(sx) > 1e-9 || std::fabs(sy) > 1e-9)
        return fail("Kraus row: sum K^dag K is not the identity");
    } else if ((op.flags & 0xff) == AQC_OP_KRAUS2) {
      const int nk = (op.flags >> 16) & 0xff;
      if (const char* why = aqc::kraus2_first_row_error(op, n, nprog - i)) return fail(why);
      if (int rc = build_group(prog + i, nk, &rows[i], ev++)) return rc;
      i += nk - 1;
    } else {
      return fail("unknown row flags");
    }
  }
  *nev = ev;
  return AQC_OK;
}

int threads_for(int n) {  // a quarter of the amplitudes, within 64 .. 512
  const int t = n >= 2 ? 1 << (n - 2) : 1;
  return std::max(64, std::min(kMaxThreads, t));
}

// workgroups for ntraj trajectories of n qubits
int grid_for(int n, int ntraj, int threads, bool k2, int* grid) {
  const size_t dim = (size_t)1 << n;
  if (n <= kLdsMaxQubits) {
    int dev = 0, cus = 0;
    AQC_HIP_CHECK(hipGetDevice(&dev));
    AQC_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    // workgroups that fit a CU together: LDS (160 KB), 32 waves, and at most 8
    const size_t lds = dim * sizeof(cplx) + side_bytes(k2);
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>({(size_t)160 * 1024 / lds, (size_t)(2048 / threads), 8}));
    *grid = (int)std::min<size_t>((size_t)ntraj, (size_t)std::max(cus, 1) * per_cu);
  } else {
    *grid = (int)std::max<size_t>(
        1, std::min<size_t>({(size_t)ntraj, (size_t)kMaxGlobalWgs, kMaxGlobalBytes / (dim * sizeof(cplx))}));
  }
  return AQC_OK;
}

template <int MODE, int END, bool K2>
int launch_as(const TrajJob& j, int grid, int threads) {
  const size_t dyn = (MODE == kLds ? ((size_t)1 << j.n) * sizeof(cplx) : 0) + side_bytes(K2);
  if (int e = aqc::allow_dynamic_lds((const void*)k_sv_traj<MODE, END, K2>, (int)dyn)) return e;
  hipLaunchKernelGGL((k_sv_traj<MODE, END, K2>), dim3(grid), dim3(threads), dyn, 0, j);
  return AQC_OK;
}

// k2: the program holds a Kraus group
template <int END>
int launch(const TrajJob& j, int grid, int threads, bool in_lds, bool k2) {
  if (in_lds) return k2 ? launch_as<kLds, END, true>(j, grid, threads) : launch_as<kLds, END, false>(j, grid, threads);
  return k2 ? launch_as<kGlobal, END, true>(j, grid, threads) : launch_as<kGlobal, END, false>(j, grid, threads);
}

}  // namespace

extern "C" int aqc_sv_traj_sample(int n, const aqc_op_t* prog, int nprog, int nshots, uint64_t seed, uint64_t run,
                                  const double* u, uint64_t* out, uint8_t* choices) {
  t_entry = "aqc_sv_traj_sample";
  AQC_REQUIRE(out && nprog >= 0 && (prog || nprog == 0), "aqc_sv_traj_sample: null argument");
  AQC_REQUIRE(n >= 1 && n <= kMaxQubits, "aqc_sv_traj_sample: n must be in 1 .. 24");
  AQC_REQUIRE(nshots >= 1 && nshots <= kMaxShots, "aqc_sv_traj_sample: nshots must be in 1 .. 2^30");
  std::vector<TrajRow> rows;
  int nev = 0;
  if (int rc = build_rows(n, prog, nprog, rows, &nev)) return rc;
  const bool k2 = std::any_of(rows.begin(), rows.end(), [](const TrajRow& r) { return r.kind == kKraus2; });
  const size_t nu = (size_t)nshots * (nev + 1);
  if (u)
    for (size_t e = 0; e < nu; ++e)
      if (!(u[e] >= 0.0 && u[e] < 1.0)) return fail("u must lie in [0, 1)");
  const bool want_choices = choices && nev > 0;
  const size_t dim = (size_t)1 << n;
  const bool in_lds = n <= kLdsMaxQubits;
  const int threads = threads_for(n);
  int grid = 0;
  if (int rc = grid_for(n, nshots, threads, k2, &grid)) return rc;
  const size_t pb = up256(std::max<size_t>(1, rows.size()) * sizeof(TrajRow));
  const size_t ub = u ? up256(nu * sizeof(double)) : 0;
  const size_t ob = up256((size_t)nshots * sizeof(uint64_t));
  const size_t cb = want_choices ? up256((size_t)nshots * nev) : 0;
  const size_t wb = in_lds ? 0 : (size_t)grid * dim * sizeof(cplx);
  hipStream_t st = nullptr;
  AQC_HIP_CHECK(hipDeviceSynchronize());  // (the scratch may be regrown)
  aqc::DevScratch& sc = g_scr.here();
  if (int rc = sc.ensure(pb + ub + ob + cb + wb)) return rc;
  char* buf = sc.dev;
  TrajJob j;
  std::memset(&j, 0, sizeof(j));
  j.prog = (const TrajRow*)buf;
  j.nprog = nprog;
  j.n = n;
  j.nshots = nshots;
  j.nev = nev;
  j.ustride = nev + 1;
  j.u = u ? (const double*)(buf + pb) : nullptr;
  j.seed = seed;
  j.run = run;
  j.out = (uint64_t*)(buf + pb + ub);
  j.choices = want_choices ? (uint8_t*)(buf + pb + ub + ob) : nullptr;
  j.ws = in_lds ? nullptr : (cplx*)(buf + pb + ub + ob + cb);
  if (!rows.empty())
    AQC_HIP_CHECK(hipMemcpyAsync(buf, rows.data(), rows.size() * sizeof(TrajRow), hipMemcpyHostToDevice, st));
  if (u) AQC_HIP_CHECK(hipMemcpyAsync(buf + pb, u, nu * sizeof(double), hipMemcpyHostToDevice, st));
  aqc::KernelTimer::begin(st, "sv_traj", 0.0, (double)nshots * (double)nprog * (double)dim * 14.0);
  const int rc = launch<kEndDraw>(j, grid, threads, in_lds, k2);
  aqc::KernelTimer::end(st);
  if (rc != AQC_OK) return rc;
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipMemcpyAsync(out, j.out, (size_t)nshots * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (want_choices)
    AQC_HIP_CHECK(hipMemcpyAsync(choices, j.choices, (size_t)nshots * nev, hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  return AQC_OK;
}

extern "C" int aqc_sv_traj_pair_tomo(int n, const aqc_op_t* prog, int nprog, const int* pairs, int npairs,
                                     const double* effects, int nshots, uint64_t seed, uint64_t run, const double* u,
                                     int64_t* counts, uint8_t* outcomes) {
  t_entry = "aqc_sv_traj_pair_tomo";
  AQC_REQUIRE(counts && pairs && effects && nprog >= 0 && (prog || nprog == 0), "aqc_sv_traj_pair_tomo: null argument");
  AQC_REQUIRE(n >= 2 && n <= kMaxQubits, "aqc_sv_traj_pair_tomo: n must be in 2 .. 24");
  AQC_REQUIRE(npairs >= 1 && npairs <= kMaxPairs, "aqc_sv_traj_pair_tomo: npairs must be in 1 .. 4096");
  AQC_REQUIRE(nshots >= 1 && nshots <= kMaxShots / 9, "aqc_sv_traj_pair_tomo: 9 nshots must be in 9 .. 2^30");
  for (int p = 0; p < npairs; ++p) {
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    if (a < 0 || a >= n || b < 0 || b >= n || a == b) return fail("a pair needs two different qubits in 0 .. n-1");
  }
  if (int rc = aqc::check_effects(n, effects, t_entry)) return rc;
  std::vector<TrajRow> rows;
  int nev = 0;
  if (int rc = build_rows(n, prog, nprog, rows, &nev)) return rc;
  const bool k2 = std::any_of(rows.begin(), rows.end(), [](const TrajRow& r) { return r.kind == kKraus2; });
  const int ntraj = 9 * nshots;
  const int ustride = nev + npairs;
  const size_t nu = (size_t)ntraj * ustride;
  if (u)
    for (size_t e = 0; e < nu; ++e)
      if (!(u[e] >= 0.0 && u[e] < 1.0)) return fail("u must lie in [0, 1)");
  const size_t dim = (size_t)1 << n;
  const bool in_lds = n <= kLdsMaxQubits;
  const int threads = threads_for(n);
  int grid = 0;
  if (int rc = grid_for(n, ntraj, threads, k2, &grid)) return rc;
  const size_t pb = up256(std::max<size_t>(1, rows.size()) * sizeof(TrajRow));
  const size_t ub = u ? up256(nu * sizeof(double)) : 0;
  const size_t qb = up256((size_t)npairs * 2 * sizeof(int));
  const size_t eb = up256((size_t)n * 24 * sizeof(double));
  const size_t tb = up256((size_t)npairs * 36 * sizeof(int64_t));
  const size_t ob = outcomes ? up256((size_t)ntraj * npairs) : 0;
  const size_t wb = in_lds ? 0 : (size_t)grid * dim * sizeof(cplx);
  hipStream_t st = nullptr;
  AQC_HIP_CHECK(hipDeviceSynchronize());  // (the scratch may be regrown)
  aqc::DevScratch& sc = g_scr.here();
  if (int rc = sc.ensure(pb + ub + qb + eb + tb + ob + wb)) return rc;
  char* buf = sc.dev;
  TrajJob j;
  std::memset(&j, 0, sizeof(j));
  j.prog = (const TrajRow*)buf;
  j.nprog = nprog;
  j.n = n;
  j.nshots = ntraj;
  j.nev = nev;
  j.ustride = ustride;
  j.u = u ? (const double*)(buf + pb) : nullptr;
  j.seed = seed;
  j.run = run;
  j.npairs = npairs;
  j.pairs = (const int*)(buf + pb + ub);
  j.effects = (const double*)(buf + pb + ub + qb);
  j.counts = (unsigned long long*)(buf + pb + ub + qb + eb);
  j.outcomes = outcomes ? (uint8_t*)(buf + pb + ub + qb + eb + tb) : nullptr;
  j.ws = in_lds ? nullptr : (cplx*)(buf + pb + ub + qb + eb + tb + ob);
  if (!rows.empty())
    AQC_HIP_CHECK(hipMemcpyAsync(buf, rows.data(), rows.size() * sizeof(TrajRow), hipMemcpyHostToDevice, st));
  if (u) AQC_HIP_CHECK(hipMemcpyAsync(buf + pb, u, nu * sizeof(double), hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemcpyAsync((void*)j.pairs, pairs, (size_t)npairs * 2 * sizeof(int), hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemcpyAsync((void*)j.effects, effects, (size_t)n * 24 * sizeof(double), hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemsetAsync(j.counts, 0, (size_t)npairs * 36 * sizeof(int64_t), st));
  aqc::KernelTimer::begin(st, "sv_traj_pair_tomo", 0.0,
                          (double)ntraj * ((double)nprog * 14.0 + (double)npairs * 10.0) * (double)dim);
  const int rc = launch<kEndPairs>(j, grid, threads, in_lds, k2);
  aqc::KernelTimer::end(st);
  if (rc != AQC_OK) return rc;
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipMemcpyAsync(counts, j.counts, (size_t)npairs * 36 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  if (outcomes)
    AQC_HIP_CHECK(hipMemcpyAsync(outcomes, j.outcomes, (size_t)ntraj * npairs, hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  return AQC_OK;
}

namespace {

// The term records of the Pauli readout from the codes (nterms x n; 0 I, 1 X, 2 Y, 3 Z) and the effects:
// per qubit of a term's support D = E[q][c-1][0] - E[q][c-1][1]; a D that is a multiple of a Pauli
// matrix within 1e-14, entry by entry, goes into the masks and the scalar, any other into the general
// factors.
int build_terms(int n, const uint8_t* codes, int nterms, const double* effects, std::vector<PauliTerm>& terms) {
  constexpr double tol = 1e-14;
  terms.assign((size_t)nterms, PauliTerm());
  for (int t = 0; t < nterms; ++t) {
    PauliTerm& tm = terms[t];
    std::memset(&tm, 0, sizeof(tm));
    double scal = 1.0;
    int ny = 0, weight = 0;
    for (int q = 0; q < n; ++q) {
      const int c = codes[(size_t)t * n + q];
      if (c > 3) return fail("a Pauli code must be 0 (I), 1 (X), 2 (Y) or 3 (Z)");
      if (c == 0) continue;
      ++weight;
      const double* e0 = effects + (size_t)((q * 3 + c - 1) * 2) * 4;
      double d[4];
      for (int i = 0; i < 4; ++i) d[i] = e0[i] - e0[4 + i];
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
        if (tm.ng == kMaxGeneral)
          return fail("a term has more than 4 factors that are not a multiple of a Pauli matrix (the limit of "
                      "general factors per term is 4)");
        tm.gq[tm.ng] = q;
        std::memcpy(tm.g[tm.ng], d, sizeof(d));
        ++tm.ng;
      }
    }
    if (weight == 0) return fail("an all-identity term (its value is 1: the caller answers it)");
    // (-i)^ny: entry (k, k ^ 1) of Y is -i (-1)^k
    static const double ph[4][2] = {{1.0, 0.0}, {0.0, -1.0}, {-1.0, 0.0}, {0.0, 1.0}};
    tm.cr = scal * ph[ny & 3][0];
    tm.ci = scal * ph[ny & 3][1];
  }
  return AQC_OK;
}

}  // namespace

extern "C" int aqc_sv_traj_pauli_counts(int n, const aqc_op_t* prog, int nprog, const uint8_t* codes, int nterms,
                                        const double* effects, int nshots, uint64_t seed, uint64_t run, const double* u,
                                        int64_t* plus, double* values, uint8_t* outcomes) {
  t_entry = "aqc_sv_traj_pauli_counts";
  AQC_REQUIRE(plus && codes && effects && nprog >= 0 && (prog || nprog == 0), "aqc_sv_traj_pauli_counts: null argument");
  AQC_REQUIRE(n >= 1 && n <= kMaxQubits, "aqc_sv_traj_pauli_counts: n must be in 1 .. 24");
  AQC_REQUIRE(nterms >= 1 && nterms <= kMaxTerms, "aqc_sv_traj_pauli_counts: nterms must be in 1 .. 65536");
  AQC_REQUIRE(nshots >= 1 && nshots <= kMaxShots, "aqc_sv_traj_pauli_counts: nshots must be in 1 .. 2^30");
  if (int rc = aqc::check_effects(n, effects, t_entry)) return rc;
  std::vector<PauliTerm> terms;
  if (int rc = build_terms(n, codes, nterms, effects, terms)) return rc;
  std::vector<TrajRow> rows;
  int nev = 0;
  if (int rc = build_rows(n, prog, nprog, rows, &nev)) return rc;
  const bool k2 = std::any_of(rows.begin(), rows.end(), [](const TrajRow& r) { return r.kind == kKraus2; });
  const int ustride = nev + nterms;
  const size_t nu = (size_t)nshots * ustride;
  if (u)
    for (size_t e = 0; e < nu; ++e)
      if (!(u[e] >= 0.0 && u[e] < 1.0)) return fail("u must lie in [0, 1)");
  const size_t dim = (size_t)1 << n;
  const bool in_lds = n <= kLdsMaxQubits;
  const int threads = threads_for(n);
  int grid = 0;
  if (int rc = grid_for(n, nshots, threads, k2, &grid)) return rc;
  const size_t nout = (size_t)nshots * nterms;
  const size_t pb = up256(std::max<size_t>(1, rows.size()) * sizeof(TrajRow));
  const size_t ub = u ? up256(nu * sizeof(double)) : 0;
  const size_t tb = up256((size_t)nterms * sizeof(PauliTerm));
  const size_t cb = up256((size_t)nterms * sizeof(int64_t));
  const size_t vb = values ? up256(nout * sizeof(double)) : 0;
  const size_t ob = outcomes ? up256(nout) : 0;
  const size_t wb = in_lds ? 0 : (size_t)grid * dim * sizeof(cplx);
  hipStream_t st = nullptr;
  AQC_HIP_CHECK(hipDeviceSynchronize());  // (the scratch may be regrown)
  aqc::DevScratch& sc = g_scr.here();
  if (int rc = sc.ensure(pb + ub + tb + cb + vb + ob + wb)) return rc;
  char* buf = sc.dev;
  TrajJob j;
  std::memset(&j, 0, sizeof(j));
  j.prog = (const TrajRow*)buf;
  j.nprog = nprog;
  j.n = n;
  j.nshots = nshots;
  j.nev = nev;
  j.ustride = ustride;
  j.u = u ? (const double*)(buf + pb) : nullptr;
  j.seed = seed;
  j.run = run;
  j.nterms = nterms;
  j.terms = (const PauliTerm*)(buf + pb + ub);
  j.plus = (unsigned long long*)(buf + pb + ub + tb);
  j.values = values ? (double*)(buf + pb + ub + tb + cb) : nullptr;
  j.outcomes = outcomes ? (uint8_t*)(buf + pb + ub + tb + cb + vb) : nullptr;
  j.ws = in_lds ? nullptr : (cplx*)(buf + pb + ub + tb + cb + vb + ob);
  if (!rows.empty())
    AQC_HIP_CHECK(hipMemcpyAsync(buf, rows.data(), rows.size() * sizeof(TrajRow), hipMemcpyHostToDevice, st));
  if (u) AQC_HIP_CHECK(hipMemcpyAsync(buf + pb, u, nu * sizeof(double), hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemcpyAsync((void*)j.terms, terms.data(), (size_t)nterms * sizeof(PauliTerm), hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemsetAsync(j.plus, 0, (size_t)nterms * sizeof(int64_t), st));
  aqc::KernelTimer::begin(st, "sv_traj_pauli_counts", 0.0,
                          (double)nshots * ((double)nprog * 14.0 + (double)nterms * 12.0) * (double)dim);
  const int rc = launch<kEndPaulis>(j, grid, threads, in_lds, k2);
  aqc::KernelTimer::end(st);
  if (rc != AQC_OK) return rc;
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipMemcpyAsync(plus, j.plus, (size_t)nterms * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  if (values) AQC_HIP_CHECK(hipMemcpyAsync(values, j.values, nout * sizeof(double), hipMemcpyDeviceToHost, st));
  if (outcomes) AQC_HIP_CHECK(hipMemcpyAsync(outcomes, j.outcomes, nout, hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  return AQC_OK;
}
