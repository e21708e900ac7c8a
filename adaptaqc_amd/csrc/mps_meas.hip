// MPS measurements (the aqc_research.mps_operations quantities the cost functions read): the zero
// overlap, the Hamming-weight-1 amplitudes -- by full chains and through a window of rewritten
// sites -- and <a|b>.  They share the handle and the job staging with gate application (mps.hip,
// mps_internal.h) and nothing else.
#include <algorithm>
#include <cstring>

#include "mps_internal.h"

using aqc::cplx;

namespace {

using aqc::fresh_tid;
using aqc::StagingLease;
using aqc::wave_sum_d;

constexpr int kT = 256;

struct MeasJob {
  const cplx* gam;
  const double* lam;
  const int* dims;
  int n;
  int cap;
  cplx* out;
  cplx* vec;   // zero-chain scratch (2*(n+1)*cap)
};

__device__ __forceinline__ cplx site_a(const cplx* gam, const double* lam, int cap, int i, int s, int l,
                                        int r) {
  // A_i[s][l][r] = Gamma_i[s][l][r] * lambda_{i+1}[r]  (aqc_research _preprocess_mps)
  const size_t ss = (size_t)2 * cap * cap;
  return aqc::cscale(gam[(size_t)i * ss + (size_t)s * cap * cap + (size_t)l * cap + r],
                     lam[(size_t)(i + 1) * cap + r]);
}

// The left zero chain v <- v A_i[0] through every site, the running vectors in the dynamic LDS (two
// of vc complex; the caller has set ovz_lds[0] = 1 and passed a barrier): lanes along r, the four
// waves splitting l, their partials summed as (p0 + p1) + (p2 + p3).  STORE: bond b's vector also to
// L + b cap.  Returns which of the two vectors is the last.
template <bool STORE>
__device__ __forceinline__ int left_zero_chain(const MeasJob& j, int vc, int tid, cplx* L) {
  extern __shared__ cplx ovz_lds[];
  __shared__ cplx part[4][64];
  const int q = tid >> 6, lane = tid & 63;
  const int cap = j.cap, n = j.n;
  int cur = 0;
  for (int i = 0; i < n; ++i) {
    const int cl = j.dims[i], cr = j.dims[i + 1];
    for (int r0 = 0; r0 < cr; r0 += 64) {
      const int r = r0 + lane;
      cplx acc = aqc::cmk(0, 0);
      if (r < cr)
        for (int l = q; l < cl; l += 4) acc = aqc::cfma(ovz_lds[cur * vc + l], site_a(j.gam, j.lam, cap, i, 0, l, r), acc);
      part[q][lane] = acc;
      __syncthreads();
      if (q == 0 && r < cr) {
        const cplx s = aqc::cadd(aqc::cadd(part[0][lane], part[1][lane]), aqc::cadd(part[2][lane], part[3][lane]));
        ovz_lds[(cur ^ 1) * vc + r] = s;
        if (STORE) L[(size_t)(i + 1) * cap + r] = s;
      }
      __syncthreads();
    }
    cur ^= 1;
  }
  return cur;
}

// <0...0|psi>: v <- v A_i[0] from the left.  One workgroup per state.
// The running vectors in dynamic LDS sized by the batch's largest capacity (vc complex each): at
// capacity-1024 static arrays (48 KB) three of the bench's four workgroups per CU fit and its 1024
// states ran in two rounds (483 -> 761 us a launch).
__global__ __launch_bounds__(kT) void k_overlap_zero(const MeasJob* __restrict__ jobs, int vc) {
  const MeasJob& j = jobs[blockIdx.x];
  extern __shared__ cplx ovz_lds[];
  const int tid = fresh_tid();
  if (tid == 0) ovz_lds[0] = aqc::cmk(1.0, 0.0);
  __syncthreads();
  const int cur = left_zero_chain<false>(j, vc, tid, nullptr);
  if (tid == 0) j.out[0] = ovz_lds[cur * vc];
}

// Zero chains: vec[b] (left, bond b) = <0..0| A_0..A_{b-1};  vec[(n+1)+b] (right) = A_b..A_{n-1}|0..0>.
// blockIdx.y = 0 -> left chain, 1 -> right chain.  The running vector in the LDS; the left chain as
// k_overlap_zero (lanes along r, the four waves splitting l), the right one with lanes along r too
// (coalesced rows of A) and one wave sum per output row.  (Round 6: one thread per output entry
// with the whole dot product and the vector in global memory, columns of A read with a cap stride,
// made the softened-cost batch's HW-1 amplitudes ~2 ms a call.)
__global__ __launch_bounds__(kT) void k_zero_chains(const MeasJob* __restrict__ jobs, int vc) {
  const MeasJob& j = jobs[blockIdx.x];
  const int tid = fresh_tid(), q = tid >> 6, lane = tid & 63;
  const int cap = j.cap, n = j.n;
  cplx* L = j.vec;
  cplx* R = j.vec + (size_t)(n + 1) * cap;
  extern __shared__ cplx ovz_lds[];  // (as k_overlap_zero)
  if (tid == 0) ovz_lds[0] = aqc::cmk(1.0, 0.0);
  if (blockIdx.y == 0) {
    if (tid == 0) L[0] = aqc::cmk(1.0, 0.0);
    __syncthreads();
    left_zero_chain<true>(j, vc, tid, L);
  } else {
    int cur = 0;
    if (tid == 0) R[(size_t)n * cap] = aqc::cmk(1.0, 0.0);
    __syncthreads();
    for (int i = n - 1; i >= 0; --i) {
      const int cl = j.dims[i], cr = j.dims[i + 1];
      for (int l = q; l < cl; l += 4) {  // (uniform per wave)
        cplx acc = aqc::cmk(0, 0);
        for (int r = lane; r < cr; r += 64) acc = aqc::cfma(site_a(j.gam, j.lam, cap, i, 0, l, r), ovz_lds[cur * vc + r], acc);
        acc.x = wave_sum_d(acc.x);
        acc.y = wave_sum_d(acc.y);
        if (lane == 0) {
          ovz_lds[(cur ^ 1) * vc + l] = acc;
          R[(size_t)i * cap + l] = acc;
        }
      }
      __syncthreads();
      cur ^= 1;
    }
  }
}

// amp_i = <e_i|psi> = L[i] A_i[1] R[i+1].  blockIdx.x = site, blockIdx.y = job.
__global__ __launch_bounds__(kT) void k_hw1(const MeasJob* __restrict__ jobs) {
  const MeasJob& j = jobs[blockIdx.y];
  const int i = blockIdx.x;
  const int cap = j.cap, n = j.n;
  if (i >= n) return;
  const cplx* L = j.vec + (size_t)i * cap;
  const cplx* R = j.vec + (size_t)(n + 1) * cap + (size_t)(i + 1) * cap;
  const int cl = j.dims[i], cr = j.dims[i + 1];
  __shared__ double red[2][kT];
  cplx acc = aqc::cmk(0, 0);
  for (int e = threadIdx.x; e < cl * cr; e += kT) {
    const int l = e / cr, r = e % cr;
    acc = aqc::cfma(aqc::cmul(L[l], site_a(j.gam, j.lam, cap, i, 1, l, r)), R[r], acc);
  }
  red[0][threadIdx.x] = acc.x;
  red[1][threadIdx.x] = acc.y;
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) j.out[i] = aqc::cmk(red[0][0], red[1][0]);
}

// ---- zero and Hamming-weight-1 amplitudes through a window (round 6) --------------------------
// The global cost's <0|psi> and the softened cost's <e_i|psi> (aer_mps_backend.py:49-70, 88-93)
// are linear in every site tensor.  Rows from the left, per bond b: row 0 = <0..0| A_0 .. A_{b-1}
// (all sites on 0), row 1 + k = the same with site k < b on 1; from the right: row 0 =
// A_b .. A_{n-1} |0..0>, row 1 + k = with site k >= b on 1.  A Rotoselect candidate differs from
// the prefix only on the sites lo..hi it rewrote, so with the prefix's left rows at bond lo (Ml) and
// right rows at bond hi + 1 (Nr), cached on the prefix handle, and the candidate's own row-0
// vectors through the window, u_b (from Ml[0], bonds lo .. hi + 1) and y_b (from Nr[0], bonds
// hi + 1 .. lo):
//   <0|psi> = u_b . y_b (any window bond: the two chains meet in the middle when only it is asked)
//   amp_k   = Ml[1 + k] . y_lo (k < lo),  u_k A_k[1] y_{k+1} (lo <= k <= hi),  u_{hi+1} . Nr[1 + k] (k > hi)
// -- w small vector steps per candidate instead of two n-step chains and n closings.
//
// One vector step for up to kHwR vectors at once (the same site): left out_r[c] = sum_l v_r[l] A_t[l][c],
// right out_r[l] = sum_c A_t[l][c] v_r[c].  The four waves split the contraction, lanes run over
// 64 outputs, partial sums meet in the LDS (two barriers per 64 outputs); t = 1 for the rows
// flagged in newmask (the flipped site), A_0 otherwise.  src(r, k), dst(r, x, value).
constexpr int kHwR = 8;
template <typename FS, typename FD>
__device__ __forceinline__ void hw_step(const cplx* gam, const double* lam, int cap, int i, bool right, int nrows,
                                        unsigned newmask, int ke, int m2, FS src, FD dst, cplx (*part)[kHwR][64]) {
  const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t cc = (size_t)cap * cap;
  const cplx* g = gam + (size_t)i * 2 * cc;
  const double* lm = lam + (size_t)(i + 1) * cap;
  for (int x0 = 0; x0 < m2; x0 += 64) {
    const int x = x0 + lane;
    cplx acc[kHwR];
#pragma unroll
    for (int r = 0; r < kHwR; ++r) acc[r] = aqc::cmk(0, 0);
    if (x < m2) {
      for (int k = q; k < ke; k += 4) {
        // A_t[l][c] = Gamma_t[l][c] lambda_{i+1}[c]: left (l, c) = (k, x), right (x, k)
        const size_t o = right ? (size_t)x * cap + k : (size_t)k * cap + x;
        const double lv = lm[right ? k : x];
        const cplx a0 = aqc::cscale(g[o], lv);
        const cplx a1 = newmask ? aqc::cscale(g[cc + o], lv) : a0;
#pragma unroll
        for (int r = 0; r < kHwR; ++r)
          if (r < nrows) acc[r] = aqc::cfma(src(r, k), (newmask >> r) & 1 ? a1 : a0, acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < kHwR; ++r)
      if (r < nrows) part[q][r][lane] = acc[r];
    __syncthreads();
    for (int e = threadIdx.x; e < nrows * 64; e += kT) {
      const int r = e >> 6, ln = e & 63;
      if (x0 + ln < m2)
        dst(r, x0 + ln, aqc::cadd(aqc::cadd(part[0][r][ln], part[1][r][ln]), aqc::cadd(part[2][r][ln], part[3][r][ln])));
    }
    __syncthreads();
  }
}

struct HwRowsJob {
  const cplx* gam;
  const double* lam;
  const int* dims;
  int n, cap;
  int dir, first, nsteps;  // left: sites first .. first + nsteps - 1; right: first down
  int full;                // every row, or row 0 only
  cplx* rows;              // bond b's (n + 1) x cap block at rows + b (n + 1) cap
};

// The prefix's rows.  grid (directions, G): with `full`, workgroup g owns the flip rows 1 + k with
// k % G == g (each an independent chain once created) and every workgroup carries row 0 itself
// (workgroup 0 stores it), so the workgroups never wait on each other.  Every bond has its own
// block, written once per launch and read by the next step only (no stale L1 line); row 0 is also
// kept in the LDS.
constexpr int kHwRowsG = 8;
__global__ __launch_bounds__(kT) void k_hw_rows(const HwRowsJob* __restrict__ jobs) {
  const HwRowsJob& j = jobs[blockIdx.x];
  const int n = j.n, cap = j.cap, g = blockIdx.y, G = gridDim.y;
  const size_t blk = (size_t)(n + 1) * cap;
  extern __shared__ cplx hw_lds[];
  cplx* v0[2] = {hw_lds, hw_lds + cap};  // row 0, this workgroup's copy
  cplx (*part)[kHwR][64] = reinterpret_cast<cplx (*)[kHwR][64]>(hw_lds + 2 * cap);
  {
    const int b = j.dir == 0 ? j.first : j.first + 1, d = j.dims[b];
    for (int e = threadIdx.x; e < d; e += kT) v0[0][e] = j.rows[(size_t)b * blk + e];
  }
  __syncthreads();
  for (int s = 0; s < j.nsteps; ++s) {
    const int i = j.dir == 0 ? j.first + s : j.first - s;
    const bool right = j.dir != 0;
    const int ke = right ? j.dims[i + 1] : j.dims[i], m2 = right ? j.dims[i] : j.dims[i + 1];
    const cplx* M = j.rows + (size_t)(right ? i + 1 : i) * blk;
    cplx* O = j.rows + (size_t)(right ? i : i + 1) * blk;
    const cplx* v = v0[s & 1];
    cplx* vn = v0[(s + 1) & 1];
    // this workgroup's rows: 0; the old flip rows k (left: k < i, right: k > i) with k % G == g;
    // the new row 1 + i (from row 0 with the site on 1) when i % G == g
    int k0 = 0, nold = 0;
    if (j.full) {
      if (!right) nold = i > g ? (i - g + G - 1) / G : 0, k0 = g;
      else {
        k0 = i + 1 + ((g - (i + 1) % G) % G + G) % G;
        nold = k0 < n ? (n - 1 - k0) / G + 1 : 0;
      }
    }
    const int nnew = j.full && i % G == g ? 1 : 0, nr = 1 + nold + nnew;
    // row list position p: 0 = row 0, 1 .. nold = old rows, nold + 1 = the new row
    auto row_of = [&](int p) { return p == 0 ? 0 : (p <= nold ? 1 + k0 + G * (p - 1) : 1 + i); };
    for (int p0 = 0; p0 < nr; p0 += kHwR) {
      const int cnt = min(kHwR, nr - p0);
      const unsigned nm = (nnew && nr - 1 >= p0 && nr - 1 < p0 + cnt) ? 1u << (nr - 1 - p0) : 0u;
      hw_step(
          j.gam, j.lam, cap, i, right, cnt, nm, ke, m2,
          [&](int r, int k) {
            const int p = p0 + r;
            return (p == 0 || p == nold + 1) ? v[k] : M[(size_t)row_of(p) * cap + k];
          },
          [&](int r, int x, cplx val) {
            const int p = p0 + r;
            if (p == 0) vn[x] = val;
            if (p != 0 || g == 0) O[(size_t)row_of(p) * cap + x] = val;
          },
          part);
    }
  }
}

struct HwWinJob {
  const cplx* gam;
  const double* lam;
  const int* dims;
  int n, cap, lo, hi;
  const cplx* ml;  // prefix's left rows at bond lo
  const cplx* nr;  // prefix's right rows at bond hi + 1
  cplx* ov;        // <0..0|psi> (the amplitude; the host conjugates for mps_dot(psi, zero))
  cplx* amps;      // n amplitudes, or nullptr
  cplx* uy;        // with amps: u_b at uy + (b - lo) cap, y_b at uy + (w + 1 + b - lo) cap
  cplx* fin;       // the two chains' last vectors (2 cap): u at fin, y at fin + cap
  int* cnt;        // the job's hand-off counter (0 at launch)
  int pad;
};

// Vectors handed between the two chains' workgroups (possibly on different XCDs): agent-scope
// stores and loads, as the environment chains' hand-offs (ent.hip)
typedef __attribute__((address_space(1))) double win_gdbl;
__device__ __forceinline__ void win_st(cplx* p, cplx v) {
  win_gdbl* q = (win_gdbl*)(double*)p;
  __hip_atomic_store(q, v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(q + 1, v.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ cplx win_ld(const cplx* p) {
  win_gdbl* q = (win_gdbl*)(double*)p;
  return aqc::cmk(__hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                  __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// One window step with the running vector v in the LDS (out in the LDS too, and to `store` when
// not null).  Left (site i, bond i -> i + 1): out[x] = sum_k v[k] A_i[0][k][x] -- lanes along x
// (coalesced rows of Gamma), the four waves splitting k, partial sums through the LDS.  Right (bond
// i + 1 -> i): out[x] = sum_k A_i[0][x][k] v[k] -- lanes along k (coalesced rows again), four
// outputs per wave in flight, wave sums.  A = Gamma lambda_{i+1}.
__device__ __forceinline__ void win_step(const cplx* __restrict__ gam, const double* __restrict__ lam, int cap, int i,
                                         bool right, int ke, int m2, const cplx* v, cplx* out, cplx* store,
                                         cplx (*part)[64]) {
  const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const cplx* g = gam + (size_t)i * 2 * cap * cap;
  const double* lm = lam + (size_t)(i + 1) * cap;
  if (!right) {
    for (int x0 = 0; x0 < m2; x0 += 64) {
      const int x = x0 + lane;
      cplx acc = aqc::cmk(0, 0);
      if (x < m2) {
        int k = q;
        for (; k + 12 < ke; k += 16) {  // four rows' loads issued together
          cplx a[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) a[t] = g[(size_t)(k + 4 * t) * cap + x];
#pragma unroll
          for (int t = 0; t < 4; ++t) acc = aqc::cfma(v[k + 4 * t], a[t], acc);
        }
        for (; k < ke; k += 4) acc = aqc::cfma(v[k], g[(size_t)k * cap + x], acc);
        acc = aqc::cscale(acc, lm[x]);
      }
      part[q][lane] = acc;
      __syncthreads();
      if (q == 0 && x < m2) {
        const cplx r = aqc::cadd(aqc::cadd(part[0][lane], part[1][lane]), aqc::cadd(part[2][lane], part[3][lane]));
        out[x] = r;
        if (store) win_st(store + x, r);
      }
      __syncthreads();
    }
  } else {
    for (int x0 = 4 * q; x0 < m2; x0 += 16) {  // (uniform per wave)
      // (four named sums: as an array the compiler kept them in scratch)
      cplx c0 = aqc::cmk(0, 0), c1 = c0, c2 = c0, c3 = c0;
      const bool h1 = x0 + 1 < m2, h2 = x0 + 2 < m2, h3 = x0 + 3 < m2;
      for (int k = lane; k < ke; k += 64) {
        const cplx vk = aqc::cscale(v[k], lm[k]);
        const cplx* gk = g + (size_t)x0 * cap + k;
        c0 = aqc::cfma(gk[0], vk, c0);
        if (h1) c1 = aqc::cfma(gk[cap], vk, c1);
        if (h2) c2 = aqc::cfma(gk[2 * (size_t)cap], vk, c2);
        if (h3) c3 = aqc::cfma(gk[3 * (size_t)cap], vk, c3);
      }
      c0.x = wave_sum_d(c0.x), c0.y = wave_sum_d(c0.y);
      c1.x = wave_sum_d(c1.x), c1.y = wave_sum_d(c1.y);
      c2.x = wave_sum_d(c2.x), c2.y = wave_sum_d(c2.y);
      c3.x = wave_sum_d(c3.x), c3.y = wave_sum_d(c3.y);
      if (lane < 4 && x0 + lane < m2) {
        cplx r = c0;
        if (lane == 1) r = c1;
        if (lane == 2) r = c2;
        if (lane == 3) r = c3;
        out[x0 + lane] = r;
        if (store) win_st(store + x0 + lane, r);
      }
    }
    __syncthreads();
  }
}

// Two workgroups per state (blockIdx.y): the left chain u through sites lo .. lo + nl - 1 (bond lo
// -> lo + nl) and the right chain y through hi .. hi - ny + 1 (bond hi + 1 -> hi + 1 - ny) run side
// by side; without amplitudes they meet at bond lo + nl, with them both run the whole window.
// Each writes its last vector to fin; the second to finish (the job's counter) closes: <0|psi> =
// u . y and, with amps, the window's amplitudes from the bond vectors in uy (every vector written
// once to global memory before the hand-off, read after it).  Dynamic LDS: two vectors (2 cap)
// and the step partials.  (One workgroup running the two chains one step after the other: ~190 us
// a launch in the paper-setting layer, lanes strided by cap on the right chain's rows.)
__global__ __launch_bounds__(kT) void k_hw_win(const HwWinJob* __restrict__ jobs) {
  const HwWinJob& j = jobs[blockIdx.x];
  const int side = blockIdx.y;
  extern __shared__ cplx hw_lds[];
  const int cap = j.cap, n = j.n, lo = j.lo, hi = j.hi, w = hi - lo + 1;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  cplx (*part)[64] = reinterpret_cast<cplx (*)[64]>(hw_lds + 2 * cap);
  const bool amps = j.amps != nullptr;
  const int nl = amps ? w : (w + 1) / 2, ny = amps ? w : w - nl;
  cplx* U = j.uy;
  cplx* Y = j.uy + (size_t)(w + 1) * cap;
  const int steps = side == 0 ? nl : ny;
  {
    const int d0 = side == 0 ? j.dims[lo] : j.dims[hi + 1];
    const cplx* src = side == 0 ? j.ml : j.nr;
    cplx* st0 = amps ? (side == 0 ? U : Y + (size_t)w * cap) : nullptr;
    for (int e = tid; e < d0; e += kT) {
      hw_lds[e] = src[e];
      if (st0) win_st(st0 + e, src[e]);
    }
  }
  __syncthreads();
  if (cap <= 64) {
    // capacity <= 64: a step's whole 64 x 64 tile is 16 entries per thread, all loaded at once --
    // and the next step's issued before this step's products (the tiles do not depend on the
    // running vector), so a step waits on no global load.  Left: thread (q, x) holds A[q + 4t][x];
    // right: thread (q, k) holds A[q + 4t][k] (rows along the lanes either way: coalesced), its 16
    // products reduced over k through the LDS (red, 64 x 65).
    cplx (*red)[65] = reinterpret_cast<cplx (*)[65]>(hw_lds + 2 * cap + 4 * 64);
    auto site_of = [&](int s) { return side == 0 ? lo + s : hi - s; };
    auto fetch = [&](int s, cplx (&a)[16]) {
      const int i = site_of(s);
      const int rows = side == 0 ? j.dims[i] : j.dims[i];      // A's row count (left: k; right: x)
      const int cols = side == 0 ? j.dims[i + 1] : j.dims[i + 1];
      const cplx* g = j.gam + (size_t)i * 2 * cap * cap;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int r = wave + 4 * t;
        a[t] = (r < rows && lane < cols) ? g[(size_t)r * cap + lane] : aqc::cmk(0, 0);
      }
    };
    cplx a[16], an[16];
    if (steps > 0) fetch(0, a);
    for (int s = 0; s < steps; ++s) {
      if (s + 1 < steps) fetch(s + 1, an);
      const int i = site_of(s);
      const cplx* v = hw_lds + (s & 1) * cap;
      cplx* vn = hw_lds + ((s + 1) & 1) * cap;
      const double* lm = j.lam + (size_t)(i + 1) * cap;
      if (side == 0) {  // out[x] = lambda[x] sum_k v[k] A[k][x], x = lane
        const int ke = j.dims[i], m2 = j.dims[i + 1];
        cplx acc = aqc::cmk(0, 0);
#pragma unroll
        for (int t = 0; t < 16; ++t)
          if (wave + 4 * t < ke) acc = aqc::cfma(v[wave + 4 * t], a[t], acc);
        part[wave][lane] = acc;
        __syncthreads();
        if (wave == 0 && lane < m2) {
          const cplx r = aqc::cscale(aqc::cadd(aqc::cadd(part[0][lane], part[1][lane]), aqc::cadd(part[2][lane], part[3][lane])),
                                     lm[lane]);
          vn[lane] = r;
          if (amps) win_st(U + (size_t)(s + 1) * cap + lane, r);
        }
      } else {  // out[x] = sum_k A[x][k] lambda[k] v[k], k = lane
        const int ke = j.dims[i + 1], m2 = j.dims[i];
        const cplx vk = lane < ke ? aqc::cscale(v[lane], lm[lane]) : aqc::cmk(0, 0);
#pragma unroll
        for (int t = 0; t < 16; ++t) red[wave + 4 * t][lane] = aqc::cmul(a[t], vk);
        __syncthreads();
        {  // thread (x = tid / 4, quarter p = tid % 4): 16 k's, then the four quarters by shuffles
          const int x = tid >> 2, p = tid & 3;
          cplx acc = aqc::cmk(0, 0);
#pragma unroll
          for (int c = 0; c < 16; ++c) acc = aqc::cadd(acc, red[x][16 * p + c]);
          acc.x += __shfl_xor(acc.x, 1);
          acc.y += __shfl_xor(acc.y, 1);
          acc.x += __shfl_xor(acc.x, 2);
          acc.y += __shfl_xor(acc.y, 2);
          if (p == 0 && x < m2) {
            vn[x] = acc;
            if (amps) win_st(Y + (size_t)(i - lo) * cap + x, acc);
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 16; ++t) a[t] = an[t];
    }
  } else
  for (int s = 0; s < steps; ++s) {
    const cplx* v = hw_lds + (s & 1) * cap;
    cplx* vn = hw_lds + ((s + 1) & 1) * cap;
    if (side == 0) {
      const int i = lo + s;
      win_step(j.gam, j.lam, cap, i, false, j.dims[i], j.dims[i + 1], v, vn, amps ? U + (size_t)(s + 1) * cap : nullptr,
               part);
    } else {
      const int i = hi - s;
      win_step(j.gam, j.lam, cap, i, true, j.dims[i + 1], j.dims[i], v, vn, amps ? Y + (size_t)(i - lo) * cap : nullptr,
               part);
    }
  }
  {
    const cplx* v = hw_lds + (steps & 1) * cap;
    const int d = side == 0 ? j.dims[lo + nl] : j.dims[hi + 1 - ny];
    for (int e = tid; e < d; e += kT) win_st(j.fin + (size_t)side * cap + e, v[e]);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  __shared__ int last;
  if (tid == 0) last = __hip_atomic_fetch_add(j.cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1;
  __syncthreads();
  if (!last) return;
  const cplx* u = j.fin;        // at bond lo + nl
  const cplx* y = j.fin + cap;  // at bond hi + 1 - ny
  const int dl = j.dims[lo], dr = j.dims[hi + 1];
  // closings, a wave per output, lanes along the bond: output 0 = <0|psi>, 1 + k = amp_k (with
  // amps; window sites as u_k A_k[1] y_{k+1}: lanes along the right index, a loop over the left)
  const int nout = amps ? n + 1 : 1;
  for (int o = wave; o < nout; o += kT / 64) {  // (uniform per wave)
    const int k = o - 1;
    cplx acc = aqc::cmk(0, 0);
    if (o == 0) {  // (with amps u is at bond hi + 1: against Nr[0]; else the chains' meeting bond)
      const cplx* yy = amps ? j.nr : y;
      const int d = j.dims[lo + nl];
      for (int c = lane; c < d; c += 64) acc = aqc::cfma(win_ld(u + c), amps ? yy[c] : win_ld(yy + c), acc);
    } else if (k < lo) {
      for (int c = lane; c < dl; c += 64) acc = aqc::cfma(j.ml[(size_t)(1 + k) * cap + c], win_ld(y + c), acc);
    } else if (k > hi) {
      for (int c = lane; c < dr; c += 64) acc = aqc::cfma(win_ld(u + c), j.nr[(size_t)(1 + k) * cap + c], acc);
    } else {
      const cplx* uk = U + (size_t)(k - lo) * cap;
      const cplx* yk = Y + (size_t)(k + 1 - lo) * cap;
      const int kl = j.dims[k], kr = j.dims[k + 1];
      for (int r = lane; r < kr; r += 64) {
        cplx t = aqc::cmk(0, 0);
        for (int l = 0; l < kl; ++l) t = aqc::cfma(win_ld(uk + l), site_a(j.gam, j.lam, cap, k, 1, l, r), t);
        acc = aqc::cfma(t, win_ld(yk + r), acc);
      }
    }
    acc.x = wave_sum_d(acc.x);
    acc.y = wave_sum_d(acc.y);
    if (lane == 0) {
      if (o == 0) j.ov[0] = acc;
      else j.amps[k] = acc;
    }
  }
}

// Transfer-matrix environments of <a|b> (one workgroup per chain):
//   left : E_{i+1}[ra][rb] = sum_s sum_{la,lb} conj(A_i[s][la][ra]) E_i[la][lb] B_i[s][lb][rb]
//   right: E_i[la][lb]     = sum_s sum_{ra,rb} conj(A_i[s][la][ra]) B_i[s][lb][rb] E_{i+1}[ra][rb]
// With keep_all, every bond's environment is stored (env + b*cap*cap), else only the final one.
struct EnvJob {
  const cplx* ga;
  const double* la;
  const int* da;
  const cplx* gb;
  const double* lb;
  const int* db;
  int n;
  int cap;
  cplx* env;  // (n+1) * cap * cap if keep_all, else 2 * cap*cap ping-pong
  cplx* tmp;  // 2 * cap * cap
  int keep_all;
  int right;
  cplx* out;
};

__global__ __launch_bounds__(kT) void k_env(const EnvJob* __restrict__ jobs) {
  const EnvJob& j = jobs[blockIdx.x];
  const int tid = fresh_tid();
  const int cap = j.cap, n = j.n;
  const size_t cc = (size_t)cap * cap;
  auto envp = [&](int b) -> cplx* { return j.keep_all ? j.env + (size_t)b * cc : j.env + (size_t)(b & 1) * cc; };
  if (!j.right) {
    if (tid == 0) envp(0)[0] = aqc::cmk(1.0, 0.0);
    __syncthreads();
    for (int i = 0; i < n; ++i) {
      const int la = j.da[i], ra = j.da[i + 1], lb = j.db[i], rb = j.db[i + 1];
      const cplx* E = envp(i);
      cplx* En = envp(i + 1);
      // X[s][la][rb] = sum_lb E[la][lb] B[s][lb][rb]   (X in tmp, ld = cap)
      for (int e = tid; e < 2 * la * rb; e += kT) {
        const int s = e / (la * rb), rem = e % (la * rb), a = rem / rb, c = rem % rb;
        cplx acc = aqc::cmk(0, 0);
        for (int b = 0; b < lb; ++b) acc = aqc::cfma(E[(size_t)a * cap + b], site_a(j.gb, j.lb, cap, i, s, b, c), acc);
        j.tmp[(size_t)s * cc + (size_t)a * cap + c] = acc;
      }
      __syncthreads();
      for (int e = tid; e < ra * rb; e += kT) {
        const int a = e / rb, c = e % rb;
        cplx acc = aqc::cmk(0, 0);
        for (int s = 0; s < 2; ++s)
          for (int x = 0; x < la; ++x)
            acc = aqc::cfmac(site_a(j.ga, j.la, cap, i, s, x, a), j.tmp[(size_t)s * cc + (size_t)x * cap + c], acc);
        En[(size_t)a * cap + c] = acc;
      }
      __syncthreads();
    }
    if (tid == 0 && j.out) j.out[0] = envp(n)[0];
  } else {
    if (tid == 0) envp(n)[0] = aqc::cmk(1.0, 0.0);
    __syncthreads();
    for (int i = n - 1; i >= 0; --i) {
      const int la = j.da[i], ra = j.da[i + 1], lb = j.db[i], rb = j.db[i + 1];
      const cplx* E = envp(i + 1);
      cplx* En = envp(i);
      // Y[s][lb][ra] = sum_rb B[s][lb][rb] E[ra][rb]
      for (int e = tid; e < 2 * lb * ra; e += kT) {
        const int s = e / (lb * ra), rem = e % (lb * ra), b = rem / ra, a = rem % ra;
        cplx acc = aqc::cmk(0, 0);
        for (int c = 0; c < rb; ++c) acc = aqc::cfma(site_a(j.gb, j.lb, cap, i, s, b, c), E[(size_t)a * cap + c], acc);
        j.tmp[(size_t)s * cc + (size_t)b * cap + a] = acc;
      }
      __syncthreads();
      for (int e = tid; e < la * lb; e += kT) {
        const int a = e / lb, b = e % lb;
        cplx acc = aqc::cmk(0, 0);
        for (int s = 0; s < 2; ++s)
          for (int x = 0; x < ra; ++x)
            acc = aqc::cfmac(site_a(j.ga, j.la, cap, i, s, a, x), j.tmp[(size_t)s * cc + (size_t)b * cap + x], acc);
        En[(size_t)a * cap + b] = acc;
      }
      __syncthreads();
    }
    if (tid == 0 && j.out) j.out[0] = envp(0)[0];
  }
}

MeasJob make_meas(aqc_mps_t h, cplx* out) {
  return MeasJob{h->d.gam, h->d.lam, h->d.dims, h->d.n, h->d.cap, out, h->d.vec};
}

}  // namespace

extern "C" {

int aqc_mps_overlap_zero_batch(aqc_mps_t* hs, int ns, double* out) {
  AQC_REQUIRE(hs && out && ns >= 0, "aqc_mps_overlap_zero_batch: null argument");
  if (ns == 0) return AQC_OK;
  int rc = aqc_mps_sort_batch(hs, ns);
  if (rc != AQC_OK) return rc;
  // results (ns complex) and the states' gathered error flags (ns ints) in one device buffer: one
  // read-back for both (the caller needs no aqc_mps_check_batch round trip after it)
  static aqc::PerDevice<aqc::DevScratch> dres_tab;
  aqc::DevScratch& dres = dres_tab.here();
  hipStream_t st = aqc::mps_stream();
  const size_t rbytes = (size_t)ns * sizeof(cplx), need = rbytes + (size_t)ns * sizeof(int);
  if (dres.cap < need) AQC_HIP_CHECK(hipStreamSynchronize(st));
  rc = dres.ensure(need);
  if (rc != AQC_OK) return rc;
  cplx* dr = (cplx*)dres.dev;
  int* dflags = (int*)(dres.dev + rbytes);
  // the jobs and flag pointers through a pinned staging set of the ring: no wait for the stream's
  // earlier work (the chain that wrote the states) before these launches are queued
  StagingLease lease(st);
  if (lease.rc() != AQC_OK) return lease.rc();
  const size_t jb = aqc::up256(ns * sizeof(MeasJob)), fpb = (size_t)ns * sizeof(int*);
  rc = lease.ensure(jb + fpb);
  if (rc != AQC_OK) return rc;
  char* hj = lease.buf().host;
  char* dj = lease.buf().dev;
  MeasJob* hjobs = (MeasJob*)hj;
  for (int s = 0; s < ns; ++s) hjobs[s] = make_meas(hs[s], dr + s);  // one contiguous result array
  aqc::flag_ptrs(hs, ns, (int**)(hj + jb));
  if (int e = aqc::upload_async(dj, hj, jb + fpb, st)) return e;
  double bytes = 0;
  for (int s = 0; s < ns; ++s) bytes += (double)hs[s]->d.n * hs[s]->d.cap * hs[s]->d.cap * 16.0;
  aqc::KernelTimer::begin(st, "mps_overlap0", bytes, bytes / 2.0);
  int vc = 1;
  for (int s = 0; s < ns; ++s) vc = std::max(vc, hs[s]->d.cap);
  hipLaunchKernelGGL(k_overlap_zero, dim3(ns), dim3(kT), 2 * vc * sizeof(cplx), st, (const MeasJob*)dj, vc);
  aqc::KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  rc = aqc::queue_flag_gather((int* const*)(dj + jb), ns, dflags, st);
  if (rc != AQC_OK) return rc;
  std::vector<char> hv(need);
  AQC_HIP_CHECK(hipMemcpyAsync(hv.data(), dres.dev, need, hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  const cplx* v = (const cplx*)hv.data();
  rc = aqc::settle_flags(hs, ns, (const int*)(hv.data() + rbytes));
  if (rc != AQC_OK) return rc;
  for (int s = 0; s < ns; ++s) {
    // mps_dot(psi, zero) = <psi|0..0> = conj(amplitude of |0..0>)
    out[2 * s] = v[s].x;
    out[2 * s + 1] = -v[s].y;
  }
  return AQC_OK;
}

int aqc_mps_overlap_zero(aqc_mps_t h, double* re, double* im) {
  AQC_REQUIRE(re && im, "aqc_mps_overlap_zero: null argument");
  double o[2];
  int rc = aqc_mps_overlap_zero_batch(&h, 1, o);
  *re = o[0];
  *im = o[1];
  return rc;
}

int aqc_mps_amps_hw1_batch(aqc_mps_t* hs, int ns, double* out) {
  AQC_REQUIRE(hs && ns >= 0 && (out || ns == 0), "aqc_mps_amps_hw1_batch: null argument");
  if (ns == 0) return AQC_OK;
  const int n = hs[0]->d.n;
  for (int s = 0; s < ns; ++s) AQC_REQUIRE(hs[s] && hs[s]->d.n == n, "aqc_mps_amps_hw1_batch: all states need the same n");
  int rc = aqc_mps_sort_batch(hs, ns);
  if (rc != AQC_OK) return rc;
  static aqc::PerDevice<aqc::DevScratch> dres_tab;
  aqc::DevScratch& dres = dres_tab.here();
  hipStream_t st = aqc::mps_stream();
  const size_t need = (size_t)ns * n;
  if (dres.cap < need * sizeof(cplx)) AQC_HIP_CHECK(hipStreamSynchronize(st));
  rc = dres.ensure(need * sizeof(cplx));
  if (rc != AQC_OK) return rc;
  StagingLease lease(st);  // (after the sort, which takes one itself)
  if (lease.rc() != AQC_OK) return lease.rc();
  const size_t jb = ns * sizeof(MeasJob);
  rc = lease.ensure(jb);
  if (rc != AQC_OK) return rc;
  MeasJob* hjobs = (MeasJob*)lease.buf().host;
  for (int s = 0; s < ns; ++s) hjobs[s] = make_meas(hs[s], (cplx*)dres.dev + (size_t)s * n);
  const MeasJob* dj = (const MeasJob*)lease.buf().dev;
  if (int e = aqc::upload_async(lease.buf().dev, hjobs, jb, st)) return e;
  int vc = 1;
  for (int s = 0; s < ns; ++s) vc = std::max(vc, hs[s]->d.cap);
  hipLaunchKernelGGL(k_zero_chains, dim3(ns, 2), dim3(kT), 2 * vc * sizeof(cplx), st, dj, vc);
  AQC_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_hw1, dim3(n, ns), dim3(kT), 0, st, dj);
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipMemcpyAsync(out, dres.dev, need * sizeof(cplx), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  return AQC_OK;
}

/* <psi|0..0> (out_ov, 2 doubles per state, as aqc_mps_overlap_zero_batch) and, when out_amps is
   not null, the amplitudes <e_i|psi> (2 n doubles per state, as aqc_mps_amps_hw1_batch) of every
   state (sorted first): a state copied from `base` while base has not changed since contracts only
   the sites it rewrote against rows cached on base; any other state (or a window too wide for the
   LDS) takes the full chains. */
int aqc_mps_zero_hw1_batch(aqc_mps_t base, aqc_mps_t* hs, int ns, double* out_ov, double* out_amps) {
  AQC_REQUIRE(base && hs && ns >= 0 && (out_ov || ns == 0), "aqc_mps_zero_hw1_batch: bad arguments");
  if (ns == 0) return AQC_OK;
  const int n = base->d.n, cap = base->d.cap;
  for (int s = 0; s < ns; ++s)
    AQC_REQUIRE(hs[s] && hs[s] != base && hs[s]->d.n == n && hs[s]->d.cap == cap,
                "aqc_mps_zero_hw1_batch: every state needs base's n and capacity (and is not base)");
  int rc = aqc_mps_sort_batch(hs, ns);
  if (rc != AQC_OK) return rc;
  std::vector<int> win, lo(ns), hi(ns), fb;
  int need_l = 0, need_r = n;
  for (int s = 0; s < ns; ++s) {
    const aqc_mps_s* h = hs[s];
    const bool ok = h->synced_src == base->uid && h->synced_ver == base->version;
    lo[s] = h->dirty_hi >= h->dirty_lo ? h->dirty_lo : 0;
    hi[s] = h->dirty_hi >= h->dirty_lo ? h->dirty_hi : 0;
    if (!ok) {
      fb.push_back(s);
      continue;
    }
    need_l = std::max(need_l, lo[s]);
    need_r = std::min(need_r, hi[s] + 1);
    win.push_back(s);
  }
  hipStream_t st = aqc::mps_stream();
  const size_t blk = (size_t)(n + 1) * cap;
  if (!win.empty()) {
    if (!base->hwenv) {
      base->hwenv = (cplx*)aqc::dev_alloc(2 * (size_t)(n + 1) * blk * sizeof(cplx));
      AQC_REQUIRE(base->hwenv, "aqc_mps_zero_hw1_batch: out of device memory");
      AQC_HIP_CHECK(hipMemsetAsync(base->hwenv, 0, 2 * (size_t)(n + 1) * blk * sizeof(cplx), st));
      const double one = 1.0;
      AQC_HIP_CHECK(hipMemcpyAsync(base->hwenv, &one, sizeof(double), hipMemcpyHostToDevice, st));
      AQC_HIP_CHECK(hipMemcpyAsync(base->hwenv + (size_t)(n + 1) * blk + (size_t)n * blk, &one, sizeof(double),
                                   hipMemcpyHostToDevice, st));
      AQC_HIP_CHECK(hipStreamSynchronize(st));  // (the host constant's copies)
      base->hl = base->h0l = 0;
      base->hr = base->h0r = n;
    }
    cplx* HL = base->hwenv;
    cplx* HR = base->hwenv + (size_t)(n + 1) * blk;
    std::vector<HwRowsJob> rj;
    const int full = out_amps ? 1 : 0;
    auto rows_job = [&](int dir, int first, int nsteps, cplx* rows) {
      rj.push_back(HwRowsJob{base->d.gam, base->d.lam, base->d.dims, n, cap, dir, first, nsteps, full, rows});
    };
    // (the amplitudes need every row; the overlap alone row 0)
    const int hl = full ? base->hl : base->h0l, hr = full ? base->hr : base->h0r;
    if (need_l > hl) rows_job(0, hl, need_l - hl, HL);
    if (need_r < hr) rows_job(1, hr - 1, hr - need_r, HR);
    std::vector<HwWinJob> wj;
    const size_t jb = aqc::up256(rj.size() * sizeof(HwRowsJob));
    const size_t wb = aqc::up256(win.size() * sizeof(HwWinJob));
    const size_t rb = aqc::up256((size_t)win.size() * (n + 1) * sizeof(cplx));
    const size_t fnb = (size_t)win.size() * 2 * cap * sizeof(cplx);  // the chains' last vectors
    const size_t cb = aqc::up256(win.size() * sizeof(int));  // hand-off counters
    size_t uyb = 0;  // with amps: each state's window vectors (2 (w + 1) cap)
    if (out_amps)
      for (int s : win) uyb += 2 * (size_t)(hi[s] - lo[s] + 2) * cap * sizeof(cplx);
    // the states' and base's error flags are gathered beside the results (one read-back: the
    // caller needs no separate aqc_mps_check_batch round trip)
    const size_t flb = aqc::up256(((size_t)ns + 1) * sizeof(int));
    char* d = (char*)aqc::dev_alloc(rb + flb + fnb + uyb + 256);
    AQC_REQUIRE(d, "aqc_mps_zero_hw1_batch: out of device memory");
    cplx* res = (cplx*)d;
    int* dflags = (int*)(d + rb);
    cplx* fin = (cplx*)(d + rb + flb);
    cplx* uy = (cplx*)(d + rb + flb + fnb);
    for (size_t k = 0; k < win.size(); ++k) {
      const int s = win[k];
      HwWinJob j;
      j.gam = hs[s]->d.gam;
      j.lam = hs[s]->d.lam;
      j.dims = hs[s]->d.dims;
      j.n = n;
      j.cap = cap;
      j.lo = lo[s];
      j.hi = hi[s];
      j.ml = HL + (size_t)lo[s] * blk;
      j.nr = HR + (size_t)(hi[s] + 1) * blk;
      j.ov = res + k * (n + 1);
      j.amps = out_amps ? res + k * (n + 1) + 1 : nullptr;
      j.uy = out_amps ? uy : nullptr;
      if (out_amps) uy += 2 * (size_t)(hi[s] - lo[s] + 2) * cap;
      j.fin = fin + k * 2 * (size_t)cap;
      j.cnt = nullptr;  // (set below: in the staging buffer)
      j.pad = 0;
      wj.push_back(j);
    }
    // (capacity <= 64: plus the right steps' 64 x 65 reduction tile)
    const size_t lds_win = (2 * (size_t)cap + 4 * 64 + (cap <= 64 ? 64 * 65 : 0)) * sizeof(cplx);
    const size_t lds_rows = (2 * (size_t)cap + 4 * kHwR * 64) * sizeof(cplx);
    // the job arrays through a pinned staging set of the ring (pageable copies were a host round
    // trip each, between the candidates' replay and these kernels)
    StagingLease lease(st);
    if (lease.rc() != AQC_OK) {
      aqc::dev_free(d);
      return lease.rc();
    }
    const size_t fpb = ((size_t)ns + 1) * sizeof(int*);
    rc = lease.ensure(jb + wb + cb + fpb);
    if (rc != AQC_OK) {
      aqc::dev_free(d);
      return rc;
    }
    char* hj = lease.buf().host;
    char* dj = lease.buf().dev;
    for (size_t k = 0; k < wj.size(); ++k) wj[k].cnt = (int*)(dj + jb + wb) + k;
    if (!rj.empty()) std::memcpy(hj, rj.data(), rj.size() * sizeof(HwRowsJob));
    std::memcpy(hj + jb, wj.data(), wj.size() * sizeof(HwWinJob));
    std::memset(hj + jb + wb, 0, cb);
    std::vector<aqc_mps_t> flagged(hs, hs + ns);  // (base's flag is the extra last entry)
    flagged.push_back(base);
    aqc::flag_ptrs(flagged.data(), ns + 1, (int**)(hj + jb + wb + cb));
    if (int e = aqc::upload_async(dj, hj, jb + wb + cb + fpb, st)) {
      aqc::dev_free(d);
      return e;
    }
    // (up to 98 KB at capacity 1024)
    if (int e = aqc::allow_dynamic_lds((const void*)k_hw_win, 128 * 1024)) return e;
    if (int e = aqc::allow_dynamic_lds((const void*)k_hw_rows, 128 * 1024)) return e;
    if (!rj.empty()) {
      hipLaunchKernelGGL(k_hw_rows, dim3((unsigned)rj.size(), full ? kHwRowsG : 1), dim3(kT), lds_rows, st,
                         (const HwRowsJob*)dj);
      AQC_CHECK_LAUNCH();
    }
    aqc::KernelTimer::begin(st, "mps_zero_hw1", 0.0, 0.0);
    hipLaunchKernelGGL(k_hw_win, dim3((unsigned)win.size(), 2), dim3(kT), lds_win, st, (const HwWinJob*)(dj + jb));
    aqc::KernelTimer::end(st);
    AQC_CHECK_LAUNCH();
    rc = aqc::queue_flag_gather((int* const*)(dj + jb + wb + cb), ns + 1, dflags, st);
    if (rc != AQC_OK) return rc;
    std::vector<cplx> h(rb / sizeof(cplx) + flb / sizeof(cplx));
    AQC_HIP_CHECK(hipMemcpyAsync(h.data(), res, rb + flb, hipMemcpyDeviceToHost, st));
    AQC_HIP_CHECK(hipStreamSynchronize(st));
    aqc::dev_free(d);
    rc = aqc::settle_flags(flagged.data(), ns + 1, (const int*)((const char*)h.data() + rb));
    if (rc != AQC_OK) return rc;
    base->h0l = std::max(base->h0l, need_l);
    base->h0r = std::min(base->h0r, need_r);
    if (full) {
      base->hl = std::max(hl, need_l);
      base->hr = std::min(hr, need_r);
    }
    for (size_t k = 0; k < win.size(); ++k) {
      const int s = win[k];
      const cplx* v = h.data() + k * (n + 1);
      out_ov[2 * s] = v[0].x;  // mps_dot(psi, zero) = conj(amplitude of |0..0>)
      out_ov[2 * s + 1] = -v[0].y;
      if (out_amps)
        for (int q = 0; q < n; ++q) {
          out_amps[((size_t)s * n + q) * 2] = v[1 + q].x;
          out_amps[((size_t)s * n + q) * 2 + 1] = v[1 + q].y;
        }
    }
  }
  if (!fb.empty()) {  // the full chains
    std::vector<aqc_mps_t> fh;
    for (int s : fb) fh.push_back(hs[s]);
    std::vector<double> o(2 * fb.size()), a(out_amps ? 2 * fb.size() * n : 0);
    rc = aqc_mps_overlap_zero_batch(fh.data(), (int)fh.size(), o.data());
    if (rc != AQC_OK) return rc;
    if (out_amps) {
      rc = aqc_mps_amps_hw1_batch(fh.data(), (int)fh.size(), a.data());
      if (rc != AQC_OK) return rc;
    }
    fh.push_back(base);  // (their error flags and base's, as on the window path)
    rc = aqc_mps_check_batch(fh.data(), (int)fh.size());
    if (rc != AQC_OK) return rc;
    for (size_t k = 0; k < fb.size(); ++k) {
      const int s = fb[k];
      out_ov[2 * s] = o[2 * k];
      out_ov[2 * s + 1] = o[2 * k + 1];
      if (out_amps) std::memcpy(out_amps + (size_t)s * 2 * n, a.data() + k * 2 * n, 2 * n * sizeof(double));
    }
  }
  return AQC_OK;
}

int aqc_mps_amps_hw1(aqc_mps_t h, double* out) {
  AQC_REQUIRE(h && out, "aqc_mps_amps_hw1: null argument");
  return aqc_mps_amps_hw1_batch(&h, 1, out);
}

static int ensure_env(aqc_mps_t h) {
  if (h->d.env) return AQC_OK;
  const size_t cap = h->d.cap;
  h->d.env = (cplx*)aqc::dev_alloc(2 * (size_t)(h->d.n + 1) * cap * cap * sizeof(cplx));
  if (!h->d.env) {
    aqc::set_error("aqc_mps: out of device memory (environments)");
    return AQC_ERR_NOMEM;
  }
  return AQC_OK;
}

int aqc_mps_dot(aqc_mps_t a, aqc_mps_t b, double* re, double* im) {
  AQC_REQUIRE(a && b && re && im && a->d.n == b->d.n, "aqc_mps_dot: bad arguments");
  int rc = aqc_mps_sort(a);
  if (rc != AQC_OK) return rc;
  rc = aqc_mps_sort(b);
  if (rc != AQC_OK) return rc;
  rc = ensure_env(a);
  if (rc != AQC_OK) return rc;
  AQC_REQUIRE(a->d.cap == b->d.cap, "aqc_mps_dot: both MPS must share chi_cap");
  EnvJob j;
  std::memset(&j, 0, sizeof(j));
  j.ga = a->d.gam;
  j.la = a->d.lam;
  j.da = a->d.dims;
  j.gb = b->d.gam;
  j.lb = b->d.lam;
  j.db = b->d.dims;
  j.n = a->d.n;
  j.cap = a->d.cap;
  j.env = a->d.env;
  j.tmp = a->d.tmp;
  j.keep_all = 0;
  j.right = 0;
  j.out = a->d.scal;
  hipStream_t st = aqc::mps_stream();
  StagingLease lease(st);  // (after the sorts, which take one themselves)
  if (lease.rc() != AQC_OK) return lease.rc();
  rc = lease.ensure(sizeof(EnvJob));
  if (rc != AQC_OK) return rc;
  std::memcpy(lease.buf().host, &j, sizeof(EnvJob));
  if (int e = aqc::upload_async(lease.buf().dev, lease.buf().host, sizeof(EnvJob), st)) return e;
  hipLaunchKernelGGL(k_env, dim3(1), dim3(kT), 0, st, (const EnvJob*)lease.buf().dev);
  AQC_CHECK_LAUNCH();
  cplx v;
  AQC_HIP_CHECK(hipMemcpyAsync(&v, a->d.scal, sizeof(cplx), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  *re = v.x;
  *im = v.y;
  return AQC_OK;
}

int aqc_mps_z_all(aqc_mps_t h, double* out) {
  AQC_REQUIRE(h && out, "aqc_mps_z_all: null argument");
  // the batched path (ent.hip: left / right environment chains over several workgroups on the
  // matrix cores, P_b per site, one trace each): O(n chi^3).  The per-site kernel used until round
  // 6 contracted L A R for each output entry, O(chi^4) per site -- 83 s for one 21-qubit state at
  // bond 512 (profiles/r6_zall_cap1024_kernel_stats.csv).
  return aqc_mps_z_all_batch(&h, 1, out);
}

}  // extern "C"
