// Shot sampling: measurement outcomes of every qubit drawn on the device, for the statevector and
// for the MPS.  Replaces the counts that the reference's QiskitSamplingBackend
// (adaptaqc/backends/qiskit_sampling_backend.py:78-89) obtains from Aer's qasm_simulator.
//
// Random numbers are counter based (sample_rng.h): a shot's outcome depends only on (seed, run,
// shot, site), not on the grid or the schedule.
//
// Statevector: inverse CDF.  With p_k = |psi_k|^2, total P and inclusive prefix sums C_k, a shot
// with uniform u takes the smallest k with C_k > u P.  The sums are hierarchical and fixed:
//   k_sv_tile_sums   S[t] of each tile of 4096 amplitudes: a wave per tile, lane l sums its 64
//                    contiguous p_k in order, then a wave prefix scan (S[t] = its last value)
//   k_sv_tile_scan   E[t] = E[t-1] + S[t-1] in order (one workgroup, carry), E[ntiles] = P
//   k_sv_shots       a wave per shot: binary search for the tile with E[t] <= u P < E[t+1], the
//                    same lane sums and scan of that tile, then the owning lane walks its 64.
// Where rounding leaves no k (u P >= P, or the residual past the tile's last prefix) the shot takes
// the last k with p_k > 0 (of the state, or of the tile).
//
// MPS (sorted qubits, A_i^s = Gamma_i^s lambda_{i+1}, no canonical form assumed): with the right
// environments R_i of ent.hip (R_n = 1) and v = [1], site by site
//   w_s = v A_i^s,  p_s = Re(w_s R_{i+1} w_s^dag),  bit = [u (p_0 + p_1) >= p_0],  v <- w_bit / sqrt(p_bit).
// k_mps_sample carries a tile of 64 shots through all n sites in one workgroup, as GEMMs on the
// FP64 matrix cores (aqc::block_cgemm): W = V [A^0 | A^1] (64 x 2 chi_r, contraction chi_l), then
// per s the product W_s R_{i+1}, whose store folds Re(Q o conj(W_s)) into a 64 x chi_r real tile
// that four threads per row sum in a fixed order.  No communication between workgroups.
#include <algorithm>
#include <cstring>
#include <vector>

#include "aqc_gemm.h"
#include "mps_internal.h"
#include "sample_rng.h"

using aqc::cplx;

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 4096;    // amplitudes per tile (the tiling of k_sv_zpartial)
constexpr int kPerLane = 64;   // contiguous amplitudes per lane of a tile's wave
constexpr int kShotTile = 64;  // shots per workgroup of the MPS sampler
constexpr int kMaxShots = 1 << 30;  // per call: shot and tile indices stay within int

// ---- uniforms ----------------------------------------------------------------------------------
__global__ void k_uniforms(uint64_t seed, uint64_t run, int nshots, int nper, double* __restrict__ out) {
  const size_t total = (size_t)nshots * nper;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x)
    out[e] = aqc::sample_uniform(seed, run, e / nper, (uint32_t)(e % nper));
}

// ---- statevector -------------------------------------------------------------------------------
__device__ __forceinline__ double amp_prob(const cplx* __restrict__ state, uint64_t dim, uint64_t x) {
  return x < dim ? aqc::cnorm2(aqc::ldg(state + x)) : 0.0;
}

// sum of the lane's 64 contiguous probabilities from `base`, in index order
__device__ __forceinline__ double lane_sum(const cplx* __restrict__ state, uint64_t dim, uint64_t base) {
  double s = 0.0;
  for (int j = 0; j < kPerLane; ++j) s += amp_prob(state, dim, base + j);
  return s;
}

// inclusive prefix sums over the wave's lanes (the same association in every caller)
__device__ __forceinline__ double wave_scan(double v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const double t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

__global__ __launch_bounds__(kThreads) void k_sv_tile_sums(const cplx* __restrict__ state, uint64_t dim,
                                                           uint64_t ntiles, double* __restrict__ S) {
  const int lane = threadIdx.x & 63;
  const uint64_t tile = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (tile >= ntiles) return;
  const double incl = wave_scan(lane_sum(state, dim, tile * kTile + (uint64_t)lane * kPerLane), lane);
  if (lane == 63) S[tile] = incl;
}

// E[t] = sum of S[0 .. t-1] in index order (E[t+1] = fl(E[t] + S[t]): monotone), E[ntiles] = P;
// meta[0] = the last tile with S > 0 (-1: none).  One workgroup; thread 0 carries the sum.
__global__ __launch_bounds__(kThreads) void k_sv_tile_scan(const double* __restrict__ S, uint64_t ntiles,
                                                           double* __restrict__ E, long long* __restrict__ meta) {
  __shared__ double buf[kTile];
  double carry = 0.0;
  long long last = -1;
  for (uint64_t c0 = 0; c0 < ntiles; c0 += kTile) {
    const int cnt = ntiles - c0 < (uint64_t)kTile ? (int)(ntiles - c0) : kTile;
    for (int i = threadIdx.x; i < cnt; i += kThreads) buf[i] = S[c0 + i];
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 0; i < cnt; ++i) {
        const double s = buf[i];
        buf[i] = carry;
        if (s > 0.0) last = (long long)(c0 + i);
        carry += s;
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += kThreads) E[c0 + i] = buf[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    E[ntiles] = carry;
    meta[0] = last;
  }
}

__global__ __launch_bounds__(kThreads) void k_sv_shots(const cplx* __restrict__ state, uint64_t dim, uint64_t ntiles,
                                                       const double* __restrict__ E, const long long* __restrict__ meta,
                                                       const double* __restrict__ u, uint64_t seed, uint64_t run,
                                                       int nshots, uint64_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int shot = (int)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (shot >= nshots) return;  // (a whole wave: the kernel has no barrier)
  const long long last = meta[0];
  if (last < 0) {  // the zero vector: nothing to draw from
    if (lane == 0) out[shot] = 0;
    return;
  }
  const double uu = u ? u[shot] : aqc::sample_uniform(seed, run, (uint64_t)shot, 0u);
  const double P = E[ntiles], target = uu * P;
  const bool past = !(target < P);  // rounding: the last outcome with p > 0
  uint64_t t = (uint64_t)last;
  if (!past) {
    uint64_t lo = 0, hi = ntiles;  // E[lo] <= target < E[hi]
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (E[mid] <= target) lo = mid;
      else hi = mid;
    }
    t = lo;
  }
  const double r = target - E[t];
  const uint64_t base = t * kTile + (uint64_t)lane * kPerLane;
  const double s = lane_sum(state, dim, base);
  const double incl = wave_scan(s, lane);
  double excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = 0.0;
  const unsigned long long hit = __ballot(!past && incl > r);
  int owner;
  bool walk = hit != 0ull;
  if (walk) {
    owner = __ffsll((long long)hit) - 1;
  } else {  // no prefix above the residual: the tile's last outcome with p > 0
    const unsigned long long nz = __ballot(s > 0.0);
    owner = nz ? 63 - __clzll((long long)nz) : 0;
  }
  if (lane == owner) {
    int idx = -1, lastnz = -1;
    double c = excl;
    for (int j = 0; j < kPerLane; ++j) {
      const double p = amp_prob(state, dim, base + j);
      if (p > 0.0) lastnz = j;
      if (walk && idx < 0) {
        c += p;
        if (c > r) idx = j;
      }
    }
    if (idx < 0) idx = lastnz < 0 ? 0 : lastnz;
    out[shot] = base + (uint64_t)idx;
  }
}

// ---- MPS ---------------------------------------------------------------------------------------
struct SampleJob {
  const cplx* gam;
  const double* lam;
  const int* dims;
  const cplx* Renv;  // (n+1) cap^2: R_b at b cap^2, row-major with row stride cap
  int n, cap;
  int nshots, words, ntiles;
  const double* u;  // null, or nshots x n
  uint64_t seed, run;
  uint64_t* out;  // nshots x words
  cplx* W;        // per workgroup 64 x 2 cap
  cplx* Vg;       // per workgroup 64 x cap   (global-workspace path)
  double* Tg;     // per workgroup 64 x cap   (global-workspace path)
};

// VLDS: V and the real tile T in the LDS (64 cap complex + 64 cap doubles of dynamic LDS beside the
// GEMM's staging tiles: capacity <= 64); else in the per-workgroup global workspace.  W (64 x 2 cap)
// is in the global workspace either way: at capacity 64 it alone is 128 KB of the CU's 160 KB.
template <bool VLDS>
__global__ __launch_bounds__(kThreads) void k_mps_sample(const SampleJob j) {
  __shared__ aqc::GemmLds lds;
  __shared__ double ps[2][kShotTile];
  __shared__ double scale[kShotTile];
  __shared__ int bits[kShotTile];
  extern __shared__ double2 smp_lds[];
  const int tid = threadIdx.x, row = tid >> 2, part = tid & 3;
  const int n = j.n, cap = j.cap;
  const size_t cc = (size_t)cap * cap;
  cplx* V = VLDS ? (cplx*)smp_lds : j.Vg + (size_t)blockIdx.x * kShotTile * cap;
  double* T = VLDS ? (double*)(smp_lds + (size_t)kShotTile * cap) : j.Tg + (size_t)blockIdx.x * kShotTile * cap;
  cplx* W = j.W + (size_t)blockIdx.x * kShotTile * 2 * cap;
  for (int tile = blockIdx.x; tile < j.ntiles; tile += gridDim.x) {
    const int shot = tile * kShotTile + row;
    const bool valid = shot < j.nshots;  // (rows past nshots carry zeros and write nothing)
    if (part == 0) V[(size_t)row * cap] = aqc::cmk(valid ? 1.0 : 0.0, 0.0);
    uint64_t word = 0;
    __syncthreads();
    for (int i = 0; i < n; ++i) {
      const int cl = j.dims[i], cr = j.dims[i + 1];
      const cplx* g = j.gam + (size_t)i * 2 * cc;
      const double* lam = j.lam + (size_t)(i + 1) * cap;
      const cplx* R = j.Renv + (size_t)(i + 1) * cc;
      // W[:, s cap + r] = sum_k V[:, k] A^s[k][r]
      aqc::block_cgemm<true, false, true>(
          kShotTile, 2 * cr, cl, [&](int r, int k) { return V[(size_t)r * cap + k]; },
          [&](int k, int c) {
            const int s = c >= cr ? 1 : 0, rr = c - s * cr;
            return aqc::cscale(aqc::ldg(g + (size_t)s * cc + (size_t)k * cap + rr), aqc::ldg(lam + rr));
          },
          [&](int r, int c, cplx v) { W[(size_t)r * 2 * cap + (c >= cr ? cap + c - cr : c)] = v; }, lds);
      __syncthreads();
      for (int s = 0; s < 2; ++s) {
        const cplx* Ws = W + (size_t)s * cap;
        // T = Re((W_s R) o conj(W_s)); p_s[row] = its row sum
        aqc::block_cgemm<true, false, true>(
            kShotTile, cr, cr, [&](int r, int k) { return Ws[(size_t)r * 2 * cap + k]; },
            [&](int k, int c) { return aqc::ldg(R + (size_t)k * cap + c); },
            [&](int r, int c, cplx v) {
              const cplx w = Ws[(size_t)r * 2 * cap + c];
              T[(size_t)r * cap + c] = fma(v.x, w.x, v.y * w.y);
            },
            lds);
        __syncthreads();
        double acc = 0.0;
        for (int c = part; c < cr; c += 4) acc += T[(size_t)row * cap + c];
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        if (part == 0) ps[s][row] = acc;
        __syncthreads();
      }
      if (part == 0) {
        const double p0 = ps[0][row], p1 = ps[1][row], tot = p0 + p1;
        double uu = 0.0;
        if (valid) uu = j.u ? j.u[(size_t)shot * n + i] : aqc::sample_uniform(j.seed, j.run, (uint64_t)shot, (uint32_t)i);
        const int bit = uu * tot >= p0 ? 1 : 0;
        const double pb = bit ? p1 : p0;
        scale[row] = (valid && pb > 0.0) ? 1.0 / sqrt(pb) : 0.0;
        bits[row] = bit;
        if (bit) word |= 1ull << (i & 63);
        if ((i & 63) == 63 || i == n - 1) {
          if (valid) j.out[(size_t)shot * j.words + (i >> 6)] = word;
          word = 0;
        }
      }
      __syncthreads();
      {
        const cplx* Wb = W + (size_t)row * 2 * cap + (size_t)bits[row] * cap;
        const double sc = scale[row];
        for (int c = part; c < cr; c += 4) V[(size_t)row * cap + c] = aqc::cscale(Wb[c], sc);
      }
      __syncthreads();
    }
  }
}

// per-device grow-only scratch of the statevector sampler and aqc_sample_uniforms
aqc::PerDevice<aqc::DevScratch> g_scr;
using aqc::up256;

int check_uniforms(const double* u, size_t count, const char* who) {
  for (size_t e = 0; e < count; ++e)
    if (!(u[e] >= 0.0 && u[e] < 1.0)) {
      aqc::set_error(std::string(who) + ": u must lie in [0, 1)");
      return AQC_ERR_ARG;
    }
  return AQC_OK;
}

}  // namespace

extern "C" {

int aqc_sample_uniforms(uint64_t seed, uint64_t run, int nshots, int nper, double* out) {
  AQC_REQUIRE(out && nshots >= 1 && nper >= 1, "aqc_sample_uniforms: bad arguments");
  const size_t total = (size_t)nshots * nper;
  AQC_HIP_CHECK(hipDeviceSynchronize());  // (the scratch may be regrown)
  aqc::DevScratch& sc = g_scr.here();
  if (int rc = sc.ensure(total * sizeof(double))) return rc;
  char* buf = sc.dev;
  const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(k_uniforms, dim3(grid), dim3(256), 0, 0, seed, run, nshots, nper, (double*)buf);
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipMemcpy(out, buf, total * sizeof(double), hipMemcpyDeviceToHost));
  return AQC_OK;
}

int aqc_sv_sample(aqc_sv_t h, int nshots, uint64_t seed, uint64_t run, const double* u, uint64_t* out) {
  AQC_REQUIRE(h && out, "aqc_sv_sample: null argument");
  AQC_REQUIRE(nshots >= 1 && nshots <= kMaxShots, "aqc_sv_sample: nshots must be in 1 .. 2^30");
  if (u)
    if (int rc = check_uniforms(u, (size_t)nshots, "aqc_sv_sample")) return rc;
  const cplx* state = nullptr;
  int n = 0;
  hipStream_t st = nullptr;
  if (int rc = aqc::sv_view(h, &state, &n, &st)) return rc;
  const uint64_t dim = 1ull << n, ntiles = (dim + kTile - 1) / kTile;
  const size_t sb = up256(ntiles * sizeof(double)), eb = up256((ntiles + 1) * sizeof(double)), mb = 256;
  const size_t ub = up256((size_t)nshots * sizeof(double)), ob = up256((size_t)nshots * sizeof(uint64_t));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  aqc::DevScratch& sc = g_scr.here();
  if (int rc = sc.ensure(sb + eb + mb + ub + ob)) return rc;
  char* buf = sc.dev;
  double* S = (double*)buf;
  double* E = (double*)(buf + sb);
  long long* meta = (long long*)(buf + sb + eb);
  double* du = (double*)(buf + sb + eb + mb);
  uint64_t* dout = (uint64_t*)(buf + sb + eb + mb + ub);
  if (u) AQC_HIP_CHECK(hipMemcpyAsync(du, u, (size_t)nshots * sizeof(double), hipMemcpyHostToDevice, st));
  const int wpb = kThreads / 64;
  aqc::KernelTimer::begin(st, "sv_sample", 16.0 * (double)dim + (double)nshots * kTile * 16.0, 0.0);
  hipLaunchKernelGGL(k_sv_tile_sums, dim3((unsigned)((ntiles + wpb - 1) / wpb)), dim3(kThreads), 0, st, state, dim, ntiles,
                     S);
  AQC_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_sv_tile_scan, dim3(1), dim3(kThreads), 0, st, (const double*)S, ntiles, E, meta);
  AQC_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_sv_shots, dim3((unsigned)((nshots + wpb - 1) / wpb)), dim3(kThreads), 0, st, state, dim, ntiles,
                     (const double*)E, (const long long*)meta, u ? (const double*)du : nullptr, seed, run, nshots, dout);
  aqc::KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipMemcpyAsync(out, dout, (size_t)nshots * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  return AQC_OK;
}

int aqc_mps_sample(aqc_mps_t h, int nshots, uint64_t seed, uint64_t run, const double* u, uint64_t* out) {
  AQC_REQUIRE(h && out, "aqc_mps_sample: null argument");
  AQC_REQUIRE(nshots >= 1 && nshots <= kMaxShots, "aqc_mps_sample: nshots must be in 1 .. 2^30");
  const int n = h->d.n, cap = h->d.cap;
  if (u)
    if (int rc = check_uniforms(u, (size_t)nshots * n, "aqc_mps_sample")) return rc;
  int rc = aqc_mps_sort(h);  // qubits back in site order, as measurements do
  if (rc != AQC_OK) return rc;
  rc = aqc_mps_check_batch(&h, 1);  // pending capacity / SVD flags of queued work: AQC_ERR_STATE
  if (rc != AQC_OK) return rc;
  const int words = (n + 63) / 64, ntiles = (nshots + kShotTile - 1) / kShotTile;
  const bool vlds = cap <= 64;
  const size_t wb = up256((size_t)kShotTile * 2 * cap * sizeof(cplx));
  const size_t vb = vlds ? 0 : up256((size_t)kShotTile * cap * sizeof(cplx));
  const size_t tb = vlds ? 0 : up256((size_t)kShotTile * cap * sizeof(double));
  // workgroups: one per tile up to 256, within 512 MB of workspace (a workgroup loops over tiles)
  const size_t per_wg = wb + vb + tb;
  const int nwg = (int)std::max<size_t>(1, std::min<size_t>({(size_t)ntiles, (size_t)256, ((size_t)512 << 20) / per_wg}));
  const size_t ub = u ? up256((size_t)nshots * n * sizeof(double)) : 0;
  const size_t ob = up256((size_t)nshots * words * sizeof(uint64_t));
  const cplx* renv = nullptr;
  void* extra = nullptr;
  hipStream_t st = nullptr;
  rc = aqc::mps_right_envs(h, ub + ob + (size_t)nwg * per_wg, &renv, &extra, &st);
  if (rc != AQC_OK) return rc;
  char* base = (char*)extra;
  SampleJob j;
  std::memset(&j, 0, sizeof(j));
  j.gam = h->d.gam;
  j.lam = h->d.lam;
  j.dims = h->d.dims;
  j.Renv = renv;
  j.n = n;
  j.cap = cap;
  j.nshots = nshots;
  j.words = words;
  j.ntiles = ntiles;
  j.u = u ? (const double*)base : nullptr;
  j.seed = seed;
  j.run = run;
  j.out = (uint64_t*)(base + ub);
  j.W = (cplx*)(base + ub + ob);
  j.Vg = vlds ? nullptr : (cplx*)(base + ub + ob + (size_t)nwg * wb);
  j.Tg = vlds ? nullptr : (double*)(base + ub + ob + (size_t)nwg * (wb + vb));
  if (u) AQC_HIP_CHECK(hipMemcpyAsync(base, u, (size_t)nshots * n * sizeof(double), hipMemcpyHostToDevice, st));
  const double c2 = (double)cap * cap;
  aqc::KernelTimer::begin(st, "mps_sample", 0.0, (double)nshots * n * 8.0 * 4.0 * c2);
  if (vlds) {
    const size_t dyn = (size_t)kShotTile * cap * (sizeof(cplx) + sizeof(double));
    if (int e = aqc::allow_dynamic_lds((const void*)k_mps_sample<true>, 96 * 1024)) return e;
    hipLaunchKernelGGL(k_mps_sample<true>, dim3(nwg), dim3(kThreads), dyn, st, j);
  } else {
    hipLaunchKernelGGL(k_mps_sample<false>, dim3(nwg), dim3(kThreads), 0, st, j);
  }
  aqc::KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipMemcpyAsync(out, j.out, (size_t)nshots * words * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  return AQC_OK;
}

}  // extern "C"
