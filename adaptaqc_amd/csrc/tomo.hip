// Shot-based pair tomography: the counts, the fit and the observable concurrence bound of every
// coupling-map pair from the pairs' reduced density matrices.  Replaces the per-pair circuits of
// adaptaqc/utils/entanglement_measures.py:101-135 (perform_quantum_tomography: nine rotated copies
// of the circuit per pair through qiskit-experiments' StateTomography) and :138-250
// (measure_concurrence_lower_bound: three two-copy circuits per pair).
//
// Each of those circuits measures two qubits (or two copies of them), so its counts are a
// multinomial draw from probabilities that the pair's 4x4 RDM fixes.  The state is simulated once,
// the RDMs of all pairs come from aqc_sv_pair_rdms / aqc_mps_pair_rdms, and then
//   k_tomo_probs    36 probabilities per pair: setting s = 3 b_hi + b_lo (basis 0 X, 1 Y, 2 Z),
//                   outcome o = 2 o_hi + o_lo (0: the +1 eigenstate), p = max(0, <v|rho|v>)
//   k_bound_probs   3 per pair: P("1111"), P("0011"), P("1100") of the two-copy circuits
//   k_multinomial   counts of nshots draws per job (a job: K probabilities).  A workgroup per
//                   (job, chunk of shots): threads stride over the chunk's shots with the counters in
//                   registers, a shot's uniform is sample_uniform(seed, run, shot, job)
//                   (sample_rng.h), its outcome the smallest k with C_k > u P (C: in-order inclusive
//                   sums, P = C_{K-1}; where rounding leaves none, the last k with p_k > 0: the
//                   statevector sampler's rule).  Lane sums by shuffles, the waves' through the LDS,
//                   chunk partials (more than one chunk only) by k_sum_chunks.  Integer sums: the
//                   counts do not depend on the launch shape; no atomics.
//   k_tomo_fit      per pair: frequencies per setting, linear inversion rho = 1/4 sum T[P][Q] P (x) Q,
//                   then the positive-semidefinite rescaling of Smolin, Gambetta and Smith
//                   (PRL 108, 070502) on the eigenvalues (herm4_eig), and division by the trace.
// RDM index: 2 bit_hi + bit_lo, hi = the pair's larger qubit (as the pair-RDM entry points return).
#include <algorithm>
#include <cstring>
#include <vector>

#include "herm4.h"
#include "mps_internal.h"
#include "sample_rng.h"

using aqc::cplx;

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 65536;       // shots per workgroup of k_multinomial
constexpr int kMaxShots = 1 << 30;  // per call, as the samplers
constexpr int kMaxK = 16;

// the +1 / -1 eigenvector (o = 0 / 1) of basis b (0 X, 1 Y, 2 Z)
__device__ __forceinline__ void eigvec(int b, int o, cplx v[2]) {
  const double r = 0.70710678118654752440;
  if (b == 2) {
    v[0] = aqc::cmk(o == 0 ? 1.0 : 0.0, 0.0);
    v[1] = aqc::cmk(o == 0 ? 0.0 : 1.0, 0.0);
  } else {
    const double sg = o == 0 ? r : -r;
    v[0] = aqc::cmk(r, 0.0);
    v[1] = b == 0 ? aqc::cmk(sg, 0.0) : aqc::cmk(0.0, sg);
  }
}

// a thread per (pair, setting): out[(pair 9 + s) 4 + o]
__global__ void k_tomo_probs(const cplx* __restrict__ rdms, int npairs, double* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= npairs * 9) return;
  const int p = e / 9, s = e % 9, bh = s / 3, bl = s % 3;
  cplx rho[4][4];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) rho[r][c] = rdms[(size_t)p * 16 + r * 4 + c];
  for (int o = 0; o < 4; ++o) {
    cplx vh[2], vl[2], v[4];
    eigvec(bh, o >> 1, vh);
    eigvec(bl, o & 1, vl);
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b) v[2 * a + b] = aqc::cmul(vh[a], vl[b]);
    double acc = 0.0;
    for (int r = 0; r < 4; ++r) {
      cplx w = aqc::cmk(0, 0);  // (rho v)_r
      for (int c = 0; c < 4; ++c) w = aqc::cfma(rho[r][c], v[c], w);
      acc += aqc::cconjmul(v[r], w).x;
    }
    out[(size_t)e * 4 + o] = fmax(0.0, acc);
  }
}

// a thread per pair: (P("1111"), P("0011"), P("1100")); rho_1 = the marginal of the lower qubit
__global__ void k_bound_probs(const cplx* __restrict__ rdms, int npairs, double* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npairs) return;
  cplx rho[4][4];
  double t12 = 0.0;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      rho[r][c] = rdms[(size_t)p * 16 + r * 4 + c];
      t12 += aqc::cnorm2(rho[r][c]);
    }
  double t1 = 0.0, t2 = 0.0;
  for (int x = 0; x < 2; ++x)
    for (int y = 0; y < 2; ++y) {
      t1 += aqc::cnorm2(aqc::cadd(rho[x][y], rho[2 + x][2 + y]));                  // lower qubit
      t2 += aqc::cnorm2(aqc::cadd(rho[2 * x][2 * y], rho[2 * x + 1][2 * y + 1]));  // higher qubit
    }
  out[(size_t)p * 3 + 0] = fmax(0.0, (1.0 - t1 - t2 + t12) / 4.0);
  out[(size_t)p * 3 + 1] = fmax(0.0, (1.0 - t1) / 2.0);
  out[(size_t)p * 3 + 2] = fmax(0.0, (1.0 - t2) / 2.0);
}

// grid (jobs, chunks), kThreads threads; KP: K rounded up to 2, 4, 8 or 16 (the padding has p = 0,
// which no shot can take).  out: counts (one chunk) or the chunk partials [chunk][job][K].
template <int KP>
__global__ __launch_bounds__(kThreads) void k_multinomial(const double* __restrict__ probs, int njobs, int K, int nshots,
                                                          uint64_t seed, uint64_t run, const double* __restrict__ u,
                                                          long long* __restrict__ out, int* __restrict__ err) {
  __shared__ unsigned red[kThreads / 64][KP];
  const int job = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x;
  double C[KP];
  double acc = 0.0;
  int lastnz = -1;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const double p = k < K ? probs[(size_t)job * K + k] : 0.0;
    if (!(p >= 0.0)) bad = true;
    if (p > 0.0) lastnz = k;
    acc += p;  // (sequential adds: the order of the restatement)
    C[k] = acc;
  }
  const double P = C[KP - 1];
  if (bad || !(P > 0.0) || !(P < 1e300)) {  // (the whole workgroup: before any barrier)
    if (tid == 0) *err = 1;
    return;
  }
  unsigned cnt[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) cnt[k] = 0u;
  const int t0 = ch * kChunk, t1 = min(nshots, t0 + kChunk);
  for (int t = t0 + tid; t < t1; t += kThreads) {
    const double uu = u ? u[(size_t)t * njobs + job] : aqc::sample_uniform(seed, run, (uint64_t)t, (uint32_t)job);
    const double target = uu * P;
    int k = 0;  // C is non-decreasing: the number of C_j <= target is the smallest k with C_k > target
#pragma unroll
    for (int j = 0; j < KP; ++j) k += C[j] <= target ? 1 : 0;
    if (k >= KP) k = lastnz;
#pragma unroll
    for (int j = 0; j < KP; ++j) cnt[j] += k == j ? 1u : 0u;
  }
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    unsigned v = cnt[k];
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    if ((tid & 63) == 0) red[tid >> 6][k] = v;
  }
  __syncthreads();
  if (tid < K) {
    long long s = 0;
    for (int w = 0; w < kThreads / 64; ++w) s += (long long)red[w][tid];
    out[((size_t)ch * njobs + job) * K + tid] = s;
  }
}

__global__ void k_sum_chunks(const long long* __restrict__ partial, size_t total, int nchunks,
                             long long* __restrict__ counts) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    long long s = 0;
    for (int c = 0; c < nchunks; ++c) s += partial[(size_t)c * total + e];
    counts[e] = s;
  }
}

// Pauli matrix P (0 I, 1 X, 2 Y, 3 Z), entry [r][c]
__device__ __forceinline__ cplx pauli_entry(int P, int r, int c) {
  switch (P) {
    case 0: return aqc::cmk(r == c ? 1.0 : 0.0, 0.0);
    case 1: return aqc::cmk(r != c ? 1.0 : 0.0, 0.0);
    case 2: return r == c ? aqc::cmk(0.0, 0.0) : aqc::cmk(0.0, r == 0 ? -1.0 : 1.0);
    default: return aqc::cmk(r != c ? 0.0 : (r == 0 ? 1.0 : -1.0), 0.0);
  }
}

// a thread per pair: counts[pair][9][4] -> the fitted 4x4 density matrix
__global__ void k_tomo_fit(const long long* __restrict__ counts, int npairs, cplx* __restrict__ out,
                           int* __restrict__ err) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npairs) return;
  double T[4][4];  // [hi letter][lo letter], 0 I, 1 X, 2 Y, 3 Z
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) T[a][b] = 0.0;
  T[0][0] = 1.0;
  for (int s = 0; s < 9; ++s) {
    const long long* c = counts + ((size_t)p * 9 + s) * 4;
    const long long tot = c[0] + c[1] + c[2] + c[3];
    if (tot <= 0 || c[0] < 0 || c[1] < 0 || c[2] < 0 || c[3] < 0) {
      *err = 1;
      return;
    }
    const double g0 = (double)c[0] / (double)tot, g1 = (double)c[1] / (double)tot;
    const double g2 = (double)c[2] / (double)tot, g3 = (double)c[3] / (double)tot;
    const int a = s / 3 + 1, b = s % 3 + 1;
    T[a][b] = ((g0 - g1) - g2) + g3;
    T[a][0] += (((g0 + g1) - g2) - g3) / 3.0;
    T[0][b] += (((g0 - g1) + g2) - g3) / 3.0;
  }
  cplx H[4][4], V[4][4];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      cplx acc = aqc::cmk(0, 0);
      for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) {
          const cplx m = aqc::cmul(pauli_entry(a, r >> 1, c >> 1), pauli_entry(b, r & 1, c & 1));
          acc = aqc::cadd(acc, aqc::cscale(m, 0.25 * T[a][b]));
        }
      H[r][c] = acc;
    }
  double mu[4];
  aqc::herm4_eig(H, mu, V, true);
  int idx[4] = {0, 1, 2, 3};  // eigenvalues in descending order
  for (int x = 0; x < 4; ++x)
    for (int z = x + 1; z < 4; ++z)
      if (mu[idx[z]] > mu[idx[x]]) {
        const int t = idx[x];
        idx[x] = idx[z];
        idx[z] = t;
      }
  double a = 0.0;
  int i = 4;
  while (i > 0 && mu[idx[i - 1]] + a / i < 0.0) {
    a += mu[idx[i - 1]];
    mu[idx[i - 1]] = 0.0;
    --i;
  }
  double tr = 0.0;
  for (int j = 0; j < i; ++j) {
    mu[idx[j]] += a / i;
    tr += mu[idx[j]];
  }
  if (!(tr > 0.0)) {
    *err = 1;
    return;
  }
  for (int r = 0; r < 4; ++r)
    for (int c = r; c < 4; ++c) {
      cplx acc = aqc::cmk(0, 0);
      for (int k = 0; k < 4; ++k) acc = aqc::cfma(aqc::cscale(V[r][k], mu[k] / tr), aqc::cconj(V[c][k]), acc);
      if (r == c) acc.y = 0.0;
      out[(size_t)p * 16 + r * 4 + c] = acc;
      if (r != c) out[(size_t)p * 16 + c * 4 + r] = aqc::cconj(acc);
    }
}

// per-device grow-only scratch
aqc::PerDevice<aqc::DevScratch> g_scr;
using aqc::up256;

// does p address device memory?  (plain host memory is unknown to the runtime: an error on some
// versions, an unregistered type on others)
bool is_device_ptr(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice;
}

// rdms -> `per` doubles a pair by `kernel` (a thread per `items_per_pair` items a pair)
template <typename Launch>
int rdm_map(const double* rdms, int npairs, double* out, int on_device, int per, Launch launch) {
  hipStream_t st = aqc::mps_stream();
  const size_t rb = up256((size_t)npairs * 16 * sizeof(cplx)), ob = up256((size_t)npairs * per * sizeof(double));
  const cplx* drdm = (const cplx*)rdms;
  double* dout = out;
  if (!on_device) {
    AQC_HIP_CHECK(hipStreamSynchronize(st));
    aqc::DevScratch& sc = g_scr.here();
    if (int rc = sc.ensure(rb + ob)) return rc;
    char* buf = sc.dev;
    AQC_HIP_CHECK(hipMemcpyAsync(buf, rdms, (size_t)npairs * 16 * sizeof(cplx), hipMemcpyHostToDevice, st));
    drdm = (const cplx*)buf;
    dout = (double*)(buf + rb);
  }
  launch(drdm, dout, st);
  AQC_CHECK_LAUNCH();
  if (!on_device) AQC_HIP_CHECK(hipMemcpyAsync(out, dout, (size_t)npairs * per * sizeof(double), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  return AQC_OK;
}

}  // namespace

extern "C" {

int aqc_pair_tomo_probs(const double* rdms, int npairs, double* out, int on_device) {
  AQC_REQUIRE(rdms && out && npairs >= 0 && npairs <= (1 << 24), "aqc_pair_tomo_probs: bad arguments");
  if (npairs == 0) return AQC_OK;
  return rdm_map(rdms, npairs, out, on_device, 36, [&](const cplx* r, double* o, hipStream_t st) {
    hipLaunchKernelGGL(k_tomo_probs, dim3((npairs * 9 + 255) / 256), dim3(256), 0, st, r, npairs, o);
  });
}

int aqc_concurrence_bound_probs(const double* rdms, int npairs, double* out, int on_device) {
  AQC_REQUIRE(rdms && out && npairs >= 0 && npairs <= (1 << 24), "aqc_concurrence_bound_probs: bad arguments");
  if (npairs == 0) return AQC_OK;
  return rdm_map(rdms, npairs, out, on_device, 3, [&](const cplx* r, double* o, hipStream_t st) {
    hipLaunchKernelGGL(k_bound_probs, dim3((npairs + 63) / 64), dim3(64), 0, st, r, npairs, o);
  });
}

int aqc_multinomial_counts(const double* probs, int njobs, int K, int nshots, uint64_t seed, uint64_t run,
                           const double* u, int64_t* counts) {
  AQC_REQUIRE(probs && counts && njobs >= 1, "aqc_multinomial_counts: bad arguments");
  AQC_REQUIRE(K >= 2 && K <= kMaxK, "aqc_multinomial_counts: K must be in 2 .. 16");
  AQC_REQUIRE(nshots >= 1 && nshots <= kMaxShots, "aqc_multinomial_counts: nshots must be in 1 .. 2^30");
  AQC_REQUIRE((size_t)njobs * K <= (size_t)1 << 28, "aqc_multinomial_counts: more than 2^28 probabilities");
  const bool pdev = is_device_ptr(probs), cdev = is_device_ptr(counts), udev = u && is_device_ptr(u);
  const size_t total = (size_t)njobs * K;
  const int nchunks = (nshots + kChunk - 1) / kChunk;
  if (u && !udev) {
    for (size_t e = 0; e < (size_t)nshots * njobs; ++e)
      AQC_REQUIRE(u[e] >= 0.0 && u[e] < 1.0, "aqc_multinomial_counts: u must lie in [0, 1)");
  }
  const size_t eb = 256, pb = pdev ? 0 : up256(total * sizeof(double)), cb = cdev ? 0 : up256(total * sizeof(long long));
  const size_t ub = (u && !udev) ? up256((size_t)nshots * njobs * sizeof(double)) : 0;
  const size_t qb = nchunks > 1 ? up256((size_t)nchunks * total * sizeof(long long)) : 0;
  hipStream_t st = aqc::mps_stream();
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  aqc::DevScratch& sc = g_scr.here();
  if (int rc = sc.ensure(eb + pb + cb + ub + qb)) return rc;
  char* buf = sc.dev;
  int* derr = (int*)buf;
  const double* dprobs = pdev ? probs : (const double*)(buf + eb);
  long long* dcounts = cdev ? (long long*)counts : (long long*)(buf + eb + pb);
  const double* du = !u ? nullptr : udev ? u : (const double*)(buf + eb + pb + cb);
  long long* partial = nchunks > 1 ? (long long*)(buf + eb + pb + cb + ub) : dcounts;
  AQC_HIP_CHECK(hipMemsetAsync(derr, 0, sizeof(int), st));
  if (!pdev) AQC_HIP_CHECK(hipMemcpyAsync(buf + eb, probs, total * sizeof(double), hipMemcpyHostToDevice, st));
  if (u && !udev)
    AQC_HIP_CHECK(hipMemcpyAsync(buf + eb + pb + cb, u, (size_t)nshots * njobs * sizeof(double), hipMemcpyHostToDevice, st));
  const dim3 grid((unsigned)njobs, (unsigned)nchunks);
  aqc::KernelTimer::begin(st, "multinomial", (double)total * 16.0, 0.0);
  if (K <= 2)
    hipLaunchKernelGGL(k_multinomial<2>, grid, dim3(kThreads), 0, st, dprobs, njobs, K, nshots, seed, run, du, partial, derr);
  else if (K <= 4)
    hipLaunchKernelGGL(k_multinomial<4>, grid, dim3(kThreads), 0, st, dprobs, njobs, K, nshots, seed, run, du, partial, derr);
  else if (K <= 8)
    hipLaunchKernelGGL(k_multinomial<8>, grid, dim3(kThreads), 0, st, dprobs, njobs, K, nshots, seed, run, du, partial, derr);
  else
    hipLaunchKernelGGL(k_multinomial<16>, grid, dim3(kThreads), 0, st, dprobs, njobs, K, nshots, seed, run, du, partial, derr);
  AQC_CHECK_LAUNCH();
  if (nchunks > 1) {
    const unsigned g = (unsigned)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(k_sum_chunks, dim3(g), dim3(256), 0, st, (const long long*)partial, total, nchunks, dcounts);
    AQC_CHECK_LAUNCH();
  }
  aqc::KernelTimer::end(st);
  int e = 0;
  AQC_HIP_CHECK(hipMemcpyAsync(&e, derr, sizeof(int), hipMemcpyDeviceToHost, st));
  if (!cdev) AQC_HIP_CHECK(hipMemcpyAsync(counts, dcounts, total * sizeof(long long), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  AQC_REQUIRE(e == 0, "aqc_multinomial_counts: a job's probabilities must be >= 0 with a positive finite sum");
  return AQC_OK;
}

int aqc_tomo_fit(const int64_t* counts, int npairs, double* out_rdms, int on_device) {
  AQC_REQUIRE(counts && out_rdms && npairs >= 0 && npairs <= (1 << 24), "aqc_tomo_fit: bad arguments");
  if (npairs == 0) return AQC_OK;
  hipStream_t st = aqc::mps_stream();
  const size_t eb = 256, cb = on_device ? 0 : up256((size_t)npairs * 36 * sizeof(long long));
  const size_t ob = on_device ? 0 : up256((size_t)npairs * 16 * sizeof(cplx));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  aqc::DevScratch& sc = g_scr.here();
  if (int rc = sc.ensure(eb + cb + ob)) return rc;
  char* buf = sc.dev;
  int* derr = (int*)buf;
  const long long* dcounts = on_device ? (const long long*)counts : (const long long*)(buf + eb);
  cplx* dout = on_device ? (cplx*)out_rdms : (cplx*)(buf + eb + cb);
  AQC_HIP_CHECK(hipMemsetAsync(derr, 0, sizeof(int), st));
  if (!on_device)
    AQC_HIP_CHECK(hipMemcpyAsync(buf + eb, counts, (size_t)npairs * 36 * sizeof(long long), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_tomo_fit, dim3((npairs + 63) / 64), dim3(64), 0, st, dcounts, npairs, dout, derr);
  AQC_CHECK_LAUNCH();
  int e = 0;
  AQC_HIP_CHECK(hipMemcpyAsync(&e, derr, sizeof(int), hipMemcpyDeviceToHost, st));
  if (!on_device) AQC_HIP_CHECK(hipMemcpyAsync(out_rdms, dout, (size_t)npairs * 16 * sizeof(cplx), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  AQC_REQUIRE(e == 0, "aqc_tomo_fit: every setting needs a positive total of non-negative counts");
  return AQC_OK;
}

}  // extern "C"
