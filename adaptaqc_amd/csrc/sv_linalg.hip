// Linear algebra on whole statevectors: y = sum_t c_t P_t psi, <a|b> and y <- a y + b x.  With these a
// Krylov method (utils/hamiltonians.py calculate_ground_state, the reference's hamiltonians.py:80-85
// on OpenFermion's sparse eigensolver) is a host loop over device vectors.
//
// Apply.  P = i^{popcount(x & z)} X^x Z^z as in pauli.hip, so (P psi)[j] = i^ny (-1)^{popcount((j^x) & z)}
// psi[j ^ x].  The host folds i^ny into the coefficient and groups the terms by x mask (groups in
// order of first appearance, terms of a group in input order): one thread owns one output amplitude
// j (grid stride), loads psi[j ^ X_g] once per group, sums the group's +-c'_t by the parity of
// (j ^ X_g) & z_t in term order, multiplies and accumulates in registers, and stores out[j] once.
// The tables are a stream of 16-byte words -- per group a header (X, term count) and two words a term
// (z; c') -- staged in LDS in chunks of kStageWords with vector loads and read as broadcasts.  The
// host cuts the stream at group headers; a group of more than kMaxGroupTerms terms is cut into
// several records of the same X (its amplitude is then loaded once per record).  One chunk (every
// Hamiltonian of a few hundred terms) is staged once per workgroup; several are restaged for every
// amplitude a thread owns.  64-bit indices, no atomics, no workgroup waits for another: the same
// inputs give the same bits.  Per call (records + 1) 16 2^n bytes: the reads of psi come from the
// L2 / MALL after the first while the state fits there.
//
// Dot.  conj(a_k) b_k summed by a thread in index order (grid stride), then the wave, the waves in
// order, and a second launch adds the workgroups' partials in order: k_sv_pauli's scheme.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "aqc_internal.h"

using aqc::cplx;
using aqc::up256;

namespace {

constexpr int kThreads = 256;
constexpr int kStageWords = 768;                         // 16-byte table words staged at a time (12 KB)
constexpr int kMaxGroupTerms = (kStageWords - 1) / 2;    // terms of one record (header + 2 words a term)
constexpr int kMaxApplyBlocks = 2048;                    // 8 workgroups a CU: every wave slot of the chip
constexpr int kMaxApplyTerms = 1 << 20;                  // stated limit of aqc_sv_pauli_apply
constexpr uint64_t kElemBlocks = (uint64_t)1 << 26;      // 2^34 amplitudes / 256: axpby's largest grid

// chunk c holds words chunk_off[c] .. chunk_off[c + 1] of `words`
template <bool kSingle>
__global__ __launch_bounds__(kThreads) void k_sv_pauli_apply(const cplx* __restrict__ in, cplx* __restrict__ out,
                                                             uint64_t dim, const ulonglong2* __restrict__ words,
                                                             const int* __restrict__ chunk_off, int nchunks) {
  __shared__ ulonglong2 stage[kStageWords];
  int nst = 0;
  if (kSingle) {
    nst = chunk_off[1];
    for (int w = threadIdx.x; w < nst; w += kThreads) stage[w] = words[w];
    __syncthreads();
  }
  // base is uniform over the workgroup, so every thread reaches the barriers of the staging
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads; base < dim; base += (uint64_t)gridDim.x * kThreads) {
    const uint64_t j = base + threadIdx.x;
    const bool mine = j < dim;
    cplx acc = aqc::cmk(0.0, 0.0);
    for (int c = 0; c < nchunks; ++c) {
      if (!kSingle) {
        const int off = chunk_off[c];
        nst = chunk_off[c + 1] - off;
        __syncthreads();  // the previous chunk has been read
        for (int w = threadIdx.x; w < nst; w += kThreads) stage[w] = words[(size_t)off + w];
        __syncthreads();
      }
      if (!mine) continue;
      for (int p = 0; p < nst;) {
        const ulonglong2 hd = stage[p];  // (X, term count): uniform
        const uint64_t k = j ^ hd.x;
        const int nt = (int)hd.y;
        const cplx v = aqc::ldg(in + k);
        double sr = 0.0, si = 0.0;
        for (int t = 0; t < nt; ++t) {
          const uint64_t z = stage[p + 1 + 2 * t].x;
          const ulonglong2 cw = stage[p + 2 + 2 * t];
          const cplx cf = aqc::cmk(__longlong_as_double((long long)cw.x), __longlong_as_double((long long)cw.y));
          if (__popcll(k & z) & 1) {
            sr -= cf.x;
            si -= cf.y;
          } else {
            sr += cf.x;
            si += cf.y;
          }
        }
        acc = aqc::cfma(aqc::cmk(sr, si), v, acc);
        p += 1 + 2 * nt;
      }
    }
    if (mine) aqc::stg(out + j, acc);
  }
}

// partial[2 blockIdx.x], [2 blockIdx.x + 1] = re, im of the workgroup's share of sum conj(a_k) b_k
__global__ __launch_bounds__(kThreads) void k_sv_dot(const cplx* __restrict__ a, const cplx* __restrict__ b,
                                                     uint64_t dim, double* __restrict__ partial) {
  __shared__ double red[4];
  double sr = 0.0, si = 0.0;
  for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < dim; k += (uint64_t)gridDim.x * kThreads) {
    const cplx v = aqc::cconjmul(aqc::ldg(a + k), aqc::ldg(b + k));
    sr += v.x;
    si += v.y;
  }
  const double tr = aqc::block_sum256(sr, red);
  const double ti = aqc::block_sum256(si, red);
  if (threadIdx.x == 0) {
    partial[2 * (size_t)blockIdx.x] = tr;
    partial[2 * (size_t)blockIdx.x + 1] = ti;
  }
}

__global__ void k_sv_dot_sum(const double* __restrict__ partial, int nblk, double* __restrict__ out2) {
  const int c = threadIdx.x;
  if (c >= 2) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partial[2 * (size_t)b + c];
  out2[c] = s;
}

// y <- a y + b x; x == nullptr: y <- a y
__global__ __launch_bounds__(kThreads) void k_sv_axpby(cplx* __restrict__ y, const cplx* __restrict__ x, uint64_t dim,
                                                       cplx a, cplx b) {
  const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= dim) return;
  cplx v = aqc::cmul(a, y[k]);
  if (x) v = aqc::cfma(b, aqc::ldg(x + k), v);
  y[k] = v;
}

// per-device grow-only scratch (tables, partials, results)
aqc::PerDevice<aqc::DevScratch> g_scr;

}  // namespace

extern "C" {

int aqc_sv_pauli_apply(aqc_sv_t in, aqc_sv_t out, const uint64_t* xmask, const uint64_t* zmask, const double* coeff,
                       int nterms) {
  AQC_REQUIRE(in && out, "aqc_sv_pauli_apply: null handle");
  AQC_REQUIRE(in != out, "aqc_sv_pauli_apply: in and out must be different states");
  AQC_REQUIRE(nterms >= 0 && nterms <= kMaxApplyTerms, "aqc_sv_pauli_apply: nterms outside 0 .. 2^20");
  AQC_REQUIRE((xmask && zmask && coeff) || nterms == 0, "aqc_sv_pauli_apply: null masks or coefficients");
  const cplx* src = nullptr;
  int n = 0, n_out = 0;
  hipStream_t st_in = nullptr, st = nullptr;
  cplx* dst = nullptr;
  n = aqc::sv_qubits(in);
  n_out = aqc::sv_qubits(out);
  AQC_REQUIRE(n == n_out, "aqc_sv_pauli_apply: in and out have different qubit counts");
  const uint64_t valid = n >= 64 ? ~0ull : (1ull << n) - 1;
  for (int t = 0; t < nterms; ++t) {
    AQC_REQUIRE(((xmask[t] | zmask[t]) & ~valid) == 0, "aqc_sv_pauli_apply: a mask bit at or above n");
    AQC_REQUIRE(std::isfinite(coeff[2 * t]) && std::isfinite(coeff[2 * t + 1]),
                "aqc_sv_pauli_apply: a coefficient is not finite");
  }
  if (int rc = aqc::sv_view(in, &src, &n, &st_in)) return rc;
  if (int rc = aqc::sv_overwrite(out, n, &dst, &st)) return rc;

  // groups by x mask in order of first appearance, terms of a group in input order
  std::vector<uint64_t> gx;
  std::vector<std::vector<int>> members;
  std::unordered_map<uint64_t, size_t> group_of;
  for (int t = 0; t < nterms; ++t) {
    auto it = group_of.find(xmask[t]);
    if (it == group_of.end()) {
      it = group_of.emplace(xmask[t], gx.size()).first;
      gx.push_back(xmask[t]);
      members.emplace_back();
    }
    members[it->second].push_back(t);
  }
  // the word stream and its chunks (cut at record headers)
  std::vector<ulonglong2> words;
  std::vector<int> chunk_off{0};
  auto bits = [](double d) {
    uint64_t v;
    std::memcpy(&v, &d, sizeof(v));
    return v;
  };
  int records = 0;
  for (size_t g = 0; g < gx.size(); ++g)
    for (size_t m0 = 0; m0 < members[g].size(); m0 += kMaxGroupTerms) {
      const int nt = (int)std::min<size_t>(kMaxGroupTerms, members[g].size() - m0);
      if ((int)words.size() - chunk_off.back() + 1 + 2 * nt > kStageWords) chunk_off.push_back((int)words.size());
      words.push_back(make_ulonglong2(gx[g], (uint64_t)nt));
      for (int i = 0; i < nt; ++i) {
        const int t = members[g][m0 + i];
        const double re = coeff[2 * t], im = coeff[2 * t + 1];
        double cr, ci;  // i^ny (re + i im)
        switch (__builtin_popcountll(xmask[t] & zmask[t]) & 3) {
          case 0: cr = re, ci = im; break;
          case 1: cr = -im, ci = re; break;
          case 2: cr = -re, ci = -im; break;
          default: cr = im, ci = -re; break;
        }
        words.push_back(make_ulonglong2(zmask[t], 0));
        words.push_back(make_ulonglong2(bits(cr), bits(ci)));
      }
      ++records;
    }
  chunk_off.push_back((int)words.size());
  const int nchunks = (int)chunk_off.size() - 1;

  const uint64_t dim = 1ull << n;
  const size_t wb = up256(std::max<size_t>(1, words.size()) * sizeof(ulonglong2));
  const size_t cb = up256(chunk_off.size() * sizeof(int));
  // in's queued work first (it lives on its own stream); the scratch is free again once this call's
  // own work has drained, which the wait at the end ensures for the next call
  AQC_HIP_CHECK(hipStreamSynchronize(st_in));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  aqc::DevScratch& sc = g_scr.here();
  if (int rc = sc.ensure(wb + cb)) return rc;
  ulonglong2* dwords = (ulonglong2*)sc.dev;
  int* dchunks = (int*)(sc.dev + wb);
  if (!words.empty())
    AQC_HIP_CHECK(hipMemcpyAsync(dwords, words.data(), words.size() * sizeof(ulonglong2), hipMemcpyHostToDevice, st));
  AQC_HIP_CHECK(hipMemcpyAsync(dchunks, chunk_off.data(), chunk_off.size() * sizeof(int), hipMemcpyHostToDevice, st));
  const unsigned grid = (unsigned)std::min<uint64_t>((dim + kThreads - 1) / kThreads, kMaxApplyBlocks);
  const double bytes = 16.0 * (double)dim * (records + 1), flops = (double)dim * (2.0 * nterms + 8.0 * records);
  if (nchunks == 1) {
    aqc::KernelTimer::begin(st, "sv_pauli_apply", bytes, flops);
    hipLaunchKernelGGL(k_sv_pauli_apply<true>, dim3(grid), dim3(kThreads), 0, st, src, dst, dim, (const ulonglong2*)dwords,
                       (const int*)dchunks, nchunks);
  } else {
    aqc::KernelTimer::begin(st, "sv_pauli_apply_chunks", bytes, flops);
    hipLaunchKernelGGL(k_sv_pauli_apply<false>, dim3(grid), dim3(kThreads), 0, st, src, dst, dim,
                       (const ulonglong2*)dwords, (const int*)dchunks, nchunks);
  }
  aqc::KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  return AQC_OK;
}

int aqc_sv_dot(aqc_sv_t a, aqc_sv_t b, double* out2) {
  AQC_REQUIRE(a && b, "aqc_sv_dot: null handle");
  AQC_REQUIRE(out2, "aqc_sv_dot: null out");
  const cplx *pa = nullptr, *pb = nullptr;
  int na = 0, nb = 0;
  hipStream_t sa = nullptr, st = nullptr;
  if (int rc = aqc::sv_view(a, &pa, &na, &sa)) return rc;
  if (int rc = aqc::sv_view(b, &pb, &nb, &st)) return rc;
  AQC_REQUIRE(na == nb, "aqc_sv_dot: the states have different qubit counts");
  const uint64_t dim = 1ull << na;
  const int nblk = (int)std::min<uint64_t>(256, std::max<uint64_t>(1, dim / 4096));
  const size_t pb_bytes = up256((size_t)2 * nblk * sizeof(double));
  if (sa != st) AQC_HIP_CHECK(hipStreamSynchronize(sa));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  aqc::DevScratch& sc = g_scr.here();
  if (int rc = sc.ensure(pb_bytes + 256)) return rc;
  double* partial = (double*)sc.dev;
  double* dout = (double*)(sc.dev + pb_bytes);
  aqc::KernelTimer::begin(st, "sv_dot", 32.0 * (double)dim, 8.0 * (double)dim);
  hipLaunchKernelGGL(k_sv_dot, dim3(nblk), dim3(kThreads), 0, st, pa, pb, dim, partial);
  AQC_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_sv_dot_sum, dim3(1), dim3(64), 0, st, (const double*)partial, nblk, dout);
  aqc::KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  AQC_HIP_CHECK(hipMemcpyAsync(out2, dout, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  return AQC_OK;
}

int aqc_sv_axpby(aqc_sv_t y, double ar, double ai, aqc_sv_t x, double br, double bi) {
  AQC_REQUIRE(y, "aqc_sv_axpby: null y");
  AQC_REQUIRE(x != y, "aqc_sv_axpby: x and y must be different states");
  AQC_REQUIRE(std::isfinite(ar) && std::isfinite(ai) && std::isfinite(br) && std::isfinite(bi),
              "aqc_sv_axpby: a coefficient is not finite");
  const bool scale_only = br == 0.0 && bi == 0.0;
  AQC_REQUIRE(x || scale_only, "aqc_sv_axpby: null x with b != 0");
  const cplx* px = nullptr;
  int n = 0, nx = 0;
  hipStream_t sx = nullptr, st = nullptr;
  if (x) {
    if (int rc = aqc::sv_view(x, &px, &nx, &sx)) return rc;
  }
  cplx* py = nullptr;
  if (int rc = aqc::sv_mutable(y, &py, &n, &st)) return rc;
  AQC_REQUIRE(!x || nx == n, "aqc_sv_axpby: x and y have different qubit counts");
  if (scale_only) px = nullptr;
  if (px) AQC_HIP_CHECK(hipStreamSynchronize(sx));  // x's queued work (its own stream) first
  const uint64_t dim = 1ull << n;
  const uint64_t grid = (dim + kThreads - 1) / kThreads;
  AQC_REQUIRE(grid <= kElemBlocks, "aqc_sv_axpby: more than 2^34 amplitudes");
  aqc::KernelTimer::begin(st, "sv_axpby", (px ? 48.0 : 32.0) * (double)dim, (px ? 14.0 : 6.0) * (double)dim);
  hipLaunchKernelGGL(k_sv_axpby, dim3((unsigned)grid), dim3(kThreads), 0, st, py, px, dim, aqc::cmk(ar, ai),
                     aqc::cmk(br, bi));
  aqc::KernelTimer::end(st);
  AQC_CHECK_LAUNCH();
  // x is read on y's stream: done before the caller can rewrite or free it
  AQC_HIP_CHECK(hipStreamSynchronize(st));
  return AQC_OK;
}

}  // extern "C"
