// MPS engine internals shared by mps.hip (gate application), mps_meas.hip (measurements),
// mps_traj.hip (noisy trajectories) and grad.hip (candidate sweep).
#pragma once

#include <algorithm>
#include <mutex>
#include <vector>

#include "aqc_internal.h"

struct aqc_dmrg_s;  // dmrg.hip

namespace aqc {

// Device layout of one MPS (Vidal form, as Aer's MPS simulator keeps it):
//   gam : n sites x [2][cap][cap] complex, row-major [s][l][r]; site i uses l < dims[i],
//         r < dims[i+1].
//   lam : (n+1) bonds x cap doubles; bond b sits left of site b; lam[0] = lam[n] = {1}.
//   dims: (n+1) ints on device, dims[0] = dims[n] = 1.
// The qubit permutation created by Aer's swap routing lives on the host (order / loc).
// Largest two-site column count 2 chi (bond capacity <= 1024): the singular-value buffer holds the
// raw column norms at [0, kSigMax) and the sorted values at [kSigMax, 2 kSigMax).  sig[kSigTail]:
// the part of the reduce_zeros tail sum that an SVD path which decides the kept count itself (the
// Gram paths, svd_gram.h / gram_big.hip) has already removed -- it writes the kept singular values
// and zeros, and the rank step's tail rule continues from this sum (then resets it to 0).
constexpr int kSigMax = 2048;
constexpr int kMaxCap = kSigMax / 2;
constexpr int kSigTail = 2 * kSigMax;
constexpr int kSigLen = 2 * kSigMax + 2;  // doubles
// Two-site work buffer (complex elements): 4 cap^2 (the Jacobi's working columns), and at least what
// the 2 chi = 128 Gram path lays out in it (svd_gram.h: reflectors, W, the compact-WY factors and the
// inverse-iteration scratch of more than 64 kept vectors)
constexpr size_t kGramWorkElems = 36864;
inline size_t work_elems(size_t cap) { return 4 * cap * cap > kGramWorkElems ? 4 * cap * cap : kGramWorkElems; }

struct MpsDev {
  int n = 0;
  int cap = 0;
  cplx* gam = nullptr;
  double* lam = nullptr;
  int* dims = nullptr;
  // two-site workspace
  cplx* theta = nullptr;  // (2cap)^2, column-major M x N
  cplx* work = nullptr;   // work_elems(cap): Jacobi working columns / Gram-path scratch
  double* sig = nullptr;  // kSigLen: column norms, then the sorted values, then the removed tail
  int* perm = nullptr;    // kSigMax sorted -> column index
  int* flags = nullptr;   // [0] capacity overflow, [1] jacobi non-convergence, [2] max sweeps used
  // measurement workspace
  cplx* env = nullptr;    // 2 * (n+1) * cap * cap  (left and right environments)
  cplx* tmp = nullptr;    // 2 * cap * cap
  cplx* vec = nullptr;    // 2 * (n+1) * cap  (left / right zero-chains)
  cplx* scal = nullptr;   // scratch results (2n + 8 complex)

  size_t site_stride() const { return (size_t)2 * cap * cap; }
  cplx* site(int i) const { return gam + (size_t)i * site_stride(); }
  double* bond(int b) const { return lam + (size_t)b * cap; }
};

// One two-site update of one state (k_theta -> SVD -> k_rank -> k_split_*), see mps.hip.
struct TwoSiteJob {
  cplx* gp;
  cplx* gq;
  const double* ll;
  double* lm;
  const double* lr;
  int* dims;  // &dims[p] : dims[0] = chi_l, dims[1] = chi_m, dims[2] = chi_r
  cplx* theta;
  cplx* work;
  double* sig;
  int* perm;
  int* flags;
  int cap;
  int max_chi;
  double thr;
  double jtol;  // Jacobi rotation threshold factor
  double jtiny; // sweep stop: a sweep whose counted rotations all had |t| <= jtiny is the last
  int qr;      // 1: Jacobi ran on R^H of a pivoted QR -> W holds the other side (see k_jacobi_reg)
  int dbg;      // diagnostics (aqc_svd_debug): 1 = stop after the QR phase, write X unpermuted
  int gram;     // 1: try the Gram / tridiagonal SVD first (svd_gram.h), the Jacobi as fallback
  int pad_;
  double jnoise;  // Jacobi dot-product noise floor, in units of eps ||W|| (|a| + |b|) (0: off)
  cplx G[16];  // row = 2*s1'+s2' (out), col = 2*s1+s2 (in)
};

// Squared dot-product noise floor factor of the Jacobi rotations: a pair rotates only if
// |g|^2 > jacobi_noise2(j, ||W||^2) (|a|^2 + |b|^2) (mps.hip, jacobi_reg_body).
__device__ __forceinline__ double jacobi_noise2(const TwoSiteJob& j, double fro2) {
  const double e = j.jnoise * 2.220446049250313e-16;
  return 2.0 * e * e * fro2;
}

// Rotation parameters of the pair (alpha, beta, gamma = gx + i gy): t = sgn(zeta) /
// (|zeta| + sqrt(1 + zeta^2)), zeta = (beta - alpha) / (2|gamma|), c = 1/sqrt(1 + t^2) and
// s e = c t gamma / |gamma|.  v_rsq_f64 / v_rcp_f64 seeds with two Newton steps each (full double
// precision) instead of the IEEE sqrt / divide sequences: this chain is serial per round.
__device__ __forceinline__ void jacobi_params(double al, double be, double gx, double gy, double g2, double& c,
                                              double& ex, double& ey) {
  double rg = __builtin_amdgcn_rsq(g2);  // 1 / |gamma|
  rg = rg * fma(-0.5 * g2 * rg, rg, 1.5);
  rg = rg * fma(-0.5 * g2 * rg, rg, 1.5);
  const double zeta = 0.5 * (be - al) * rg;
  const double q = fma(zeta, zeta, 1.0);
  double rq = __builtin_amdgcn_rsq(q);
  rq = rq * fma(-0.5 * q * rq, rq, 1.5);
  rq = rq * fma(-0.5 * q * rq, rq, 1.5);
  const double den = fabs(zeta) + q * rq;  // |zeta| + sqrt(1 + zeta^2)
  double inv = __builtin_amdgcn_rcp(den);
  inv = inv * fma(-den, inv, 2.0);
  inv = inv * fma(-den, inv, 2.0);
  const double t = zeta >= 0 ? inv : -inv;
  const double p = fma(t, t, 1.0);
  double cc = __builtin_amdgcn_rsq(p);
  cc = cc * fma(-0.5 * p * cc, cc, 1.5);
  cc = cc * fma(-0.5 * p * cc, cc, 1.5);
  c = cc;
  const double sc = cc * t * rg;
  ex = gx * sc;
  ey = gy * sc;
}

// Jacobi rotation of the pair (alpha = |a|^2, beta = |b|^2, |g|^2 = |a^H b|^2): t = sgn(zeta) /
// (|zeta| + sqrt(1 + zeta^2)), zeta = (beta - alpha) / (2|g|), c = 1 / sqrt(p), p = 1 + t^2,
// rg = 1 / |g| (rsq / rcp seeds with two Newton steps each: full double precision).
__device__ __forceinline__ void jacobi_tc(double al, double be, double g2, double& t, double& c, double& p,
                                          double& rg) {
  double r = __builtin_amdgcn_rsq(g2);
  r = r * fma(-0.5 * g2 * r, r, 1.5);
  r = r * fma(-0.5 * g2 * r, r, 1.5);
  rg = r;
  const double zeta = 0.5 * (be - al) * r;
  const double q = fma(zeta, zeta, 1.0);
  double rq = __builtin_amdgcn_rsq(q);
  rq = rq * fma(-0.5 * q * rq, rq, 1.5);
  rq = rq * fma(-0.5 * q * rq, rq, 1.5);
  const double den = fabs(zeta) + q * rq;
  double inv = __builtin_amdgcn_rcp(den);
  inv = inv * fma(-den, inv, 2.0);
  inv = inv * fma(-den, inv, 2.0);
  t = zeta >= 0 ? inv : -inv;
  p = fma(t, t, 1.0);
  double cc = __builtin_amdgcn_rsq(p);
  cc = cc * fma(-0.5 * p * cc, cc, 1.5);
  cc = cc * fma(-0.5 * p * cc, cc, 1.5);
  c = cc;
}

// The same rotation without |g|: with h = (beta - alpha) / 2, t / |g| = sgn(h) / (|h| + sqrt(h^2 +
// |g|^2)) =: te, so t e = te g, t |g| = te |g|^2 and p = 1 + t^2 = 1 + te^2 |g|^2.  One rsq and
// one rcp, each with a single Newton step (their ~2^-23 seeds -> ~2^-46: the angle needs no more,
// as long as c = 1 / sqrt(p) is exact for the t actually applied -- two Newton steps there).
__device__ __forceinline__ void jacobi_te(double al, double be, double g2, double& te, double& c, double& p) {
  const double h = 0.5 * (be - al);
  const double q = fma(h, h, g2);
  double rq = __builtin_amdgcn_rsq(q);
  rq = rq * fma(-0.5 * q * rq, rq, 1.5);
  const double den = fabs(h) + q * rq;
  double inv = __builtin_amdgcn_rcp(den);
  inv = inv * fma(-den, inv, 2.0);
  te = h >= 0 ? inv : -inv;
  p = fma(te * te, g2, 1.0);
  double cc = __builtin_amdgcn_rsq(p);
  cc = cc * fma(-0.5 * p * cc, cc, 1.5);
  cc = cc * fma(-0.5 * p * cc, cc, 1.5);
  c = cc;
}

constexpr double kReduceChop = 1e-16;  // reduce_zeros' CHOP on sigma^2 (mps.hip kChop)
// Both Gram paths (svd_gram.h gs_clusters, gram_big.hip k_gb_gs): eigenvalues of T closer than this
// times ||T|| share a cluster and are orthogonalised against each other after the inverse iteration
constexpr double kGramClusterGap = 1e-5;

// reduce_zeros (oracle/mps.py truncation_rank: Aer's rule as the reference drives it,
// aer_mps_backend.py:27-42) on the top KE eigenvalues lam (descending, = sigma^2) of G, each known to
// +-err: CHOP (sigma^2 > 1e-16), the max_chi cap, then the tail rule (drop the smallest while the
// dropped sum stays below thr).  Every comparison must hold for any values inside the error bars --
// err is the multisection bracket, plus the noise of forming and reducing G (16 C eps ||T||) -- and
// the kept values must clear the Gram path's floor (lambda_K > floor lambda_1, 1e-9); otherwise -1 (the
// caller declines and the Jacobi decides).  An eigenvalue whose CHOP decision is open may still be
// dropped by the tail rule from either start, which then decides nothing: it enters the tail as
// [0, lam + err].  Returns the kept count K, and in tail_out the dropped tail sum (handed to
// rank_body through sig[kSigTail], whose own tail rule then keeps all K).
// cert (optional): where that fails only because of values in the CHOP's open band -- a rank-deficient
// theta', whose numerically zero eigenvalues come out of G as +-(noise) -- the decision that they all
// fall below the CHOP, with *cert = 1: valid if the caller then shows ||X - X V V^H||_F^2 < CHOP / 2
// for the K kept right vectors V (every dropped sigma^2 is then below it; gram_big.hip k_gb_cert).
[[maybe_unused]] static __device__ __noinline__ int gram_keep(const double* lam, const double* err, int KE, int C, int max_chi,
                                             double thr, double tn, double floor, double& tail_out,
                                             int* cert = nullptr) {
  const double noise = 16.0 * C * 2.220446049250313e-16 * tn;
  int k_lo = 0, k_hi = 0;  // counts surely / possibly above the CHOP (lam descending)
  for (int i = 0; i < KE; ++i) {
    const double e = err[i] + noise;
    if (lam[i] - e > kReduceChop) k_lo = i + 1;
    if (lam[i] + e > kReduceChop) k_hi = i + 1;
  }
  if (cert) *cert = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    // attempt 0: the open values as [0, lam + err]; attempt 1 (cert): the open values chopped
    if (attempt == 1 && !(cert && k_hi > k_lo)) return -1;
    int k = attempt == 0 ? k_hi : k_lo;
    if (k < 1) k = 1;
    if (max_chi > 0 && k > max_chi) k = max_chi;
    double tail = 0.0, unc = 0.0;
    bool ok = true;
    while (k > 1) {
      const int i = k - 1;
      const double e = err[i] + noise;
      double v = lam[i], ev = e;
      if (i >= k_lo) {  // CHOP open: contributes anything in [0, lam + e] if dropped
        v = 0.5 * (lam[i] + e);
        ev = v;
      }
      const double sum = tail + v, m = unc + ev;
      if (fabs(sum - thr) <= m) {  // the comparison is open
        ok = false;
        break;
      }
      if (sum >= thr) break;
      if (attempt == 1) {  // (a surely-kept value dropped: the certificate cannot tell them apart)
        ok = false;
        break;
      }
      tail = sum;
      unc = m;
      --k;
    }
    if (!ok) continue;
    if (k > k_lo) continue;  // a kept value whose CHOP is open (also far below the floor)
    if (!(lam[0] > 0.0) || !(lam[k - 1] > floor * lam[0])) return -1;
    tail_out = tail;
    if (attempt == 1) *cert = !(max_chi > 0 && k_lo >= max_chi);
    return k;
  }
  return -1;
}

// Multi-workgroup block one-sided Jacobi SVD for 2 * chi > 128 (bjacobi.hip): factors the nj
// two-site thetas of `jobs` (device array) into the k_jacobi output contract (W columns = U sigma,
// sig = column norms, qr = 0).  Enqueued on `st`; synchronises the host once per sweep (from the
// third on) to stop when every decomposition has converged.
int block_jacobi(const TwoSiteJob* jobs, int nj, int cap_max, hipStream_t st);

// Two-site SVDs at 2 chi = side in (128, 2048] (gram_big.hip): the multi-workgroup Gram path
// (G = X^H X of the C x C side, C = min(2 chi_l, 2 chi_r) <= 1024; tridiagonalisation over several
// workgroups per job, inverse iteration, V = Q Z; output contract qr = 1, written into the device
// job), the block Jacobi for the jobs it declines (and for C > 1024).
// hjobs: host copies of the device jobs (qr = 0).  Synchronises the host once.
int big_svd(const TwoSiteJob* hjobs, const TwoSiteJob* jobs, int nj, int side, int cap_max, hipStream_t st);

hipStream_t mps_stream();
hipStream_t mps_stream_if_any(int dev);

// threadIdx.x read through an empty asm: values a phase derives from it cannot be hoisted out of
// the chain loop in k_chain (where they would stay live across every other phase)
__device__ __forceinline__ int fresh_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Job staging for the launches on the MPS stream: a ring of buffer sets per device, each with an
// event recorded after the launches that read it, so that building the next batch's jobs waits
// only for the set's previous use (four calls back) instead of draining the stream -- the host
// schedules while the GPU still runs the previous work.
constexpr int kStagingRing = 4;
struct StagingRing {
  std::mutex mu;
  DevScratch set[kStagingRing];
  int next = 0;
  void release() {
    for (auto& s : set) s.release();
  }
};

StagingRing& staging_ring();  // the current device's (the one table, mps.hip)

// A lease on the next set of this device's ring.  It holds the device's staging mutex for its
// lifetime (several host threads may drive one device) and records the set's event on the stream
// on EVERY exit path -- an early error return included -- so the set is never handed out again
// while kernels queued before the error may still read it.  The mutex is not recursive: no lease is
// held across a call that takes one (run_waves, and so the sorts, every batched measurement).
class StagingLease {
 public:
  explicit StagingLease(hipStream_t st) : st_(st), ring_(staging_ring()), lk_(ring_.mu) {
    ss_ = &ring_.set[ring_.next];
    ring_.next = (ring_.next + 1) % kStagingRing;
    rc_ = ss_->wait();
  }
  ~StagingLease() {
    // no event: drain instead, so the next user finds the set idle
    if (ss_->mark(st_) != AQC_OK) hipStreamSynchronize(st_);
  }
  StagingLease(const StagingLease&) = delete;
  StagingLease& operator=(const StagingLease&) = delete;
  DevScratch& buf() { return *ss_; }
  int rc() const { return rc_; }

  // Sizes the leased set for `bytes`.  A set that must grow brings the whole ring to the new size
  // at once (waiting for the other sets' last uses): grown one set at a time, a workload whose
  // calls per step are not a multiple of the ring's length met a fresh (smaller) set in each of
  // its first four steps, and each growth's hipFree drained the device mid-step.
  int ensure(size_t bytes) {
    if (bytes <= ss_->cap && bytes <= ss_->hcap) return AQC_OK;
    const size_t want = std::max({bytes, ss_->cap * 2, ss_->hcap * 2});
    for (DevScratch& s : ring_.set) {
      if (&s != ss_)
        if (int rc = s.wait()) return rc;
      if (int rc = s.ensure(want, want)) return rc;
    }
    return AQC_OK;
  }

 private:
  hipStream_t st_;
  StagingRing& ring_;
  std::unique_lock<std::mutex> lk_;
  DevScratch* ss_ = nullptr;
  int rc_ = AQC_OK;
};

// ---- host-side scheduling (mps.hip; mps_traj.hip builds its schedules with the same types) --------
struct DevOp {
  // 1: one-site, 2: two-site (p, p+1), 3: one-site Kraus / measurement row, 4: a correlated group's
  // event as a two-site update of (p, p+1) whose 4x4 operator is chosen on the device, 5: a
  // product-unitary group's event on the sites p and p2 (any two; mps_traj.hip), 6: a DMRG update of
  // (p, p+1): theta is formed with the identity and a Lanczos iteration on the bond's effective
  // Hamiltonian replaces it with the lowest Ritz vector (dmrg.hip); slot = the sweep's output slot of
  // the Ritz value, grp = the direction (0: left to right)
  int kind;
  int p;
  cplx m[16];  // kind 3: the nk 2x2 operators K_k, 4 elements each; kind 4: the identity (theta's G)
  // kind 3 only.  nk: the number of operators; slot: the row's uniform and output slot -- the event
  // index e of a Kraus row, the qubit q of a measurement row (meas = 1, K = {|0><0|, |1><1|})
  // kinds 4 and 5: slot = the event index, grp = the group's place in the call's table (Kraus2Group)
  int nk, slot, meas, grp;
  int p2, pad;  // kind 5: the second site
};

// the rows that run as two-site updates of (p, p+1)
inline bool two_site(const DevOp& d) { return d.kind == 2 || d.kind == 4 || d.kind == 6; }

// host complex arithmetic without fma(): the x86 host build has no FMA instructions enabled, so
// fma() is a libm call per operation
inline cplx hc(double r, double i) { return cmk(r, i); }
inline cplx hmul(cplx a, cplx b) { return cmk(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
inline cplx hfma(cplx a, cplx b, cplx c) { return cmk(c.x + a.x * b.x - a.y * b.y, c.y + a.x * b.y + a.y * b.x); }

inline void mat2_mul(const cplx* a, const cplx* b, cplx* out) {  // out = a b (2x2)
  cplx t[4];
  for (int r = 0; r < 2; ++r)
    for (int c = 0; c < 2; ++c)
      t[r * 2 + c] = hfma(a[r * 2 + 1], b[2 + c], hmul(a[r * 2], b[c]));
  for (int e = 0; e < 4; ++e) out[e] = t[e];
}

struct Scheduler {
  int n;
  std::vector<int>& order;
  std::vector<int>& loc;
  std::vector<cplx> pend;     // 4 per qubit
  std::vector<char> has;
  std::vector<DevOp>& out;

  Scheduler(int n_, std::vector<int>& o, std::vector<int>& l, std::vector<DevOp>& dst)
      : n(n_), order(o), loc(l), pend(4 * n_), has(n_, 0), out(dst) {}

  void swap_sites(int p) {
    DevOp d = DevOp();
    d.kind = 2;
    d.p = p;
    // SWAP in site order: out (s1', s2') = in (s2, s1)
    for (int o = 0; o < 4; ++o) {
      const int s1 = o >> 1, s2 = o & 1;
      const int in = 2 * s2 + s1;
      d.m[o * 4 + in] = hc(1, 0);
    }
    out.push_back(d);
    const int qa = order[p], qb = order[p + 1];
    order[p] = qb;
    order[p + 1] = qa;
    loc[qa] = p + 1;
    loc[qb] = p;
  }

  void one(int q, const double* m) {
    cplx u[4];
    for (int e = 0; e < 4; ++e) u[e] = hc(m[2 * e], m[2 * e + 1]);
    if (!has[q]) {
      for (int e = 0; e < 4; ++e) pend[4 * q + e] = u[e];
      has[q] = 1;
    } else {
      mat2_mul(u, &pend[4 * q], &pend[4 * q]);
    }
  }

  // swap-left routing of (qa, qb) to adjacent sites (low, low + 1); returns low
  int route(int qa, int qb) {
    const int pa = loc[qa], pb = loc[qb];
    const int low = std::min(pa, pb), high = std::max(pa, pb);
    for (int i = high; i > low + 1; --i) swap_sites(i - 1);  // change_position(high, low+1)
    return low;
  }

  // the pending one-qubit gates of qa and qb (the identity where none)
  void pending(int qa, int qb, cplx* Pa, cplx* Pb) const {
    for (int e = 0; e < 4; ++e) Pa[e] = Pb[e] = hc(e == 0 || e == 3 ? 1 : 0, 0);
    if (has[qa])
      for (int e = 0; e < 4; ++e) Pa[e] = pend[4 * qa + e];
    if (has[qb])
      for (int e = 0; e < 4; ++e) Pb[e] = pend[4 * qb + e];
  }

  // M4 (index 2*b1 + b0, b0 <-> qa) with the pending gates Pa, Pb folded in, in the site order of
  // (low, low + 1) where the routed qubits sit: out[(2 s1' + s2')][(2 s1 + s2)]
  void fold_site_order(int qa, int low, const cplx* M4, const cplx* Pa, const cplx* Pb, cplx* out16) const {
    // fold pending one-qubit gates: M' = M . kron(P_b, P_a)   (index 2*b1 + b0, b0 <-> qa)
    cplx K[16];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) K[r * 4 + c] = hmul(Pb[(r >> 1) * 2 + (c >> 1)], Pa[(r & 1) * 2 + (c & 1)]);
    cplx Mf[16];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) {
        cplx acc = hc(0, 0);
        for (int t = 0; t < 4; ++t) acc = hfma(M4[r * 4 + t], K[t * 4 + c], acc);
        Mf[r * 4 + c] = acc;
      }
    // to site order: G[(2 s1' + s2')][(2 s1 + s2)]
    const bool a_low = loc[qa] == low;
    for (int so = 0; so < 4; ++so)
      for (int si = 0; si < 4; ++si) {
        const int s1o = so >> 1, s2o = so & 1, s1i = si >> 1, s2i = si & 1;
        int ro, ci;
        if (a_low) {  // b0 = s1 (qa), b1 = s2 (qb)
          ro = 2 * s2o + s1o;
          ci = 2 * s2i + s1i;
        } else {  // b0 = s2 (qa), b1 = s1 (qb)
          ro = 2 * s1o + s2o;
          ci = 2 * s1i + s2i;
        }
        out16[so * 4 + si] = Mf[ro * 4 + ci];
      }
  }

  void two(int qa, int qb, const double* m) {
    const int low = route(qa, qb);
    cplx M4[16];
    for (int e = 0; e < 16; ++e) M4[e] = hc(m[2 * e], m[2 * e + 1]);
    cplx Pa[4], Pb[4];
    pending(qa, qb, Pa, Pb);
    has[qa] = has[qb] = 0;
    DevOp d = DevOp();
    d.kind = 2;
    d.p = low;
    fold_site_order(qa, low, M4, Pa, Pb, d.m);
    out.push_back(d);
  }

  void flush() {
    for (int q = 0; q < n; ++q) {
      if (!has[q]) continue;
      DevOp d = DevOp();
      d.kind = 1;
      d.p = loc[q];
      for (int e = 0; e < 4; ++e) d.m[e] = pend[4 * q + e];
      out.push_back(d);
      has[q] = 0;
    }
  }

  void sort() {
    for (int left = 0; left < n; ++left) {
      const int pos = loc[left];
      for (int j = pos; j > left; --j) swap_sites(j - 1);
    }
  }
};

// What the Kraus / measurement rows of a batch of trajectories share (mps_traj.hip): state s of the
// lists handed to run_waves carries shot shot0 + s.  Row slots: Kraus event e -> e, the measurement of
// qubit q -> nev + q, out of nper = nev + n per shot (aqc_mps_traj_pair_tomo has no measurement rows:
// nper = nev + npairs, pair j's draw in slot nev + j).
struct Kraus2Group;
struct TrajCtx {
  uint64_t seed, run;
  const double* u;   // device: null, or [shot][nper] uniforms replacing sample_uniform(seed, run, shot, slot)
  uint64_t* out;     // device: [shot][words] outcome words, zeroed by the caller (null without measurement rows)
  uint8_t* choices;  // device: null, or [shot][nev]
  int shot0, nev, nper, words;
  // correlated groups (null / 0 in a call without one): the call's group table, and for the general
  // events of one wave k_mps_kraus2_rho's partial sums [job][k2_slices][16] and the chosen operator
  // [job][16]; k2_jobs: the most general events one wave may hold
  const Kraus2Group* groups;
  double* k2_part;
  cplx* k2_sel;
  int k2_slices, k2_jobs;
};

// One correlated group of a call, in device memory once per call.  A general group: K[k] the folded
// 4x4 operator in site order, out 2 s1' + s2', in 2 s1 + s2; W[k] = K_k^dag K_k as M00 M11 M22 M33 then
// (Re, Im) of M01 M02 M03 M12 M13 M23.  A product-unitary group: K[k][0..3] the 2x2 unitary of the
// event's site p (the operator's scalar over its modulus folded in), K[k][4..7] that of site p2.
// flat: every K_k^dag K_k is a multiple of I, the constant weight p_k in W[k][0].
struct Kraus2Group {
  cplx K[16][16];
  double W[16][16];
  int nk, flat, pad[2];
};

// One general group event of one state as the k_mps_kraus2_* kernels read it: `two` indexes the
// wave's two-site jobs, whose theta the event acts on.
struct Kraus2Job {
  int two, grp, slot, shot;
};

// One product-unitary group event of one state (k_mps_kraus2_prod).
struct Kraus2ProdJob {
  cplx* g0;  // Gamma of the site of K[k][0..3]
  cplx* g1;  // Gamma of the site of K[k][4..7]
  const int* dims0;
  const int* dims1;
  int cap, grp, slot, shot;
};

// One Kraus / measurement row of one state, as k_mps_kraus1 reads it (mps_traj.hip).
struct KrausJob {
  cplx* g;           // the site's Gamma [2][cap][cap]
  const double* ll;  // lambda left of the site
  const double* lr;  // lambda right of it
  const int* dims;   // &dims[p]
  int cap, nk, slot, meas;
  int shot, pad;
  cplx K[16];        // K_k at K + 4 k
  double w[16];      // (M00, M11, Re M01, Im M01) of M = K_k^dag K_k at w + 4 k
};

// Queues k_mps_kraus1 over nj device jobs on st (mps_traj.hip).
int launch_kraus(const KrausJob* jobs, int nj, const TrajCtx& ctx, hipStream_t st);
// Queues a wave's general group events on st, behind the k_theta launch that formed their thetas
// (G = identity) and in front of the wave's SVDs: rho in slices, the choice, the chosen operator
// applied to theta in place (mps_traj.hip).  cap_max: the largest capacity among the jobs.
int launch_kraus2(const TwoSiteJob* two, const Kraus2Job* jobs, int nj, int cap_max, const TrajCtx& ctx, hipStream_t st);
// Queues k_mps_kraus2_prod over nj device jobs on st (mps_traj.hip).
int launch_kraus2_prod(const Kraus2ProdJob* jobs, int nj, int cap_max, const TrajCtx& ctx, hipStream_t st);

// Queues a kind-6 op's eigensolver on st, behind the k_theta launch that formed its theta (G = identity)
// and in front of the wave's SVD: the lowest Ritz vector of the bond's effective Hamiltonian over theta,
// normalised, the Ritz value to the sweep's slot (dmrg.hip).
int launch_heff(const DevOp& op, aqc_dmrg_s* dmrg, hipStream_t st);
// Queues, behind the op's split, the environment step through the site the update has just fixed.
int launch_dmrg_env(const DevOp& op, aqc_dmrg_s* dmrg, hipStream_t st);

// Runs per-state device-op lists in lock-step waves on the MPS stream (mps.hip); returns once the
// work is queued.  Lists with kind-3 rows need ctx and never take the fused chain.  Kind-6 ops need
// dmrg, one state, and never take the fused chain either.
int run_waves(aqc_mps_s** hs, int ns, std::vector<std::vector<DevOp>>& lists, const TrajCtx* ctx = nullptr,
              aqc_dmrg_s* dmrg = nullptr);

// The handle back to |0...0> in sorted qubit order, queued on the MPS stream (mps.hip).
int mps_reset_zero(aqc_mps_s* h);

// The error flags of many states in a read-back the caller makes anyway (mps.hip).  The caller puts
// the states' flag pointers (flag_ptrs) into the staging it uploads, queues the gather of
// flags[0] | flags[1] per state into `out` (device, ns ints) behind it, and hands the host copy of
// `out` to settle_flags: every raised flag is read and reset, the first error (in list order) is
// reported.
void flag_ptrs(const aqc_mps_t* hs, int ns, int** ptrs);
int queue_flag_gather(int* const* dptrs, int ns, int* out, hipStream_t st);
int settle_flags(const aqc_mps_t* hs, int ns, const int* raised);

}  // namespace aqc

// The right environments R_1 .. R_n of one state in sorted qubit order (ent.hip: the chains that
// aqc_mps_z_all_batch runs at the state's capacity, with its single-workgroup re-run after a
// hand-off timeout), complete when the call returns: R_b at renv + b cap^2, row-major with row
// stride cap.  They live in ent.hip's per-device buffer until its next use, followed by `extra_bytes`
// of workspace for the caller (256-byte aligned); *stream is the library's stream.
namespace aqc {
int mps_right_envs(aqc_mps_s* h, size_t extra_bytes, const cplx** renv, void** extra, hipStream_t* stream);
// Both sides for ns states of one n and capacity (sorted; the caller checks that), from the same
// chains in one set of launches: state s has L_0 .. L_{n-1} ([bra][ket]) at lenv + s state_stride +
// b cap^2 and R_1 .. R_n ([ket][bra]) (n + 1) cap^2 elements further, row stride cap.  `family`
// names the launches for aqc_timing_query; the rest as above (*extra is 16-byte aligned).
int mps_envs_batch(aqc_mps_s** hs, int ns, size_t extra_bytes, const char* family, const cplx** lenv,
                   size_t* state_stride, void** extra, hipStream_t* stream);
// Bytes of that buffer mps_envs_batch takes per state of n qubits at capacity cap (both sides and the
// chains' scratch), for a caller that budgets device memory.
size_t env_state_bytes(int n, int cap);
// Bytes of that buffer aqc_mps_pair_rdms_batch takes per state of n qubits at capacity cap, for pairs
// with `na` distinct lower qubits (a caller that budgets device memory sizes its batches by it).
size_t pair_rdm_state_bytes(int n, int cap, int na);
}

struct aqc_mps_s {
  aqc::MpsDev d;
  double thr = 1e-16;
  int max_chi = 0;
  int dev = 0;  // the device the handle's buffers live on (aqc_mps_create's current device)
  std::vector<int> order;  // site -> qubit
  // host upper bounds of the bond dimensions (n + 1; exact after a load or a dims read-back, then
  // advanced per two-site update as min(2 chi_l, 2 chi_r, cap, max_chi)): the lock-step path picks
  // each wave's SVD kernel by the largest theta the wave can hold, not by the capacity
  std::vector<int> ub;
  std::vector<int> loc;    // qubit -> site
  // Reload bookkeeping (aqc_mps_copy_batch): `version` changes with every change of the device
  // contents; after a copy from the handle with id `synced_src` at its version `synced_ver`, the
  // Gamma sites changed since are [dirty_lo, dirty_hi], so a reload from the same, unchanged
  // source rewrites only those (lambdas and dims in full): the result is that of a full copy.
  unsigned long long uid = 0;
  unsigned long long version = 0;
  unsigned long long synced_src = 0;
  unsigned long long synced_ver = 0;
  int dirty_lo = 1 << 30, dirty_hi = -1;
  // Cached Z-sum environments (ent.hip, aqc_mps_z_sum_batch): zenv holds, per bond b, the left pair
  // (L_b, LZ_b) and the right pair (R_b, RZ_b); left pairs are current for bonds <= zl, right pairs
  // for bonds >= zr.  A rewrite of Gamma sites lo..hi (and the lambdas between them) leaves the left
  // environments up to bond lo and the right ones from bond hi + 1 as they were.
  aqc::cplx* zenv = nullptr;
  int zl = 0, zr = 1 << 30;
  // Cached zero / Hamming-weight-1 rows (mps_meas.hip, aqc_mps_zero_hw1_batch), per bond b: from the
  // left <0..0| A_0 .. A_{b-1} (row 0) and the same with site k < b flipped (row 1 + k); from the
  // right A_b .. A_{n-1} |0..0> (row 0) and with site k >= b flipped (row 1 + k).  Every row is
  // current for bonds <= hl (left) and >= hr (right), row 0 for bonds <= h0l / >= h0r.
  aqc::cplx* hwenv = nullptr;
  int hl = 0, hr = 1 << 30, h0l = 0, h0r = 1 << 30;
  void changed(int lo, int hi) {  // Gamma sites lo..hi rewritten
    ++version;
    dirty_lo = lo < dirty_lo ? lo : dirty_lo;
    dirty_hi = hi > dirty_hi ? hi : dirty_hi;
    zl = lo < zl ? lo : zl;
    zr = hi + 1 > zr ? hi + 1 : zr;
    hl = lo < hl ? lo : hl;
    hr = hi + 1 > hr ? hi + 1 : hr;
    h0l = lo < h0l ? lo : h0l;
    h0r = hi + 1 > h0r ? hi + 1 : h0r;
  }
  void changed_all() {
    ++version;
    synced_src = 0;
    zenv_stale();
  }
  void zenv_stale() {  // every cached environment and row past the boundaries
    zl = hl = h0l = 0;
    zr = hr = h0r = d.n;
  }
  // the one device block the handle's fixed buffers are carved from (aqc::dev_alloc)
  void* base = nullptr;
  // scratch for the candidate sweep (grad.hip), allocated lazily
  aqc::cplx* gw = nullptr;
  size_t gw_bytes = 0;
  // extra two-site workspaces for concurrent updates of disjoint bonds (mps.hip run_waves)
  struct Slot {
    aqc::cplx* theta = nullptr;
    aqc::cplx* work = nullptr;
    double* sig = nullptr;
    int* perm = nullptr;
  };
  std::vector<Slot> slots;
};
