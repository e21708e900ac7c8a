// The pair readout both noisy tomography entries share (traj.hip: k_sv_traj's pair ending; mps_traj.hip:
// k_mps_traj_pair_draw), and the host check of the effects table they take.
#pragma once

#include <cmath>
#include <string>

#include "aqc_internal.h"

namespace aqc {

// entry (r, c) of the Hermitian 2x2 effect e = (E00, E11, Re E01, Im E01)
__device__ __forceinline__ cplx effect_entry(const double* e, int r, int c) {
  if (r == c) return cmk(e[r], 0.0);
  return cmk(e[2], r < c ? e[3] : -e[3]);
}

// One outcome o = 2 o_hi + o_lo of a pair in one setting.  The pair's 4x4 RDM (index 2 bit_hi + bit_lo)
// comes as its diagonal d[s] = rho_ss and its upper triangle (ox, oy)[c] = rho_st, s < t in row order;
// eh / el: the two effects (4 doubles each) of the hi / lo qubit in the setting's bases.
// p_o = max(0, Re Tr[(eh[o_hi] (x) el[o_lo]) rho]), summed in a fixed order; then aqc_multinomial_counts'
// rule: the smallest o with C_o > uu P, else the last o with p_o > 0.
__device__ __forceinline__ int pair_outcome(const double* eh, const double* el, const double* d, const double* ox,
                                            const double* oy, double uu) {
  double pk[4], P = 0.0;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const double* A = eh + 4 * (o >> 1);
    const double* B = el + 4 * (o & 1);
    // Tr(E rho) = sum_s E_ss rho_ss + 2 Re sum_{s<t} E_st conj(rho_st), E = A (x) B
    double acc = 0.0;
    int c = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      acc += A[s >> 1] * B[s & 1] * d[s];
#pragma unroll
      for (int t = s + 1; t < 4; ++t, ++c) {
        const cplx e = cmul(effect_entry(A, s >> 1, t >> 1), effect_entry(B, s & 1, t & 1));
        acc += 2.0 * (e.x * ox[c] + e.y * oy[c]);
      }
    }
    pk[o] = fmax(0.0, acc);
    P += pk[o];
  }
  const double target = uu * P;
  int k = -1, lastnz = 0;
  double c = 0.0;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    c += pk[o];
    if (pk[o] > 0.0) lastnz = o;
    if (k < 0 && c > target) k = o;
  }
  return k < 0 ? lastnz : k;
}

// The Hermitian 2x2 effects [n][3][2][4]: finite, E0 + E1 = I within 1e-9, each PSD within 1e-12.
// `entry` names the calling entry point in the error message.
inline int check_effects(int n, const double* effects, const char* entry) {
  auto fail = [&](const char* msg) {
    set_error(std::string(entry) + ": " + msg);
    return AQC_ERR_ARG;
  };
  for (int qb = 0; qb < n * 3; ++qb) {
    const double* e0 = effects + (size_t)qb * 8;
    const double* e1 = e0 + 4;
    for (int c = 0; c < 8; ++c)
      if (!std::isfinite(e0[c])) return fail("an effect is not finite");
    if (std::fabs(e0[0] + e1[0] - 1.0) > 1e-9 || std::fabs(e0[1] + e1[1] - 1.0) > 1e-9 ||
        std::fabs(e0[2] + e1[2]) > 1e-9 || std::fabs(e0[3] + e1[3]) > 1e-9)
      return fail("the two effects of a qubit and basis do not sum to the identity");
    for (const double* e : {e0, e1}) {
      const double half_gap = std::hypot(0.5 * (e[0] - e[1]), std::hypot(e[2], e[3]));
      if (0.5 * (e[0] + e[1]) - half_gap < -1e-12) return fail("an effect is not positive semidefinite");
    }
  }
  return AQC_OK;
}

}  // namespace aqc
