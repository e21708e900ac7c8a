// The host check of a correlated two-qubit Kraus group (AQC_OP_KRAUS2: nk consecutive rows, one 4x4
// operator each), shared by the statevector trajectory engine (traj.hip) and the MPS one
// (mps_traj.hip): both refuse the same programs with the same words, before any device call, and
// take a group's constant weights from the same arithmetic.
#pragma once

#include <cmath>

#include "../../include/aqc_hip.h"

namespace aqc {

// M = K^dag K of a 4x4 operator m (row-major, (re, im) pairs) as the kernels read it: M00 M11 M22 M33,
// then (Re, Im) of M01 M02 M03 M12 M13 M23.
inline void kraus2_weights(const double* m, double* w) {
  // M_st = sum_r conj(K_rs) K_rt; K_rs = m[2 (4 r + s)] + i m[2 (4 r + s) + 1]
  int c = 0;
  for (int s = 0; s < 4; ++s)
    for (int t = s; t < 4; ++t) {
      double x = 0.0, y = 0.0;
      for (int q = 0; q < 4; ++q) {
        const double ar = m[2 * (4 * q + s)], ai = m[2 * (4 * q + s) + 1];
        const double br = m[2 * (4 * q + t)], bi = m[2 * (4 * q + t) + 1];
        x += ar * br + ai * bi;
        y += ar * bi - ai * br;
      }
      if (t == s) {
        w[s] = x;
      } else {
        w[4 + 2 * c] = x, w[5 + 2 * c] = y;
        ++c;
      }
    }
}

// The first row of a group at row i of an nprog-row program on n qubits: null, or what is wrong with it.
inline const char* kraus2_first_row_error(const aqc_op_t& op, int n, int rows_left) {
  const int nk = (op.flags >> 16) & 0xff;
  if (op.flags != (AQC_OP_KRAUS2 | (nk << 16)) || nk < 1 || nk > 16 || nk > rows_left)
    return "malformed Kraus group: its first row needs k = 0 and 1 .. 16 operators within the program";
  if (op.q0 < 0 || op.q0 >= n || op.q1 < 0 || op.q1 >= n || op.q0 == op.q1) return "Kraus group: bad qubits";
  return nullptr;
}

// The nk rows of a group whose first row has passed kraus2_first_row_error: every row's flags and
// qubits, finite entries, M_k = K_k^dag K_k into w[k], sum M_k = I within 1e-9.  *flat: every M_k is a
// multiple of I within 1e-12 (the multiple is w[k][0]).  Null, or what is wrong.
inline const char* kraus2_group_error(const aqc_op_t* ops, int nk, double (*w)[16], bool* flat) {
  double sum[16] = {0.0};
  *flat = true;
  for (int k = 0; k < nk; ++k) {
    const aqc_op_t& op = ops[k];
    if (op.flags != (AQC_OP_KRAUS2 | (k << 8) | (nk << 16)) || op.nq != 2 || op.q0 != ops[0].q0 || op.q1 != ops[0].q1)
      return "malformed Kraus group: rows k = 0 .. nk-1 in order on the same qubits";
    for (int e = 0; e < 32; ++e)
      if (!std::isfinite(op.m[e])) return "malformed Kraus group: a matrix entry is not finite";
    kraus2_weights(op.m, w[k]);
    for (int e = 0; e < 16; ++e) sum[e] += w[k][e];
    for (int s = 0; s < 4; ++s)
      if (std::fabs(w[k][s] - w[k][0]) > 1e-12) *flat = false;
    for (int e = 4; e < 16; ++e)
      if (std::fabs(w[k][e]) > 1e-12) *flat = false;
  }
  for (int e = 0; e < 16; ++e)
    if (std::fabs(sum[e] - (e < 4 ? 1.0 : 0.0)) > 1e-9) return "Kraus group: sum K^dag K is not the identity";
  return nullptr;
}

}  // namespace aqc
