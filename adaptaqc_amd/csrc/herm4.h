// 4x4 Hermitian eigensolver shared by the entanglement measures (ent.hip) and the tomography fit
// (tomo.hip).
#pragma once

#include "aqc_internal.h"

namespace aqc {

// Cyclic complex Jacobi on a 4x4 Hermitian matrix: eigenvalues in ev, eigenvectors (columns)
// in V when want_v.
__device__ inline void herm4_eig(cplx H[4][4], double ev[4], cplx V[4][4], bool want_v) {
  if (want_v)
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) V[r][c] = aqc::cmk(r == c ? 1.0 : 0.0, 0.0);
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0, dia = 0;
    for (int p = 0; p < 4; ++p) {
      dia += H[p][p].x * H[p][p].x;
      for (int q = p + 1; q < 4; ++q) off += aqc::cnorm2(H[p][q]);
    }
    if (off <= 1e-34 * (dia + 1e-300)) break;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double g = sqrt(aqc::cnorm2(H[p][q]));
        if (g == 0.0) continue;
        const cplx e = aqc::cmk(H[p][q].x / g, H[p][q].y / g);  // phase of H[p][q]
        const double tau = (H[q][q].x - H[p][p].x) / (2.0 * g);
        const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double c = 1.0 / sqrt(1.0 + t * t), sn = t * c;
        // J = [[c, s], [-s conj(e), c conj(e)]] on (p, q): H <- J^H H J, V <- V J
        const cplx ec = aqc::cconj(e);
        for (int k = 0; k < 4; ++k) {  // columns
          const cplx hp = H[k][p], hq = H[k][q];
          H[k][p] = aqc::csub(aqc::cscale(hp, c), aqc::cscale(aqc::cmul(hq, ec), sn));
          H[k][q] = aqc::cadd(aqc::cscale(hp, sn), aqc::cscale(aqc::cmul(hq, ec), c));
        }
        for (int k = 0; k < 4; ++k) {  // rows (conjugate transpose of the column update)
          const cplx hp = H[p][k], hq = H[q][k];
          H[p][k] = aqc::csub(aqc::cscale(hp, c), aqc::cscale(aqc::cmul(hq, e), sn));
          H[q][k] = aqc::cadd(aqc::cscale(hp, sn), aqc::cscale(aqc::cmul(hq, e), c));
        }
        H[p][q] = aqc::cmk(0, 0);
        H[q][p] = aqc::cmk(0, 0);
        if (want_v)
          for (int k = 0; k < 4; ++k) {
            const cplx vp = V[k][p], vq = V[k][q];
            V[k][p] = aqc::csub(aqc::cscale(vp, c), aqc::cscale(aqc::cmul(vq, ec), sn));
            V[k][q] = aqc::cadd(aqc::cscale(vp, sn), aqc::cscale(aqc::cmul(vq, ec), c));
          }
      }
  }
  for (int p = 0; p < 4; ++p) ev[p] = H[p][p].x;
}

}  // namespace aqc
