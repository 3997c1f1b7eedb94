// Shared core of the joint q'-batch acquisition kernels (bbh_acq.hip, bbh_objacq.hip) for a factor in strided memory, and the
// one upload their launches share.
#pragma once
#include <string.h>

#include <vector>

#include "bbh_common.h"

// ---- shared core of the joint q'-batch kernels ----------------------------------------------------------------------------
// q' = 1 + p points: the candidate, then the p pending points.  Per candidate: Sigma = [[v0, c^T], [c, cov_pp]] (v0 = var[i],
// c = cross[i p ...]), its Cholesky factor with exact psd_safe_cholesky semantics - diagonal jitter 0, 1e-8, 1e-7, 1e-6, a pivot
// !(s > 0) ends an attempt, no factor after the fourth (gpytorch raises NotPSDError; the kernels score NaN) - and per base sample
// the draw y_r = m_r + sum_c L_rc z_c.  The factor is thread-private, packed lower-triangular (element (r, c) at tri(r, c)), and
// these three pieces are written once per storage class:
//   strided memory, run-time q'  element e at L[e * stride]: stride 64 in LDS (bbh_qlogei_pending_kernel, bbh_mc_pending_kernel),
//                                stride N in a global workspace (bbh_qlogei_pending_big_kernel); a failed pivot breaks out
//   registers, template <int Q>  every index a compile-time constant (bbh_qlogei_pending_q_kernel, bbh_mc_pending_q_kernel);
//                                a failed pivot lets the attempt run on and discards it
// Both factor row by row with the k loop subtracting in ascending order, and draw by fma in ascending c from the mean.
#define QMAX 16
#define QTRI (QMAX * (QMAX + 1) / 2)
__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }

template <typename ST>  // ST: type of the stride (int 64, int64_t N)
__device__ __forceinline__ bool bbh_joint_factor(double* L, ST stride, int p, double v0, const double* cross_i, const double* cov_pp,
                                                 double* jitter_used = nullptr) {  // jitter_used: the diagonal jitter of the last attempt
  const int q = p + 1;
  double jitter = 0.0;
  bool ok = false;
  for (int attempt = 0; attempt < 4 && !ok; attempt++) {
    ok = true;
    for (int r = 0; r < q && ok; r++) {
      for (int c = 0; c <= r; c++) {
        double s;
        if (r == 0)
          s = v0;
        else if (c == 0)
          s = cross_i[r - 1];
        else
          s = cov_pp[(r - 1) * p + (c - 1)];
        if (r == c) s += jitter;
        for (int k = 0; k < c; k++) s -= L[tri(r, k) * stride] * L[tri(c, k) * stride];
        if (r == c) {
          if (!(s > 0.0)) {
            ok = false;
            break;
          }
          L[tri(r, r) * stride] = sqrt(s);
        } else {
          L[tri(r, c) * stride] = s / L[tri(c, c) * stride];
        }
      }
    }
    if (jitter_used) *jitter_used = jitter;
    if (!ok) jitter = 1e-8 * pow(10.0, (double)attempt);
  }
  return ok;
}

template <typename ST>
__device__ __forceinline__ double bbh_joint_draw(const double* L, ST stride, int r, double m, const double* zs) {
  double y = m;
  for (int c = 0; c <= r; c++) y = fma(L[tri(r, c) * stride], zs[c], y);
  return y;
}

// One upload per joint launch: [z [S, q'] | zbar [q'] (column means of z: the MC family only) | mean_p [p] | cov_pp [p, p]]
struct bbh_joint_dev {
  const double *z, *zbar, *mean_p, *cov_pp;
  size_t bytes;  // of the whole upload
};
static inline int bbh_upload_joint(bbh_handle* h, const double* z_host, int64_t S, int64_t p, const double* mp_host, const double* cpp_host,
                            bool with_zbar, bbh_joint_dev* d) {
  const int64_t q = p + 1, nzb = with_zbar ? q : 0;
  std::vector<double> buf((size_t)S * q + nzb + p + (size_t)p * p, 0.0);
  memcpy(buf.data(), z_host, sizeof(double) * S * q);
  double* zb = buf.data() + S * q;
  if (with_zbar) {
    for (int64_t s = 0; s < S; s++)
      for (int c = 0; c < q; c++) zb[c] += z_host[s * q + c];
    for (int c = 0; c < q; c++) zb[c] /= (double)S;
  }
  memcpy(zb + nzb, mp_host, sizeof(double) * p);
  memcpy(zb + nzb + p, cpp_host, sizeof(double) * p * p);
  const int rc = bbh_upload_z(h, buf.data(), buf.size());
  if (rc) return rc;
  d->z = h->d_z;
  d->zbar = with_zbar ? d->z + S * q : nullptr;
  d->mean_p = d->z + S * q + nzb;
  d->cov_pp = d->mean_p + p;
  d->bytes = sizeof(double) * buf.size();
  return 0;
}

