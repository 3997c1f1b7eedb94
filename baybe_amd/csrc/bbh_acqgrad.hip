// qLogEI with its partial derivatives with respect to a candidate's posterior statistics (bbh_qlogei_partials): the value of
// bbh_qlogei_q1 / bbh_qlogei_pending and d A / d (mean_i, var_i, cross_i1 .. cross_ip), for a gradient-based continuous optimiser
// that chains them with bbh_posterior_grad.  On the shared core of the joint q'-batch kernels (bbh_joint.h): Sigma =
// [[v0, c^T], [c, cov_pp]], its factor with the jitter ladder in strided LDS, draws by fma in ascending column order.
//
// Reverse mode through that same computation.  Per sample s, with li_r = log fatplus(t_r), t_r = (sign y_r - best_f) / tau_relu,
// u_r = 2 / (2 + (mx - li_r) / tau_max), fm = mx + tau_max log sum_r u_r^2 and e_s = exp(fm):
//   d fm / d li_r = u_r^3 / sum u^2 + [r = argmax] (1 - sum u^3 / sum u^2),
//   d li_r / d y_r = (sigmoid(t_r) - 0.2 t_r / (1 + t_r^2)^2) / fatplus(t_r) * sign / tau_relu,
// and ybar_r = e_s (d fm / d li_r)(d li_r / d y_r) is accumulated into mbar_0 (r = 0) and Lbar_rc += ybar_r z_sc.  After the
// samples the adjoint of the factor is taken back through the row-by-row Cholesky in reverse order, which leaves
// d / d Sigma_rc in place of Lbar_rc: d / d v0 = Sigmabar_00, d / d cross_r = Sigmabar_r0.  Everything is linear in the
// sample weights e_s, so the sample axis is cut into slices (blockIdx.y) whose partial sums a finishing kernel adds in a fixed
// order and divides by the total weight: no floating-point atomics, a row's result does not depend on N.
#include <math.h>

#include "bbh_common.h"
#include "bbh_acqmath.h"
#include "bbh_joint.h"

#define AG_PIVOT_RTOL 1e-8

__global__ __launch_bounds__(64) void bbh_qlogei_partials_kernel(const double* __restrict__ mean, const double* __restrict__ var,
                                                                 const double* __restrict__ cross, int64_t N, int p,
                                                                 const double* __restrict__ mean_p, const double* __restrict__ cov_pp,
                                                                 const double* __restrict__ z, int S, int per, double best_f, double sign,
                                                                 double* __restrict__ psum, double* __restrict__ ppart,
                                                                 uint8_t* __restrict__ ok_out) {
  extern __shared__ __attribute__((aligned(16))) double ag_lds[];
  const int q = p + 1, nt = q * (q + 1) / 2, np1 = 2 + p;
  double* s_L = ag_lds;            // [nt][64] factor
  double* s_B = s_L + nt * 64;     // [nt][64] its adjoint
  double* s_li = s_B + nt * 64;    // [q][64]  li_r
  double* s_d = s_li + q * 64;     // [q][64]  d li_r / d y_r
  double* s_mp = s_d + q * 64;     // [QMAX]
  double* s_cpp = s_mp + QMAX;     // [p, p]
  const int t = threadIdx.x;
  for (int e = t; e < p; e += 64) s_mp[e] = mean_p[e];
  for (int e = t; e < p * p; e += 64) s_cpp[e] = cov_pp[e];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 64 + t;
  if (i >= N) return;
  const int slice = blockIdx.y;
  double* out = ppart + ((int64_t)slice * N + i) * np1;
  for (int k = 0; k < np1; k++) out[k] = 0.0;
  double* L = s_L + t;
  double* B = s_B + t;
  double* li = s_li + t;
  double* dl = s_d + t;
  const double v0 = var[i], m0 = mean[i];
  double jit = 0.0;
  const bool factored = bbh_joint_factor(L, 64, p, v0, cross + i * p, s_cpp, &jit);
  bool good = factored && jit == 0.0 && v0 > 0.0;  // the derivative is that of the un-jittered computation only
  // ... and of a factor whose pivots are above the rounding of the covariances they are differences of (the posterior covariances
  // carry ~1e-8 relative: tests/test_gpu_parity.py): a candidate that copies a pending point leaves a pivot of either sign at
  // rounding level, which the plain factorisation may accept - its reciprocal would be the whole derivative
  if (good)
    for (int r = 0; r < q; r++) {
      const double srr = (r == 0) ? v0 : s_cpp[(r - 1) * p + (r - 1)];
      const double lrr = L[tri(r, r) * 64];
      if (!(lrr * lrr > AG_PIVOT_RTOL * srr)) good = false;
    }
  if (slice == 0) ok_out[i] = good ? 1 : 0;
  if (!factored) {
    psum[(int64_t)slice * N + i] = NAN;  // not PSD even with jitter 1e-6, as the value kernels score it
    return;
  }
  for (int e = 0; e < nt; e++) B[e * 64] = 0.0;
  const double inv_tau = 1.0 / TAU_RELU;
  double sum = 0.0, mb0 = 0.0;
  const int s0 = slice * per, s1 = (s0 + per < S) ? s0 + per : S;
  for (int s = s0; s < s1; s++) {
    const double* zs = z + (int64_t)s * q;
    double mx = -INFINITY;
    int kstar = 0;
#pragma unroll 1
    for (int r = 0; r < q; r++) {
      const double y = bbh_joint_draw(L, 64, r, (r == 0) ? m0 : s_mp[r - 1], zs);
      const double tt = (sign * y - best_f) * inv_tau;
      const double fp = bbh_fatplus_core(tt);
      const double v = log(fp);  // li_r - log tau_relu: the fat maximum commutes with the shift
      const double et = exp(-fabs(tt));
      const double sg = (tt >= 0.0 ? 1.0 : et) / (1.0 + et);
      const double d2 = fma(tt, tt, 1.0);
      const double dfp = (d2 < INFINITY) ? sg - 0.2 * tt / (d2 * d2) : sg;
      li[r * 64] = v;
      dl[r * 64] = dfp / fp * (sign * inv_tau);
      if (v > mx) {
        mx = v;
        kstar = r;
      }
    }
    double acc = 0.0, acc3 = 0.0;
#pragma unroll 1
    for (int r = 0; r < q; r++) {
      const double u = 2.0 / (2.0 + (mx - li[r * 64]) / TAU_MAX);
      acc = fma(u, u, acc);
      acc3 = fma(u * u, u, acc3);
    }
    const double fm = mx + TAU_MAX * log(acc);
    const double e = exp(fm);
    sum += e;
    if (good) {
#pragma unroll 1
      for (int r = 0; r < q; r++) {
        const double u = 2.0 / (2.0 + (mx - li[r * 64]) / TAU_MAX);
        double dli = u * u * u / acc;
        if (r == kstar) dli += 1.0 - acc3 / acc;
        const double yb = e * dli * dl[r * 64];
        if (r == 0) mb0 += yb;
        for (int c = 0; c <= r; c++) B[tri(r, c) * 64] = fma(yb, zs[c], B[tri(r, c) * 64]);
      }
    }
  }
  psum[(int64_t)slice * N + i] = sum;
  if (!good) return;
  // adjoint of the factorisation: the forward order (r ascending, c ascending) walked backwards
  for (int r = q - 1; r >= 0; r--)
    for (int c = r; c >= 0; c--) {
      double sb;
      if (r == c) {
        sb = B[tri(r, r) * 64] / (2.0 * L[tri(r, r) * 64]);
      } else {
        sb = B[tri(r, c) * 64] / L[tri(c, c) * 64];
        B[tri(c, c) * 64] -= sb * L[tri(r, c) * 64];
      }
      B[tri(r, c) * 64] = sb;
      for (int k = 0; k < c; k++) {
        if (r == c) {
          B[tri(r, k) * 64] -= 2.0 * sb * L[tri(r, k) * 64];
        } else {
          B[tri(r, k) * 64] -= sb * L[tri(c, k) * 64];
          B[tri(c, k) * 64] -= sb * L[tri(r, k) * 64];
        }
      }
    }
  out[0] = mb0;
  out[1] = B[0];
  for (int r = 1; r < q; r++) out[1 + r] = B[tri(r, 0) * 64];
}

__global__ __launch_bounds__(256) void bbh_qlogei_partials_finish_kernel(const double* __restrict__ psum, const double* __restrict__ ppart,
                                                                         int slices, int64_t N, int S, int np1,
                                                                         const uint8_t* __restrict__ ok, double* __restrict__ scores,
                                                                         double* __restrict__ part) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double total = 0.0;
  for (int k = 0; k < slices; k++) total += psum[(int64_t)k * N + i];  // NaN (no positive definite factor) propagates
  scores[i] = LOG_TAU_RELU + log(total) - log((double)S);
  for (int j = 0; j < np1; j++) {
    double g = 0.0;
    for (int k = 0; k < slices; k++) g += ppart[((int64_t)k * N + i) * np1 + j];
    part[i * np1 + j] = ok[i] ? g / total : 0.0;
  }
}

extern "C" int bbh_qlogei_partials(bbh_handle* h, const double* mean_dev, const double* var_dev, const double* cross_dev, int64_t N,
                                   const double* z_host, int64_t S, double best_f, double sign, double* scores_dev, double* part_dev,
                                   uint8_t* ok_dev) {
  if (!h) return -1;
  const int p = h->p;
  if (!mean_dev || !var_dev || (p > 0 && !cross_dev) || !z_host || !scores_dev || !part_dev || !ok_dev || N < 0 || S < 1 || S > 8192 ||
      p > BBH_MAX_PENDING) {
    h->err = "bbh_qlogei_partials: bad arguments (every output, 1 <= S <= 8192, cross_dev unless no pending point is set)";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  const double none = 0.0;
  bbh_joint_dev d;
  int rc = bbh_upload_joint(h, z_host, S, p, p ? h->pend_mean.data() : &none, p ? h->pend_cov.data() : &none, false, &d);
  if (rc) return rc;
  // slices of the sample axis: a function of S alone, so that a row's bits do not depend on the candidate count
  int slices = (int)((S + 7) / 8);
  if (slices > 32) slices = 32;
  const int per = (int)((S + slices - 1) / slices);
  slices = (int)((S + per - 1) / per);
  const int q = p + 1, np1 = 2 + p;
  rc = bbh_ensure_ws(h, sizeof(double) * (size_t)slices * (size_t)N * (size_t)(1 + np1));
  if (rc) return rc;
  double* psum = h->d_ws;
  double* ppart = psum + (size_t)slices * N;
  const size_t lds = sizeof(double) * ((size_t)64 * (q * (q + 1) + 2 * q) + QMAX + (size_t)p * p);
  if (lds > h->lds_per_block) {
    h->err = "bbh_qlogei_partials: the factor and its adjoint do not fit the device's LDS";
    return -1;
  }
  BBH_HIP_TRY(h, bbh_allow_lds(h->device, (const void*)bbh_qlogei_partials_kernel, lds));
  hipLaunchKernelGGL(bbh_qlogei_partials_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)slices), dim3(64), lds, h->stream, mean_dev,
                     var_dev, cross_dev, N, p, d.mean_p, d.cov_pp, d.z, (int)S, per, best_f, sign, psum, ppart, ok_dev);
  hipLaunchKernelGGL(bbh_qlogei_partials_finish_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, psum, ppart, slices, N,
                     (int)S, np1, ok_dev, scores_dev, part_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}
