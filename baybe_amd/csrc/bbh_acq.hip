// Monte-Carlo acquisition (qLogEI) and selection kernels.
//
// qLogExpectedImprovement as BayBE builds it (baybe/acquisition/acqfs.py:219-223,
// baybe/acquisition/_builder.py:195-265): fat=True, tau_relu=1e-6, tau_max=1e-2, Sobol-normal
// base samples shared by all candidates; objective = sign * sample (minimisation = -1,
// baybe/objectives/base.py:99-105).  Maths restated in oracle/gp_oracle.py (log_fatplus, fatmax,
// logmeanexp, psd_safe_cholesky jitter).
//
// The kernels that score a candidate jointly with p pending points (bbh_qlogei_pending_q_kernel, bbh_qlogei_pending_kernel,
// bbh_qlogei_pending_big_kernel, bbh_mc_pending_q_kernel, bbh_mc_pending_kernel) share one core, "shared core of the joint
// q'-batch kernels" (strided form: bbh_joint.h, also under bbh_objacq.hip; register form: below): Sigma = [[v0, c^T], [c, cov_pp]], its Cholesky factor with the jitter ladder, and the draw
// y = m + L z, once for a factor in strided memory (LDS or the global workspace) and once for a factor in registers.  A kernel
// adds its storage and its utility; the host side shares the upload, the 60 KB rule and the Q = 2 ... 14 dispatch.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "bbh_common.h"
#include "bbh_acqmath.h"  // TAU_RELU, TAU_MAX, bbh_fatplus_core, bbh_safe_sd
#include "bbh_slices.h"   // sample slices of bbh_qlogei_pending_q_kernel: bounds, finish

#ifndef BBH_PENDING_PK
#define BBH_PENDING_PK 1  // (with BBH_PENDING_FAST) the u_r^2 terms of the fat maximum in packed single precision, two points at a time
#endif
#ifndef BBH_PENDING_FAST
#define BBH_PENDING_FAST 1  // joint q'-batch qLogEI kernels: reduced-precision logarithms where the power tau_max = 0.01 absorbs them
#endif

// q' = 1:  score = log( mean_s fatplus(sign (mu + sd z_s) - best_f) )
//               = logmeanexp_s log_fatplus(...)   (all terms positive, no cancellation)
__global__ __launch_bounds__(256) void bbh_qlogei_q1_kernel(const double* __restrict__ mean,
                                                            const double* __restrict__ var, int64_t N,
                                                            const double* __restrict__ z, int S, double best_f,
                                                            double sign, const uint8_t* __restrict__ alive,
                                                            double* __restrict__ scores) {
  extern __shared__ double s_z[];
  for (int s = threadIdx.x; s < S; s += blockDim.x) s_z[s] = z[s];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if (alive && !alive[i]) {
    scores[i] = -INFINITY;
    return;
  }
  const double inv_tau = 1.0 / TAU_RELU;
  const double a = (sign * mean[i] - best_f) * inv_tau;
  const double b = sign * bbh_safe_sd(var[i]) * inv_tau;
  // four independent partial sums: the per-sample chain (fma, compare, reciprocal seed, two Newton steps) is ~10
  // dependent instructions; one accumulator left the kernel latency-bound at half the VALU rate (0.34 ms per 1e6 x 512)
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int s = 0;
  for (; s + 3 < S; s += 4) {
    s0 += bbh_fatplus_core<1>(fma(b, s_z[s], a));
    s1 += bbh_fatplus_core<1>(fma(b, s_z[s + 1], a));
    s2 += bbh_fatplus_core<1>(fma(b, s_z[s + 2], a));
    s3 += bbh_fatplus_core<1>(fma(b, s_z[s + 3], a));
  }
  for (; s < S; s++) s0 += bbh_fatplus_core<1>(fma(b, s_z[s], a));
  const double sum = (s0 + s1) + (s2 + s3);
  scores[i] = LOG_TAU_RELU + log(sum) - log((double)S);
}

#include "bbh_joint.h"  // shared core of the joint q'-batch kernels: QMAX, tri, bbh_joint_factor, bbh_joint_draw, bbh_upload_joint

// qLogEI of one candidate from its strided factor: per sample li_r = log_fatplus(sign y_r - best_f), the fat maximum over the q'
// points, a streaming log-sum-exp over the samples.  li: q' doubles of this thread, element r at li[r * li_stride].
template <typename ST>
__device__ __forceinline__ double bbh_qlogei_joint_lse(const double* L, ST stride, int q, double m0, const double* mean_p,
                                                       const double* z, int S, double best_f, double sign, double* li,
                                                       int li_stride) {
  const double inv_tau = 1.0 / TAU_RELU;
  double sum = 0.0;  // sum_s exp(fatmax_s - ref)
  double ref = -INFINITY;
  for (int s = 0; s < S; s++) {
    const double* zs = z + (int64_t)s * q;
    double mx = -INFINITY;
#pragma unroll 1
    for (int r = 0; r < q; r++) {
      const double y = bbh_joint_draw(L, stride, r, (r == 0) ? m0 : mean_p[r - 1], zs);
      const double tt = (sign * y - best_f) * inv_tau;
      const double v = LOG_TAU_RELU + log(bbh_fatplus_core(tt));
      li[r * li_stride] = v;
      mx = fmax(mx, v);
    }
    // fatmax over the q' points: mx + tau log sum_j (2 / (2 + (mx - li_j)/tau))^2
    double acc = 0.0;
#pragma unroll 1
    for (int r = 0; r < q; r++) {
      const double u = 2.0 / (2.0 + (mx - li[r * li_stride]) / TAU_MAX);
      acc = fma(u, u, acc);
    }
    const double fm = mx + TAU_MAX * log(acc);
    if (fm > ref) {
      sum = sum * exp(ref - fm) + 1.0;
      ref = fm;
    } else {
      sum += exp(fm - ref);
    }
  }
  return ref + log(sum) - log((double)S);
}

template <int Q>
__device__ __forceinline__ void bbh_joint_load_q(double (&A)[Q * (Q + 1) / 2], double v0, const double* cross_i, const double* s_cpp) {
  constexpr int P = Q - 1;
  A[0] = v0;  // lower triangle of Sigma
#pragma unroll
  for (int r = 1; r < Q; r++) {
    A[r * (r + 1) / 2] = cross_i[r - 1];
#pragma unroll
    for (int c = 1; c <= r; c++) A[r * (r + 1) / 2 + c] = s_cpp[(r - 1) * P + (c - 1)];
  }
}

template <int Q>
__device__ __forceinline__ bool bbh_joint_factor_q(const double (&A)[Q * (Q + 1) / 2], double (&L)[Q * (Q + 1) / 2]) {
  double jitter = 0.0;
  bool ok = false;
  for (int attempt = 0; attempt < 4 && !ok; attempt++) {
    ok = true;
#pragma unroll
    for (int r = 0; r < Q; r++) {
#pragma unroll
      for (int c = 0; c <= r; c++) {
        double sacc = A[r * (r + 1) / 2 + c];
        if (r == c) sacc += jitter;
#pragma unroll
        for (int k = 0; k < c; k++) sacc -= L[r * (r + 1) / 2 + k] * L[c * (c + 1) / 2 + k];
        if (r == c) {
          if (!(sacc > 0.0)) ok = false;  // the rest of this attempt is discarded (values may be NaN)
          L[r * (r + 1) / 2 + r] = sqrt(sacc);
        } else {
          L[r * (r + 1) / 2 + c] = sacc / L[c * (c + 1) / 2 + c];
        }
      }
    }
    if (!ok) jitter = 1e-8 * pow(10.0, (double)attempt);
  }
  return ok;
}

template <int Q>
__device__ __forceinline__ void bbh_joint_draw_q(const double (&L)[Q * (Q + 1) / 2], const double (&m)[Q], const double* zs,
                                                 double (&y)[Q]) {
  double zr[Q];
#pragma unroll
  for (int c = 0; c < Q; c++) zr[c] = zs[c];
#pragma unroll
  for (int r = 0; r < Q; r++) {
    y[r] = m[r];
#pragma unroll
    for (int c = 0; c <= r; c++) y[r] = fma(L[r * (r + 1) / 2 + c], zr[c], y[r]);
  }
}

// q' <= 16: the factor in LDS (element e of thread t at s_L[e * 64 + t]), log-domain streaming form.
__global__ __launch_bounds__(64) void bbh_qlogei_pending_kernel(
    const double* __restrict__ mean, const double* __restrict__ var, const double* __restrict__ cross, int64_t N, int p,
    const double* __restrict__ mean_p, const double* __restrict__ cov_pp, const double* __restrict__ z, int S,
    double best_f, double sign, const uint8_t* __restrict__ alive, double* __restrict__ scores) {
  __shared__ double s_L[QTRI * 64];
  __shared__ double s_mp[QMAX];
  __shared__ double s_cpp[QMAX * QMAX];
  const int t = threadIdx.x;
  for (int e = t; e < p; e += 64) s_mp[e] = mean_p[e];
  for (int e = t; e < p * p; e += 64) s_cpp[e] = cov_pp[e];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 64 + t;
  if (i >= N) return;
  if (alive && !alive[i]) {
    scores[i] = -INFINITY;
    return;
  }
  double* L = s_L + t;
  double li[QMAX];
  if (!bbh_joint_factor(L, 64, p, var[i], cross + i * p, s_cpp)) {
    scores[i] = NAN;  // not PSD even with jitter 1e-6
    return;
  }
  scores[i] = bbh_qlogei_joint_lse(L, 64, p + 1, mean[i], s_mp, z, S, best_f, sign, li, 1);
}

// Register-resident form of bbh_qlogei_pending_kernel for q' = Q <= 14 (208 VGPRs at Q = 8, 2 waves per SIMD from Q = 9,
// 1 from Q = 10; no spills up to Q = 13, Q = 14 reports 4 spilled VGPRs and no scratch memory: .vgpr_spill_count 4,
// .private_segment_fixed_size 0; Q = 15, 16 spill further and run no faster than the LDS form): the packed Cholesky
// factor (Q (Q + 1) / 2 doubles) and the per-sample values live in registers (every index is a
// compile-time constant), the base samples z [S, Q] in LDS (broadcast reads).  The LDS form needs 69 KB
// per 64 threads - one wave per two SIMDs - and took 30 ms per greedy step on 1e6 candidates, six times the
// fused posterior; this one runs 256-thread workgroups at full occupancy.  The factorisation (operation order
// included) is that of the LDS form; the per-sample arithmetic is not since the reduced-precision fat maximum and the
// linear-domain sum below: the two forms agree to 2.1e-9 in the score over tests/test_joint_batch_gpu.py (Q = 2, 7, 14 under
// BBH_PENDING_LDS=1 and the 60 KB hand-over at Q = 14), the LDS form within 3e-11 of the oracle and this one within 2.1e-9
// (tolerance 1e-8; profiles/joint_batch_observed_deviations.json).
// SAMPLE SLICES (gridDim.y > 1, linear-domain form only): blockIdx.y takes the samples [y per, (y + 1) per) and writes the partial sum
// of its terms to partial[y][i]; bbh_slices_finish_kernel (bbh_slices.h) adds the slices in a fixed order and takes the logarithm.  With one
// thread per candidate a 1e5-row candidate set is 1563 wavefronts, 1.5 per SIMD, each one long dependent chain: the slices bring
// the launch to the occupancy a 1e6-row set has (the joint Cholesky factor is recomputed per slice: Q^3 / 3 flops against
// per x Q x 40).
template <int Q>
__global__ __launch_bounds__(256) void bbh_qlogei_pending_q_kernel(
    const double* __restrict__ mean, const double* __restrict__ var, const double* __restrict__ cross, int64_t N,
    const double* __restrict__ mean_p, const double* __restrict__ cov_pp, const double* __restrict__ z, int S_total,
    double best_f, double sign, const uint8_t* __restrict__ alive, double* __restrict__ scores, double* __restrict__ partial) {
  extern __shared__ double s_zq[];  // [S * Q] base samples of this slice, then mean_p [Q - 1], cov_pp [(Q - 1)^2]
  constexpr int P = Q - 1;
  const int per = bbh_slice_per(S_total);
  const bbh_slice sl = bbh_slice_bounds(S_total, per, (int)blockIdx.y);
  const int S = sl.count;  // samples of this slice
  z += (int64_t)sl.begin * Q;
  if (partial) scores = partial + (int64_t)blockIdx.y * N;
  double* s_mp = s_zq + (int64_t)per * Q;
  double* s_cpp = s_mp + P;
  for (int e = threadIdx.x; e < S * Q; e += 256) s_zq[e] = z[e];
  for (int e = threadIdx.x; e < P; e += 256) s_mp[e] = mean_p[e];
  for (int e = threadIdx.x; e < P * P; e += 256) s_cpp[e] = cov_pp[e];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  if (alive && !alive[i]) {
    scores[i] = partial ? 0.0 : -INFINITY;
    return;
  }
  double L[Q * (Q + 1) / 2], A[Q * (Q + 1) / 2];
  bbh_joint_load_q<Q>(A, var[i], cross + i * P, s_cpp);
  if (!bbh_joint_factor_q<Q>(A, L)) {
    scores[i] = NAN;  // not PSD even with jitter 1e-6 (gpytorch raises NotPSDError)
    return;
  }
  double m[Q];
  m[0] = mean[i];
#pragma unroll
  for (int r = 1; r < Q; r++) m[r] = s_mp[r - 1];
  const double inv_tau = 1.0 / TAU_RELU;
  // exp(fatmax_s) = exp(mx_s) acc_s^tau_max with exp(mx_s) = tau_relu max_r fatplus_core(t_sr): the per-sample
  // exponential of the streaming log-sum-exp and the logarithm of the largest term are not needed.  The terms
  // tau_relu^-1 exp(fatmax_s) lie in [1e-41, 1e7) for every reachable t, so the plain sum neither overflows nor
  // loses its smallest terms to underflow (the streaming form is bbh_qlogei_pending_kernel: BBH_PENDING_LDS=1).
  double sum = 0.0;
  for (int s = 0; s < S; s++) {
    double y[Q], fp[Q];
    bbh_joint_draw_q<Q>(L, m, s_zq + (int64_t)s * Q, y);
    double fmx = 0.0;
#if BBH_PENDING_FAST
    // exp(fatmax_s) / tau_relu = fmx acc^tau_max with fmx = max_r fatplus(t_sr) and acc = sum_r u_r^2, u_r = 2 tau / (2 tau + D_r),
    // D_r = log(fmx / fatplus(t_sr)) >= 0.  fmx enters linearly and is kept to full precision, but acc enters through the power
    // tau_max = 0.01: an absolute error of 1e-7 in u_r^2 changes the sample's term by 1e-9 relative.  So D_r never needs a
    // double-precision logarithm:  rho = fatplus_r / fmx, x = 1 - rho;  x < 0.15: D = -log1p(-x) = x + x^2/2 + ... + x^7/7
    // (truncation 3e-8 at the edge, where u = 0.11 and du^2/dD = 100 u^3 = 0.13);  otherwise D = -ln 2 log2f(rho) in single
    // precision (error ~1e-7; rho below the float range gives D = inf, u = 0: u^2 < 6e-8 there anyway).  The reciprocal is the
    // bare v_rcp_f64 seed (2^-26), log(acc) for acc in [1, Q] single precision as well.  Per sample and point ~33 instead of
    // ~55 VALU instructions, per sample 13 instead of 34 (BBH_PENDING_FAST=0 at compile time restores the former sequence).
#pragma unroll
    for (int r = 0; r < Q; r++) {
      fp[r] = bbh_fatplus_core<1>((sign * y[r] - best_f) * inv_tau);
      fmx = fmax(fmx, fp[r]);
    }
#if BBH_PENDING_PK
    // The same in packed single precision, two points per instruction: rho_r = fp_r / fmx and x_r = (fmx - fp_r) / fmx as two
    // single-precision quotients (the difference in double precision: exact next to rho = 1, where u^2 is sensitive) sharing one
    // v_rcp_f32; series, log2, reciprocal and square on float2 values.  u^2 <= 1 to ~1e-7 relative: 1e-9 in the sample's term.
    const float rcf = __builtin_amdgcn_rcpf((float)fmx);
    bbh_f2 accp = {0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < Q; r += 2) {
      const int r1 = (r + 1 < Q) ? r + 1 : r;
      bbh_f2 x, rho;
      x.x = (float)(fmx - fp[r]);
      x.y = (float)(fmx - fp[r1]);
      rho.x = (float)fp[r];
      rho.y = (float)fp[r1];
      x = x * rcf;
      rho = rho * rcf;
      bbh_f2 ds = x * (1.0f / 7.0f) + (1.0f / 6.0f);
      ds = ds * x + 0.2f;
      ds = ds * x + 0.25f;
      ds = ds * x + (1.0f / 3.0f);
      ds = ds * x + 0.5f;
      ds = ds * x + 1.0f;
      ds = ds * x;
      bbh_f2 den;
      den.x = ((x.x < 0.15f) ? ds.x : -0.6931471805599453f * __log2f(rho.x)) + (float)(2.0 * TAU_MAX);
      den.y = ((x.y < 0.15f) ? ds.y : -0.6931471805599453f * __log2f(rho.y)) + (float)(2.0 * TAU_MAX);
      bbh_f2 u;
      u.x = __builtin_amdgcn_rcpf(den.x);  // den = inf (rho below the float range) -> 0
      u.y = (r + 1 < Q) ? __builtin_amdgcn_rcpf(den.y) : 0.0f;  // odd Q: the last point's twin does not count
      u = u * (float)(2.0 * TAU_MAX);
      accp = u * u + accp;
    }
    const float accf = accp.x + accp.y;
    const double w = (TAU_MAX * 0.6931471805599453) * (double)__log2f(accf);
#else
    double inv = __builtin_amdgcn_rcp(fmx);
    inv = fma(fma(-fmx, inv, 1.0), inv, inv);
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < Q; r++) {
      const double rho = fp[r] * inv;
      const double x = 1.0 - rho;
      double ds = fma(x, 1.0 / 7.0, 1.0 / 6.0);
      ds = fma(ds, x, 0.2);
      ds = fma(ds, x, 0.25);
      ds = fma(ds, x, 1.0 / 3.0);
      ds = fma(ds, x, 0.5);
      ds = fma(ds, x, 1.0);
      ds *= x;
      const double dl = -0.6931471805599453 * (double)__log2f((float)rho);
      const double dd = (x < 0.15) ? ds : dl;
      const double u = (2.0 * TAU_MAX) * __builtin_amdgcn_rcp(2.0 * TAU_MAX + dd);  // dd = inf -> 0
      acc = fma(u, u, acc);
    }
    const double w = (TAU_MAX * 0.6931471805599453) * (double)__log2f((float)acc);
#endif
    // acc in [1, Q]: acc^0.01 = exp(w), w = 0.01 ln acc in [0, 0.028): Taylor to the 5th power (7e-13 at w = 0.028)
    double e = fma(w, 1.0 / 120.0, 1.0 / 24.0);
    e = fma(e, w, 1.0 / 6.0);
    e = fma(e, w, 0.5);
    e = fma(e, w, 1.0);
    e = fma(e, w, 1.0);
#else
    double li[Q];
#pragma unroll
    for (int r = 0; r < Q; r++) {
      fp[r] = bbh_fatplus_core((sign * y[r] - best_f) * inv_tau);
      fmx = fmax(fmx, fp[r]);
    }
    double mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < Q; r++) {
      li[r] = bbh_fast_log_pos(fp[r]);
      mx = fmax(mx, li[r]);
    }
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < Q; r++) {
      const double u = (2.0 * TAU_MAX) * bbh_fast_recip(2.0 * TAU_MAX + (mx - li[r]));
      acc = fma(u, u, acc);
    }
    // acc in [1, Q]: acc^0.01 = exp(0.01 log acc), argument in [0, 0.021) - Taylor to the 6th power (1e-17)
    const double w = TAU_MAX * bbh_fast_log_pos(acc);
    double e = fma(w, 1.0 / 720.0, 1.0 / 120.0);
    e = fma(e, w, 1.0 / 24.0);
    e = fma(e, w, 1.0 / 6.0);
    e = fma(e, w, 0.5);
    e = fma(e, w, 1.0);
    e = fma(e, w, 1.0);
#endif
    sum = fma(fmx, e, sum);
  }
  scores[i] = partial ? sum : LOG_TAU_RELU + log(sum) - log((double)S_total);
}

template <int Q>
static void bbh_launch_pending_q(bbh_handle* h, const double* mean, const double* var, const double* cross, int64_t N,
                                 const double* mp, const double* cpp, const double* z, int S, double best_f, double sign,
                                 const uint8_t* alive, double* scores, int slices) {
  double* partial = slices > 1 ? h->d_ws : nullptr;
  const int per = bbh_slices_by_count(S, slices).per;
  const size_t lds = sizeof(double) * ((size_t)per * Q + (Q - 1) + (size_t)(Q - 1) * (Q - 1));
  hipLaunchKernelGGL((bbh_qlogei_pending_q_kernel<Q>), dim3((unsigned)((N + 255) / 256), (unsigned)slices), dim3(256), lds, h->stream, mean,
                     var, cross, N, mp, cpp, z, S, best_f, sign, alive, scores, partial);
  if (slices > 1) bbh_slices_finish<BBH_FINISH_LOG_TAU_MEAN>(h, partial, slices, 1, N, S, alive, scores);  // NaN (no positive definite factor) propagates
}

// ---- first-index argmax -----------------------------------------------------------------------
__device__ __forceinline__ void amax_combine(double& v, int64_t& i, double ov, int64_t oi) {
  // NaN never wins; ties -> lower index
  const bool better = (ov > v) || (ov == v && oi < i) || (i < 0 && oi >= 0);
  if (oi >= 0 && better) {
    v = ov;
    i = oi;
  }
}

__global__ __launch_bounds__(256) void bbh_argmax_stage1(const double* __restrict__ scores, int64_t N,
                                                         double* __restrict__ pv, int64_t* __restrict__ pi) {
  __shared__ double sv[4];
  __shared__ int64_t si[4];
  double v = -INFINITY;
  int64_t idx = -1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const double x = scores[i];
    if (x == x) amax_combine(v, idx, x, i);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_down(v, o, 64);
    const int64_t oi = __shfl_down(idx, o, 64);
    amax_combine(v, idx, ov, oi);
  }
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = v;
    si[threadIdx.x >> 6] = idx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) amax_combine(v, idx, sv[w], si[w]);
    pv[blockIdx.x] = v;
    pi[blockIdx.x] = idx;
  }
}

__global__ __launch_bounds__(256) void bbh_argmax_stage2(const double* __restrict__ pv, const int64_t* __restrict__ pi,
                                                         int nblocks, double* __restrict__ outv,
                                                         int64_t* __restrict__ outi) {
  __shared__ double sv[4];
  __shared__ int64_t si[4];
  double v = -INFINITY;
  int64_t idx = -1;
  for (int b = threadIdx.x; b < nblocks; b += 256) amax_combine(v, idx, pv[b], pi[b]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_down(v, o, 64);
    const int64_t oi = __shfl_down(idx, o, 64);
    amax_combine(v, idx, ov, oi);
  }
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = v;
    si[threadIdx.x >> 6] = idx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) amax_combine(v, idx, sv[w], si[w]);
    *outv = v;
    *outi = idx;
  }
}

__global__ void bbh_mask_one_kernel(double* scores, const int64_t* idx) {
  if (*idx >= 0) scores[*idx] = -INFINITY;
}

#define ARGMAX_BLOCKS 1024

static int bbh_ensure_red(bbh_handle* h) {
  if (!h->d_red) BBH_HIP_TRY(h, hipMalloc((void**)&h->d_red, sizeof(double) * (ARGMAX_BLOCKS + 64)));
  if (!h->d_redi) BBH_HIP_TRY(h, hipMalloc((void**)&h->d_redi, sizeof(int64_t) * (ARGMAX_BLOCKS + 64)));
  return 0;
}

// The handle's pinned staging buffer: at least `bytes` large and no longer read by an earlier staged copy.  The caller fills it,
// enqueues its hipMemcpyAsync calls from it on h->stream and then calls bbh_stage_done.  (A synchronous hipMemcpy from pageable
// memory is not an alternative: four 4 KB copies of bbh_set_model_ex took 13 - 26 ms in a process holding a 1e5-row search space -
// profiles/r06_set_model_probe.log.)
void* bbh_stage_pinned(bbh_handle* h, size_t bytes) {
  if (!h->z_evt) {
    if (hipEventCreateWithFlags(&h->z_evt, hipEventDisableTiming) != hipSuccess) return nullptr;
  } else if (hipEventSynchronize(h->z_evt) != hipSuccess) {  // previous staged copy has been consumed
    return nullptr;
  }
  if (bytes > h->zstage_bytes) {
    if (h->h_zstage) hipHostFree(h->h_zstage);
    h->h_zstage = nullptr;
    h->zstage_bytes = 0;
    const size_t want = bytes < 4096 ? 4096 : bytes;
    if (hipHostMalloc((void**)&h->h_zstage, want, hipHostMallocDefault) != hipSuccess) return nullptr;
    h->zstage_bytes = want;
  }
  return h->h_zstage;
}

int bbh_stage_done(bbh_handle* h) {
  BBH_HIP_TRY(h, hipEventRecord(h->z_evt, h->stream));
  return 0;
}

int bbh_upload_z(bbh_handle* h, const double* z_host, size_t count) {
  const size_t bytes = sizeof(double) * count;
  if (bytes > h->z_bytes) {
    if (h->d_z) hipFree(h->d_z);
    h->d_z = nullptr;
    h->z_bytes = 0;
    BBH_HIP_TRY(h, hipMalloc((void**)&h->d_z, bytes));
    h->z_bytes = bytes;
  }
  // Staged through a pinned buffer of the handle, so that the call neither waits for the kernels already in
  // the stream (a synchronous copy would: it is ordered behind them) nor depends on the caller's buffer.
  void* stage = bbh_stage_pinned(h, bytes);
  if (!stage) {
    h->err = "bbh_upload_z: no pinned staging buffer";
    (void)hipGetLastError();
    return -2;
  }
  memcpy(stage, z_host, bytes);
  BBH_HIP_TRY(h, hipMemcpyAsync(h->d_z, stage, bytes, hipMemcpyHostToDevice, h->stream));
  return bbh_stage_done(h);
}

int bbh_qlogei_q1_sliced(bbh_handle* h, const double* mean_dev, const double* var_dev, int64_t N, const double* z_host, int64_t S,
                         double best_f, double sign, const uint8_t* alive_dev, double* scores_dev);  // bbh_select.hip
int bbh_qlogei_q1_rounds(bbh_handle* h, const double* mean_dev, const double* var_dev, int64_t N, const double* z_host, int64_t S,
                         double best_f, double sign, const uint8_t* alive_dev, double* scores_dev);

extern "C" int bbh_qlogei_q1(bbh_handle* h, const double* mean_dev, const double* var_dev, int64_t N,
                             const double* z_host, int64_t S, double best_f, double sign, const uint8_t* alive_dev,
                             double* scores_dev) {
  if (!h) return -1;
  if (!mean_dev || !var_dev || !z_host || !scores_dev || N < 0 || S < 1 || S > 8192) {
    h->err = "bbh_qlogei_q1: bad arguments (1 <= S <= 8192)";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  if (h->sw.q1_sliced) {  // sample-sliced form (bbh_select.hip); 1 = does not apply (S beyond its LDS tables)
    const int rc = bbh_qlogei_q1_sliced(h, mean_dev, var_dev, N, z_host, S, best_f, sign, alive_dev, scores_dev);
    if (rc <= 0) return rc;
  }
  return bbh_qlogei_q1_rounds(h, mean_dev, var_dev, N, z_host, S, best_f, sign, alive_dev, scores_dev);
}

// one thread per candidate over all S samples (any S; A/B partner of the sliced form: BBH_Q1_SLICED=0)
int bbh_qlogei_q1_rounds(bbh_handle* h, const double* mean_dev, const double* var_dev, int64_t N, const double* z_host, int64_t S,
                         double best_f, double sign, const uint8_t* alive_dev, double* scores_dev) {
  int rc = bbh_upload_z(h, z_host, (size_t)S);
  if (rc) return rc;
  bbh_timed_scope timed(h, BBH_TIMED_Q1);
  hipLaunchKernelGGL(bbh_qlogei_q1_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), sizeof(double) * S, h->stream,
                     mean_dev, var_dev, N, h->d_z, (int)S, best_f, sign, alive_dev, scores_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

// The register forms hold the base samples and the pending statistics in LDS: an upload of at most 60 KB
static bool bbh_fits_register_form(size_t upload_bytes) { return upload_bytes <= 60 * 1024; }

// f(std::integral_constant<int, Q>) for Q == q in 2 ... 14 (the register forms' instantiations); false for any other q
template <int Q = 2, class F>
static bool bbh_dispatch_q(int q, F&& f) {
  if constexpr (Q <= 14) {
    if (q != Q) return bbh_dispatch_q<Q + 1>(q, f);
    f(std::integral_constant<int, Q>());
    return true;
  }
  return false;
}

// p <= 15 pending points with the pending statistics given explicitly (the handle's own, or a caller's - see
// bbh_qlogei_pending_big)
static int bbh_qlogei_pending_impl(bbh_handle* h, const double* mean_dev, const double* var_dev, const double* cross_dev, int64_t N,
                                   int p, const double* mp_host, const double* cpp_host, const double* z_host, int64_t S,
                                   double best_f, double sign, const uint8_t* alive_dev, double* scores_dev);

extern "C" int bbh_qlogei_pending(bbh_handle* h, const double* mean_dev, const double* var_dev,
                                  const double* cross_dev, int64_t N, const double* z_host, int64_t S, double best_f,
                                  double sign, const uint8_t* alive_dev, double* scores_dev) {
  if (!h) return -1;
  if (h->p < 1) {
    h->err = "bbh_qlogei_pending: bad arguments / no pending points set";
    return -1;
  }
  return bbh_qlogei_pending_impl(h, mean_dev, var_dev, cross_dev, N, h->p, h->pend_mean.data(), h->pend_cov.data(), z_host, S, best_f,
                                 sign, alive_dev, scores_dev);
}

static int bbh_qlogei_pending_impl(bbh_handle* h, const double* mean_dev, const double* var_dev, const double* cross_dev, int64_t N,
                                   int p, const double* mp_host, const double* cpp_host, const double* z_host, int64_t S,
                                   double best_f, double sign, const uint8_t* alive_dev, double* scores_dev) {
  if (!mean_dev || !var_dev || !cross_dev || !z_host || !scores_dev || !mp_host || !cpp_host || N < 0 || S < 1 || p < 1 ||
      p > BBH_MAX_PENDING) {
    h->err = "bbh_qlogei_pending: bad arguments / no pending points set";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  bbh_joint_dev d;
  int rc = bbh_upload_joint(h, z_host, S, p, mp_host, cpp_host, false, &d);
  if (rc) return rc;
  const bool reg_form = bbh_fits_register_form(d.bytes) && !h->sw.pending_lds_form;
  // sample slices for small candidate sets (~16 waves per SIMD; linear-domain form; each slice at least 32 samples)
  int slices = 1;
#if BBH_PENDING_FAST
  if (reg_form && p + 1 <= 14) {
    int64_t want = ((int64_t)16 * 4 * h->num_cu * 64) / (h->slice_rows > 0 ? h->slice_rows : N);
    if (h->sw.pending_slices != INT_MIN) want = h->sw.pending_slices;
    if (want > S / 32) want = S / 32;
    slices = (int)(want < 1 ? 1 : (want > 32 ? 32 : want));
    if (slices > 1) {
      rc = bbh_ensure_ws(h, sizeof(double) * (size_t)slices * (size_t)N);
      if (rc) return rc;
    }
  }
#endif
  bbh_timed_scope timed(h, BBH_TIMED_PENDING);
  if (!(reg_form && bbh_dispatch_q(p + 1, [&](auto Q) {
          bbh_launch_pending_q<decltype(Q)::value>(h, mean_dev, var_dev, cross_dev, N, d.mean_p, d.cov_pp, d.z, (int)S, best_f, sign,
                                                   alive_dev, scores_dev, slices);
        })))
    hipLaunchKernelGGL(bbh_qlogei_pending_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, h->stream, mean_dev, var_dev,
                       cross_dev, N, p, d.mean_p, d.cov_pp, d.z, (int)S, best_f, sign, alive_dev, scores_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

// ---- joint q'-batches beyond 16 points ------------------------------------------------------------------------------------
// The reference has no cap on batch_size + pending experiments (botorch/discrete.py:120-126); the register form above holds
// q' <= 14, the LDS form q' <= 16.  For larger q' the thread-private Cholesky factor (q' (q' + 1) / 2 doubles: 4.2 KB at q' = 32)
// lives in a global workspace, element e of candidate i at Lws[e N + i] (coalesced across the wave), the per-sample
// log-fat-softplus values in LDS ([q'][64]); mean_p / cov_pp / z are read from global memory at wave-uniform addresses.  The
// same routines as bbh_qlogei_pending_kernel (log-domain streaming form, psd_safe_cholesky's jitter retries) over stride N.
// Memory-bound on the factor (q'^2 / 2 loads per sample): ~0.1 s per 1e5 candidates at q' = 32 - a correctness path for the
// rare large batch, not a tuned one.
#define QBIG_MAX 64
#define QBIG_WS_BYTES ((size_t)512 << 20)  // workspace bound of bbh_qlogei_pending_big (env BBH_QBIG_WS_MB for tests)
__global__ __launch_bounds__(64) void bbh_qlogei_pending_big_kernel(
    const double* __restrict__ mean, const double* __restrict__ var, const double* __restrict__ cross, int64_t N, int p,
    const double* __restrict__ mean_p, const double* __restrict__ cov_pp, const double* __restrict__ z, int S,
    double best_f, double sign, const uint8_t* __restrict__ alive, double* __restrict__ scores, double* __restrict__ Lws) {
  extern __shared__ double s_li[];  // [q][64]
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 64 + t;
  if (i >= N) return;
  if (alive && !alive[i]) {
    scores[i] = -INFINITY;
    return;
  }
  double* L = Lws + i;
  if (!bbh_joint_factor(L, N, p, var[i], cross + i * p, cov_pp)) {
    scores[i] = NAN;
    return;
  }
  scores[i] = bbh_qlogei_joint_lse(L, N, p + 1, mean[i], mean_p, z, S, best_f, sign, s_li + t, 64);
}

extern "C" int bbh_qlogei_pending_big(bbh_handle* h, const double* mean_dev, const double* var_dev, const double* cross_dev,
                                      int64_t N, int64_t p, const double* mean_p_host, const double* cov_pp_host,
                                      const double* z_host, int64_t S, double best_f, double sign, const uint8_t* alive_dev,
                                      double* scores_dev) {
  if (!h) return -1;
  if (!mean_dev || !var_dev || !cross_dev || !mean_p_host || !cov_pp_host || !z_host || !scores_dev || N < 0 || S < 1 || p < 1 ||
      p + 1 > QBIG_MAX) {
    h->err = "bbh_qlogei_pending_big: bad arguments (1 <= p <= 63 pending points)";
    return -1;
  }
  if (N == 0) return 0;
  if (p <= BBH_MAX_PENDING)  // the register / LDS kernels, with the caller's statistics instead of the handle's
    return bbh_qlogei_pending_impl(h, mean_dev, var_dev, cross_dev, N, (int)p, mean_p_host, cov_pp_host, z_host, S, best_f, sign,
                                   alive_dev, scores_dev);
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  const int64_t q = p + 1;
  bbh_joint_dev d;
  int rc = bbh_upload_joint(h, z_host, S, p, mean_p_host, cov_pp_host, false, &d);
  if (rc) return rc;
  // The per-candidate factor workspace is q'(q' + 1) / 2 doubles: 16 GB for 1e6 candidates at q' = 64.  The candidates are walked in
  // chunks whose workspace stays below QBIG_WS_BYTES (the handle's grow-only workspace outlives the call, also in the handle pool);
  // chunks are multiples of 64 rows, every chunk addresses its own rows from 0.
  const int64_t tri_q = q * (q + 1) / 2;
  const size_t ws_bound = h->sw.qbig_ws_mb ? (size_t)h->sw.qbig_ws_mb << 20 : QBIG_WS_BYTES;
  int64_t chunk = (int64_t)(ws_bound / (sizeof(double) * (size_t)tri_q)) / 64 * 64;
  if (chunk < 64) chunk = 64;
  if (chunk > N) chunk = N;
  rc = bbh_ensure_ws(h, sizeof(double) * (size_t)tri_q * (size_t)chunk);
  if (rc) return rc;
  bbh_timed_scope timed(h, BBH_TIMED_PENDING);
  for (int64_t c0 = 0; c0 < N; c0 += chunk) {
    const int64_t nc = std::min(chunk, N - c0);
    hipLaunchKernelGGL(bbh_qlogei_pending_big_kernel, dim3((unsigned)((nc + 63) / 64)), dim3(64), sizeof(double) * q * 64, h->stream,
                       mean_dev + c0, var_dev + c0, cross_dev + c0 * p, nc, (int)p, d.mean_p, d.cov_pp, d.z, (int)S, best_f, sign,
                       alive_dev ? alive_dev + c0 : nullptr, scores_dev + c0, h->d_ws);
  }
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

int bbh_argmax_rounds(bbh_handle* h, const double* scores_dev, int64_t N, double* best_val_host,
                      int64_t* best_idx_host) {
  if (!h) return -1;
  if (!scores_dev || N < 1 || !best_val_host || !best_idx_host) {
    h->err = "bbh_argmax: bad arguments";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  int rc = bbh_ensure_red(h);
  if (rc) return rc;
  int nblocks = (int)((N + 255) / 256);
  if (nblocks > ARGMAX_BLOCKS) nblocks = ARGMAX_BLOCKS;
  hipLaunchKernelGGL(bbh_argmax_stage1, dim3(nblocks), dim3(256), 0, h->stream, scores_dev, N, h->d_red, h->d_redi);
  hipLaunchKernelGGL(bbh_argmax_stage2, dim3(1), dim3(256), 0, h->stream, h->d_red, h->d_redi, nblocks,
                     h->d_red + ARGMAX_BLOCKS, h->d_redi + ARGMAX_BLOCKS);
  BBH_HIP_TRY(h, hipMemcpyAsync(best_val_host, h->d_red + ARGMAX_BLOCKS, sizeof(double), hipMemcpyDeviceToHost,
                                h->stream));
  BBH_HIP_TRY(h, hipMemcpyAsync(best_idx_host, h->d_redi + ARGMAX_BLOCKS, sizeof(int64_t), hipMemcpyDeviceToHost,
                                h->stream));
  BBH_HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

// ---- single-pass top-k -----------------------------------------------------------------------------
// stage 1: each workgroup owns a chunk of <= TOPK_CHUNK scores in LDS and extracts its k best by k
// rounds of workgroup-argmax + mask; stage 2: one workgroup merges the (blocks x k) survivors.
#define TOPK_CHUNK 4096
#define TOPK_MAXK 64

__device__ __forceinline__ void bbh_wg_argmax(double& v, int64_t& idx, double* sv, int64_t* si) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_down(v, o, 64);
    const int64_t oi = __shfl_down(idx, o, 64);
    amax_combine(v, idx, ov, oi);
  }
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = v;
    si[threadIdx.x >> 6] = idx;
  }
  __syncthreads();
  v = sv[0];
  idx = si[0];
  for (int w = 1; w < 4; w++) amax_combine(v, idx, sv[w], si[w]);
  __syncthreads();
}

__global__ __launch_bounds__(256) void bbh_topk_stage1(const double* __restrict__ scores, int64_t N, int k,
                                                       double* __restrict__ pv, int64_t* __restrict__ pi) {
  __shared__ double s_val[TOPK_CHUNK];
  __shared__ double sv[4];
  __shared__ int64_t si[4];
  const int64_t base = (int64_t)blockIdx.x * TOPK_CHUNK;
  const int cnt = (int)((N - base < TOPK_CHUNK) ? N - base : TOPK_CHUNK);
  for (int e = threadIdx.x; e < TOPK_CHUNK; e += 256) s_val[e] = (e < cnt) ? scores[base + e] : NAN;
  __syncthreads();
  for (int j = 0; j < k; j++) {
    double v = -INFINITY;
    int64_t idx = -1;
    for (int e = threadIdx.x; e < cnt; e += 256) {
      const double x = s_val[e];
      if (x == x) amax_combine(v, idx, x, base + e);
    }
    bbh_wg_argmax(v, idx, sv, si);
    if (threadIdx.x == 0) {
      pv[(int64_t)blockIdx.x * k + j] = v;
      pi[(int64_t)blockIdx.x * k + j] = idx;
      if (idx >= 0) s_val[idx - base] = NAN;  // taken
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void bbh_topk_stage2(double* __restrict__ pv, const int64_t* __restrict__ pi, int64_t cnt,
                                                       int k, double* __restrict__ outv, int64_t* __restrict__ outi) {
  __shared__ double sv[4];
  __shared__ int64_t si[4];
  __shared__ int64_t s_pos;
  for (int j = 0; j < k; j++) {
    double v = -INFINITY;
    int64_t idx = -1, pos = -1;
    for (int64_t e = threadIdx.x; e < cnt; e += 256) {
      const double x = pv[e];
      const int64_t gi = pi[e];
      if (gi >= 0 && x == x) {
        const int64_t before = idx;
        amax_combine(v, idx, x, gi);
        if (idx != before) pos = e;
      }
    }
    double bv = v;
    int64_t bi = idx;
    bbh_wg_argmax(bv, bi, sv, si);
    if (idx == bi && bi >= 0 && pos >= 0) s_pos = pos;  // unique owner: global indices are distinct
    __syncthreads();
    if (threadIdx.x == 0) {
      outv[j] = bv;
      outi[j] = bi;
      if (bi >= 0) pv[s_pos] = NAN;
    }
    __syncthreads();
  }
}

// k best scores on the device by k rounds of workgroup argmax (the form before bbh_select.hip; BBH_SELECT=0 routes bbh_topk /
// bbh_argmax here for A/B): *vals_dev / *idx_dev point into the handle's workspace (valid until its next use)
int bbh_topk_rounds_device(bbh_handle* h, const double* scores_dev, int64_t N, int64_t k, double** vals_dev, int64_t** idx_dev) {
  if (!scores_dev || N < 1 || k < 1 || k > N || k > TOPK_MAXK) {
    h->err = "bbh_topk: bad arguments (1 <= k <= min(N, 64))";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  const int64_t blocks = (N + TOPK_CHUNK - 1) / TOPK_CHUNK;
  const size_t need = (sizeof(double) + sizeof(int64_t)) * (size_t)(blocks * k + k);
  int rc = bbh_ensure_ws(h, need);
  if (rc) return rc;
  double* pv = h->d_ws;
  double* outv = pv + blocks * k;
  int64_t* pi = (int64_t*)(outv + k);
  int64_t* outi = pi + blocks * k;
  hipLaunchKernelGGL(bbh_topk_stage1, dim3((unsigned)blocks), dim3(256), 0, h->stream, scores_dev, N, (int)k, pv, pi);
  hipLaunchKernelGGL(bbh_topk_stage2, dim3(1), dim3(256), 0, h->stream, pv, pi, blocks * k, (int)k, outv, outi);
  BBH_HIP_TRY(h, hipGetLastError());
  *vals_dev = outv;
  *idx_dev = outi;
  return 0;
}

int bbh_topk_rounds(bbh_handle* h, const double* scores_dev, int64_t N, int64_t k, double* vals_host,
                    int64_t* idx_host) {
  if (!h) return -1;
  if (!vals_host || !idx_host) {
    h->err = "bbh_topk: bad arguments (1 <= k <= min(N, 64))";
    return -1;
  }
  double* outv = nullptr;
  int64_t* outi = nullptr;
  int rc = bbh_topk_rounds_device(h, scores_dev, N, k, &outv, &outi);
  if (rc) return rc;
  BBH_HIP_TRY(h, hipMemcpyAsync(vals_host, outv, sizeof(double) * k, hipMemcpyDeviceToHost, h->stream));
  BBH_HIP_TRY(h, hipMemcpyAsync(idx_host, outi, sizeof(int64_t) * k, hipMemcpyDeviceToHost, h->stream));
  BBH_HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int bbh_score_qlogei(bbh_handle* h, const double* X_dev, int64_t N, int64_t ldx, const double* z_host,
                                int64_t S, double best_f, double sign, const uint8_t* alive_dev, double* mean_dev,
                                double* var_dev, double* scores_dev) {
  if (!h) return -1;
  if (!h->factorized || N < 0 || (N > 0 && !X_dev) || ldx < h->desc.d || !z_host || S < 1 || S > 4096 || !scores_dev) {
    h->err = "bbh_score_qlogei: model not factorised / bad arguments (1 <= S <= 4096)";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  if (bbh_materialised_only(h)) {  // no fused form: materialised-K* posterior, then the stand-alone scoring kernel
    double *tm = mean_dev, *tv = var_dev, *scratch = nullptr;
    if (!tm || !tv) {
      BBH_HIP_TRY(h, hipMalloc((void**)&scratch, sizeof(double) * 2 * (size_t)N));
      tm = tm ? tm : scratch;
      tv = tv ? tv : scratch + N;
    }
    int rc2 = bbh_launch_fused(h, X_dev, N, ldx, tm, tv, nullptr, true);
    if (!rc2) rc2 = bbh_qlogei_q1(h, tm, tv, N, z_host, S, best_f, sign, alive_dev, scores_dev);
    if (scratch) {
      hipStreamSynchronize(h->stream);
      hipFree(scratch);
    }
    return rc2;
  }
  int rc = bbh_upload_z(h, z_host, (size_t)S);
  if (rc) return rc;
  h->fuse_qz = h->d_z;
  h->fuse_S = (int)S;
  h->fuse_best_f = best_f;
  h->fuse_sign = sign;
  h->fuse_alive = alive_dev;
  h->fuse_scores = scores_dev;
  rc = bbh_launch_fused(h, X_dev, N, ldx, mean_dev, var_dev, nullptr, true);
  h->fuse_qz = nullptr;
  h->fuse_scores = nullptr;
  return rc;
}

// =================================================================================================
// Other acquisition functions of baybe/acquisition/acqfs.py:161-290 on the same (mean, var, cross)
// inputs.  MC family (BoTorch SampleReducingMCAcquisitionFunction): mean_s max_j u(obj_sj);
// analytic family: closed forms in (mu~, sigma), sigma^2 clamped at 1e-12 as BoTorch does.
// =================================================================================================
__global__ __launch_bounds__(256) void bbh_mc_q1_kernel(int kind, const double* __restrict__ mean, const double* __restrict__ var,
                                                        int64_t N, const double* __restrict__ z, int S, double zbar,
                                                        double best_f, double sign, double cu,
                                                        const uint8_t* __restrict__ alive, double* __restrict__ scores) {
  extern __shared__ double s_z[];
  for (int s = threadIdx.x; s < S; s += blockDim.x) s_z[s] = z[s];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if (alive && !alive[i]) {
    scores[i] = -INFINITY;
    return;
  }
  const double a = sign * mean[i], b = sign * bbh_safe_sd(var[i]);
  const double m = fma(b, zbar, a);
  double sum = 0.0;
  for (int s = 0; s < S; s++) sum += bbh_mc_utility(kind, fma(b, s_z[s], a), m, best_f, cu);
  scores[i] = sum / (double)S;
}

__global__ __launch_bounds__(64) void bbh_mc_pending_kernel(int kind, const double* __restrict__ mean, const double* __restrict__ var,
                                                            const double* __restrict__ cross, int64_t N, int p,
                                                            const double* __restrict__ mean_p, const double* __restrict__ cov_pp,
                                                            const double* __restrict__ z, const double* __restrict__ zbar, int S,
                                                            double best_f, double sign, double cu,
                                                            const uint8_t* __restrict__ alive, double* __restrict__ scores) {
  __shared__ double s_L[QTRI * 64];
  __shared__ double s_mp[QMAX];
  __shared__ double s_cpp[QMAX * QMAX];
  const int t = threadIdx.x;
  const int q = p + 1;
  for (int e = t; e < p; e += 64) s_mp[e] = mean_p[e];
  for (int e = t; e < p * p; e += 64) s_cpp[e] = cov_pp[e];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 64 + t;
  if (i >= N) return;
  if (alive && !alive[i]) {
    scores[i] = -INFINITY;
    return;
  }
  double* L = s_L + t;
  if (!bbh_joint_factor(L, 64, p, var[i], cross + i * p, s_cpp)) {
    scores[i] = NAN;
    return;
  }
  const double m0 = mean[i];
  double mbar[QMAX];  // per-point sample means of the objective: the draw at zbar
#pragma unroll 1
  for (int r = 0; r < q; r++) mbar[r] = sign * bbh_joint_draw(L, 64, r, (r == 0) ? m0 : s_mp[r - 1], zbar);
  double sum = 0.0;
  for (int s = 0; s < S; s++) {
    const double* zs = z + (int64_t)s * q;
    double mx = -INFINITY;
#pragma unroll 1
    for (int r = 0; r < q; r++) {
      const double y = bbh_joint_draw(L, 64, r, (r == 0) ? m0 : s_mp[r - 1], zs);
      mx = fmax(mx, bbh_mc_utility(kind, sign * y, mbar[r], best_f, cu));
    }
    sum += mx;
  }
  scores[i] = sum / (double)S;
}

// Register-resident form of bbh_mc_pending_kernel for q' = Q <= 14 (see bbh_qlogei_pending_q_kernel): same
// arithmetic in the same order, factor and per-point values in registers, base samples in LDS.
template <int Q>
__global__ __launch_bounds__(256) void bbh_mc_pending_q_kernel(int kind, const double* __restrict__ mean,
                                                              const double* __restrict__ var, const double* __restrict__ cross,
                                                              int64_t N, const double* __restrict__ mean_p,
                                                              const double* __restrict__ cov_pp, const double* __restrict__ z,
                                                              const double* __restrict__ zbar, int S, double best_f, double sign,
                                                              double cu, const uint8_t* __restrict__ alive,
                                                              double* __restrict__ scores) {
  extern __shared__ double s_zq[];  // [S * Q] base samples, then zbar [Q], mean_p [Q - 1], cov_pp [(Q - 1)^2]
  constexpr int P = Q - 1;
  double* s_zb = s_zq + (int64_t)S * Q;
  double* s_mp = s_zb + Q;
  double* s_cpp = s_mp + P;
  for (int e = threadIdx.x; e < S * Q; e += 256) s_zq[e] = z[e];
  for (int e = threadIdx.x; e < Q; e += 256) s_zb[e] = zbar[e];
  for (int e = threadIdx.x; e < P; e += 256) s_mp[e] = mean_p[e];
  for (int e = threadIdx.x; e < P * P; e += 256) s_cpp[e] = cov_pp[e];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  if (alive && !alive[i]) {
    scores[i] = -INFINITY;
    return;
  }
  double L[Q * (Q + 1) / 2], A[Q * (Q + 1) / 2];
  bbh_joint_load_q<Q>(A, var[i], cross + i * P, s_cpp);
  if (!bbh_joint_factor_q<Q>(A, L)) {
    scores[i] = NAN;
    return;
  }
  double m[Q], mbar[Q], y[Q];
  m[0] = mean[i];
#pragma unroll
  for (int r = 1; r < Q; r++) m[r] = s_mp[r - 1];
  bbh_joint_draw_q<Q>(L, m, s_zb, y);  // per-point sample means of the objective: the draw at zbar
#pragma unroll
  for (int r = 0; r < Q; r++) mbar[r] = sign * y[r];
  double sum = 0.0;
  for (int s = 0; s < S; s++) {
    bbh_joint_draw_q<Q>(L, m, s_zq + (int64_t)s * Q, y);
    double mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < Q; r++) mx = fmax(mx, bbh_mc_utility(kind, sign * y[r], mbar[r], best_f, cu));
    sum += mx;
  }
  scores[i] = sum / (double)S;
}

template <int Q>
static void bbh_launch_mc_pending_q(hipStream_t st, int kind, const double* mean, const double* var, const double* cross,
                                    int64_t N, const double* mp, const double* cpp, const double* z, const double* zbar, int S,
                                    double best_f, double sign, double cu, const uint8_t* alive, double* scores) {
  const size_t lds = sizeof(double) * ((size_t)S * Q + Q + (Q - 1) + (size_t)(Q - 1) * (Q - 1));
  hipLaunchKernelGGL((bbh_mc_pending_q_kernel<Q>), dim3((unsigned)((N + 255) / 256)), dim3(256), lds, st, kind, mean, var,
                     cross, N, mp, cpp, z, zbar, S, best_f, sign, cu, alive, scores);
}

__device__ __forceinline__ double bbh_log_h(double u) {
  // log(phi(u) + u Phi(u)), asymptotic branch for u < -1 (BoTorch _log_ei_helper)
  const double inv_sqrt2 = 0.7071067811865476, half_log_2pi = 0.9189385332046727;
  if (u > -1.0) {
    const double phi = exp(-0.5 * u * u - half_log_2pi), Phi = 0.5 * erfc(-u * inv_sqrt2);
    return log(phi + u * Phi);
  }
  const double au = fabs(u);
  const double logphi = -0.5 * u * u - half_log_2pi;
  if (u > -1e6) return logphi + log1p(-au * erfcx(au * inv_sqrt2) * 1.2533141373155003);
  return logphi - 2.0 * log(au);
}

__global__ void bbh_analytic_kernel(int kind, const double* __restrict__ mean, const double* __restrict__ var, int64_t N,
                                    double best_f, double sign, double beta, int maximize,
                                    const uint8_t* __restrict__ alive, double* __restrict__ scores) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if (alive && !alive[i]) {
    scores[i] = -INFINITY;
    return;
  }
  const double mt = sign * mean[i];
  const double v = var[i];
  double out;
  if (kind == BBH_ACQ_PM) {
    out = mt;
  } else if (kind == BBH_ACQ_PSTD) {
    const double sd = sqrt(fmax(v, 0.0));
    out = maximize ? sd : -sd;
  } else {
    const double sd = sqrt(fmax(v, 1e-12));
    const double u = (mt - best_f) / sd;
    if (kind == BBH_ACQ_UCB)
      out = mt + sqrt(beta) * sd;
    else if (kind == BBH_ACQ_EI)
      out = sd * (exp(-0.5 * u * u - 0.9189385332046727) + u * 0.5 * erfc(-u * 0.7071067811865476));
    else if (kind == BBH_ACQ_PI)
      out = 0.5 * erfc(-u * 0.7071067811865476);
    else
      out = log(sd) + bbh_log_h(u);  // LogEI
  }
  scores[i] = out;
}

extern "C" int bbh_mc_acq_q1(bbh_handle* h, int32_t kind, const double* mean_dev, const double* var_dev, int64_t N,
                             const double* z_host, int64_t S, double best_f, double sign, double beta,
                             const uint8_t* alive_dev, double* scores_dev) {
  if (!h) return -1;
  if (kind == BBH_ACQ_QLOGEI) return bbh_qlogei_q1(h, mean_dev, var_dev, N, z_host, S, best_f, sign, alive_dev, scores_dev);
  if (kind < BBH_ACQ_QEI || kind > BBH_ACQ_QPSTD || !mean_dev || !var_dev || !z_host || !scores_dev || N < 0 || S < 1 ||
      S > 8192) {
    h->err = "bbh_mc_acq_q1: bad arguments";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  double zbar = 0.0;
  for (int64_t s = 0; s < S; s++) zbar += z_host[s];
  zbar /= (double)S;
  int rc = bbh_upload_z(h, z_host, (size_t)S);
  if (rc) return rc;
  bbh_timed_scope timed(h, BBH_TIMED_Q1);
  hipLaunchKernelGGL(bbh_mc_q1_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), sizeof(double) * S, h->stream, kind,
                     mean_dev, var_dev, N, h->d_z, (int)S, zbar, best_f, sign, bbh_mc_cu(kind, beta), alive_dev, scores_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

extern "C" int bbh_mc_acq_pending(bbh_handle* h, int32_t kind, const double* mean_dev, const double* var_dev,
                                  const double* cross_dev, int64_t N, const double* z_host, int64_t S, double best_f,
                                  double sign, double beta, const uint8_t* alive_dev, double* scores_dev) {
  if (!h) return -1;
  if (kind == BBH_ACQ_QLOGEI)
    return bbh_qlogei_pending(h, mean_dev, var_dev, cross_dev, N, z_host, S, best_f, sign, alive_dev, scores_dev);
  const int p = h->p;
  if (kind < BBH_ACQ_QEI || kind > BBH_ACQ_QPSTD || !mean_dev || !var_dev || !cross_dev || !z_host || !scores_dev ||
      N < 0 || S < 1 || p < 1) {
    h->err = "bbh_mc_acq_pending: bad arguments / no pending points set";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  bbh_joint_dev d;
  const int rc = bbh_upload_joint(h, z_host, S, p, h->pend_mean.data(), h->pend_cov.data(), true, &d);
  if (rc) return rc;
  const double cu = bbh_mc_cu(kind, beta);
  bbh_timed_scope timed(h, BBH_TIMED_PENDING);
  if (!(bbh_fits_register_form(d.bytes) && !h->sw.pending_lds_form && bbh_dispatch_q(p + 1, [&](auto Q) {
          bbh_launch_mc_pending_q<decltype(Q)::value>(h->stream, kind, mean_dev, var_dev, cross_dev, N, d.mean_p, d.cov_pp, d.z, d.zbar,
                                                      (int)S, best_f, sign, cu, alive_dev, scores_dev);
        })))
    hipLaunchKernelGGL(bbh_mc_pending_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, h->stream, kind, mean_dev, var_dev,
                       cross_dev, N, p, d.mean_p, d.cov_pp, d.z, d.zbar, (int)S, best_f, sign, cu, alive_dev, scores_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

extern "C" int bbh_analytic_acq(bbh_handle* h, int32_t kind, const double* mean_dev, const double* var_dev, int64_t N,
                                double best_f, double sign, double beta, int32_t maximize, const uint8_t* alive_dev,
                                double* scores_dev) {
  if (!h) return -1;
  if (kind < BBH_ACQ_PM || kind > BBH_ACQ_PI || !mean_dev || !var_dev || !scores_dev || N < 0) {
    h->err = "bbh_analytic_acq: bad arguments";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(bbh_analytic_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, kind, mean_dev, var_dev,
                     N, best_f, sign, beta, (int)maximize, alive_dev, scores_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}
