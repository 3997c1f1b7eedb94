// Per-sample building blocks shared by the acquisition kernels (bbh_acq.hip, bbh_qnehvi.hip, bbh_nei.hip, the scoring epilogue of
// bbh_coopcols.h): the fat softplus of qLogEI-type utilities, the 1 x 1 psd_safe_cholesky, the short reciprocal / logarithm.  Maths restated in
// oracle/gp_oracle.py (log_fatplus, _safe_sqrt_var).
#pragma once
#include <math.h>

#include "bbh_common.h"

#define TAU_RELU 1e-6
#define LOG_TAU_RELU -13.815510557964274  // log(TAU_RELU): the same double as the folded library call (-0x1.ba18a998fffap+3)
#define TAU_MAX 1e-2                      // temperature of the fat maximum / minimum
typedef float bbh_f2 __attribute__((ext_vector_type(2)));

// fatplus(x; tau) / tau = softplus(t) + 0.1 / (1 + t^2),  t = x / tau; torch softplus threshold 20
template <int NEWTON = 2>
__device__ __forceinline__ double bbh_fatplus_core(double t) {
  // softplus: t / tau_relu is huge in magnitude for almost every sample, so the log1p(exp) branch is rare.
  // It is entered through a wave-uniform test (ballot): a per-lane branch in unrolled callers is
  // if-converted by the compiler into "always evaluate both sides", i.e. ~50 extra VALU per call.
  double sp = (t > 20.0) ? t : 0.0;
  const bool mid = !(t > 20.0) && !(t < -750.0);
  if (__builtin_amdgcn_ballot_w64(mid) != 0) {
    if (mid) sp = log1p(exp(t));
  }
  // 0.1 / (1 + t^2) without the IEEE division sequence (div_scale / div_fmas / div_fixup, ~15 VALU
  // of the ~22 per sample): v_rcp_f64 seed (2^-26) and two Newton steps; 1 + t^2 is in [1, 1e40) for
  // every reachable t, so no scaling is needed.  Relative error <= 2 ulp.
  const double d = fma(t, t, 1.0);
  double y = __builtin_amdgcn_rcp(d);
  y = fma(fma(-d, y, 1.0), y, y);
  if (NEWTON > 1) y = fma(fma(-d, y, 1.0), y, y);  // (one step: <= 2^-46 relative - enough where the caller's own terms are single precision)
  y = (d < INFINITY) ? y : 0.0;  // |t| = inf (unbounded cell): the Newton step would produce inf * 0
  return fma(0.1, y, sp);
}

// 1x1 psd_safe_cholesky: v <= 0 (or NaN) -> add jitter 1e-8, 1e-7, 1e-6
__device__ __forceinline__ double bbh_safe_sd(double v) {
  if (!(v > 0.0)) {
    v += 1e-8;
    if (!(v > 0.0)) {
      v += 1e-7;
      if (!(v > 0.0)) v += 1e-6;
    }
  }
  return sqrt(fmax(v, 0.0));
}

// log(x) for positive, finite, normal x (the fat-softplus values and sums of squares below): exponent and
// mantissa by v_frexp, m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(s), s = (m - 1)/(m + 1) through a
// v_rcp_f64 seed with two Newton steps, odd series to s^19 (|s| <= 0.1716: truncation 2e-17), two-word ln 2.
// ~26 VALU instead of ~40 for the library call; relative error <= 3e-16 (also next to x = 1, where the
// result is 2 s (1 + R) with no cancellation).
__device__ __forceinline__ double bbh_fast_recip(double d) {
  double y = __builtin_amdgcn_rcp(d);
  y = fma(fma(-d, y, 1.0), y, y);
  return fma(fma(-d, y, 1.0), y, y);
}
__device__ __forceinline__ double bbh_fast_log_pos(double x) {
  double m = __builtin_amdgcn_frexp_mant(x);  // [0.5, 1)
  int e = __builtin_amdgcn_frexp_exp(x);
  const bool lowm = m < 0.70710678118654752440;
  m = lowm ? 2.0 * m : m;
  e = lowm ? e - 1 : e;
  const double f = m - 1.0;
  const double s = f * bbh_fast_recip(2.0 + f);
  const double z = s * s;
  double r = fma(z, 1.0 / 19.0, 1.0 / 17.0);
  r = fma(r, z, 1.0 / 15.0);
  r = fma(r, z, 1.0 / 13.0);
  r = fma(r, z, 1.0 / 11.0);
  r = fma(r, z, 1.0 / 9.0);
  r = fma(r, z, 1.0 / 7.0);
  r = fma(r, z, 1.0 / 5.0);
  r = fma(r, z, 1.0 / 3.0);
  const double lm = fma(2.0 * s * z, r, 2.0 * s);
  const double ed = (double)e;
  const double r2 = fma(ed, 6.93147180369123816490e-01, fma(ed, 1.90821492927058770002e-10, lm));
  return (x < INFINITY) ? r2 : x;  // log(inf) = inf (NaN propagates)
}

// ---- MC family (BoTorch SampleReducingMCAcquisitionFunction): the utility of one objective sample; m: the sample mean of the
// objective (qUCB / qPSTD), cu: bbh_mc_cu ------------------------------------------------------------------------------------
__device__ __forceinline__ double bbh_mc_utility(int kind, double obj, double m, double best_f, double cu) {
  switch (kind) {
    case BBH_ACQ_QEI: return fmax(obj - best_f, 0.0);
    case BBH_ACQ_QPI: return 1.0 / (1.0 + exp(-(obj - best_f) * 1e3));
    case BBH_ACQ_QSR: return obj;
    case BBH_ACQ_QUCB: return m + cu * fabs(obj - m);
    default: return cu * fabs(obj - m);  // QPSTD
  }
}

static inline double bbh_mc_cu(int kind, double beta) {
  if (kind == BBH_ACQ_QUCB) return sqrt(beta * 3.141592653589793 / 2.0);
  if (kind == BBH_ACQ_QPSTD) return sqrt(3.141592653589793 / 2.0);
  return 0.0;
}

// ---- qNEI / qLogNEI (bbh_nei.hip) ----------------------------------------------------------------
// One MC sample of a candidate: the joint draw f_s = E[f(x) | D, F_b,s] + sd z_x,s against the sample's best baseline
// value, u_s = sign f_s - best_s.  LOG: fatplus(u_s; tau_relu) / tau_relu (summed in the linear domain like
// bbh_qlogei_q1_kernel: the terms lie in [1e-17 / u_s^2, |u_s| / tau], no scaling is needed for any reachable u_s);
// otherwise max(u_s, 0).  The fused epilogue and the unfused verification kernel both call this, so their terms are equal
// bit for bit and only the order of the sums differs.
template <bool LOG>
__device__ __forceinline__ double bbh_nei_term(double cond_mean, double sd, double zx, double best, double sign) {
  const double u = sign * fma(sd, zx, cond_mean) - best;
  if constexpr (LOG) return bbh_fatplus_core<2>(u * (1.0 / TAU_RELU));
  return fmax(u, 0.0);
}
// sum over the S samples -> score
template <bool LOG>
__device__ __forceinline__ double bbh_nei_finish(double sum, int S) {
  if constexpr (LOG) return LOG_TAU_RELU + log(sum) - log((double)S);
  return sum / (double)S;
}
