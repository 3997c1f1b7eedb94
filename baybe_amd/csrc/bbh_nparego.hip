// qLogNParEGO on the device (BoTorch qLogNParEGO: qLogNoisyExpectedImprovement under an augmented Chebyshev scalarisation of the
// m oriented targets; built with X_baseline = all training inputs and prune_baseline at baybe/acquisition/_builder.py:319-324).
//
// The set-up is qLogNEHVI's (bbh_nehvi_samples per target on the model extended by the baseline rows: oriented baseline samples
// F_b [S, nb, m] + the S weight columns of the conditional means), the rest is qLogNEI's with the scalarisation in front:
//
//   t_o    = w_o (hi_o - y_o) / (hi_o - lo_o),   g(y) = -(max_o t_o + 0.05 sum_o t_o)      (hi, lo: bounds of the baseline's
//                                                                                            oriented posterior means)
//   best_s = max_b g(F_b[s, b, :])                                                           bbh_scalarized_best_dev
//   f_s,o  = sign_o (E[f_o(x) | D, F_b,s,o] + safe_sd(v_o) z_x,s,o),   u_s = g(f_s) - best_s
//   score  = logmeanexp_s log_fatplus(u_s; 1e-6)                                             bbh_nparego_q1
//
// and prune_inferior_points keeps the baseline rows that are the first-index argmax of g in at least one of 2048 joint draws
// (bbh_scalarized_best_frequency_dev).
//
// Scoring geometry: a 2-D grid of candidates x sample slices, as bbh_qlognehvi_lin_kernel (one thread per candidate alone is
// 256 workgroups for a 65 536-row chunk - one per CU, each a long chain of dependent loads).  Every lane of a wave works on the
// same samples, so z_x and best_s are scalar loads and the scalarisation constants kernel arguments.  A slice is a FIXED number of
// samples (not a function of the candidate count): a candidate's partial sums, and with them its score, do not depend on which
// chunk of a chunked pass it sits in.  The slices' sums of fatplus terms (linear domain, as bbh_nei_term<true>) are combined
// in slice order by the finish kernel of bbh_slices.h: no atomics, identical rows score bit-identically.
#include "bbh_acqmath.h"
#include "bbh_slices.h"

namespace {

constexpr int NP_SLICE = 16;  // MC samples per slice
constexpr double NP_ALPHA = 0.05;

struct NparegoScal {  // augmented Chebyshev scalarisation of m oriented values
  double w[BBH_MAX_OBJECTIVES], hi[BBH_MAX_OBJECTIVES], inv[BBH_MAX_OBJECTIVES];  // inv = 1 / (hi - lo)
};

template <int M>
__device__ __forceinline__ double np_scalarize(const NparegoScal& sc, const double* y) {
  double mx = -INFINITY, sum = 0.0;
#pragma unroll
  for (int o = 0; o < M; o++) {
    const double t = sc.w[o] * (sc.hi[o] - y[o]) * sc.inv[o];
    mx = fmax(mx, t);
    sum += t;
  }
  return -fma(NP_ALPHA, sum, mx);
}

// one thread per sample over F_b [S, nb, M]: the sample's largest scalarised baseline value and its first index
template <int M>
__global__ __launch_bounds__(256) void bbh_scalarized_best_kernel(const double* __restrict__ Fb, int64_t S, int64_t nb, const NparegoScal sc,
                                                                  double* __restrict__ best_out, unsigned long long* __restrict__ counts) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const double* row = Fb + s * nb * M;
  double best = -INFINITY;
  int64_t arg = 0;
  for (int64_t b = 0; b < nb; b++) {
    double y[M];
#pragma unroll
    for (int o = 0; o < M; o++) y[o] = row[b * M + o];
    const double g = np_scalarize<M>(sc, y);
    if (b == 0 || g > best) {  // (strict: ties go to the first index)
      best = g;
      arg = b;
    }
  }
  if (best_out) best_out[s] = best;
  if (counts) atomicAdd(&counts[arg], 1ULL);
}

struct NparegoArgs {
  bbh_targets t;  // tmat [S, N] sample-major
  NparegoScal sc;
  int64_t N;
  int S;
  const double* zx;    // [S, M]
  const double* best;  // [S]
  const uint8_t* alive;
};

template <int M>
__device__ __forceinline__ double np_term(const NparegoArgs& a, const double* sd, int64_t i, int s) {
  double f[M];
#pragma unroll
  for (int o = 0; o < M; o++) f[o] = a.t.sign[o] * fma(sd[o], a.zx[(int64_t)s * M + o], a.t.tmat[o][(int64_t)s * a.N + i]);
  const double u = np_scalarize<M>(a.sc, f) - a.best[s];
  return bbh_fatplus_core<2>(u * (1.0 / TAU_RELU));
}

// thread (i, slice): sum over the slice's samples of fatplus(u_s; tau) / tau -> partial [slices, N]
template <int M>
__global__ __launch_bounds__(256) void bbh_nparego_q1_kernel(const NparegoArgs a, double* __restrict__ partial) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  const bbh_slice sl = bbh_slice_bounds(a.S, NP_SLICE, (int)blockIdx.y);
  if (a.alive && !a.alive[i]) {
    partial[(int64_t)blockIdx.y * a.N + i] = 0.0;
    return;
  }
  double sd[M];
#pragma unroll
  for (int o = 0; o < M; o++) sd[o] = bbh_safe_sd(a.t.var[o][i]);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;  // independent chains: 4 M loads in flight per lane
  int s = sl.begin;
  for (; s + 3 < sl.end; s += 4) {
    s0 += np_term<M>(a, sd, i, s);
    s1 += np_term<M>(a, sd, i, s + 1);
    s2 += np_term<M>(a, sd, i, s + 2);
    s3 += np_term<M>(a, sd, i, s + 3);
  }
  for (; s < sl.end; s++) s0 += np_term<M>(a, sd, i, s);
  partial[(int64_t)blockIdx.y * a.N + i] = (s0 + s1) + (s2 + s3);
}

bool np_fill_scal(NparegoScal& sc, int32_t m, const double* w, const double* hi, const double* inv) {
  for (int o = 0; o < BBH_MAX_OBJECTIVES; o++) {
    sc.w[o] = o < m ? w[o] : 0.0;
    sc.hi[o] = o < m ? hi[o] : 0.0;
    sc.inv[o] = o < m ? inv[o] : 1.0;
    if (o < m && !(sc.w[o] >= 0.0 && sc.inv[o] > 0.0 && sc.inv[o] < INFINITY && sc.hi[o] == sc.hi[o])) return false;
  }
  return true;
}

int np_scalarized_best(bbh_handle* h, const char* what, const double* Fb_dev, int64_t S, int64_t nb, int32_t m, const double* w,
                       const double* hi, const double* inv, double* best_dev, int64_t* counts_host) {
  if (!h) return -1;
  NparegoScal sc;
  if (!Fb_dev || S < 1 || nb < 1 || m < 1 || m > BBH_MAX_OBJECTIVES || !w || !hi || !inv || !np_fill_scal(sc, m, w, hi, inv) ||
      (!best_dev && !counts_host)) {
    h->err = std::string(what) + ": bad arguments (S >= 1, nb >= 1, 1 <= m <= 4, weights >= 0, finite 1 / (hi - lo) > 0)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  unsigned long long* d_cnt = nullptr;
  if (counts_host) {
    int rc = bbh_ensure_ws(h, sizeof(unsigned long long) * (size_t)nb);
    if (rc) return rc;
    d_cnt = (unsigned long long*)h->d_ws;
    BBH_HIP_TRY(h, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * nb, h->stream));
  }
  const dim3 grid((unsigned)((S + 255) / 256)), block(256);
  bbh_dispatch_m(m, [&](auto M) {
    hipLaunchKernelGGL(bbh_scalarized_best_kernel<decltype(M)::value>, grid, block, 0, h->stream, Fb_dev, S, nb, sc, best_dev, d_cnt);
  });
  BBH_HIP_TRY(h, hipGetLastError());
  if (counts_host) {
    BBH_HIP_TRY(h, hipMemcpyAsync(counts_host, d_cnt, sizeof(int64_t) * nb, hipMemcpyDeviceToHost, h->stream));
    BBH_HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  return 0;
}

}  // namespace

extern "C" int bbh_scalarized_best_dev(bbh_handle* h, const double* Fb_dev, int64_t S, int64_t nb, int32_t m, const double* w_host,
                                       const double* hi_host, const double* inv_range_host, double* best_dev) {
  if (h && !best_dev) {
    h->err = "bbh_scalarized_best_dev: bad arguments (no output)";
    return -1;
  }
  return np_scalarized_best(h, "bbh_scalarized_best_dev", Fb_dev, S, nb, m, w_host, hi_host, inv_range_host, best_dev, nullptr);
}

extern "C" int bbh_scalarized_best_frequency_dev(bbh_handle* h, const double* Fb_dev, int64_t S, int64_t nb, int32_t m,
                                                 const double* w_host, const double* hi_host, const double* inv_range_host,
                                                 int64_t* counts_host) {
  if (h && !counts_host) {
    h->err = "bbh_scalarized_best_frequency_dev: bad arguments (no output)";
    return -1;
  }
  return np_scalarized_best(h, "bbh_scalarized_best_frequency_dev", Fb_dev, S, nb, m, w_host, hi_host, inv_range_host, nullptr, counts_host);
}

extern "C" int bbh_nparego_q1(bbh_handle* h, int32_t m, int64_t N, const double* const* tmat_sm_dev, const double* const* var_dev,
                              const double* sign_host, const double* zx_dev, int64_t S, const double* w_host, const double* hi_host,
                              const double* inv_range_host, const double* best_dev, const uint8_t* alive_dev, double* scores_dev) {
  if (!h) return -1;
  NparegoArgs a;
  if (m < 1 || m > BBH_MAX_OBJECTIVES || N < 0 || S < 1 || S > 8192 || !tmat_sm_dev || !var_dev || !sign_host || !zx_dev || !w_host ||
      !hi_host || !inv_range_host || !best_dev || !scores_dev || !np_fill_scal(a.sc, m, w_host, hi_host, inv_range_host)) {
    h->err = "bbh_nparego_q1: bad arguments (1 <= m <= 4, 1 <= S <= 8192, weights >= 0, finite 1 / (hi - lo) > 0)";
    return -1;
  }
  if (!bbh_fill_targets(a.t, m, N, tmat_sm_dev, var_dev, sign_host)) {
    h->err = "bbh_nparego_q1: bad arguments (a target without conditional means or variances)";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  const int slices = bbh_slices_by_len(S, NP_SLICE).count;
  int rc = bbh_ensure_ws(h, sizeof(double) * (size_t)slices * (size_t)N);
  if (rc) return rc;
  a.N = N;
  a.S = (int)S;
  a.zx = zx_dev;  // (the caller's block: one upload per step, no host wait per chunk)
  a.best = best_dev;
  a.alive = alive_dev;
  bbh_timed_scope timed(h, BBH_TIMED_Q1);
  const dim3 sgrid((unsigned)((N + 255) / 256), (unsigned)slices), block(256);
  bbh_dispatch_m(m, [&](auto M) { hipLaunchKernelGGL(bbh_nparego_q1_kernel<decltype(M)::value>, sgrid, block, 0, h->stream, a, h->d_ws); });
  bbh_slices_finish<BBH_FINISH_LOG_TAU_MEAN>(h, h->d_ws, slices, 1, N, S, alive_dev, scores_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}
