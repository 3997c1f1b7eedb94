// qNoisyExpectedImprovement / qLogNoisyExpectedImprovement on the device (baybe/acquisition/acqfs.py:226-243; built with
// X_baseline = all training inputs and prune_baseline at baybe/acquisition/_builder.py:319-324).
//
// BoTorch draws f(x) jointly with the baseline values f(X_b) through a cached Cholesky root and scores the improvement over
// the sample's own best baseline value.  The set-up is qLogNEHVI's with one target (bbh_nehvi_samples on the model extended
// by the baseline rows: oriented baseline samples + the S weight columns of the conditional means), the rest is
//
//   best_s = max_b F_b,s                                       bbh_sample_best_dev
//   f_s    = E[f(x) | D, F_b,s] + safe_sd(Var[f(x) | D, X_b]) z_x,s
//   u_s    = sign f_s - best_s
//   qLogNEI = logmeanexp_s log_fatplus(u_s; 1e-6),  qNEI = mean_s max(u_s, 0)
//
// and prune_inferior_points keeps the baseline rows that are the best of at least one of 2048 joint draws
// (bbh_best_frequency_dev).  Two forms of the scoring pass:
//   fused    bbh_score_nei: the cooperative columns kernel with a scoring epilogue (bbh_coopcols.h) - for S <= 512 its
//            accumulators hold a candidate's whole sample axis, so the [S, N] matrix of conditional means is never written;
//   unfused  bbh_nei_q1 over a sample-major block from bbh_posterior_columns_sm: verification form, composite-kernel models
//            (materialised K*), S > 512.  The caller chunks the candidates.
// Neither form allocates anything that grows with S N: the fused pass takes no workspace at all (the S base samples go
// through the handle's staging buffer, bbh_upload_z), the unfused one reads the caller's block.
#include "bbh_coopcols.h"

void bbh_fill_fused_args(bbh_handle* h, FusedArgs& a, const double* X_dev, int64_t N, int64_t ldx);  // bbh_panel.hip

namespace {

// one thread per sample: first index of the sample's largest baseline value
__global__ __launch_bounds__(256) void bbh_best_freq_kernel(const double* __restrict__ obj, int64_t S, int64_t nb,
                                                            unsigned long long* __restrict__ counts) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const double* row = obj + s * nb;
  double best = row[0];
  int64_t arg = 0;
  for (int64_t b = 1; b < nb; b++) {
    const double v = row[b];
    if (v > best) {  // (strict: ties go to the first index)
      best = v;
      arg = b;
    }
  }
  atomicAdd(&counts[arg], 1ULL);
}

__global__ __launch_bounds__(256) void bbh_sample_best_kernel(const double* __restrict__ obj, int64_t S, int64_t nb,
                                                              double* __restrict__ best_out) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const double* row = obj + s * nb;
  double best = row[0];
  for (int64_t b = 1; b < nb; b++) best = fmax(best, row[b]);
  best_out[s] = best;
}

// one thread per candidate over a sample-major block tmat [S, N]: coalesced reads, the samples' constants are wave-uniform
template <bool LOG>
__global__ __launch_bounds__(256) void bbh_nei_q1_kernel(const double* __restrict__ tmat, const double* __restrict__ var, int64_t N,
                                                         const double* __restrict__ zx, const double* __restrict__ best, int S,
                                                         double sign, const uint8_t* __restrict__ alive, double* __restrict__ scores) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  if (alive && !alive[i]) {
    scores[i] = -INFINITY;
    return;
  }
  const double sd = bbh_safe_sd(var[i]);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;  // independent chains, as bbh_qlogei_q1_kernel
  int s = 0;
  for (; s + 3 < S; s += 4) {
    s0 += bbh_nei_term<LOG>(tmat[(int64_t)s * N + i], sd, zx[s], best[s], sign);
    s1 += bbh_nei_term<LOG>(tmat[(int64_t)(s + 1) * N + i], sd, zx[s + 1], best[s + 1], sign);
    s2 += bbh_nei_term<LOG>(tmat[(int64_t)(s + 2) * N + i], sd, zx[s + 2], best[s + 2], sign);
    s3 += bbh_nei_term<LOG>(tmat[(int64_t)(s + 3) * N + i], sd, zx[s + 3], best[s + 3], sign);
  }
  for (; s < S; s++) s0 += bbh_nei_term<LOG>(tmat[(int64_t)s * N + i], sd, zx[s], best[s], sign);
  scores[i] = bbh_nei_finish<LOG>((s0 + s1) + (s2 + s3), S);
}

bool nei_kind_ok(int32_t kind) { return kind == BBH_ACQ_QNEI || kind == BBH_ACQ_QLOGNEI; }

template <bool HAS_TBL, int KIND, int NT>
int nei_launch(bbh_handle* h, bool log_form, dim3 grid, size_t lds, const FusedArgs& a, int64_t groups, int64_t nks, const NeiEpilogue& ne) {
  const void* kfn = log_form ? (const void*)bbh_coop_nei_kernel<HAS_TBL, KIND, NT, true> : (const void*)bbh_coop_nei_kernel<HAS_TBL, KIND, NT, false>;
  BBH_HIP_TRY(h, bbh_allow_lds(h->device, kfn, lds));
  if (log_form)
    hipLaunchKernelGGL((bbh_coop_nei_kernel<HAS_TBL, KIND, NT, true>), grid, dim3(256), lds, h->stream, a, h->d_colfrag, groups, nks, ne);
  else
    hipLaunchKernelGGL((bbh_coop_nei_kernel<HAS_TBL, KIND, NT, false>), grid, dim3(256), lds, h->stream, a, h->d_colfrag, groups, nks, ne);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int bbh_best_frequency_dev(bbh_handle* h, const double* obj_dev, int64_t S, int64_t nb, int64_t* counts_host) {
  if (!h) return -1;
  if (!obj_dev || !counts_host || S < 1 || nb < 1) {
    h->err = "bbh_best_frequency_dev: bad arguments (S >= 1, nb >= 1)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  int rc = bbh_ensure_ws(h, sizeof(unsigned long long) * (size_t)nb);
  if (rc) return rc;
  unsigned long long* d_cnt = (unsigned long long*)h->d_ws;
  BBH_HIP_TRY(h, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * nb, h->stream));
  hipLaunchKernelGGL(bbh_best_freq_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, h->stream, obj_dev, S, nb, d_cnt);
  BBH_HIP_TRY(h, hipGetLastError());
  BBH_HIP_TRY(h, hipMemcpyAsync(counts_host, d_cnt, sizeof(int64_t) * nb, hipMemcpyDeviceToHost, h->stream));
  BBH_HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int bbh_sample_best_dev(bbh_handle* h, const double* obj_dev, int64_t S, int64_t nb, double* best_dev) {
  if (!h) return -1;
  if (!obj_dev || !best_dev || S < 1 || nb < 1) {
    h->err = "bbh_sample_best_dev: bad arguments (S >= 1, nb >= 1)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(bbh_sample_best_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, h->stream, obj_dev, S, nb, best_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

extern "C" int bbh_nei_q1(bbh_handle* h, int32_t kind, const double* tmat_sm_dev, const double* var_dev, int64_t N, const double* zx_host,
                          int64_t S, const double* best_dev, double sign, const uint8_t* alive_dev, double* scores_dev) {
  if (!h) return -1;
  if (!nei_kind_ok(kind) || N < 0 || S < 1 || S > 8192 || !zx_host || !best_dev || !scores_dev || (N > 0 && (!tmat_sm_dev || !var_dev))) {
    h->err = "bbh_nei_q1: bad arguments (kind BBH_ACQ_QNEI / BBH_ACQ_QLOGNEI, 1 <= S <= 8192)";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  int rc = bbh_upload_z(h, zx_host, (size_t)S);
  if (rc) return rc;
  bbh_timed_scope timed(h, BBH_TIMED_Q1);
  const dim3 grid((unsigned)((N + 255) / 256)), block(256);
  if (kind == BBH_ACQ_QLOGNEI)
    hipLaunchKernelGGL(bbh_nei_q1_kernel<true>, grid, block, 0, h->stream, tmat_sm_dev, var_dev, N, h->d_z, best_dev, (int)S, sign, alive_dev, scores_dev);
  else
    hipLaunchKernelGGL(bbh_nei_q1_kernel<false>, grid, block, 0, h->stream, tmat_sm_dev, var_dev, N, h->d_z, best_dev, (int)S, sign, alive_dev, scores_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  h->last_nei_form = 2;
  return 0;
}

// 0: the fused pass is enqueued; 1: it does not apply to this model / sample count / switch setting and nothing was enqueued
// (the caller takes bbh_posterior_columns_sm + bbh_nei_q1); < 0: error.
extern "C" int bbh_score_nei(bbh_handle* h, int32_t kind, const double* X_dev, int64_t N, int64_t ldx, const double* var_dev,
                             const double* zx_host, int64_t S, const double* best_dev, double sign, const uint8_t* alive_dev,
                             double* scores_dev) {
  if (!h) return -1;
  if (!h->factorized || h->ncols < 1 || !h->d_colfrag || !nei_kind_ok(kind) || N < 0 || (N > 0 && (!X_dev || !var_dev)) || ldx < h->desc.d ||
      !zx_host || S != h->ncols || !best_dev || !scores_dev) {
    h->err = "bbh_score_nei: install the weight columns first (bbh_nehvi_samples with S columns) / bad arguments";
    return -1;
  }
  if (bbh_is_rff(h)) {
    h->err = "bbh_score_nei: not available with the RFF kernel";
    return -1;
  }
  if (!h->sw.nei_fused || S > 512 || bbh_materialised_only(h)) return 1;
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  int rc = bbh_upload_z(h, zx_host, (size_t)S);
  if (rc) return rc;
  bbh_timed_scope timed(h, BBH_TIMED_COLUMNS);
  FusedArgs a;
  bbh_fill_fused_args(h, a, X_dev, N, ldx);
  NeiEpilogue ne;
  ne.var = var_dev;
  ne.zx = h->d_z;
  ne.best = best_dev;
  ne.alive = alive_dev;
  ne.scores = scores_dev;
  ne.sign = sign;
  ne.S = (int)S;
  const bool has_tbl = (h->T > 1) || h->desc.use_outputscale;
  const bool m52 = (a.kind == BBH_KERNEL_MATERN52);
  const bool log_form = kind == BBH_ACQ_QLOGNEI;
  const int64_t groups = bbh_round_up(S, 128) / 128, nks = h->np / 4;
  const int nt = (h->sw.columns_nt == 1 || !m52) ? 1 : 2;  // (runtime kernel kinds: two tiles spill, as in bbh_posterior_columns)
  const dim3 grid((unsigned)((N + 16 * nt - 1) / (16 * nt)));
  // candidate fragments | kernel-value slots | partial sums [nt][4][16] | sample table [2][512]
  const size_t lds = sizeof(double) * ((size_t)nt * h->kd * 64 + 2 * (size_t)nt * 1024 + (size_t)nt * 64 + 1024);
  if (m52 && nt == 2)
    rc = has_tbl ? nei_launch<true, BBH_KERNEL_MATERN52, 2>(h, log_form, grid, lds, a, groups, nks, ne)
                 : nei_launch<false, BBH_KERNEL_MATERN52, 2>(h, log_form, grid, lds, a, groups, nks, ne);
  else if (m52)
    rc = has_tbl ? nei_launch<true, BBH_KERNEL_MATERN52, 1>(h, log_form, grid, lds, a, groups, nks, ne)
                 : nei_launch<false, BBH_KERNEL_MATERN52, 1>(h, log_form, grid, lds, a, groups, nks, ne);
  else
    rc = has_tbl ? nei_launch<true, -1, 1>(h, log_form, grid, lds, a, groups, nks, ne)
                 : nei_launch<false, -1, 1>(h, log_form, grid, lds, a, groups, nks, ne);
  if (rc) return rc;
  h->last_nei_form = 1;
  return 0;
}

extern "C" int bbh_last_nei_form(bbh_handle* h) { return h ? h->last_nei_form : -1; }
