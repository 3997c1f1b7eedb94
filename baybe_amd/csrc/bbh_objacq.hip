// MC acquisition functions of a transformed target: the kernels of bbh_acq.hip's MC family with an objective program
// (bbh_objective.h) between the draw and the utility.
//
// The reference fits the surrogate on the raw target and hands the acquisition function the target's transformation as an MC
// objective (baybe/acquisition/_builder.py:211-254: objective = GenericMCObjective over objectives/base.py:130-150), which BoTorch
// applies to every posterior sample before the utility (botorch MCAcquisitionFunction._get_samples_and_objectives).  So per
// candidate and base sample:  y = mu + L z  (the joint draw of bbh_joint.h),  g = prog(y),  u = utility(g), then the (fat) maximum
// over the q' points and the mean over the samples, exactly as bbh_mc_q1_kernel / bbh_mc_pending_kernel / the qLogEI kernels do
// with g = sign y.  Differences to those kernels that the objective forces:
//   - qUCB / qPSTD need mean_s g_s (BoTorch's obj.mean(dim=0)).  For g = sign y that is the draw at zbar; for any other program it
//     is not, so a first pass over the samples takes the mean of g itself.
//   - no fused posterior + score pass, no register-resident Q instantiations, no sample slices: one thread per candidate in the
//     run-time-q' LDS form only (follow-up, see KERNELS.md).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "bbh_common.h"
#include "bbh_acqmath.h"    // TAU_RELU, bbh_fatplus_core, bbh_safe_sd, bbh_mc_utility, bbh_mc_cu
#include "bbh_joint.h"      // QMAX, QTRI, bbh_joint_factor, bbh_joint_draw, bbh_upload_joint
#include "bbh_objective.h"  // bbh_apply_objective

#define OBJ_TAU_MAX 1e-2

// q' = 1.  qLogEI: log mean_s fatplus(g_s - best_f) summed in the linear domain like bbh_qlogei_q1_kernel (all terms positive).
__global__ __launch_bounds__(256) void bbh_obj_q1_kernel(int kind, const bbh_objective_prog prog, const double* __restrict__ mean,
                                                         const double* __restrict__ var, int64_t N, const double* __restrict__ z,
                                                         int S, double best_f, double cu, const uint8_t* __restrict__ alive,
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
  const double a = mean[i], b = bbh_safe_sd(var[i]);
  double sum = 0.0;
  if (kind == BBH_ACQ_QLOGEI) {
    const double inv_tau = 1.0 / TAU_RELU;
    for (int s = 0; s < S; s++) sum += bbh_fatplus_core<2>((bbh_apply_objective(prog, fma(b, s_z[s], a)) - best_f) * inv_tau);
    scores[i] = log(TAU_RELU) + log(sum) - log((double)S);
    return;
  }
  double m = 0.0;
  if (kind == BBH_ACQ_QUCB || kind == BBH_ACQ_QPSTD) {
    for (int s = 0; s < S; s++) m += bbh_apply_objective(prog, fma(b, s_z[s], a));
    m /= (double)S;
  }
  for (int s = 0; s < S; s++) sum += bbh_mc_utility(kind, bbh_apply_objective(prog, fma(b, s_z[s], a)), m, best_f, cu);
  scores[i] = sum / (double)S;
}

// q' = 1 + p <= 16 in the form of bbh_mc_pending_kernel: the factor in LDS (element e of thread t at s_L[e * 64 + t]), the base
// samples and pending statistics at wave-uniform addresses.  s_v holds one double per point and thread: the per-point means of g
// (qUCB / qPSTD) or the per-point log-fat-softplus values of the current sample (qLogEI) - in LDS because a thread-private array
// under a run-time index would live in scratch memory.  69 632 + 8 192 + 2 176 B of LDS: two workgroups per CU, as the parent form.
__global__ __launch_bounds__(64) void bbh_obj_pending_kernel(int kind, const bbh_objective_prog prog, const double* __restrict__ mean,
                                                             const double* __restrict__ var, const double* __restrict__ cross,
                                                             int64_t N, int p, const double* __restrict__ mean_p,
                                                             const double* __restrict__ cov_pp, const double* __restrict__ z, int S,
                                                             double best_f, double cu, const uint8_t* __restrict__ alive,
                                                             double* __restrict__ scores) {
  __shared__ double s_L[QTRI * 64];
  __shared__ double s_v[QMAX * 64];
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
  double* v = s_v + t;  // element r at v[r * 64]
  if (!bbh_joint_factor(L, 64, p, var[i], cross + i * p, s_cpp)) {
    scores[i] = NAN;  // not PSD even with jitter 1e-6
    return;
  }
  const double m0 = mean[i];
  if (kind == BBH_ACQ_QLOGEI) {
    // log-domain streaming form of bbh_qlogei_joint_lse: li_r = log_fatplus(g_r - best_f), fat maximum over the points,
    // log-sum-exp over the samples
    const double inv_tau = 1.0 / TAU_RELU;
    double sum = 0.0, ref = -INFINITY;
    for (int s = 0; s < S; s++) {
      const double* zs = z + (int64_t)s * q;
      double mx = -INFINITY;
#pragma unroll 1
      for (int r = 0; r < q; r++) {
        const double g = bbh_apply_objective(prog, bbh_joint_draw(L, 64, r, (r == 0) ? m0 : s_mp[r - 1], zs));
        const double li = log(TAU_RELU) + log(bbh_fatplus_core<2>((g - best_f) * inv_tau));
        v[r * 64] = li;
        mx = fmax(mx, li);
      }
      double acc = 0.0;
#pragma unroll 1
      for (int r = 0; r < q; r++) {
        const double u = 2.0 / (2.0 + (mx - v[r * 64]) / OBJ_TAU_MAX);
        acc = fma(u, u, acc);
      }
      const double fm = mx + OBJ_TAU_MAX * log(acc);
      if (fm > ref) {
        sum = sum * exp(ref - fm) + 1.0;
        ref = fm;
      } else {
        sum += exp(fm - ref);
      }
    }
    scores[i] = ref + log(sum) - log((double)S);
    return;
  }
  const bool centred = kind == BBH_ACQ_QUCB || kind == BBH_ACQ_QPSTD;
  if (centred) {  // per-point means of g over the samples
#pragma unroll 1
    for (int r = 0; r < q; r++) {
      const double mr = (r == 0) ? m0 : s_mp[r - 1];
      double acc = 0.0;
      for (int s = 0; s < S; s++) acc += bbh_apply_objective(prog, bbh_joint_draw(L, 64, r, mr, z + (int64_t)s * q));
      v[r * 64] = acc / (double)S;
    }
  }
  double sum = 0.0;
  for (int s = 0; s < S; s++) {
    const double* zs = z + (int64_t)s * q;
    double mx = -INFINITY;
#pragma unroll 1
    for (int r = 0; r < q; r++) {
      const double g = bbh_apply_objective(prog, bbh_joint_draw(L, 64, r, (r == 0) ? m0 : s_mp[r - 1], zs));
      mx = fmax(mx, bbh_mc_utility(kind, g, centred ? v[r * 64] : 0.0, best_f, cu));
    }
    sum += mx;
  }
  scores[i] = sum / (double)S;
}

static bool bbh_obj_prog_ok(const bbh_objective_prog* prog) {
  if (!prog || prog->n_ops < 1 || prog->n_ops > BBH_OBJ_MAX_OPS) return false;
  for (int k = 0; k < prog->n_ops; k++)
    if (prog->op[k] < BBH_OBJ_AFFINE || prog->op[k] > BBH_OBJ_SIGMOID) return false;
  return true;
}

extern "C" int bbh_mc_acq_obj_q1(bbh_handle* h, int32_t kind, const bbh_objective_prog* prog, const double* mean_dev,
                                 const double* var_dev, int64_t N, const double* z_host, int64_t S, double best_f, double beta,
                                 const uint8_t* alive_dev, double* scores_dev) {
  if (!h) return -1;
  if (kind < BBH_ACQ_QLOGEI || kind > BBH_ACQ_QPSTD || !bbh_obj_prog_ok(prog) || !mean_dev || !var_dev || !z_host || !scores_dev ||
      N < 0 || S < 1 || S > 8192) {
    h->err = "bbh_mc_acq_obj_q1: bad arguments (1 <= S <= 8192, 1 ... 8 operations)";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  const int rc = bbh_upload_z(h, z_host, (size_t)S);
  if (rc) return rc;
  bbh_timed_scope timed(h, BBH_TIMED_Q1);
  hipLaunchKernelGGL(bbh_obj_q1_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), sizeof(double) * S, h->stream, (int)kind, *prog,
                     mean_dev, var_dev, N, h->d_z, (int)S, best_f, bbh_mc_cu(kind, beta), alive_dev, scores_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

extern "C" int bbh_mc_acq_obj_pending(bbh_handle* h, int32_t kind, const bbh_objective_prog* prog, const double* mean_dev,
                                      const double* var_dev, const double* cross_dev, int64_t N, int64_t p,
                                      const double* mean_p_host, const double* cov_pp_host, const double* z_host, int64_t S,
                                      double best_f, double beta, const uint8_t* alive_dev, double* scores_dev) {
  if (!h) return -1;
  if (kind < BBH_ACQ_QLOGEI || kind > BBH_ACQ_QPSTD || !bbh_obj_prog_ok(prog) || !mean_dev || !var_dev || !cross_dev ||
      !mean_p_host || !cov_pp_host || !z_host || !scores_dev || N < 0 || S < 1 || p < 1 || p > BBH_MAX_PENDING) {
    h->err = "bbh_mc_acq_obj_pending: bad arguments (1 <= p <= 15 pending points, 1 ... 8 operations)";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  bbh_joint_dev d;
  const int rc = bbh_upload_joint(h, z_host, S, p, mean_p_host, cov_pp_host, false, &d);
  if (rc) return rc;
  bbh_timed_scope timed(h, BBH_TIMED_PENDING);
  hipLaunchKernelGGL(bbh_obj_pending_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, h->stream, (int)kind, *prog, mean_dev, var_dev,
                     cross_dev, N, (int)p, d.mean_p, d.cov_pp, d.z, (int)S, best_f, bbh_mc_cu(kind, beta), alive_dev, scores_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}
