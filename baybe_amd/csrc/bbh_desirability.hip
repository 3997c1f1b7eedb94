// MC acquisition functions of a DesirabilityObjective with one surrogate per target (the reference's default,
// as_pre_transformation=False: baybe/objectives/desirability.py:229-264).
//
// The reference fits one GP per target and hands the acquisition function an MC objective that maps every posterior sample
// [.., T] to one desirability value: per target the oriented transformation, then the weighted arithmetic or geometric mean.  So
// per candidate, base sample s and point r of the q'-batch [x_i ; pending]:
//     y_{r,t} = m_{r,t} + sum_c L_t[r, c] z[s, c, t]    T independent joint draws (bbh_joint.h: psd_safe_cholesky per target)
//     g_{r,t} = prog_t(y_{r,t})                         bbh_objective.h
//     d_r     = sum_t w_t g_{r,t}                       BBH_SCAL_MEAN
//             = exp(sum_t w_t log(g_{r,t} + 2^-52))     BBH_SCAL_GEOM_MEAN   (ascending t, products not fused: the host interpreter)
// and from there exactly what bbh_obj_q1_kernel / bbh_obj_pending_kernel (bbh_objacq.hip) do with d_r in the place of g.
//
// The T thread-private factors live in strided memory, in one of two storage classes that instantiate the same routines (so their
// operation order - and every bit of the result - is the same):
//     form 0  dynamic LDS, element e of target t of thread i at s_L[(t tri(q') + e) 64 + i]
//     form 1  a global workspace, element e of target t of row i at Lws[(t tri(q') + e) chunk + i], the rows walked in chunks
//             that keep the workspace bounded (as bbh_qlogei_pending_big)
// Behind the factors sit, in LDS in both forms, one row of q' doubles per thread (per-point values of the current sample, or the
// per-point sample means of qUCB / qPSTD) and the candidate's T means.
//
// The descriptor (bbh_desirability, 1.9 KB) is uploaded behind the base samples and read through a kernel-argument pointer at
// wave-uniform addresses: the loop over the targets stays a run-time loop (one copy of the program interpreter per call site, not
// eight), and nothing is indexed at run time in a by-value struct, so the kernels have no private segment.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "bbh_common.h"
#include "bbh_acqmath.h"    // TAU_RELU, bbh_fatplus_core, bbh_safe_sd, bbh_mc_utility, bbh_mc_cu
#include "bbh_joint.h"      // QMAX, tri, bbh_joint_factor, bbh_joint_draw
#include "bbh_objective.h"  // bbh_apply_objective

#define DES_TAU_MAX 1e-2
#define DES_EPS 2.220446049250313e-16  // 2^-52: torch.finfo(float64).eps, the reference's guard inside the logarithm
#define DES_WS_BYTES ((size_t)512 << 20)  // workspace bound of form 1 (env BBH_QBIG_WS_MB, shared with bbh_qlogei_pending_big)

// One target's contribution to the running scalarisation (ascending t; product and sum rounded separately).
__device__ __forceinline__ double bbh_des_accumulate(int scal, double acc, double w, double g) {
#pragma clang fp contract(off)
  const double term = (scal == BBH_SCAL_GEOM_MEAN) ? log(g + DES_EPS) : g;
  const double prod = w * term;
  return acc + prod;
}
__device__ __forceinline__ double bbh_des_finish(int scal, double acc) { return (scal == BBH_SCAL_GEOM_MEAN) ? exp(acc) : acc; }

// ---- q' = 1 -----------------------------------------------------------------------------------------------------------------
// One thread per candidate; its T means and standard deviations sit in LDS (a thread-private array under the run-time target index
// would live in scratch memory).  z [S, T] is read at wave-uniform addresses.
__global__ __launch_bounds__(256) void bbh_des_q1_kernel(int kind, const bbh_desirability* __restrict__ des,
                                                         const double* __restrict__ mean, const double* __restrict__ var, int64_t N,
                                                         const double* __restrict__ z, int S, double best_f, double cu,
                                                         const uint8_t* __restrict__ alive, double* __restrict__ scores) {
  __shared__ double s_a[BBH_DES_MAX_TARGETS * 256];
  __shared__ double s_b[BBH_DES_MAX_TARGETS * 256];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if (alive && !alive[i]) {
    scores[i] = -INFINITY;
    return;
  }
  const int T = des->n_targets, scal = des->scalarizer;
  double* a = s_a + threadIdx.x;  // target t at a[t * 256]
  double* b = s_b + threadIdx.x;
  for (int t = 0; t < T; t++) {
    a[t * 256] = mean[(int64_t)t * N + i];
    b[t * 256] = bbh_safe_sd(var[(int64_t)t * N + i]);
  }
  auto desirability = [&](int s) {
    const double* zs = z + (int64_t)s * T;
    double acc = 0.0;
#pragma unroll 1
    for (int t = 0; t < T; t++)
      acc = bbh_des_accumulate(scal, acc, des->weight[t], bbh_apply_objective(des->prog[t], fma(b[t * 256], zs[t], a[t * 256])));
    return bbh_des_finish(scal, acc);
  };
  double sum = 0.0;
  if (kind == BBH_ACQ_QLOGEI) {  // linear-domain sum: all terms positive (bbh_obj_q1_kernel)
    const double inv_tau = 1.0 / TAU_RELU;
#pragma unroll 1
    for (int s = 0; s < S; s++) sum += bbh_fatplus_core<2>((desirability(s) - best_f) * inv_tau);
    scores[i] = log(TAU_RELU) + log(sum) - log((double)S);
    return;
  }
  double m = 0.0;
  if (kind == BBH_ACQ_QUCB || kind == BBH_ACQ_QPSTD) {  // first pass: the sample mean of d
#pragma unroll 1
    for (int s = 0; s < S; s++) m += desirability(s);
    m /= (double)S;
  }
#pragma unroll 1
  for (int s = 0; s < S; s++) sum += bbh_mc_utility(kind, desirability(s), m, best_f, cu);
  scores[i] = sum / (double)S;
}

// ---- q' = 1 + p <= 16 ---------------------------------------------------------------------------------------------------------
// d_r of one sample: zs = this sample's base samples [T, q'] (the host transposes [S, q', T] on upload, so that every target's
// column block is contiguous as bbh_joint_draw reads it); m0: the candidate's means, target t at m0[t * 64].
template <typename ST>
__device__ __forceinline__ double bbh_des_point(const bbh_desirability* __restrict__ des, int T, int scal, const double* L, ST stride,
                                                int triq, int r, int q, const double* m0, const double* __restrict__ mean_p,
                                                const double* __restrict__ zs) {
  double acc = 0.0;
#pragma unroll 1
  for (int t = 0; t < T; t++) {
    const double m = (r == 0) ? m0[t * 64] : mean_p[t * (q - 1) + r - 1];
    const double y = bbh_joint_draw(L + (ST)(t * triq) * stride, stride, r, m, zs + t * q);
    acc = bbh_des_accumulate(scal, acc, des->weight[t], bbh_apply_objective(des->prog[t], y));
  }
  return bbh_des_finish(scal, acc);
}

// mean / var [T, ldn], cross [T, ldn, p]: the kernel scores the rows row0 ... row0 + nrows - 1 (one chunk of form 1; all rows in
// form 0).  Dynamic LDS: [WS ? 0 : T tri(q') 64 | q' 64 | T 64] doubles.
template <bool WS>
__global__ __launch_bounds__(64) void bbh_des_pending_kernel(int kind, const bbh_desirability* __restrict__ des,
                                                             const double* __restrict__ mean, const double* __restrict__ var,
                                                             const double* __restrict__ cross, int64_t ldn, int64_t row0,
                                                             int64_t nrows, int p, const double* __restrict__ mean_p,
                                                             const double* __restrict__ cov_pp, const double* __restrict__ z, int S,
                                                             double best_f, double cu, const uint8_t* __restrict__ alive,
                                                             double* __restrict__ scores, double* __restrict__ Lws, int64_t ws_stride) {
  extern __shared__ double s_dyn[];
  using ST = typename std::conditional<WS, int64_t, int>::type;
  const int tid = threadIdx.x;
  const int64_t local = (int64_t)blockIdx.x * 64 + tid;
  if (local >= nrows) return;
  const int64_t i = row0 + local;
  if (alive && !alive[i]) {
    scores[i] = -INFINITY;
    return;
  }
  const int T = des->n_targets, scal = des->scalarizer;
  const int q = p + 1, triq = q * (q + 1) / 2;
  double* L = WS ? Lws + local : s_dyn + tid;
  const ST stride = WS ? (ST)ws_stride : (ST)64;
  double* v = s_dyn + (WS ? 0 : T * triq * 64) + tid;  // point r at v[r * 64]
  double* m0 = v + q * 64;                             // target t at m0[t * 64]
  bool ok = true;
#pragma unroll 1
  for (int t = 0; t < T; t++) {
    const int64_t it = (int64_t)t * ldn + i;
    m0[t * 64] = mean[it];
    ok = bbh_joint_factor(L + (ST)(t * triq) * stride, stride, p, var[it], cross + it * p, cov_pp + t * p * p) && ok;
  }
  if (!ok) {
    scores[i] = NAN;  // a target's joint covariance is not PSD even with jitter 1e-6
    return;
  }
  const int Tq = T * q;
  if (kind == BBH_ACQ_QLOGEI) {  // log-domain streaming form with the fat maximum (bbh_obj_pending_kernel)
    const double inv_tau = 1.0 / TAU_RELU;
    double sum = 0.0, ref = -INFINITY;
#pragma unroll 1
    for (int s = 0; s < S; s++) {
      const double* zs = z + (int64_t)s * Tq;
      double mx = -INFINITY;
#pragma unroll 1
      for (int r = 0; r < q; r++) {
        const double d = bbh_des_point<ST>(des, T, scal, L, stride, triq, r, q, m0, mean_p, zs);
        const double li = log(TAU_RELU) + log(bbh_fatplus_core<2>((d - best_f) * inv_tau));
        v[r * 64] = li;
        mx = fmax(mx, li);
      }
      double acc = 0.0;
#pragma unroll 1
      for (int r = 0; r < q; r++) {
        const double u = 2.0 / (2.0 + (mx - v[r * 64]) / DES_TAU_MAX);
        acc = fma(u, u, acc);
      }
      const double fm = mx + DES_TAU_MAX * log(acc);
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
  if (centred) {  // per-point means of d over the samples
#pragma unroll 1
    for (int r = 0; r < q; r++) {
      double acc = 0.0;
#pragma unroll 1
      for (int s = 0; s < S; s++) acc += bbh_des_point<ST>(des, T, scal, L, stride, triq, r, q, m0, mean_p, z + (int64_t)s * Tq);
      v[r * 64] = acc / (double)S;
    }
  }
  double sum = 0.0;
#pragma unroll 1
  for (int s = 0; s < S; s++) {
    const double* zs = z + (int64_t)s * Tq;
    double mx = -INFINITY;
#pragma unroll 1
    for (int r = 0; r < q; r++) {
      const double d = bbh_des_point<ST>(des, T, scal, L, stride, triq, r, q, m0, mean_p, zs);
      mx = fmax(mx, bbh_mc_utility(kind, d, centred ? v[r * 64] : 0.0, best_f, cu));
    }
    sum += mx;
  }
  scores[i] = sum / (double)S;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static bool bbh_des_ok(const bbh_desirability* des) {
  if (!des || des->n_targets < 2 || des->n_targets > BBH_DES_MAX_TARGETS) return false;
  if (des->scalarizer != BBH_SCAL_MEAN && des->scalarizer != BBH_SCAL_GEOM_MEAN) return false;
  for (int t = 0; t < des->n_targets; t++) {
    const bbh_objective_prog& prog = des->prog[t];
    if (!(des->weight[t] == des->weight[t]) || prog.n_ops < 1 || prog.n_ops > BBH_OBJ_MAX_OPS) return false;
    for (int k = 0; k < prog.n_ops; k++)
      if (prog.op[k] < BBH_OBJ_AFFINE || prog.op[k] > BBH_OBJ_SIGMOID) return false;
  }
  return true;
}

static_assert(sizeof(bbh_desirability) % sizeof(double) == 0, "the descriptor rides behind the base samples as doubles");
#define DES_DOUBLES (sizeof(bbh_desirability) / sizeof(double))

// dynamic LDS of bbh_des_pending_kernel
static size_t bbh_des_lds_bytes(int T, int q, bool ws) {
  return sizeof(double) * 64 * ((ws ? 0 : (size_t)T * (q * (q + 1) / 2)) + (size_t)q + (size_t)T);
}

extern "C" int bbh_desirability_q1(bbh_handle* h, int32_t kind, const bbh_desirability* des, const double* mean_dev,
                                   const double* var_dev, int64_t N, const double* z_host, int64_t S, double best_f, double beta,
                                   const uint8_t* alive_dev, double* scores_dev) {
  if (!h) return -1;
  if (kind < BBH_ACQ_QLOGEI || kind > BBH_ACQ_QPSTD || !bbh_des_ok(des) || !mean_dev || !var_dev || !z_host || !scores_dev || N < 0 ||
      S < 1 || S > 8192) {
    h->err = "bbh_desirability_q1: bad arguments (2 ... 8 targets of 1 ... 8 operations, 1 <= S <= 8192)";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  const int T = des->n_targets;
  std::vector<double> buf((size_t)S * T + DES_DOUBLES);
  memcpy(buf.data(), z_host, sizeof(double) * S * T);
  memcpy(buf.data() + (size_t)S * T, des, sizeof(bbh_desirability));
  const int rc = bbh_upload_z(h, buf.data(), buf.size());
  if (rc) return rc;
  bbh_timed_scope timed(h, BBH_TIMED_Q1);
  hipLaunchKernelGGL(bbh_des_q1_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, (int)kind,
                     (const bbh_desirability*)(h->d_z + (size_t)S * T), mean_dev, var_dev, N, h->d_z, (int)S, best_f,
                     bbh_mc_cu(kind, beta), alive_dev, scores_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

extern "C" int bbh_desirability_pending(bbh_handle* h, int32_t kind, const bbh_desirability* des, const double* mean_dev,
                                        const double* var_dev, const double* cross_dev, int64_t N, int64_t p,
                                        const double* mean_p_host, const double* cov_pp_host, const double* z_host, int64_t S,
                                        double best_f, double beta, int32_t form, const uint8_t* alive_dev, double* scores_dev) {
  if (!h) return -1;
  if (kind < BBH_ACQ_QLOGEI || kind > BBH_ACQ_QPSTD || !bbh_des_ok(des) || !mean_dev || !var_dev || !cross_dev || !mean_p_host ||
      !cov_pp_host || !z_host || !scores_dev || N < 0 || S < 1 || p < 1 || p > BBH_MAX_PENDING || form < -1 || form > 1) {
    h->err = "bbh_desirability_pending: bad arguments (2 ... 8 targets of 1 ... 8 operations, 1 <= p <= 15 pending points, form -1, 0 or 1)";
    return -1;
  }
  const int T = des->n_targets, q = (int)p + 1;
  const bool lds_fits = bbh_des_lds_bytes(T, q, false) <= h->lds_per_block;
  if (form == 0 && !lds_fits) {
    h->err = "bbh_desirability_pending: bad arguments (the factors of form 0 do not fit the workgroup's LDS; use form 1 or -1)";
    return -1;
  }
  if (N == 0) return 0;
  const bool ws = form == 1 || (form == -1 && !lds_fits);
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  // one upload: [z [S, T, q'] (transposed from [S, q', T]) | mean_p [T, p] | cov_pp [T, p, p] | descriptor]
  const size_t nz = (size_t)S * T * q, nmp = (size_t)T * p, ncpp = (size_t)T * p * p;
  std::vector<double> buf(nz + nmp + ncpp + DES_DOUBLES);
  for (int64_t s = 0; s < S; s++)
    for (int c = 0; c < q; c++)
      for (int t = 0; t < T; t++) buf[((size_t)s * T + t) * q + c] = z_host[((size_t)s * q + c) * T + t];
  memcpy(buf.data() + nz, mean_p_host, sizeof(double) * nmp);
  memcpy(buf.data() + nz + nmp, cov_pp_host, sizeof(double) * ncpp);
  memcpy(buf.data() + nz + nmp + ncpp, des, sizeof(bbh_desirability));
  int rc = bbh_upload_z(h, buf.data(), buf.size());
  if (rc) return rc;
  const double *d_z = h->d_z, *d_mp = d_z + nz, *d_cpp = d_mp + nmp;
  const bbh_desirability* d_des = (const bbh_desirability*)(d_cpp + ncpp);
  const size_t lds = bbh_des_lds_bytes(T, q, ws);
  const double cu = bbh_mc_cu(kind, beta);
  if (!ws) {
    BBH_HIP_TRY(h, bbh_allow_lds(h->device, (const void*)bbh_des_pending_kernel<false>, lds));
    bbh_timed_scope timed(h, BBH_TIMED_PENDING);
    hipLaunchKernelGGL(bbh_des_pending_kernel<false>, dim3((unsigned)((N + 63) / 64)), dim3(64), lds, h->stream, (int)kind, d_des,
                       mean_dev, var_dev, cross_dev, N, (int64_t)0, N, (int)p, d_mp, d_cpp, d_z, (int)S, best_f, cu, alive_dev,
                       scores_dev, (double*)nullptr, (int64_t)0);
    BBH_HIP_TRY(h, hipGetLastError());
    h->last_des_form = 0;
    return 0;
  }
  // form 1: T tri(q') doubles per row; the rows are walked in chunks (multiples of 64) whose workspace stays below the bound, every
  // chunk addressing the workspace from 0
  const size_t per_row = sizeof(double) * (size_t)T * (size_t)(q * (q + 1) / 2);
  const size_t ws_bound = h->sw.qbig_ws_mb ? (size_t)h->sw.qbig_ws_mb << 20 : DES_WS_BYTES;
  int64_t chunk = (int64_t)(ws_bound / per_row) / 64 * 64;
  if (chunk < 64) chunk = 64;
  if (chunk > N) chunk = N;
  rc = bbh_ensure_ws(h, per_row * (size_t)chunk);
  if (rc) return rc;
  bbh_timed_scope timed(h, BBH_TIMED_PENDING);
  for (int64_t c0 = 0; c0 < N; c0 += chunk) {
    const int64_t nc = std::min(chunk, N - c0);
    hipLaunchKernelGGL(bbh_des_pending_kernel<true>, dim3((unsigned)((nc + 63) / 64)), dim3(64), lds, h->stream, (int)kind, d_des, mean_dev,
                       var_dev, cross_dev, N, c0, nc, (int)p, d_mp, d_cpp, d_z, (int)S, best_f, cu, alive_dev, scores_dev, h->d_ws, chunk);
  }
  BBH_HIP_TRY(h, hipGetLastError());
  h->last_des_form = 1;
  return 0;
}

extern "C" int bbh_desirability_last_form(bbh_handle* h) { return h ? h->last_des_form : -1; }
