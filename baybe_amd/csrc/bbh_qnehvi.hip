// The box-decomposition scorers of the noisy hypervolume pair (q' = 1), against the per-sample cell lists of bbh_nehvi.hip
// (bbh_cells_build_dev) or a caller's:
//
//   qLogNoisyExpectedHypervolumeImprovement: per MC sample, log-sum over the cells of that sample's box decomposition of
//     sum_o fatmin( log_fatplus(f_o - lo_o; tau_relu), loglen_o; tau_max ),  then logmeanexp over samples
//     (bbh_qlognehvi_lin_kernel: linear-domain sums, the default; bbh_qlognehvi_kernel: log domain, BBH_NEHVI_LOG=1);
//   qNoisyExpectedHypervolumeImprovement (plain): the same set-up (extended models, box decompositions, pruning, reference point)
//     scored without the smoothing -
//     score = (1/S) sum_s sum_{cells of s} prod_o max(min(f_s,o - lo_o, len_o), 0),   f_s,o = sign_o (E[f_o(x) | D, F_b,s,o] + sd_o z_x,s,o)
//     (oracle/nehvi_oracle.py::hvi_from_cells per sample; bbh_qnehvi_kernel).  Double precision throughout: unlike the log form
//     there is no power tau_max = 0.01 that would absorb single-precision factors.
//
// One thread per candidate (and sample slice: bbh_slices.h); the cell data is uniform across the wave (scalar / broadcast loads).
// Both families share the operand struct, the cell upload, the _cells front end and the launch; also here: the Pareto frequency of
// the baseline points (pruning).
#include <math.h>
#include <string.h>

#include <vector>

#include "bbh_acqmath.h"  // TAU_RELU, TAU_MAX, bbh_fatplus_core, bbh_safe_sd, bbh_fast_recip, bbh_fast_log_pos
#include "bbh_slices.h"

struct NehviArgs {
  bbh_targets t;
  int m;
  int64_t N;
  int S;
  const double* zx;        // [S, m]
  const int64_t* cell_off; // [S + 1]
  const double* cell_lo;   // [ncells, m]
  const double* cell_ll;   // [ncells, m] log side lengths (the plain form does not read them)
  int sample_major;        // t.tmat[o] is [S, N] (bbh_posterior_columns_sm) instead of [N, S]
  const uint8_t* alive;
  double* scores;
};

__device__ __forceinline__ double bbh_fatmin2(double a, double b) {
  // min(a,b) - tau log(1 + (alpha / (alpha + |a-b|/tau))^alpha), alpha = 2, tau = 1e-2
  const double mn = fmin(a, b);
  double diff = fabs(a - b);
  if (!(diff == diff)) diff = INFINITY;  // (-inf) - (-inf)
  // u = 2 / (2 + diff / tau) and log1p(u^2) through the short reciprocal / logarithm sequences (u^2 in (0, 1]:
  // forming 1 + u^2 costs at most 1e-16 absolute, times tau = 1e-2); diff = inf gives u = 0 exactly
  const double u = (diff < INFINITY) ? (2.0 * TAU_MAX) * bbh_fast_recip(fma(2.0, TAU_MAX, diff)) : 0.0;
  return fma(-TAU_MAX, bbh_fast_log_pos(fma(u, u, 1.0)), mn);
}

template <int M>
__global__ __launch_bounds__(256) void bbh_qlognehvi_kernel(const NehviArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.N) return;
  if (a.alive && !a.alive[i]) {
    a.scores[i] = -INFINITY;
    return;
  }
  double sd[M], sg[M];
  const double* trow[M];
#pragma unroll
  for (int o = 0; o < M; o++) {
    sd[o] = bbh_safe_sd(a.t.var[o][i]);
    sg[o] = a.t.sign[o];
    trow[o] = a.sample_major ? a.t.tmat[o] + i : a.t.tmat[o] + i * (int64_t)a.S;
  }
  const int64_t tstride = a.sample_major ? a.N : 1;
  const double inv_tau = 1.0 / TAU_RELU;
  const double log_tau = LOG_TAU_RELU;
  double sref = -INFINITY, ssum = 0.0;  // streaming log-sum-exp over MC samples
  for (int s = 0; s < a.S; s++) {
    double f[M];
#pragma unroll
    for (int o = 0; o < M; o++) f[o] = sg[o] * fma(sd[o], a.zx[(int64_t)s * M + o], trow[o][s * tstride]);
    double cref = -INFINITY, csum = 0.0;  // streaming log-sum-exp over the cells of this sample
    const int64_t c0 = a.cell_off[s], c1 = a.cell_off[s + 1];
    for (int64_t c = c0; c < c1; c++) {
      double la = 0.0;
#pragma unroll
      for (int o = 0; o < M; o++) {
        const double t = (f[o] - a.cell_lo[c * M + o]) * inv_tau;
        const double li = log_tau + bbh_fast_log_pos(bbh_fatplus_core(t));
        la += bbh_fatmin2(li, a.cell_ll[c * M + o]);
      }
      if (la > cref) {
        csum = csum * exp(cref - la) + 1.0;
        cref = la;
      } else if (la > -INFINITY) {
        csum += exp(la - cref);
      }
    }
    const double v = (cref > -INFINITY) ? cref + log(csum) : -INFINITY;
    if (v > sref) {
      ssum = ssum * exp(sref - v) + 1.0;
      sref = v;
    } else if (v > -INFINITY) {
      ssum += exp(v - sref);
    }
  }
  a.scores[i] = (sref > -INFINITY) ? sref + log(ssum) - log((double)a.S) : -INFINITY;
}

// The same value with the sums over cells and samples taken in the LINEAR domain:
//   score = log( (1/S) sum_s sum_c prod_o exp(fatmin(li_o, ll_o)) ),
//   exp(fatmin(a, b)) = min(e^a, e^b) (1 + u^2)^(-tau_max),  u = 2 tau_max / (2 tau_max + |a - b|),
// where e^a = tau_relu fatplus(t) is at hand BEFORE any logarithm is taken and e^b is the cell's side length.  Every term is a
// product of m side lengths >= ~1e-25 (the fat tail 0.1 tau_relu / (1 + t^2) at |t| <= 1e10), far inside the fp64 range, so
// nothing needs the log domain; what the log-domain form pays per (cell, target) - two double-precision logarithms, and per
// cell an exponential for the streaming log-sum-exp - shrinks to series and single-precision logarithms (see the loop body: the
// power tau_max = 0.01 absorbs their error).  BBH_NEHVI_LOG=1 selects the log-domain kernel (A/B, tests).
// One thread per candidate and SAMPLE SLICE (blockIdx.y of gridDim.y slices): with one thread per candidate a 1e5-row
// candidate set is 1563 wavefronts - 1.5 per SIMD, each a long dependent chain - and the kernel ran at a fifth of the VALU
// issue rate; the slices bring the launch to >= 8 waves per SIMD.  All lanes of a wave work on the same samples, so the
// cell data stays wave-uniform (scalar loads).  The slices' partial sums are combined in a fixed order by
// bbh_slices_finish_kernel (sums of positive terms in the linear domain: no atomics, reproducible).
// delta = 1 - (1 + u^2)^(-tau_max) <= 0.007 of TWO (cell, target) terms at once, in packed single precision (v_pk_fma_f32 /
// v_pk_mul_f32): the term is min(A, B) (1 - delta), so a relative error of ~1e-6 in delta is 7e-9 in the term - the same budget
// the double-precision form below spends on its single-precision logarithms.  rho = min / max, x1 = 1 - rho (taken in double
// precision, where it is exact next to rho = 1).  rho = 0 (cell unbounded above, or a ratio below the single-precision range):
// log2 -> -inf, |li - ll| = inf, u = 0, delta = 0.
__device__ __forceinline__ bbh_f2 bbh_fatmin_delta2(bbh_f2 rho, bbh_f2 x1) {
  bbh_f2 ds = x1 * (1.0f / 7.0f) + (1.0f / 6.0f);
  ds = ds * x1 + 0.2f;
  ds = ds * x1 + 0.25f;
  ds = ds * x1 + (1.0f / 3.0f);
  ds = ds * x1 + 0.5f;
  ds = ds * x1 + 1.0f;
  ds = ds * x1;  // -log1p(-x1), x1 < 0.15
  bbh_f2 dl;
  dl.x = -0.6931471805599453f * __log2f(rho.x);
  dl.y = -0.6931471805599453f * __log2f(rho.y);
  bbh_f2 den;
  den.x = (x1.x < 0.15f ? ds.x : dl.x) + (float)(2.0 * TAU_MAX);
  den.y = (x1.y < 0.15f ? ds.y : dl.y) + (float)(2.0 * TAU_MAX);
  bbh_f2 u;
  u.x = __builtin_amdgcn_rcpf(den.x);
  u.y = __builtin_amdgcn_rcpf(den.y);
  u = u * (float)(2.0 * TAU_MAX);
  const bbh_f2 w = u * u;
  bbh_f2 lps = w * -0.25f + (1.0f / 3.0f);
  lps = lps * w - 0.5f;
  lps = lps * w + 1.0f;
  lps = lps * w;  // log1p(w), w < 0.03
  bbh_f2 lp;
  lp.x = (w.x < 0.03f) ? lps.x : 0.6931471805599453f * __log2f(1.0f + w.x);
  lp.y = (w.y < 0.03f) ? lps.y : 0.6931471805599453f * __log2f(1.0f + w.y);
  const bbh_f2 x = lp * (float)TAU_MAX;  // in [0, 0.00694]
  bbh_f2 d = x * (-1.0f / 24.0f) + (1.0f / 6.0f);
  d = d * x - 0.5f;
  d = d * x + 1.0f;
  return d * x;  // 1 - exp(-x)
}

// PK: the (1 + u^2)^(-tau_max) factors in packed single precision, two cells at a time (default); PK = false is the double-precision
// sequence (BBH_NEHVI_PK=0: A/B, tests)
template <int M, bool PK>
__global__ __launch_bounds__(256) void bbh_qlognehvi_lin_kernel(const NehviArgs a, const double* __restrict__ cell_len,
                                                                double* __restrict__ partial) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.N) return;
  const bbh_slice sl = bbh_slice_bounds(a.S, bbh_slice_per(a.S), (int)blockIdx.y);
  if (a.alive && !a.alive[i]) {
    partial[(int64_t)blockIdx.y * a.N + i] = 0.0;
    return;
  }
  double sd[M], sg[M];
  const double* trow[M];
  const int64_t tstride = a.sample_major ? a.N : 1;  // between consecutive samples of this candidate
#pragma unroll
  for (int o = 0; o < M; o++) {
    sd[o] = bbh_safe_sd(a.t.var[o][i]);
    sg[o] = a.t.sign[o];
    trow[o] = a.sample_major ? a.t.tmat[o] + i : a.t.tmat[o] + i * (int64_t)a.S;
  }
  const double inv_tau = 1.0 / TAU_RELU;
  double total = 0.0;
  for (int s = sl.begin; s < sl.end; s++) {
    double f[M];
#pragma unroll
    for (int o = 0; o < M; o++) f[o] = sg[o] * fma(sd[o], a.zx[(int64_t)s * M + o], trow[o][s * tstride]);
    const int64_t c0 = a.cell_off[s], c1 = a.cell_off[s + 1];
    double ssum = 0.0;
    int64_t c = c0;
    if (PK) {
      for (; c < c1; c += 2) {
        const int64_t cb = (c + 1 < c1) ? c + 1 : c;  // odd cell count: the last cell is paired with itself, its twin is not added
        double pa = 1.0, pb = 1.0;
#pragma unroll
        for (int o = 0; o < M; o++) {
          double mn2[2];
          bbh_f2 rho, x1, rc;
#pragma unroll
          for (int h = 0; h < 2; h++) {
            const int64_t cc = h ? cb : c;
            const double B = cell_len[cc * M + o];
            const double A = TAU_RELU * bbh_fatplus_core<1>((f[o] - a.cell_lo[cc * M + o]) * inv_tau);
            const double mn = fmin(A, B), mxv = fmax(A, B);
            // rho = min / max and x1 = 1 - rho = (max - min) / max, each with its own relative accuracy (x1 next to rho = 1, where the
            // term is sensitive; rho next to 0, where delta ~ 1e-8 would vanish in 1 - x1): the difference in double precision,
            // the quotients in single precision - no double-precision reciprocal
            const float gap = (float)(mxv - mn), mnf = (float)mn, mxf = (float)mxv;
            mn2[h] = mn;
            if (h) {
              x1.y = gap;
              rho.y = mnf;
              rc.y = __builtin_amdgcn_rcpf(mxf);
            } else {
              x1.x = gap;
              rho.x = mnf;
              rc.x = __builtin_amdgcn_rcpf(mxf);
            }
          }
          x1 = x1 * rc;  // max = inf (cell unbounded above): inf * 0 = NaN -> 1;  rho = min * 0 = 0
          rho = rho * rc;
          x1.x = (x1.x == x1.x) ? x1.x : 1.0f;
          x1.y = (x1.y == x1.y) ? x1.y : 1.0f;
          const bbh_f2 dl = bbh_fatmin_delta2(rho, x1);
          pa *= fma(-mn2[0], (double)dl.x, mn2[0]);
          pb *= fma(-mn2[1], (double)dl.y, mn2[1]);
        }
        ssum += pa;
        if (c + 1 < c1) ssum += pb;
      }
    }
    for (; !PK && c < c1; c++) {
      double prod = 1.0;
#pragma unroll
      for (int o = 0; o < M; o++) {
        const double B = cell_len[c * M + o];
        const double fp = bbh_fatplus_core((f[o] - a.cell_lo[c * M + o]) * inv_tau);
        const double A = TAU_RELU * fp;
        // |li - ll| = -log(rho), rho = min(A, B) / max(A, B): a 7-term series of -log1p(-x) next to rho = 1 (x = 1 - rho <
        // 0.15, where the term is sensitive: d log(term) = u^3 d|li - ll|), single precision beyond (u < 0.11 there: an error of
        // 1e-7 moves the term by 1e-10 relative).  B = inf (cell unbounded above): rho = 0, u = 0.  No double-precision
        // logarithm is left: inside a wave some lane is nearly always close to rho = 1, so a wave-uniform skip never skipped.
        const double mn = fmin(A, B), mxv = fmax(A, B);
        double inv = __builtin_amdgcn_rcp(mxv);
        inv = fma(fma(-mxv, inv, 1.0), inv, inv);
        const double rho = (mxv < INFINITY) ? mn * inv : 0.0;
        const double x1 = 1.0 - rho;
        double ds = fma(x1, 1.0 / 7.0, 1.0 / 6.0);
        ds = fma(ds, x1, 0.2);
        ds = fma(ds, x1, 0.25);
        ds = fma(ds, x1, 1.0 / 3.0);
        ds = fma(ds, x1, 0.5);
        ds = fma(ds, x1, 1.0);
        ds *= x1;
        const double dl = -0.6931471805599453 * (double)__log2f((float)rho);  // rho = 0 -> inf
        const double diff = (x1 < 0.15) ? ds : dl;
        const double u = (2.0 * TAU_MAX) * __builtin_amdgcn_rcp(fma(2.0, TAU_MAX, diff));  // bare seed (2^-26); diff = inf -> 0
        const double w = u * u;
        // log1p(w), w in [0, 1]: series below 0.03 (error w^5 / 5 < 5e-9), single precision above (1.2e-7) - times tau_max = 0.01
        const double lps = w * fma(w, fma(w, fma(w, -0.25, 1.0 / 3.0), -0.5), 1.0);
        const double lpf = 0.6931471805599453 * (double)__log2f((float)(1.0 + w));
        const double lp = (w < 0.03) ? lps : lpf;
        const double x = TAU_MAX * lp;  // in [0, 0.00694]
        const double e = fma(x, fma(x, fma(x, fma(x, fma(x, -1.0 / 120.0, 1.0 / 24.0), -1.0 / 6.0), 0.5), -1.0), 1.0);  // exp(-x)
        prod *= mn * e;
      }
      ssum += prod;
    }
    total += ssum;
  }
  partial[(int64_t)blockIdx.y * a.N + i] = total;
}

namespace {

// The plain form.  A slice is a FIXED number of samples (not a function of the candidate count), so a candidate's score does not
// depend on how many rows are scored with it.
constexpr int QN_SLICE = 8;  // MC samples per slice

template <int M>
__global__ __launch_bounds__(256) void bbh_qnehvi_kernel(const NehviArgs a, const double* __restrict__ cell_len,
                                                         double* __restrict__ partial) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  const bbh_slice sl = bbh_slice_bounds(a.S, QN_SLICE, (int)blockIdx.y);
  if (a.alive && !a.alive[i]) {
    partial[(int64_t)blockIdx.y * a.N + i] = 0.0;
    return;
  }
  double sd[M];
#pragma unroll
  for (int o = 0; o < M; o++) sd[o] = bbh_safe_sd(a.t.var[o][i]);
  double total = 0.0;
  for (int s = sl.begin; s < sl.end; s++) {
    double f[M];
#pragma unroll
    for (int o = 0; o < M; o++) f[o] = a.t.sign[o] * fma(sd[o], a.zx[(int64_t)s * M + o], a.t.tmat[o][(int64_t)s * a.N + i]);
    const int64_t c0 = a.cell_off[s], c1 = a.cell_off[s + 1];
    double ssum = 0.0;
    for (int64_t c = c0; c < c1; c++) {
      double prod = 1.0;
#pragma unroll
      for (int o = 0; o < M; o++) prod *= fmax(fmin(f[o] - a.cell_lo[c * M + o], cell_len[c * M + o]), 0.0);
      ssum += prod;
    }
    total += ssum;
  }
  partial[(int64_t)blockIdx.y * a.N + i] = total;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// the arguments every entry point checks alike -> a (its cell operands are the caller's to set); the plain form is sample-major only
bool nehvi_args(NehviArgs& a, bool plain, int32_t m, int64_t N, const double* const* tmat_dev, const double* const* var_dev,
                const double* sign_host, const double* zx_host, int64_t S, const uint8_t* alive_dev, double* scores_dev, bool sample_major) {
  if (m < 1 || m > BBH_MAX_OBJECTIVES || N < 0 || S < 1 || (plain && S > 65535) || !tmat_dev || !var_dev || !sign_host || !zx_host ||
      !scores_dev || !bbh_fill_targets(a.t, m, N, tmat_dev, var_dev, sign_host))
    return false;
  a.m = m;
  a.N = N;
  a.S = (int)S;
  a.alive = alive_dev;
  a.scores = scores_dev;
  a.sample_major = sample_major ? 1 : 0;
  return true;
}

// launches with every operand on the device: a.zx, a.cell_off, a.cell_lo, a.cell_ll set by the caller, len_dev = side lengths
int nehvi_run(bbh_handle* h, const NehviArgs& a, const double* len_dev, bool plain) {
  const int64_t N = a.N, S = a.S;
  const dim3 grid((unsigned)((N + 255) / 256)), block(256);
  if (!plain && h->sw.nehvi_log) {  // log-domain sums, one thread per candidate over all samples
    bbh_timed_scope timed(h, BBH_TIMED_NEHVI);
    bbh_dispatch_m(a.m, [&](auto M) { hipLaunchKernelGGL(bbh_qlognehvi_kernel<decltype(M)::value>, grid, block, 0, h->stream, a); });
    BBH_HIP_TRY(h, hipGetLastError());
    return 0;
  }
  bbh_slicing sl = bbh_slices_by_len(S, QN_SLICE);
  if (!plain) {
    // sample slices: ~16 waves per SIMD (4 SIMDs per CU; 11.3 / 10.4 / 10.0 / 9.8 ms for 6 / 12 / 24 / 48 slices at 1e5 candidates), each slice at least 8 samples
    const int64_t srows = h->slice_rows > 0 ? h->slice_rows : N;
    int64_t slices = ((int64_t)16 * 4 * h->num_cu * 64 + srows - 1) / srows;
    if (h->sw.nehvi_slices != INT_MIN) slices = h->sw.nehvi_slices;
    if (slices > S / 8) slices = S / 8;
    if (slices > 64) slices = 64;
    if (slices < 1) slices = 1;
    sl = bbh_slices_by_count(S, slices);
  }
  int rc = bbh_ensure_ws(h, sizeof(double) * (size_t)sl.count * (size_t)N);
  if (rc) return rc;
  bbh_timed_scope timed(h, BBH_TIMED_NEHVI);
  const dim3 sgrid(grid.x, (unsigned)sl.count);
  bbh_dispatch_m(a.m, [&](auto Mc) {
    constexpr int M = decltype(Mc)::value;
    if (plain)
      hipLaunchKernelGGL(bbh_qnehvi_kernel<M>, sgrid, block, 0, h->stream, a, len_dev, h->d_ws);
    else
      bbh_dispatch_flag(h->sw.nehvi_pk, [&](auto PK) {
        hipLaunchKernelGGL((bbh_qlognehvi_lin_kernel<M, decltype(PK)::value>), sgrid, block, 0, h->stream, a, len_dev, h->d_ws);
      });
  });
  if (plain)
    bbh_slices_finish<BBH_FINISH_MEAN>(h, h->d_ws, sl.count, 1, N, S, a.alive, a.scores);
  else
    bbh_slices_finish<BBH_FINISH_LOG_MEAN>(h, h->d_ws, sl.count, 1, N, S, a.alive, a.scores);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

// a caller's cell lists: one upload, zx [S m] | cell_lo [ncells m] | cell_ll [ncells m] | cell_len [ncells m] | cell_off [S + 1]
// (int64, 8-byte slots; the plain form reads no cell_ll)
int nehvi_score_sm(bbh_handle* h, const char* name, NehviArgs& a, bool plain, const double* zx_host, const int64_t* cell_off_host,
                   const double* cell_lo_host, const double* cell_loglen_host) {
  const int64_t S = a.S, m = a.m, ncells = cell_off_host[S];
  if (ncells < 0 || (ncells > 0 && (!cell_lo_host || !cell_loglen_host))) {
    h->err = std::string(name) + ": inconsistent cell arrays";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  const size_t nd = (size_t)S * m + 3 * (size_t)ncells * m;
  std::vector<double> buf(nd + (size_t)S + 1);
  memcpy(buf.data(), zx_host, sizeof(double) * S * m);
  if (ncells > 0) {
    memcpy(buf.data() + S * m, cell_lo_host, sizeof(double) * ncells * m);
    memcpy(buf.data() + S * m + ncells * m, cell_loglen_host, sizeof(double) * ncells * m);
    double* len = buf.data() + S * m + 2 * ncells * m;  // side lengths e^ll (inf for cells unbounded above)
    for (int64_t e = 0; e < ncells * m; e++) len[e] = exp(cell_loglen_host[e]);
  }
  memcpy(buf.data() + nd, cell_off_host, sizeof(int64_t) * (S + 1));
  int rc = bbh_upload_z(h, buf.data(), buf.size());
  if (rc) return rc;
  a.zx = h->d_z;
  a.cell_lo = h->d_z + S * m;
  a.cell_ll = h->d_z + S * m + ncells * m;
  a.cell_off = (const int64_t*)(h->d_z + nd);
  return nehvi_run(h, a, h->d_z + S * m + 2 * ncells * m, plain);
}

int nehvi_log_sm(bbh_handle* h, int32_t m, int64_t N, const double* const* tmat_dev, const double* const* var_dev,
                 const double* sign_host, const double* zx_host, int64_t S, const int64_t* cell_off_host, const double* cell_lo_host,
                 const double* cell_loglen_host, const uint8_t* alive_dev, double* scores_dev, bool sample_major) {
  if (!h) return -1;
  NehviArgs a;
  if (!cell_off_host || !nehvi_args(a, false, m, N, tmat_dev, var_dev, sign_host, zx_host, S, alive_dev, scores_dev, sample_major)) {
    h->err = "bbh_qlognehvi: bad arguments (1 <= m <= 4)";
    return -1;
  }
  if (N == 0) return 0;
  return nehvi_score_sm(h, "bbh_qlognehvi", a, false, zx_host, cell_off_host, cell_lo_host, cell_loglen_host);
}

// the device-resident cell lists of bbh_cells_build_dev on this handle: only the candidate's base samples zx_host [S, m] travel
int nehvi_score_cells(bbh_handle* h, const char* name, bool plain, int32_t m, int64_t N, const double* const* tmat_dev,
                      const double* const* var_dev, const double* sign_host, const double* zx_host, int64_t S, const uint8_t* alive_dev,
                      double* scores_dev) {
  if (!h) return -1;
  const bbh_nehvi_state* st = (const bbh_nehvi_state*)h->nehvi_state;
  NehviArgs a;
  if (!st || st->S != S || st->m != m || !nehvi_args(a, plain, m, N, tmat_dev, var_dev, sign_host, zx_host, S, alive_dev, scores_dev, true)) {
    h->err = std::string(name) + ": bad arguments, or no cell lists for this S and m on the handle (bbh_cells_build_dev)";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  int rc = bbh_upload_z(h, zx_host, (size_t)S * m);
  if (rc) return rc;
  a.zx = h->d_z;
  a.cell_off = st->off();
  a.cell_lo = st->lo();
  a.cell_ll = st->ll();
  return nehvi_run(h, a, st->len(), plain);
}

}  // namespace

extern "C" int bbh_qlognehvi(bbh_handle* h, int32_t m, int64_t N, const double* const* tmat_dev,
                             const double* const* var_dev, const double* sign_host, const double* zx_host, int64_t S,
                             const int64_t* cell_off_host, const double* cell_lo_host, const double* cell_loglen_host,
                             const uint8_t* alive_dev, double* scores_dev) {
  return nehvi_log_sm(h, m, N, tmat_dev, var_dev, sign_host, zx_host, S, cell_off_host, cell_lo_host, cell_loglen_host, alive_dev, scores_dev,
                      false);
}

extern "C" int bbh_qlognehvi_sm(bbh_handle* h, int32_t m, int64_t N, const double* const* tmat_dev,
                                const double* const* var_dev, const double* sign_host, const double* zx_host, int64_t S,
                                const int64_t* cell_off_host, const double* cell_lo_host, const double* cell_loglen_host,
                                const uint8_t* alive_dev, double* scores_dev) {
  return nehvi_log_sm(h, m, N, tmat_dev, var_dev, sign_host, zx_host, S, cell_off_host, cell_lo_host, cell_loglen_host, alive_dev, scores_dev,
                      true);
}

extern "C" int bbh_qlognehvi_cells(bbh_handle* h, int32_t m, int64_t N, const double* const* tmat_dev,
                                   const double* const* var_dev, const double* sign_host, const double* zx_host, int64_t S,
                                   const uint8_t* alive_dev, double* scores_dev) {
  return nehvi_score_cells(h, "bbh_qlognehvi_cells", false, m, N, tmat_dev, var_dev, sign_host, zx_host, S, alive_dev, scores_dev);
}

extern "C" int bbh_qnehvi_cells(bbh_handle* h, int32_t m, int64_t N, const double* const* tmat_dev, const double* const* var_dev,
                                const double* sign_host, const double* zx_host, int64_t S, const uint8_t* alive_dev, double* scores_dev) {
  return nehvi_score_cells(h, "bbh_qnehvi_cells", true, m, N, tmat_dev, var_dev, sign_host, zx_host, S, alive_dev, scores_dev);
}

extern "C" int bbh_qnehvi_sm(bbh_handle* h, int32_t m, int64_t N, const double* const* tmat_dev, const double* const* var_dev,
                             const double* sign_host, const double* zx_host, int64_t S, const int64_t* cell_off_host,
                             const double* cell_lo_host, const double* cell_loglen_host, const uint8_t* alive_dev, double* scores_dev) {
  if (!h) return -1;
  NehviArgs a;
  if (!cell_off_host || !nehvi_args(a, true, m, N, tmat_dev, var_dev, sign_host, zx_host, S, alive_dev, scores_dev, true)) {
    h->err = "bbh_qnehvi_sm: bad arguments (1 <= m <= 4, 1 <= S <= 65535)";
    return -1;
  }
  if (N == 0) return 0;
  bool ok = cell_off_host[0] == 0;
  for (int64_t s = 0; ok && s < S; s++) ok = cell_off_host[s] <= cell_off_host[s + 1];  // (the kernel indexes the cell arrays by these)
  if (!ok) {
    h->err = "bbh_qnehvi_sm: inconsistent cell arrays";
    return -1;
  }
  return nehvi_score_sm(h, "bbh_qnehvi_sm", a, true, zx_host, cell_off_host, cell_lo_host, cell_loglen_host);
}

// ---- Pareto frequency of the baseline points over MC samples (pruning) ---------------------------
template <int M>
__global__ __launch_bounds__(256) void bbh_pareto_freq_kernel(const double* __restrict__ obj, int n, const double* __restrict__ ref,
                                                              unsigned long long* __restrict__ counts) {
  extern __shared__ double s_obj[];  // [n, M] of this sample
  const double* src = obj + (int64_t)blockIdx.x * n * M;
  for (int e = threadIdx.x; e < n * M; e += blockDim.x) s_obj[e] = src[e];
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    double yi[M];
    bool above = true;
#pragma unroll
    for (int o = 0; o < M; o++) {
      yi[o] = s_obj[i * M + o];
      above = above && (yi[o] > ref[o]);
    }
    bool dominated = false;
    for (int j = 0; j < n && !dominated; j++) {
      bool ge = true, gt = false;
#pragma unroll
      for (int o = 0; o < M; o++) {
        const double yj = s_obj[j * M + o];
        ge = ge && (yj >= yi[o]);
        gt = gt || (yj > yi[o]);
      }
      dominated = ge && gt;
    }
    if (above && !dominated) atomicAdd(&counts[i], 1ULL);
  }
}

static int bbh_pareto_frequency_impl(bbh_handle* h, const double* obj, bool on_device, int64_t S, int64_t n, int32_t m,
                                     const double* ref_host, int64_t* counts_host) {
  if (!h) return -1;
  if (!obj || !ref_host || !counts_host || S < 1 || n < 1 || n > 8192 / (m > 0 ? m : 1) || m < 1 ||
      m > BBH_MAX_OBJECTIVES) {
    h->err = "bbh_pareto_frequency: bad arguments (n * m <= 8192, 1 <= m <= 4)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  const size_t nobj = on_device ? 0 : (size_t)S * n * m;
  int rc = bbh_ensure_ws(h, sizeof(double) * (nobj + m + n));
  if (rc) return rc;
  double* d_obj = h->d_ws;
  double* d_ref = d_obj + nobj;
  unsigned long long* d_cnt = (unsigned long long*)(d_ref + m);
  if (!on_device) BBH_HIP_TRY(h, hipMemcpyAsync(d_obj, obj, sizeof(double) * nobj, hipMemcpyHostToDevice, h->stream));
  const double* src = on_device ? obj : d_obj;
  BBH_HIP_TRY(h, hipMemcpyAsync(d_ref, ref_host, sizeof(double) * m, hipMemcpyHostToDevice, h->stream));
  BBH_HIP_TRY(h, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * n, h->stream));
  const size_t lds = sizeof(double) * n * m;
  dim3 grid((unsigned)S), block(256);
  bbh_dispatch_m(m, [&](auto M) {
    hipLaunchKernelGGL(bbh_pareto_freq_kernel<decltype(M)::value>, grid, block, lds, h->stream, src, (int)n, d_ref, d_cnt);
  });
  BBH_HIP_TRY(h, hipGetLastError());
  BBH_HIP_TRY(h, hipMemcpyAsync(counts_host, d_cnt, sizeof(int64_t) * n, hipMemcpyDeviceToHost, h->stream));
  BBH_HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int bbh_pareto_frequency(bbh_handle* h, const double* obj_host, int64_t S, int64_t n, int32_t m,
                                    const double* ref_host, int64_t* counts_host) {
  return bbh_pareto_frequency_impl(h, obj_host, false, S, n, m, ref_host, counts_host);
}

// ... with the objective samples already on the device (bbh_nehvi_samples wrote them): nothing but the counts travels
extern "C" int bbh_pareto_frequency_dev(bbh_handle* h, const double* obj_dev, int64_t S, int64_t n, int32_t m,
                                        const double* ref_host, int64_t* counts_host) {
  return bbh_pareto_frequency_impl(h, obj_dev, true, S, n, m, ref_host, counts_host);
}
