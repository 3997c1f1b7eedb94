// qExpectedHypervolumeImprovement / qLogExpectedHypervolumeImprovement (baybe/acquisition/acqfs.py:429-464) on the device.
//
// Unlike the noisy pair (bbh_nehvi.hip, bbh_qnehvi.hip) there is ONE cell list per recommendation - the box decomposition of the
// models' oriented posterior means at the measurement rows (baybe/acquisition/_builder.py:286-299, acquisition/utils.py:26-84) -
// and the pending points are not cached into a baseline: every candidate scores the joint batch [x_i ; pending] of q' = 1 + p
// points by inclusion-exclusion over its non-empty subsets.  Per candidate, base sample s, point r and target j:
//     y[r, j] = m[r, j] + sum_c L_j[r, c] z[s, c, j]      m independent joint draws (bbh_joint.h: psd_safe_cholesky per target)
// (every operand arrives oriented: include/baybe_hip.h) and per cell (lo, up):
//     plain   a[r, j] = min(y[r, j], up_j) - lo_j;                    cell = sum_A (-1)^(|A|+1) prod_j max(0, min_{r in A} a[r, j])
//     log     a[r, j] = log_fatplus(y[r, j] - lo_j; 1e-6);            t_A = sum_j fatmin2(fatmin_{r in A} a[r, j], log(min(up_j, 1e10) - lo_j))
//             cell = logdiffexp(logaddexp_{odd i} lse_i, logaddexp_{even i} lse_i),   lse_i = logsumexp_{|A| = i} t_A
// then the sum (logsumexp) over the cells and the mean (logmeanexp) over the samples.  The q' m per-point quantities a are computed
// once per sample and cell; the subsets are then walked by ascending size, lexicographically within a size, from a table of bit
// masks the host builds - that order fixes the bits.  The odd - even difference cancels up to 2^q'-fold where the points coincide,
// so everything is double precision (the packed-single factors of the qLogNEHVI cell kernel have no place here).
//
// Layout.  One thread per candidate and sample slice: grid (rows, slices), a slice being a fixed number of samples (EH_SLICE, so a
// candidate's bits do not depend on how many rows are scored with it).  Each slice leaves a partial - the plain sum, or the
// (reference, sum) pair of its streaming logsumexp - and a finish kernel combines the partials in slice order: no atomics, two
// runs give the same bits.  Cells, base samples, pending statistics and the subset table ride in one upload and are read at
// wave-uniform addresses (scalar loads).  Per thread, strided by the workgroup's 64 lanes (conflict-free 8-byte LDS accesses):
//     m tri(q') factor elements     form 0: dynamic LDS;  form 1: a chunked global workspace (one copy per slice) - same routines,
//                                   same bits (the template on the stride type of bbh_joint.h)
//     q' m draws y, q' m values a, m candidate means:  LDS in both forms
// Nothing is indexed at run time in a thread-private array, so the kernels have no private segment (bbh_desirability.hip).
// Form 0 is legal where a workgroup needs at most EH_LDS_BYTES (half of gfx950's 160 KB: two workgroups per CU; sized on paper).
// Form -1 takes the workspace form: at 1e5 rows it measured 1.2 - 2.6 times faster than form 0, whose LDS footprint leaves a CU
// with one to eight 64-thread workgroups (KERNELS.md 4.14).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "bbh_common.h"
#include "bbh_acqmath.h"  // TAU_RELU, TAU_MAX, bbh_fatplus_core, bbh_safe_sd
#include "bbh_joint.h"    // tri, bbh_joint_factor, bbh_joint_draw
#include "bbh_slices.h"   // slice bounds, finish kernel, dispatch

namespace {

constexpr int EH_SLICE = 16;                            // MC samples per slice (env BBH_EHVI_SLICE; 0: all samples in one slice)
constexpr double EH_UPPER_CLAMP = 1e10;                 // cell_upper_bounds.clamp_max(1e10) in the log form
constexpr size_t EH_LDS_BYTES = (size_t)80 << 10;       // form 0: at most this much LDS per workgroup
constexpr size_t EH_WS_BYTES = (size_t)512 << 20;       // workspace bound of form 1 (env BBH_QBIG_WS_MB)
constexpr int EH_TAB_MASKS = 16;                        // subset table: tab[i] = number of subsets of size i (i <= 8), masks from tab[16]
constexpr int EH_TAB_INTS = EH_TAB_MASKS + 256;

struct EhCells {
  const double *lo, *up, *ll;  // [C, m]; ll = log(min(up, 1e10) - lo)
  int C;
};

__device__ __forceinline__ double eh_log_fatplus(double x) { return LOG_TAU_RELU + log(bbh_fatplus_core<2>(x * (1.0 / TAU_RELU))); }

// fatmin over the pair (a, b), both finite: -fatmax(-a, -b) with tau_max and alpha = 2
__device__ __forceinline__ double eh_fatmin2(double a, double b) {
  const double u = 2.0 / (2.0 + fabs(a - b) / TAU_MAX);
  return fmin(a, b) - TAU_MAX * log1p(u * u);
}

// streaming logsumexp: (ref, sum) with value ref + log(sum), started at (-inf, 0); a NaN term makes the sum NaN
__device__ __forceinline__ void eh_lse_add(double& ref, double& sum, double v) {
  if (v > ref) {
    sum = sum * exp(ref - v) + 1.0;
    ref = v;
  } else {
    sum += (v == -INFINITY) ? 0.0 : exp(v - ref);
  }
}

__device__ __forceinline__ double eh_logaddexp(double a, double b) {
  const double mx = fmax(a, b), mn = fmin(a, b);
  return (mx == -INFINITY) ? mx : mx + log1p(exp(mn - mx));
}

// log(e^a - e^b) = a + log1mexp(b - a)
__device__ __forceinline__ double eh_logdiffexp(double a, double b) {
  const double x = b - a;
  return a + ((x > -0.6931471805599453) ? log(-expm1(x)) : log1p(-exp(x)));
}

// partials of slice k: plain [k 2 N + i] = the slice's sum; log [k 2 N + i], [(k 2 + 1) N + i] = (reference, sum)
template <bool LOG>
__device__ __forceinline__ void eh_store_partial(double* __restrict__ partial, int64_t N, int64_t i, int k, double a, double b) {
  partial[(int64_t)(2 * k) * N + i] = a;
  if (LOG) partial[(int64_t)(2 * k + 1) * N + i] = b;
}

// ---- q' = 1 -----------------------------------------------------------------------------------------------------------------
template <int M, bool LOG>
__global__ __launch_bounds__(256) void bbh_ehvi_q1_kernel(const double* __restrict__ mean, const double* __restrict__ var, int64_t N,
                                                          const double* __restrict__ z, int S, int slice, const EhCells cells,
                                                          const uint8_t* __restrict__ alive, double* __restrict__ partial) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  if (alive && !alive[i]) return;  // (the finish kernel writes -inf without reading the partials)
  const int k = (int)blockIdx.y;
  const bbh_slice sl = bbh_slice_bounds(S, slice, k);
  double mu[M], sd[M];
#pragma unroll
  for (int o = 0; o < M; o++) {
    mu[o] = mean[(int64_t)o * N + i];
    sd[o] = bbh_safe_sd(var[(int64_t)o * N + i]);
  }
  double ref = -INFINITY, sum = 0.0;
#pragma unroll 1
  for (int s = sl.begin; s < sl.end; s++) {
    double y[M];
#pragma unroll
    for (int o = 0; o < M; o++) y[o] = fma(sd[o], z[(int64_t)s * M + o], mu[o]);
    if (LOG) {
      double cref = -INFINITY, csum = 0.0;
#pragma unroll 1
      for (int c = 0; c < cells.C; c++) {
        double la = 0.0;
#pragma unroll
        for (int o = 0; o < M; o++) la += eh_fatmin2(eh_log_fatplus(y[o] - cells.lo[c * M + o]), cells.ll[c * M + o]);
        eh_lse_add(cref, csum, la);
      }
      eh_lse_add(ref, sum, cref + log(csum));
    } else {
      double ssum = 0.0;
#pragma unroll 1
      for (int c = 0; c < cells.C; c++) {
        double prod = 1.0;
#pragma unroll
        for (int o = 0; o < M; o++) prod *= fmax(fmin(y[o], cells.up[c * M + o]) - cells.lo[c * M + o], 0.0);
        ssum += prod;
      }
      sum += ssum;
    }
  }
  eh_store_partial<LOG>(partial, N, i, k, LOG ? ref : sum, sum);
}

// ---- q' = 1 + p <= 8 ----------------------------------------------------------------------------------------------------------
// mean / var [m, ldn], cross [m, ldn, p]: the launch scores the rows row0 ... row0 + nrows - 1 (one chunk of form 1; all rows in
// form 0).  z [S, m, q'] (the host transposes [S, q', m] on upload: every target's column block contiguous, as bbh_joint_draw reads
// it).  Dynamic LDS: [WS ? 0 : m tri(q') 64 | q' m 64 | q' m 64 | m 64] doubles.
template <bool WS, bool LOG>
__global__ __launch_bounds__(64) void bbh_ehvi_pending_kernel(int m, const double* __restrict__ mean, const double* __restrict__ var,
                                                              const double* __restrict__ cross, int64_t ldn, int64_t row0, int64_t nrows,
                                                              int p, const double* __restrict__ mean_p, const double* __restrict__ cov_pp,
                                                              const double* __restrict__ z, int S, int slice, const EhCells cells,
                                                              const int* __restrict__ tab, const uint8_t* __restrict__ alive,
                                                              double* __restrict__ partial, double* __restrict__ Lws, int64_t chunk,
                                                              int64_t ws_stride) {
  extern __shared__ double s_dyn[];
  using ST = typename std::conditional<WS, int64_t, int>::type;
  const int tid = threadIdx.x;
  const int64_t local = (int64_t)blockIdx.x * 64 + tid;
  if (local >= nrows) return;
  const int64_t i = row0 + local;
  if (alive && !alive[i]) return;
  const int k = (int)blockIdx.y;
  const bbh_slice sl = bbh_slice_bounds(S, slice, k);
  const int q = p + 1, triq = q * (q + 1) / 2, qm = q * m;
  double* L = WS ? Lws + (int64_t)k * chunk + local : s_dyn + tid;
  const ST stride = WS ? (ST)ws_stride : (ST)64;
  double* yv = s_dyn + (WS ? 0 : m * triq * 64) + tid;  // draw of point r, target j at yv[(r m + j) 64]
  double* av = yv + qm * 64;                            // its per-cell quantity at av[(r m + j) 64]
  double* m0 = av + qm * 64;                            // the candidate's mean of target j at m0[j 64]
  bool ok = true;
#pragma unroll 1
  for (int j = 0; j < m; j++) {
    const int64_t ij = (int64_t)j * ldn + i;
    m0[j * 64] = mean[ij];
    ok = bbh_joint_factor(L + (ST)(j * triq) * stride, stride, p, var[ij], cross + ij * p, cov_pp + j * p * p) && ok;
  }
  if (!ok) {  // a target's joint covariance is not PSD even with jitter 1e-6
    eh_store_partial<LOG>(partial, ldn, i, k, LOG ? 0.0 : NAN, NAN);
    return;
  }
  double ref = -INFINITY, sum = 0.0;
#pragma unroll 1
  for (int s = sl.begin; s < sl.end; s++) {
    const double* zs = z + (int64_t)s * qm;
#pragma unroll 1
    for (int j = 0; j < m; j++) {
#pragma unroll 1
      for (int r = 0; r < q; r++) {
        const double mr = (r == 0) ? m0[j * 64] : mean_p[j * p + r - 1];
        yv[(r * m + j) * 64] = bbh_joint_draw(L + (ST)(j * triq) * stride, stride, r, mr, zs + j * q);
      }
    }
    double cref = -INFINITY, csum = 0.0;  // over the cells of this sample (plain: csum alone)
#pragma unroll 1
    for (int c = 0; c < cells.C; c++) {
      const double *lo = cells.lo + c * m, *up = cells.up + c * m, *ll = cells.ll + c * m;
#pragma unroll 1
      for (int r = 0; r < q; r++) {
#pragma unroll 1
        for (int j = 0; j < m; j++) {
          const double y = yv[(r * m + j) * 64];
          av[(r * m + j) * 64] = LOG ? eh_log_fatplus(y - lo[j]) : fmin(y, up[j]) - lo[j];
        }
      }
      const int* mask = tab + EH_TAB_MASKS;
      double odd = LOG ? -INFINITY : 0.0, even = odd;  // plain: the sums of the odd and the even sizes
#pragma unroll 1
      for (int size = 1; size <= q; size++) {
        const int n = tab[size];
        double zref = -INFINITY, zsum = 0.0;  // over the subsets of this size (plain: zsum alone)
#pragma unroll 1
        for (int t = 0; t < n; t++) {
          const int A = *mask++;
          double acc = LOG ? 0.0 : 1.0;  // sum (log) or product (plain) over the targets
#pragma unroll 1
          for (int j = 0; j < m; j++) {
            double mn = INFINITY;
            for (int bits = A; bits; bits &= bits - 1) mn = fmin(mn, av[(__builtin_ctz(bits) * m + j) * 64]);
            if (LOG) {
              if (size > 1) {  // fat minimum of the members (one member: the value itself)
                double w = 0.0;
                for (int bits = A; bits; bits &= bits - 1) {
                  const double u = 2.0 / (2.0 + (av[(__builtin_ctz(bits) * m + j) * 64] - mn) / TAU_MAX);
                  w = fma(u, u, w);
                }
                mn -= TAU_MAX * log(w);
              }
              acc += eh_fatmin2(mn, ll[j]);
            } else {
              acc *= fmax(mn, 0.0);
            }
          }
          if (LOG)
            eh_lse_add(zref, zsum, acc);
          else
            zsum += acc;
        }
        if (LOG) {
          const double v = zref + log(zsum);
          if (size & 1)
            odd = eh_logaddexp(odd, v);
          else
            even = eh_logaddexp(even, v);
        } else {
          if (size & 1)
            odd += zsum;
          else
            even += zsum;
        }
      }
      if (LOG)
        eh_lse_add(cref, csum, eh_logdiffexp(odd, even));
      else
        csum += odd - even;
    }
    if (LOG)
      eh_lse_add(ref, sum, cref + log(csum));
    else
      sum += csum;
  }
  eh_store_partial<LOG>(partial, ldn, i, k, LOG ? ref : sum, sum);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
bool eh_cells_ok(int m, const double* lo, const double* up, int64_t C) {
  if (!lo || !up || C < 1 || C > (1 << 20)) return false;
  for (int64_t e = 0; e < C * m; e++)
    if (!(lo[e] > -INFINITY) || !(up[e] > lo[e])) return false;  // (NaN fails both; up may be +inf)
  return true;
}

// [lo | up | ll] behind `at` doubles of buf
void eh_put_cells(std::vector<double>& buf, size_t at, int m, const double* lo, const double* up, int64_t C) {
  const size_t n = (size_t)C * m;
  memcpy(buf.data() + at, lo, sizeof(double) * n);
  memcpy(buf.data() + at + n, up, sizeof(double) * n);
  for (size_t e = 0; e < n; e++) buf[at + 2 * n + e] = log(std::min(up[e], EH_UPPER_CLAMP) - lo[e]);
}

// the non-empty subsets of {0 ... q - 1} as bit masks: ascending size, lexicographic within a size (itertools.combinations)
void eh_subset_table(int q, int* tab) {
  memset(tab, 0, sizeof(int) * EH_TAB_INTS);
  int at = EH_TAB_MASKS;
  for (int size = 1; size <= q; size++) {
    int idx[BBH_EHVI_MAX_Q];
    for (int a = 0; a < size; a++) idx[a] = a;
    for (;;) {
      int mask = 0;
      for (int a = 0; a < size; a++) mask |= 1 << idx[a];
      tab[at++] = mask;
      tab[size]++;
      int a = size - 1;
      while (a >= 0 && idx[a] == q - size + a) a--;
      if (a < 0) break;
      idx[a]++;
      for (int b = a + 1; b < size; b++) idx[b] = idx[b - 1] + 1;
    }
  }
}

int eh_slice_len(const bbh_handle* h, int64_t S) {
  const int sw = h->sw.ehvi_slice;
  return (sw == INT_MIN) ? EH_SLICE : (sw <= 0 ? (int)S : sw);
}

size_t eh_lds_bytes(int m, int q, bool ws) {
  return sizeof(double) * 64 * ((ws ? 0 : (size_t)m * (q * (q + 1) / 2)) + 2 * (size_t)q * m + (size_t)m);
}

// the slices' partials (two rows per slice) in slice order -> score
template <bool LOG>
void eh_finish(bbh_handle* h, const double* partial, int slices, int64_t N, int64_t S, const uint8_t* alive_dev, double* scores_dev) {
  bbh_slices_finish<LOG ? BBH_FINISH_LSE_PAIRS : BBH_FINISH_MEAN>(h, partial, slices, 2, N, S, alive_dev, scores_dev);
}

template <int M, bool LOG>
void eh_launch_q1(bbh_handle* h, const double* mean_dev, const double* var_dev, int64_t N, const double* d_z, int S, int slice, int slices,
                  const EhCells& cells, const uint8_t* alive_dev, double* scores_dev) {
  hipLaunchKernelGGL((bbh_ehvi_q1_kernel<M, LOG>), dim3((unsigned)((N + 255) / 256), (unsigned)slices), dim3(256), 0, h->stream, mean_dev,
                     var_dev, N, d_z, S, slice, cells, alive_dev, h->d_ws);
  eh_finish<LOG>(h, h->d_ws, slices, N, S, alive_dev, scores_dev);
}

template <bool WS, bool LOG>
hipError_t eh_launch_pending(bbh_handle* h, size_t lds, int64_t nrows, int slices, int m, const double* mean_dev, const double* var_dev,
                             const double* cross_dev, int64_t N, int64_t row0, int p, const double* d_mp, const double* d_cpp,
                             const double* d_z, int S, int slice, const EhCells& cells, const int* d_tab, const uint8_t* alive_dev,
                             double* partial, double* Lws, int64_t chunk) {
  const hipError_t e = bbh_allow_lds(h->device, (const void*)bbh_ehvi_pending_kernel<WS, LOG>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((bbh_ehvi_pending_kernel<WS, LOG>), dim3((unsigned)((nrows + 63) / 64), (unsigned)slices), dim3(64), lds, h->stream, m,
                     mean_dev, var_dev, cross_dev, N, row0, nrows, p, d_mp, d_cpp, d_z, S, slice, cells, d_tab, alive_dev, partial, Lws,
                     chunk, chunk * slices);
  return hipSuccess;
}

}  // namespace

extern "C" int bbh_ehvi_q1(bbh_handle* h, int32_t log, int32_t m, const double* mean_dev, const double* var_dev, int64_t N,
                           const double* cell_lo_host, const double* cell_up_host, int64_t C, const double* z_host, int64_t S,
                           const uint8_t* alive_dev, double* scores_dev) {
  if (!h) return -1;
  if (m < 2 || m > BBH_MAX_OBJECTIVES || !mean_dev || !var_dev || !z_host || !scores_dev || N < 0 || S < 1 || S > 8192 ||
      !eh_cells_ok(m, cell_lo_host, cell_up_host, C)) {
    h->err = "bbh_ehvi_q1: bad arguments (2 ... 4 targets, 1 <= S <= 8192, at least one cell, finite lower bounds below the upper ones)";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  const size_t nz = (size_t)S * m, nc = (size_t)C * m;
  std::vector<double> buf(nz + 3 * nc);
  memcpy(buf.data(), z_host, sizeof(double) * nz);
  eh_put_cells(buf, nz, m, cell_lo_host, cell_up_host, C);
  int rc = bbh_upload_z(h, buf.data(), buf.size());
  if (rc) return rc;
  const bbh_slicing sl = bbh_slices_by_len(S, eh_slice_len(h, S));
  rc = bbh_ensure_ws(h, sizeof(double) * 2 * (size_t)sl.count * (size_t)N);
  if (rc) return rc;
  const EhCells cells = {h->d_z + nz, h->d_z + nz + nc, h->d_z + nz + 2 * nc, (int)C};
  bbh_timed_scope timed(h, BBH_TIMED_Q1);
  bbh_dispatch_m<2>(m, [&](auto M) {
    bbh_dispatch_flag(log != 0, [&](auto LOG) {
      eh_launch_q1<decltype(M)::value, decltype(LOG)::value>(h, mean_dev, var_dev, N, h->d_z, (int)S, sl.per, sl.count, cells, alive_dev,
                                                             scores_dev);
    });
  });
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

extern "C" int bbh_ehvi_pending(bbh_handle* h, int32_t log, int32_t m, const double* mean_dev, const double* var_dev,
                                const double* cross_dev, int64_t N, int64_t p, const double* mean_p_host, const double* cov_pp_host,
                                const double* cell_lo_host, const double* cell_up_host, int64_t C, const double* z_host, int64_t S,
                                int32_t form, const uint8_t* alive_dev, double* scores_dev) {
  if (!h) return -1;
  if (m < 2 || m > BBH_MAX_OBJECTIVES || !mean_dev || !var_dev || !cross_dev || !mean_p_host || !cov_pp_host || !z_host || !scores_dev ||
      N < 0 || S < 1 || S > 8192 || p < 1 || p > BBH_EHVI_MAX_Q - 1 || form < -1 || form > 1 ||
      !eh_cells_ok(m, cell_lo_host, cell_up_host, C)) {
    h->err = "bbh_ehvi_pending: bad arguments (2 ... 4 targets, 1 <= p <= 7 pending points, 1 <= S <= 8192, at least one cell, form -1, 0 or 1)";
    return -1;
  }
  const int q = (int)p + 1;
  const size_t lds_budget = std::min(h->lds_per_block, EH_LDS_BYTES);
  const bool lds_fits = eh_lds_bytes(m, q, false) <= lds_budget;
  if (form == 0 && !lds_fits) {
    h->err = "bbh_ehvi_pending: bad arguments (the factors of form 0 do not fit the workgroup's share of the LDS; use form 1 or -1)";
    return -1;
  }
  if (N == 0) return 0;
  const bool ws = form != 0;  // form -1: the workspace form measured faster at every shape tried (KERNELS.md 4.14)
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  // one upload: [z [S, m, q'] (transposed from [S, q', m]) | mean_p [m, p] | cov_pp [m, p, p] | lo, up, ll [C, m] each | subset table]
  const size_t nz = (size_t)S * m * q, nmp = (size_t)m * p, ncpp = (size_t)m * p * p, nc = (size_t)C * m;
  static_assert(EH_TAB_INTS % 2 == 0, "the subset table rides behind the cells in 8-byte slots");
  std::vector<double> buf(nz + nmp + ncpp + 3 * nc + EH_TAB_INTS / 2);
  for (int64_t s = 0; s < S; s++)
    for (int c = 0; c < q; c++)
      for (int t = 0; t < m; t++) buf[((size_t)s * m + t) * q + c] = z_host[((size_t)s * q + c) * m + t];
  memcpy(buf.data() + nz, mean_p_host, sizeof(double) * nmp);
  memcpy(buf.data() + nz + nmp, cov_pp_host, sizeof(double) * ncpp);
  eh_put_cells(buf, nz + nmp + ncpp, m, cell_lo_host, cell_up_host, C);
  int tab[EH_TAB_INTS];
  eh_subset_table(q, tab);
  memcpy(buf.data() + nz + nmp + ncpp + 3 * nc, tab, sizeof(tab));
  int rc = bbh_upload_z(h, buf.data(), buf.size());
  if (rc) return rc;
  const double *d_z = h->d_z, *d_mp = d_z + nz, *d_cpp = d_mp + nmp, *d_cells = d_cpp + ncpp;
  const EhCells cells = {d_cells, d_cells + nc, d_cells + 2 * nc, (int)C};
  const int* d_tab = (const int*)(d_cells + 3 * nc);
  const bbh_slicing sl = bbh_slices_by_len(S, eh_slice_len(h, S));
  const int slice = sl.per, slices = sl.count;
  const size_t lds = eh_lds_bytes(m, q, ws);
  const size_t npartial = 2 * (size_t)slices * (size_t)N;
  if (!ws) {
    rc = bbh_ensure_ws(h, sizeof(double) * npartial);
    if (rc) return rc;
    bbh_timed_scope timed(h, BBH_TIMED_PENDING);
    const hipError_t launched = bbh_dispatch_flag(log != 0, [&](auto LOG) {
      constexpr bool L = decltype(LOG)::value;
      const hipError_t e = eh_launch_pending<false, L>(h, lds, N, slices, m, mean_dev, var_dev, cross_dev, N, 0, (int)p, d_mp, d_cpp, d_z, (int)S,
                                                       slice, cells, d_tab, alive_dev, h->d_ws, nullptr, 0);
      if (e == hipSuccess) eh_finish<L>(h, h->d_ws, slices, N, S, alive_dev, scores_dev);
      return e;
    });
    BBH_HIP_TRY(h, launched);
    BBH_HIP_TRY(h, hipGetLastError());
    h->last_ehvi_form = 0;
    return 0;
  }
  // form 1: m tri(q') doubles per row and slice; the rows are walked in chunks (multiples of 64) whose workspace stays below the
  // bound, every chunk addressing the factors from 0; the partials of all rows sit in front of them
  const size_t per_row = sizeof(double) * (size_t)m * (size_t)(q * (q + 1) / 2) * (size_t)slices;
  const size_t ws_bound = h->sw.qbig_ws_mb ? (size_t)h->sw.qbig_ws_mb << 20 : EH_WS_BYTES;
  int64_t chunk = (int64_t)(ws_bound / per_row) / 64 * 64;
  if (chunk < 64) chunk = 64;
  if (chunk > N) chunk = N;
  rc = bbh_ensure_ws(h, sizeof(double) * npartial + per_row * (size_t)chunk);
  if (rc) return rc;
  double* Lws = h->d_ws + npartial;
  bbh_timed_scope timed(h, BBH_TIMED_PENDING);
  const hipError_t launched = bbh_dispatch_flag(log != 0, [&](auto LOG) {
    constexpr bool L = decltype(LOG)::value;
    for (int64_t c0 = 0; c0 < N; c0 += chunk) {
      const hipError_t e = eh_launch_pending<true, L>(h, lds, std::min(chunk, N - c0), slices, m, mean_dev, var_dev, cross_dev, N, c0, (int)p, d_mp,
                                                      d_cpp, d_z, (int)S, slice, cells, d_tab, alive_dev, h->d_ws, Lws, chunk);
      if (e != hipSuccess) return e;
    }
    eh_finish<L>(h, h->d_ws, slices, N, S, alive_dev, scores_dev);
    return hipSuccess;
  });
  BBH_HIP_TRY(h, launched);
  BBH_HIP_TRY(h, hipGetLastError());
  h->last_ehvi_form = 1;
  return 0;
}

extern "C" int bbh_ehvi_last_form(bbh_handle* h) { return h ? h->last_ehvi_form : -1; }
