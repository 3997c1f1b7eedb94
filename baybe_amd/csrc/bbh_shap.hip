// Exact interventional Shapley values of the posterior mean (baybe/insights/shap.py: SHAPInsight; what shap.KernelExplainer returns
// once its budget enumerates every coalition, M <= 11 with the default budget).  M features = groups of comp-rep columns,
// R explained rows x_r, B background rows b:
//
//   v(r, S)  = (1 / B) sum_b f(compose(x_r on the groups of S, b elsewhere)),   f = posterior mean, original target scale
//   phi_g(r) = sum_{S without g} |S|! (M - |S| - 1)! / M! [v(r, S + g) - v(r, S)]            (= W v, W [M, 2^M])
//   base     = v(., empty) = mean_b f(b)
//
// bbh_shap_values is the fused form: single task, one stationary kernel (Matern-1/2, Matern-3/2, Matern-5/2, RBF), n <= 512,
// 1 <= M <= 16.  The squared scaled distance is a sum over columns, so the distance of a composed row to training point t is
//
//   d2(x, b, S, t) = sum_{g in S} Dx[g, t] + sum_{g not in S} Db[b, g, t]  (+ Db[b, rest, t]: the columns in no group stay b's)
//
// and no composed row is ever materialised:
//   (1) bbh_shap_partial_kernel writes the per-group partial squared distances Dx [R, M, np] and Db [B, M + 1, np] (slot M = the
//       columns in no group): direct differences of the normalised coordinates, ascending column order inside a group, fma;
//   (2) bbh_shap_v_kernel: a workgroup owns one explained row and a chunk of consecutive coalitions, a thread CPT of them.  Per
//       (b, block of 16 training points) the workgroup builds in LDS the two meet-in-the-middle tables lo[S_lo] (groups 0 .. Ml,
//       Ml = ceil(M / 2)) and hi[S_hi] (groups Ml .. M, then the rest slot) by direct ascending-group sums - every entry adds its
//       own M terms from zero, nothing is carried from one coalition to the next - so d2(S) = lo[S_lo] + hi[S_hi] costs one add.
//       A thread accumulates alpha_t k(d2) over t ascending, then the rows b ascending;
//   (3) bbh_shap_phi_kernel: phi_g = sum over the masks S without g, ascending, of w(|S|) (v[S + g] - v[S]); the M weights
//       w(s) = s! (M - s - 1)! / M! come from the host, from exact integer factorials.
// Every sum has one fixed order that depends on neither R, B nor the row's position: equal rows give equal bits, two runs give
// equal bits.  No floating-point atomics.  The work is VALU and transcendental (one kernel value per (r, S, b, t)); no MFMA.
//
// bbh_shap_compose / bbh_shap_reduce are the generic form's device ends: composed rows [chunk, d] of a range of (r, S, b) triples
// for ANY model's posterior pass, and the mean over b in ascending order of what that pass returned.  bbh_shap_apply is (3) alone.
#include <math.h>

#include "bbh_common.h"

#define SHAP_MAXM 16
#define SHAP_TB 16  // training points per table build

struct ShapArgs {
  const double *Dx, *Db, *alpha;
  double* v;
  int64_t B;
  int n, np, M, Ml, nlo, nhi, chunk, nchunks;
  double os, ybar, ysd, mean_const;
};

struct ShapWeights {
  double w[SHAP_MAXM];  // w[s] = s! (M - s - 1)! / M!
};

template <int KIND>
__device__ __forceinline__ double shap_kval(double os, double r2) {
  r2 = r2 > 1e-30 ? r2 : 1e-30;  // gpytorch's distance: sqrt(clamp_min(r^2, 1e-30))
  if (KIND == BBH_KERNEL_RBF) return os * exp(-0.5 * r2);
  const double r = sqrt(r2);
  if (KIND == BBH_KERNEL_MATERN52) return os * ((1.0 + BBH_SQRT5 * r + (5.0 / 3.0) * r2) * exp(-BBH_SQRT5 * r));
  if (KIND == BBH_KERNEL_MATERN32) return os * ((1.0 + BBH_SQRT3 * r) * exp(-BBH_SQRT3 * r));
  return os * exp(-r);
}

// (1) out[row, g, t] = sum over the numerical columns j of group g, ascending, of ((x_j - X_tj) / l_j)^2; grp[j] = slot of column j
// (a column in no group: slot M, which only the background's table has)
__global__ __launch_bounds__(256) void bbh_shap_partial_kernel(const double* __restrict__ X, int64_t rows, int64_t ldx,
                                                               const double* __restrict__ xnT, const double* __restrict__ par,
                                                               const int* __restrict__ numcol, const int* __restrict__ grp, int n, int np,
                                                               int dn, int slots, double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * slots * n) return;
  const int t = (int)(idx % n);
  const int g = (int)((idx / n) % slots);
  const int64_t row = idx / ((int64_t)n * slots);
  const double* lo = par;
  const double* rng = par + dn;
  const double* il = par + 2 * dn;
  double acc = 0.0;
  for (int j = 0; j < dn; j++) {
    if (grp[j] != g) continue;
    const double xn = (X[row * ldx + numcol[j]] - lo[j]) / rng[j];
    const double sd = (xn - xnT[(int64_t)j * np + t]) * il[j];
    acc = fma(sd, sd, acc);
  }
  out[(row * slots + g) * np + t] = acc;
}

// (2) v[r, S] for the chunk blockIdx.x % nchunks of row blockIdx.x / nchunks; thread tid owns the masks S0 + k nt + tid, k < CPT
template <int KIND, int CPT>
__global__ __launch_bounds__(256) void bbh_shap_v_kernel(const ShapArgs a) {
  extern __shared__ __attribute__((aligned(16))) double shap_lds[];
  const int M = a.M, Ml = a.Ml, nlo = a.nlo, nhi = a.nhi, np = a.np;
  const int nt = blockDim.x, tid = threadIdx.x;
  double* s_px = shap_lds;                  // [TB][M]     partial distances of x_r
  double* s_pb = s_px + SHAP_TB * M;        // [TB][M + 1] ... of the background row (slot M: columns in no group)
  double* s_lo = s_pb + SHAP_TB * (M + 1);  // [TB][nlo]
  double* s_hi = s_lo + SHAP_TB * nlo;      // [TB][nhi]
  double* s_al = s_hi + SHAP_TB * nhi;      // [TB]
  const int64_t r = blockIdx.x / a.nchunks;
  const int S0 = (int)(blockIdx.x % a.nchunks) * a.chunk, hi0 = S0 >> Ml, total = 1 << M;
  int mlo[CPT], mhi[CPT];
#pragma unroll
  for (int k = 0; k < CPT; k++) {
    int S = S0 + k * nt + tid;
    if (S >= total) S = S0;  // (a chunk wider than 2^M: the surplus threads repeat a mask and store nothing)
    mlo[k] = S & (nlo - 1);
    mhi[k] = (S >> Ml) - hi0;
  }
  double tot[CPT];
#pragma unroll
  for (int k = 0; k < CPT; k++) tot[k] = 0.0;
  const int q2 = 2 * M + 1, ntab = nlo + nhi;
  for (int64_t b = 0; b < a.B; b++) {
    double acc[CPT];
#pragma unroll
    for (int k = 0; k < CPT; k++) acc[k] = 0.0;
    for (int t0 = 0; t0 < a.n; t0 += SHAP_TB) {
      const int tc = a.n - t0 < SHAP_TB ? a.n - t0 : SHAP_TB;
      for (int e = tid; e < tc * q2; e += nt) {
        const int tt = e / q2, q = e - tt * q2;
        if (q < M)
          s_px[tt * M + q] = a.Dx[(r * M + q) * np + t0 + tt];
        else
          s_pb[tt * (M + 1) + (q - M)] = a.Db[(b * (M + 1) + (q - M)) * np + t0 + tt];
      }
      if (tid < tc) s_al[tid] = a.alpha[t0 + tid];
      __syncthreads();
      for (int e = tid; e < tc * ntab; e += nt) {
        const int tt = e / ntab, i = e - tt * ntab;
        const double* px = s_px + tt * M;
        const double* pb = s_pb + tt * (M + 1);
        double s = 0.0;
        if (i < nlo) {
          for (int g = 0; g < Ml; g++) s += ((i >> g) & 1) ? px[g] : pb[g];
          s_lo[tt * nlo + i] = s;
        } else {
          const int m = hi0 + (i - nlo);
          for (int g = Ml; g < M; g++) s += ((m >> (g - Ml)) & 1) ? px[g] : pb[g];
          s += pb[M];
          s_hi[tt * nhi + (i - nlo)] = s;
        }
      }
      __syncthreads();
      if (tc == SHAP_TB) {
        // a full block: four training points in flight - their kernel values are independent chains, the additions keep their order
#pragma unroll 4
        for (int tt = 0; tt < SHAP_TB; tt++) {
          const double al = s_al[tt];
#pragma unroll
          for (int k = 0; k < CPT; k++) {
            const double d2 = s_lo[tt * nlo + mlo[k]] + s_hi[tt * nhi + mhi[k]];
            acc[k] = fma(al, shap_kval<KIND>(a.os, d2), acc[k]);
          }
        }
      } else {
        for (int tt = 0; tt < tc; tt++) {
          const double al = s_al[tt];
#pragma unroll
          for (int k = 0; k < CPT; k++) {
            const double d2 = s_lo[tt * nlo + mlo[k]] + s_hi[tt * nhi + mhi[k]];
            acc[k] = fma(al, shap_kval<KIND>(a.os, d2), acc[k]);
          }
        }
      }
      __syncthreads();  // (the next block of training points rewrites the partials and the weights)
    }
#pragma unroll
    for (int k = 0; k < CPT; k++) tot[k] += acc[k];
  }
#pragma unroll
  for (int k = 0; k < CPT; k++) {
    const int S = S0 + k * nt + tid;
    if (S < total) a.v[r * total + S] = a.ybar + a.ysd * (a.mean_const + tot[k] / (double)a.B);
  }
}

// (3) one thread per (r, g): the masks without g in ascending order
__global__ __launch_bounds__(256) void bbh_shap_phi_kernel(const double* __restrict__ v, int64_t R, int M, const ShapWeights wt,
                                                           double* __restrict__ phi) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= R * M) return;
  const int g = (int)(idx % M);
  const int64_t r = idx / M;
  const double* vr = v + r * ((int64_t)1 << M);
  const int bit = 1 << g, half = 1 << (M - 1);
  double acc = 0.0;
  for (int i = 0; i < half; i++) {
    const int S = ((i >> g) << (g + 1)) | (i & (bit - 1));  // the i-th mask without bit g
    acc = fma(wt.w[__popc(S)], vr[S | bit] - vr[S], acc);
  }
  phi[idx] = acc;
}

// rows[e - first] = compose(x_r on S, b elsewhere) for the triple e = (r 2^M + S) B + b; a column in no group is b's
__global__ __launch_bounds__(256) void bbh_shap_compose_kernel(const double* __restrict__ X, int64_t ldx, const double* __restrict__ Bg,
                                                               int64_t B, int64_t ldb, const int* __restrict__ grp, int d, int M,
                                                               int64_t first, int64_t count, double* __restrict__ rows) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= count * d) return;
  const int j = (int)(idx % d);
  const int64_t e = first + idx / d;
  const int64_t b = e % B, rs = e / B;
  const int64_t S = rs & (((int64_t)1 << M) - 1), r = rs >> M;
  const int g = grp[j];
  rows[idx] = (g >= 0 && ((S >> g) & 1)) ? X[r * ldx + j] : Bg[b * ldb + j];
}

// out[p] = (f[p B] + f[p B + 1] + ...) / B, ascending
__global__ __launch_bounds__(256) void bbh_shap_reduce_kernel(const double* __restrict__ f, int64_t pairs, int64_t B, double* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= pairs) return;
  double s = 0.0;
  for (int64_t b = 0; b < B; b++) s += f[p * B + b];
  out[p] = s / (double)B;
}

static int shap_weights(bbh_handle* h, const char* who, int M, ShapWeights* wt) {
  if (M < 1 || M > SHAP_MAXM) {
    h->err = std::string(who) + ": 1 <= M <= 16 features (the exact enumeration visits 2^M coalitions; M = " + std::to_string(M) + ")";
    return -1;
  }
  uint64_t fact[SHAP_MAXM + 1];
  fact[0] = 1;
  for (int i = 1; i <= SHAP_MAXM; i++) fact[i] = fact[i - 1] * (uint64_t)i;  // 16! < 2^53: numerator and denominator are exact doubles
  for (int s = 0; s < SHAP_MAXM; s++) wt->w[s] = s < M ? (double)(fact[s] * fact[M - s - 1]) / (double)fact[M] : 0.0;
  return 0;
}

static int shap_check_groups(bbh_handle* h, const char* who, const int32_t* grp, int d, int M) {
  if (!grp) {
    h->err = std::string(who) + ": no column-to-group map";
    return -1;
  }
  for (int j = 0; j < d; j++)
    if (grp[j] < -1 || grp[j] >= M) {
      h->err = std::string(who) + ": group index of column " + std::to_string(j) + " outside -1 .. M - 1";
      return -1;
    }
  return 0;
}

static int shap_launch_phi(bbh_handle* h, const double* v_dev, int64_t R, int M, const ShapWeights& wt, double* phi_dev) {
  hipLaunchKernelGGL(bbh_shap_phi_kernel, dim3((unsigned)((R * M + 255) / 256)), dim3(256), 0, h->stream, v_dev, R, M, wt, phi_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

template <int KIND>
static void shap_launch_v(hipStream_t s, int cpt, unsigned grid, int nt, size_t lds, const ShapArgs& a) {
  if (cpt == 4)
    hipLaunchKernelGGL((bbh_shap_v_kernel<KIND, 4>), dim3(grid), dim3(nt), lds, s, a);
  else
    hipLaunchKernelGGL((bbh_shap_v_kernel<KIND, 1>), dim3(grid), dim3(nt), lds, s, a);
}

extern "C" int bbh_shap_values(bbh_handle* h, const double* X_dev, int64_t R, int64_t ldx, const double* Bg_dev, int64_t B, int64_t ldb,
                               const int32_t* group_of_col_host, int32_t M, double* v_dev, double* phi_dev, double* base_host) {
  if (!h) return -1;
  const char* who = "bbh_shap_values";
  if (!h->factorized) {
    h->err = "bbh_shap_values: model not factorised";
    return -1;
  }
  const int kind = h->desc.kernel_kind;
  if (bbh_is_rff(h) || h->F != 1 || kind < BBH_KERNEL_MATERN12 || kind > BBH_KERNEL_RBF) {
    h->err = "bbh_shap_values: the fused form needs a single Matern-1/2, Matern-3/2, Matern-5/2 or RBF kernel (no composite, RFF or other kind)";
    return -1;
  }
  if (h->T != 1 || h->hadamard) {
    h->err = "bbh_shap_values: the fused form needs a single-task model";
    return -1;
  }
  if (h->n > 512) {
    h->err = "bbh_shap_values: the fused form takes at most 512 training points (n = " + std::to_string(h->n) + ")";
    return -1;
  }
  ShapWeights wt;
  int rc = shap_weights(h, who, M, &wt);
  if (rc) return rc;
  const int d = h->desc.d, dn = h->dn;
  rc = shap_check_groups(h, who, group_of_col_host, d, M);
  if (rc) return rc;
  if (R < 1 || B < 1 || !X_dev || !Bg_dev || ldx < d || ldb < d || !phi_dev) {
    h->err = "bbh_shap_values: bad arguments (need R >= 1 explained rows, B >= 1 background rows, ldx >= d, ldb >= d and phi)";
    return -1;
  }
  const int64_t total = (int64_t)1 << M, np = h->np;
  const int n = (int)h->n;
  // block shape: 64 threads up to 64 coalitions, else 256; four coalitions per thread once that still leaves two workgroups per CU
  // (BBH_SHAP_CPT forces one or four; four needs 1024 coalitions)
  const int nt = total <= 64 ? 64 : 256;
  int cpt = 1;
  if (total >= 4 * nt && (h->sw.shap_cpt == 4 || (h->sw.shap_cpt != 1 && R * (total / (4 * nt)) >= 2 * (int64_t)h->num_cu))) cpt = 4;
  const int chunk = nt * cpt;
  const int64_t nchunks = (total + chunk - 1) / chunk;
  if (R * nchunks > (int64_t)INT_MAX || (double)R * (double)total * 8.0 > 16.0 * 1073741824.0) {
    h->err = "bbh_shap_values: R 2^M too large for one call (the coalition values take R 2^M 8 bytes); explain fewer rows per call";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  // workspace: par [3 dn] | grp [dn] (ints, in the space of dn doubles) | Dx [R, M, np] | Db [B, M + 1, np] | v [R, 2^M] (unless given)
  const size_t n_par = 4 * (size_t)dn, n_dx = (size_t)R * M * np, n_db = (size_t)B * (M + 1) * np;
  rc = bbh_ensure_ws(h, sizeof(double) * (n_par + n_dx + n_db + (v_dev ? 0 : (size_t)R * total)));
  if (rc) return rc;
  double* d_par = h->d_ws;
  int* d_grp = (int*)(d_par + 3 * dn);
  double* Dx = d_par + n_par;
  double* Db = Dx + n_dx;
  double* v = v_dev ? v_dev : Db + n_db;
  std::vector<double> par(3 * (size_t)dn);
  std::vector<int> grp(dn);
  for (int c = 0; c < dn; c++) {
    par[c] = h->lo[c];
    par[dn + c] = h->hi[c] - h->lo[c];
    par[2 * dn + c] = 1.0 / h->theta[3 + c];
    const int gc = group_of_col_host[h->numcol[c]];
    grp[c] = gc < 0 ? M : gc;
  }
  BBH_HIP_TRY(h, hipMemcpyAsync(d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, s));
  BBH_HIP_TRY(h, hipMemcpyAsync(d_grp, grp.data(), sizeof(int) * grp.size(), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(bbh_shap_partial_kernel, dim3((unsigned)((R * M * n + 255) / 256)), dim3(256), 0, s, X_dev, R, ldx, h->d_xnT, d_par,
                     h->d_numcol, d_grp, n, (int)np, dn, (int)M, Dx);
  hipLaunchKernelGGL(bbh_shap_partial_kernel, dim3((unsigned)((B * (M + 1) * n + 255) / 256)), dim3(256), 0, s, Bg_dev, B, ldb, h->d_xnT,
                     d_par, h->d_numcol, d_grp, n, (int)np, dn, (int)M + 1, Db);
  ShapArgs a{};
  a.Dx = Dx;
  a.Db = Db;
  a.alpha = h->d_alpha;
  a.v = v;
  a.B = B;
  a.n = n;
  a.np = (int)np;
  a.M = M;
  a.Ml = (M + 1) / 2;
  a.nlo = 1 << a.Ml;
  const int64_t span = total < chunk ? total : chunk;  // masks a workgroup covers
  a.nhi = (int)(span >> a.Ml) > 1 ? (int)(span >> a.Ml) : 1;
  a.chunk = chunk;
  a.nchunks = (int)nchunks;
  a.os = h->desc.use_outputscale ? h->theta[2] : 1.0;
  a.ybar = h->ybar;
  a.ysd = h->ysd;
  a.mean_const = h->theta[1];
  const size_t lds = sizeof(double) * SHAP_TB * (size_t)(2 * M + 1 + a.nlo + a.nhi + 1);  // at most 16 (33 + 256 + 4 + 1) 8 = 37 632 bytes
  const unsigned grid = (unsigned)(R * nchunks);
  if (kind == BBH_KERNEL_RBF)
    shap_launch_v<BBH_KERNEL_RBF>(s, cpt, grid, nt, lds, a);
  else if (kind == BBH_KERNEL_MATERN52)
    shap_launch_v<BBH_KERNEL_MATERN52>(s, cpt, grid, nt, lds, a);
  else if (kind == BBH_KERNEL_MATERN32)
    shap_launch_v<BBH_KERNEL_MATERN32>(s, cpt, grid, nt, lds, a);
  else
    shap_launch_v<BBH_KERNEL_MATERN12>(s, cpt, grid, nt, lds, a);
  BBH_HIP_TRY(h, hipGetLastError());
  rc = shap_launch_phi(h, v, R, M, wt, phi_dev);
  if (rc) return rc;
  double base = 0.0;
  BBH_HIP_TRY(h, hipMemcpyAsync(&base, v, sizeof(double), hipMemcpyDeviceToHost, s));  // v(r, empty) is the same for every r
  BBH_HIP_TRY(h, hipStreamSynchronize(s));  // (pageable staging vectors; the caller reads base)
  if (base_host) *base_host = base;
  return 0;
}

extern "C" int bbh_shap_compose(bbh_handle* h, const double* X_dev, int64_t R, int64_t ldx, const double* Bg_dev, int64_t B, int64_t ldb,
                                const int32_t* group_of_col_host, int32_t d, int32_t M, int64_t first, int64_t count, double* rows_dev) {
  if (!h) return -1;
  const char* who = "bbh_shap_compose";
  ShapWeights wt;
  int rc = shap_weights(h, who, M, &wt);
  if (rc) return rc;
  if (d < 1 || d > 65536) {
    h->err = "bbh_shap_compose: 1 <= d <= 65536 columns";
    return -1;
  }
  rc = shap_check_groups(h, who, group_of_col_host, d, M);
  if (rc) return rc;
  const double triples = (double)R * (double)((int64_t)1 << M) * (double)B;
  if (R < 1 || B < 1 || !X_dev || !Bg_dev || ldx < d || ldb < d || first < 0 || count < 0 || (double)first + (double)count > triples ||
      (count > 0 && !rows_dev)) {
    h->err = "bbh_shap_compose: bad arguments (need R >= 1, B >= 1, ldx >= d, ldb >= d and a range inside the R 2^M B triples)";
    return -1;
  }
  if (count == 0) return 0;
  if ((double)count * (double)d > 256.0 * (double)INT_MAX) {
    h->err = "bbh_shap_compose: chunk too large for one launch";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  rc = bbh_ensure_ws(h, sizeof(int) * (size_t)d);
  if (rc) return rc;
  int* d_grp = (int*)h->d_ws;
  BBH_HIP_TRY(h, hipMemcpyAsync(d_grp, group_of_col_host, sizeof(int32_t) * d, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(bbh_shap_compose_kernel, dim3((unsigned)((count * d + 255) / 256)), dim3(256), 0, s, X_dev, ldx, Bg_dev, B, ldb, d_grp,
                     (int)d, (int)M, first, count, rows_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  BBH_HIP_TRY(h, hipStreamSynchronize(s));  // (the caller's map is pageable; the model's pass that follows may regrow the workspace)
  return 0;
}

extern "C" int bbh_shap_reduce(bbh_handle* h, const double* f_dev, int64_t pairs, int64_t B, double* out_dev) {
  if (!h) return -1;
  if (pairs < 0 || B < 1 || (pairs > 0 && (!f_dev || !out_dev))) {
    h->err = "bbh_shap_reduce: bad arguments (need B >= 1, f [pairs B] and out [pairs])";
    return -1;
  }
  if (pairs == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(bbh_shap_reduce_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, h->stream, f_dev, pairs, B, out_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

extern "C" int bbh_shap_apply(bbh_handle* h, const double* v_dev, int64_t R, int32_t M, double* phi_dev) {
  if (!h) return -1;
  ShapWeights wt;
  int rc = shap_weights(h, "bbh_shap_apply", M, &wt);
  if (rc) return rc;
  if (R < 1 || !v_dev || !phi_dev) {
    h->err = "bbh_shap_apply: bad arguments (need R >= 1, v [R, 2^M] and phi [R, M])";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  return shap_launch_phi(h, v_dev, R, M, wt, phi_dev);
}
