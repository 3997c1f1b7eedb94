// Bayesian linear (ARD) surrogate: predictive mean and variance of every candidate row in one pass over the resident matrix.
//
// What the reference does here (BayesianLinearSurrogate, baybe/surrogates/linear.py:62-82): scikit-learn's
// ARDRegression.predict(X, return_std=True) over all N candidates on the host - np.dot(X, sigma_) * X, an [N, k] temporary and
// N k^2 flops - wrapped into an MVN that BoTorch scores in chunks.  The fit (ARDRegression.fit) stays on the host; the host packs, per
// kept column j < k (lambda_ < threshold_lambda), its comp-rep column, lo, hi - lo and coef, and ONE k x k matrix T with
// T[i][i] = Ss[i][i], T[i][j] = 2 Ss[i][j] for j < i and 0 above the diagonal, Ss = (sigma_ + sigma_^T) / 2, so that
// x~^T sigma_ x~ = x~^T T x~ = sum_i x~_i sum_{j <= i} T[i][j] x~_j and only the blocks on and below the diagonal carry work.
//
//   x~_j  = (x[col_j] - lo_j) / range_j                          (a subtraction and a division, as the GP path's Normalize)
//   mean  = ybar + ysd * (sum_j x~_j coef_j + intercept)
//   var   = ysd^2 * (x~^T T x~ + inv_alpha)
//
//   bbh_linear_fill_kernel       k = 0 (constant targets, every column pruned): the two constants.
//   bbh_linear_reg_kernel<KP>    k <= 32, KP in {8, 16, 32}: one thread per row, x~ in registers at compile-time indices (padded BY INDEX:
//                                nothing is read for j >= k), T and the column table at wave-uniform LDS addresses; the rows reach
//                                their threads through LDS so that global loads run along the rows.  HBM-bound by derivation: 8 d
//                                bytes against k (k + 1) / 2 + k multiply-adds per row.
//   bbh_linear_block_kernel      any k <= 512: 16 rows per wave, x~ of the workgroup's rows in LDS, (T x~) for one 16-column block of T
//                                at a time on v_mfma_f64_16x16x4_f64 - the block's 16 rows of T staged through LDS, the K steps right
//                                of the diagonal block skipped, as bbh_gmm_estep_kernel skips them - then dotted with the same block
//                                of x~.  k is padded to a multiple of 16 by index: a padded lane contributes 0.0.
//
// Every sum has a fixed order (j ascending on one thread; the MFMA's own order, column blocks ascending, then a 16-lane butterfly)
// that does not depend on where a row sits, and nothing is contracted: equal rows get equal bits within a form.  No atomics.  No entry
// point keeps state beyond the form of the last call: all buffers are the caller's, all launches on the handle's stream.
#include "bbh_common.h"

#pragma clang fp contract(off)

#define LIN_MAX_K 512
#define LIN_REG_MAX_K 32       // kept columns the register form holds (64 VGPRs of x~)
#define LIN_AUTO_REG_MAX_K 16  // form 0 takes the register form up to here: measured (profiles/linear_pass.json), the <32> instantiation loses to the block form
#define LIN_REG_ROWS 128  // rows (threads) per workgroup of the register form: 128 x 33 doubles of x~ next to T stay below 48 KB of LDS
#define LIN_MAX_ROWS ((int64_t)INT_MAX - 256)

struct LinArgs {
  const double* X;  // [N][ldx]
  int64_t N, ldx;
  const int* cols;   // [k]
  const double* lo;  // [k]
  const double* rg;  // [k]
  const double* cf;  // [k]
  const double* T;   // [k][k]
  int k;
  double intercept, inv_alpha, ybar, ysd;
  double* mean;  // [N]
  double* var;   // [N]
};

__device__ __forceinline__ void lin_store(const LinArgs& A, int64_t row, double m, double v) {
  A.mean[row] = A.ybar + A.ysd * (m + A.intercept);
  A.var[row] = (A.ysd * A.ysd) * (v + A.inv_alpha);
}

__global__ __launch_bounds__(256) void bbh_linear_fill_kernel(const LinArgs A) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row < A.N) lin_store(A, row, 0.0, 0.0);
}

// grid ceil(N / LIN_REG_ROWS), LIN_REG_ROWS threads.  The kept columns of the workgroup's rows are read with the lanes along a row
// (consecutive kept columns are consecutive addresses), scaled, and handed to the row's thread through LDS (row stride KP + 1: odd, no
// bank conflicts); a thread reading its own row from global memory has its 64 lanes 8 ldx bytes apart in every load.
template <int KP>
__global__ __launch_bounds__(LIN_REG_ROWS) void bbh_linear_reg_kernel(const LinArgs A) {
  constexpr int XS = KP + 1;
  __shared__ double s_T[KP * KP];
  __shared__ double s_x[LIN_REG_ROWS * XS];
  __shared__ double s_lo[KP], s_rg[KP], s_cf[KP];
  __shared__ int s_col[KP];
  const int tid = threadIdx.x, k = A.k;
  for (int e = tid; e < KP * KP; e += LIN_REG_ROWS) {
    const int i = e / KP, j = e - i * KP;
    s_T[e] = (i < k && j <= i) ? A.T[i * k + j] : 0.0;
  }
  if (tid < KP) {
    const bool kept = tid < k;
    s_col[tid] = kept ? A.cols[tid] : 0;
    s_lo[tid] = kept ? A.lo[tid] : 0.0;
    s_rg[tid] = kept ? A.rg[tid] : 1.0;
    s_cf[tid] = kept ? A.cf[tid] : 0.0;
  }
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * LIN_REG_ROWS;
  for (int e = tid; e < LIN_REG_ROWS * k; e += LIN_REG_ROWS) {
    const int r = e / k, j = e - r * k;
    if (r0 + r < A.N) s_x[r * XS + j] = (A.X[(r0 + r) * A.ldx + s_col[j]] - s_lo[j]) / s_rg[j];
  }
  __syncthreads();
  const int64_t row = r0 + tid;
  if (row >= A.N) return;
  const double* xr = s_x + tid * XS;
  double x[KP];
#pragma unroll
  for (int j = 0; j < KP; j++) x[j] = (j < k) ? xr[j] : 0.0;
  double m = 0.0, v = 0.0;
#pragma unroll
  for (int i = 0; i < KP; i++) {
    if (i < k) {  // (wave-uniform)
      m = m + x[i] * s_cf[i];
      double y = 0.0;
#pragma unroll
      for (int j = 0; j <= i; j++) y = y + s_T[i * KP + j] * x[j];
      v = v + x[i] * y;
    }
  }
  lin_store(A, row, m, v);
}

// Row stride of the LDS images in doubles: KP + 2 (mod 32) - the 16 rows a half-wave's A / B fragments come from fall into 16 distinct
// bank pairs, and a row is written with consecutive addresses.
static inline int lin_stride(int KP) { return KP + 2 + (KP % 32); }
static inline size_t lin_block_lds(int W, int KP) { return sizeof(double) * ((size_t)(16 * W + 16) * lin_stride(KP) + KP + 16 * W); }

// grid ceil(N / R), 64 W threads, R = 16 W rows.  dynamic LDS: x~ [R][XS] | the panel T[16 cb .. 16 cb + 15][0 .. 16 (cb + 1)) as [16][XS] |
// coef [KP] | the quadratic forms [R]
__global__ __launch_bounds__(256) void bbh_linear_block_kernel(const LinArgs A, int nb, int XS) {
  extern __shared__ double s_lin[];
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lp = lane >> 4;
  const int R = nthr >> 2, k = A.k, KP = 16 * nb;
  double* s_x = s_lin;
  double* s_p = s_x + (size_t)R * XS;
  double* s_cf = s_p + 16 * XS;
  double* s_v = s_cf + KP;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  for (int e = tid; e < R * KP; e += nthr) {
    const int r = e / KP, j = e - r * KP;
    const int64_t row = r0 + r;
    double xv = 0.0;
    if (row < A.N && j < k) xv = (A.X[row * A.ldx + A.cols[j]] - A.lo[j]) / A.rg[j];
    s_x[r * XS + j] = xv;
  }
  for (int e = tid; e < KP; e += nthr) s_cf[e] = (e < k) ? A.cf[e] : 0.0;
  double sq[4] = {0.0, 0.0, 0.0, 0.0};
  const double* xa = s_x + (wave * 16 + li) * XS + lp;  // A fragment: x~[row li][4 kb + lp]
  const double* pb = s_p + li * XS + lp;                // B fragment: T[16 cb + li][4 kb + lp]
  for (int cb = 0; cb < nb; cb++) {
    const int KK = 16 * (cb + 1);
    __syncthreads();  // the x~ tile is complete / the previous panel has been read
    for (int e = tid; e < 16 * KK; e += nthr) {
      const int n = e / KK, kk = e - n * KK, i = 16 * cb + n;
      s_p[n * XS + kk] = (i < k && kk <= i) ? A.T[(int64_t)i * k + kk] : 0.0;
    }
    __syncthreads();
    d4 acc = d4{0.0, 0.0, 0.0, 0.0};
    for (int kb = 0; kb < 4 * (cb + 1); kb++)  // columns of T right of the diagonal block are zero: skipped
      acc = mfma_f64(xa[kb * 4], pb[kb * 4], acc);
#pragma unroll
    for (int q = 0; q < 4; q++) sq[q] = sq[q] + acc[q] * s_x[(wave * 16 + lp + 4 * q) * XS + 16 * cb + li];
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1)
#pragma unroll
    for (int q = 0; q < 4; q++) sq[q] = sq[q] + __shfl_xor(sq[q], o, 64);
  if (li == 0) {
#pragma unroll
    for (int q = 0; q < 4; q++) s_v[wave * 16 + lp + 4 * q] = sq[q];
  }
  __syncthreads();
  if (lane < 16) {
    const int r = wave * 16 + lane;
    const int64_t row = r0 + r;
    if (row < A.N) {
      const double* xrow = s_x + r * XS;
      double m = 0.0;
      for (int j = 0; j < k; j++) m = m + xrow[j] * s_cf[j];
      lin_store(A, row, m, s_v[r]);
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
extern "C" int bbh_linear_moments(bbh_handle* h, const double* X_dev, int64_t N, int32_t d, int64_t ldx, const int32_t* cols_dev,
                                  const double* scale_dev, const double* T_dev, int32_t k, double intercept, double inv_alpha, double ybar,
                                  double ysd, int32_t form, double* mean_dev, double* var_dev) {
  if (!h) return -1;
  if (k < 0 || k > LIN_MAX_K || form < 0 || form > 2 || N < 0 || N > LIN_MAX_ROWS) {
    h->err = "bbh_linear_moments: bad arguments (need 0 <= k <= 512, form 0 (auto), 1 (register) or 2 (block) and 0 <= N < 2^31 - 256)";
    return -1;
  }
  if (form == 1 && k > LIN_REG_MAX_K) {
    h->err = "bbh_linear_moments: bad arguments (the register form holds at most 32 kept columns; use form 0 or 2)";
    return -1;
  }
  if (N == 0) return 0;
  if (!mean_dev || !var_dev || (k > 0 && (!X_dev || !cols_dev || !scale_dev || !T_dev || d < 1 || ldx < d))) {
    h->err = "bbh_linear_moments: bad arguments (need both outputs and, for k > 0, the rows with 1 <= d <= ldx, the column list, the "
             "scale table [3, k] and T [k, k])";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  if (k > 0) {  // a column index outside the rows would be read out of bounds: looked at before anything is launched
    std::vector<int32_t> cols((size_t)k);
    BBH_HIP_TRY(h, hipMemcpyAsync(cols.data(), cols_dev, sizeof(int32_t) * (size_t)k, hipMemcpyDeviceToHost, h->stream));
    BBH_HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int32_t j = 0; j < k; j++)
      if (cols[j] < 0 || cols[j] >= d) {
        h->err = "bbh_linear_moments: bad arguments (a kept column's index lies outside the d columns of the rows)";
        return -1;
      }
  }
  LinArgs a;
  a.X = X_dev, a.N = N, a.ldx = ldx, a.cols = cols_dev, a.lo = scale_dev, a.rg = scale_dev + k, a.cf = scale_dev + 2 * (int64_t)k;
  a.T = T_dev, a.k = (int)k, a.intercept = intercept, a.inv_alpha = inv_alpha, a.ybar = ybar, a.ysd = ysd, a.mean = mean_dev, a.var = var_dev;
  const int taken = (form == 2 || (form == 0 && k > LIN_AUTO_REG_MAX_K)) ? 2 : 1;
  const unsigned g256 = (unsigned)((N + 255) / 256);
  if (k == 0) {
    hipLaunchKernelGGL(bbh_linear_fill_kernel, dim3(g256), dim3(256), 0, h->stream, a);
  } else if (taken == 1) {
    const dim3 grid((unsigned)((N + LIN_REG_ROWS - 1) / LIN_REG_ROWS)), block(LIN_REG_ROWS);
    if (k <= 8)
      hipLaunchKernelGGL(bbh_linear_reg_kernel<8>, grid, block, 0, h->stream, a);
    else if (k <= 16)
      hipLaunchKernelGGL(bbh_linear_reg_kernel<16>, grid, block, 0, h->stream, a);
    else
      hipLaunchKernelGGL(bbh_linear_reg_kernel<32>, grid, block, 0, h->stream, a);
  } else {
    const int nb = (k + 15) / 16, KP = 16 * nb;
    int W = 4;  // waves per workgroup: as many 16-row tiles as fit into LDS next to the panel
    while (W > 1 && lin_block_lds(W, KP) > h->lds_per_block) W >>= 1;
    const size_t lds = lin_block_lds(W, KP);
    if (lds > h->lds_per_block) {
      h->err = "bbh_linear_moments: 16 rows of the kept columns and a panel of T do not fit into this device's LDS";
      return -1;
    }
    BBH_HIP_TRY(h, bbh_allow_lds(h->device, (const void*)bbh_linear_block_kernel, lds));
    const int R = 16 * W;
    hipLaunchKernelGGL(bbh_linear_block_kernel, dim3((unsigned)((N + R - 1) / R)), dim3(64 * W), lds, h->stream, a, nb, lin_stride(KP));
  }
  BBH_HIP_TRY(h, hipGetLastError());
  h->last_linear_form = taken;
  return 0;
}

extern "C" int bbh_linear_last_form(bbh_handle* h) { return h ? h->last_linear_form : -1; }
