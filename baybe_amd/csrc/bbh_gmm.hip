// Gaussian mixture clustering (EM, full covariances) over the device-resident candidate matrix, batched over the restarts.
//
// What the reference does here (GaussianMixtureClusteringRecommender, baybe/recommenders/pure/nonpredictive/clustering.py:255-304):
// hand the scaled candidates to sklearn.mixture.GaussianMixture(n_components=batch_size) - EM on the host, once per restart, over
// the whole candidate set - then model.predict and one np.random.choice per non-empty component.  The two sweeps of an EM iteration
// are GEMM-shaped (N k d^2 each in fp64); here both run on v_mfma_f64_16x16x4_f64, with the restarts as a grid dimension.
//
//   bbh_gmm_sums_kernel         M-step, sweep 1: per strip of 256-position tiles and chunk of components, r = exp(log_resp) (or the
//                               one-hot of the labels) staged in LDS, then every accumulator (component, dimension | count) is owned
//                               by ONE thread that adds the strip's positions in ascending order.
//   bbh_gmm_means_kernel        one workgroup per restart: the strips added in ascending order, nk = sum r + 10 * 2^-52, mu = sum r x / nk.
//   bbh_gmm_cov_kernel<NB>      M-step, sweep 2: per (strip, component, restart) the weighted outer products
//                               sum_j r_jc (x_j - mu_c)(x_j - mu_c)^T on the MFMA: positions are the K dimension (4 per instruction),
//                               d is padded to 16 * NB BY INDEX (a padded lane contributes 0.0, nothing is read past d), only the
//                               16 x 16 blocks on and below the diagonal are computed.  A wave takes 64 positions of every tile of
//                               the strip; the four waves' accumulators are added in wave order.
//   bbh_gmm_cov_finish_kernel   one workgroup per (component, restart): the strips added in ascending order, / nk, + reg_covar on the
//                               diagonal, the mirrored upper triangle, and the weight nk / N (divided by the sum of all weights,
//                               ascending, after an EM step).
//   bbh_gmm_precision_kernel    one workgroup per (component, restart): Sigma = L L^T and L^-1 in LDS, sequential in ascending index;
//                               P = (L^-1)^T, logdet = sum_i log P[i][i]; a pivot that is not finite and positive flags the restart.
//   bbh_gmm_estep_kernel<NB>    per 256-position tile and restart: P_c and mu_c of a chunk of components in LDS, y = (x - mu_c) P_c
//                               on the MFMA (16 positions x 16 output columns per block; the K steps below the diagonal block of the
//                               upper-triangular P_c are skipped), q = |y|^2, lp, the max-shifted log-sum-exp over the components
//                               in ascending order, log_resp (component-major: a wave's stores are consecutive), the label (the
//                               smallest component among equal maxima) and the tile's sum of lpn.
//   bbh_gmm_bound_kernel        per restart: lower_bound = (the tile sums added in ascending tile order) / N.
//
// No floating-point atomics anywhere: every sum has a fixed shape (positions ascending inside a strip, strips ascending, the block
// sum of bbh_rows.h, or the MFMA's own order), so two runs give the same bits; nothing is contracted (bbh_rows.h).  No entry point
// keeps state: all buffers are the caller's, all launches asynchronous on the handle's stream.
#include "bbh_rows.h"

#define GM_TP BBH_ROWS_TILE        // positions per tile
#define GM_MAX_D 64                // full covariances: k d^2 doubles, factorised by one workgroup in LDS (64 x 65 doubles = 33 KB)
#define GM_MAX_STRIPS 64           // partials per accumulator at the most, whatever M is (k = 100, d = 64: 64 * 100 * 10 * 2 KB = 128 MB)
#define GM_LDS_BUDGET ((size_t)64 * 1024)
#define GM_S1_ACC 4                // sweep 1: accumulators per thread
#define GM_S1_KC 16                // sweep 1: components per workgroup at the most (r of a tile: 16 * 256 doubles = 32 KB)
#define GM_LOG_2PI 1.8378770664093453
#define GM_TINY 2.220446049250313e-15  // 10 * 2^-52

namespace {

struct GmPlan {
  int nb, dpad;   // 16-column blocks of d, d padded to them
  int kc, chunks; // E-step: components per LDS chunk
  int kc1;        // sweep 1: components per workgroup
  int64_t ntiles, tps, strips;
  size_t lds;
};

GmPlan gm_plan(const bbh_handle* h, int d, int64_t k, int64_t M) {
  GmPlan p;
  p.nb = (d + 15) / 16, p.dpad = 16 * p.nb;
  const size_t budget = (h->lds_per_block < GM_LDS_BUDGET) ? h->lds_per_block : GM_LDS_BUDGET;
  const size_t per = sizeof(double) * ((size_t)p.dpad * p.dpad + p.dpad + 2 + GM_TP);  // P_c, mu_c, logdet_c and log w_c, q of the tile
  int64_t kc = (int64_t)(budget / per);
  if (kc < 1) kc = 1;
  if (kc > k) kc = k;
  p.kc = (int)kc, p.chunks = (int)((k + kc - 1) / kc), p.lds = per * (size_t)kc;
  int64_t kc1 = (GM_TP * GM_S1_ACC) / (d + 1);
  if (kc1 > GM_S1_KC) kc1 = GM_S1_KC;
  if (kc1 > k) kc1 = k;
  p.kc1 = (int)kc1;
  p.ntiles = (M + GM_TP - 1) / GM_TP;
  p.tps = (p.ntiles + GM_MAX_STRIPS - 1) / GM_MAX_STRIPS;
  p.strips = (p.ntiles + p.tps - 1) / p.tps;
  return p;
}

// r_jc from its source: exp(log_resp [.., k, M]) or the one-hot of labels [.., M] (-1: a row of zeros)
__device__ __forceinline__ double gm_resp(const double* __restrict__ log_resp, const int* __restrict__ labels, int64_t slot, int64_t k,
                                          int64_t c, int64_t M, int64_t j) {
  if (log_resp) return exp(log_resp[(slot * k + c) * M + j]);
  return (labels[slot * M + j] == (int)c) ? 1.0 : 0.0;
}

}  // namespace

struct GmMstepArgs {
  const double* P;  // [d][ldp]
  int64_t ldp, M;
  int d;
  const double* log_resp;  // [G][k][M] or null
  const int* labels;       // [G][M] or null
  const int* rid;          // [n_active]: the restarts of this launch (indices into the [R, ...] parameter arrays)
  int64_t src_base;        // restart r reads row r - src_base of log_resp / labels
  int64_t n_active, k, tps, ntiles, strips;
  int kc1, normalize;
  double reg_covar;
  double* part1;  // [strips][n_active][k][d + 1]
  double* part2;  // [strips][n_active][k][blocks][256]
  double* nk;     // [R][k]
  double* w;      // [R][k]
  double* mu;     // [R][k][d]
  double* cov;    // [R][k][d][d]
};

// grid (strips, ceil(k / kc1), n_active)
__global__ __launch_bounds__(256) void bbh_gmm_sums_kernel(const GmMstepArgs A) {
  __shared__ double s_r[GM_S1_KC][GM_TP];
  const int tid = threadIdx.x, d = A.d, d1 = A.d + 1;
  const int64_t s = blockIdx.x, slot = blockIdx.z;
  const int64_t r = A.rid[slot], src = r - A.src_base;
  const int64_t c0 = (int64_t)blockIdx.y * A.kc1;
  const int nc = (A.k - c0 < A.kc1) ? (int)(A.k - c0) : A.kc1;
  double acc[GM_S1_ACC];
#pragma unroll
  for (int u = 0; u < GM_S1_ACC; u++) acc[u] = 0.0;
  const int64_t t1 = ((s + 1) * A.tps < A.ntiles) ? (s + 1) * A.tps : A.ntiles;
  for (int64_t t = s * A.tps; t < t1; t++) {
    const int64_t j0 = t * GM_TP, j = j0 + tid;
    __syncthreads();
    for (int c = 0; c < nc; c++) s_r[c][tid] = (j < A.M) ? gm_resp(A.log_resp, A.labels, src, A.k, c0 + c, A.M, j) : 0.0;
    __syncthreads();
    const int np = (A.M - j0 < GM_TP) ? (int)(A.M - j0) : GM_TP;
#pragma unroll
    for (int u = 0; u < GM_S1_ACC; u++) {
      const int a = tid + GM_TP * u;
      if (a >= nc * d1) continue;
      const int c = a / d1, dim = a - c * d1;
      const double* rr = s_r[c];
      double v = acc[u];
      if (dim == d) {
        for (int p = 0; p < np; p++) v = v + rr[p];
      } else {
        const double* xg = A.P + (int64_t)dim * A.ldp + j0;
        for (int p = 0; p < np; p++) v = v + rr[p] * xg[p];
      }
      acc[u] = v;
    }
  }
#pragma unroll
  for (int u = 0; u < GM_S1_ACC; u++) {
    const int a = tid + GM_TP * u;
    if (a < nc * d1) A.part1[((s * A.n_active + slot) * A.k + c0) * d1 + a] = acc[u];
  }
}

// grid (n_active)
__global__ __launch_bounds__(256) void bbh_gmm_means_kernel(const GmMstepArgs A) {
  const int d = A.d, d1 = A.d + 1;
  const int64_t slot = blockIdx.x, r = A.rid[slot];
  const int64_t per = A.k * d1;
  for (int64_t a = threadIdx.x; a < per; a += 256) {
    const int64_t c = a / d1;
    const int dim = (int)(a - c * d1);
    double v = 0.0, n = 0.0;
    for (int64_t s = 0; s < A.strips; s++) {
      const double* p = A.part1 + (s * A.n_active + slot) * per;
      v = v + p[a];
      n = n + p[c * d1 + d];
    }
    n = n + GM_TINY;
    if (dim == d)
      A.nk[r * A.k + c] = n;
    else
      A.mu[(r * A.k + c) * d + dim] = v / n;
  }
}

// grid (strips, k, n_active); block idx of (bi, bj), bj <= bi: bi (bi + 1) / 2 + bj
template <int NB>
__global__ __launch_bounds__(256) void bbh_gmm_cov_kernel(const GmMstepArgs A) {
  constexpr int NBLK = NB * (NB + 1) / 2;
  __shared__ double s_acc[NBLK * 256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lp = lane >> 4, d = A.d;
  const int64_t s = blockIdx.x, c = blockIdx.y, slot = blockIdx.z;
  const int64_t r = A.rid[slot], src = r - A.src_base;
  double mu_l[NB];
#pragma unroll
  for (int b = 0; b < NB; b++) mu_l[b] = (b * 16 + li < d) ? A.mu[(r * A.k + c) * d + b * 16 + li] : 0.0;
  d4 acc[NBLK];
#pragma unroll
  for (int i = 0; i < NBLK; i++) acc[i] = d4{0.0, 0.0, 0.0, 0.0};
  const int64_t t1 = ((s + 1) * A.tps < A.ntiles) ? (s + 1) * A.tps : A.ntiles;
  for (int64_t t = s * A.tps; t < t1; t++) {
    for (int step = 0; step < 16; step++) {
      const int64_t j = t * GM_TP + wave * 64 + step * 4 + lp;
      const bool live = j < A.M;
      const double rv = live ? gm_resp(A.log_resp, A.labels, src, A.k, c, A.M, j) : 0.0;
      double xc[NB];
#pragma unroll
      for (int b = 0; b < NB; b++) xc[b] = (live && b * 16 + li < d) ? A.P[(int64_t)(b * 16 + li) * A.ldp + j] - mu_l[b] : 0.0;
      int idx = 0;
#pragma unroll
      for (int bi = 0; bi < NB; bi++) {
        const double a = rv * xc[bi];
#pragma unroll
        for (int bj = 0; bj <= bi; bj++) {
          acc[idx] = mfma_f64(a, xc[bj], acc[idx]);
          idx++;
        }
      }
    }
  }
  for (int w = 1; w < 4; w++) {  // ((wave 0 + wave 1) + wave 2) + wave 3
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < NBLK; i++)
#pragma unroll
        for (int q = 0; q < 4; q++) s_acc[i * 256 + q * 64 + lane] = acc[i][q];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int i = 0; i < NBLK; i++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[i][q] = acc[i][q] + s_acc[i * 256 + q * 64 + lane];
    }
  }
  if (wave == 0) {
    double* out = A.part2 + ((s * A.n_active + slot) * A.k + c) * (int64_t)(NBLK * 256);
#pragma unroll
    for (int i = 0; i < NBLK; i++)
#pragma unroll
      for (int q = 0; q < 4; q++) out[i * 256 + q * 64 + lane] = acc[i][q];
  }
}

// grid (k, n_active).  Element (i, j), j <= i, of the accumulator: block (i / 16, j / 16), register (i % 16) / 4, lane
// ((i % 16) % 4) * 16 + j % 16 (the C layout of the MFMA: lane l, register q holds C[(l >> 4) + 4 q][l & 15]).
__global__ __launch_bounds__(256) void bbh_gmm_cov_finish_kernel(const GmMstepArgs A) {
  const int d = A.d, nb = (A.d + 15) / 16, nblk = nb * (nb + 1) / 2;
  const int64_t c = blockIdx.x, slot = blockIdx.y, r = A.rid[slot];
  const double n = A.nk[r * A.k + c];
  double* cov = A.cov + (r * A.k + c) * (int64_t)d * d;
  for (int e = threadIdx.x; e < d * d; e += 256) {
    const int i = e / d, j = e - i * d;
    if (j > i) continue;
    const int bi = i >> 4, bj = j >> 4, ii = i & 15, jj = j & 15;
    const int64_t at = (int64_t)(bi * (bi + 1) / 2 + bj) * 256 + (ii >> 2) * 64 + (ii & 3) * 16 + jj;
    double v = 0.0;
    for (int64_t s = 0; s < A.strips; s++) v = v + A.part2[((s * A.n_active + slot) * A.k + c) * (int64_t)(nblk * 256) + at];
    v = v / n;
    if (i == j) v = v + A.reg_covar;
    cov[i * d + j] = v;
    cov[j * d + i] = v;
  }
  if (threadIdx.x == 0) {
    const double N = (double)A.M;
    double w = n / N;
    if (A.normalize) {
      double tot = 0.0;
      for (int64_t q = 0; q < A.k; q++) tot = tot + A.nk[r * A.k + q] / N;
      w = w / tot;
    }
    A.w[r * A.k + c] = w;
  }
}

// grid (k, n_active), 64 threads: thread i owns row i of L (lower triangle of s_A) and column i of L^-1 (kept in row i of the strict
// upper triangle: L^-1[m][i] at s_A[i][m], m > i).
__global__ __launch_bounds__(64) void bbh_gmm_precision_kernel(const double* __restrict__ cov, const int* __restrict__ rid, int64_t k, int d,
                                                               double* __restrict__ prec, double* __restrict__ logdet, int* __restrict__ flags) {
  __shared__ double s_A[GM_MAX_D][GM_MAX_D + 1];
  __shared__ double s_piv;
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x, r = rid[blockIdx.y];
  const double* S = cov + (r * k + c) * (int64_t)d * d;
  for (int e = tid; e < d * d; e += 64) s_A[e / d][e % d] = S[e];
  if (tid == 0) s_bad = 0;
  for (int j = 0; j < d; j++) {
    __syncthreads();
    double s = 0.0;
    if (tid >= j && tid < d) {
      s = s_A[tid][j];
      for (int m = 0; m < j; m++) s = s - s_A[tid][m] * s_A[j][m];
    }
    if (tid == j) {
      if (!(isfinite(s) && s > 0.0)) s_bad = 1;
      s_piv = sqrt(s);
    }
    __syncthreads();
    if (tid == j)
      s_A[j][j] = s_piv;
    else if (tid > j && tid < d)
      s_A[tid][j] = s / s_piv;
  }
  __syncthreads();
  double* Pc = prec + (r * k + c) * (int64_t)d * d;
  if (tid < d) {
    const double inv = 1.0 / s_A[tid][tid];
    for (int i = tid + 1; i < d; i++) {
      double s = s_A[i][tid] * inv;
      for (int m = tid + 1; m < i; m++) s = s + s_A[i][m] * s_A[tid][m];
      s_A[tid][i] = (0.0 - s) / s_A[i][i];
    }
    for (int i = 0; i < d; i++) Pc[tid * d + i] = (i < tid) ? 0.0 : (i == tid) ? inv : s_A[tid][i];
  }
  if (tid == 0) {
    // ascending i with the rounding error of every addition carried along (Neumaier): d terms of one sign reach |logdet| ~ 4 d on a
    // scaled covariance, where a plain running sum loses several ulps of the total - an absolute error that goes straight into lp
    double ld = 0.0, lost = 0.0;
    for (int i = 0; i < d; i++) {
      const double v = log(1.0 / s_A[i][i]);
      const double t = ld + v;
      lost = lost + ((fabs(ld) >= fabs(v)) ? (ld - t) + v : (v - t) + ld);
      ld = t;
    }
    logdet[r * k + c] = ld + lost;
    if (s_bad) atomicOr(flags + r, 1);
  }
}

struct GmEstepArgs {
  const double* P;  // [d][ldp]
  int64_t ldp, M;
  int d;
  const double* w;       // [R][k]
  const double* mu;      // [R][k][d]
  const double* prec;    // [R][k][d][d], upper triangular
  const double* logdet;  // [R][k]
  const int* rid;        // [n_active]
  int64_t dst_base;      // restart r writes row r - dst_base of log_resp / labels
  int64_t n_active, k, ntiles;
  int kc;
  double* log_resp;  // [G][k][M]
  int* labels;       // [G][M]
  double* lpn;       // [G][M] or null
  double* part;      // [tiles][n_active]
  double* lower;     // [R]
};

// grid (tiles, n_active).  dynamic LDS: [kc][dpad * dpad] P_c, [kc][dpad] mu_c, [kc] logdet_c, [kc] log w_c, [kc][256] q
template <int NB>
__global__ __launch_bounds__(256) void bbh_gmm_estep_kernel(const GmEstepArgs A) {
  extern __shared__ double s_gm[];
  __shared__ double s_w[4];
  constexpr int DP = 16 * NB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lp = lane >> 4, d = A.d, kc = A.kc;
  const int64_t tile = blockIdx.x, slot = blockIdx.y;
  const int64_t r = A.rid[slot], dst = r - A.dst_base;
  const int64_t j0 = tile * GM_TP, j = j0 + tid;
  const bool live = j < A.M;
  double* s_P = s_gm;
  double* s_mu = s_P + (size_t)kc * DP * DP;
  double* s_ld = s_mu + (size_t)kc * DP;
  double* s_lw = s_ld + kc;
  double* s_q = s_lw + kc;
  double* lr = A.log_resp + dst * A.k * A.M + (live ? j : 0);
  double best = -INFINITY;
  int lab = 0;
  for (int64_t c0 = 0; c0 < A.k; c0 += kc) {
    const int nc = (A.k - c0 < kc) ? (int)(A.k - c0) : kc;
    __syncthreads();
    for (int e = tid; e < nc * DP * DP; e += 256) {
      const int cc = e / (DP * DP), rem = e - cc * DP * DP, i = rem / DP, n = rem - i * DP;
      s_P[e] = (i < d && n < d) ? A.prec[((r * A.k + c0 + cc) * d + i) * d + n] : 0.0;
    }
    for (int e = tid; e < nc * DP; e += 256) {
      const int cc = e / DP, dim = e - cc * DP;
      s_mu[e] = (dim < d) ? A.mu[(r * A.k + c0 + cc) * d + dim] : 0.0;
    }
    for (int e = tid; e < nc; e += 256) s_ld[e] = A.logdet[r * A.k + c0 + e], s_lw[e] = log(A.w[r * A.k + c0 + e]);
    __syncthreads();
    for (int g = 0; g < 4; g++) {
      const int p0 = wave * 64 + g * 16;
      const int64_t jj = j0 + p0 + li;
      double xr[4 * NB];
#pragma unroll
      for (int kb = 0; kb < 4 * NB; kb++) xr[kb] = (jj < A.M && kb * 4 + lp < d) ? A.P[(int64_t)(kb * 4 + lp) * A.ldp + jj] : 0.0;
      for (int cc = 0; cc < nc; cc++) {
        const double* Pc = s_P + (size_t)cc * DP * DP;
        const double* mc = s_mu + (size_t)cc * DP;
        double sq[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int nb = 0; nb < NB; nb++) {
          d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int kb = 0; kb < 4 * (nb + 1); kb++)  // rows of P_c beyond the diagonal block are zero: skipped
            acc = mfma_f64(xr[kb] - mc[kb * 4 + lp], Pc[(kb * 4 + lp) * DP + nb * 16 + li], acc);
#pragma unroll
          for (int q = 0; q < 4; q++) sq[q] = sq[q] + acc[q] * acc[q];
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1)
#pragma unroll
          for (int q = 0; q < 4; q++) sq[q] = sq[q] + __shfl_xor(sq[q], o, 64);
        if (li == 0) {
#pragma unroll
          for (int q = 0; q < 4; q++) s_q[cc * GM_TP + p0 + lp + 4 * q] = sq[q];
        }
      }
    }
    __syncthreads();
    for (int cc = 0; cc < nc; cc++) {
      const double v = (-0.5 * ((double)d * GM_LOG_2PI + s_q[cc * GM_TP + tid]) + s_ld[cc]) + s_lw[cc];
      if (live) lr[(c0 + cc) * A.M] = v;
      if (v > best) best = v, lab = (int)(c0 + cc);  // ascending component, strict >: the smallest index of equal maxima
    }
  }
  double lpn = 0.0;
  if (live) {
    double sum = 0.0;
    for (int64_t c = 0; c < A.k; c++) sum = sum + exp(lr[c * A.M] - best);
    lpn = best + log(sum);
    for (int64_t c = 0; c < A.k; c++) lr[c * A.M] = lr[c * A.M] - lpn;
    A.labels[dst * A.M + j] = lab;
    if (A.lpn) A.lpn[dst * A.M + j] = lpn;
  }
  lpn = bbh_rows_block4_sum(lpn, s_w);
  if (tid == 0) A.part[tile * A.n_active + slot] = lpn;
}

// grid (n_active), 64 threads
__global__ __launch_bounds__(64) void bbh_gmm_bound_kernel(const GmEstepArgs A) {
  if (threadIdx.x != 0) return;
  const int64_t slot = blockIdx.x;
  double v = 0.0;
  for (int64_t t = 0; t < A.ntiles; t++) v = v + A.part[t * A.n_active + slot];
  A.lower[A.rid[slot]] = v / (double)A.M;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
extern "C" int bbh_gmm_plan(bbh_handle* h, int32_t d, int64_t k, int64_t M, int32_t* comps_per_chunk, int32_t* tiles_per_strip) {
  if (!h) return -1;
  if (d < 1 || d > GM_MAX_D || k < 1 || M < 1 || M > BBH_ROWS_MAX || k > M || !comps_per_chunk || !tiles_per_strip) {
    h->err = "bbh_gmm_plan: bad arguments (need 1 <= d <= 64, 1 <= k <= M < 2^31 - 256 and both outputs)";
    return -1;
  }
  const GmPlan p = gm_plan(h, d, k, M);
  *comps_per_chunk = p.kc, *tiles_per_strip = (int32_t)p.tps;
  return 0;
}

extern "C" int bbh_gmm_mstep(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, const double* log_resp_dev,
                             const int32_t* labels_dev, int64_t src_base, const int32_t* rid_dev, int64_t n_active, int64_t k,
                             double reg_covar, int32_t normalize, double* work_dev, int64_t work_len, double* nk_dev, double* w_dev,
                             double* mu_dev, double* cov_dev) {
  if (!h) return -1;
  int rc = bbh_rows_check(h, "bbh_gmm_mstep", P_dev, M, d, ldp, GM_MAX_D);
  if (rc) return rc;
  if ((!log_resp_dev) == (!labels_dev) || !rid_dev || !work_dev || !nk_dev || !w_dev || !mu_dev || !cov_dev || k < 1 || k > M || k > 65535 ||
      n_active < 1 || n_active > 65535 || src_base < 0 || !(reg_covar >= 0.0)) {
    h->err = "bbh_gmm_mstep: bad arguments (need log_resp or labels (one of them), the restart list, the work array, the outputs, "
             "1 <= k <= min(M, 65535), 1 <= restarts <= 65535 and reg_covar >= 0)";
    return -1;
  }
  const GmPlan p = gm_plan(h, d, k, M);
  const int nblk = p.nb * (p.nb + 1) / 2;
  const int64_t len1 = p.strips * n_active * k * (d + 1), len2 = p.strips * n_active * k * nblk * 256;
  if (work_len < len1 + len2) {
    h->err = "bbh_gmm_mstep: bad arguments (the work array needs strips * restarts * k * (d + 1 + 256 * blocks) doubles)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  GmMstepArgs a;
  a.P = P_dev, a.ldp = ldp, a.M = M, a.d = (int)d, a.log_resp = log_resp_dev, a.labels = labels_dev, a.rid = rid_dev, a.src_base = src_base;
  a.n_active = n_active, a.k = k, a.tps = p.tps, a.ntiles = p.ntiles, a.strips = p.strips, a.kc1 = p.kc1, a.normalize = normalize;
  a.reg_covar = reg_covar, a.part1 = work_dev, a.part2 = work_dev + len1, a.nk = nk_dev, a.w = w_dev, a.mu = mu_dev, a.cov = cov_dev;
  const unsigned S = (unsigned)p.strips, K = (unsigned)k, R = (unsigned)n_active;
  hipLaunchKernelGGL(bbh_gmm_sums_kernel, dim3(S, (unsigned)((k + p.kc1 - 1) / p.kc1), R), dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(bbh_gmm_means_kernel, dim3(R), dim3(256), 0, h->stream, a);
  switch (p.nb) {
    case 1: hipLaunchKernelGGL(bbh_gmm_cov_kernel<1>, dim3(S, K, R), dim3(256), 0, h->stream, a); break;
    case 2: hipLaunchKernelGGL(bbh_gmm_cov_kernel<2>, dim3(S, K, R), dim3(256), 0, h->stream, a); break;
    case 3: hipLaunchKernelGGL(bbh_gmm_cov_kernel<3>, dim3(S, K, R), dim3(256), 0, h->stream, a); break;
    default: hipLaunchKernelGGL(bbh_gmm_cov_kernel<4>, dim3(S, K, R), dim3(256), 0, h->stream, a); break;
  }
  hipLaunchKernelGGL(bbh_gmm_cov_finish_kernel, dim3(K, R), dim3(256), 0, h->stream, a);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

extern "C" int bbh_gmm_precision(bbh_handle* h, const double* cov_dev, const int32_t* rid_dev, int64_t n_active, int64_t k, int32_t d,
                                 double* prec_dev, double* logdet_dev, int32_t* flags_dev) {
  if (!h) return -1;
  if (!cov_dev || !rid_dev || !prec_dev || !logdet_dev || !flags_dev || d < 1 || d > GM_MAX_D || k < 1 || k > 65535 || n_active < 1 ||
      n_active > 65535) {
    h->err = "bbh_gmm_precision: bad arguments (need the covariances, the restart list, the outputs, 1 <= d <= 64, 1 <= k <= 65535 and "
             "1 <= restarts <= 65535)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(bbh_gmm_precision_kernel, dim3((unsigned)k, (unsigned)n_active), dim3(64), 0, h->stream, cov_dev, rid_dev, k, (int)d,
                     prec_dev, logdet_dev, flags_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

extern "C" int bbh_gmm_estep(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, const double* w_dev, const double* mu_dev,
                             const double* prec_dev, const double* logdet_dev, const int32_t* rid_dev, int64_t n_active, int64_t k,
                             int64_t dst_base, double* log_resp_dev, int32_t* labels_dev, double* lpn_dev, double* work_dev,
                             int64_t work_len, double* lower_dev) {
  if (!h) return -1;
  int rc = bbh_rows_check(h, "bbh_gmm_estep", P_dev, M, d, ldp, GM_MAX_D);
  if (rc) return rc;
  if (!w_dev || !mu_dev || !prec_dev || !logdet_dev || !rid_dev || !log_resp_dev || !labels_dev || !work_dev || !lower_dev || k < 1 || k > M ||
      n_active < 1 || n_active > 65535 || dst_base < 0) {
    h->err = "bbh_gmm_estep: bad arguments (need the parameters, the restart list, the outputs, the work array, 1 <= k <= M and "
             "1 <= restarts <= 65535)";
    return -1;
  }
  const GmPlan p = gm_plan(h, d, k, M);
  if (work_len < p.ntiles * n_active) {
    h->err = "bbh_gmm_estep: bad arguments (the work array needs tiles * restarts doubles)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  GmEstepArgs a;
  a.P = P_dev, a.ldp = ldp, a.M = M, a.d = (int)d, a.w = w_dev, a.mu = mu_dev, a.prec = prec_dev, a.logdet = logdet_dev, a.rid = rid_dev;
  a.dst_base = dst_base, a.n_active = n_active, a.k = k, a.ntiles = p.ntiles, a.kc = p.kc, a.log_resp = log_resp_dev, a.labels = labels_dev;
  a.lpn = lpn_dev, a.part = work_dev, a.lower = lower_dev;
  const dim3 grid((unsigned)p.ntiles, (unsigned)n_active);
  switch (p.nb) {
    case 1:
      BBH_HIP_TRY(h, bbh_allow_lds(h->device, (const void*)bbh_gmm_estep_kernel<1>, p.lds));
      hipLaunchKernelGGL(bbh_gmm_estep_kernel<1>, grid, dim3(256), p.lds, h->stream, a);
      break;
    case 2:
      BBH_HIP_TRY(h, bbh_allow_lds(h->device, (const void*)bbh_gmm_estep_kernel<2>, p.lds));
      hipLaunchKernelGGL(bbh_gmm_estep_kernel<2>, grid, dim3(256), p.lds, h->stream, a);
      break;
    case 3:
      BBH_HIP_TRY(h, bbh_allow_lds(h->device, (const void*)bbh_gmm_estep_kernel<3>, p.lds));
      hipLaunchKernelGGL(bbh_gmm_estep_kernel<3>, grid, dim3(256), p.lds, h->stream, a);
      break;
    default:
      BBH_HIP_TRY(h, bbh_allow_lds(h->device, (const void*)bbh_gmm_estep_kernel<4>, p.lds));
      hipLaunchKernelGGL(bbh_gmm_estep_kernel<4>, grid, dim3(256), p.lds, h->stream, a);
      break;
  }
  hipLaunchKernelGGL(bbh_gmm_bound_kernel, dim3((unsigned)n_active), dim3(64), 0, h->stream, a);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}
