// Posterior value AND its derivatives with respect to a candidate's continuous coordinates (bbh_posterior_grad): what a
// gradient-based continuous optimiser needs in place of autograd through GPyTorch (the reference: botorch/hybrid.py:95-136 ->
// optimize_acqf_mixed).  Single task, one stationary kernel (Matern-3/2, Matern-5/2, RBF), n <= 512.
//
//   k*_i = os kappa(r_i),   g_ij = d k*_i / d x_j = gf_i Delta_ij / l_j^2   (no division by r):
//     Matern-3/2  gf = -3 os exp(-sqrt3 r)     Matern-5/2  gf = -(5/3) os (1 + sqrt5 r) exp(-sqrt5 r)     RBF  gf = -k*
//   w = (K + s2 I)^-1 k*;   d mean_j = sum_i alpha_i g_ij,   d var_j = -2 sum_i w_i g_ij,
//   d cross_rj = d k(x, p_r) / d x_j - sum_i beta_ri g_ij
//
// bbh_factorize leaves L and X = L^-1 current but not (K + s2 I)^-1 (only a fit evaluation builds that), so the first call
// after a factorisation forms M = X^T X once, into a buffer of its own, with the library's GEMM.
//
// One workgroup per 16 candidates.  LDS holds two [16][np + 16] tiles: k* (replaced by w once the values are out) and gf;
// columns np .. np + p are the pending points, which enter every sum exactly like training points through the rows
// np .. np + 15 of the mean operand [alpha | -beta] (unit weight in their own column).  W = K* M runs on
// v_mfma_f64_16x16x4_f64, four waves sharing the column blocks.  Every sum over the training points runs in ascending order
// in one thread, so a row's results do not depend on its position in the tile or on N: equal rows give equal bits.
#include <math.h>

#include "bbh_common.h"

#define PG_MAXDC 32

struct bbh_postgrad_state {
  double* M = nullptr;    // [np, np] (K + s2 I)^-1 of the current factorisation
  double* par = nullptr;  // [3, dn]  lo | hi - lo | 1 / lengthscale
  int64_t np = 0;
  int dn = 0;
  bool ready = false;
};

struct PostGradArgs {
  const double* X;
  int64_t N, ldx;
  const double *xnT, *pendT, *par, *M, *meanB;
  const int* numcol;
  int n, np, dn, p, dc, kind;
  int colnum[PG_MAXDC];  // numerical column of each differentiated comp-rep column
  double os, ybar, ysd, mean_const;
  double *mean, *var, *cross, *dmean, *dvar, *dcross;
};

__global__ __launch_bounds__(256) void bbh_postgrad_kernel(const PostGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) double pg_lds[];
  const int np = a.np, dn = a.dn, ne = np + 16;
  const int LD = ne + 2;  // row pitch: the 16 rows of a column fall on 16 different bank pairs
  double* s_k = pg_lds;           // [16][LD] k*, then w
  double* s_g = s_k + 16 * LD;    // [16][LD] gf
  double* s_x = s_g + 16 * LD;    // [16][dn] normalised candidate coordinates
  double* s_red = s_x + 16 * dn;  // [4][16]  per-wave partial sums of k* . w
  int* s_col = (int*)(s_red + 64);
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const int64_t tile0 = (int64_t)blockIdx.x * 16;
  const double* lo = a.par;
  const double* rng = a.par + dn;
  const double* il = a.par + 2 * dn;

  if (t < PG_MAXDC) s_col[t] = t < a.dc ? a.colnum[t] : 0;
  for (int e = t; e < 16 * dn; e += 256) {
    const int c = e / dn, j = e - c * dn;
    int64_t gi = tile0 + c;
    if (gi >= a.N) gi = a.N - 1;  // (rows beyond N repeat the last row and are not stored)
    s_x[e] = (a.X[gi * a.ldx + a.numcol[j]] - lo[j]) / rng[j];
  }
  __syncthreads();

  // ---- k* and gf of the tile against the training points and the pending points ----
  for (int c = 0; c < 16; c++)
    for (int i = t; i < ne; i += 256) {
      double kv = 0.0, gf = 0.0;
      if (i < a.n || (i >= np && i - np < a.p)) {
        double r2 = 0.0;
        for (int j = 0; j < dn; j++) {
          const double xt = i < np ? a.xnT[(int64_t)j * np + i] : a.pendT[j * 16 + (i - np)];
          const double sd = (s_x[c * dn + j] - xt) * il[j];
          r2 = fma(sd, sd, r2);
        }
        r2 = r2 > 1e-30 ? r2 : 1e-30;  // gpytorch's distance: sqrt(clamp_min(r^2, 1e-30))
        if (a.kind == BBH_KERNEL_RBF) {
          kv = a.os * exp(-0.5 * r2);
          gf = -kv;
        } else if (a.kind == BBH_KERNEL_MATERN52) {
          const double r = sqrt(r2), ex = exp(-BBH_SQRT5 * r);
          kv = a.os * ((1.0 + BBH_SQRT5 * r + (5.0 / 3.0) * r2) * ex);
          gf = -(5.0 / 3.0) * a.os * ((1.0 + BBH_SQRT5 * r) * ex);
        } else {
          const double r = sqrt(r2), ex = exp(-BBH_SQRT3 * r);
          kv = a.os * ((1.0 + BBH_SQRT3 * r) * ex);
          gf = -3.0 * a.os * ex;
        }
      }
      s_k[c * LD + i] = kv;
      s_g[c * LD + i] = gf;
    }
  __syncthreads();

  const int c = t & 15, jl = t >> 4;  // thread (candidate, column slot) of the sums below
  const int64_t gi = tile0 + c;
  const double s2 = a.ysd * a.ysd;

  // ---- mean and cross: column jl of [alpha | -beta] against k*, ascending ----
  {
    double acc = 0.0;
    for (int i = 0; i < a.n; i++) acc = fma(a.meanB[i * 16 + jl], s_k[c * LD + i], acc);
    for (int i = np; i < np + a.p; i++) acc = fma(a.meanB[i * 16 + jl], s_k[c * LD + i], acc);
    if (gi < a.N) {
      if (jl == 0)
        a.mean[gi] = a.ybar + a.ysd * (a.mean_const + acc);
      else if (jl <= a.p)
        a.cross[gi * a.p + (jl - 1)] = s2 * acc;
    }
  }

  // ---- W = K* M: wave w owns the column blocks w, w + 4, ... ----
  const int nbw = np / 64;
  d4 acc[8];
#pragma unroll
  for (int b = 0; b < 8; b++) acc[b] = d4{0.0, 0.0, 0.0, 0.0};
  {
    const int steps = (a.n + 3) / 4;
    for (int s = 0; s < steps; s++) {
      const int krow = 4 * s + (l >> 4);
      const double av = s_k[(l & 15) * LD + krow];
      const double* mrow = a.M + (int64_t)krow * np + (l & 15);
#pragma unroll
      for (int b = 0; b < 8; b++)
        if (b < nbw) acc[b] = mfma_f64(av, krow < a.n ? mrow[(w + 4 * b) * 16] : 0.0, acc[b]);
    }
  }
  // var = s2 (os - k* . w): lane l, register r holds w[candidate (l >> 4) + 4 r][point 16 blk + (l & 15)]
  {
    double part[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int b = 0; b < 8; b++)
      if (b < nbw) {
#pragma unroll
        for (int r = 0; r < 4; r++) part[r] = fma(acc[b][r], s_k[((l >> 4) + 4 * r) * LD + (w + 4 * b) * 16 + (l & 15)], part[r]);
      }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      double s = part[r];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      s += __shfl_xor(s, 8, 64);
      if ((l & 15) == 0) s_red[w * 16 + (l >> 4) + 4 * r] = s;
    }
  }
  __syncthreads();  // every read of k* is done
  if (t < 16 && tile0 + t < a.N) a.var[tile0 + t] = s2 * (a.os - (((s_red[t] + s_red[16 + t]) + s_red[32 + t]) + s_red[48 + t]));
#pragma unroll
  for (int b = 0; b < 8; b++)
    if (b < nbw) {
#pragma unroll
      for (int r = 0; r < 4; r++) s_k[((l >> 4) + 4 * r) * LD + (w + 4 * b) * 16 + (l & 15)] = acc[b][r];
    }
  s_k[c * LD + np + jl] = 0.0;  // a pending point has no weight in the variance
  __syncthreads();

  // ---- derivatives: thread (c, jl) owns the columns jl and jl + 16; one ascending pass over the points ----
  const bool has0 = jl < a.dc, has1 = jl + 16 < a.dc;
  if (!has0) return;
  const int n0 = s_col[jl], n1 = has1 ? s_col[jl + 16] : n0;
  const double x0 = s_x[c * dn + n0], x1 = s_x[c * dn + n1];
  const double q0 = il[n0] * il[n0], q1 = il[n1] * il[n1];
  double am0 = 0.0, am1 = 0.0, av0 = 0.0, av1 = 0.0, ac0[15], ac1[15];
#pragma unroll
  for (int r = 0; r < 15; r++) ac0[r] = ac1[r] = 0.0;
  const int p = a.p;
  for (int pass = 0; pass < 2; pass++) {
    const int i0 = pass ? np : 0, i1 = pass ? np + p : a.n;
    for (int i = i0; i < i1; i++) {
      const double gf = s_g[c * LD + i], wv = s_k[c * LD + i];
      const double* bm = a.meanB + i * 16;
      const double t0 = pass ? a.pendT[n0 * 16 + (i - np)] : a.xnT[(int64_t)n0 * np + i];
      const double t1 = pass ? a.pendT[n1 * 16 + (i - np)] : a.xnT[(int64_t)n1 * np + i];
      const double d0 = x0 - t0, d1 = x1 - t1;  // the differences stay differences: nothing is contracted into them
      const double g0 = gf * (d0 * q0), g1 = gf * (d1 * q1);
      const double al = bm[0];
      am0 = fma(al, g0, am0);
      am1 = fma(al, g1, am1);
      av0 = fma(wv, g0, av0);
      av1 = fma(wv, g1, av1);
#pragma unroll
      for (int r = 0; r < 15; r++)
        if (r < p) {
          const double b = bm[1 + r];
          ac0[r] = fma(b, g0, ac0[r]);
          ac1[r] = fma(b, g1, ac1[r]);
        }
    }
  }
  if (gi >= a.N) return;
  const double ir0 = 1.0 / rng[n0], ir1 = 1.0 / rng[n1];
  a.dmean[gi * a.dc + jl] = a.ysd * am0 * ir0;
  a.dvar[gi * a.dc + jl] = -2.0 * s2 * av0 * ir0;
  if (has1) {
    a.dmean[gi * a.dc + jl + 16] = a.ysd * am1 * ir1;
    a.dvar[gi * a.dc + jl + 16] = -2.0 * s2 * av1 * ir1;
  }
#pragma unroll
  for (int r = 0; r < 15; r++)
    if (r < p) {
      a.dcross[(gi * p + r) * a.dc + jl] = s2 * ac0[r] * ir0;
      if (has1) a.dcross[(gi * p + r) * a.dc + jl + 16] = s2 * ac1[r] * ir1;
    }
}

void bbh_postgrad_invalidate(bbh_handle* h) {
  if (h->postgrad_state) ((bbh_postgrad_state*)h->postgrad_state)->ready = false;
}

void bbh_postgrad_destroy(bbh_handle* h) {
  bbh_postgrad_state* st = (bbh_postgrad_state*)h->postgrad_state;
  if (!st) return;
  if (st->M) hipFree(st->M);
  if (st->par) hipFree(st->par);
  delete st;
  h->postgrad_state = nullptr;
}

// (K + s2 I)^-1 = X^T X and the per-column constants of the current factorisation
static int bbh_postgrad_setup(bbh_handle* h) {
  if (!h->postgrad_state) h->postgrad_state = new bbh_postgrad_state();
  bbh_postgrad_state* st = (bbh_postgrad_state*)h->postgrad_state;
  if (st->ready) return 0;
  const int64_t np = h->np;
  const int dn = h->dn;
  if (st->np != np || st->dn != dn) {
    if (st->M) hipFree(st->M);
    if (st->par) hipFree(st->par);
    st->M = st->par = nullptr;
    st->np = 0;
    BBH_HIP_TRY(h, hipMalloc((void**)&st->M, sizeof(double) * np * np));
    BBH_HIP_TRY(h, hipMalloc((void**)&st->par, sizeof(double) * 3 * dn));
    st->np = np;
    st->dn = dn;
  }
  bbh_gemm(h->stream, true, false, np, np, np, 1.0, h->d_X, np, 0, h->d_X, np, 0, 0.0, st->M, np, 0, 1);
  std::vector<double> par(3 * (size_t)dn);
  for (int j = 0; j < dn; j++) {
    par[j] = h->lo[j];
    par[dn + j] = h->hi[j] - h->lo[j];
    par[2 * dn + j] = 1.0 / h->theta[3 + j];
  }
  BBH_HIP_TRY(h, hipMemcpyAsync(st->par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, h->stream));
  BBH_HIP_TRY(h, hipStreamSynchronize(h->stream));  // (pageable staging vector)
  st->ready = true;
  return 0;
}

extern "C" int bbh_posterior_grad(bbh_handle* h, const double* X_dev, int64_t N, int64_t ldx, const int32_t* cols_host, int32_t dc,
                                  double* mean_dev, double* var_dev, double* cross_dev, double* dmean_dev, double* dvar_dev,
                                  double* dcross_dev) {
  if (!h) return -1;
  if (!h->factorized) {
    h->err = "bbh_posterior_grad: model not factorised";
    return -1;
  }
  const int kind = h->desc.kernel_kind;
  if (bbh_is_rff(h) || h->F != 1 || (kind != BBH_KERNEL_MATERN32 && kind != BBH_KERNEL_MATERN52 && kind != BBH_KERNEL_RBF)) {
    h->err = "bbh_posterior_grad: needs a single Matern-3/2, Matern-5/2 or RBF kernel (no composite, RFF or other kind)";
    return -1;
  }
  if (h->T != 1 || h->hadamard) {
    h->err = "bbh_posterior_grad: needs a single-task model";
    return -1;
  }
  if (h->n > 512) {
    h->err = "bbh_posterior_grad: at most 512 training points (n = " + std::to_string(h->n) + ")";
    return -1;
  }
  if (dc < 1 || dc > PG_MAXDC || !cols_host) {
    h->err = "bbh_posterior_grad: 1 <= dc <= 32 differentiated columns";
    return -1;
  }
  if (N < 0 || (N > 0 && !X_dev) || ldx < h->desc.d || !mean_dev || !var_dev || !dmean_dev || !dvar_dev ||
      (h->p > 0 && (!cross_dev || !dcross_dev))) {
    h->err = "bbh_posterior_grad: bad arguments (need ldx >= d and every output; the cross outputs may be null only without pending points)";
    return -1;
  }
  PostGradArgs a{};
  for (int k = 0; k < dc; k++) {
    int nj = -1;
    for (int j = 0; j < h->dn; j++)
      if (h->numcol[j] == cols_host[k]) nj = j;
    if (nj < 0 || (k > 0 && cols_host[k] <= cols_host[k - 1])) {
      h->err = "bbh_posterior_grad: cols must be ascending numerical columns of the model";
      return -1;
    }
    a.colnum[k] = nj;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  const int64_t np = h->np;
  const size_t lds = sizeof(double) * (2 * 16 * (size_t)(np + 18) + 16 * (size_t)h->dn + 64) + sizeof(int) * PG_MAXDC;
  if (lds > h->lds_per_block) {
    h->err = "bbh_posterior_grad: the tile does not fit the device's LDS (too many numerical columns)";
    return -1;
  }
  int rc = bbh_postgrad_setup(h);
  if (rc) return rc;
  const bbh_postgrad_state* st = (const bbh_postgrad_state*)h->postgrad_state;
  a.X = X_dev;
  a.N = N;
  a.ldx = ldx;
  a.xnT = h->d_xnT;
  a.pendT = h->d_pendT;
  a.par = st->par;
  a.M = st->M;
  a.meanB = h->d_meanB;
  a.numcol = h->d_numcol;
  a.n = (int)h->n;
  a.np = (int)np;
  a.dn = h->dn;
  a.p = h->p;
  a.dc = dc;
  a.kind = kind;
  a.os = h->desc.use_outputscale ? h->theta[2] : 1.0;
  a.ybar = h->ybar;
  a.ysd = h->ysd;
  a.mean_const = h->theta[1];
  a.mean = mean_dev;
  a.var = var_dev;
  a.cross = cross_dev;
  a.dmean = dmean_dev;
  a.dvar = dvar_dev;
  a.dcross = dcross_dev;
  BBH_HIP_TRY(h, bbh_allow_lds(h->device, (const void*)bbh_postgrad_kernel, lds));
  hipLaunchKernelGGL(bbh_postgrad_kernel, dim3((unsigned)((N + 15) / 16)), dim3(256), lds, h->stream, a);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}
