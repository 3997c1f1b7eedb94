// qNegIntegratedPosteriorVariance (baybe/acquisition/acqfs.py: qNIPV) over a discrete candidate set: the variance reduction at M
// integration points p_1 .. p_M that conditioning the GP on [x ; B] buys, B = the b <= 15 pending points of the handle.
// Single task, one stationary kernel (Matern-1/2, Matern-3/2, Matern-5/2, RBF), n <= 512.
//
//   A = (K + s2 I)^-1 K(X, P)  [n, M]      H = G^-1 cov(B, P)  [b, M]      G = cov(B, B) + s2 I
//   C_j(x)  = k(x, p_j) - k(x, X) A[:, j] - cov(x, B) H[:, j]               (= cov(p_j, x | B))
//   gain(x) = sum_j C_j(x)^2 / (max(var(x) - cov(x, B) G^-1 cov(B, x), 0) + s2)
//
// bbh_nipv_set_points builds A once per recommendation from the factorisation's X = L^-1 (two multiplications, as
// bbh_pending_set; no explicit inverse) and keeps [A ; H] resident as one [np + 16, Mpad] operand, Mpad = M rounded up to the
// column block of 64.  bbh_nipv_gain is one pass from the candidate matrix to gain[N]:
//
//   (1) a workgroup takes a tile of 16 candidates (32 under BBH_NIPV_TILE=32, measured slower) and forms [k*(x) | cov(x, B) / ysd^2] once in LDS, by direct
//       differences of the normalised coordinates (stage (1) of bbh_postgrad.hip, same row pitch);
//   (2) [k* | cov(x, B)] [A ; H] runs on v_mfma_f64_16x16x4_f64 over column blocks of P; wave w owns the 64-column blocks
//       w, w + 4, ... of the workgroup's column slice;
//   (3) k(x, p_j) is evaluated in the accumulator layout, the difference is squared and added per row in registers: the
//       [N, M] matrix is never written.
//
// The M columns are cut into slices of a fixed width over the second grid dimension (a slice of [A ; H] stays in the L2 while
// the resident workgroups walk the candidate tiles); a second kernel adds the slices in slice order and divides.  Every sum
// has one fixed order that depends on neither the row's place in its tile nor on N: equal rows give equal bits, two runs give
// equal bits.  No floating-point atomics.
#include <math.h>

#include "bbh_common.h"

#define NIPV_COLBLOCK 64                         // columns per wave and pass: Mpad is a multiple of it
#define NIPV_KGROUP 4                            // k-steps per prefetch group of the MFMA loop (16 training rows)
#define NIPV_BUDGET_BYTES ((size_t)256 << 20)    // bound on the resident operand (np + 16) Mpad 8: M = 16384 at np = 512 takes 66 MiB

int bbh_kstar_solve_chunk(bbh_handle* h, const double* X_dev, int64_t Nc, int64_t ldx, double* Kst, double* V, const double* d_lo,
                          const double* d_hi);  // bbh_panel.hip

struct bbh_nipv_state {
  double* Aext = nullptr;  // [np + 16, Mpad]  rows 0 .. np: A; rows np .. np + 16: H of the current pending state
  double* pnT = nullptr;   // [dn, Mpad]       normalised integration points, transposed
  double* par = nullptr;   // [3, dn] lo | hi - lo | 1 / lengthscale, then [16, 16] G^-1
  size_t a_bytes = 0, p_bytes = 0;
  int64_t M = 0, Mpad = 0, np = 0;
  int dn = 0;
  bool ready = false;
  int last_form = -1;
};

struct NipvArgs {
  const double* X;
  int64_t N, ldx;
  const double *xnT, *par, *Aext, *pnT, *cross;
  const int* numcol;
  int n, np, dn, b, kind, slice;
  int64_t M, Mpad;
  double os, inv_y2;
  double* part;  // [slices, N]
};

__device__ __forceinline__ double nipv_kval(int kind, double os, double r2) {
  r2 = r2 > 1e-30 ? r2 : 1e-30;  // gpytorch's distance: sqrt(clamp_min(r^2, 1e-30))
  if (kind == BBH_KERNEL_RBF) return os * exp(-0.5 * r2);
  const double r = sqrt(r2);
  if (kind == BBH_KERNEL_MATERN52) return os * ((1.0 + BBH_SQRT5 * r + (5.0 / 3.0) * r2) * exp(-BBH_SQRT5 * r));
  if (kind == BBH_KERNEL_MATERN32) return os * ((1.0 + BBH_SQRT3 * r) * exp(-BBH_SQRT3 * r));
  return os * exp(-r);
}

// RT row tiles of 16 candidates per workgroup: every B fragment read from [A ; H] feeds RT MFMAs
template <int RT>
__global__ __launch_bounds__(256) void bbh_nipv_kernel(const NipvArgs a) {
  extern __shared__ __attribute__((aligned(16))) double nipv_lds[];
  constexpr int R = 16 * RT;
  const int np = a.np, dn = a.dn, ne = np + 16;
  const int LD = ne + 2;  // row pitch: the 16 rows of a column fall on 16 different bank pairs
  double* s_k = nipv_lds;         // [R][LD] k* | cov(x, B) / ysd^2
  double* s_x = s_k + R * LD;     // [R][dn] normalised candidate coordinates
  double* s_red = s_x + R * dn;   // [4][R]  per-wave partial sums
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const int64_t tile0 = (int64_t)blockIdx.x * R;
  const double* lo = a.par;
  const double* rng = a.par + dn;
  const double* il = a.par + 2 * dn;

  for (int e = t; e < R * dn; e += 256) {
    const int c = e / dn, j = e - c * dn;
    int64_t gi = tile0 + c;
    if (gi >= a.N) gi = a.N - 1;  // (rows beyond N repeat the last row and are not stored)
    s_x[e] = (a.X[gi * a.ldx + a.numcol[j]] - lo[j]) / rng[j];
  }
  __syncthreads();

  // ---- (1) the extended row operand of the tile: a thread owns a training point and reads its coordinates once for the 16 rows
  //      of a row tile (one thread per entry re-read them per row: 0.8 of the 2.0 ms of a 1e5 x 256 pass, KERNELS.md 4.15) ----
  for (int i = t; i < ne; i += 256) {
    if (i < a.n) {
#pragma unroll
      for (int rt = 0; rt < RT; rt++) {
        double r2[16];
#pragma unroll
        for (int c = 0; c < 16; c++) r2[c] = 0.0;
        for (int j = 0; j < dn; j++) {
          const double xt = a.xnT[(int64_t)j * np + i], ilj = il[j];
#pragma unroll
          for (int c = 0; c < 16; c++) {
            const double sd = (s_x[(rt * 16 + c) * dn + j] - xt) * ilj;
            r2[c] = fma(sd, sd, r2[c]);
          }
        }
#pragma unroll
        for (int c = 0; c < 16; c++) s_k[(rt * 16 + c) * LD + i] = nipv_kval(a.kind, a.os, r2[c]);
      }
    } else {
      for (int c = 0; c < R; c++) {
        int64_t gi = tile0 + c;
        if (gi >= a.N) gi = a.N - 1;
        s_k[c * LD + i] = (i >= np && i - np < a.b) ? a.cross[gi * a.b + (i - np)] * a.inv_y2 : 0.0;
      }
    }
  }
  __syncthreads();

  // ---- (2) + (3): the 64-column blocks w, w + 4, ... of this workgroup's slice ----
  const int64_t col_lo = (int64_t)blockIdx.y * a.slice;
  const int64_t col_hi = col_lo + a.slice < a.Mpad ? col_lo + a.slice : a.Mpad;
  const int lc = l & 15, lq = l >> 4;
  double part[RT][4];
#pragma unroll
  for (int rt = 0; rt < RT; rt++)
#pragma unroll
    for (int r = 0; r < 4; r++) part[rt][r] = 0.0;
  const int steps = (a.n + 3) / 4, psteps = (a.b + 3) / 4;
  for (int64_t col0 = col_lo + (int64_t)w * NIPV_COLBLOCK; col0 < col_hi; col0 += 4 * NIPV_COLBLOCK) {
    d4 acc[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
      for (int blk = 0; blk < 4; blk++) acc[rt][blk] = d4{0.0, 0.0, 0.0, 0.0};
    // groups of NIPV_KGROUP k-steps: the B fragments of the next group are in flight while the MFMAs of this one run (rows n .. np of
    // A are zero - the padding of L^-1 is the identity and K(X, P) is zero there - and the rows of k* beyond n are zero in LDS, so the
    // last group needs no guard: np is a multiple of 64)
    const double* bcol = a.Aext + col0 + lc;
    const int groups = (steps + NIPV_KGROUP - 1) / NIPV_KGROUP;
    double bv[NIPV_KGROUP][4], bn[NIPV_KGROUP][4];
#pragma unroll
    for (int u = 0; u < NIPV_KGROUP; u++)
#pragma unroll
      for (int blk = 0; blk < 4; blk++) bv[u][blk] = bcol[(int64_t)(4 * u + lq) * a.Mpad + blk * 16];
    for (int gk = 0; gk < groups; gk++) {
      const int k0 = 4 * NIPV_KGROUP * gk;
      if (gk + 1 < groups) {
#pragma unroll
        for (int u = 0; u < NIPV_KGROUP; u++)
#pragma unroll
          for (int blk = 0; blk < 4; blk++) bn[u][blk] = bcol[(int64_t)(k0 + 4 * NIPV_KGROUP + 4 * u + lq) * a.Mpad + blk * 16];
      } else {
#pragma unroll
        for (int u = 0; u < NIPV_KGROUP; u++)
#pragma unroll
          for (int blk = 0; blk < 4; blk++) bn[u][blk] = 0.0;
      }
#pragma unroll
      for (int u = 0; u < NIPV_KGROUP; u++) {
        const int krow = k0 + 4 * u + lq;
#pragma unroll
        for (int rt = 0; rt < RT; rt++) {
          const double av = s_k[(rt * 16 + lc) * LD + krow];
#pragma unroll
          for (int blk = 0; blk < 4; blk++) acc[rt][blk] = mfma_f64(av, bv[u][blk], acc[rt][blk]);
        }
      }
#pragma unroll
      for (int u = 0; u < NIPV_KGROUP; u++)
#pragma unroll
        for (int blk = 0; blk < 4; blk++) bv[u][blk] = bn[u][blk];
    }
    for (int s = 0; s < psteps; s++) {  // rows np + b .. np + 16 of the operand are zero on both sides
      const int krow = np + 4 * s + lq;
      const double* brow = a.Aext + (int64_t)krow * a.Mpad + col0 + lc;
#pragma unroll
      for (int rt = 0; rt < RT; rt++) {
        const double av = s_k[(rt * 16 + lc) * LD + krow];
#pragma unroll
        for (int blk = 0; blk < 4; blk++) acc[rt][blk] = mfma_f64(av, brow[blk * 16], acc[rt][blk]);
      }
    }
    // lane l, register r of block blk holds row (l >> 4) + 4 r, column col0 + 16 blk + (l & 15)
#pragma unroll
    for (int blk = 0; blk < 4; blk++) {
      const int64_t col = col0 + blk * 16 + lc;
      double r2[RT][4];
#pragma unroll
      for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int r = 0; r < 4; r++) r2[rt][r] = 0.0;
      for (int j = 0; j < dn; j++) {
        const double pj = a.pnT[(int64_t)j * a.Mpad + col], ilj = il[j];
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const double sd = (s_x[(rt * 16 + lq + 4 * r) * dn + j] - pj) * ilj;
            r2[rt][r] = fma(sd, sd, r2[rt][r]);
          }
      }
      const bool live = col < a.M;
#pragma unroll
      for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const double df = nipv_kval(a.kind, a.os, r2[rt][r]) - acc[rt][blk][r];
          part[rt][r] = live ? fma(df, df, part[rt][r]) : part[rt][r];
        }
    }
  }
#pragma unroll
  for (int rt = 0; rt < RT; rt++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      double s = part[rt][r];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      s += __shfl_xor(s, 8, 64);
      if (lc == 0) s_red[w * R + rt * 16 + lq + 4 * r] = s;
    }
  __syncthreads();
  if (t < R && tile0 + t < a.N)
    a.part[(int64_t)blockIdx.y * a.N + tile0 + t] = ((s_red[t] + s_red[R + t]) + s_red[2 * R + t]) + s_red[3 * R + t];
}

// the slices in slice order, then the division: gain = ysd^4 sum / (max(var - cov(x, B) G^-1 cov(B, x), 0) + s2)
__global__ __launch_bounds__(256) void bbh_nipv_finish_kernel(const double* __restrict__ part, int nsl, int64_t N,
                                                              const double* __restrict__ var, const double* __restrict__ cross,
                                                              const double* __restrict__ ginv, int b, double s2, double y4,
                                                              const uint8_t* __restrict__ alive, double* __restrict__ gain) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double sum = 0.0;
  for (int s = 0; s < nsl; s++) sum += part[(int64_t)s * N + i];
  double q = 0.0;
  for (int r = 0; r < b; r++) {
    double tq = 0.0;
    for (int m = 0; m < b; m++) tq = fma(ginv[r * b + m], cross[i * b + m], tq);
    q = fma(cross[i * b + r], tq, q);
  }
  const double red = var[i] - q;
  const double den = (red > 0.0 ? red : 0.0) + s2;
  gain[i] = (alive && !alive[i]) ? -INFINITY : y4 * sum / den;
}

// var(p_j) = ysd^2 (os - |L^-1 k(X, p_j)|^2), ascending over the training points
__global__ __launch_bounds__(256) void bbh_nipv_varp_kernel(const double* __restrict__ Tm, int64_t Mc, int64_t np, double os,
                                                            double y2, double* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= Mc) return;
  double s = 0.0;
  for (int64_t r = 0; r < np; r++) {
    const double v = Tm[j * np + r];
    s = fma(v, v, s);
  }
  out[j] = y2 * (os - s);
}

void bbh_nipv_invalidate(bbh_handle* h) {
  if (h->nipv_state) ((bbh_nipv_state*)h->nipv_state)->ready = false;
}

void bbh_nipv_destroy(bbh_handle* h) {
  bbh_nipv_state* st = (bbh_nipv_state*)h->nipv_state;
  if (!st) return;
  if (st->Aext) hipFree(st->Aext);
  if (st->pnT) hipFree(st->pnT);
  if (st->par) hipFree(st->par);
  delete st;
  h->nipv_state = nullptr;
}

size_t bbh_nipv_resident_bytes(const bbh_handle* h) {
  const bbh_nipv_state* st = (const bbh_nipv_state*)h->nipv_state;
  return st ? st->a_bytes + st->p_bytes : 0;
}

static int bbh_nipv_check_model(bbh_handle* h, const char* who) {
  if (!h->factorized) {
    h->err = std::string(who) + ": model not factorised";
    return -1;
  }
  const int kind = h->desc.kernel_kind;
  if (bbh_is_rff(h) || h->F != 1 || kind < BBH_KERNEL_MATERN12 || kind > BBH_KERNEL_RBF) {
    h->err = std::string(who) + ": needs a single Matern-1/2, Matern-3/2, Matern-5/2 or RBF kernel (no composite, RFF or other kind)";
    return -1;
  }
  if (h->T != 1 || h->hadamard) {
    h->err = std::string(who) + ": needs a single-task model";
    return -1;
  }
  if (h->n > 512) {
    h->err = std::string(who) + ": at most 512 training points (n = " + std::to_string(h->n) + ")";
    return -1;
  }
  return 0;
}

extern "C" int bbh_nipv_set_points(bbh_handle* h, const double* P_host, int64_t M, double* var_p_host) {
  if (!h) return -1;
  int rc = bbh_nipv_check_model(h, "bbh_nipv_set_points");
  if (rc) return rc;
  if (M < 1 || !P_host) {
    h->err = "bbh_nipv_set_points: at least one integration point";
    return -1;
  }
  const int64_t np = h->np, Mpad = bbh_round_up(M, NIPV_COLBLOCK);
  const int d = h->desc.d, dn = h->dn;
  if ((double)(np + 16) * (double)Mpad * 8.0 > (double)NIPV_BUDGET_BYTES) {
    h->err = "bbh_nipv_set_points: " + std::to_string(M) + " integration points need a resident operand of (np + 16) Mpad 8 = " +
             std::to_string((double)(np + 16) * (double)Mpad * 8.0 / 1048576.0) + " MiB at np = " + std::to_string(np) +
             ", over the budget of " + std::to_string(NIPV_BUDGET_BYTES >> 20) + " MiB; use fewer integration points (sampling_n_points / sampling_fraction)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  if (!h->nipv_state) h->nipv_state = new bbh_nipv_state();
  bbh_nipv_state* st = (bbh_nipv_state*)h->nipv_state;
  st->ready = false;
  hipStream_t s = h->stream;
  const size_t a_bytes = sizeof(double) * (size_t)(np + 16) * (size_t)Mpad, p_bytes = sizeof(double) * (size_t)dn * (size_t)Mpad;
  if (a_bytes > st->a_bytes) {
    if (st->Aext) hipFree(st->Aext);
    st->Aext = nullptr;
    st->a_bytes = 0;
    BBH_HIP_TRY(h, hipMalloc((void**)&st->Aext, a_bytes));
    st->a_bytes = a_bytes;
  }
  if (p_bytes > st->p_bytes) {
    if (st->pnT) hipFree(st->pnT);
    st->pnT = nullptr;
    st->p_bytes = 0;
    BBH_HIP_TRY(h, hipMalloc((void**)&st->pnT, p_bytes));
    st->p_bytes = p_bytes;
  }
  if (st->dn != dn || !st->par) {
    if (st->par) hipFree(st->par);
    st->par = nullptr;
    BBH_HIP_TRY(h, hipMalloc((void**)&st->par, sizeof(double) * (3 * (size_t)dn + 256)));
    st->dn = dn;
  }
  st->M = M;
  st->Mpad = Mpad;
  st->np = np;
  // normalised points, transposed (the candidates' own normalisation: equal rows give a distance of exactly zero), and constants
  std::vector<double> pnT((size_t)dn * Mpad, 0.0), par(3 * (size_t)dn);
  for (int64_t j = 0; j < M; j++)
    for (int c = 0; c < dn; c++) pnT[(size_t)c * Mpad + j] = (P_host[j * d + h->numcol[c]] - h->lo[c]) / (h->hi[c] - h->lo[c]);
  for (int c = 0; c < dn; c++) {
    par[c] = h->lo[c];
    par[dn + c] = h->hi[c] - h->lo[c];
    par[2 * dn + c] = 1.0 / h->theta[3 + c];
  }
  BBH_HIP_TRY(h, hipMemcpyAsync(st->pnT, pnT.data(), sizeof(double) * pnT.size(), hipMemcpyHostToDevice, s));
  BBH_HIP_TRY(h, hipMemcpyAsync(st->par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, s));
  BBH_HIP_TRY(h, hipMemsetAsync(st->Aext + np * Mpad, 0, sizeof(double) * 16 * (size_t)Mpad, s));
  // A = X^T (X K(X, P)), X = L^-1, in row chunks of P: workspace raw rows [chunk, d] | Kst [chunk, np] | Tm [chunk, np] | var [chunk] | lo, hi
  const int64_t chunk = Mpad < 2048 ? Mpad : 2048;
  rc = bbh_ensure_ws(h, sizeof(double) * ((size_t)chunk * d + 2 * (size_t)chunk * np + (size_t)chunk + 2 * (size_t)dn));
  if (rc) return rc;
  double* d_xp = h->d_ws;
  double* Kst = d_xp + chunk * d;
  double* Tm = Kst + chunk * np;
  double* d_var = Tm + chunk * np;
  double* d_lo = d_var + chunk;
  double* d_hi = d_lo + dn;
  BBH_HIP_TRY(h, hipMemcpyAsync(d_lo, h->lo.data(), sizeof(double) * dn, hipMemcpyHostToDevice, s));
  BBH_HIP_TRY(h, hipMemcpyAsync(d_hi, h->hi.data(), sizeof(double) * dn, hipMemcpyHostToDevice, s));
  const double os = h->desc.use_outputscale ? h->theta[2] : 1.0;
  for (int64_t c0 = 0; c0 < M; c0 += chunk) {
    const int64_t Mc = M - c0 < chunk ? M - c0 : chunk, Mcpad = bbh_round_up(Mc, 64);
    BBH_HIP_TRY(h, hipMemcpyAsync(d_xp, P_host + c0 * d, sizeof(double) * Mc * d, hipMemcpyHostToDevice, s));
    rc = bbh_kstar_solve_chunk(h, d_xp, Mc, d, Kst, Tm, d_lo, d_hi);  // Tm[j] = (L^-1 k(X, p_j))^T
    if (rc) return rc;
    bbh_gemm(s, true, true, np, Mcpad, np, 1.0, h->d_X, np, 0, Tm, np, 0, 0.0, st->Aext + c0, Mpad, 0, 1);  // A[:, j] = L^-T t_j
    if (var_p_host) {
      hipLaunchKernelGGL(bbh_nipv_varp_kernel, dim3((unsigned)((Mc + 255) / 256)), dim3(256), 0, s, Tm, Mc, np, os, h->ysd * h->ysd, d_var);
      BBH_HIP_TRY(h, hipMemcpyAsync(var_p_host + c0, d_var, sizeof(double) * Mc, hipMemcpyDeviceToHost, s));
    }
    BBH_HIP_TRY(h, hipStreamSynchronize(s));  // (the chunk's workspace is rewritten by the next one; pageable host buffers)
  }
  // the kernel walks the training rows in groups of 16 without a guard: the padding rows n .. np are zero by construction (L^-1 is
  // the identity there and K(X, P) zero), and are written as zero here so that nothing rests on it
  if (np > h->n) BBH_HIP_TRY(h, hipMemsetAsync(st->Aext + h->n * Mpad, 0, sizeof(double) * (size_t)(np - h->n) * (size_t)Mpad, s));
  BBH_HIP_TRY(h, hipGetLastError());
  BBH_HIP_TRY(h, hipStreamSynchronize(s));
  st->ready = true;
  return 0;
}

extern "C" int bbh_nipv_gain(bbh_handle* h, const double* X_dev, int64_t N, int64_t ldx, const double* var_dev, const double* cross_dev,
                             const double* H_host, const double* ginv_host, const uint8_t* alive_dev, double* gain_dev) {
  if (!h) return -1;
  int rc = bbh_nipv_check_model(h, "bbh_nipv_gain");
  if (rc) return rc;
  bbh_nipv_state* st = (bbh_nipv_state*)h->nipv_state;
  if (!st || !st->ready || st->np != h->np) {
    h->err = "bbh_nipv_gain: no integration points set for the current factorisation (bbh_nipv_set_points)";
    return -1;
  }
  const int b = h->p;
  if (N < 0 || (N > 0 && (!X_dev || !var_dev || !gain_dev)) || ldx < h->desc.d || (b > 0 && (!cross_dev || !H_host || !ginv_host))) {
    h->err = "bbh_nipv_gain: bad arguments (need ldx >= d, var and gain; cross, H and G^-1 may be null only without pending points)";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int64_t np = h->np, M = st->M, Mpad = st->Mpad;
  const int dn = h->dn;
  int slice = h->sw.nipv_slice;
  slice = slice <= 0 ? (int)(Mpad < INT_MAX ? Mpad : INT_MAX) : (int)bbh_round_up(slice, NIPV_COLBLOCK);
  const int64_t nsl = (Mpad + slice - 1) / slice;
  if (nsl > 65535) {
    h->err = "bbh_nipv_gain: more than 65535 column slices (BBH_NIPV_SLICE too small)";
    return -1;
  }
  int rt = h->sw.nipv_tile == 32 ? 2 : 1;
  auto lds_of = [&](int r) { return sizeof(double) * ((size_t)16 * r * (size_t)(np + 18) + (size_t)16 * r * dn + (size_t)64 * r); };
  if (rt == 2 && lds_of(2) > h->lds_per_block) rt = 1;
  const size_t lds = lds_of(rt);
  if (lds > h->lds_per_block) {
    h->err = "bbh_nipv_gain: the tile does not fit the device's LDS (too many numerical columns)";
    return -1;
  }
  rc = bbh_ensure_ws(h, sizeof(double) * (size_t)nsl * (size_t)N);
  if (rc) return rc;
  // H of the current pending state into the rows np .. np + b of the operand, G^-1 behind the constants
  BBH_HIP_TRY(h, hipMemsetAsync(st->Aext + np * Mpad, 0, sizeof(double) * 16 * (size_t)Mpad, s));
  double* d_ginv = st->par + 3 * dn;
  if (b > 0) {
    BBH_HIP_TRY(h, hipMemcpy2DAsync(st->Aext + np * Mpad, sizeof(double) * Mpad, H_host, sizeof(double) * M, sizeof(double) * M, b,
                                    hipMemcpyHostToDevice, s));
    BBH_HIP_TRY(h, hipMemcpyAsync(d_ginv, ginv_host, sizeof(double) * b * b, hipMemcpyHostToDevice, s));
    BBH_HIP_TRY(h, hipStreamSynchronize(s));  // (pageable host buffers the caller may reuse)
  }
  NipvArgs a{};
  a.X = X_dev;
  a.N = N;
  a.ldx = ldx;
  a.xnT = h->d_xnT;
  a.par = st->par;
  a.Aext = st->Aext;
  a.pnT = st->pnT;
  a.cross = cross_dev;
  a.numcol = h->d_numcol;
  a.n = (int)h->n;
  a.np = (int)np;
  a.dn = dn;
  a.b = b;
  a.kind = h->desc.kernel_kind;
  a.slice = slice;
  a.M = M;
  a.Mpad = Mpad;
  a.os = h->desc.use_outputscale ? h->theta[2] : 1.0;
  const double y2 = h->ysd * h->ysd;
  a.inv_y2 = 1.0 / y2;
  a.part = h->d_ws;
  const dim3 grid((unsigned)((N + 16 * rt - 1) / (16 * rt)), (unsigned)nsl);
  if (rt == 2) {
    BBH_HIP_TRY(h, bbh_allow_lds(h->device, (const void*)bbh_nipv_kernel<2>, lds));
    hipLaunchKernelGGL(bbh_nipv_kernel<2>, grid, dim3(256), lds, s, a);
  } else {
    BBH_HIP_TRY(h, bbh_allow_lds(h->device, (const void*)bbh_nipv_kernel<1>, lds));
    hipLaunchKernelGGL(bbh_nipv_kernel<1>, grid, dim3(256), lds, s, a);
  }
  hipLaunchKernelGGL(bbh_nipv_finish_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, h->d_ws, (int)nsl, N, var_dev, cross_dev,
                     d_ginv, b, y2 * h->theta[0], y2 * y2, alive_dev, gain_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  st->last_form = rt == 2 ? 1 : 0;
  return 0;
}

extern "C" int bbh_last_nipv_form(bbh_handle* h) {
  if (!h) return -1;
  const bbh_nipv_state* st = (const bbh_nipv_state*)h->nipv_state;
  return st ? st->last_form : -1;
}
