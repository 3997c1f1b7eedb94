// qNoisyExpectedHypervolumeImprovement (plain, q' = 1) on the device: qLogNEHVI's set-up unchanged (extended models, per-sample box
// decompositions, pruning, reference point), scored without the smoothing -
//
//   score = (1/S) sum_s sum_{cells of s} prod_o max(min(f_s,o - lo_o, len_o), 0),   f_s,o = sign_o (E[f_o(x) | D, F_b,s,o] + sd_o z_x,s,o)
//
// (oracle/nehvi_oracle.py::hvi_from_cells per sample).  Double precision throughout: unlike the log form there is no power
// tau_max = 0.01 that would absorb single-precision factors.  Geometry of bbh_qlognehvi_lin_kernel: candidates x sample slices,
// the cell data wave-uniform (scalar loads), the slices' partial sums combined in slice order by a finish kernel (no atomics).
// A slice is a fixed number of samples, so a candidate's score does not depend on how many rows are scored with it.
#include <math.h>
#include <string.h>

#include <vector>

#include "bbh_acqmath.h"

namespace {

constexpr int QN_SLICE = 8;  // MC samples per slice

struct QnehviArgs {
  const double* tmat[BBH_MAX_OBJECTIVES];  // [S, N] sample-major conditional means
  const double* var[BBH_MAX_OBJECTIVES];   // [N]
  double sign[BBH_MAX_OBJECTIVES];
  int64_t N;
  int S;
  const double* zx;         // [S, M]
  const int64_t* cell_off;  // [S + 1]
  const double* cell_lo;    // [ncells, M]
  const double* cell_len;   // [ncells, M] side lengths (inf: unbounded above)
  const uint8_t* alive;
};

template <int M>
__global__ __launch_bounds__(256) void bbh_qnehvi_kernel(const QnehviArgs a, double* __restrict__ partial) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  const int s_begin = (int)blockIdx.y * QN_SLICE;
  const int s_end = (s_begin + QN_SLICE < a.S) ? s_begin + QN_SLICE : a.S;
  if (a.alive && !a.alive[i]) {
    partial[(int64_t)blockIdx.y * a.N + i] = 0.0;
    return;
  }
  double sd[M];
#pragma unroll
  for (int o = 0; o < M; o++) sd[o] = bbh_safe_sd(a.var[o][i]);
  double total = 0.0;
  for (int s = s_begin; s < s_end; s++) {
    double f[M];
#pragma unroll
    for (int o = 0; o < M; o++) f[o] = a.sign[o] * fma(sd[o], a.zx[(int64_t)s * M + o], a.tmat[o][(int64_t)s * a.N + i]);
    const int64_t c0 = a.cell_off[s], c1 = a.cell_off[s + 1];
    double ssum = 0.0;
    for (int64_t c = c0; c < c1; c++) {
      double prod = 1.0;
#pragma unroll
      for (int o = 0; o < M; o++) prod *= fmax(fmin(f[o] - a.cell_lo[c * M + o], a.cell_len[c * M + o]), 0.0);
      ssum += prod;
    }
    total += ssum;
  }
  partial[(int64_t)blockIdx.y * a.N + i] = total;
}

__global__ __launch_bounds__(256) void bbh_qnehvi_finish_kernel(const double* __restrict__ partial, int slices, int64_t N, int S,
                                                                const uint8_t* __restrict__ alive, double* __restrict__ scores) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double total = 0.0;
  for (int k = 0; k < slices; k++) total += partial[(int64_t)k * N + i];
  scores[i] = (alive && !alive[i]) ? -INFINITY : total / (double)S;
}

bool qn_fill(QnehviArgs& a, int32_t m, int64_t N, const double* const* tmat_dev, const double* const* var_dev, const double* sign_host,
             int64_t S, const uint8_t* alive_dev) {
  for (int o = 0; o < BBH_MAX_OBJECTIVES; o++) {
    a.tmat[o] = o < m ? tmat_dev[o] : nullptr;
    a.var[o] = o < m ? var_dev[o] : nullptr;
    a.sign[o] = o < m ? sign_host[o] : 1.0;
    if (o < m && N > 0 && (!a.tmat[o] || !a.var[o])) return false;
  }
  a.N = N;
  a.S = (int)S;
  a.alive = alive_dev;
  return true;
}

// every operand on the device: a.zx, a.cell_off, a.cell_lo, a.cell_len set by the caller
int qn_run(bbh_handle* h, const QnehviArgs& a, int m, double* scores_dev) {
  const int64_t slices = ((int64_t)a.S + QN_SLICE - 1) / QN_SLICE;
  int rc = bbh_ensure_ws(h, sizeof(double) * (size_t)slices * (size_t)a.N);
  if (rc) return rc;
  bbh_timed_scope timed(h, BBH_TIMED_NEHVI);
  const dim3 grid((unsigned)((a.N + 255) / 256)), sgrid(grid.x, (unsigned)slices), block(256);
  switch (m) {
    case 1: hipLaunchKernelGGL(bbh_qnehvi_kernel<1>, sgrid, block, 0, h->stream, a, h->d_ws); break;
    case 2: hipLaunchKernelGGL(bbh_qnehvi_kernel<2>, sgrid, block, 0, h->stream, a, h->d_ws); break;
    case 3: hipLaunchKernelGGL(bbh_qnehvi_kernel<3>, sgrid, block, 0, h->stream, a, h->d_ws); break;
    default: hipLaunchKernelGGL(bbh_qnehvi_kernel<4>, sgrid, block, 0, h->stream, a, h->d_ws); break;
  }
  hipLaunchKernelGGL(bbh_qnehvi_finish_kernel, grid, block, 0, h->stream, h->d_ws, (int)slices, a.N, a.S, a.alive, scores_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int bbh_qnehvi_cells(bbh_handle* h, int32_t m, int64_t N, const double* const* tmat_dev, const double* const* var_dev,
                                const double* sign_host, const double* zx_host, int64_t S, const uint8_t* alive_dev, double* scores_dev) {
  if (!h) return -1;
  const bbh_nehvi_state* st = (const bbh_nehvi_state*)h->nehvi_state;
  QnehviArgs a;
  if (m < 1 || m > BBH_MAX_OBJECTIVES || N < 0 || S < 1 || S > 65535 || !tmat_dev || !var_dev || !sign_host || !zx_host || !scores_dev ||
      !st || st->S != S || st->m != m || !qn_fill(a, m, N, tmat_dev, var_dev, sign_host, S, alive_dev)) {
    h->err = "bbh_qnehvi_cells: bad arguments, or no cell lists for this S and m on the handle (bbh_cells_build_dev)";
    return -1;
  }
  if (N == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  int rc = bbh_upload_z(h, zx_host, (size_t)S * m);
  if (rc) return rc;
  a.zx = h->d_z;
  a.cell_off = st->off();
  a.cell_lo = st->lo();
  a.cell_len = st->len();
  return qn_run(h, a, m, scores_dev);
}

extern "C" int bbh_qnehvi_sm(bbh_handle* h, int32_t m, int64_t N, const double* const* tmat_dev, const double* const* var_dev,
                             const double* sign_host, const double* zx_host, int64_t S, const int64_t* cell_off_host,
                             const double* cell_lo_host, const double* cell_loglen_host, const uint8_t* alive_dev, double* scores_dev) {
  if (!h) return -1;
  QnehviArgs a;
  if (m < 1 || m > BBH_MAX_OBJECTIVES || N < 0 || S < 1 || S > 65535 || !tmat_dev || !var_dev || !sign_host || !zx_host || !cell_off_host ||
      !scores_dev || !qn_fill(a, m, N, tmat_dev, var_dev, sign_host, S, alive_dev)) {
    h->err = "bbh_qnehvi_sm: bad arguments (1 <= m <= 4, 1 <= S <= 65535)";
    return -1;
  }
  if (N == 0) return 0;
  const int64_t ncells = cell_off_host[S];
  bool ok = cell_off_host[0] == 0 && ncells >= 0 && (ncells == 0 || (cell_lo_host && cell_loglen_host));
  for (int64_t s = 0; ok && s < S; s++) ok = cell_off_host[s] <= cell_off_host[s + 1];  // (the kernel indexes the cell arrays by these)
  if (!ok) {
    h->err = "bbh_qnehvi_sm: inconsistent cell arrays";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  // one upload: zx [S m] | cell_lo [ncells m] | cell_len [ncells m] | cell_off [S + 1] (int64, 8-byte slots)
  const size_t nd = (size_t)S * m + 2 * (size_t)ncells * m;
  std::vector<double> buf(nd + (size_t)S + 1);
  memcpy(buf.data(), zx_host, sizeof(double) * S * m);
  if (ncells > 0) {
    memcpy(buf.data() + S * m, cell_lo_host, sizeof(double) * ncells * m);
    double* len = buf.data() + S * m + ncells * m;  // side lengths e^ll (inf for cells unbounded above)
    for (int64_t e = 0; e < ncells * m; e++) len[e] = exp(cell_loglen_host[e]);
  }
  memcpy(buf.data() + nd, cell_off_host, sizeof(int64_t) * (S + 1));
  int rc = bbh_upload_z(h, buf.data(), buf.size());
  if (rc) return rc;
  a.zx = h->d_z;
  a.cell_lo = h->d_z + S * m;
  a.cell_len = h->d_z + S * m + ncells * m;
  a.cell_off = (const int64_t*)(h->d_z + nd);
  return qn_run(h, a, m, scores_dev);
}
