// k-medoids clustering (method "alternate") over the device-resident candidate matrix.
//
// What the reference does here (baybe/utils/clustering_algorithms/third_party/kmedoids.py, driven by PAMClusteringRecommender,
// baybe/recommenders/pure/nonpredictive/clustering.py:100-132): build the full N x N distance matrix on the host
// (sklearn.metrics.pairwise_distances, kmedoids.py:231: 80 GB at N = 1e5), seed k medoids (k-medoids++ or random), then alternate
// between labelling every point with its nearest medoid and moving every medoid to the member with the smallest sum of in-cluster
// distances.  Here the matrix never exists:
//
//   bbh_pam_dist_rows_kernel     dist(rows[t], j) for T given rows: the rows of D the k-medoids++ set-up reads.
//   bbh_pam_assign_kernel        label[j] / dist[j]: one thread per row j, the medoids' coordinates staged in LDS as [k][TC] tiles
//                                (TC medoids per tile, chosen so that d * TC doubles fit), eight medoids' chains in flight, compared
//                                in ascending cluster order with a strict <.
//   bbh_pam_table_kernel         the grid of the cost kernel: one (cluster, row tile) pair per workgroup, so unequal clusters balance.
//   bbh_pam_cost_kernel<DP>      the in-cluster cost, d <= 32: the points arrive GROUPED by label (stable: position order survives
//                                inside a cluster), one thread per row i with its DP >= d coordinates in registers, tiles of 64
//                                rows j of the same cluster staged in LDS as [j][DP] and visited in ascending order; four d^2 chains
//                                in flight, their square roots added to the running cost one by one in j order.
//   bbh_pam_cost_generic_kernel  the same for any d <= 768: eight chains per thread, x_i re-read per group of eight j, the j tile in
//                                LDS as [k][TJ].
//   bbh_pam_update_kernel        one workgroup per cluster: minimum cost at the smallest position, curr_cost, the strict comparison,
//                                the empty / changed flags.
//
// The deciding values:  d^2(x, y) = sum_k (x_k - y_k) * (x_k - y_k),  k ascending from 0.0, subtract / multiply / add each rounded
// to fp64 (contraction is off for the whole file), dist = sqrt(d^2) correctly rounded, and DISTANCES - not squares - are compared and
// summed, as in the reference.  A cost is the sequential sum over the members in ascending position: np.cumsum(v)[-1].  Padding
// lanes add nothing (they are skipped, not added as zeros of another point).  Every tie goes to the first in position / cluster
// order.  No entry point keeps state: all buffers are the caller's, all launches asynchronous on the handle's stream.
#include <math.h>

#include "bbh_common.h"

#pragma clang fp contract(off)

#define PAM_TI 256          // rows i per workgroup (one per thread)
#define PAM_TJ 64           // rows j per LDS tile of the register form
#define PAM_MAX_D 768       // an 8-column tile of d coordinates within the default LDS limit
#define PAM_MAX_ROWS 2147483392ll  // positions are 32-bit inside the kernels (2^31 - 256)

namespace {

__device__ __forceinline__ double pam_sqrt(double x) { return __dsqrt_rn(x); }

// tile width (log2) of a [d][T] LDS tile of doubles within 48 KB
inline int pam_tile_shift(int d) { return (d <= 96) ? 6 : (d <= 192) ? 5 : (d <= 384) ? 4 : 3; }

int pam_check_matrix(bbh_handle* h, const char* who, const double* P_dev, int64_t M, int32_t d, int64_t ldp) {
  if (!P_dev || M < 1 || M > PAM_MAX_ROWS || d < 1 || d > PAM_MAX_D || ldp < M) {
    h->err = std::string(who) + ": bad arguments (need the matrix, 1 <= M < 2^31 - 256, 1 <= d <= 768, ld >= M)";
    return -1;
  }
  return 0;
}

}  // namespace

// out[t][j] = dist(rows[t], j)
__global__ __launch_bounds__(256) void bbh_pam_dist_rows_kernel(const double* __restrict__ P, int64_t ldp, int64_t M, int d,
                                                                const int64_t* __restrict__ rows, int T, double* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int t = blockIdx.y;
  if (j >= M || t >= T) return;
  const int64_t r = rows[t];
  double v = NAN;
  if (r >= 0 && r < M) {
    double acc = 0.0;
    for (int k = 0; k < d; k++) {
      const double s = P[(int64_t)k * ldp + r] - P[(int64_t)k * ldp + j];
      acc = acc + s * s;
    }
    v = pam_sqrt(acc);
  }
  out[(int64_t)t * M + j] = v;
}

// LDS tile [k][TC] of medoid coordinates (TC = 1 << tc_shift, a multiple of 8), dynamic LDS d * TC doubles
__global__ __launch_bounds__(256) void bbh_pam_assign_kernel(const double* __restrict__ P, int64_t ldp, int64_t M, int d,
                                                             const int64_t* __restrict__ medoids, int64_t K, int tc_shift,
                                                             int* __restrict__ labels, double* __restrict__ dist) {
  extern __shared__ double s_med[];
  const int TC = 1 << tc_shift;
  const int tid = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * 256 + tid;
  const double* Pj = P + ((j < M) ? j : 0);  // (a valid address for the idle lanes)
  double best = INFINITY;
  int64_t lab = 0;
  for (int64_t c0 = 0; c0 < K; c0 += TC) {
    __syncthreads();
    for (int e = tid; e < d * TC; e += 256) {
      const int k = e >> tc_shift;
      const int64_t c = c0 + (e & (TC - 1));
      double v = NAN;  // beyond K or an index out of range: never the minimum
      if (c < K) {
        const int64_t m = medoids[c];
        if (m >= 0 && m < M) v = P[(int64_t)k * ldp + m];
      }
      s_med[e] = v;
    }
    __syncthreads();
    const int64_t left = K - c0;
    const int nc = (left < TC) ? (int)left : TC;
    for (int cc = 0; cc < nc; cc += 8) {
      double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int k = 0; k < d; k++) {
        const double x = Pj[(int64_t)k * ldp];
        const double* ms = s_med + k * TC + cc;
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const double t = ms[u] - x;
          acc[u] = acc[u] + t * t;
        }
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const double v = pam_sqrt(acc[u]);  // ascending cluster index, strict <: the smallest index of equal distances stays
        if (v < best) best = v, lab = c0 + cc + u;
      }
    }
  }
  if (j < M) {
    labels[j] = (int)lab;
    dist[j] = best;
  }
}

// table[2 t] = cluster, table[2 t + 1] = row tile inside the cluster, for t in [tile_starts[c], tile_starts[c + 1])
__global__ __launch_bounds__(256) void bbh_pam_table_kernel(const int64_t* __restrict__ tile_starts, int64_t K, int64_t max_tiles,
                                                            int* __restrict__ table) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= K) return;
  int64_t t0 = tile_starts[c], t1 = tile_starts[c + 1];
  if (t0 < 0) t0 = 0;
  if (t1 > max_tiles) t1 = max_tiles;
  for (int64_t t = t0; t < t1; t++) {
    table[2 * t] = (int)c;
    table[2 * t + 1] = (int)(t - t0);
  }
}

struct PamCostArgs {
  const double* Ps;  // [d][lds], grouped by label
  int64_t lds;
  int M, d;
  const int64_t* starts;       // [K + 1]
  const int64_t* tile_starts;  // [K + 1]
  int64_t K, max_tiles;
  const int* table;
  double* cost;  // [M], by grouped column
};

// the (cluster, tile) of this workgroup: rows [i0, end) are its i, [start, end) its j.  false: nothing to do.
__device__ __forceinline__ bool pam_cost_range(const PamCostArgs& A, int& start, int& end, int& i0) {
  int64_t total = A.tile_starts[A.K];
  if (total > A.max_tiles) total = A.max_tiles;
  if ((int64_t)blockIdx.x >= total) return false;
  const int64_t c = A.table[2 * (int64_t)blockIdx.x];
  const int64_t t = A.table[2 * (int64_t)blockIdx.x + 1];
  if (c < 0 || c >= A.K || t < 0) return false;
  int64_t s = A.starts[c], e = A.starts[c + 1];
  if (s < 0) s = 0;
  if (e > A.M) e = A.M;
  const int64_t first = s + t * PAM_TI;
  if (first >= e) return false;
  start = (int)s, end = (int)e, i0 = (int)first;
  return true;
}

template <int DP>
__global__ __launch_bounds__(256) void bbh_pam_cost_kernel(const PamCostArgs A) {
  __shared__ double s_x[PAM_TJ * DP];  // [j][DP]
  constexpr int NPRE = (PAM_TJ * DP + 255) / 256;
  int start, end, i0;
  if (!pam_cost_range(A, start, end, i0)) return;  // (uniform)
  const int tid = threadIdx.x;
  const int i = i0 + tid;
  const bool live_i = i < end;
  double xi[DP];
#pragma unroll
  for (int k = 0; k < DP; k++) xi[k] = (k < A.d && live_i) ? A.Ps[(int64_t)k * A.lds + i] : 0.0;
  double pre[NPRE];
  auto load = [&](int jt) {
#pragma unroll
    for (int u = 0; u < NPRE; u++) {
      const int e = tid + u * 256;
      const int k = e >> 6, j = jt + (e & 63);
      pre[u] = (k < A.d && j < end) ? A.Ps[(int64_t)k * A.lds + j] : 0.0;
    }
  };
  double cost = 0.0;
  load(start);
  for (int j0 = start; j0 < end; j0 += PAM_TJ) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NPRE; u++) {
      const int e = tid + u * 256;
      if (e < PAM_TJ * DP) s_x[(e & 63) * DP + (e >> 6)] = pre[u];
    }
    __syncthreads();
    if (j0 + PAM_TJ < end) load(j0 + PAM_TJ);  // in flight during the tile's arithmetic
    const int nj = (end - j0 < PAM_TJ) ? end - j0 : PAM_TJ;
    for (int jj = 0; jj < nj; jj += 4) {
      const double* x0 = s_x + jj * DP;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
      for (int k = 0; k < DP; k++) {
        const double t0 = xi[k] - x0[k], t1 = xi[k] - x0[DP + k], t2 = xi[k] - x0[2 * DP + k], t3 = xi[k] - x0[3 * DP + k];
        a0 = a0 + t0 * t0;
        a1 = a1 + t1 * t1;
        a2 = a2 + t2 * t2;
        a3 = a3 + t3 * t3;
      }
      const double r0 = pam_sqrt(a0), r1 = pam_sqrt(a1), r2 = pam_sqrt(a2), r3 = pam_sqrt(a3);
      // the four chains ran side by side; the sum takes them in j order, and only the j that exist
      cost = cost + r0;
      if (jj + 1 < nj) cost = cost + r1;
      if (jj + 2 < nj) cost = cost + r2;
      if (jj + 3 < nj) cost = cost + r3;
    }
  }
  if (live_i) A.cost[i] = cost;
}

// any d: LDS tile [k][TJ] (TJ = 1 << tj_shift in {8, 16, 32, 64}), dynamic LDS d * TJ doubles
__global__ __launch_bounds__(256) void bbh_pam_cost_generic_kernel(const PamCostArgs A, int tj_shift) {
  extern __shared__ double s_xg[];
  int start, end, i0;
  if (!pam_cost_range(A, start, end, i0)) return;
  const int TJ = 1 << tj_shift;
  const int tid = threadIdx.x;
  const int i = i0 + tid;
  const bool live_i = i < end;
  const double* Pi = A.Ps + (live_i ? i : i0);  // (i0 < end: a valid address for the idle lanes)
  double cost = 0.0;
  for (int j0 = start; j0 < end; j0 += TJ) {
    __syncthreads();
    for (int e = tid; e < A.d * TJ; e += 256) {
      const int k = e >> tj_shift, j = j0 + (e & (TJ - 1));
      s_xg[e] = (j < end) ? A.Ps[(int64_t)k * A.lds + j] : 0.0;
    }
    __syncthreads();
    const int nj = (end - j0 < TJ) ? end - j0 : TJ;
    for (int jj = 0; jj < nj; jj += 8) {
      double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int k = 0; k < A.d; k++) {
        const double x = Pi[(int64_t)k * A.lds];
        const double* xs = s_xg + k * TJ + jj;
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const double t = x - xs[u];
          acc[u] = acc[u] + t * t;
        }
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const double r = pam_sqrt(acc[u]);
        if (jj + u < nj) cost = cost + r;  // j order
      }
    }
  }
  if (live_i) A.cost[i] = cost;
}

// One workgroup per cluster.  flags[c]: 1 = empty, 2 = medoid changed, 0 = neither.
__global__ __launch_bounds__(256) void bbh_pam_update_kernel(const double* __restrict__ cost, const int64_t* __restrict__ perm, int64_t M,
                                                             const int64_t* __restrict__ starts, int64_t* __restrict__ medoids,
                                                             int* __restrict__ flags) {
  __shared__ double s_v[4];
  __shared__ long long s_s[4];
  __shared__ long long s_cur;
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x;
  int64_t s0 = starts[c], s1 = starts[c + 1];
  if (s0 < 0) s0 = 0;
  if (s1 > M) s1 = M;
  if (s0 >= s1) {  // "Cluster k is empty!": skipped (kmedoids.py:317-324)
    if (tid == 0) flags[c] = 1;
    return;
  }
  const int64_t med = medoids[c];
  if (tid == 0) s_cur = -1;
  __syncthreads();
  double v = INFINITY;
  long long vs = -1;  // grouped column of the minimum; -1: none yet
  for (int64_t s = s0 + tid; s < s1; s += 256) {
    const double x = cost[s];
    if (vs < 0 || x < v) v = x, vs = s;  // ascending s, strict <: the smallest column of equal costs stays
    if (perm[s] == med) s_cur = s;        // (positions are unique: at most one writer)
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const long long os = __shfl_xor(vs, o, 64);
    if (os >= 0 && (vs < 0 || ov < v || (ov == v && os < vs))) v = ov, vs = os;
  }
  if ((tid & 63) == 0) s_v[tid >> 6] = v, s_s[tid >> 6] = vs;
  __syncthreads();
  if (tid == 0) {
    v = s_v[0], vs = s_s[0];
    for (int w = 1; w < 4; w++) {
      const double ov = s_v[w];
      const long long os = s_s[w];
      if (os >= 0 && (vs < 0 || ov < v || (ov == v && os < vs))) v = ov, vs = os;
    }
    const double curr = cost[(s_cur >= 0) ? s_cur : s0];  // a medoid outside its own cluster: the first member's cost
    int f = 0;
    if (v < curr) {
      const int64_t m = perm[vs];
      if (m != med) f = 2;
      medoids[c] = m;
    }
    flags[c] = f;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
extern "C" int bbh_pam_dist_rows(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, const int64_t* rows_dev, int64_t T,
                                 double* out_dev) {
  if (!h) return -1;
  int rc = pam_check_matrix(h, "bbh_pam_dist_rows", P_dev, M, d, ldp);
  if (rc) return rc;
  if (!rows_dev || !out_dev || T < 1 || T > 65535) {
    h->err = "bbh_pam_dist_rows: bad arguments (need the rows, the output and 1 <= T <= 65535)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(bbh_pam_dist_rows_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)T), dim3(256), 0, h->stream, P_dev, ldp, M, (int)d,
                     rows_dev, (int)T, out_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

extern "C" int bbh_pam_assign(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, const int64_t* medoids_dev, int64_t k,
                              int32_t* labels_dev, double* dist_dev) {
  if (!h) return -1;
  int rc = pam_check_matrix(h, "bbh_pam_assign", P_dev, M, d, ldp);
  if (rc) return rc;
  if (!medoids_dev || !labels_dev || !dist_dev || k < 1 || k > M) {
    h->err = "bbh_pam_assign: bad arguments (need the medoids, both outputs and 1 <= k <= M)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  const int tc_shift = pam_tile_shift(d);
  const size_t lds = sizeof(double) * (size_t)d * ((size_t)1 << tc_shift);  // <= 48 KB
  hipLaunchKernelGGL(bbh_pam_assign_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), lds, h->stream, P_dev, ldp, M, (int)d, medoids_dev, k,
                     tc_shift, labels_dev, dist_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

template <int DP>
static void pam_launch_cost(bbh_handle* h, unsigned grid, const PamCostArgs& a) {
  hipLaunchKernelGGL(bbh_pam_cost_kernel<DP>, dim3(grid), dim3(256), 0, h->stream, a);
}

extern "C" int bbh_pam_cost(bbh_handle* h, const double* Ps_dev, int64_t M, int32_t d, int64_t lds, const int64_t* starts_dev,
                            const int64_t* tile_starts_dev, int64_t k, int32_t* table_dev, int64_t max_tiles, double* cost_dev) {
  if (!h) return -1;
  int rc = pam_check_matrix(h, "bbh_pam_cost", Ps_dev, M, d, lds);
  if (rc) return rc;
  if (!starts_dev || !tile_starts_dev || !table_dev || !cost_dev || k < 1 || k > M || max_tiles < M / PAM_TI + k ||
      max_tiles > 2147483647ll) {
    h->err = "bbh_pam_cost: bad arguments (need both prefix arrays, the table, the output, 1 <= k <= M and M / 256 + k <= max_tiles < 2^31)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(bbh_pam_table_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, h->stream, tile_starts_dev, k, max_tiles, table_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  PamCostArgs a;
  a.Ps = Ps_dev, a.lds = lds, a.M = (int)M, a.d = (int)d, a.starts = starts_dev, a.tile_starts = tile_starts_dev, a.K = k;
  a.max_tiles = max_tiles, a.table = table_dev, a.cost = cost_dev;
  const unsigned grid = (unsigned)(M / PAM_TI + k);  // sum_c ceil(n_c / 256) never exceeds it; surplus workgroups leave at once
  if (d <= 2) pam_launch_cost<2>(h, grid, a);
  else if (d <= 4) pam_launch_cost<4>(h, grid, a);
  else if (d <= 8) pam_launch_cost<8>(h, grid, a);
  else if (d <= 12) pam_launch_cost<12>(h, grid, a);
  else if (d <= 16) pam_launch_cost<16>(h, grid, a);
  else if (d <= 20) pam_launch_cost<20>(h, grid, a);
  else if (d <= 24) pam_launch_cost<24>(h, grid, a);
  else if (d <= 32) pam_launch_cost<32>(h, grid, a);
  else {
    const int tj_shift = pam_tile_shift(d);
    const size_t bytes = sizeof(double) * (size_t)d * ((size_t)1 << tj_shift);  // <= 48 KB
    hipLaunchKernelGGL(bbh_pam_cost_generic_kernel, dim3(grid), dim3(256), bytes, h->stream, a, tj_shift);
  }
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

extern "C" int bbh_pam_update(bbh_handle* h, const double* cost_dev, const int64_t* perm_dev, int64_t M, const int64_t* starts_dev, int64_t k,
                              int64_t* medoids_dev, int32_t* flags_dev) {
  if (!h) return -1;
  if (!cost_dev || !perm_dev || !starts_dev || !medoids_dev || !flags_dev || M < 1 || M > PAM_MAX_ROWS || k < 1 || k > M) {
    h->err = "bbh_pam_update: bad arguments (need the costs, the permutation, the prefix array, the medoids, the flags, "
             "1 <= M < 2^31 - 256 and 1 <= k <= M)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(bbh_pam_update_kernel, dim3((unsigned)k), dim3(256), 0, h->stream, cost_dev, perm_dev, M, starts_dev, medoids_dev, flags_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}
