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
// The deciding values: d^2 by the arithmetic contract of bbh_rows.h (the chains, the pair walks and the key reduction come from
// there), dist = sqrt(d^2) correctly rounded, and DISTANCES - not squares - are compared and summed, as in the reference.  A cost is
// the sequential sum over the members in ascending position: np.cumsum(v)[-1].  Padding lanes add nothing (they are skipped, not
// added as zeros of another point).  Every tie goes to the first in position / cluster order.  No entry point keeps state: all
// buffers are the caller's, all launches asynchronous on the handle's stream.
#include "bbh_rows.h"

#define PAM_TI BBH_ROWS_TILE  // rows i per workgroup (one per thread)

namespace {

__device__ __forceinline__ double pam_sqrt(double x) { return __dsqrt_rn(x); }

}  // namespace

// out[t][j] = dist(rows[t], j)
__global__ __launch_bounds__(256) void bbh_pam_dist_rows_kernel(const double* __restrict__ P, int64_t ldp, int64_t M, int d,
                                                                const int64_t* __restrict__ rows, int T, double* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int t = blockIdx.y;
  if (j >= M || t >= T) return;
  const int64_t r = rows[t];
  double v = NAN;
  if (r >= 0 && r < M) v = pam_sqrt(bbh_rows_d2(P, ldp, d, r, j));
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
      double acc[8];
      bbh_rows_d2x8(Pj, ldp, s_med + cc, TC, d, acc);
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

namespace {

// a j beyond the cluster is staged as zero and not visited
struct PamCostLoad {
  static constexpr bool whole_tiles = false;
  int end;
  __device__ __forceinline__ bool live(int j) const { return j < end; }
  __device__ __forceinline__ double pad() const { return 0.0; }
};

// the chains of a group ran side by side; the sum takes their square roots one by one in j order, and only the j that exist
struct PamCostVisit {
  double& cost;
  __device__ __forceinline__ void operator()(int, double d2, bool exists) const {
    const double sum = cost + pam_sqrt(d2);
    cost = exists ? sum : cost;  // (a select, no branch: the chains of a group stay in one block)
  }
};

}  // namespace

template <int DP>
__global__ __launch_bounds__(256) void bbh_pam_cost_kernel(const PamCostArgs A) {
  __shared__ double s_x[BBH_ROWS_TJ * DP];  // [j][DP]
  int start, end, i0;
  if (!pam_cost_range(A, start, end, i0)) return;  // (uniform)
  const int i = i0 + threadIdx.x;
  const bool live_i = i < end;
  double cost = 0.0;
  bbh_rows_pair_walk<DP>(A.Ps, A.lds, A.d, i, live_i, start, end, s_x, PamCostLoad{end}, PamCostVisit{cost});
  if (live_i) A.cost[i] = cost;
}

// any d: LDS tile [k][TJ] (TJ = 1 << tj_shift in {8, 16, 32, 64}), dynamic LDS d * TJ doubles
__global__ __launch_bounds__(256) void bbh_pam_cost_generic_kernel(const PamCostArgs A, int tj_shift) {
  extern __shared__ double s_xg[];
  int start, end, i0;
  if (!pam_cost_range(A, start, end, i0)) return;
  const int i = i0 + threadIdx.x;
  const bool live_i = i < end;
  double cost = 0.0;
  // (i0 < end: a valid address for the idle lanes)
  bbh_rows_pair_walk_generic(A.Ps, A.lds, A.d, A.Ps + (live_i ? i : i0), start, end, tj_shift, s_xg, PamCostLoad{end}, PamCostVisit{cost});
  if (live_i) A.cost[i] = cost;
}

// One workgroup per cluster.  flags[c]: 1 = empty, 2 = medoid changed, 0 = neither.
__global__ __launch_bounds__(256) void bbh_pam_update_kernel(const double* __restrict__ cost, const int64_t* __restrict__ perm, int64_t M,
                                                             const int64_t* __restrict__ starts, int64_t* __restrict__ medoids,
                                                             int* __restrict__ flags) {
  __shared__ bbh_rows_min_key s_key[4];
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
  bbh_rows_min_key best = {INFINITY, -1};  // the minimum and its grouped column; -1: none yet
  for (int64_t s = s0 + tid; s < s1; s += 256) {
    const double x = cost[s];
    if (best.p < 0 || x < best.v) best.v = x, best.p = s;  // ascending s, strict <: the smallest column of equal costs stays
    if (perm[s] == med) s_cur = s;                         // (positions are unique: at most one writer)
  }
  best = bbh_rows_block_best(best, s_key, bbh_rows_min_beats);
  if (tid == 0) {
    const double curr = cost[(s_cur >= 0) ? s_cur : s0];  // a medoid outside its own cluster: the first member's cost
    int f = 0;
    if (best.v < curr) {
      const int64_t m = perm[best.p];
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
  int rc = bbh_rows_check(h, "bbh_pam_dist_rows", P_dev, M, d, ldp);
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
  int rc = bbh_rows_check(h, "bbh_pam_assign", P_dev, M, d, ldp);
  if (rc) return rc;
  if (!medoids_dev || !labels_dev || !dist_dev || k < 1 || k > M) {
    h->err = "bbh_pam_assign: bad arguments (need the medoids, both outputs and 1 <= k <= M)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  const int tc_shift = bbh_rows_tile_shift(d);
  const size_t lds = sizeof(double) * (size_t)d * ((size_t)1 << tc_shift);  // <= 48 KB
  hipLaunchKernelGGL(bbh_pam_assign_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), lds, h->stream, P_dev, ldp, M, (int)d, medoids_dev, k,
                     tc_shift, labels_dev, dist_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

extern "C" int bbh_pam_cost(bbh_handle* h, const double* Ps_dev, int64_t M, int32_t d, int64_t lds, const int64_t* starts_dev,
                            const int64_t* tile_starts_dev, int64_t k, int32_t* table_dev, int64_t max_tiles, double* cost_dev) {
  if (!h) return -1;
  int rc = bbh_rows_check(h, "bbh_pam_cost", Ps_dev, M, d, lds);
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
  bbh_rows_dispatch_dp(d, [&](auto dp) {
    constexpr int DP = decltype(dp)::value;
    if constexpr (DP > 0) {
      hipLaunchKernelGGL(bbh_pam_cost_kernel<DP>, dim3(grid), dim3(256), 0, h->stream, a);
    } else {
      const int tj_shift = bbh_rows_tile_shift(d);
      const size_t bytes = sizeof(double) * (size_t)d * ((size_t)1 << tj_shift);  // <= 48 KB
      hipLaunchKernelGGL(bbh_pam_cost_generic_kernel, dim3(grid), dim3(256), bytes, h->stream, a, tj_shift);
    }
  });
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

extern "C" int bbh_pam_update(bbh_handle* h, const double* cost_dev, const int64_t* perm_dev, int64_t M, const int64_t* starts_dev, int64_t k,
                              int64_t* medoids_dev, int32_t* flags_dev) {
  if (!h) return -1;
  if (!cost_dev || !perm_dev || !starts_dev || !medoids_dev || !flags_dev || M < 1 || M > BBH_ROWS_MAX || k < 1 || k > M) {
    h->err = "bbh_pam_update: bad arguments (need the costs, the permutation, the prefix array, the medoids, the flags, "
             "1 <= M < 2^31 - 256 and 1 <= k <= M)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(bbh_pam_update_kernel, dim3((unsigned)k), dim3(256), 0, h->stream, cost_dev, perm_dev, M, starts_dev, medoids_dev, flags_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}
