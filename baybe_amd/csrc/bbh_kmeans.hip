// k-means clustering (Lloyd, k-means++ seeding) over the device-resident candidate matrix, batched over the restarts.
//
// What the reference does here (KMeansClusteringRecommender, baybe/recommenders/pure/nonpredictive/clustering.py:196-252): hand the
// scaled candidates to sklearn.cluster.KMeans with {"max_iter": 1000, "n_init": 50} - fifty Lloyd runs on the host, one after the
// other - then build an [N, k] distance matrix on the host and take the member nearest to each centre.  Here the restarts are ONE
// workload: a pass scores every still-running restart, and a point is read once per RESTART TILE (as many restarts' centres as
// fit in LDS), not once per restart.
//
//   bbh_kmeans_seed_update_kernel  closest[r][j] = d2(x_j, x_centre(r))  (or the minimum with what it held), and the 256-position
//                                  tile sums of closest.
//   bbh_kmeans_seed_search_kernel  one workgroup per restart: pot = the tile sums added in ascending tile order, the T values
//                                  u * pot searched in the running sum (tiles first, then the positions of one tile), clipped.
//   bbh_kmeans_seed_trial_kernel   the T trial potentials: tile sums of min(closest, d2(., x_cand_t)).
//   bbh_kmeans_seed_pick_kernel    one workgroup per restart: the trial potentials (tiles ascending), the smallest, first on ties.
//   bbh_kmeans_pass_kernel         one Lloyd pass of one restart tile over one 256-position tile: the centres of the tile's restarts
//                                  in LDS as [dim][centre] (streamed through LDS in chunks where one restart's centres do not
//                                  fit: the one-restart form), eight centres' chains in flight per point, the label = the smallest
//                                  cluster index among equal minima; then every (restart, cluster, dimension) accumulator is owned
//                                  by ONE thread that adds the tile's members in ascending position.  Per tile and restart it
//                                  leaves the member sums and counts, the sum of d2 and whether a label changed.
//   bbh_kmeans_finish_kernel       one workgroup per restart: the tile partials added in ascending tile order, the division by the
//                                  counts, shift = sum |new - old|^2, inertia, and the flags (labels unchanged / empty cluster met).
//   bbh_kmeans_select_kernel       one workgroup per cluster: the member with the smallest sqrt(d2), first on ties; position 0 for a
//                                  cluster without members.
//
// Arithmetic: the contract of bbh_rows.h (the chains, the wave sums and the key reduction come from there).  Beyond its shapes a
// sum here is one owner's in ascending position inside a tile and ascending across tiles, so two runs give the same bits.  No entry
// point keeps state: all buffers are the caller's, all launches asynchronous on the handle's stream.
#include "bbh_rows.h"

#define KM_TP BBH_ROWS_TILE        // positions per tile (one per thread)
#define KM_XS 257                  // row stride of the LDS tiles [..][256]: one past the tile, so that rows fall on different banks
#define KM_LDS_BUDGET ((size_t)64 * 1024)  // per workgroup: two workgroups share a CU's 160 KB
#define KM_X_LDS_MAX_D 16          // the tile's own coordinates are staged in LDS up to this width (33 KB), read from L1/L2 beyond
#define KM_MAX_TRIALS 32           // T = 2 + int(log k) <= 23 for k < 2^31
#define KM_MAX_SLOTS 48            // restarts per tile at the most
#define KM_SLOT_BYTES ((size_t)KM_XS * 4 + 4 * 8 + 4 * 4)  // labels of the tile, four wave partials of the inertia and of "changed"

namespace {

struct KmPlan {
  int rt;        // restarts per tile
  int tq;        // centres per LDS chunk (a multiple of 8)
  int x_lds;     // the tile's coordinates staged in LDS
  int chunks;    // > 1: the one-restart form, its centres streamed through LDS
  size_t lds;
};

KmPlan km_plan(const bbh_handle* h, int d, int64_t k, int64_t R) {
  KmPlan p;
  const size_t budget = (h->lds_per_block < KM_LDS_BUDGET) ? h->lds_per_block : KM_LDS_BUDGET;
  p.x_lds = d <= KM_X_LDS_MAX_D;
  const size_t xb = p.x_lds ? sizeof(double) * (size_t)d * KM_XS : 0;
  auto bytes = [&](int64_t rt, int64_t tq) { return xb + sizeof(double) * (size_t)d * (size_t)tq + KM_SLOT_BYTES * (size_t)rt; };
  int64_t rt = 0;
  const int64_t cap = (R < KM_MAX_SLOTS) ? R : KM_MAX_SLOTS;
  if (k <= (int64_t)(budget / 8)) {
    while (rt < cap && bytes(rt + 1, bbh_round_up((rt + 1) * k, 8)) <= budget) rt++;
  }
  if (rt >= 1) {
    p.rt = (int)rt, p.tq = (int)bbh_round_up(rt * k, 8), p.chunks = 1;
  } else {  // one restart at a time, its centres through LDS in chunks of tq (d * 64 bytes * 8 <= 48 KB: at least one group of 8)
    int64_t tq = (int64_t)((budget - xb - KM_SLOT_BYTES) / (sizeof(double) * (size_t)d)) / 8 * 8;
    if (tq > bbh_round_up(k, 8)) tq = bbh_round_up(k, 8);
    p.rt = 1, p.tq = (int)tq, p.chunks = (int)((k + tq - 1) / tq);
  }
  p.lds = bytes(p.rt, p.tq);
  return p;
}

__device__ __forceinline__ int64_t km_clamp_row(int64_t i, int64_t M) { return (i < 0) ? 0 : (i >= M) ? M - 1 : i; }

}  // namespace

// ---- k-means++ seeding, all restarts at once -----------------------------------------------------------------------------------------
// grid (tiles, R).  centre of restart r: idx[r * k + c].
__global__ __launch_bounds__(256) void bbh_kmeans_seed_update_kernel(const double* __restrict__ P, int64_t ldp, int64_t M, int d,
                                                                     const int64_t* __restrict__ idx, int64_t k, int64_t c, int first,
                                                                     double* __restrict__ closest, double* __restrict__ tilesum,
                                                                     int64_t ntiles) {
  __shared__ double s_w[4];
  const int tid = threadIdx.x;
  const int64_t r = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * KM_TP + tid;
  const int64_t i = km_clamp_row(idx[r * k + c], M);
  double v = 0.0;
  if (j < M) {
    v = bbh_rows_d2(P, ldp, d, j, i);
    if (!first) {
      const double old = closest[r * M + j];
      v = (old < v) ? old : v;
    }
    closest[r * M + j] = v;
  }
  v = bbh_rows_block4_sum(v, s_w);
  if (tid == 0) tilesum[r * ntiles + blockIdx.x] = v;
}

// grid (R), 64 threads; thread t < T searches u[r][(c - 1) T + t] * pot: the first position whose running sum reaches it
__global__ __launch_bounds__(64) void bbh_kmeans_seed_search_kernel(const double* __restrict__ closest, const double* __restrict__ tilesum,
                                                                    int64_t M, int64_t ntiles, const double* __restrict__ U, int64_t ldu,
                                                                    int64_t c, int T, int64_t* __restrict__ cand) {
  const int t = threadIdx.x;
  const int64_t r = blockIdx.x;
  if (t >= T) return;
  const double* ts = tilesum + r * ntiles;
  double pot = 0.0;
  for (int64_t b = 0; b < ntiles; b++) pot = pot + ts[b];
  const double rv = U[r * ldu + (c - 1) * T + t] * pot;
  double cum = 0.0;
  int64_t b = 0;
  for (; b < ntiles; b++) {
    const double nxt = cum + ts[b];
    if (nxt >= rv) break;
    cum = nxt;
  }
  int64_t found = M - 1;  // beyond the last running sum: clipped
  if (b < ntiles) {
    const int64_t j0 = b * KM_TP;
    const int64_t j1 = (j0 + KM_TP < M) ? j0 + KM_TP : M;
    found = j1 - 1;  // (the tile's own sum reached rv; should the sequential one fall an ulp short, its last position)
    const double* cl = closest + r * M;
    for (int64_t j = j0; j < j1; j++) {
      cum = cum + cl[j];
      if (cum >= rv) {
        found = j;
        break;
      }
    }
  }
  cand[r * T + t] = found;
}

// grid (tiles, R): trialpart[(r T + t) ntiles + tile] = the tile's sum of min(closest, d2(., x_cand[r][t]))
__global__ __launch_bounds__(256) void bbh_kmeans_seed_trial_kernel(const double* __restrict__ P, int64_t ldp, int64_t M, int d,
                                                                    const double* __restrict__ closest, const int64_t* __restrict__ cand,
                                                                    int T, double* __restrict__ trialpart, int64_t ntiles) {
  __shared__ double s_w[KM_MAX_TRIALS][4];
  const int tid = threadIdx.x;
  const int64_t r = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * KM_TP + tid;
  const double cl = (j < M) ? closest[r * M + j] : 0.0;
  for (int t = 0; t < T; t++) {
    double v = 0.0;
    if (j < M) {
      v = bbh_rows_d2(P, ldp, d, j, km_clamp_row(cand[r * T + t], M));
      v = (cl < v) ? cl : v;
    }
    v = bbh_rows_wave_sum(v);
    if ((tid & 63) == 0) s_w[t][tid >> 6] = v;
  }
  __syncthreads();
  if (tid < T) trialpart[(r * T + tid) * ntiles + blockIdx.x] = bbh_rows_sum4(s_w[tid]);
}

// grid (R), 64 threads: idx[r k + c] = the candidate with the smallest trial potential, first on ties
__global__ __launch_bounds__(64) void bbh_kmeans_seed_pick_kernel(const double* __restrict__ trialpart, int64_t ntiles, const int64_t* __restrict__ cand,
                                                                  int T, int64_t k, int64_t c, int64_t* __restrict__ idx) {
  __shared__ double s_pot[KM_MAX_TRIALS];
  const int t = threadIdx.x;
  const int64_t r = blockIdx.x;
  if (t < T) {
    const double* tp = trialpart + (r * T + t) * ntiles;
    double pot = 0.0;
    for (int64_t b = 0; b < ntiles; b++) pot = pot + tp[b];
    s_pot[t] = pot;
  }
  __syncthreads();
  if (t == 0) {
    int best = 0;
    for (int u = 1; u < T; u++)
      if (s_pot[u] < s_pot[best]) best = u;
    idx[r * k + c] = cand[r * T + best];
  }
}

// ---- the Lloyd pass --------------------------------------------------------------------------------------------------------------------
struct KmPassArgs {
  const double* P;  // [d][ldp]
  int64_t ldp, M;
  int d;
  const double* C;  // [R][k][d]
  const int* rid;   // [n_slots]: the restarts of this launch
  int n_slots;
  int64_t k;
  int tq, x_lds, want_sums;
  int* labels;         // [R][M], read (the previous labels) and written
  double* d2;          // [R][M]
  double* part_sum;    // [tiles][n_slots][k][d]
  int* part_cnt;       // [tiles][n_slots][k]
  double* part_inert;  // [tiles][n_slots]
  int* part_chg;       // [tiles][n_slots]
};

// dynamic LDS: [d][KM_XS] coordinates of the tile (x_lds), [d][tq] centres, then per slot KM_XS labels, 4 doubles, 4 ints
__global__ __launch_bounds__(256) void bbh_kmeans_pass_kernel(const KmPassArgs A) {
  extern __shared__ double s_km[];
  const int tid = threadIdx.x, d = A.d, tq = A.tq, ns = A.n_slots;
  const int64_t j0 = (int64_t)blockIdx.x * KM_TP;
  const int64_t j = j0 + tid;
  const bool live = j < A.M;
  double* s_x = s_km;
  double* s_c = s_km + (A.x_lds ? (size_t)d * KM_XS : 0);
  double* s_inert = s_c + (size_t)d * tq;            // [ns][4]
  int* s_lab = (int*)(s_inert + (size_t)ns * 4);     // [ns][KM_XS]
  int* s_chg = s_lab + (size_t)ns * KM_XS;           // [ns][4]
  const double* Pj = A.P + (live ? j : 0);  // (a valid address for the idle lanes)
  if (A.x_lds)
    for (int dim = 0; dim < d; dim++) s_x[dim * KM_XS + tid] = live ? Pj[(int64_t)dim * A.ldp] : 0.0;
  const int64_t Q = (int64_t)ns * A.k;  // the centres of this launch, restart after restart
  int slot = 0;
  int64_t c = 0;
  double best = INFINITY;
  int lab = 0;
  for (int64_t q0 = 0; q0 < Q; q0 += tq) {
    __syncthreads();
    const int64_t left = Q - q0;
    const int nq = (left < tq) ? (int)left : tq;
    for (int e = tid; e < nq * d; e += 256) {  // (consecutive threads read consecutive doubles of a centre)
      const int u = e / d, dim = e - u * d;
      const int64_t q = q0 + u;
      const int64_t s = q / A.k;
      s_c[dim * tq + u] = A.C[((int64_t)A.rid[s] * A.k + (q - s * A.k)) * d + dim];
    }
    for (int e = tid; e < (tq - nq) * d; e += 256) {  // the rest of the last group of eight: never compared
      const int u = nq + e / d, dim = e % d;
      s_c[dim * tq + u] = 0.0;
    }
    __syncthreads();
    for (int qq = 0; qq < nq; qq += 8) {
      double acc[8];
      if (A.x_lds) bbh_rows_d2x8(s_x + tid, KM_XS, s_c + qq, tq, d, acc);
      else bbh_rows_d2x8(Pj, A.ldp, s_c + qq, tq, d, acc);
#pragma unroll
      for (int u = 0; u < 8; u++) {
        if (qq + u < nq) {  // (uniform: every thread walks the same centres)
          if (acc[u] < best) best = acc[u], lab = (int)c;  // ascending cluster index, strict <: the smallest index of equal minima
          c++;
          if (c == A.k) {  // the restart's last centre: its label is final
            int changed = 0;
            double v = 0.0;
            if (live) {
              const int64_t o = (int64_t)A.rid[slot] * A.M + j;
              changed = A.labels[o] != lab;
              A.labels[o] = lab;
              A.d2[o] = best;
              v = best;
            }
            s_lab[slot * KM_XS + tid] = live ? lab : -1;
            v = bbh_rows_wave_sum(v);
            const int any = __any(changed);
            if ((tid & 63) == 0) s_inert[slot * 4 + (tid >> 6)] = v, s_chg[slot * 4 + (tid >> 6)] = any;
            slot++, c = 0, best = INFINITY, lab = 0;
          }
        }
      }
    }
  }
  __syncthreads();
  const int64_t tile = blockIdx.x;
  if (tid < ns) {
    const int* g = s_chg + tid * 4;
    A.part_inert[tile * ns + tid] = bbh_rows_sum4(s_inert + tid * 4);
    A.part_chg[tile * ns + tid] = g[0] | g[1] | g[2] | g[3];
  }
  if (!A.want_sums) return;
  const int64_t rest = A.M - j0;
  const int np = (rest < KM_TP) ? (int)rest : KM_TP;
  const int64_t KD = A.k * d, total = (int64_t)ns * KD;
  for (int64_t t = tid; t < total; t += 256) {  // one owner per (restart, cluster, dimension): the members in ascending position
    const int64_t s = t / KD, rem = t - s * KD;
    const int cc = (int)(rem / d), dim = (int)(rem - (int64_t)cc * d);
    const int* lb = s_lab + s * KM_XS;
    double acc = 0.0;
    int cnt = 0;
    if (A.x_lds) {
      const double* xs = s_x + dim * KM_XS;
      for (int p = 0; p < np; p++)
        if (lb[p] == cc) acc = acc + xs[p], cnt++;
    } else {
      const double* xg = A.P + (int64_t)dim * A.ldp + j0;
      for (int p = 0; p < np; p++)
        if (lb[p] == cc) acc = acc + xg[p], cnt++;
    }
    A.part_sum[tile * total + t] = acc;
    if (dim == 0) A.part_cnt[(tile * ns + s) * A.k + cc] = cnt;
  }
}

struct KmFinishArgs {
  const double* part_sum;
  const int* part_cnt;
  const double* part_inert;
  const int* part_chg;
  int64_t ntiles, k;
  int n_slots, d, want_sums;
  const int* rid;
  const double* C;  // [R][k][d]: the centres the pass used
  double* Cnew;     // [R][k][d]
  double* sums;     // [R][k][d]
  int* counts;      // [R][k]
  double* shift;    // [R]
  double* inertia;  // [R]
  int* flags;       // [R]: bit 0 = no label changed, bit 1 = an empty cluster was met
};

namespace {
// s[0..255] added as a fixed tree
__device__ __forceinline__ double km_block_sum(double v, double* s) {
  const int tid = threadIdx.x;
  __syncthreads();
  s[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s[tid] = s[tid] + s[tid + o];
    __syncthreads();
  }
  return s[0];
}
}  // namespace

// grid (n_slots): tile partials in ascending tile order (a thread's share of the tiles first where only scalars are added)
__global__ __launch_bounds__(256) void bbh_kmeans_finish_kernel(const KmFinishArgs A) {
  __shared__ double s_red[256];
  const int tid = threadIdx.x, ns = A.n_slots, d = A.d;
  const int64_t s = blockIdx.x;
  const int64_t r = A.rid[s];
  double in = 0.0;
  int chg = 0;
  for (int64_t b = tid; b < A.ntiles; b += 256) in = in + A.part_inert[b * ns + s], chg |= A.part_chg[b * ns + s];
  in = km_block_sum(in, s_red);
  chg = __syncthreads_or(chg);
  int empty = 0;
  double sh = 0.0;
  if (A.want_sums) {
    const int64_t KD = A.k * d, total = (int64_t)ns * KD;
    for (int64_t t = tid; t < KD; t += 256) {
      const int64_t cc = t / d;
      double acc = 0.0;
      int64_t cnt = 0;
      for (int64_t b = 0; b < A.ntiles; b++) {
        acc = acc + A.part_sum[b * total + s * KD + t];
        cnt += A.part_cnt[(b * ns + s) * A.k + cc];
      }
      A.sums[r * KD + t] = acc;
      if (t - cc * d == 0) A.counts[r * A.k + cc] = (int)cnt;
      if (cnt == 0) empty = 1;
      const double now = (cnt > 0) ? acc / (double)cnt : acc;
      const double diff = now - A.C[r * KD + t];
      A.Cnew[r * KD + t] = now;
      sh = sh + diff * diff;
    }
    sh = km_block_sum(sh, s_red);
    empty = __syncthreads_or(empty);
  }
  if (tid == 0) {
    A.inertia[r] = in;
    A.shift[r] = sh;
    A.flags[r] = (chg ? 0 : 1) | (empty ? 2 : 0);
  }
}

// grid (k): out[c] = the member of cluster c with the smallest sqrt(d2), the smallest position among equal ones; 0 without members
__global__ __launch_bounds__(256) void bbh_kmeans_select_kernel(const int* __restrict__ labels, const double* __restrict__ d2, int64_t M,
                                                                int64_t* __restrict__ out) {
  __shared__ bbh_rows_min_key s_key[4];
  const int c = blockIdx.x;
  bbh_rows_min_key best = {INFINITY, -1};
  for (int64_t j = threadIdx.x; j < M; j += 256) {
    if (labels[j] != c) continue;
    const double x = __dsqrt_rn(d2[j]);
    if (best.p < 0 || x < best.v) best.v = x, best.p = j;
  }
  best = bbh_rows_block_best(best, s_key, bbh_rows_min_beats);
  if (threadIdx.x == 0) out[c] = (best.p < 0) ? 0 : best.p;  // argmin of an all-infinite column
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
extern "C" int bbh_kmeans_plan(bbh_handle* h, int32_t d, int64_t k, int64_t R, int32_t* restarts_per_tile, int32_t* chunks) {
  if (!h) return -1;
  if (d < 1 || d > BBH_ROWS_MAX_D || k < 1 || k > BBH_ROWS_MAX || R < 1 || !restarts_per_tile || !chunks) {
    h->err = "bbh_kmeans_plan: bad arguments (need 1 <= d <= 768, 1 <= k < 2^31 - 256, R >= 1 and both outputs)";
    return -1;
  }
  const KmPlan p = km_plan(h, d, k, R);
  *restarts_per_tile = p.rt, *chunks = p.chunks;
  return 0;
}

extern "C" int bbh_kmeans_seed(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, int64_t* idx_dev, const double* U_dev,
                               int64_t R, int64_t k, int32_t T, double* closest_dev, double* tilesum_dev, double* trialpart_dev,
                               int64_t* cand_dev) {
  if (!h) return -1;
  int rc = bbh_rows_check(h, "bbh_kmeans_seed", P_dev, M, d, ldp);
  if (rc) return rc;
  if (!idx_dev || !closest_dev || !tilesum_dev || k < 1 || k > M || R < 1 || R > 65535 || T < 1 || T > KM_MAX_TRIALS ||
      (k > 1 && (!U_dev || !trialpart_dev || !cand_dev))) {
    h->err = "bbh_kmeans_seed: bad arguments (need the indices, the uniforms, the work arrays, 1 <= k <= M, 1 <= R <= 65535 and "
             "1 <= T <= 32)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  const int64_t ntiles = (M + KM_TP - 1) / KM_TP;
  const dim3 grid((unsigned)ntiles, (unsigned)R);
  const int64_t ldu = (k - 1) * T;
  for (int64_t c = 0; c < k; c++) {
    if (c > 0) {
      hipLaunchKernelGGL(bbh_kmeans_seed_search_kernel, dim3((unsigned)R), dim3(64), 0, h->stream, closest_dev, tilesum_dev, M, ntiles, U_dev, ldu,
                         c, (int)T, cand_dev);
      hipLaunchKernelGGL(bbh_kmeans_seed_trial_kernel, grid, dim3(256), 0, h->stream, P_dev, ldp, M, (int)d, closest_dev, cand_dev, (int)T,
                         trialpart_dev, ntiles);
      hipLaunchKernelGGL(bbh_kmeans_seed_pick_kernel, dim3((unsigned)R), dim3(64), 0, h->stream, trialpart_dev, ntiles, cand_dev, (int)T, k, c,
                         idx_dev);
    }
    if (c + 1 < k)
      hipLaunchKernelGGL(bbh_kmeans_seed_update_kernel, grid, dim3(256), 0, h->stream, P_dev, ldp, M, (int)d, idx_dev, k, c, (int)(c == 0),
                         closest_dev, tilesum_dev, ntiles);
    BBH_HIP_TRY(h, hipGetLastError());
  }
  return 0;
}

extern "C" int bbh_kmeans_pass(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, const double* C_dev, const int32_t* rid_dev,
                               int64_t n_active, int64_t k, int32_t want_sums, int32_t* labels_dev, double* d2_dev, double* work_f64_dev,
                               int64_t work_f64_len, int32_t* work_i32_dev, int64_t work_i32_len, double* Cnew_dev, double* sums_dev,
                               int32_t* counts_dev, double* shift_dev, double* inertia_dev, int32_t* flags_dev) {
  if (!h) return -1;
  int rc = bbh_rows_check(h, "bbh_kmeans_pass", P_dev, M, d, ldp);
  if (rc) return rc;
  if (!C_dev || !rid_dev || !labels_dev || !d2_dev || !work_f64_dev || !work_i32_dev || !shift_dev || !inertia_dev || !flags_dev ||
      (want_sums && (!Cnew_dev || !sums_dev || !counts_dev)) || k < 1 || k > M || n_active < 1 || n_active > 65535) {
    h->err = "bbh_kmeans_pass: bad arguments (need the centres, the restart list, the outputs, both work arrays, 1 <= k <= M and "
             "1 <= restarts <= 65535)";
    return -1;
  }
  const KmPlan p = km_plan(h, d, k, n_active);
  const int64_t ntiles = (M + KM_TP - 1) / KM_TP;
  const int64_t need_f64 = ntiles * p.rt * ((want_sums ? k * d : 0) + 1), need_i32 = ntiles * p.rt * ((want_sums ? k : 0) + 1);
  if (work_f64_len < need_f64 || work_i32_len < need_i32) {
    h->err = "bbh_kmeans_pass: bad arguments (the work arrays need tiles * restarts_per_tile * (k * d + 1) doubles and "
             "tiles * restarts_per_tile * (k + 1) ints)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  BBH_HIP_TRY(h, bbh_allow_lds(h->device, (const void*)bbh_kmeans_pass_kernel, p.lds));
  for (int64_t r0 = 0; r0 < n_active; r0 += p.rt) {
    const int ns = (int)((n_active - r0 < p.rt) ? n_active - r0 : p.rt);
    KmPassArgs a;
    a.P = P_dev, a.ldp = ldp, a.M = M, a.d = (int)d, a.C = C_dev, a.rid = rid_dev + r0, a.n_slots = ns, a.k = k;
    a.tq = p.tq, a.x_lds = p.x_lds, a.want_sums = want_sums, a.labels = labels_dev, a.d2 = d2_dev;
    a.part_inert = work_f64_dev, a.part_sum = work_f64_dev + ntiles * p.rt;
    a.part_chg = work_i32_dev, a.part_cnt = work_i32_dev + ntiles * p.rt;
    hipLaunchKernelGGL(bbh_kmeans_pass_kernel, dim3((unsigned)ntiles), dim3(256), p.lds, h->stream, a);
    BBH_HIP_TRY(h, hipGetLastError());
    KmFinishArgs f;
    f.part_sum = a.part_sum, f.part_cnt = a.part_cnt, f.part_inert = a.part_inert, f.part_chg = a.part_chg, f.ntiles = ntiles, f.k = k;
    f.n_slots = ns, f.d = (int)d, f.want_sums = want_sums, f.rid = a.rid, f.C = C_dev, f.Cnew = Cnew_dev, f.sums = sums_dev;
    f.counts = counts_dev, f.shift = shift_dev, f.inertia = inertia_dev, f.flags = flags_dev;
    hipLaunchKernelGGL(bbh_kmeans_finish_kernel, dim3((unsigned)ns), dim3(256), 0, h->stream, f);
    BBH_HIP_TRY(h, hipGetLastError());
  }
  return 0;
}

extern "C" int bbh_kmeans_select(bbh_handle* h, const int32_t* labels_dev, const double* d2_dev, int64_t M, int64_t k, int64_t* out_dev) {
  if (!h) return -1;
  if (!labels_dev || !d2_dev || !out_dev || M < 1 || M > BBH_ROWS_MAX || k < 1 || k > M) {
    h->err = "bbh_kmeans_select: bad arguments (need the labels, the squared distances, the output, 1 <= M < 2^31 - 256 and "
             "1 <= k <= M)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(bbh_kmeans_select_kernel, dim3((unsigned)k), dim3(256), 0, h->stream, labels_dev, d2_dev, M, out_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}
