// Farthest point sampling over the device-resident candidate matrix.
//
// What the reference does here (baybe/utils/sampling_algorithms.py:15-172, called by FPSRecommender._recommend_discrete,
// baybe/recommenders/pure/nonpredictive/sampling.py:146-177): standard-scale the candidates, sort them lexicographically, build the
// full N x N distance matrix on the host (sklearn.metrics.pairwise_distances: 80 GB at N = 1e5), start from the argmax of that
// matrix and add, pick by pick, the point with the largest minimum distance to the selection.  Here the matrix never exists:
//
//   bbh_fps_prepare_kernel       P[k][r] = (X[order[r]][k] - mean[k]) / scale[k]: the scaled points, transposed and in rank order
//                                (IEEE subtraction and division: the values equal numpy's bit for bit).
//   bbh_fps_pairs_kernel<DP>     the all-pairs maximum, d <= 32: one thread per row i with its DP >= d coordinates in registers
//                                (columns beyond d are zero: adding +0.0 changes no bit of a sum that starts at +0.0), tiles of 64
//                                rows j staged in LDS as [j][DP] and read at wave-uniform addresses, a running (d^2, j) per thread
//                                updated with a strict >, one (d^2, a, b) key per workgroup.  Grid: (segments of j, tiles of i);
//                                workgroups below the diagonal leave an empty key.
//   bbh_fps_pairs_generic_kernel the same for any d <= 768: eight accumulators per thread, x_i re-read from global memory per group
//                                of eight j, the j tile in LDS as [k][TJ].
//   bbh_fps_pairs_final_kernel   one workgroup reduces the keys.
//   bbh_fps_pass_kernel          one greedy pass: mind[r] = min(mind[r], d^2(r, c)) with c read from DEVICE memory (the previous
//                                pick), fused with the chunk keys (max, count of bit-equal rows) of the updated mind.
//   bbh_fps_pick_kernel          one workgroup: global maximum of the chunk keys, the count of bit-equal rows, and the k-th of them
//                                in rank order (k < 0: the last one).
//
// The deciding value is always d^2 by the arithmetic contract of bbh_rows.h (the generic pair walk, the chain between two columns
// and the key reduction come from there).  Tie rules, all in ranks: the farthest pair is the smallest a, then the smallest b, over a < b; a
// greedy pick is the k-th row in rank order among the bit-equal maxima.  Dead (masked) rows: NaN in the staged j tile (NaN > x is
// false) and mind = -inf.
#include <string.h>

#include "bbh_rows.h"

#define FPS_TI BBH_ROWS_TILE  // rows i per workgroup (one per thread)
#define FPS_MAX_SEGS 64       // segments of j per tile of i (bounds the key count: tiles x segments)

namespace {

struct fps_state {
  // all-pairs keys [tiles x segments]
  double* d_key_v = nullptr;
  int* d_key_a = nullptr;
  int* d_key_b = nullptr;
  size_t key_cap = 0;
  // greedy state of the selection in progress
  const double* P = nullptr;  // caller-owned [d][ldp]
  int64_t M = 0, ldp = 0;
  int d = 0;
  double* d_mind = nullptr;   // [M] minimum d^2 to the selection; -inf: dead or selected
  int64_t* d_sel = nullptr;   // [M] selected ranks in selection order
  size_t row_cap = 0;
  double* d_cmax = nullptr;   // chunk keys of mind
  int* d_ccnt = nullptr;
  size_t chunk_cap = 0;
  int64_t n_sel = 0;          // entries of d_sel in use
  int64_t pending = -1;       // entry of d_sel whose pass has not run yet
  bool active = false;
  // results: host-mapped [ranks cap | d2 cap], a device twin where mapping is not available
  void* h_res = nullptr;
  void* h_res_dev = nullptr;
  size_t res_cap = 0;         // picks the block holds
  bool res_mapped = false;
  // farthest pair / tie count: host-mapped [d2 | a | b | count]
  void* h_small = nullptr;
  void* h_small_dev = nullptr;
};

fps_state* fps_get(bbh_handle* h) {
  if (!h->fps_state) h->fps_state = new fps_state();
  return (fps_state*)h->fps_state;
}

// (d^2 descending, a ascending, b ascending): does x beat y?  b < 0 marks an empty key.
struct FpsPairKey {
  double v;
  int a, b;
  __device__ __forceinline__ FpsPairKey shfl_xor(int o) const { return {__shfl_xor(v, o, 64), __shfl_xor(a, o, 64), __shfl_xor(b, o, 64)}; }
};
__device__ __forceinline__ bool fps_pair_beats(const FpsPairKey& x, const FpsPairKey& y) {
  if (x.b < 0) return false;
  if (y.b < 0) return true;
  return x.v > y.v || (x.v == y.v && (x.a < y.a || (x.a == y.a && x.b < y.b)));
}

}  // namespace

// P[k][r], r < M: row order[r] of X (order null: row r), scaled.  sclofs: [mean d | scale d].
__global__ __launch_bounds__(256) void bbh_fps_prepare_kernel(const double* __restrict__ X, int64_t ldx, int d, const double* __restrict__ sclofs,
                                                              const int64_t* __restrict__ order, int64_t N, int64_t M, double* __restrict__ P,
                                                              int64_t ldp) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= ldp) return;
  int64_t src = -1;
  if (r < M) {
    src = order ? order[r] : r;
    if (src < 0 || src >= N) src = -1;  // (checked on the host side; never read out of bounds)
  }
  for (int k = 0; k < d; k++) {
    double v = 0.0;  // padding columns of P
    if (r < M) v = (src >= 0) ? (X[src * ldx + k] - sclofs[k]) / sclofs[d + k] : NAN;
    P[(int64_t)k * ldp + r] = v;
  }
}

struct FpsPairArgs {
  const double* P;
  int64_t ldp;
  int M, d, seg_rows;
  const uint8_t* alive;
  double* key_v;
  int* key_a;
  int* key_b;
};

namespace {

// a j beyond the segment or a dead j is staged as NaN: visited, and never a maximum
struct FpsPairLoad {
  static constexpr bool whole_tiles = true;
  const uint8_t* alive;
  int seg1;
  __device__ __forceinline__ bool live(int j) const { return j < seg1 && (!alive || alive[j]); }
  __device__ __forceinline__ double pad() const { return NAN; }
};

// The workgroup's share of the pairs: rows i of tile blockIdx.y against the rows j > i of segment blockIdx.x (multiples of 64 at
// both ends but the last).  false: the segment lies below the tile's diagonal, an empty key.
struct FpsPairRange {
  int i0, i, j_begin, seg1;
  bool live_i;
  __device__ __forceinline__ bool set(const FpsPairArgs& A) {
    i0 = blockIdx.y * FPS_TI, i = i0 + threadIdx.x;
    const int seg0 = blockIdx.x * A.seg_rows;
    seg1 = (A.M - seg0 < A.seg_rows) ? A.M : seg0 + A.seg_rows;  // (seg0 < M by the grid)
    j_begin = (seg0 > i0) ? seg0 : i0;
    live_i = i < A.M && (!A.alive || A.alive[i]);
    return seg1 > i0 + 1;  // some j of the segment lies above the smallest i (uniform)
  }
};

// the running maximum of a row: ascending j, strict >, so the smallest j of equal distances stays
struct FpsPairVisit {
  int i;
  double& best;
  int& bj;
  __device__ __forceinline__ void operator()(int j, double d2, bool) const {
    const bool take = (d2 > best) & (j > i);  // (two selects, no branch: the chains of a group stay in one block)
    best = take ? d2 : best, bj = take ? j : bj;
  }
};

// one key per workgroup
__device__ __forceinline__ void fps_pairs_store(const FpsPairArgs& A, FpsPairKey* s_key, double best, int i, int bj) {
  const FpsPairKey top = bbh_rows_block_best(FpsPairKey{best, i, bj}, s_key, fps_pair_beats);
  if (threadIdx.x == 0) {
    const int key = blockIdx.y * gridDim.x + blockIdx.x;
    A.key_v[key] = top.v;
    A.key_a[key] = top.a;
    A.key_b[key] = top.b;
  }
}

}  // namespace

// The register form keeps a walk of its own - the one of bbh_rows_pair_walk with whole tiles, NaN for a dead or padded j and a
// running maximum: written through the template the <12> instantiation takes 82 VGPRs instead of 80 (5 waves per SIMD instead of 6)
// and the loops come out in another instruction order.  The key index is computed BEFORE the walk for the same reason: computed
// after it, the same source compiles to 82 VGPRs as well.
template <int DP>
__global__ __launch_bounds__(256) void bbh_fps_pairs_kernel(const FpsPairArgs A) {
  __shared__ double s_x[BBH_ROWS_TJ * DP];  // [j][DP]
  __shared__ FpsPairKey s_key[4];
  constexpr int NPRE = (BBH_ROWS_TJ * DP + 255) / 256;
  const int tid = threadIdx.x;
  const int i0 = blockIdx.y * FPS_TI;
  const int i = i0 + tid;
  const int seg0 = blockIdx.x * A.seg_rows;
  const int seg1 = (A.M - seg0 < A.seg_rows) ? A.M : seg0 + A.seg_rows;  // (seg0 < M by the grid)
  const int key = blockIdx.y * gridDim.x + blockIdx.x;
  double best = -INFINITY;
  int bj = -1;
  if (seg1 > i0 + 1) {  // some j of the segment lies above the smallest i (uniform)
    const bool live_i = i < A.M && (!A.alive || A.alive[i]);
    double xi[DP];
#pragma unroll
    for (int k = 0; k < DP; k++) xi[k] = (k < A.d && live_i) ? A.P[(int64_t)k * A.ldp + i] : 0.0;
    int j0 = (seg0 > i0) ? seg0 : i0;  // multiples of 64
    double pre[NPRE];
    auto load = [&](int jt) {
#pragma unroll
      for (int u = 0; u < NPRE; u++) {
        const int e = tid + u * 256;
        const int k = e >> 6, j = jt + (e & 63);
        double v = 0.0;
        if (k < A.d) v = (j < seg1 && (!A.alive || A.alive[j])) ? A.P[(int64_t)k * A.ldp + j] : NAN;
        pre[u] = v;
      }
    };
    load(j0);
    for (; j0 < seg1; j0 += BBH_ROWS_TJ) {
      __syncthreads();
#pragma unroll
      for (int u = 0; u < NPRE; u++) {
        const int e = tid + u * 256;
        if (e < BBH_ROWS_TJ * DP) s_x[(e & 63) * DP + (e >> 6)] = pre[u];
      }
      __syncthreads();
      if (j0 + BBH_ROWS_TJ < seg1) load(j0 + BBH_ROWS_TJ);  // in flight during the tile's arithmetic
      for (int jj = 0; jj < BBH_ROWS_TJ; jj += 4) {
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
        const int j = j0 + jj;  // ascending j, strict >: the smallest j of equal distances stays
        if (a0 > best && j > i) best = a0, bj = j;
        if (a1 > best && j + 1 > i) best = a1, bj = j + 1;
        if (a2 > best && j + 2 > i) best = a2, bj = j + 2;
        if (a3 > best && j + 3 > i) best = a3, bj = j + 3;
      }
    }
    if (!live_i) bj = -1;
  }
  const FpsPairKey top = bbh_rows_block_best(FpsPairKey{best, i, bj}, s_key, fps_pair_beats);
  if (tid == 0) A.key_v[key] = top.v, A.key_a[key] = top.a, A.key_b[key] = top.b;
}

// any d: LDS tile [k][TJ] (TJ in {8, 16, 32, 64}: tj_shift), dynamic LDS d * TJ doubles
__global__ __launch_bounds__(256) void bbh_fps_pairs_generic_kernel(const FpsPairArgs A, int tj_shift) {
  extern __shared__ double s_xg[];
  __shared__ FpsPairKey s_key[4];
  FpsPairRange r;
  double best = -INFINITY;
  int bj = -1;
  if (r.set(A)) {
    const double* xi = A.P + (r.live_i ? r.i : r.i0);  // (i0 < M by the grid: a valid address for the idle lanes)
    bbh_rows_pair_walk_generic(A.P, A.ldp, A.d, xi, r.j_begin, r.seg1, tj_shift, s_xg, FpsPairLoad{A.alive, r.seg1}, FpsPairVisit{r.i, best, bj});
    if (!r.live_i) bj = -1;
  }
  fps_pairs_store(A, s_key, best, r.i, bj);
}

// out: [d2 | a | b] as three 8-byte words (a = b = -1: fewer than two live rows)
__global__ __launch_bounds__(256) void bbh_fps_pairs_final_kernel(const double* __restrict__ key_v, const int* __restrict__ key_a,
                                                                  const int* __restrict__ key_b, int64_t nkeys, double* __restrict__ out) {
  __shared__ FpsPairKey s_key[4];
  FpsPairKey best = {-INFINITY, -1, -1};
  for (int64_t e = threadIdx.x; e < nkeys; e += 256) {
    const FpsPairKey key = {key_v[e], key_a[e], key_b[e]};
    if (fps_pair_beats(key, best)) best = key;
  }
  best = bbh_rows_block_best(best, s_key, fps_pair_beats);
  if (threadIdx.x == 0) {
    out[0] = best.v;
    ((int64_t*)out)[1] = (best.b >= 0) ? best.a : -1;
    ((int64_t*)out)[2] = best.b;
  }
}

__global__ __launch_bounds__(256) void bbh_fps_init_kernel(const uint8_t* __restrict__ alive, int64_t M, double* __restrict__ mind) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < M) mind[r] = (!alive || alive[r]) ? INFINITY : -INFINITY;
}

// One pass for the selected point c = *csel: mind[r] = min(mind[r], d^2(r, c)), mind[c] = -inf; chunk keys of the result.
__global__ __launch_bounds__(256) void bbh_fps_pass_kernel(const double* __restrict__ P, int64_t ldp, int64_t M, int d,
                                                           const int64_t* __restrict__ csel, double* __restrict__ mind,
                                                           double* __restrict__ cmax, int* __restrict__ ccnt) {
  __shared__ double s_v[4];
  __shared__ int s_c[4];
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t c = *csel;
  const bool have_c = c >= 0 && c < M;  // (a pick that found no row left writes -1: nothing changes then)
  double v = -INFINITY;
  if (r < M) {
    v = mind[r];
    if (have_c) {
      const double acc = bbh_rows_d2(P, ldp, d, r, c);
      v = (r == c) ? -INFINITY : ((acc < v) ? acc : v);
      mind[r] = v;
    }
  }
  // chunk key: maximum and how many rows hold it bit for bit
  double mv = v;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(mv, o, 64);
    mv = (ov > mv) ? ov : mv;
  }
  if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = mv;
  __syncthreads();
  mv = s_v[0];
  for (int w = 1; w < 4; w++) mv = (s_v[w] > mv) ? s_v[w] : mv;
  const bool hit = r < M && v == mv && mv > -INFINITY;
  const unsigned long long bal = __ballot(hit);
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) {
    cmax[blockIdx.x] = mv;
    ccnt[blockIdx.x] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
  }
}

// k-th (k < 0: last) row in rank order among the rows whose mind equals the global maximum.  count_only: only the tie count.
// Outputs: sel[0] (device: the next pass reads it), out_rank[0] / out_d2[0] (host-mapped or device), *out_cnt.
__global__ __launch_bounds__(256) void bbh_fps_pick_kernel(const double* __restrict__ mind, int64_t M, const double* __restrict__ cmax,
                                                           const int* __restrict__ ccnt, int nchunks, int64_t k, int count_only,
                                                           int64_t* __restrict__ sel, int64_t* __restrict__ out_rank,
                                                           double* __restrict__ out_d2, int64_t* __restrict__ out_cnt) {
  __shared__ double s_v[4];
  __shared__ long long s_cnt[256];
  __shared__ int s_flag[256];
  __shared__ long long s_krem;
  __shared__ int s_owner, s_chunk;
  const int tid = threadIdx.x;
  double mv = -INFINITY;
  for (int c = tid; c < nchunks; c += 256) {
    const double x = cmax[c];
    mv = (x > mv) ? x : mv;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(mv, o, 64);
    mv = (ov > mv) ? ov : mv;
  }
  if ((tid & 63) == 0) s_v[tid >> 6] = mv;
  __syncthreads();
  mv = s_v[0];
  for (int w = 1; w < 4; w++) mv = (s_v[w] > mv) ? s_v[w] : mv;
  // tie counts of contiguous chunk ranges, one range per thread (rank order = chunk order)
  const int per = (nchunks + 255) / 256;
  const int c_lo = tid * per, c_hi = (c_lo + per < nchunks) ? c_lo + per : nchunks;
  long long mine = 0;
  if (mv > -INFINITY)
    for (int c = c_lo; c < c_hi; c++)
      if (cmax[c] == mv) mine += ccnt[c];
  s_cnt[tid] = mine;
  __syncthreads();
  if (tid == 0) {
    long long total = 0;
    for (int t = 0; t < 256; t++) total += s_cnt[t];
    if (out_cnt) *out_cnt = total;
    long long kk = (k < 0 || k >= total) ? total - 1 : k;
    int owner = -1;
    for (int t = 0; t < 256 && kk >= 0; t++) {
      if (kk < s_cnt[t]) {
        owner = t;
        break;
      }
      kk -= s_cnt[t];
    }
    s_owner = (total > 0) ? owner : -1;
    s_krem = kk;
  }
  __syncthreads();
  if (count_only) return;
  const int owner = s_owner;
  if (owner < 0) {  // no row left
    if (tid == 0) {
      sel[0] = -1;
      out_rank[0] = -1;
      out_d2[0] = -INFINITY;
    }
    return;
  }
  if (tid == owner) {
    long long kk = s_krem;
    int chunk = -1;
    for (int c = c_lo; c < c_hi; c++) {
      if (cmax[c] != mv) continue;
      if (kk < ccnt[c]) {
        chunk = c;
        break;
      }
      kk -= ccnt[c];
    }
    s_chunk = chunk;
    s_krem = kk;
  }
  __syncthreads();
  const int chunk = s_chunk;
  const int64_t r = (int64_t)chunk * 256 + tid;
  s_flag[tid] = (chunk >= 0 && r < M && mind[r] == mv) ? 1 : 0;
  __syncthreads();
  if (tid == 0) {
    long long kk = s_krem;
    int64_t rank = -1;
    for (int t = 0; t < 256 && chunk >= 0; t++)
      if (s_flag[t]) {
        if (kk == 0) {
          rank = (int64_t)chunk * 256 + t;
          break;
        }
        kk--;
      }
    sel[0] = rank;
    out_rank[0] = rank;
    out_d2[0] = (rank >= 0) ? mv : -INFINITY;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
void bbh_fps_destroy(bbh_handle* h) {
  if (!h->fps_state) return;
  fps_state* st = (fps_state*)h->fps_state;
  if (st->d_key_v) hipFree(st->d_key_v);
  if (st->d_key_a) hipFree(st->d_key_a);
  if (st->d_key_b) hipFree(st->d_key_b);
  if (st->d_mind) hipFree(st->d_mind);
  if (st->d_sel) hipFree(st->d_sel);
  if (st->d_cmax) hipFree(st->d_cmax);
  if (st->d_ccnt) hipFree(st->d_ccnt);
  if (st->h_res) (st->res_mapped ? hipHostFree(st->h_res) : hipFree(st->h_res_dev));
  if (st->h_small) hipHostFree(st->h_small);
  delete st;
  h->fps_state = nullptr;
}

// The selection in progress refers to the caller's matrix: a handle that goes back to the pool forgets it (bbh_trim).
void bbh_fps_reset(bbh_handle* h) {
  if (!h->fps_state) return;
  fps_state* st = (fps_state*)h->fps_state;
  st->active = false;
  st->P = nullptr;
  st->pending = -1;
}

static int fps_small(bbh_handle* h, fps_state* st) {
  if (st->h_small) return 0;
  BBH_HIP_TRY(h, hipHostMalloc(&st->h_small, 64, hipHostMallocMapped));
  BBH_HIP_TRY(h, hipHostGetDevicePointer(&st->h_small_dev, st->h_small, 0));
  return 0;
}

// result block for `picks` picks: host-mapped where the device can write to host memory, a device buffer + copy otherwise
static int fps_results(bbh_handle* h, fps_state* st, size_t picks) {
  if (picks <= st->res_cap) return 0;
  if (st->h_res) (st->res_mapped ? hipHostFree(st->h_res) : hipFree(st->h_res_dev));
  st->h_res = st->h_res_dev = nullptr;
  st->res_cap = 0;
  const size_t cap = picks < 64 ? 64 : picks;
  if (hipHostMalloc(&st->h_res, cap * 16, hipHostMallocMapped) == hipSuccess &&
      hipHostGetDevicePointer(&st->h_res_dev, st->h_res, 0) == hipSuccess) {
    st->res_mapped = true;
  } else {
    (void)hipGetLastError();
    if (st->h_res) hipHostFree(st->h_res);
    st->res_mapped = false;
    BBH_HIP_TRY(h, hipMalloc(&st->h_res_dev, cap * 16));
    st->h_res = st->h_res_dev;  // (non-null marker; read through a copy)
  }
  st->res_cap = cap;
  return 0;
}

extern "C" int bbh_fps_prepare(bbh_handle* h, const double* X_dev, int64_t N, int32_t d, int64_t ldx, const double* mean_host,
                               const double* scale_host, const int64_t* order_dev, int64_t M, double* P_dev, int64_t ldp) {
  if (!h) return -1;
  if (!X_dev || !P_dev || !mean_host || !scale_host || N < 1 || d < 1 || ldx < d || M < 1 || ldp < M || (!order_dev && M > N)) {
    h->err = "bbh_fps_prepare: bad arguments (need N, M >= 1, d >= 1, ldx >= d, ldp >= M; without an order M <= N)";
    return -1;
  }
  for (int k = 0; k < d; k++)
    if (!(scale_host[k] > 0.0)) {
      h->err = "bbh_fps_prepare: scale must be positive";
      return -1;
    }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  std::vector<double> so((size_t)2 * d);
  memcpy(so.data(), mean_host, sizeof(double) * d);
  memcpy(so.data() + d, scale_host, sizeof(double) * d);
  int rc = bbh_upload_z(h, so.data(), so.size());
  if (rc) return rc;
  hipLaunchKernelGGL(bbh_fps_prepare_kernel, dim3((unsigned)((ldp + 255) / 256)), dim3(256), 0, h->stream, X_dev, ldx, (int)d, h->d_z, order_dev,
                     N, M, P_dev, ldp);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

extern "C" int bbh_fps_farthest_pair(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, const uint8_t* alive_dev,
                                     double* d2_host, int64_t* a_host, int64_t* b_host) {
  if (!h) return -1;
  int rc = bbh_rows_check(h, "bbh_fps_farthest_pair", P_dev, M, d, ldp);
  if (rc) return rc;
  if (!d2_host || !a_host || !b_host || M < 2) {
    h->err = "bbh_fps_farthest_pair: bad arguments (need M >= 2 and the three result pointers)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  fps_state* st = fps_get(h);
  if ((rc = fps_small(h, st))) return rc;
  const int64_t tiles = (M + FPS_TI - 1) / FPS_TI;
  const int64_t seg_tiles = (tiles + FPS_MAX_SEGS - 1) / FPS_MAX_SEGS;  // >= 1
  const int64_t seg_rows = seg_tiles * FPS_TI;
  const int64_t segs = (M + seg_rows - 1) / seg_rows;  // <= FPS_MAX_SEGS
  if (tiles > 65535) {
    h->err = "bbh_fps_farthest_pair: more than 65535 row tiles (M > 16.7e6)";
    return -1;
  }
  const size_t nkeys = (size_t)(tiles * segs);
  if (nkeys > st->key_cap) {
    if (st->d_key_v) hipFree(st->d_key_v);
    if (st->d_key_a) hipFree(st->d_key_a);
    if (st->d_key_b) hipFree(st->d_key_b);
    st->d_key_v = nullptr, st->d_key_a = st->d_key_b = nullptr, st->key_cap = 0;
    BBH_HIP_TRY(h, hipMalloc((void**)&st->d_key_v, sizeof(double) * nkeys));
    BBH_HIP_TRY(h, hipMalloc((void**)&st->d_key_a, sizeof(int) * nkeys));
    BBH_HIP_TRY(h, hipMalloc((void**)&st->d_key_b, sizeof(int) * nkeys));
    st->key_cap = nkeys;
  }
  FpsPairArgs a;
  a.P = P_dev, a.ldp = ldp, a.M = (int)M, a.d = (int)d, a.seg_rows = (int)seg_rows, a.alive = alive_dev;
  a.key_v = st->d_key_v, a.key_a = st->d_key_a, a.key_b = st->d_key_b;
  const dim3 grid((unsigned)segs, (unsigned)tiles);
  bbh_rows_dispatch_dp(d, [&](auto dp) {
    constexpr int DP = decltype(dp)::value;
    if constexpr (DP > 0) {
      hipLaunchKernelGGL(bbh_fps_pairs_kernel<DP>, grid, dim3(256), 0, h->stream, a);
    } else {
      const int tj_shift = bbh_rows_tile_shift(d);
      const size_t lds = sizeof(double) * (size_t)d * ((size_t)1 << tj_shift);  // <= 48 KB
      hipLaunchKernelGGL(bbh_fps_pairs_generic_kernel, grid, dim3(256), lds, h->stream, a, tj_shift);
    }
  });
  BBH_HIP_TRY(h, hipGetLastError());
  hipLaunchKernelGGL(bbh_fps_pairs_final_kernel, dim3(1), dim3(256), 0, h->stream, st->d_key_v, st->d_key_a, st->d_key_b, (int64_t)nkeys,
                     (double*)st->h_small_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  BBH_HIP_TRY(h, hipStreamSynchronize(h->stream));
  *d2_host = ((double*)st->h_small)[0];
  *a_host = ((int64_t*)st->h_small)[1];
  *b_host = ((int64_t*)st->h_small)[2];
  return 0;
}

static int fps_run_pending_pass(bbh_handle* h, fps_state* st) {
  if (st->pending < 0) return 0;
  const unsigned chunks = (unsigned)((st->M + 255) / 256);
  hipLaunchKernelGGL(bbh_fps_pass_kernel, dim3(chunks), dim3(256), 0, h->stream, st->P, st->ldp, st->M, st->d, st->d_sel + st->pending,
                     st->d_mind, st->d_cmax, st->d_ccnt);
  BBH_HIP_TRY(h, hipGetLastError());
  st->pending = -1;
  return 0;
}

extern "C" int bbh_fps_greedy(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, const uint8_t* alive_dev,
                              const int64_t* start_ranks_host, int64_t n_start, int64_t n_picks, int64_t k, int64_t* ranks_host,
                              double* d2_host, int64_t* count_host) {
  if (!h) return -1;
  if (n_start < 0 || n_picks < 0 || (n_picks > 0 && (!ranks_host || !d2_host)) || (k >= 0 && n_picks > 1)) {
    h->err = "bbh_fps_greedy: bad arguments (n_start, n_picks >= 0; result pointers with n_picks > 0; k >= 0 picks one row per call)";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  fps_state* st = fps_get(h);
  int rc = fps_small(h, st);
  if (rc) return rc;
  if (n_start > 0) {  // a new selection
    if ((rc = bbh_rows_check(h, "bbh_fps_greedy", P_dev, M, d, ldp, 0))) return rc;  // (the pass loops over any d)
    if (!start_ranks_host || n_start > M) {
      h->err = "bbh_fps_greedy: start ranks missing or more of them than rows";
      return -1;
    }
    for (int64_t s = 0; s < n_start; s++)
      if (start_ranks_host[s] < 0 || start_ranks_host[s] >= M) {
        h->err = "bbh_fps_greedy: start rank out of range";
        return -1;
      }
    st->active = false;
    if ((size_t)M > st->row_cap) {
      if (st->d_mind) hipFree(st->d_mind);
      if (st->d_sel) hipFree(st->d_sel);
      st->d_mind = nullptr, st->d_sel = nullptr, st->row_cap = 0;
      BBH_HIP_TRY(h, hipMalloc((void**)&st->d_mind, sizeof(double) * (size_t)M));
      BBH_HIP_TRY(h, hipMalloc((void**)&st->d_sel, sizeof(int64_t) * (size_t)M));
      st->row_cap = (size_t)M;
    }
    const size_t chunks = (size_t)((M + 255) / 256);
    if (chunks > st->chunk_cap) {
      if (st->d_cmax) hipFree(st->d_cmax);
      if (st->d_ccnt) hipFree(st->d_ccnt);
          st->d_cmax = nullptr, st->d_ccnt = nullptr, st->chunk_cap = 0;
      BBH_HIP_TRY(h, hipMalloc((void**)&st->d_cmax, sizeof(double) * chunks));
      BBH_HIP_TRY(h, hipMalloc((void**)&st->d_ccnt, sizeof(int) * chunks));
      st->chunk_cap = chunks;
    }
    st->P = P_dev, st->M = M, st->ldp = ldp, st->d = (int)d;
    hipLaunchKernelGGL(bbh_fps_init_kernel, dim3((unsigned)chunks), dim3(256), 0, h->stream, alive_dev, M, st->d_mind);
    BBH_HIP_TRY(h, hipGetLastError());
    void* stage = bbh_stage_pinned(h, sizeof(int64_t) * (size_t)n_start);
    if (!stage) {
      h->err = "bbh_fps_greedy: no pinned staging buffer";
      (void)hipGetLastError();
      return -2;
    }
    memcpy(stage, start_ranks_host, sizeof(int64_t) * (size_t)n_start);
    BBH_HIP_TRY(h, hipMemcpyAsync(st->d_sel, stage, sizeof(int64_t) * (size_t)n_start, hipMemcpyHostToDevice, h->stream));
    if ((rc = bbh_stage_done(h))) return rc;
    for (int64_t s = 0; s < n_start; s++) {
      st->pending = s;
      if ((rc = fps_run_pending_pass(h, st))) return rc;
    }
    st->n_sel = n_start;
    st->active = true;
  } else if (!st->active) {
    h->err = "bbh_fps_greedy: no selection in progress (pass start ranks first)";
    return -1;
  }
  if (st->n_sel + n_picks > st->M) {
    h->err = "bbh_fps_greedy: more picks requested than rows";
    return -1;
  }
  const int chunks = (int)((st->M + 255) / 256);
  if (n_picks > 0 && (rc = fps_results(h, st, (size_t)n_picks))) return rc;
  int64_t* res_rank = (int64_t*)st->h_res_dev;
  double* res_d2 = (double*)((char*)st->h_res_dev + st->res_cap * 8);
  for (int64_t p = 0; p < n_picks; p++) {
    if ((rc = fps_run_pending_pass(h, st))) return rc;
    hipLaunchKernelGGL(bbh_fps_pick_kernel, dim3(1), dim3(256), 0, h->stream, st->d_mind, st->M, st->d_cmax, st->d_ccnt, chunks, k, 0,
                       st->d_sel + st->n_sel, res_rank + p, res_d2 + p, (int64_t*)nullptr);
    BBH_HIP_TRY(h, hipGetLastError());
    st->pending = st->n_sel;
    st->n_sel += 1;
  }
  if (count_host) {  // tie count of the maximum the NEXT pick would take
    if ((rc = fps_run_pending_pass(h, st))) return rc;
    hipLaunchKernelGGL(bbh_fps_pick_kernel, dim3(1), dim3(256), 0, h->stream, st->d_mind, st->M, st->d_cmax, st->d_ccnt, chunks, (int64_t)-1, 1,
                       (int64_t*)nullptr, (int64_t*)nullptr, (double*)nullptr, (int64_t*)st->h_small_dev + 3);
    BBH_HIP_TRY(h, hipGetLastError());
  }
  if (n_picks > 0 && !st->res_mapped) {
    BBH_HIP_TRY(h, hipMemcpyAsync(ranks_host, res_rank, sizeof(int64_t) * (size_t)n_picks, hipMemcpyDeviceToHost, h->stream));
    BBH_HIP_TRY(h, hipMemcpyAsync(d2_host, res_d2, sizeof(double) * (size_t)n_picks, hipMemcpyDeviceToHost, h->stream));
  }
  if (n_picks > 0 || count_host) BBH_HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (n_picks > 0 && st->res_mapped) {
    memcpy(ranks_host, st->h_res, sizeof(int64_t) * (size_t)n_picks);
    memcpy(d2_host, (char*)st->h_res + st->res_cap * 8, sizeof(double) * (size_t)n_picks);
  }
  if (count_host) *count_host = ((int64_t*)st->h_small)[3];
  for (int64_t p = 0; p < n_picks; p++)
    if (ranks_host[p] < 0) {
      h->err = "bbh_fps_greedy: no unselected live row left";
      st->active = false;
      return -4;
    }
  return 0;
}
