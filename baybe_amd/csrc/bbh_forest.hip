// Random forest surrogate on the device: per-tree predictions, ensemble moments and the fused MC acquisition pass over a forest that
// scikit-learn fitted on the host (baybe/surrogates/random_forest.py: RandomForestRegressor(**model_params).fit, then one
// predictor.predict(candidates) per tree and an EnsemblePosterior over the [T, N] matrix).  Here candidates go in and scores come out;
// only bbh_forest_predict writes a [T, n] array, for small row sets.  Maths restated in tests/_oracle_forest.py.
//
// Traversal rule (what makes a prediction equal scikit-learn's bit for bit): the row is cast to float32, and a node sends it left iff
// (double)x32[feature] <= threshold; a leaf is a node whose left child is negative.  A tree is two arrays over its nodes: meta
// (int32 x 4: feature, left, right, unused; children relative to the tree's first node) and tv (fp64: the threshold of an inner node,
// the value of a leaf).
//
// One workgroup of 256 threads owns a tile of rows (256, 128 or 64 by the LDS the row copies need), one row per thread.  LDS holds the
// tile's float32 rows with an odd row stride (lanes reading one feature hit 64 different banks) - the feature index is data, a
// register array would live in scratch - and two node tables of FR_LDS_NODES nodes: tree o is walked out of table o & 1 while the
// nodes of tree o + 1 travel global -> registers, and go registers -> table (o + 1) & 1 after the walk; one barrier per tree.  A tree
// with more nodes than the budget is walked in global memory instead (same walk, other pointers).  Nodes are checked when they are
// staged (per step on the global path): a feature or child index out of range turns the node into a NaN leaf, and a walk ends after as
// many steps as the tree has nodes, so a table that is not a tree gives NaN and not a stray read or an endless loop.
//
// Order of arithmetic: a row's result is one chain over the trees in the order the caller lists them, owned by one thread; it does not
// depend on the tile or lane the row sits in, so equal rows get equal bits (forest scores are piecewise constant - ties are the normal
// case, and selection resolves them by first index).  No atomics.
#include <math.h>

#include "bbh_acqmath.h"

#define FR_THREADS 256
#define FR_LDS_NODES 1024                   // nodes per LDS table (a fully grown tree on 512 rows has at most 1023)
#define FR_PRE (FR_LDS_NODES / FR_THREADS)  // nodes a thread carries while the next tree is in flight
#define FR_MAX_PEND 63                      // pending points next to the candidate (the joint q'-batch limit of the GP path)
#define FR_PV 64                            // doubles per pending-term slot
#define FR_TAU_MAX 1e-2
#define FR_FIXED_LDS ((size_t)2 * FR_LDS_NODES * 8 + (size_t)3 * FR_PV * 8 + (size_t)2 * FR_LDS_NODES * 16)

struct FrArgs {
  const double* X;  // [N, ldx]
  int64_t N, ldx;
  int d, dpad, rows;
  int cshift;  // log2 of the threads that share a row while the tile is loaded (the power of two >= d, 256 at the most)
  const int4* meta;  // [n_nodes]
  const double* tv;  // [n_nodes]
  const int64_t* off;  // [T + 1]
  int64_t n_nodes;
  int T;
  const int32_t* order;  // [n_order]: the trees visited, in this order
  int n_order;
  int lds_nodes;  // trees with more nodes are walked in global memory
  const int32_t* counts;  // [T] (acquisition pass)
  const double* pend;     // [T, k]
  int k, kind;
  double S, best_f, sign, cu;
  const uint8_t* alive;
  double* out0;  // P [T, N] | mean [N] | scores [N]
  double* out1;  // var [N]
};

struct FrLds {
  double* tv;   // [2][FR_LDS_NODES]
  double* pv;   // [2][FR_PV]: the pending points' terms of a tree
  double* mp;   // [FR_PV]: the pending points' sample means (qUCB / qPSTD)
  int4* meta;   // [2][FR_LDS_NODES]
  float* rows;  // [rows][dpad]
};

__device__ __forceinline__ FrLds fr_carve(unsigned char* base) {
  FrLds L;
  L.tv = (double*)base;
  L.pv = L.tv + 2 * FR_LDS_NODES;
  L.mp = L.pv + 2 * FR_PV;
  L.meta = (int4*)(L.mp + FR_PV);
  L.rows = (float*)(L.meta + 2 * FR_LDS_NODES);
  return L;
}

__device__ __forceinline__ void fr_sanitize(int4& m, double& t, int nn, int d) {
  if (m.y >= 0 && ((unsigned)m.x >= (unsigned)d || (unsigned)m.y >= (unsigned)nn || (unsigned)m.z >= (unsigned)nn)) {
    m.y = -1;
    t = NAN;
  }
}

// first node and node count of tree t; 0 nodes (every walk gives NaN) for a tree or a range that does not exist
__device__ __forceinline__ int fr_tree(const FrArgs& a, int t, int64_t* base) {
  *base = 0;
  if ((unsigned)t >= (unsigned)a.T) return 0;
  const int64_t b = a.off[t], n = a.off[t + 1] - b;
  if (b < 0 || n < 1 || n > INT_MAX || b + n > a.n_nodes) return 0;
  *base = b;
  return (int)n;
}

template <bool CHECK>
__device__ __forceinline__ double fr_walk(const int4* meta, const double* tv, int nn, int d, const float* row) {
  int node = 0;
  for (int step = 0; step < nn; step++) {
    int4 m = meta[node];
    double t = tv[node];
    if (CHECK) fr_sanitize(m, t, nn, d);
    if (m.y < 0) return t;
    node = ((double)row[m.x] <= t) ? m.y : m.z;
  }
  return NAN;
}

// The tile's rows as float32: 2^cshift threads walk the columns of one row (consecutive addresses), the thread groups the rows - shifts
// and masks only, no division by d.
__device__ __forceinline__ void fr_load_rows(const FrArgs& a, const FrLds& L) {
  const int64_t row0 = (int64_t)blockIdx.x * a.rows;
  const int per_row = 1 << a.cshift;
  const int c0 = threadIdx.x & (per_row - 1);
  for (int r = threadIdx.x >> a.cshift; r < a.rows; r += FR_THREADS >> a.cshift) {
    const int64_t i = row0 + r;
    for (int f = c0; f < a.d; f += per_row) L.rows[r * a.dpad + f] = (i < a.N) ? (float)a.X[i * a.ldx + f] : 0.0f;
  }
}

// One pass over the listed trees.  stage(t, slot): the pending points' terms of tree t into L.pv[slot] (threads < k; may do nothing);
// use(t, slot, value): this thread's row in tree t (active threads only).  Ends behind a barrier.
template <class StageFn, class UseFn>
__device__ __forceinline__ void fr_sweep(const FrArgs& a, const FrLds& L, const float* row, bool active, StageFn stage, UseFn use) {
  const int tid = threadIdx.x;
  int64_t base;
  int t = a.order[0];
  int nn = fr_tree(a, t, &base);
  if (nn <= a.lds_nodes) {
    for (int idx = tid; idx < nn; idx += FR_THREADS) {
      int4 m = a.meta[base + idx];
      double v = a.tv[base + idx];
      fr_sanitize(m, v, nn, a.d);
      L.meta[idx] = m, L.tv[idx] = v;
    }
  }
  stage(t, 0);
  __syncthreads();
  for (int o = 0; o < a.n_order; o++) {
    const int buf = o & 1;
    int64_t base_n = 0;
    int t_n = -1, nn_n = 0;
    if (o + 1 < a.n_order) {
      t_n = a.order[o + 1];
      nn_n = fr_tree(a, t_n, &base_n);
    }
    const bool pre = t_n >= 0 && nn_n <= a.lds_nodes;
    int4 pm[FR_PRE];
    double pt[FR_PRE];
    if (pre) {
#pragma unroll
      for (int j = 0; j < FR_PRE; j++) {
        const int idx = tid + j * FR_THREADS;
        if (idx < nn_n) pm[j] = a.meta[base_n + idx], pt[j] = a.tv[base_n + idx];
      }
    }
    if (active && (unsigned)t < (unsigned)a.T) {  // (a listed tree that does not exist contributes nothing)
      const double v = (nn <= a.lds_nodes) ? fr_walk<false>(L.meta + buf * FR_LDS_NODES, L.tv + buf * FR_LDS_NODES, nn, a.d, row)
                                           : fr_walk<true>(a.meta + base, a.tv + base, nn, a.d, row);
      use(t, buf, v);
    }
    if (pre) {
#pragma unroll
      for (int j = 0; j < FR_PRE; j++) {
        const int idx = tid + j * FR_THREADS;
        if (idx < nn_n) {
          fr_sanitize(pm[j], pt[j], nn_n, a.d);
          L.meta[(buf ^ 1) * FR_LDS_NODES + idx] = pm[j], L.tv[(buf ^ 1) * FR_LDS_NODES + idx] = pt[j];
        }
      }
    }
    if (t_n >= 0) stage(t_n, buf ^ 1);
    __syncthreads();
    t = t_n, nn = nn_n, base = base_n;
  }
}

// ---- per-tree predictions P [T, N] -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FR_THREADS) void bbh_forest_predict_kernel(FrArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fr_smem[];
  const FrLds L = fr_carve(fr_smem);
  fr_load_rows(a, L);
  const int64_t i = (int64_t)blockIdx.x * a.rows + threadIdx.x;
  const bool active = (int)threadIdx.x < a.rows && i < a.N;
  const float* row = L.rows + (int)threadIdx.x * a.dpad;
  fr_sweep(a, L, row, active, [](int, int) {}, [&](int t, int, double v) { a.out0[(int64_t)t * a.N + i] = v; });
}

// ---- mean and unbiased variance over the trees: two passes (the mean, then the squared distances from it) ----------------------------
__global__ __launch_bounds__(FR_THREADS) void bbh_forest_moments_kernel(FrArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fr_smem[];
  const FrLds L = fr_carve(fr_smem);
  fr_load_rows(a, L);
  const int64_t i = (int64_t)blockIdx.x * a.rows + threadIdx.x;
  const bool active = (int)threadIdx.x < a.rows && i < a.N;
  const float* row = L.rows + (int)threadIdx.x * a.dpad;
  double sum = 0.0;
  fr_sweep(a, L, row, active, [](int, int) {}, [&](int, int, double v) { sum += v; });
  const double mean = sum / (double)a.n_order;
  double ss = 0.0;
  if (a.n_order > 1) {
    fr_sweep(a, L, row, active, [](int, int) {}, [&](int, int, double v) {
      const double dv = v - mean;
      ss += dv * dv;
    });
  }
  if (active) {
    a.out0[i] = mean;
    a.out1[i] = (a.n_order > 1) ? ss / (double)(a.n_order - 1) : 0.0;
  }
}

// ---- fused MC acquisition: sample s reads tree idx_s, so tree t stands for counts[t] of the S samples ----------------------------------
// LOG: qLogEI - li = log_fatplus(sign P_t - best_f) per point, the fat maximum over [candidate, pending ...], a streaming
// log-sum-exp over the trees weighted by their counts, - log S.  Otherwise bbh_mc_utility per point, the maximum over the points, the
// count-weighted mean; qUCB / qPSTD need every point's sample mean first (one more pass for the candidate's).
template <bool LOG>
__global__ __launch_bounds__(FR_THREADS) void bbh_forest_acq_kernel(FrArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fr_smem[];
  const FrLds L = fr_carve(fr_smem);
  const int tid = threadIdx.x;
  fr_load_rows(a, L);
  const int64_t i = (int64_t)blockIdx.x * a.rows + tid;
  const bool in_range = tid < a.rows && i < a.N;
  const bool active = in_range && (!a.alive || a.alive[i]);
  const float* row = L.rows + tid * a.dpad;
  const double inv_tau = 1.0 / TAU_RELU;
  const bool needs_mean = !LOG && (a.kind == BBH_ACQ_QUCB || a.kind == BBH_ACQ_QPSTD);
  double m_x = 0.0;
  if (needs_mean) {
    if (tid < a.k) {
      double s = 0.0;
      for (int o = 0; o < a.n_order; o++) {
        const int t = a.order[o];
        if ((unsigned)t < (unsigned)a.T) s += (double)a.counts[t] * (a.sign * a.pend[(int64_t)t * a.k + tid]);
      }
      L.mp[tid] = s / a.S;
    }
    double s = 0.0;
    fr_sweep(a, L, row, active, [](int, int) {}, [&](int t, int, double v) { s += (double)a.counts[t] * (a.sign * v); });
    m_x = s / a.S;  // (the sweep's barriers also publish L.mp)
  }
  auto stage = [&](int t, int slot) {
    if (tid < a.k && (unsigned)t < (unsigned)a.T) {
      const double obj = a.sign * a.pend[(int64_t)t * a.k + tid];
      double term;
      if constexpr (LOG)
        term = log(TAU_RELU) + log(bbh_fatplus_core((obj - a.best_f) * inv_tau));
      else
        term = bbh_mc_utility(a.kind, obj, needs_mean ? L.mp[tid] : 0.0, a.best_f, a.cu);
      L.pv[slot * FR_PV + tid] = term;
    }
  };
  double acc = 0.0, ref = -INFINITY;
  fr_sweep(a, L, row, active, stage, [&](int t, int slot, double v) {
    const double c = (double)a.counts[t];
    const double obj = a.sign * v;
    const double* pv = L.pv + slot * FR_PV;
    if constexpr (LOG) {
      const double li = log(TAU_RELU) + log(bbh_fatplus_core((obj - a.best_f) * inv_tau));
      double mx = li;
      for (int j = 0; j < a.k; j++) mx = fmax(mx, pv[j]);
      // fatmax over the q' points, the candidate first: mx + tau log sum_j (2 / (2 + (mx - li_j) / tau))^2
      double u = 2.0 / (2.0 + (mx - li) / FR_TAU_MAX);
      double fs = u * u;
      for (int j = 0; j < a.k; j++) {
        u = 2.0 / (2.0 + (mx - pv[j]) / FR_TAU_MAX);
        fs = fma(u, u, fs);
      }
      const double fm = mx + FR_TAU_MAX * log(fs);
      if (fm > ref) {
        acc = acc * exp(ref - fm) + c;
        ref = fm;
      } else {
        acc += c * exp(fm - ref);
      }
    } else {
      double best = bbh_mc_utility(a.kind, obj, m_x, a.best_f, a.cu);
      for (int j = 0; j < a.k; j++) best = fmax(best, pv[j]);
      acc += c * best;
    }
  });
  if (in_range) {
    double score = -INFINITY;
    if (active) score = LOG ? ref + log(acc) - log(a.S) : acc / a.S;
    a.out0[i] = score;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
extern "C" int bbh_forest_lds_nodes(void) { return FR_LDS_NODES; }

static int fr_setup(bbh_handle* h, const char* who, const double* X_dev, int64_t N, int32_t d, int64_t ldx, const int32_t* meta_dev,
                    const double* tv_dev, const int64_t* off_dev, int64_t T, int64_t n_nodes, const int32_t* order_dev, int64_t n_order,
                    int32_t lds_nodes, FrArgs* a, size_t* lds) {
  if (!X_dev || !meta_dev || !tv_dev || !off_dev || !order_dev || N < 1 || N > (int64_t)INT_MAX - FR_THREADS || d < 1 || ldx < d || T < 1 ||
      T > INT_MAX || n_nodes < T || n_order < 1 || n_order > INT_MAX || lds_nodes < 0) {
    h->err = std::string(who) + ": bad arguments (need the rows, the node tables, the tree list, 1 <= N < 2^31 - 256, 1 <= d <= ldx, "
                                "1 <= T <= nodes, at least one listed tree and lds_nodes >= 0)";
    return -1;
  }
  const int dpad = d | 1;
  int rows = 0;
  for (int r = FR_THREADS; r >= 64 && !rows; r /= 2)
    if (FR_FIXED_LDS + (size_t)r * dpad * 4 <= h->lds_per_block) rows = r;
  if (!rows) {
    h->err = std::string(who) + ": bad arguments (the float32 copies of 64 rows of d columns do not fit into LDS next to the node tables)";
    return -1;
  }
  *lds = FR_FIXED_LDS + (size_t)rows * dpad * 4;
  *a = FrArgs();
  a->X = X_dev, a->N = N, a->ldx = ldx, a->d = (int)d, a->dpad = dpad, a->rows = rows;
  while ((1 << a->cshift) < d && (1 << a->cshift) < FR_THREADS) a->cshift++;
  a->meta = (const int4*)meta_dev, a->tv = tv_dev, a->off = off_dev, a->n_nodes = n_nodes, a->T = (int)T;
  a->order = order_dev, a->n_order = (int)n_order, a->lds_nodes = lds_nodes < FR_LDS_NODES ? lds_nodes : FR_LDS_NODES;
  return 0;
}

template <class K>
static int fr_launch(bbh_handle* h, K kernel, const FrArgs& a, size_t lds) {
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  BBH_HIP_TRY(h, bbh_allow_lds(h->device, (const void*)kernel, lds));
  const unsigned grid = (unsigned)((a.N + a.rows - 1) / a.rows);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(FR_THREADS), lds, h->stream, a);
  BBH_HIP_TRY(h, hipGetLastError());
  return 0;
}

extern "C" int bbh_forest_predict(bbh_handle* h, const double* X_dev, int64_t N, int32_t d, int64_t ldx, const int32_t* meta_dev,
                                  const double* tv_dev, const int64_t* off_dev, int64_t T, int64_t n_nodes, const int32_t* order_dev,
                                  int64_t n_order, int32_t lds_nodes, double* P_dev) {
  if (!h) return -1;
  FrArgs a;
  size_t lds;
  int rc = fr_setup(h, "bbh_forest_predict", X_dev, N, d, ldx, meta_dev, tv_dev, off_dev, T, n_nodes, order_dev, n_order, lds_nodes, &a, &lds);
  if (rc) return rc;
  if (!P_dev) {
    h->err = "bbh_forest_predict: bad arguments (need the output)";
    return -1;
  }
  a.out0 = P_dev;
  return fr_launch(h, bbh_forest_predict_kernel, a, lds);
}

extern "C" int bbh_forest_moments(bbh_handle* h, const double* X_dev, int64_t N, int32_t d, int64_t ldx, const int32_t* meta_dev,
                                  const double* tv_dev, const int64_t* off_dev, int64_t T, int64_t n_nodes, const int32_t* order_dev,
                                  int64_t n_order, int32_t lds_nodes, double* mean_dev, double* var_dev) {
  if (!h) return -1;
  FrArgs a;
  size_t lds;
  int rc = fr_setup(h, "bbh_forest_moments", X_dev, N, d, ldx, meta_dev, tv_dev, off_dev, T, n_nodes, order_dev, n_order, lds_nodes, &a, &lds);
  if (rc) return rc;
  if (!mean_dev || !var_dev) {
    h->err = "bbh_forest_moments: bad arguments (need both outputs)";
    return -1;
  }
  a.out0 = mean_dev, a.out1 = var_dev;
  return fr_launch(h, bbh_forest_moments_kernel, a, lds);
}

extern "C" int bbh_forest_mc_acq(bbh_handle* h, int32_t kind, const double* X_dev, int64_t N, int32_t d, int64_t ldx,
                                 const int32_t* meta_dev, const double* tv_dev, const int64_t* off_dev, int64_t T, int64_t n_nodes,
                                 const int32_t* order_dev, int64_t n_order, int32_t lds_nodes, const int32_t* counts_dev, int64_t S,
                                 const double* pend_dev, int64_t k, double best_f, double sign, double beta, const uint8_t* alive_dev,
                                 double* scores_dev) {
  if (!h) return -1;
  FrArgs a;
  size_t lds;
  int rc = fr_setup(h, "bbh_forest_mc_acq", X_dev, N, d, ldx, meta_dev, tv_dev, off_dev, T, n_nodes, order_dev, n_order, lds_nodes, &a, &lds);
  if (rc) return rc;
  if (kind < BBH_ACQ_QLOGEI || kind > BBH_ACQ_QPSTD || !counts_dev || S < 1 || k < 0 || k > FR_MAX_PEND || (k > 0 && !pend_dev) || !scores_dev) {
    h->err = "bbh_forest_mc_acq: bad arguments (need an MC kind qLogEI ... qPSTD, the counts, S >= 1, 0 <= k <= 63 pending points with "
             "their per-tree values, and the output)";
    return -1;
  }
  a.counts = counts_dev, a.pend = pend_dev, a.k = (int)k, a.kind = kind, a.S = (double)S, a.best_f = best_f, a.sign = sign;
  a.cu = bbh_mc_cu(kind, beta), a.alive = alive_dev, a.out0 = scores_dev;
  if (kind == BBH_ACQ_QLOGEI) return fr_launch(h, bbh_forest_acq_kernel<true>, a, lds);
  return fr_launch(h, bbh_forest_acq_kernel<false>, a, lds);
}
