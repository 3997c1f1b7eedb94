// Scaffold of the sample-sliced Monte-Carlo scorers (pending-point qLogEI in bbh_acq.hip, qLogNEHVI / qNEHVI in bbh_qnehvi.hip,
// qLogNParEGO in bbh_nparego.hip, qEHVI / qLogEHVI in bbh_ehvi.hip): one thread per candidate and sample slice (blockIdx.y), every
// slice's partial to the workspace, one finish kernel that combines the partials in slice order (no atomics: two runs give the
// same bits).  Here: the slice bounds, the per-target operand block, the finish kernel and the target-count dispatch.  What a
// scorer adds is its per-sample arithmetic and the policy that chooses its slice count.
#pragma once
#include <type_traits>

#include "bbh_acqmath.h"  // bbh_nei_finish

// ---- slice bounds: slice k of `per` samples each is [begin, end); a slice that starts at or beyond S is empty (begin >= end) ----
struct bbh_slice {
  int begin, end, count;  // count = max(end - begin, 0)
};
__device__ __forceinline__ bbh_slice bbh_slice_bounds(int S, int per, int k) {
  const int b = k * per;
  return {b, (b + per < S) ? b + per : S, (b + per <= S) ? per : (S > b ? S - b : 0)};
}
// kernels launched with a wanted slice count derive the length from the grid: the same number as bbh_slices_by_count's
__device__ __forceinline__ int bbh_slice_per(int S) { return (S + (int)gridDim.y - 1) / (int)gridDim.y; }

struct bbh_slicing {
  int per, count;  // samples per slice, slices (gridDim.y)
};
static inline bbh_slicing bbh_slices_by_len(int64_t S, int64_t per) { return {(int)per, (int)((S + per - 1) / per)}; }
static inline bbh_slicing bbh_slices_by_count(int64_t S, int64_t count) { return {(int)((S + count - 1) / count), (int)count}; }

// ---- per-target operands of the multi-objective scorers ----
struct bbh_targets {
  const double* tmat[BBH_MAX_OBJECTIVES];  // conditional means, [S, N] sample-major (qLogNEHVI's candidate-major entry point: [N, S])
  const double* var[BBH_MAX_OBJECTIVES];   // [N]
  double sign[BBH_MAX_OBJECTIVES];
};
// false: a used target without conditional means or variances while there are rows to score
static inline bool bbh_fill_targets(bbh_targets& t, int32_t m, int64_t N, const double* const* tmat_dev, const double* const* var_dev,
                                    const double* sign_host) {
  for (int o = 0; o < BBH_MAX_OBJECTIVES; o++) {
    t.tmat[o] = o < m ? tmat_dev[o] : nullptr;
    t.var[o] = o < m ? var_dev[o] : nullptr;
    t.sign[o] = o < m ? sign_host[o] : 1.0;
    if (o < m && N > 0 && (!t.tmat[o] || !t.var[o])) return false;
  }
  return true;
}

// ---- finish: partial[(k rows) N + i] over the slices k in slice order -> score; a masked row scores -inf (its partials are not read) ----
enum bbh_finish {
  BBH_FINISH_MEAN,         // total / S                                          (NaN propagates)
  BBH_FINISH_LOG_MEAN,     // log(total) - log(S), -inf unless total > 0         (qLogNEHVI)
  BBH_FINISH_LOG_TAU_MEAN, // log(tau_relu) + log(total) - log(S)                (sums of fatplus / tau_relu; NaN propagates)
  BBH_FINISH_LSE_PAIRS,    // partials are (reference, sum) pairs of streaming logsumexps in rows 2k, 2k + 1 (rows = 2)
};

template <bbh_finish F>
__global__ __launch_bounds__(256) void bbh_slices_finish_kernel(const double* __restrict__ partial, int slices, int rows, int64_t N, int S,
                                                                const uint8_t* __restrict__ alive, double* __restrict__ scores) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  if (alive && !alive[i]) {
    scores[i] = -INFINITY;
    return;
  }
  if constexpr (F == BBH_FINISH_LSE_PAIRS) {
    double ref = -INFINITY, sum = 0.0;
    for (int k = 0; k < slices; k++) {
      const double rk = partial[(int64_t)(rows * k) * N + i], sk = partial[(int64_t)(rows * k + 1) * N + i];
      if (rk > ref) {
        sum = sum * exp(ref - rk) + sk;
        ref = rk;
      } else {
        sum += (sk == 0.0) ? 0.0 : sk * exp(rk - ref);
      }
    }
    scores[i] = ref + log(sum) - log((double)S);
  } else {
    double total = 0.0;
    for (int k = 0; k < slices; k++) total += partial[(int64_t)(rows * k) * N + i];
    if constexpr (F == BBH_FINISH_MEAN) scores[i] = bbh_nei_finish<false>(total, S);
    if constexpr (F == BBH_FINISH_LOG_MEAN) scores[i] = (total > 0.0) ? log(total) - log((double)S) : -INFINITY;
    if constexpr (F == BBH_FINISH_LOG_TAU_MEAN) scores[i] = bbh_nei_finish<true>(total, S);
  }
}

template <bbh_finish F>
static inline void bbh_slices_finish(bbh_handle* h, const double* partial, int slices, int rows, int64_t N, int64_t S,
                                     const uint8_t* alive_dev, double* scores_dev) {
  hipLaunchKernelGGL(bbh_slices_finish_kernel<F>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, partial, slices, rows, N,
                     (int)S, alive_dev, scores_dev);
}

// ---- dispatch: f(std::integral_constant<int, M>) for M == m in M0 ... BBH_MAX_OBJECTIVES (the caller has checked the range; a
// larger m takes the last instantiation), f(std::bool_constant<b>) for a flag ----
template <int M0 = 1, class F>
static inline decltype(auto) bbh_dispatch_m(int m, F&& f) {
  if constexpr (M0 < BBH_MAX_OBJECTIVES) {
    if (m != M0) return bbh_dispatch_m<M0 + 1>(m, f);
  }
  return f(std::integral_constant<int, M0>());
}
template <class F>
static inline decltype(auto) bbh_dispatch_flag(bool b, F&& f) {
  if (b) return f(std::true_type());
  return f(std::false_type());
}
