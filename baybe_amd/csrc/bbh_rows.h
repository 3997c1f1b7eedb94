// The row-distance core shared by the kernels that work on the resident matrix P [d][ldp] of bbh_fps_prepare: farthest point
// sampling (bbh_fps.hip), k-medoids (bbh_pam.hip), k-means (bbh_kmeans.hip) and the Gaussian mixture (bbh_gmm.hip).
//
// The arithmetic contract, stated here once:
//   * d2(x, y) = sum_k (x_k - y_k) * (x_k - y_k), k ascending from 0.0, subtract / multiply / add each rounded to fp64.
//     Contraction is off from here to the end of the including file, so no v_fma_f64 appears in a distance chain and every
//     comparison of two distances sees the bits a numpy loop over k produces.  (x - y)^2 is symmetric bit for bit.
//   * Every sum has a fixed shape (no floating-point atomics): the 64-lane butterfly, then the four waves in order.
//   * Every tie goes to the first position: chains are visited in ascending j, keys compare their positions last.
#pragma once
#include <math.h>

#include <type_traits>

#include "bbh_common.h"

#pragma clang fp contract(off)

#define BBH_ROWS_TILE 256           // rows per workgroup (one per thread)
#define BBH_ROWS_TJ 64              // rows j per LDS tile of the register-form pair walk
#define BBH_ROWS_MAX 2147483392ll   // positions are 32-bit inside the kernels (2^31 - 256)
#define BBH_ROWS_MAX_D 768          // an 8-column tile of d coordinates within the default LDS limit

// max_d = 0: no limit on the columns (an entry point whose kernels loop over any d)
inline int bbh_rows_check(bbh_handle* h, const char* who, const double* P, int64_t M, int32_t d, int64_t ldp, int max_d = BBH_ROWS_MAX_D) {
  if (!P || M < 1 || M > BBH_ROWS_MAX || d < 1 || (max_d && d > max_d) || ldp < M) {
    h->err = std::string(who) + ": bad arguments (need the matrix, 1 <= M < 2^31 - 256, " +
             (max_d ? "1 <= d <= " + std::to_string(max_d) : std::string("d >= 1")) + ", ld >= M)";
    return -1;
  }
  return 0;
}

// tile width (log2) of a [d][T] LDS tile of doubles within 48 KB
inline int bbh_rows_tile_shift(int d) { return (d <= 96) ? 6 : (d <= 192) ? 5 : (d <= 384) ? 4 : 3; }

// f(std::integral_constant<int, DP>): the register-form width DP >= d, or 0 for the generic form (d > 32)
template <class F>
inline void bbh_rows_dispatch_dp(int d, F&& f) {
  if (d <= 2) f(std::integral_constant<int, 2>());
  else if (d <= 4) f(std::integral_constant<int, 4>());
  else if (d <= 8) f(std::integral_constant<int, 8>());
  else if (d <= 12) f(std::integral_constant<int, 12>());
  else if (d <= 16) f(std::integral_constant<int, 16>());
  else if (d <= 20) f(std::integral_constant<int, 20>());
  else if (d <= 24) f(std::integral_constant<int, 24>());
  else if (d <= 32) f(std::integral_constant<int, 32>());
  else f(std::integral_constant<int, 0>());
}

// d2 between the columns a and b of P
__device__ __forceinline__ double bbh_rows_d2(const double* __restrict__ P, int64_t ldp, int d, int64_t a, int64_t b) {
  double acc = 0.0;
  for (int k = 0; k < d; k++) {
    const double t = P[(int64_t)k * ldp + a] - P[(int64_t)k * ldp + b];
    acc = acc + t * t;
  }
  return acc;
}

// eight chains: acc[u] = d2(x, entry u of the tile), x[k * x_stride] in global memory or LDS, the tile in LDS as [k][tile_stride]
__device__ __forceinline__ void bbh_rows_d2x8(const double* x, int64_t x_stride, const double* tile, int tile_stride, int d, double (&acc)[8]) {
#pragma unroll
  for (int u = 0; u < 8; u++) acc[u] = 0.0;
  for (int k = 0; k < d; k++) {
    const double xk = x[(int64_t)k * x_stride];
    const double* ts = tile + k * tile_stride;
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const double t = xk - ts[u];
      acc[u] = acc[u] + t * t;
    }
  }
}

// ---- the pair walks: row i against the rows [j_begin, j_end), in ascending j --------------------------------------------------------
// A load policy says which rows j are read - bool live(int j): false for a j beyond the range or a dead one - and what the others
// are staged as: double pad().  Its  whole_tiles  says whether such entries count as rows (true: the walk takes every tile in
// full and the visitor sees them, e.g. as NaN) or not (false: the walk stops at j_end).  visit(j, d2, exists) is called for the
// chains of a group in ascending j; exists is false for the chains of the last group beyond j_end, which ran all the same.
// A visitor writes a conditional update as a select (x = c ? y : x), not as an if: a branch between the chains of a group lets the
// optimiser sink a whole chain below it, which keeps the tile's LDS values live (46 more VGPRs at DP = 32).

// Register form, d <= DP <= 32: row i in DP registers (columns beyond d are zero: adding +0.0 changes no bit of a sum that starts
// at +0.0), tiles of 64 rows j staged in s_x as [j][DP] through a prefetch and read at wave-uniform addresses, four chains in
// flight.  j_begin < j_end.
template <int DP, class Load, class Visit>
__device__ __forceinline__ void bbh_rows_pair_walk(const double* P, int64_t ldp, int d, int i, bool live_i, int j_begin, int j_end, double* s_x,
                                                   Load load, Visit visit) {
  constexpr int NPRE = (BBH_ROWS_TJ * DP + 255) / 256;
  const int tid = threadIdx.x;
  double xi[DP];
#pragma unroll
  for (int k = 0; k < DP; k++) xi[k] = (k < d && live_i) ? P[(int64_t)k * ldp + i] : 0.0;
  double pre[NPRE];
  auto fetch = [&](int jt) {
#pragma unroll
    for (int u = 0; u < NPRE; u++) {
      const int e = tid + u * 256;
      const int k = e >> 6, j = jt + (e & 63);
      pre[u] = (k < d && load.live(j)) ? P[(int64_t)k * ldp + j] : (k < d) ? load.pad() : 0.0;
    }
  };
  fetch(j_begin);
  for (int j0 = j_begin; j0 < j_end; j0 += BBH_ROWS_TJ) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NPRE; u++) {
      const int e = tid + u * 256;
      if (e < BBH_ROWS_TJ * DP) s_x[(e & 63) * DP + (e >> 6)] = pre[u];
    }
    __syncthreads();
    if (j0 + BBH_ROWS_TJ < j_end) fetch(j0 + BBH_ROWS_TJ);  // in flight during the tile's arithmetic
    const int nj = (Load::whole_tiles || j_end - j0 >= BBH_ROWS_TJ) ? BBH_ROWS_TJ : j_end - j0;
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
      const int j = j0 + jj;  // the four chains ran side by side; they are visited in j order
      visit(j, a0, true);
      visit(j + 1, a1, Load::whole_tiles || jj + 1 < nj);
      visit(j + 2, a2, Load::whole_tiles || jj + 2 < nj);
      visit(j + 3, a3, Load::whole_tiles || jj + 3 < nj);
    }
  }
}

// Generic form, any d <= 768: eight chains, x_i re-read from xi (= P + i, a valid address for idle lanes too) per group of eight j,
// the j tile in s_t as [k][TJ], TJ = 1 << tj_shift = 1 << bbh_rows_tile_shift(d), d * TJ doubles.
template <class Load, class Visit>
__device__ __forceinline__ void bbh_rows_pair_walk_generic(const double* P, int64_t ldp, int d, const double* xi, int j_begin, int j_end,
                                                           int tj_shift, double* s_t, Load load, Visit visit) {
  const int TJ = 1 << tj_shift;
  const int tid = threadIdx.x;
  for (int j0 = j_begin; j0 < j_end; j0 += TJ) {
    __syncthreads();
    for (int e = tid; e < d * TJ; e += 256) {
      const int k = e >> tj_shift, j = j0 + (e & (TJ - 1));
      s_t[e] = load.live(j) ? P[(int64_t)k * ldp + j] : load.pad();
    }
    __syncthreads();
    const int nj = (Load::whole_tiles || j_end - j0 >= TJ) ? TJ : j_end - j0;
    for (int jj = 0; jj < nj; jj += 8) {
      double acc[8];
      bbh_rows_d2x8(xi, ldp, s_t + jj, TJ, d, acc);
#pragma unroll
      for (int u = 0; u < 8; u++) visit(j0 + jj + u, acc[u], Load::whole_tiles || jj + u < nj);
    }
  }
}

// ---- the fixed-shape sums -----------------------------------------------------------------------------------------------------------
// the same bits in every lane: a + b == b + a
__device__ __forceinline__ double bbh_rows_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// the four wave partials in order
__device__ __forceinline__ double bbh_rows_sum4(const double* w) { return ((w[0] + w[1]) + w[2]) + w[3]; }

// the sum over the 256 threads of a workgroup, in every thread; s4: four doubles of LDS that nobody is reading
__device__ __forceinline__ double bbh_rows_block4_sum(double v, double* s4) {
  v = bbh_rows_wave_sum(v);
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return bbh_rows_sum4(s4);
}

// ---- the key reduction --------------------------------------------------------------------------------------------------------------
// The best key of the 256 threads of a workgroup, in every thread: butterfly, then the four wave keys with the first wave winning
// ties.  Key: a struct with  Key shfl_xor(int o) const  (its members from lane ^ o); beats(x, y): does x strictly beat y (a total
// order: equal keys beat nobody); scratch: four keys of LDS that nobody is reading.
template <class Key, class Beats>
__device__ __forceinline__ Key bbh_rows_block_best(Key key, Key* scratch, Beats beats) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const Key other = key.shfl_xor(o);
    if (beats(other, key)) key = other;
  }
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = key;
  __syncthreads();
  key = scratch[0];
  for (int w = 1; w < 4; w++)
    if (beats(scratch[w], key)) key = scratch[w];
  return key;
}

// (value ascending, position ascending); p = -1: no key
struct bbh_rows_min_key {
  double v;
  long long p;
  __device__ __forceinline__ bbh_rows_min_key shfl_xor(int o) const { return {__shfl_xor(v, o, 64), __shfl_xor(p, o, 64)}; }
};
__device__ __forceinline__ bool bbh_rows_min_beats(const bbh_rows_min_key& x, const bbh_rows_min_key& y) {
  return x.p >= 0 && (y.p < 0 || x.v < y.v || (x.v == y.v && x.p < y.p));
}
