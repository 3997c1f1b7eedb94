// The cooperative conditional-mean columns kernel of qLogNEHVI (bbh_posterior_columns) and, on the same main loop, the fused
// qNEI / qLogNEI scoring pass (bbh_score_nei, bbh_nei.hip): one body, two epilogues.
#pragma once
#include "bbh_acqmath.h"
#include "bbh_coop.h"  // (bbh_fused.h with the translation unit's settings of bbh_panel.hip)

// Scoring epilogue of the fused qNEI / qLogNEI pass: what it reads besides the accumulators, and where the scores go.
struct NeiEpilogue {
  const double* var;     // [N] conditional variance of the candidates under the extended model
  const double* zx;      // [S] the candidate's base samples
  const double* best;    // [S] per-sample maximum of the oriented baseline draw
  const uint8_t* alive;  // [N] or null
  double* scores;        // [N]
  double sign;
  int S;                 // <= 512: one super-group holds the whole sample axis
};

// SM accumulators at the end of the main loop: lane (cnd, q) of wave w holds, for candidate tile0 + 16 t + cnd, the conditional
// means of samples col0 + 16 cb + q + 4 r (8 x 4 = 32 of the wave's 128).  Each lane turns its 32 samples into utility terms and
// sums them; the four q groups of a candidate meet by two shuffles, the four waves through 64 doubles of LDS per tile, and
// lane m of tile t writes one score.  Samples >= S (padding of the last column group) are left out; waves without a column
// group (S <= 384) contribute zero.
template <bool HAS_TBL, int NT, bool LOG>
__device__ __forceinline__ void bbh_nei_epilogue(const FusedArgs& a, const NeiEpilogue& ne, const d4 (&acc)[NT][8], const int (&tc)[NT],
                                                 double* red, bool live, int col0, int64_t tile0, int l, int w) {
  const int cnd = l & 15, q = l >> 4;
  const double* s_zb = red + NT * 64;  // [2][512]
#pragma unroll
  for (int t = 0; t < NT; t++) {
    double part = 0.0;
    if (live) {  // (wave-uniform)
      const int64_t gi = tile0 + 16 * t + cnd;
      const double sd = bbh_safe_sd(ne.var[gi < a.N ? gi : a.N - 1]);
      const double mc = (HAS_TBL && a.taskmean) ? a.taskmean[tc[t]] : a.mean_const;  // (this lane's own row)
      double p4[4] = {0.0, 0.0, 0.0, 0.0};  // one partial sum per r: four independent chains
#pragma unroll
      for (int cb = 0; cb < 8; cb++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int s = col0 + 16 * cb + q + 4 * r;
          const double term = bbh_nei_term<LOG>(a.ybar + a.ysd * (mc + acc[t][cb][r]), sd, s_zb[s], s_zb[512 + s], ne.sign);
          p4[r] += s < ne.S ? term : 0.0;
        }
      part = (p4[0] + p4[1]) + (p4[2] + p4[3]);
      part += __shfl_xor(part, 16, 64);
      part += __shfl_xor(part, 32, 64);
    }
    if (q == 0) red[t * 64 + w * 16 + cnd] = part;
  }
  __syncthreads();
  if (threadIdx.x < 16 * NT) {  // wave 0: lane m + 16 t finishes candidate m of tile t
    const int m = threadIdx.x & 15, t = threadIdx.x >> 4;
    const int64_t gi = tile0 + 16 * t + m;
    const double* rv = red + t * 64;
    const double sum = (rv[m] + rv[16 + m]) + (rv[32 + m] + rv[48 + m]);
    if (gi < a.N) ne.scores[gi] = (ne.alive && !ne.alive[gi]) ? -INFINITY : bbh_nei_finish<LOG>(sum, ne.S);
  }
}

// Cooperative variant for S >= 384 alternative columns: one workgroup per tile of 16 candidates, wave w contracts the tile's
// kernel values with column group 4 G + w (128 columns) of a super-group of 512.  The kernel values are the expensive part (a
// distance GEMM and a libm sqrt / exp per value: more pipe time than the 32 column MFMAs of a k-block) and the plain kernel
// (bbh_fused_columns_kernel, bbh_panel.hip) recomputes them for every group of 128 columns; here the four waves take turns - k-block 4 g + w is produced by wave w - and
// exchange them through a double-buffered 8 KB slot in LDS, one barrier per four k-blocks: every value is computed once per
// candidate for 512 columns.
// NT = candidate tiles (of 16) per workgroup: every column fragment that comes back from L2 feeds NT MFMAs (the column matrix is
// re-read by every workgroup: 1.2 MB per 16 NT candidates at n = 288, S = 512 - L2 -> L1 bandwidth, not HBM).
// SM (sample-major output [S, N]): the MFMAs run with swapped operands - the column fragment as A, the kernel values as B, the same
// registers either way - so that the accumulators hold the transposed block (lane = candidate, register = column) and a store
// instruction writes 16 consecutive candidates of a column (128 B) instead of 32 B pieces of 16 columns that lie N doubles apart.
// NEI != 0 (1 = qNEI, 2 = qLogNEI; SM only, one super-group): the accumulators are not stored but scored (bbh_nei_epilogue); the
// dynamic LDS then ends with [NT][4 waves][16] partial sums and the [2][512] sample table.
template <bool HAS_TBL, int KIND, int NT, bool SM, int NEI>
__device__ __forceinline__ void bbh_coop_columns_body(const FusedArgs& a, const double* __restrict__ colfrag, int64_t group0, int64_t groups,
                                                      int64_t nks, int64_t str_c, int64_t str_s, int64_t s_total,
                                                      double* __restrict__ tmat, const NeiEpilogue* ne) {
  extern __shared__ __attribute__((aligned(16))) double s_coopc[];  // candidate fragments [NT][kd][64] | kv [2][NT][4 k-blocks][4][64]
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int cnd = l & 15, q = l >> 4;
  const int64_t tile0 = (int64_t)blockIdx.x * 16 * NT;
  double* kvx = s_coopc + NT * a.kd * 64;
  if constexpr (NEI != 0) {  // the samples' candidate base sample and best baseline value, zero beyond S (visible after the barrier below)
    double* s_zb = kvx + 2 * NT * 1024 + NT * 64;
    for (int s = threadIdx.x; s < 512; s += 256) {
      s_zb[s] = s < ne->S ? ne->zx[s] : 0.0;
      s_zb[512 + s] = s < ne->S ? ne->best[s] : 0.0;
    }
  }
  int tc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int64_t row = (tile0 + 16 * t + cnd < a.N) ? tile0 + 16 * t + cnd : a.N - 1;
    const double* xr = a.X + row * a.ldx;
    double* candw = s_coopc + t * a.kd * 64;
    if (w == t) {  // tile t's normalised candidate fragments, augmented as in the plain kernel (wave t builds them; NT <= 4)
      double nbsum = 0.0;
      for (int k0 = 0; k0 < a.kd; k0++) {
        double v = 0.0;
        if (4 * k0 + q < a.dn) {
          v = fma(xr[a.numcol[4 * k0 + q]], a.scl[4 * k0 + q], a.ofs[4 * k0 + q]);
          nbsum = fma(v, v, nbsum);
        }
        candw[k0 * 64 + l] = v;
      }
      nbsum += __shfl_xor(nbsum, 16, 64);
      nbsum += __shfl_xor(nbsum, 32, 64);
      const int k1 = a.dn >> 2, q1 = a.dn & 3;
      if (q == q1) candw[k1 * 64 + l] = 1.0;
      const int k2 = (a.dn + 1) >> 2, q2 = (a.dn + 1) & 3;
      if (q == q2) candw[k2 * 64 + l] = nbsum;
    }
    tc[t] = 0;
    if (HAS_TBL && a.task_col >= 0) {
      tc[t] = (int)xr[a.task_col];
      tc[t] = tc[t] < 0 ? 0 : (tc[t] >= a.T ? a.T - 1 : tc[t]);
    }
  }
  __syncthreads();
  WaveCtx c[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    c[t].tf = a.trainfrag + l;
    c[t].candl = s_coopc + t * a.kd * 64 + l;
    c[t].mb = a.meanB + l;
    c[t].tbl = a.tasktbl;
    c[t].taskext = a.taskext;
    c[t].kvc = nullptr;
    c[t].kvl = (bbh_lds_double*)nullptr;
    c[t].nl = 0;
    c[t].ncache = 0;
    c[t].al = (const bbh_lds_double*)nullptr;
    c[t].kd = a.kd;
    c[t].kind = a.kind;
    c[t].T = a.T;
    c[t].tc = tc[t];
    c[t].q = q;
    c[t].l = l;
    c[t].dn = a.dn;
  }
  const bool live = group0 + w < groups;  // (the last super-group may have fewer than four column groups: those waves only produce)
  d4 acc[NT][8];
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int cb = 0; cb < 8; cb++) acc[t][cb] = (d4){0.0, 0.0, 0.0, 0.0};
  const double* cf = colfrag + (live ? group0 + w : group0) * nks * 8 * 64 + l;
  const int ngrp = (a.nb + 3) >> 2;
  // Column fragments through a register ring of RD k-steps (8 fragments each), refilled right after the MFMAs that consumed a slot:
  // the loads of k-step s + RD are in flight during the 8 NT (RD - 1) MFMAs in between (the fragments are static data: the ring runs
  // ahead across the group barriers).  As plain loads at the head of every k-block the first MFMA of each block waited out the
  // whole L2 latency: half the pipe time of this loop.
  constexpr int RD = (NT == 1 && KIND >= 0) ? 8 : 4;  // (runtime kernel kinds: the deeper ring spills)
  const int nsteps = 4 * a.nb;
  double ring[RD][8];
  if (live) {
#pragma unroll
    for (int i = 0; i < RD; i++)
      if (i < nsteps) {
#pragma unroll
        for (int cb = 0; cb < 8; cb++) ring[i][cb] = cf[((int64_t)i * 8 + cb) * 64];
      }
  }
  for (int g = 0; g < ngrp; g++) {
    double* slot = kvx + (g & 1) * (NT * 1024);
#pragma unroll
    for (int t = 0; t < NT; t++) {
      double kv[4] = {0.0, 0.0, 0.0, 0.0};
      if (4 * g + w < a.nb) compute_kv<HAS_TBL, KIND>(c[t], 4 * g + w, kv);
#pragma unroll
      for (int r = 0; r < 4; r++) slot[t * 1024 + (w * 4 + r) * 64 + l] = kv[r];
    }
    __syncthreads();  // one barrier per group: the buffer written two groups later is only reached after the next barrier
    if (live) {
#pragma unroll
      for (int blk = 0; blk < 16 / RD; blk++) {
#pragma unroll
        for (int i = 0; i < RD; i++) {
          const int step = 16 * g + blk * RD + i;  // k-step 4 tb + r
          if ((step >> 2) < a.nb) {  // wave-uniform
            double kvv[NT];
#pragma unroll
            for (int t = 0; t < NT; t++) kvv[t] = slot[t * 1024 + ((blk * RD + i) & 15) * 64 + l];
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
              for (int cb = 0; cb < 8; cb++)
                acc[t][cb] = SM ? mfma_f64(ring[i][cb], kvv[t], acc[t][cb]) : mfma_f64(kvv[t], ring[i][cb], acc[t][cb]);
            if (step + RD < nsteps) {
#pragma unroll
              for (int cb = 0; cb < 8; cb++) ring[i][cb] = cf[((int64_t)(step + RD) * 8 + cb) * 64];
            }
          }
        }
      }
    }
  }
  if constexpr (NEI != 0) {
    bbh_nei_epilogue<HAS_TBL, NT, NEI == 2>(a, *ne, acc, tc, kvx + 2 * NT * 1024, live, 128 * (int)(group0 + w), tile0, l, w);
    return;
  }
  if (!live) return;
  const int64_t col0 = 128 * (group0 + w);
  if (SM) {  // acc[t][cb][r]: column col0 + 16 cb + q + 4 r of candidate tile0 + 16 t + cnd
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const int64_t gi = tile0 + 16 * t + cnd;
      const double mc = (HAS_TBL && a.taskmean) ? a.taskmean[tc[t]] : a.mean_const;  // (this lane's own row: tc[t] is candidate cnd's task)
      if (gi < a.N) {
#pragma unroll
        for (int cb = 0; cb < 8; cb++)
#pragma unroll
          for (int r = 0; r < 4; r++)
            if (col0 + 16 * cb + q + 4 * r < s_total) tmat[gi * str_c + (col0 + 16 * cb + q + 4 * r) * str_s] = a.ybar + a.ysd * (mc + acc[t][cb][r]);
      }
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int64_t gi = tile0 + 16 * t + q + 4 * r;
      const int tcm = __shfl(tc[t], q + 4 * r, 64);  // lane m (< 16) holds candidate m's task
      const double mc = (HAS_TBL && a.taskmean) ? a.taskmean[tcm] : a.mean_const;
      if (gi < a.N) {
#pragma unroll
        for (int cb = 0; cb < 8; cb++)
          if (col0 + 16 * cb + cnd < s_total) tmat[gi * str_c + (col0 + 16 * cb + cnd) * str_s] = a.ybar + a.ysd * (mc + acc[t][cb][r]);
      }
    }
}

template <bool HAS_TBL, int KIND, int NT, bool SM>
__global__ __launch_bounds__(256, 2) void bbh_coop_columns_kernel(const FusedArgs a, const double* __restrict__ colfrag, int64_t group0,
                                                                  int64_t groups, int64_t nks, int64_t str_c, int64_t str_s,
                                                                  int64_t s_total, double* __restrict__ tmat) {
  bbh_coop_columns_body<HAS_TBL, KIND, NT, SM, 0>(a, colfrag, group0, groups, nks, str_c, str_s, s_total, tmat, nullptr);
}

// candidates in, N scores out: the conditional means never leave the registers.
// Register budget (-Rpass-analysis=kernel-resource-usage, gfx950; 256 VGPRs at two workgroups per CU): Matern-5/2 NT = 2 takes
// 254 - 256 VGPRs, NT = 1 248, runtime kinds (NT = 1) 224 - 228, all with 0 bytes of scratch.  NT = 2 has no headroom left: after a
// change to the epilogue or a compiler update, check that its ScratchSize is still 0 before trusting a timing.
template <bool HAS_TBL, int KIND, int NT, bool LOG>
__global__ __launch_bounds__(256, 2) void bbh_coop_nei_kernel(const FusedArgs a, const double* __restrict__ colfrag, int64_t groups,
                                                              int64_t nks, const NeiEpilogue ne) {
  bbh_coop_columns_body<HAS_TBL, KIND, NT, true, LOG ? 2 : 1>(a, colfrag, 0, groups, nks, 1, 0, ne.S, nullptr, &ne);
}
