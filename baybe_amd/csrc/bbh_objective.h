// Objective programs on the device: a target's transformation (baybe/transformations/basic.py) as at most BBH_OBJ_MAX_OPS scalar
// operations (bbh_objective_prog, include/baybe_hip.h), evaluated per posterior sample between the draw and the utility
// (bbh_objacq.hip).  Host-side counterpart and numpy interpreter: baybe_amd/objective.py.
#pragma once
#include <math.h>

#include "bbh_common.h"

// The program is a kernel argument passed by value, so every field is wave-uniform (scalar registers) and the branches below are
// uniform.  The loop is fully unrolled: op[k] / p[k][..] are then read at compile-time offsets of the argument segment - a run-time
// index into the by-value struct would send it to scratch memory.
__device__ __forceinline__ double bbh_apply_objective(const bbh_objective_prog& prog, double y) {
#pragma unroll
  for (int k = 0; k < BBH_OBJ_MAX_OPS; k++) {
    if (k >= prog.n_ops) break;
    const int op = prog.op[k];
    const double p0 = prog.p[k][0], p1 = prog.p[k][1], p2 = prog.p[k][2];
    if (op == BBH_OBJ_AFFINE) {
      y = y * p0 + p1;  // (not fused: the host interpreter and the reference round the product)
    } else if (op == BBH_OBJ_CLAMP) {
      y = (y != y) ? y : fmin(fmax(y, p0), p1);  // NaN stays NaN, as torch.clamp
    } else if (op == BBH_OBJ_TWOSIDED) {
      y = (y - p2) * ((y < p2) ? p0 : p1);
    } else if (op == BBH_OBJ_LOG) {
      y = log(y);
    } else if (op == BBH_OBJ_POW) {  // integer exponent by squaring (uniform trip count; negative bases keep their sign rule)
      const int n = (int)p0;
      unsigned m = n < 0 ? 0u - (unsigned)n : (unsigned)n;
      double r = 1.0, b = y;
      while (m) {
        if (m & 1u) r *= b;
        m >>= 1;
        if (m) b *= b;
      }
      y = n < 0 ? 1.0 / r : r;
    } else {  // BELL, EXP, SIGMOID: one exponential
      double t = y;
      if (op == BBH_OBJ_BELL) {
        const double u = (y - p0) / p1;
        t = -(u * u) / 2.0;
      } else if (op == BBH_OBJ_SIGMOID) {
        t = p1 * (y - p0);
      }
      const double e = exp(t);
      y = (op == BBH_OBJ_SIGMOID) ? 1.0 / (1.0 + e) : e;
    }
  }
  return y;
}
