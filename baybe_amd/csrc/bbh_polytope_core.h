// The per-chain and per-point bodies of bbh_polytope.hip: one hit-and-run chain, one projection onto
//   { c in R^dc : lo <= c <= hi, E c = e, G c >= g }.
// Plain C++ on pointers with a stride (the kernels keep a thread's state in LDS at [index * stride]); the same text compiles for the
// host with stride 1, which is how the bodies were first held against the numpy restatement.
//
// The arithmetic contract is that of bbh_rows.h: nothing contracted (no fused multiply-add), every sum over the columns and over
// the rows ascending from 0.0, each product and each addition rounded to fp64; no transcendental function anywhere.  The sampler
// is therefore a function of its arguments alone that a numpy loop reproduces bit for bit (tests/_oracle_polytope.py).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BBH_POLY_HD __host__ __device__ __forceinline__
#else
#define BBH_POLY_HD inline
#endif

#pragma clang fp contract(off)

#define BBH_POLY_MAX_DC 32     // continuous columns (MAX_GRADIENT_CONTINUOUS)
#define BBH_POLY_MAX_ROWS 16   // equality + inequality rows after normalisation
#define BBH_POLY_FEAS_C 4.0    // C of the feasibility bound C (dc + M) eps S_abs the projection meets and recognises
#define BBH_POLY_MAX_ITER 200  // trial points of one projection before it reports status 1
#define BBH_POLY_GOLDEN 0x9E3779B97F4A7C15ull

// ---- counter-based uniforms: SplitMix64's finaliser on a Weyl sequence ---------------------------------------------------------
// key(seed, chain) = mix(mix(seed + G) + G (chain + 1));  h(step, draw) = mix(key + G (64 step + draw + 1)), draw < 64;
// u = (h >> 11) 2^-53 in [0, 1).  G = 0x9E3779B97F4A7C15 (SplitMix64's increment): h is SplitMix64's output number
// 64 step + draw + 1 of the generator seeded with key.  All of it in wrapping 64-bit integer arithmetic, no state anywhere.
BBH_POLY_HD uint64_t bbh_poly_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
BBH_POLY_HD uint64_t bbh_poly_chain_key(uint64_t seed, uint64_t chain) {
  return bbh_poly_mix64(bbh_poly_mix64(seed + BBH_POLY_GOLDEN) + BBH_POLY_GOLDEN * (chain + 1ull));
}
BBH_POLY_HD double bbh_poly_uniform(uint64_t key, uint64_t step, uint64_t draw) {
  const uint64_t h = bbh_poly_mix64(key + BBH_POLY_GOLDEN * (64ull * step + draw + 1ull));
  return (double)(h >> 11) * 0x1.0p-53;
}

// The feasible set in the reduced coordinates c = c0 + Z y, y in R^dz (Z an orthonormal basis of null(E), c0 the Chebyshev centre):
//   bl_k <= Z_k . y <= bu_k  (bl = lo - c0, bu = hi - c0; the 2 dc box rows share their dot product),   GZ_i . y >= bg_i.
struct bbh_poly_reduced {
  const double* Z;   // [dc, dz]
  const double* GZ;  // [mi, dz]
  const double* c0;  // [dc]
  const double* lo;  // [dc]
  const double* hi;  // [dc]
  const double* bl;  // [dc]
  const double* bu;  // [dc]
  const double* bg;  // [mi]
  int dc, dz, mi;
};

// One chain of T hit-and-run steps from y = 0; y and d are the chain's [dz] state at stride st; out [dc] receives
// clip(c0 + Z y, lo, hi).  One step: d_j = u_j - 1/2 (draws 0 .. dz - 1), the chord [t_lo, t_hi] by the ratio test over all rows with
// the slacks recomputed from y, widened to hold 0 (a slack that rounding made negative must not turn the chord inside out),
// t = t_lo + u' (t_hi - t_lo) (draw dz), y += t d.
BBH_POLY_HD void bbh_poly_chain(const bbh_poly_reduced& P, uint64_t seed, uint64_t chain, int T, double* y, double* d, int st, double* out) {
  const int dc = P.dc, dz = P.dz, mi = P.mi;
  const uint64_t key = bbh_poly_chain_key(seed, chain);
  for (int j = 0; j < dz; j++) y[j * st] = 0.0;
  for (int step = 0; step < T; step++) {
    for (int j = 0; j < dz; j++) d[j * st] = bbh_poly_uniform(key, (uint64_t)step, (uint64_t)j) - 0.5;
    const double up = bbh_poly_uniform(key, (uint64_t)step, (uint64_t)dz);
    double tlo = -INFINITY, thi = INFINITY;
    for (int k = 0; k < dc; k++) {
      const double* z = P.Z + (size_t)k * dz;
      double w = 0.0, v = 0.0;
      for (int j = 0; j < dz; j++) {
        w = w + z[j] * y[j * st];
        v = v + z[j] * d[j * st];
      }
      const double sl = w - P.bl[k], su = P.bu[k] - w;  // slacks of the lower and the upper bound
      if (v > 0.0) {
        tlo = fmax(tlo, -sl / v);
        thi = fmin(thi, su / v);
      } else if (v < 0.0) {
        thi = fmin(thi, -sl / v);
        tlo = fmax(tlo, su / v);
      }
    }
    for (int i = 0; i < mi; i++) {
      const double* gz = P.GZ + (size_t)i * dz;
      double w = 0.0, v = 0.0;
      for (int j = 0; j < dz; j++) {
        w = w + gz[j] * y[j * st];
        v = v + gz[j] * d[j * st];
      }
      const double s = w - P.bg[i];
      if (v > 0.0)
        tlo = fmax(tlo, -s / v);
      else if (v < 0.0)
        thi = fmin(thi, -s / v);
    }
    tlo = fmin(tlo, 0.0);
    thi = fmax(thi, 0.0);
    double t = 0.0;  // (a direction along which no row moves - d = 0 - leaves the chain where it is)
    if (tlo > -INFINITY && thi < INFINITY) t = tlo + up * (thi - tlo);
    for (int j = 0; j < dz; j++) y[j * st] = y[j * st] + t * d[j * st];
  }
  for (int k = 0; k < dc; k++) {
    const double* z = P.Z + (size_t)k * dz;
    double acc = 0.0;
    for (int j = 0; j < dz; j++) acc = acc + z[j] * y[j * st];
    double c = P.c0[k] + acc;
    c = c < P.lo[k] ? P.lo[k] : (c > P.hi[k] ? P.hi[k] : c);
    out[k] = c;
  }
}

// ---- projection -----------------------------------------------------------------------------------------------------------------
// The rows R [m, dc] = [E; G] with right-hand sides t [m] = [e; g], m = me + mi <= 16.  The dual of the projection of p in the m
// multipliers nu (free for an equality, >= 0 for an inequality), the box applied as a clip:
//   x(nu) = clip(p + R^T nu, lo, hi),   q(nu) = 1/2 |x - p|^2 - nu . (R x - t)  concave and piecewise quadratic,  grad q = -(R x - t).
// A regularised semismooth Newton ascent on q: working rows W = equalities and the inequalities with nu_i > 0 or a violated row;
// (R_WF R_WF^T + mu I) delta = -(R x - t)_W over the coordinates F strictly inside the box; nu <- max(nu + delta, 0).  A trial is
// kept if q rose (or, within the rounding of q, if the KKT measure fell), and mu shrinks tenfold; otherwise mu grows.  A damped
// step, and one taken where every coordinate is clipped (the Hessian is 0, q linear), is doubled while q keeps rising.  For the
// mixture case m = 1 this is the Newton form of the monotone piecewise-linear root find.  Once the multipliers have converged at
// the scale of p, the point itself is refined on its face (x_F -= R_WF^T delta), which brings the residuals down to the scale of x:
// |p| may be far larger.
struct bbh_poly_rows {
  const double* R;   // [m, dc]
  const double* t;   // [m]
  const double* lo;  // [dc]
  const double* hi;  // [dc]
  int dc, me, mi;
  double tolf;    // C (dc + M) eps, M = 2 dc + mi
  double mu_min;  // 1e-10 max_i |R_i|^2
};

// per-point scratch at stride st: nu [m], nun [m], rho [m], x [dc], dl [m], H [m (m + 1) / 2]
#define BBH_POLY_STATE(m, dc) (4 * (m) + (dc) + (m) * ((m) + 1) / 2)

// rho = R x - t; returns the worst violation over its tolerance tolf S_i.  kkt: an inequality with nu_i > 0 counts as an equality,
// and S_i is taken at the scale of p (sum_k |R_ik| max(|x_k|, |p_k|) + |t_i|); otherwise feasibility alone at the scale of x:
// S_abs,i = sum_k |R_ik x_k| + |t_i|.
BBH_POLY_HD double bbh_poly_residuals(const bbh_poly_rows& Q, const double* x, const double* p, const double* nu, bool kkt, double* rho, int st) {
  const int dc = Q.dc, m = Q.me + Q.mi;
  double phi = 0.0;
  for (int i = 0; i < m; i++) {
    const double* r = Q.R + (size_t)i * dc;
    double acc = 0.0, s = 0.0;
    for (int k = 0; k < dc; k++) {
      const double xk = x[k * st];
      acc = acc + r[k] * xk;
      s = s + (kkt ? fabs(r[k]) * fmax(fabs(xk), fabs(p[k])) : fabs(r[k] * xk));
    }
    acc = acc - Q.t[i];
    s = s + fabs(Q.t[i]);
    rho[i * st] = acc;
    const bool two_sided = i < Q.me || (kkt && nu[i * st] > 0.0);
    const double viol = two_sided ? fabs(acc) : (acc < 0.0 ? -acc : 0.0);
    const double tol = Q.tolf * s;
    if (viol > tol) phi = fmax(phi, tol > 0.0 ? viol / tol : INFINITY);
  }
  return phi;
}

// x = clip(p + R^T nu); returns q(nu) without its nu . rho term; *mask: the coordinates strictly inside the box
BBH_POLY_HD double bbh_poly_point(const bbh_poly_rows& Q, const double* p, const double* nu, double* x, int st, uint32_t* mask) {
  const int dc = Q.dc, m = Q.me + Q.mi;
  double q = 0.0;
  uint32_t f = 0;
  for (int k = 0; k < dc; k++) {
    double z = p[k];
    for (int i = 0; i < m; i++) z = z + nu[i * st] * Q.R[(size_t)i * dc + k];
    if (z > Q.lo[k] && z < Q.hi[k]) f |= 1u << k;
    const double xk = z < Q.lo[k] ? Q.lo[k] : (z > Q.hi[k] ? Q.hi[k] : z);
    x[k * st] = xk;
    const double dx = xk - p[k];
    q = q + 0.5 * (dx * dx);
  }
  *mask = f;
  return q;
}

// Solves (R_WF R_WF^T + mu I) delta = rhs on the working rows (bit i of work), delta_i = 0 elsewhere; rhs in, delta out, in place.
BBH_POLY_HD void bbh_poly_solve(const bbh_poly_rows& Q, uint32_t work, uint32_t freem, double mu, double* H, double* v, int st) {
  const int dc = Q.dc, m = Q.me + Q.mi;
  for (int i = 0; i < m; i++)
    for (int j = 0; j <= i; j++) {
      double acc = 0.0;
      if ((work >> i & 1u) && (work >> j & 1u)) {
        for (int k = 0; k < dc; k++)
          if (freem >> k & 1u) acc = acc + Q.R[(size_t)i * dc + k] * Q.R[(size_t)j * dc + k];
        if (i == j) acc = acc + mu;
      } else if (i == j) {
        acc = 1.0;
      }
      H[(i * (i + 1) / 2 + j) * st] = acc;
    }
  for (int i = 0; i < m; i++)
    if (!(work >> i & 1u)) v[i * st] = 0.0;
  // Cholesky H = L L^T in place (packed lower), then the two triangular solves
  for (int j = 0; j < m; j++) {
    double djj = H[(j * (j + 1) / 2 + j) * st];
    for (int l = 0; l < j; l++) {
      const double a = H[(j * (j + 1) / 2 + l) * st];
      djj = djj - a * a;
    }
    if (!(djj > 0.0)) djj = mu;  // (rounding on a dependent row: the regulariser is what is left of its pivot)
    djj = sqrt(djj);
    H[(j * (j + 1) / 2 + j) * st] = djj;
    for (int i = j + 1; i < m; i++) {
      double a = H[(i * (i + 1) / 2 + j) * st];
      for (int l = 0; l < j; l++) a = a - H[(i * (i + 1) / 2 + l) * st] * H[(j * (j + 1) / 2 + l) * st];
      H[(i * (i + 1) / 2 + j) * st] = a / djj;
    }
  }
  for (int i = 0; i < m; i++) {
    double a = v[i * st];
    for (int l = 0; l < i; l++) a = a - H[(i * (i + 1) / 2 + l) * st] * v[l * st];
    v[i * st] = a / H[(i * (i + 1) / 2 + i) * st];
  }
  for (int i = m - 1; i >= 0; i--) {
    double a = v[i * st];
    for (int l = i + 1; l < m; l++) a = a - H[(l * (l + 1) / 2 + i) * st] * v[l * st];
    v[i * st] = a / H[(i * (i + 1) / 2 + i) * st];
  }
}

// Projects p [dc] (unit stride); ws: BBH_POLY_STATE doubles at stride st; out [dc] (unit stride) in [lo, hi] bit-exactly.
// Returns 0, or 1 when the iteration budget ran out (out is then the clipped point of the last multipliers).
BBH_POLY_HD int bbh_poly_project(const bbh_poly_rows& Q, const double* p, double* ws, int st, double* out) {
  const int dc = Q.dc, me = Q.me, m = Q.me + Q.mi;
  double* nu = ws;
  double* nun = nu + (size_t)m * st;
  double* rho = nun + (size_t)m * st;
  double* x = rho + (size_t)m * st;
  double* dl = x + (size_t)dc * st;
  double* H = dl + (size_t)m * st;
  for (int k = 0; k < dc; k++)
    if (!(fabs(p[k]) < INFINITY)) {  // (NaN or infinite: there is nothing to project)
      for (int kk = 0; kk < dc; kk++) out[kk] = Q.lo[kk];
      return 1;
    }
  for (int i = 0; i < m; i++) nu[i * st] = 0.0;
  uint32_t freem = 0;
  double q = bbh_poly_point(Q, p, nu, x, st, &freem);
  // a point that is in the box and meets the feasibility bound comes back bit for bit
  bool inside = true;
  for (int k = 0; k < dc; k++) inside = inside && x[k * st] == p[k];
  if (inside && bbh_poly_residuals(Q, x, p, nu, false, rho, st) <= 1.0) {
    for (int k = 0; k < dc; k++) out[k] = p[k];
    return 0;
  }
  double phi = bbh_poly_residuals(Q, x, p, nu, true, rho, st);
  bool converged = phi <= 1.0;
  int evals = 0;
  double mu = Q.mu_min;
  while (evals < BBH_POLY_MAX_ITER && !converged) {
    uint32_t work = 0, freen = 0;
    double qf = q;  // q(nu): the residuals of nu are in rho
    // working rows: the equalities, the inequalities that carry a multiplier, and of the violated others the worst one (a dual
    // active-set step: rows enter one at a time, so that the working rows stay as independent as the solution's are)
    int worst = -1;
    double worst_v = 0.0;
    for (int i = 0; i < m; i++) {
      const double r = rho[i * st];
      if (i < me || nu[i * st] > 0.0) {
        work |= 1u << i;
      } else if (r < 0.0) {
        double nrm = 0.0;
        for (int k = 0; k < dc; k++) nrm = nrm + Q.R[(size_t)i * dc + k] * Q.R[(size_t)i * dc + k];
        const double v = (r * r) / nrm;  // squared distance to the row's half-space
        if (v > worst_v) {
          worst_v = v;
          worst = i;
        }
      }
      qf = qf - nu[i * st] * r;
      dl[i * st] = -r;
    }
    if (worst >= 0) work |= 1u << worst;
    bbh_poly_solve(Q, work, freem, mu, H, dl, st);
    double tau = 1.0, best_tau = 0.0, best_q = qf, phin = phi;
    bool by_measure = false;
    for (int e = 0; e < 64; e++) {
      for (int i = 0; i < m; i++) {
        const double a = nu[i * st] + tau * dl[i * st];
        nun[i * st] = (i >= me && a < 0.0) ? 0.0 : a;
      }
      const double qn = bbh_poly_point(Q, p, nun, x, st, &freen);
      phin = bbh_poly_residuals(Q, x, p, nun, true, rho, st);
      double qnf = qn;
      for (int i = 0; i < m; i++) qnf = qnf - nun[i * st] * rho[i * st];
      evals++;
      if (qnf > best_q) {
        best_q = qnf;
        best_tau = tau;
        // a damped step, or one through the region where every coordinate is clipped (q is linear there), is doubled while q rises
        if (mu <= Q.mu_min && freem) break;
        tau = tau * 2.0;
        continue;
      }
      // near the end (residuals within 1e6 tolerances) the differences of q are those of its rounding - x - p is a difference of
      // numbers of the size of p - and say nothing any more: there the KKT measure decides
      if (best_tau == 0.0 && phin < phi && (phi < 1e6 || qnf >= qf - 64.0 * 2.220446049250313e-16 * (fabs(qn) + fabs(qf)))) {
        best_tau = tau;
        by_measure = true;
      }
      break;
    }
    if (best_tau == 0.0) {  // no rise: a larger regulariser, from the point and the residuals of nu (the same bits as before)
      bbh_poly_point(Q, p, nu, x, st, &freem);
      bbh_poly_residuals(Q, x, p, nu, true, rho, st);
      mu = mu < 1e6 * Q.mu_min ? 1e6 * Q.mu_min : mu * 10.0;
      if (mu > 1e20 * Q.mu_min) break;  // not even a gradient step rises and the KKT measure is not met: status 1
      continue;
    }
    for (int i = 0; i < m; i++) {
      const double a = nu[i * st] + best_tau * dl[i * st];
      nu[i * st] = (i >= me && a < 0.0) ? 0.0 : a;
    }
    if (best_tau == tau && (by_measure || (mu <= Q.mu_min && freem))) {  // (x and rho are those of the kept trial)
      q = best_q;
      for (int i = 0; i < m; i++) q = q + nu[i * st] * rho[i * st];
      if (by_measure) q = bbh_poly_point(Q, p, nu, x, st, &freen);
      phi = phin;
      freem = freen;
    } else {
      q = bbh_poly_point(Q, p, nu, x, st, &freem);
      phi = bbh_poly_residuals(Q, x, p, nu, true, rho, st);
    }
    mu = fmax(Q.mu_min, mu * 0.1);
    converged = phi <= 1.0;
  }
  // refinement on the face: the residuals at the scale of x
  int status = converged ? 0 : 1;
  if (converged) {
    status = 1;
    for (int pass = 0; pass < 4; pass++) {
      if (bbh_poly_residuals(Q, x, p, nu, false, rho, st) <= 1.0) {
        status = 0;
        break;
      }
      uint32_t work = 0, fm = 0;
      for (int i = 0; i < m; i++) {
        if (i < me || nu[i * st] > 0.0 || rho[i * st] < 0.0) work |= 1u << i;
        nun[i * st] = rho[i * st];
      }
      for (int k = 0; k < dc; k++)
        if (x[k * st] > Q.lo[k] && x[k * st] < Q.hi[k]) fm |= 1u << k;
      bbh_poly_solve(Q, work, fm, Q.mu_min, H, nun, st);
      for (int k = 0; k < dc; k++) {
        if (!(fm >> k & 1u)) continue;
        double acc = 0.0;
        for (int i = 0; i < m; i++) acc = acc + Q.R[(size_t)i * dc + k] * nun[i * st];
        const double z = x[k * st] - acc;
        x[k * st] = z < Q.lo[k] ? Q.lo[k] : (z > Q.hi[k] ? Q.hi[k] : z);
      }
    }
    if (status) status = bbh_poly_residuals(Q, x, p, nu, false, rho, st) <= 1.0 ? 0 : 1;
  }
  for (int k = 0; k < dc; k++) out[k] = x[k * st];
  return status;
}
