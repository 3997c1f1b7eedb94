// Linear constraints of a continuous subspace on the device: uniform samples of the polytope and Euclidean projections onto it.
//   { c in R^dc : lo <= c <= hi, E c = e, G c >= g },  dc <= 32, me + mi <= 16 rows.
// bbh_polytope_sample replaces BoTorch's get_polytope_samples (baybe/searchspace/continuous.py:544-571): one independent
// hit-and-run chain per sample instead of one long sequential chain.  bbh_polytope_project stands where maximize_box clips: one
// small quadratic programme per start and trial.  The per-chain and per-point bodies are in bbh_polytope_core.h.
//
// Layout (both kernels): one thread per chain / per point, the thread's run-time indexed state ([dz] coordinates and direction;
// multipliers, residuals, point and the packed Hessian) in LDS at [index][thread], so that a wave's 64 accesses to one index fall
// into consecutive banks; in a per-thread array they would go to scratch.  The rows of the set are the same for every thread:
// they are staged once per workgroup and read as LDS broadcasts.
#include "bbh_common.h"
#include "bbh_polytope_core.h"

#pragma clang fp contract(off)

#define POLY_SAMPLE_TB 64

// cst: Z [dc dz], GZ [mi dz], c0, lo, hi, bl, bu [dc each], bg [mi]
__global__ __launch_bounds__(POLY_SAMPLE_TB) void bbh_polytope_sample_kernel(const double* __restrict__ cst, int dc, int dz, int mi,
                                                                              int64_t R, int T, uint64_t seed, double* __restrict__ out) {
  extern __shared__ double poly_sm[];
  const int nc = dc * dz + mi * dz + 5 * dc + mi;
  for (int i = threadIdx.x; i < nc; i += POLY_SAMPLE_TB) poly_sm[i] = cst[i];
  __syncthreads();
  const int64_t chain = (int64_t)blockIdx.x * POLY_SAMPLE_TB + threadIdx.x;
  if (chain >= R) return;  // (no barrier below)
  bbh_poly_reduced P;
  P.Z = poly_sm;
  P.GZ = P.Z + dc * dz;
  P.c0 = P.GZ + mi * dz;
  P.lo = P.c0 + dc;
  P.hi = P.lo + dc;
  P.bl = P.hi + dc;
  P.bu = P.bl + dc;
  P.bg = P.bu + dc;
  P.dc = dc;
  P.dz = dz;
  P.mi = mi;
  double* y = poly_sm + nc + threadIdx.x;
  double* d = y + dz * POLY_SAMPLE_TB;
  bbh_poly_chain(P, seed, (uint64_t)chain, T, y, d, POLY_SAMPLE_TB, out + chain * dc);
}

// cst: R [m dc], t [m], lo [dc], hi [dc]
__global__ void bbh_polytope_project_kernel(const double* __restrict__ cst, int dc, int me, int mi, double tolf, double mu_min,
                                            const double* __restrict__ P, int64_t k, int64_t ldp, double* __restrict__ out,
                                            int32_t* __restrict__ status) {
  extern __shared__ double poly_sm[];
  const int m = me + mi, tb = blockDim.x;
  const int nc = m * dc + m + 2 * dc;
  for (int i = threadIdx.x; i < nc; i += tb) poly_sm[i] = cst[i];
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * tb + threadIdx.x;
  if (r >= k) return;  // (no barrier below)
  bbh_poly_rows Q;
  Q.R = poly_sm;
  Q.t = Q.R + m * dc;
  Q.lo = Q.t + m;
  Q.hi = Q.lo + dc;
  Q.dc = dc;
  Q.me = me;
  Q.mi = mi;
  Q.tolf = tolf;
  Q.mu_min = mu_min;
  status[r] = bbh_poly_project(Q, P + r * ldp, poly_sm + nc + threadIdx.x, tb, out + r * dc);
}

static int poly_upload(bbh_handle* h, const std::vector<double>& cst) {
  int rc = bbh_ensure_ws(h, sizeof(double) * cst.size());
  if (rc) return rc;
  BBH_HIP_TRY(h, hipMemcpyAsync(h->d_ws, cst.data(), sizeof(double) * cst.size(), hipMemcpyHostToDevice, h->stream));
  return 0;
}

extern "C" int bbh_polytope_sample(bbh_handle* h, int32_t dc, int32_t dz, int32_t mi, const double* Z_host, const double* GZ_host,
                                   const double* c0_host, const double* lo_host, const double* hi_host, const double* bl_host,
                                   const double* bu_host, const double* bg_host, int64_t R, int32_t T, uint64_t seed, double* out_dev) {
  if (!h) return -1;
  if (dc < 1 || dc > BBH_POLY_MAX_DC || dz < 1 || dz > dc || mi < 0 || mi > BBH_POLY_MAX_ROWS) {
    h->err = "bbh_polytope_sample: 1 <= dz <= dc <= 32 columns and 0 <= mi <= 16 inequality rows";
    return -1;
  }
  if (R < 0 || R > (int64_t)INT_MAX || T < 1 || !Z_host || !c0_host || !lo_host || !hi_host || !bl_host || !bu_host ||
      (mi > 0 && (!GZ_host || !bg_host)) || (R > 0 && !out_dev)) {
    h->err = "bbh_polytope_sample: bad arguments (need 0 <= R < 2^31 chains, T >= 1 steps, the reduced set and out [R, dc])";
    return -1;
  }
  if (R == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  std::vector<double> cst;
  cst.insert(cst.end(), Z_host, Z_host + (size_t)dc * dz);
  if (mi) cst.insert(cst.end(), GZ_host, GZ_host + (size_t)mi * dz);
  for (const double* v : {c0_host, lo_host, hi_host, bl_host, bu_host}) cst.insert(cst.end(), v, v + dc);
  if (mi) cst.insert(cst.end(), bg_host, bg_host + mi);
  int rc = poly_upload(h, cst);
  if (rc) return rc;
  const size_t lds = sizeof(double) * (cst.size() + 2 * (size_t)dz * POLY_SAMPLE_TB);  // at most (1024 + 512 + 176 + 4096) 8 = 46 464 bytes
  hipLaunchKernelGGL(bbh_polytope_sample_kernel, dim3((unsigned)((R + POLY_SAMPLE_TB - 1) / POLY_SAMPLE_TB)), dim3(POLY_SAMPLE_TB), lds,
                     h->stream, h->d_ws, (int)dc, (int)dz, (int)mi, R, (int)T, seed, out_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  BBH_HIP_TRY(h, hipStreamSynchronize(h->stream));  // (the staging vector is pageable and dies with this call)
  return 0;
}

extern "C" int bbh_polytope_project(bbh_handle* h, int32_t dc, int32_t me, int32_t mi, const double* R_host, const double* t_host,
                                    const double* lo_host, const double* hi_host, double tolf, double mu_min, const double* P_dev, int64_t k,
                                    int64_t ldp, double* out_dev, int32_t* status_dev) {
  if (!h) return -1;
  const int m = me + mi;
  if (dc < 1 || dc > BBH_POLY_MAX_DC || me < 0 || mi < 0 || m > BBH_POLY_MAX_ROWS) {
    h->err = "bbh_polytope_project: 1 <= dc <= 32 columns and me + mi <= 16 rows";
    return -1;
  }
  if (k < 0 || k > (int64_t)INT_MAX || ldp < dc || !lo_host || !hi_host || (m > 0 && (!R_host || !t_host)) || !(tolf > 0.0) ||
      !(mu_min > 0.0) || (k > 0 && (!P_dev || !out_dev || !status_dev))) {
    h->err = "bbh_polytope_project: bad arguments (need 0 <= k < 2^31 rows, ldp >= dc, the rows, tolf > 0, mu_min > 0, out [k, dc], status [k])";
    return -1;
  }
  for (int c = 0; c < dc; c++)
    if (!(lo_host[c] <= hi_host[c])) {
      h->err = "bbh_polytope_project: lo <= hi in every column";
      return -1;
    }
  if (k == 0) return 0;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  std::vector<double> cst;
  if (m) cst.insert(cst.end(), R_host, R_host + (size_t)m * dc);
  if (m) cst.insert(cst.end(), t_host, t_host + m);
  cst.insert(cst.end(), lo_host, lo_host + dc);
  cst.insert(cst.end(), hi_host, hi_host + dc);
  int rc = poly_upload(h, cst);
  if (rc) return rc;
  // a wave per workgroup where its state fits the 64 KB every launch may ask for, half a wave otherwise (m >= 11 at dc = 32)
  const size_t per_thread = BBH_POLY_STATE((size_t)m, (size_t)dc);
  int tb = 64;
  if (sizeof(double) * (cst.size() + per_thread * tb) > 65536) tb = 32;
  const size_t lds = sizeof(double) * (cst.size() + per_thread * tb);  // at most (592 + 216 * 32) 8 = 60 032 bytes
  hipLaunchKernelGGL(bbh_polytope_project_kernel, dim3((unsigned)((k + tb - 1) / tb)), dim3(tb), lds, h->stream, h->d_ws, (int)dc, (int)me,
                     (int)mi, tolf, mu_min, P_dev, k, ldp, out_dev, status_dev);
  BBH_HIP_TRY(h, hipGetLastError());
  BBH_HIP_TRY(h, hipStreamSynchronize(h->stream));  // (the staging vector is pageable and dies with this call)
  return 0;
}
