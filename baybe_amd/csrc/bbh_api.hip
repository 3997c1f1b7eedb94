// C-ABI entry points that are not tied to one kernel family: lifecycle, posterior dispatch,
// MFMA layout self-test, instrumentation.  See include/baybe_hip.h for the contract.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>

#include "bbh_common.h"

static const char* kNoHandle = "bbh: null handle";

extern "C" int bbh_version(void) { return 100; }

// Every run-time switch of the library, read from the environment when a handle is created (the handle pool of engine.py keys its
// handles by the BBH_* environment for that reason).  One row per switch and member; KERNELS.md section 4.5 documents the same names.
static bbh_switches bbh_read_switches() {
  enum how { NOT, IS, SET, INT, MB };  // value[0] != c | value[0] == c | variable present | atoi(value) | atoll(value) clamped to [1, INT_MAX]
  typedef bbh_switches S;
  static const struct {
    const char* name;
    how parse;
    char c;
    bool S::*flag;
    int S::*num;
  } table[] = {
      {"BBH_PIPELINE", NOT, '0', &S::use_pipeline, nullptr},
      {"BBH_MEAN_VALU", NOT, '0', &S::use_mean_valu, nullptr},
      {"BBH_KVCACHE", NOT, '0', &S::use_kvcache, nullptr},
      {"BBH_KV_GLOBAL", NOT, '0', nullptr, &S::kv_global_mode},
      {"BBH_KV_LDS", INT, 0, nullptr, &S::kv_lds_blocks},
      {"BBH_COOP", INT, 0, nullptr, &S::coop_mode},
      {"BBH_COOP_SMALL", NOT, '0', &S::coop_small, nullptr},
      {"BBH_COOP_SEED", NOT, '0', &S::coop_seed, nullptr},
      {"BBH_COOPG_CROSS", NOT, '0', &S::coopg_cross_on, nullptr},
      {"BBH_SMALL", NOT, '0', &S::small_on, nullptr},
      {"BBH_SMALL_FORCE", IS, '1', &S::small_force, nullptr},
      {"BBH_COLUMNS_COOP", NOT, '0', &S::columns_coop, nullptr},
      {"BBH_COLUMNS_NT", INT, 0, nullptr, &S::columns_nt},
      {"BBH_PENDING_LDS", NOT, '0', &S::pending_lds_form, nullptr},
      {"BBH_PENDING_SLICES", INT, 0, nullptr, &S::pending_slices},
      {"BBH_QBIG_WS_MB", MB, 0, nullptr, &S::qbig_ws_mb},
      {"BBH_Q1_SLICED", NOT, '0', &S::q1_sliced, nullptr},
      {"BBH_NEHVI_LOG", IS, '1', &S::nehvi_log, nullptr},
      {"BBH_NEHVI_SLICES", INT, 0, nullptr, &S::nehvi_slices},
      {"BBH_NEHVI_PK", NOT, '0', &S::nehvi_pk, nullptr},
      {"BBH_EHVI_SLICE", INT, 0, nullptr, &S::ehvi_slice},
      {"BBH_NIPV_TILE", INT, 0, nullptr, &S::nipv_tile},
      {"BBH_NIPV_SLICE", INT, 0, nullptr, &S::nipv_slice},
      {"BBH_SHAP_CPT", INT, 0, nullptr, &S::shap_cpt},
      {"BBH_NEI_FUSED", NOT, '0', &S::nei_fused, nullptr},
      {"BBH_SELECT", NOT, '0', &S::select_on, nullptr},
      {"BBH_SELECT_MAPPED", NOT, '0', &S::select_mapped, nullptr},
      {"BBH_FIT_GRAPH", NOT, '0', &S::fit_graph_mode, nullptr},
      {"BBH_FIT_OVERLAP", NOT, '0', &S::fit_overlap, nullptr},
      {"BBH_FIT_SMALL", NOT, '0', &S::fit_small, nullptr},
      {"BBH_FIT_FLOW", INT, 0, nullptr, &S::fit_flow},
      {"BBH_FLOW_SPIN", INT, 0, nullptr, &S::flow_spin_limit},
      {"BBH_FIT_POST1", NOT, '0', &S::fit_post1, nullptr},
      {"BBH_FIT_TAIL1", NOT, '0', &S::fit_tail1, nullptr},
      {"BBH_POTRF_TILES", NOT, '0', &S::potrf_tiles, nullptr},
      {"BBH_POTRF_REG", NOT, '0', &S::potrf_register_form, nullptr},
      {"BBH_TILE_SPIN", INT, 0, nullptr, &S::tile_spin_limit},
      {"BBH_TILE_ACQ", IS, '0', &S::tile_d_sc1, nullptr},  // (default: acquire fence)
      {"BBH_TILE_WT", NOT, '0', &S::tile_wt, nullptr},
      {"BBH_TILE_MT", NOT, '0', &S::tile_mt, nullptr},
      {"BBH_TILE_MT", IS, 'p', &S::tile_mt_partial, nullptr},
      {"BBH_TILE_GRAM", NOT, '0', &S::tile_gram, nullptr},
      {"BBH_TILE_GRAM_THETA", IS, 'c', &S::tile_gram_theta_copy, nullptr},
      {"BBH_SETMODEL_UPLOAD", IS, 'c', &S::setmodel_upload_copy, nullptr},
      {"BBH_SETMODEL_SYNC", NOT, '0', &S::setmodel_sync, nullptr},
      {"BBH_SETMODEL_SYNC", IS, 'p', &S::setmodel_sync_poll, nullptr},
      {"BBH_SETMODEL_TRACE", SET, 0, &S::setmodel_trace, nullptr},
      {"BBH_SETMODEL_TRACE", IS, '2', &S::setmodel_trace_quiet, nullptr},
      {"BBH_FIT_TRACE", SET, 0, &S::fit_trace, nullptr},
      {"BBH_TILE_TRACE", SET, 0, &S::tile_trace, nullptr},
      {"BBH_FLOW_TRACE", SET, 0, &S::flow_trace, nullptr},
      {"BBH_TILE_STAMPS", SET, 0, &S::tile_stamps, nullptr},
  };
  bbh_switches sw;
  for (const auto& row : table) {
    const char* e = getenv(row.name);
    if (!e) continue;
    long long v = 1;  // SET
    if (row.parse == NOT) v = e[0] != row.c;
    if (row.parse == IS) v = e[0] == row.c;
    if (row.parse == INT) v = atoi(e);
    if (row.parse == MB) v = std::min<long long>(std::max(1LL, atoll(e)), INT_MAX);
    if (row.flag) sw.*row.flag = v != 0;
    if (row.num) sw.*row.num = (int)v;
  }
  return sw;
}

hipError_t bbh_allow_lds(int device, const void* kernel, size_t bytes) {
  if (bytes <= BBH_LDS_DEFAULT_LIMIT) return hipSuccess;
  hipError_t e = device < 0 ? hipGetDevice(&device) : hipSuccess;
  if (e != hipSuccess) return e;
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> granted;  // (kernel, device) -> bytes
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = granted[{kernel, device}];
  if (bytes <= have) return hipSuccess;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) have = bytes;
  return e;
}

extern "C" int bbh_create(int device_id, bbh_handle** out) {
  if (!out) return -1;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return -10;  // no HIP device: fail loudly
  if (device_id < 0 || device_id >= count) return -11;
  if (hipSetDevice(device_id) != hipSuccess) return -12;
  bbh_handle* h = new bbh_handle();
  h->device = device_id;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) h->num_cu = cus;
  }
  {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device_id) == hipSuccess && v > 0) h->lds_per_block = (size_t)v;
  }
  h->sw = bbh_read_switches();
  *out = h;
  return 0;
}

extern "C" int bbh_destroy(bbh_handle* h) {
  if (!h) return -1;
  hipSetDevice(h->device);
  if (h->stream)
    hipStreamSynchronize(h->stream);
  else
    hipDeviceSynchronize();
  for (auto& sp : h->pending_events) {
    hipEventDestroy(sp.e0);
    hipEventDestroy(sp.e1);
  }
  bbh_comm_destroy(h);
  bbh_select_destroy(h);
  bbh_nehvi_destroy(h);
  bbh_sobol_destroy(h);
  bbh_fps_destroy(h);
  bbh_flow_destroy(h);
  bbh_postgrad_destroy(h);
  bbh_nipv_destroy(h);
  bbh_free_model_public(h);
  if (h->d_ws) hipFree(h->d_ws);
  if (h->fit_stream) {
    hipStreamSynchronize(h->fit_stream);
    hipStreamDestroy(h->fit_stream);
  }
  if (h->side_stream) {
    hipStreamSynchronize(h->side_stream);
    hipStreamDestroy(h->side_stream);
  }
  for (auto& e : h->side_events)
    if (e) hipEventDestroy(e);
  if (h->d_rstream) hipFree(h->d_rstream);
  if (h->d_rsmall) hipFree(h->d_rsmall);
  if (h->d_tileflags) hipFree(h->d_tileflags);
  if (h->d_kvcache) hipFree(h->d_kvcache);
  if (h->d_slab_flags) hipFree(h->d_slab_flags);
  if (h->d_z) hipFree(h->d_z);
  if (h->h_zstage) hipHostFree(h->h_zstage);
  if (h->z_evt) hipEventDestroy(h->z_evt);
  if (h->d_red) hipFree(h->d_red);
  if (h->d_redi) hipFree(h->d_redi);
  delete h;
  return 0;
}

extern "C" const char* bbh_last_error(bbh_handle* h) { return h ? h->err.c_str() : kNoHandle; }

extern "C" int bbh_set_stream(bbh_handle* h, void* hip_stream) {
  if (!h) return -1;
  h->stream = (hipStream_t)hip_stream;
  return 0;
}

// ---- MFMA fragment-layout self-test ---------------------------------------------------------
// C = A B with asymmetric integer-valued A (16x8) and B (8x16): catches row/col swaps and the
// f32-style C mapping (which misplaces 3 of every 4 rows on the f64 instruction).
__global__ void bbh_selftest_kernel(const double* A, const double* B, double* C) {
  const int l = threadIdx.x;
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int ks = 0; ks < 2; ks++) {
    const double a = A[(l & 15) * 8 + 4 * ks + (l >> 4)];
    const double b = B[(4 * ks + (l >> 4)) * 16 + (l & 15)];
    acc = mfma_f64(a, b, acc);
  }
  for (int r = 0; r < 4; r++) C[((l >> 4) + 4 * r) * 16 + (l & 15)] = acc[r];
}

extern "C" int bbh_selftest(bbh_handle* h) {
  if (!h) return -1;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  double hA[16 * 8], hB[8 * 16], hC[256], ref[256];
  for (int i = 0; i < 16; i++)
    for (int k = 0; k < 8; k++) hA[i * 8 + k] = (double)(3 * i + 7 * k + 1) - 0.5 * (double)(i * k);
  for (int k = 0; k < 8; k++)
    for (int j = 0; j < 16; j++) hB[k * 16 + j] = (double)(5 * k - 2 * j) + 0.25 * (double)(k * j + j);
  for (int i = 0; i < 16; i++)
    for (int j = 0; j < 16; j++) {
      double s = 0.0;
      for (int k = 0; k < 8; k++) s += hA[i * 8 + k] * hB[k * 16 + j];
      ref[i * 16 + j] = s;
    }
  int rc = bbh_ensure_ws(h, sizeof(double) * 1024);
  if (rc) return rc;
  double* dA = h->d_ws;
  double* dB = dA + 128;
  double* dC = dB + 128;
  BBH_HIP_TRY(h, hipMemcpyAsync(dA, hA, sizeof(hA), hipMemcpyHostToDevice, h->stream));
  BBH_HIP_TRY(h, hipMemcpyAsync(dB, hB, sizeof(hB), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(bbh_selftest_kernel, dim3(1), dim3(64), 0, h->stream, dA, dB, dC);
  BBH_HIP_TRY(h, hipMemcpyAsync(hC, dC, sizeof(hC), hipMemcpyDeviceToHost, h->stream));
  BBH_HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int e = 0; e < 256; e++)
    if (fabs(hC[e] - ref[e]) > 1e-9 * (1.0 + fabs(ref[e]))) {
      h->err = "bbh_selftest: v_mfma_f64_16x16x4_f64 fragment layout mismatch at element " + std::to_string(e);
      return -20;
    }
  return 0;
}

// ---- posterior ------------------------------------------------------------------------------
static int check_post_args(bbh_handle* h, const double* X_dev, int64_t N, int64_t ldx) {
  if (!h->factorized) {
    h->err = "posterior requested before bbh_factorize";
    return -1;
  }
  if (N < 0 || (N > 0 && !X_dev) || ldx < h->desc.d) {
    h->err = "posterior: bad arguments (need ldx >= d)";
    return -1;
  }
  if (h->dn > 126) {
    h->err = "fused posterior supports at most 126 numerical columns";
    return -1;
  }
  return 0;
}

extern "C" int bbh_posterior(bbh_handle* h, const double* X_dev, int64_t N, int64_t ldx, double* mean_dev,
                             double* var_dev) {
  if (!h) return -1;
  int rc = check_post_args(h, X_dev, N, ldx);
  if (rc) return rc;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  return bbh_launch_fused(h, X_dev, N, ldx, mean_dev, var_dev, nullptr, true);
}

extern "C" int bbh_posterior_unfused(bbh_handle* h, const double* X_dev, int64_t N, int64_t ldx, double* mean_dev,
                                     double* var_dev) {
  if (!h) return -1;
  int rc = check_post_args(h, X_dev, N, ldx);
  if (rc) return rc;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  return bbh_launch_unfused(h, X_dev, N, ldx, mean_dev, var_dev);
}

extern "C" int bbh_cross_cov(bbh_handle* h, const double* X_dev, int64_t N, int64_t ldx, double* cross_dev) {
  if (!h) return -1;
  int rc = check_post_args(h, X_dev, N, ldx);
  if (rc) return rc;
  if (h->p < 1 || !cross_dev) {
    h->err = "bbh_cross_cov: no pending points set";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  return bbh_launch_fused(h, X_dev, N, ldx, nullptr, nullptr, cross_dev, false);
}

extern "C" int bbh_train_posterior_mean(bbh_handle* h, double* mean_host) {
  if (!h) return -1;
  if (!h->factorized || !mean_host) {
    h->err = "bbh_train_posterior_mean: model not factorised";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  const int64_t n = h->n, d = h->desc.d;
  int rc = 0;
  double* own = nullptr;  // composite kernels: the posterior path uses the workspace itself
  if (bbh_materialised_only(h))
    BBH_HIP_TRY(h, hipMalloc((void**)&own, sizeof(double) * (size_t)(n * d + n)));
  else if ((rc = bbh_ensure_ws(h, sizeof(double) * (size_t)(n * d + n))))
    return rc;
  double* dX = own ? own : h->d_ws;
  double* dm = dX + n * d;
  hipError_t e = hipMemcpyAsync(dX, h->xraw_host.data(), sizeof(double) * n * d, hipMemcpyHostToDevice, h->stream);
  // pending columns do not affect column 0 (the mean), but keep the call side-effect free
  if (e == hipSuccess) rc = bbh_launch_fused(h, dX, n, d, dm, nullptr, nullptr, false);
  if (e == hipSuccess && !rc) e = hipMemcpyAsync(mean_host, dm, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (own) hipFree(own);
  if (rc) return rc;
  BBH_HIP_TRY(h, e);
  return 0;
}

extern "C" int bbh_set_slice_rows(bbh_handle* h, int64_t rows) {
  if (!h || rows < 0) return -1;
  h->slice_rows = rows;
  return 0;
}

// Idle handles are kept in a pool by the host side (engine.py); their grow-only buffers would pin HBM for as long as they sit there.
// Everything above keep_bytes goes: the scratch workspace, the global kernel-value cache, and the model (its buffers are re-created by
// the next bbh_set_model) when its matrices exceed the bound.  Small campaign models - what the pool is for - keep everything.
extern "C" int bbh_trim(bbh_handle* h, int64_t keep_bytes) {
  if (!h || keep_bytes < 0) return -1;
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  BBH_HIP_TRY(h, hipStreamSynchronize(h->stream));
  bbh_fps_reset(h);
  if (h->d_ws && h->ws_bytes > (size_t)keep_bytes) {
    hipFree(h->d_ws);
    h->d_ws = nullptr;
    h->ws_bytes = 0;
  }
  if (h->d_kvcache && h->kvcache_bytes > (size_t)keep_bytes) {
    hipFree(h->d_kvcache);
    h->d_kvcache = nullptr;
    h->kvcache_bytes = 0;
  }
  if (bbh_nipv_resident_bytes(h) > (size_t)keep_bytes) bbh_nipv_destroy(h);
  if (h->have_model && sizeof(double) * (size_t)h->np * (size_t)h->np * 6 > (size_t)keep_bytes) bbh_free_model_public(h);
  return 0;
}

// ---- instrumentation ------------------------------------------------------------------------
extern "C" int bbh_last_posterior_form(bbh_handle* h) { return h ? h->last_form : -1; }
extern "C" int bbh_last_posterior_seeded(bbh_handle* h) { return h ? (h->last_form == 1 && h->last_seeded) : -1; }
extern "C" int bbh_last_fit_form(bbh_handle* h) { return h ? h->last_fit_form : -1; }
extern "C" int bbh_last_factor_form(bbh_handle* h) { return h ? h->last_factor_form : -1; }

extern "C" int bbh_timing_enable(bbh_handle* h, int enable) {
  if (!h) return -1;
  h->timing = enable < 0 ? 0 : enable;  // 1: all families; 2 * mask: the families whose bit is set (events between kernels cost ~5 us each)
  return 0;
}

extern "C" int bbh_timing_read_family(bbh_handle* h, int32_t family, double* ms_total, int64_t* launches, int reset) {
  if (!h) return -1;
  if (family < 0 || family >= BBH_TIMED_FAMILIES) {
    h->err = "bbh_timing_read_family: unknown kernel family";
    return -1;
  }
  BBH_HIP_TRY(h, hipSetDevice(h->device));
  for (auto& sp : h->pending_events) {
    BBH_HIP_TRY(h, hipEventSynchronize(sp.e1));
    float ms = 0.f;
    BBH_HIP_TRY(h, hipEventElapsedTime(&ms, sp.e0, sp.e1));
    h->timed_ms[sp.family] += (double)ms;
    h->timed_launches[sp.family] += 1;
    hipEventDestroy(sp.e0);
    hipEventDestroy(sp.e1);
  }
  h->pending_events.clear();
  if (ms_total) *ms_total = h->timed_ms[family];
  if (launches) *launches = h->timed_launches[family];
  if (reset) {
    h->timed_ms[family] = 0.0;
    h->timed_launches[family] = 0;
  }
  return 0;
}

extern "C" int bbh_timing_read(bbh_handle* h, double* fused_ms_total, int64_t* fused_launches, int reset) {
  return bbh_timing_read_family(h, BBH_TIMED_POSTERIOR, fused_ms_total, fused_launches, reset);
}
