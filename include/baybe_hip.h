/*
 * baybe_hip.h — C-ABI of libbaybe_hip.so, the MI355X (gfx950) implementation of
 * BayBE's GP-surrogate recommend() hot path.
 *
 * The reference (emdgroup/baybe) is pure Python; it has no FFI of its own.  Each
 * entry point below replaces the *third-party call* BayBE makes at the cited
 * line (botorch / gpytorch, CPU), so that a ctypes stub at that call site is
 * the whole integration:
 *
 *   bbh_set_model            botorch.models.SingleTaskGP(...)            baybe/surrogates/gaussian_process/core.py:331-339
 *                            Normalize / Standardize                     baybe/surrogates/gaussian_process/core.py:301-306
 *   bbh_fit_value_grad       one closure call of fit_gpytorch_mll        baybe/surrogates/gaussian_process/core.py:340-341
 *                            (ExactMLL / LOO-PL value + gradient)        baybe/surrogates/gaussian_process/components/fit_criterion.py:31-41
 *   bbh_factorize            prediction-strategy caches (L, alpha, L^-T) baybe/surrogates/gaussian_process/core.py:268-269 (first posterior call)
 *   bbh_posterior            model.posterior(X) for N q=1 t-batches      baybe/surrogates/base.py:249-272, 308-384
 *   bbh_train_posterior_mean posterior mean at the training inputs       baybe/acquisition/_builder.py:141-161 (best_f, 256-265)
 *   bbh_qlogei_q1            qLogExpectedImprovement.forward, q'=1       baybe/acquisition/acqfs.py:219-223; baybe/acquisition/base.py:112-159
 *   bbh_pending_set /        set_X_pending + joint q'-batch posterior    baybe/acquisition/_builder.py:326-334
 *   bbh_cross_cov /
 *   bbh_qlogei_pending       qLogEI forward with pending points
 *   bbh_argmax               the argmax of optimize_acqf_discrete        baybe/recommenders/pure/bayesian/botorch/discrete.py:120-126
 *   bbh_set_model_ex /       ModelListGP member conditioned on sampled   baybe/surrogates/composite.py:125-134;
 *   bbh_posterior_joint /    baseline values (joint draw of f(X) with    baybe/acquisition/_builder.py:319-324 (X_baseline)
 *   bbh_set_mean_columns /   f(X_baseline), cached Cholesky root)
 *   bbh_posterior_columns(_sm)
 *   bbh_qlognehvi(_sm)       qLogNoisyExpectedHypervolumeImprovement     baybe/acquisition/acqfs.py:477-484
 *   bbh_score_nei /          qNoisyExpectedImprovement and               baybe/acquisition/acqfs.py:226-243;
 *   bbh_nei_q1 /             qLogNoisyExpectedImprovement, q' = 1, with  baybe/acquisition/_builder.py:319-324 (X_baseline,
 *   bbh_sample_best_dev /    prune_inferior_points                       prune_baseline)
 *   bbh_best_frequency_dev
 *   bbh_nparego_q1 /         qLogNParEGO, q' = 1 (Chebyshev scalarisation baybe/acquisition/acqfs.py:328-336
 *   bbh_scalarized_best(_frequency)_dev  of the targets under qLogNEI)
 *   bbh_qnehvi_cells / _sm   qNoisyExpectedHypervolumeImprovement        baybe/acquisition/acqfs.py:467-474
 *
 * Conventions
 *  - extern "C"; every function returns 0 on success, <0 on error;
 *    bbh_last_error(h) returns a message owned by the library (valid until the
 *    next call on that handle).
 *  - "_dev" arguments are DEVICE pointers (row-major, contiguous, fp64 unless
 *    noted) owned by the caller (e.g. torch.Tensor.data_ptr() of a ROCm tensor
 *    used purely as a container).  "_host" arguments are HOST pointers; they are
 *    O(n*d) model data or O(S*q) base samples and are copied by the call.
 *  - All work is enqueued on the handle's stream (bbh_set_stream; default: the
 *    legacy null stream).  Calls that return host data synchronise that stream.
 *  - One handle = one single-output GP on one device.  Not thread-safe per
 *    handle; distinct handles are independent.
 *  - No CPU fallback exists: without a HIP device bbh_create fails.
 */
#ifndef BAYBE_HIP_H
#define BAYBE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bbh_handle bbh_handle;

enum bbh_kernel_kind {
  BBH_KERNEL_MATERN12 = 0,
  BBH_KERNEL_MATERN32 = 1,
  BBH_KERNEL_MATERN52 = 2, /* BayBE default: presets/baybe.py:100-107 */
  BBH_KERNEL_RBF = 3,
  /* gpytorch PiecewisePolynomialKernel(q), baybe/kernels/basic.py:114-131: (1 - r)_+^(j + q) P_q(r), j = floor(dn / 2) + q + 1.
   * Compact support; evaluated through the materialised-K* posterior path (like composite kernels). */
  BBH_KERNEL_PIECEWISE0 = 4,
  BBH_KERNEL_PIECEWISE1 = 5,
  BBH_KERNEL_PIECEWISE2 = 6,
  BBH_KERNEL_PIECEWISE3 = 7,
  /* gpytorch RQKernel, baybe/kernels/basic.py:202-216: (1 + r^2 / (2 alpha))^-alpha with a learnable alpha per kernel
   * (theta: one slot per factor at the very end, present when any factor is an RQ kernel). */
  BBH_KERNEL_RQ = 8,
  /* Dot-product kernels (baybe/kernels/basic.py:20-46, 135-163): functions of s = sum_j x_j x'_j / w_j^2 over the normalised
   * inputs instead of a scaled squared distance; the lengthscale slots of theta carry the weights w_j (huge for columns the
   * kernel does not act on), and bbh_fit_value_grad returns d/dw_j in those slots.
   *   gpytorch LinearKernel with ARD variances v_j: k = sum_j v_j x_j x'_j, i.e. w_j = v_j^-1/2;
   *   gpytorch PolynomialKernel(power p): (x . x' + offset)^p, p = 1 .. 4, w_j = 1, offset in the factor's alpha slot
   *   (where an RQ kernel keeps its alpha).
   * k(x, x) is not constant: these kinds are evaluated through the materialised-K* posterior path only. */
  BBH_KERNEL_LINEAR = 9,
  BBH_KERNEL_POLY1 = 10,
  BBH_KERNEL_POLY2 = 11,
  BBH_KERNEL_POLY3 = 12,
  BBH_KERNEL_POLY4 = 13,
  /* gpytorch PeriodicKernel (baybe/kernels/basic.py:73-112): exp(-2 sum_j sin^2(pi (x_j - x'_j) / p_j) / l_j) with one lengthscale
   * l_j (lengthscale slots; note: not squared) and one period p_j per column.  theta: a block of F * dn periods at the very end
   * (after the alpha slots), present when any factor is periodic; slots of the other factors are ignored.  Materialised-K* path. */
  BBH_KERNEL_PERIODIC = 14,
  /* gpytorch.kernels.RFFKernel (baybe/kernels/basic.py:183-199): k(x, x') = z(x) . z(x') / D with z = [cos(x (W / l)), sin(x (W / l))], D =
   * num_samples frequencies W [dn, D] drawn once per model (bbh_set_rff_weights BEFORE bbh_set_model); the model is held in feature space:
   * fit and posterior cost O(n D^2 + D^3) and O(D^2) per candidate.  One task, single kernel, MLL, D <= 64; theta as for RBF. */
  BBH_KERNEL_RFF = 15
};

enum bbh_criterion {
  BBH_CRITERION_MLL = 0, /* gpytorch.ExactMarginalLogLikelihood   (1 task)  */
  BBH_CRITERION_LOO = 1  /* gpytorch.mlls.LeaveOneOutPseudoLikelihood (>1)  */
};

/* Architecture of the GP (what BayBE's component factories decide). */
typedef struct bbh_model_desc {
  int32_t kernel_kind;     /* enum bbh_kernel_kind                                   */
  int32_t d;               /* comp-rep columns, incl. the task column if any          */
  int32_t task_col;        /* column index of the INT-coded task parameter, -1 = none */
  int32_t n_tasks;         /* 1 = single task                                         */
  int32_t use_outputscale; /* 1 = ScaleKernel wrapper (user kernels)                   */
  int32_t criterion;       /* enum bbh_criterion                                      */
  int32_t hadamard;        /* 1 (n_tasks > 1 only) = one noise variance and one constant mean PER TASK:
                              HadamardGaussianLikelihood + HadamardConstantMean of the multi-task HVARFNER /
                              BOTORCH presets (surrogates/gaussian_process/components/_gpytorch.py:15-75)     */
  /* Composite kernels (baybe/kernels/composite.py:60-91): n_factors in 2..4 stationary factors, each with its own ARD
   * lengthscales over the numerical columns, combined as a ProductKernel (combine 0) or an AdditiveKernel (combine 1);
   * factor f may sit in its own ScaleKernel (factor_scaled[f]).  n_factors 0 / 1 = the single kernel_kind above;
   * factor_kind[0] must equal kernel_kind otherwise.  Evaluated through the materialised-K* posterior path (the fused
   * kernels are specialised for one factor). */
  int32_t n_factors;
  int32_t combine;
  int32_t factor_kind[4];
  int32_t factor_scaled[4];
  /* combine 2 = a sum whose members are products or single kernels - e.g. (Matern * Matern) + (Matern + Matern), the nested entry of the
   * reference's kernel matrix (tests/test_iterations.py:294-296): factor f multiplies into term factor_group[f] in 0..3,
   * k = sum_g prod_{f in g} os_f k_f.  Ignored for combine 0 (one term) and 1 (one factor per term). */
  int32_t factor_group[4];
} bbh_model_desc;

/*
 * Natural hyper-parameter vector "theta" (doubles), length bbh_theta_len(h):
 *   [0]            noise variance s2 (standardised target scale)
 *   [1]            constant mean c
 *   [2]            outputscale (ignored unless use_outputscale)
 *   [3 .. 3+dn)    ARD lengthscales of the dn = d - (task_col>=0) numerical columns,
 *                  in column order (normalised input scale)
 *   [3+dn .. +T*T) task covariance B[t][t'] row-major (only when n_tasks > 1)
 *   [.. +T) [.. +T) per-task noise variances, then per-task constant means (only with desc.hadamard;
 *                  slots [0] and [1] are then ignored and their gradients are 0)
 *   [.. +(F-1)*dn)  lengthscales of the factors 1 .. F-1 of a composite kernel (factor 0 uses [3 .. 3+dn))
 *   [.. +F)         per-factor outputscales (1 for an unscaled factor; its gradient slot is still filled)
 *                  k = outputscale * (prod_f | sum_f) os_f k_f(r_f) * B[t][t']
 *   [.. +F)         alpha of every factor (only when at least one factor is BBH_KERNEL_RQ; 1 for the other factors)
 * Gradients are returned in the same layout (for B: dL/dB[t][t'], accumulated
 * over ordered pairs, i.e. the matrix S with dL = sum_tt' S[t][t'] dB[t][t']).
 * Constraint transforms (softplus) and prior terms are O(d) scalar work and stay
 * with the host driver (baybe_amd/gp_spec.py, baybe_amd/engine.py).
 */

/* ---- lifecycle --------------------------------------------------------------------- */
int bbh_create(int device_id, bbh_handle** out);
int bbh_destroy(bbh_handle* h);
const char* bbh_last_error(bbh_handle* h);
int bbh_set_stream(bbh_handle* h, void* hip_stream);
/* library/ABI version: major*10000 + minor*100 + patch */
int bbh_version(void);
/* device self-test of the fp64 MFMA fragment layout the kernels rely on (0 = ok) */
int bbh_selftest(bbh_handle* h);

/* ---- model ------------------------------------------------------------------------- */
/* The random frequencies of a BBH_KERNEL_RFF model: W_host [dn, D] (numerical columns in comp-rep order x num_samples), as gpytorch's
 * RFFKernel._init_weights draws them (torch.randn(d, D)); kept on the handle for the next bbh_set_model / bbh_set_model_ex. */
int bbh_set_rff_weights(bbh_handle* h, const double* W_host, int32_t dn, int32_t D);
/* X_train_host [n,d] raw comp-rep rows; y_train_host [n] raw targets;
 * lo_host/hi_host [d] scaling bounds of every column (task column ignored).
 * Normalises the numerical columns, standardises y (Bessel std, <1e-8 -> 1). */
int bbh_set_model(bbh_handle* h, const bbh_model_desc* desc, int64_t n,
                  const double* X_train_host, const double* y_train_host,
                  const double* lo_host, const double* hi_host);
/* Same, with (a) an optional per-point noise mask [n] (0 = noise-free observation: the point is a
 * latent function value, as the sampled baseline values of qLogNEHVI are) and (b) an optional fixed
 * standardisation (use_given_std != 0: ybar/ysd are taken as given instead of computed from y). */
int bbh_set_model_ex(bbh_handle* h, const bbh_model_desc* desc, int64_t n, const double* X_train_host,
                     const double* y_train_host, const double* lo_host, const double* hi_host,
                     const uint8_t* noise_mask_host, int use_given_std, double ybar, double ysd);
int64_t bbh_theta_len(bbh_handle* h);
/* standardisation constants chosen by bbh_set_model */
int bbh_get_standardization(bbh_handle* h, double* ybar, double* ysd);

/* Data term of the fit objective and its gradient w.r.t. theta:
 *   MLL: log N(y~ | c 1, K_theta + s2 I);  LOO: sum_i log N(y~_i | mu_-i, s2_-i).
 * Returns 1 (and value=-inf) when K_theta + s2 I is not positive definite. */
int bbh_fit_value_grad(bbh_handle* h, const double* theta_host, double* value_host,
                       double* grad_host);

/* Build the prediction caches for theta: L = chol(K + s2 I) (jitter 1e-8*10^i on
 * failure, as gpytorch psd_safe_cholesky), alpha = (K + s2 I)^-1 (y~ - c), the
 * packed L^-T operand of the variance contraction.  jitter_used may be NULL. */
int bbh_factorize(bbh_handle* h, const double* theta_host, double* jitter_used);

/* ---- posterior --------------------------------------------------------------------- */
/* Marginal posterior (original target scale, no observation noise) of N candidates.
 * X_dev [N, ldx>=d] raw comp-rep rows on the device; mean_dev / var_dev [N]. */
int bbh_posterior(bbh_handle* h, const double* X_dev, int64_t N, int64_t ldx,
                  double* mean_dev, double* var_dev);
/* Same through the unfused verification path (materialised K(X*,X), generic GEMM). */
int bbh_posterior_unfused(bbh_handle* h, const double* X_dev, int64_t N, int64_t ldx,
                          double* mean_dev, double* var_dev);
/* Joint posterior (original scale, no observation noise) of q <= 4096 points given on the host:
 * mean_host [q], cov_host [q,q]. */
int bbh_posterior_joint(bbh_handle* h, const double* Xq_host, int64_t q, double* mean_host, double* cov_host);
/* Alternative target columns for the mean contraction: Y_host [n, S] (original target scale, point
 * major).  Computes alpha_s = (K + s2 M)^-1 (y~_s - c) for every column on the device.  With the
 * extended model of bbh_set_model_ex this yields, per MC sample s, the posterior mean of f(x)
 * conditioned on the sampled baseline values. */
int bbh_set_mean_columns(bbh_handle* h, const double* Y_host, int64_t S);
/* tmat_dev [N, S]: posterior mean of every candidate under each target column (original scale). */
int bbh_posterior_columns(bbh_handle* h, const double* X_dev, int64_t N, int64_t ldx, double* tmat_dev);
/* The same in SAMPLE-MAJOR layout, tmat_dev [S, N]: what bbh_qlognehvi_sm reads.  One thread of the scoring kernel owns one
 * candidate and walks the samples; with the candidate-major [N, S] layout the 64 lanes of a wave touch 64 different cache lines
 * per load (17 GB of L2 <-> fabric traffic per 1e5 x 512 x 3 pass instead of the 1.2 GB the values occupy), sample-major they
 * read 512 contiguous bytes. */
int bbh_posterior_columns_sm(bbh_handle* h, const double* X_dev, int64_t N, int64_t ldx, double* tmat_dev);
/* Posterior mean at the n training inputs -> host (for best_f). */
int bbh_train_posterior_mean(bbh_handle* h, double* mean_host);

/* ---- qLogEI ------------------------------------------------------------------------ */
/* q'=1 scores: scores[i] = logmeanexp_s log_fatplus(sign*(mean_i + sd_i z_s) - best_f; 1e-6).
 * z_host [S] Sobol-normal base samples; alive_dev [N] uint8 or NULL (0 -> score = -inf). */
int bbh_qlogei_q1(bbh_handle* h, const double* mean_dev, const double* var_dev, int64_t N,
                  const double* z_host, int64_t S, double best_f, double sign,
                  const uint8_t* alive_dev, double* scores_dev);

/* The same scores AND their k best (descending, ties -> lower index first; (-inf, -1) beyond the number of scored candidates) in
 * one call: the whole tail of a selection step of optimize_acqf_discrete (baybe/recommenders/pure/bayesian/botorch/
 * discrete.py:120-126) - scores kernel, one selection kernel whose results land in host-mapped memory, one synchronisation. */
int bbh_qlogei_q1_topk(bbh_handle* h, const double* mean_dev, const double* var_dev, int64_t N,
                       const double* z_host, int64_t S, double best_f, double sign,
                       const uint8_t* alive_dev, double* scores_dev, int64_t k, double* vals_host, int64_t* idx_host);

/* Fused scoring pass (the hot call of optimize_acqf_discrete's first greedy step): posterior AND
 * q'=1 qLogEI in one kernel.  mean_dev / var_dev may be NULL (scores only). */
int bbh_score_qlogei(bbh_handle* h, const double* X_dev, int64_t N, int64_t ldx, const double* z_host,
                     int64_t S, double best_f, double sign, const uint8_t* alive_dev, double* mean_dev,
                     double* var_dev, double* scores_dev);

/* Pending points (base pending + greedy picks), p <= BBH_MAX_PENDING.  Computes and
 * caches beta_j = (K+s2I)^-1 k(X, P_j), the pending posterior mean [p] and covariance
 * [p,p] (returned to the host if the pointers are non-NULL). */
#define BBH_MAX_PENDING 15
int bbh_pending_set(bbh_handle* h, const double* Xpend_host, int64_t p, double* mean_p_host,
                    double* cov_pp_host);
/* Posterior cross-covariance of every candidate with the pending points: cross_dev [N,p]. */
int bbh_cross_cov(bbh_handle* h, const double* X_dev, int64_t N, int64_t ldx, double* cross_dev);
/* q' = 1+p scores of the t-batches [x_i ; pending]; z_host [S, 1+p]. */
int bbh_qlogei_pending(bbh_handle* h, const double* mean_dev, const double* var_dev,
                       const double* cross_dev, int64_t N, const double* z_host, int64_t S,
                       double best_f, double sign, const uint8_t* alive_dev, double* scores_dev);

/* ---- derivatives for gradient-based continuous optimisation ----------------------------------------------------------------
 * What the reference obtains by autograd through GPyTorch inside optimize_acqf / optimize_acqf_mixed
 * (baybe/recommenders/pure/bayesian/botorch/hybrid.py:95-136, continuous.py): the posterior of N candidates AND its derivatives with
 * respect to the raw comp-rep coordinates of the dc columns cols_host (ascending, each a numerical column of the model,
 * 1 <= dc <= 32) - the chain rule through the input normalisation and the target standardisation is inside the call.  Conventions
 * of bbh_posterior / bbh_cross_cov (original target scale, no observation noise); p = the handle's pending count:
 *   mean_dev, var_dev [N], cross_dev [N, p];  dmean_dev, dvar_dev [N, dc], dcross_dev [N, p, dc]  (cross outputs may be NULL if p = 0).
 * Models: one task, one Matern-3/2 / Matern-5/2 / RBF kernel (with or without outputscale), n <= 512; anything else returns -1 and
 * bbh_last_error names the unmet condition.  Equal rows give equal bits, whatever their position and N.  Asynchronous. */
int bbh_posterior_grad(bbh_handle* h, const double* X_dev, int64_t N, int64_t ldx, const int32_t* cols_host, int32_t dc,
                       double* mean_dev, double* var_dev, double* cross_dev, double* dmean_dev, double* dvar_dev,
                       double* dcross_dev);
/* qLogEI of the t-batches [x_i ; pending] (p = 0: of x_i alone) from those statistics, scores_dev [N] as bbh_qlogei_q1 /
 * bbh_qlogei_pending, and its partial derivatives part_dev [N, 2 + p] = (dA/dmean_i, dA/dvar_i, dA/dcross_i1 .. dA/dcross_ip).
 * ok_dev [N]: 0 for a candidate whose variance is not > 0, whose joint factor needed jitter, or whose factor has a pivot below
 * 1e-8 of its diagonal entry (a copy of a pending point) - its partials are 0, its score the value the value kernels return (the
 * jittered one; NaN if no jitter level factors it).  z_host [S, 1 + p], S <= 8192.  Asynchronous. */
int bbh_qlogei_partials(bbh_handle* h, const double* mean_dev, const double* var_dev, const double* cross_dev, int64_t N,
                        const double* z_host, int64_t S, double best_f, double sign, double* scores_dev, double* part_dev,
                        uint8_t* ok_dev);

/* ---- the other acquisition functions of acqfs.py:161-290 on the same inputs ----------- */
enum bbh_acq_kind {
  BBH_ACQ_QLOGEI = 0, BBH_ACQ_QEI = 1, BBH_ACQ_QPI = 2, BBH_ACQ_QSR = 3, BBH_ACQ_QUCB = 4, BBH_ACQ_QPSTD = 5,
  BBH_ACQ_PM = 10, BBH_ACQ_PSTD = 11, BBH_ACQ_UCB = 12, BBH_ACQ_EI = 13, BBH_ACQ_LOGEI = 14, BBH_ACQ_PI = 15,
  BBH_ACQ_QNEI = 6, BBH_ACQ_QLOGNEI = 7 /* noisy expected improvement: scored by bbh_score_nei / bbh_nei_q1 only */
};
/* MC family, q'=1 and q'=1+p (mean_s max_j u(obj_sj); qPI tau = 1e-3; qUCB/qPSTD use the sample mean). */
int bbh_mc_acq_q1(bbh_handle* h, int32_t kind, const double* mean_dev, const double* var_dev, int64_t N,
                  const double* z_host, int64_t S, double best_f, double sign, double beta,
                  const uint8_t* alive_dev, double* scores_dev);
int bbh_mc_acq_pending(bbh_handle* h, int32_t kind, const double* mean_dev, const double* var_dev,
                       const double* cross_dev, int64_t N, const double* z_host, int64_t S, double best_f,
                       double sign, double beta, const uint8_t* alive_dev, double* scores_dev);
/* qLogEI of N t-batches [x_i ; pending] with the pending statistics GIVEN by the caller, 1 <= p <= 63 pending points - in
 * particular more than 15 (the reference's optimize_acqf_discrete has no cap on batch_size + pending experiments,
 * baybe/recommenders/pure/bayesian/botorch/discrete.py:120-126); p <= 15 runs the kernels of bbh_qlogei_pending (a greedy loop
 * that already holds the statistics of a superset of its picks saves the bbh_pending_set round trip per step).  The caller
 * supplies what bbh_pending_set keeps for p <= 15: cross_dev [N, p] (columns from bbh_cross_cov over chunks of <= 15 pending
 * points - a column does not depend on the other pending points), mean_p_host [p] and cov_pp_host [p, p] (bbh_posterior_joint of
 * the pending points), z_host [S, 1 + p].  The per-candidate Cholesky factors live in a global workspace of
 * (p + 1)(p + 2) / 2 x N doubles. */
int bbh_qlogei_pending_big(bbh_handle* h, const double* mean_dev, const double* var_dev, const double* cross_dev,
                           int64_t N, int64_t p, const double* mean_p_host, const double* cov_pp_host,
                           const double* z_host, int64_t S, double best_f, double sign, const uint8_t* alive_dev,
                           double* scores_dev);
/* ---- target transformations as MC objectives ------------------------------------------------------------------------------
 * The reference fits the surrogate on the raw target and applies the target's transformation per posterior sample, in front of
 * the acquisition utility (baybe/acquisition/_builder.py:211-254, baybe/objectives/base.py:130-150,
 * baybe/transformations/basic.py); a minimised target appends a negation (objectives/base.py:100-105).  An objective program is
 * that transformation as at most 8 scalar operations, applied first to last to every sample y: */
enum bbh_objective_op {
  BBH_OBJ_AFFINE = 0,   /* p0 y + p1 */
  BBH_OBJ_CLAMP = 1,    /* min(max(y, p0), p1); -inf / +inf = no bound */
  BBH_OBJ_TWOSIDED = 2, /* y < p2 ? (y - p2) p0 : (y - p2) p1 */
  BBH_OBJ_BELL = 3,     /* exp(-((y - p0) / p1)^2 / 2) */
  BBH_OBJ_LOG = 4,
  BBH_OBJ_EXP = 5,
  BBH_OBJ_POW = 6,      /* y^p0, p0 integer-valued */
  BBH_OBJ_SIGMOID = 7   /* 1 / (1 + exp(p1 (y - p0))) */
};
#define BBH_OBJ_MAX_OPS 8
typedef struct bbh_objective_prog {
  int32_t n_ops;
  int32_t op[BBH_OBJ_MAX_OPS];
  double p[BBH_OBJ_MAX_OPS][3];
} bbh_objective_prog;
/* bbh_mc_acq_q1 with g = prog(mu + sd z_s) in place of sign (mu + sd z_s): replaces the reference's
 * acqf(objective=GenericMCObjective(transformation))(X) for t-batches of one point.  kind: BBH_ACQ_QLOGEI ... BBH_ACQ_QPSTD;
 * qUCB / qPSTD use the mean of g over the samples (BoTorch's obj.mean(dim=0)). */
int bbh_mc_acq_obj_q1(bbh_handle* h, int32_t kind, const bbh_objective_prog* prog, const double* mean_dev, const double* var_dev,
                      int64_t N, const double* z_host, int64_t S, double best_f, double beta, const uint8_t* alive_dev,
                      double* scores_dev);
/* ... and for the t-batches [x_i ; pending], 1 <= p <= 15, with the pending statistics given by the caller as for
 * bbh_qlogei_pending_big (the same call of the reference with X_pending set): per sample the maximum over the 1 + p points of the
 * utility of prog(y_r), for qLogEI the fat maximum.  NaN for a row whose joint covariance does not factor at any jitter level,
 * -inf for a masked row. */
int bbh_mc_acq_obj_pending(bbh_handle* h, int32_t kind, const bbh_objective_prog* prog, const double* mean_dev,
                           const double* var_dev, const double* cross_dev, int64_t N, int64_t p, const double* mean_p_host,
                           const double* cov_pp_host, const double* z_host, int64_t S, double best_f, double beta,
                           const uint8_t* alive_dev, double* scores_dev);

/* ---- desirability objectives with one model per target (bbh_desirability.hip) ----------------------------------------------
 * baybe/objectives/desirability.py:229-264 (as_pre_transformation=False, the default): every target has its own surrogate and the
 * desirability is computed per posterior sample, d = scal_t(w_t, prog_t(y_t)), in front of the acquisition utility.
 * BBH_SCAL_MEAN: sum_t w_t g_t;  BBH_SCAL_GEOM_MEAN: exp(sum_t w_t log(g_t + 2^-52)); both in ascending t with rounded products. */
enum bbh_scalarizer { BBH_SCAL_MEAN = 0, BBH_SCAL_GEOM_MEAN = 1 };
#define BBH_DES_MAX_TARGETS 8
typedef struct bbh_desirability {
  int32_t n_targets, scalarizer; /* 2 ... BBH_DES_MAX_TARGETS targets */
  double weight[BBH_DES_MAX_TARGETS];
  bbh_objective_prog prog[BBH_DES_MAX_TARGETS];
} bbh_desirability;
/* t-batches of one point: mean_dev / var_dev [T, N] (target-major), z_host [S, T]; kind BBH_ACQ_QLOGEI ... BBH_ACQ_QPSTD;
 * 1 <= S <= 8192.  -inf for a masked row. */
int bbh_desirability_q1(bbh_handle* h, int32_t kind, const bbh_desirability* des, const double* mean_dev, const double* var_dev,
                        int64_t N, const double* z_host, int64_t S, double best_f, double beta, const uint8_t* alive_dev,
                        double* scores_dev);
/* t-batches [x_i ; pending], 1 <= p <= 15: cross_dev [T, N, p], mean_p_host [T, p], cov_pp_host [T, p, p], z_host [S, p + 1, T].
 * form: where the T thread-private Cholesky factors live - 0 LDS (bad arguments where they do not fit the workgroup's LDS, nothing
 * is launched), 1 a chunked global workspace, -1 LDS where it fits; both forms give the same bits.  -inf for a masked row, NaN for
 * a row of which ANY target's joint covariance does not factor at any jitter level. */
int bbh_desirability_pending(bbh_handle* h, int32_t kind, const bbh_desirability* des, const double* mean_dev, const double* var_dev,
                             const double* cross_dev, int64_t N, int64_t p, const double* mean_p_host, const double* cov_pp_host,
                             const double* z_host, int64_t S, double best_f, double beta, int32_t form, const uint8_t* alive_dev,
                             double* scores_dev);
int bbh_desirability_last_form(bbh_handle* h); /* of the last bbh_desirability_pending launch: 0 LDS, 1 workspace, -1 none yet */

/* Analytic family (q = 1): PM, PSTD(+-), UCB(beta), EI, LogEI, PI; sigma^2 clamped at 1e-12. */
int bbh_analytic_acq(bbh_handle* h, int32_t kind, const double* mean_dev, const double* var_dev, int64_t N,
                     double best_f, double sign, double beta, int32_t maximize, const uint8_t* alive_dev,
                     double* scores_dev);

/* ---- qLogNEHVI (bbh_qnehvi.hip, with the plain qNEHVI below) ------------------------- */
#define BBH_MAX_OBJECTIVES 4
/* q'=1 scores over m <= 4 independent outputs.  Per output o: tmat_dev[o] [N,S] conditional means
 * per MC sample (bbh_posterior_columns of the extended model), var_dev[o] [N] conditional variance;
 * sample f_o(x)_s = tmat[o][i][s] + sqrt(var[o][i]) zx_host[s*m+o], oriented by sign_host[o].
 * Cells of sample s: cell_off_host[s] .. cell_off_host[s+1] (prefix offsets, [S+1]); cell c stores
 * cell_lo_host[c*m+o] (lower bound) and cell_loglen_host[c*m+o] = log(min(upper,1e10) - lower).
 * score = logmeanexp_s logsumexp_c sum_o fatmin(log_fatplus(f_o - lo; 1e-6), loglen; 1e-2).
 * A null tmat_dev[o] or var_dev[o] of a used target with N > 0 is a bad-arguments error (-1), nothing is enqueued. */
int bbh_qlognehvi(bbh_handle* h, int32_t m, int64_t N, const double* const* tmat_dev,
                  const double* const* var_dev, const double* sign_host, const double* zx_host, int64_t S,
                  const int64_t* cell_off_host, const double* cell_lo_host, const double* cell_loglen_host,
                  const uint8_t* alive_dev, double* scores_dev);
/* bbh_qlognehvi with the conditional means in sample-major layout, tmat_dev[o] [S, N] (bbh_posterior_columns_sm). */
int bbh_qlognehvi_sm(bbh_handle* h, int32_t m, int64_t N, const double* const* tmat_dev,
                  const double* const* var_dev, const double* sign_host, const double* zx_host, int64_t S,
                  const int64_t* cell_off_host, const double* cell_lo_host, const double* cell_loglen_host,
                  const uint8_t* alive_dev, double* scores_dev);

/* Baseline pruning support (prune_inferior_points_multi_objective): obj_host [S, n, m] oriented
 * objective samples; counts_host[i] = number of samples in which point i is non-dominated and above
 * ref_host [m] in every objective. */
int bbh_pareto_frequency(bbh_handle* h, const double* obj_host, int64_t S, int64_t n, int32_t m,
                         const double* ref_host, int64_t* counts_host);

/* bbh_pareto_frequency with the objective samples already on the device (obj_dev [S, n, m], as bbh_nehvi_samples writes them). */
int bbh_pareto_frequency_dev(bbh_handle* h, const double* obj_dev, int64_t S, int64_t n, int32_t m,
                             const double* ref_host, int64_t* counts_host);

/* qLogNEHVI set-up of one target on the device (replaces: baseline joint posterior -> host Cholesky -> host samples -> an
 * (n + nb) x S host array for bbh_set_mean_columns).  h holds the target's model extended by nb baseline rows as noise-free
 * observations (bbh_set_model_ex with a noise mask: the last nb rows; their target values are not read) and is factorised.
 * BoTorch's joint draw of the baseline values through the cached Cholesky root (qLogNoisyExpectedHypervolumeImprovement with
 * cache_root, built at baybe/acquisition/_builder.py:319-324) is the generative form of that factor,
 * y_ext,s = c + L_ext [t; z_s] with t = L^-1 (y - c) on the training rows and z_s = z_host[s, :] the sample's base samples:
 * Fb_dev[(s * nb + b) * m + o] = sign * (baseline row b of y_ext,s, original target scale); with want_columns != 0 the S weight
 * columns L_ext^-T [t; z_s] of the model conditioned on each sample are installed for bbh_posterior_columns(_sm).
 * Asynchronous on the handle's stream. */
int bbh_nehvi_samples(bbh_handle* h, const double* z_host, int64_t S, int64_t nb, double sign, int32_t o, int32_t m,
                      double* Fb_dev, int32_t want_columns);
/* The same with the base samples already on the device (bbh_sobol_normal_dev): sample s, baseline row b reads
 * z_dev[s * ld + cols_dev[b]] (cols_dev [nb] int32: where the row's base sample sits in a draw over all baseline rows and
 * targets - repeated baseline rows are skipped by the caller). */
int bbh_nehvi_samples_dev(bbh_handle* h, const double* z_dev, int64_t ld, const int32_t* cols_dev, int64_t S, int64_t nb, double sign,
                          int32_t o, int32_t m, double* Fb_dev, int32_t want_columns);

/* Box decompositions on the device: one wavefront per MC sample over Fb_dev [S, nb, m] (oriented objective samples, as
 * bbh_nehvi_samples writes them) - the algorithm and visiting order of bbh_cells_create, the cell lists stay on the handle
 * for bbh_qlognehvi_cells.  *total_out = cells over all samples; *overflow_out = samples whose list of local upper bounds
 * exceeded the kernel's capacity (then, or for nb > 512, the caller takes the host form).  bbh_cells_read_dev copies the
 * lists out in the layout of bbh_cells_get (tests, statistics). */
int bbh_cells_build_dev(bbh_handle* h, const double* Fb_dev, int64_t S, int64_t nb, int32_t m, const double* ref_host,
                        int64_t* total_out, int64_t* overflow_out);
int bbh_cells_read_dev(bbh_handle* h, int64_t* off_host, double* lo_host, double* loglen_host);
/* bbh_qlognehvi_sm against the handle's device-resident cell lists (bbh_cells_build_dev with the same S and m). */
int bbh_qlognehvi_cells(bbh_handle* h, int32_t m, int64_t N, const double* const* tmat_dev,
                        const double* const* var_dev, const double* sign_host, const double* zx_host, int64_t S,
                        const uint8_t* alive_dev, double* scores_dev);

/* ---- qNoisyExpectedImprovement / qLogNoisyExpectedImprovement (baybe/acquisition/acqfs.py:226-243) -------------------------
 * BoTorch's qNoisyExpectedImprovement / qLogNoisyExpectedImprovement as BayBE builds them (X_baseline = all training inputs,
 * prune_baseline, cache_root: baybe/acquisition/_builder.py:319-324), q' = 1; picks and pending points join the baseline
 * (set_X_pending with a cached root).  The set-up is qLogNEHVI's with one target: h holds the model extended by the nb baseline
 * rows, bbh_nehvi_samples(h, ..., m = 1, want_columns = 1) wrote the oriented baseline samples obj_dev [S, nb] and installed the
 * S weight columns.  Per candidate and sample:  f_s = E[f(x) | D, F_b,s] + safe_sd(Var[f(x) | D, X_b]) zx[s],
 * u_s = sign f_s - best[s];  BBH_ACQ_QLOGNEI: logmeanexp_s log_fatplus(u_s; 1e-6),  BBH_ACQ_QNEI: mean_s max(u_s, 0);
 * rows with alive_dev[i] == 0 score -inf. */
/* prune_inferior_points (botorch, called from the acquisition constructor): counts_host[b] = number of the S samples whose largest
 * value is point b's (ties: the first index).  Returns after the stream has drained. */
int bbh_best_frequency_dev(bbh_handle* h, const double* obj_dev, int64_t S, int64_t nb, int64_t* counts_host);
/* best_dev[s] = max_b obj_dev[s, b]: the per-sample incumbent of the noisy improvement.  Asynchronous. */
int bbh_sample_best_dev(bbh_handle* h, const double* obj_dev, int64_t S, int64_t nb, double* best_dev);
/* Unfused form over a materialised sample-major block tmat_sm_dev [S, N] (bbh_posterior_columns_sm of the same handle):
 * verification form, models on the materialised-K* columns path, S > 512.  var_dev / alive_dev / scores_dev [N]; the caller
 * chunks the candidates.  Asynchronous. */
int bbh_nei_q1(bbh_handle* h, int32_t kind, const double* tmat_sm_dev, const double* var_dev, int64_t N, const double* zx_host,
               int64_t S, const double* best_dev, double sign, const uint8_t* alive_dev, double* scores_dev);
/* Fused form: the cooperative conditional-mean kernel with a scoring epilogue - candidates X_dev [N, ldx] in, scores out, the
 * [S, N] matrix of conditional means is never written and no workspace is taken.  S must be the installed column count.
 * Returns 0 when the pass is enqueued and 1 when the form does not apply (S > 512, a model on the materialised-K* path, or
 * BBH_NEI_FUSED=0): nothing is enqueued then and the caller takes bbh_posterior_columns_sm + bbh_nei_q1. */
int bbh_score_nei(bbh_handle* h, int32_t kind, const double* X_dev, int64_t N, int64_t ldx, const double* var_dev,
                  const double* zx_host, int64_t S, const double* best_dev, double sign, const uint8_t* alive_dev,
                  double* scores_dev);

/* ---- qLogNParEGO (BoTorch qLogNParEGO; built like the noisy forms above, baybe/acquisition/_builder.py:319-324) --------------
 * qLogNoisyExpectedImprovement of the augmented Chebyshev scalarisation of m oriented targets, q' = 1; picks and pending points
 * join the baseline.  Set-up as for qLogNEHVI: one extended model per target, bbh_nehvi_samples wrote the oriented baseline
 * samples Fb_dev [S, nb, m] and installed each target's S weight columns.  With w_host [m] weights on the simplex, hi_host [m] and
 * inv_range_host [m] = 1 / (hi - lo) (bounds of the baseline's oriented posterior means):
 *   t_o = w_o (hi_o - y_o) inv_range_o,   g(y) = -(max_o t_o + 0.05 sum_o t_o). */
/* best_dev[s] = max_b g(Fb_dev[s, b, :]): the per-sample incumbent.  Asynchronous. */
int bbh_scalarized_best_dev(bbh_handle* h, const double* Fb_dev, int64_t S, int64_t nb, int32_t m, const double* w_host,
                            const double* hi_host, const double* inv_range_host, double* best_dev);
/* prune_inferior_points under the scalarisation: counts_host[b] = number of the S samples in which point b has the largest g
 * (ties: the first index).  Returns after the stream has drained. */
int bbh_scalarized_best_frequency_dev(bbh_handle* h, const double* Fb_dev, int64_t S, int64_t nb, int32_t m, const double* w_host,
                                      const double* hi_host, const double* inv_range_host, int64_t* counts_host);
/* Scores of N candidates from the m sample-major blocks tmat_sm_dev[o] [S, N] (bbh_posterior_columns_sm of target o's handle) and
 * variances var_dev[o] [N]:  f_s,o = sign_host[o] (tmat[o][s][i] + safe_sd(var[o][i]) zx_dev[s * m + o]),  u_s = g(f_s) - best_dev[s],
 * scores_dev[i] = logmeanexp_s log_fatplus(u_s; 1e-6); rows with alive_dev[i] == 0 score -inf.  The sample axis is cut into slices
 * of a fixed length whose partial sums are combined in a fixed order: a row's score does not depend on N (the caller chunks the
 * candidates) and equal rows score bit-identically.  Workspace: S / 16 x N doubles on the handle.  Asynchronous. */
int bbh_nparego_q1(bbh_handle* h, int32_t m, int64_t N, const double* const* tmat_sm_dev, const double* const* var_dev,
                   const double* sign_host, const double* zx_dev, int64_t S, const double* w_host, const double* hi_host,
                   const double* inv_range_host, const double* best_dev, const uint8_t* alive_dev, double* scores_dev);

/* ---- qNoisyExpectedHypervolumeImprovement (plain) ----------------------------------------------------------------------------
 * The operands of bbh_qlognehvi_cells / bbh_qlognehvi_sm, scored without smoothing, in double precision:
 * scores_dev[i] = (1/S) sum_s sum_{cells c of s} prod_o max(min(f_s,o - lo_c,o, len_c,o), 0); rows with alive_dev[i] == 0 score -inf. */
int bbh_qnehvi_cells(bbh_handle* h, int32_t m, int64_t N, const double* const* tmat_dev, const double* const* var_dev,
                     const double* sign_host, const double* zx_host, int64_t S, const uint8_t* alive_dev, double* scores_dev);
int bbh_qnehvi_sm(bbh_handle* h, int32_t m, int64_t N, const double* const* tmat_dev, const double* const* var_dev,
                  const double* sign_host, const double* zx_host, int64_t S, const int64_t* cell_off_host, const double* cell_lo_host,
                  const double* cell_loglen_host, const uint8_t* alive_dev, double* scores_dev);

/* ---- qExpectedHypervolumeImprovement / qLogExpectedHypervolumeImprovement (baybe/acquisition/acqfs.py:429-464) ---------------
 * The non-noisy pair: ONE cell list per recommendation (the box decomposition of the models' oriented posterior means at the
 * measurement rows, baybe/acquisition/_builder.py:286-299), cell_lo_host / cell_up_host [C, m] (the upper bounds may be +inf),
 * C >= 1, 2 <= m <= BBH_MAX_OBJECTIVES.  Every operand arrives ORIENTED: the caller negates the means (and pending means) of a
 * minimised target and that target's base-sample column, so that y = mean + L z is sign (m + L z); variances and covariances carry
 * no sign.  The m targets are independent, the q' = 1 + p points of one target jointly Gaussian (bbh_joint.h: psd_safe_cholesky
 * per target).  Per base sample s and cell c, with y[r, j] the draw of point r and target j:
 *   log == 0 (qEHVI):    sum over the non-empty subsets A of the q' points of (-1)^(|A|+1) prod_j max(0, min_{r in A}(min(y[r,j], up_c[j]) - lo_c[j]))
 *   log != 0 (qLogEHVI): li = log_fatplus(y - lo; 1e-6); per subset sum_j fatmin2(fatmin_{r in A} li, log(min(up, 1e10) - lo); 1e-2);
 *                        logsumexp per subset size, logaddexp into an odd and an even slot, logdiffexp(odd, even) per cell
 * summed over the cells and averaged over the samples (logsumexp / logmeanexp in the log form).  The subsets are walked by
 * ascending size, lexicographically within a size; double precision throughout.  The samples are cut into slices of a fixed
 * length over a second grid dimension and the slices are finished in slice order, so two runs give the same bits.
 * -inf for a masked row. */
#define BBH_EHVI_MAX_Q 8 /* q' = 1 + p <= 8: 255 subsets */
/* q' = 1: mean_dev / var_dev [m, N] (target-major), z_host [S, m]; 1 <= S <= 8192; 1 x 1 jitter as bbh_mc_acq_q1. */
int bbh_ehvi_q1(bbh_handle* h, int32_t log, int32_t m, const double* mean_dev, const double* var_dev, int64_t N,
                const double* cell_lo_host, const double* cell_up_host, int64_t C, const double* z_host, int64_t S,
                const uint8_t* alive_dev, double* scores_dev);
/* t-batches [x_i ; pending], 1 <= p <= BBH_EHVI_MAX_Q - 1: cross_dev [m, N, p], mean_p_host [m, p], cov_pp_host [m, p, p],
 * z_host [S, p + 1, m].  form: where the m thread-private Cholesky factors live - 0 LDS (bad arguments where the workgroup's share
 * of the LDS does not hold them, nothing is launched), 1 a chunked global workspace, -1 the faster one by measurement (the
 * workspace); both forms give the same bits.  NaN for a row of which ANY target's joint covariance does not factor at any jitter level. */
int bbh_ehvi_pending(bbh_handle* h, int32_t log, int32_t m, const double* mean_dev, const double* var_dev, const double* cross_dev,
                     int64_t N, int64_t p, const double* mean_p_host, const double* cov_pp_host, const double* cell_lo_host,
                     const double* cell_up_host, int64_t C, const double* z_host, int64_t S, int32_t form, const uint8_t* alive_dev,
                     double* scores_dev);
int bbh_ehvi_last_form(bbh_handle* h); /* of the last bbh_ehvi_pending launch: 0 LDS, 1 workspace, -1 none yet */

/* ---- qNegIntegratedPosteriorVariance (baybe/acquisition/acqfs.py: qNIPV) -------------------------------------------------------
 * The variance that conditioning the GP on a t-batch [x ; B] removes at M integration points, B = the handle's b pending points
 * (bbh_pending_set).  One Matern-1/2, Matern-3/2, Matern-5/2 or RBF kernel, one task, n <= 512.  With cov the posterior covariance
 * given the training data, s2 the noise and every quantity in the target's original scale (as bbh_posterior's variance):
 *   A = (K + s2 I)^-1 K(X, P) [n, M],   G = cov(B, B) + s2 I,   H = G^-1 cov(B, P) [b, M],
 *   C_j(x) = k(x, p_j) - k(x, X) A[:, j] - cov(x, B) H[:, j],
 *   gain(x) = sum_j C_j(x)^2 / (max(var(x) - cov(x, B) G^-1 cov(B, x), 0) + s2);
 * qNIPV([x ; B]) = gain(x) / M - mean_j (var(p_j) - cov(p_j, B) H[:, j]).  The selection runs on gain (the constant would only
 * throw away its low bits).
 * bbh_nipv_set_points: once per recommendation, after bbh_factorize: P_host [M, d] rows of the candidates' representation; builds A
 * from the factorisation (two multiplications by L^-1) and keeps it resident, padded to 64 columns; var_p_host [M] (may be null)
 * receives var(p_j).  A new bbh_factorize invalidates it.  An M whose resident operand (np + 16) Mpad 8 bytes exceeds 256 MiB is
 * refused with a text (M = 16384 at n = 512 takes 66 MiB).
 * bbh_nipv_gain: var_dev [N] (bbh_posterior), cross_dev [N, b] (bbh_cross_cov), H_host [b, M], ginv_host [b, b] = G^-1; with b = 0
 * the three may be null.  gain_dev [N]; -inf for a row with alive_dev[i] == 0.  The columns are cut into slices over a second grid
 * dimension and the slices are added in slice order: two runs, and equal rows at different positions, give the same bits. */
int bbh_nipv_set_points(bbh_handle* h, const double* P_host, int64_t M, double* var_p_host);
int bbh_nipv_gain(bbh_handle* h, const double* X_dev, int64_t N, int64_t ldx, const double* var_dev, const double* cross_dev,
                  const double* H_host, const double* ginv_host, const uint8_t* alive_dev, double* gain_dev);
int bbh_last_nipv_form(bbh_handle* h); /* of the last bbh_nipv_gain launch: 0 one 16-row tile per workgroup, 1 two; -1 none yet */

/* ---- Exact Shapley explanations of the posterior mean (baybe/insights/shap.py: SHAPInsight) ---------------------------------------
 * M features = groups of comp-rep columns (group_of_col_host [d]: group index 0 .. M - 1, or -1 for a column in no group, which
 * always keeps the background row's value), R explained rows X_dev [R, ldx], B background rows Bg_dev [B, ldb]:
 *   v(r, S) = (1 / B) sum_b mean(compose(x_r on the groups of S, b elsewhere)),  mean = bbh_posterior's, original target scale,
 *   phi_g(r) = sum_{S without g} |S|! (M - |S| - 1)! / M! [v(r, S + g) - v(r, S)],  base = v(., empty) = mean_b mean(b).
 * Bit g of a mask S stands for group g.  1 <= M <= 16.
 * bbh_shap_values: the fused form - one Matern-1/2, Matern-3/2, Matern-5/2 or RBF kernel, one task, n <= 512; anything else returns
 * -1 and bbh_last_error names the unmet condition.  Per-group partial squared distances of the rows to the training points, then
 * one kernel value per (r, S, b, t) with d2 = lo[S_lo] + hi[S_hi] from two tables of direct sums; no composed row is materialised.
 * v_dev [R, 2^M] may be null (the handle's workspace holds it then); phi_dev [R, M]; base_host may be null.  Sums run over the
 * training points ascending, then the background rows ascending, then the masks ascending: equal rows give equal bits wherever
 * they stand, two runs give equal bits.
 * bbh_shap_compose: the generic form's rows for ANY model with d columns (the handle needs no model): rows_dev [count, d] holds the
 * composed rows of the triples first .. first + count of the order e = (r 2^M + S) B + b.
 * bbh_shap_reduce: out_dev [pairs] = mean over b, ascending, of f_dev [pairs, B].   bbh_shap_apply: phi_dev [R, M] from v_dev [R, 2^M]. */
int bbh_shap_values(bbh_handle* h, const double* X_dev, int64_t R, int64_t ldx, const double* Bg_dev, int64_t B, int64_t ldb,
                    const int32_t* group_of_col_host, int32_t M, double* v_dev, double* phi_dev, double* base_host);
int bbh_shap_compose(bbh_handle* h, const double* X_dev, int64_t R, int64_t ldx, const double* Bg_dev, int64_t B, int64_t ldb,
                     const int32_t* group_of_col_host, int32_t d, int32_t M, int64_t first, int64_t count, double* rows_dev);
int bbh_shap_reduce(bbh_handle* h, const double* f_dev, int64_t pairs, int64_t B, double* out_dev);
int bbh_shap_apply(bbh_handle* h, const double* v_dev, int64_t R, int32_t M, double* phi_dev);

/* ---- Linear constraints of a continuous subspace (baybe/constraints/continuous.py: ContinuousLinearConstraint) ---------------------
 * The feasible set { c in R^dc : lo <= c <= hi, E c = e, G c >= g }, dc <= 32, me + mi <= 16 rows (dependent equalities dropped by
 * the caller).  Neither call needs a model on the handle.  Nothing is contracted and every sum runs over the columns, then the
 * rows, ascending; no transcendental function is used.
 * bbh_polytope_sample replaces botorch.utils.sampling.get_polytope_samples (baybe/searchspace/continuous.py:544-571, one sequential
 * hit-and-run chain with 10 000 burn-in steps): R independent hit-and-run chains of T steps in the reduced coordinates c = c0 + Z y
 * (Z_host [dc, dz] an orthonormal basis of null(E), c0 an interior point), every chain from y = 0, over the rows
 * bl <= Z y <= bu (bl = lo - c0, bu = hi - c0) and GZ y >= bg (GZ_host [mi, dz] = G Z, bg = g - G c0).  One step: d = u - 1/2 with
 * u uniform in [0, 1)^dz, the chord by a ratio test with slacks recomputed from y, t uniform on the chord.  The uniforms are
 * counter-based (SplitMix64's finaliser): key = mix(mix(seed + G) + G (chain + 1)), h = mix(key + G (64 step + draw + 1)),
 * u = (h >> 11) 2^-53, G = 0x9E3779B97F4A7C15 - a pure function of (seed, chain, step, draw), so the same seed gives the same bits
 * however the chains are spread over the grid, and chain r of a call for R rows is chain r of any larger call.
 * out_dev [R, dc] = clip(c0 + Z y, lo, hi).  1 <= dz <= dc (dz = 0 - the equalities pin the point - is the caller's to answer).
 * bbh_polytope_project stands where the box optimiser clips (np.clip in baybe_amd/continuous.py::maximize_box; the reference hands
 * its constraints to scipy's SLSQP inside botorch's optimize_acqf): out_dev [k, dc] = the Euclidean projection of every row of
 * P_dev [k, ldp] by a regularised semismooth Newton ascent on the dual in the me + mi multipliers, the box applied as a clip.
 * R_host [me + mi, dc] = [E; G], t_host = [e; g].  status_dev [k]: 0 ok, 1 iteration budget exhausted (the row holds the clipped
 * point of the last multipliers).  The output lies in [lo, hi] bit-exactly and meets |E x - e|_i, (g - G x)_i^+ <= tolf S_abs,i,
 * S_abs,i = sum_k |row_ik x_k| + |rhs_i|; callers pass tolf = 4 (dc + 2 dc + mi) eps.  A row that already meets this comes back
 * bit for bit (so projecting twice changes nothing); equal rows give equal bits wherever they stand; two runs give equal bits.
 * mu_min: the smallest regulariser, 1e-10 max_i |row_i|^2. */
int bbh_polytope_sample(bbh_handle* h, int32_t dc, int32_t dz, int32_t mi, const double* Z_host, const double* GZ_host,
                        const double* c0_host, const double* lo_host, const double* hi_host, const double* bl_host,
                        const double* bu_host, const double* bg_host, int64_t R, int32_t T, uint64_t seed, double* out_dev);
int bbh_polytope_project(bbh_handle* h, int32_t dc, int32_t me, int32_t mi, const double* R_host, const double* t_host,
                         const double* lo_host, const double* hi_host, double tolf, double mu_min, const double* P_dev, int64_t k,
                         int64_t ldp, double* out_dev, int32_t* status_dev);

/* Box decomposition of the non-dominated region, one per MC sample (host code, no device work; BoTorch's
 * FastNondominatedPartitioning inside qLogNoisyExpectedHypervolumeImprovement, built at
 * baybe/acquisition/_builder.py:319-324).  obj_host [S, n, m] oriented baseline objective samples, ref_host [m].
 * bbh_cells_create computes every sample's disjoint boxes and returns an opaque object and the total box count;
 * bbh_cells_get copies them out in the layout bbh_qlognehvi takes (off_host [S+1], lo_host / loglen_host
 * [total, m], loglen = log(min(upper, 1e10) - lower)); bbh_cells_destroy frees the object. */
int bbh_cells_create(const double* obj_host, int64_t S, int64_t n, int32_t m, const double* ref_host,
                     void** cells_out, int64_t* total_out);
int bbh_cells_get(void* cells, int64_t* off_host, double* lo_host, double* loglen_host);
int bbh_cells_destroy(void* cells);

/* Scrambled Sobol points bitwise as torch.quasirandom.SobolEngine(dimension, scramble=True, seed) draws them (host code, integer
 * arithmetic; the engine botorch's SobolQMCNormalSampler uses).  state [dim, 30]: the engine's unscrambled direction numbers,
 * scrambled in place with the engine's random lower-triangular bit matrices ltm [dim, 30, 30] (0 / 1 entries as drawn, before
 * tril);  bbh_sobol_draw: out [n, dim] = the first n points for the scrambled state and the integer shift [dim]. */
int bbh_sobol_scramble(int64_t* state, const int64_t* ltm, int64_t dim);
int bbh_sobol_draw(const int64_t* state, const int64_t* shift, int64_t n, int64_t dim, double* out);
/* The sampler's complete base-sample draw, sqrt(2) erfinv(2 v - 1) of the engine's points for a seed (SobolQMCNormalSampler, built
 * through BoTorch's acquisition constructors at baybe/acquisition/_builder.py:195-334): state0 [dim, 30] = the engine's UNSCRAMBLED
 * direction numbers; the scrambling bits come from an MT19937 restating torch's CPU generator.  bbh_sobol_normal: host code,
 * out_host [n, dim];  bbh_sobol_normal_dev: generator and scrambling on the host, points and transform on the device into
 * out_dev [n, dim], asynchronous on the handle's stream. */
int bbh_sobol_normal(const int64_t* state0, uint64_t seed, int64_t n, int64_t dim, double* out_host);
int bbh_sobol_normal_dev(bbh_handle* h, const int64_t* state0, uint64_t seed, int64_t n, int64_t dim, double* out_dev);

/* 64-bit content key of host buffers (host code, std::threads): multiply-fold hash over 4 MB pieces, the pieces' digests folded in
 * order.  Keys the device-resident copy of the discrete subspace's computational representation on its content
 * (baybe/searchspace/discrete.py:704-735 hands the frame out on every call; botorch/discrete.py:123 converts it per call). */
uint64_t bbh_content_key(const void* const* bufs, const int64_t* lens, int32_t nbuf, int32_t threads);

/* ---- selection --------------------------------------------------------------------- */
/* First-index argmax of scores_dev [N] (NaN never wins) -> host. */
int bbh_argmax(bbh_handle* h, const double* scores_dev, int64_t N, double* best_val_host,
               int64_t* best_idx_host);
/* k best scores, descending, ties -> lower index first; -> host arrays [k]. */
int bbh_topk(bbh_handle* h, const double* scores_dev, int64_t N, int64_t k, double* vals_host,
             int64_t* idx_host);

/* ---- farthest point sampling (the initial, non-Bayesian recommendation) --------------------
 * Replaces baybe/utils/sampling_algorithms.py:15-172 (farthest_point_sampling) as FPSRecommender._recommend_discrete calls it
 * (baybe/recommenders/pure/nonpredictive/sampling.py:146-177), without the N x N matrix of sklearn.metrics.pairwise_distances
 * (sampling_algorithms.py:120-126).  Every comparison is decided by  d^2(x, y) = sum_k (x_k - y_k) * (x_k - y_k),  k ascending from
 * 0.0, each operation rounded to fp64 and nothing contracted; ties are resolved in RANKS, the positions in
 * np.lexsort(tuple(points.T)) (sampling_algorithms.py:117). */
/* StandardScaler.transform + the reordering points[sort_idx] (sampling.py:153-161, sampling_algorithms.py:117-118):
 * P_dev[k * ldp + r] = (X_dev[order_dev[r] * ldx + k] - mean_host[k]) / scale_host[k] for r < M, k < d - IEEE subtraction and
 * division, bit for bit numpy's (X - mean) / scale - and 0 for M <= r < ldp.  order_dev [M] holds rows of X_dev [N, ldx]
 * (null: the identity, M <= N).  Asynchronous on the handle's stream. */
int bbh_fps_prepare(bbh_handle* h, const double* X_dev, int64_t N, int32_t d, int64_t ldx, const double* mean_host,
                    const double* scale_host, const int64_t* order_dev, int64_t M, double* P_dev, int64_t ldp);
/* np.argmax(dist_matrix) of the "farthest" initialisation (sampling_algorithms.py:131-135): the pair of live ranks a < b with the
 * largest d^2; bit-equal maxima resolve to the smallest a, then the smallest b.  P_dev [d, ldp] as bbh_fps_prepare leaves it,
 * alive_dev [M] uint8 or null (all rows live); 2 <= M < 2^31 - 256, M <= 65535 * 256, d <= 768.  a = b = -1 with fewer than two
 * live rows.  Synchronises the stream. */
int bbh_fps_farthest_pair(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, const uint8_t* alive_dev,
                          double* d2_host, int64_t* a_host, int64_t* b_host);
/* The selection loop (sampling_algorithms.py:144-169).  n_start > 0 begins a selection from start_ranks_host [n_start] (the
 * initial selection, in ranks) on P_dev / alive_dev, which must stay valid while the selection continues; n_start = 0 continues
 * the handle's selection (the matrix arguments are ignored).  Then n_picks picks: each takes, among the live unselected rows whose
 * minimum d^2 to the selection is the maximum, the k-th in rank order - k < 0: the last one (max_indices[-1], random_tie_break
 * off), any number of picks enqueued back to back with one synchronisation; k >= 0 (np.random.choice over the tied rows, drawn
 * by the caller): n_picks <= 1.  ranks_host / d2_host [n_picks]: the picked ranks and the minimum d^2 each was picked at.
 * count_host (may be null): the number of tied rows the NEXT pick would choose from. */
int bbh_fps_greedy(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, const uint8_t* alive_dev,
                   const int64_t* start_ranks_host, int64_t n_start, int64_t n_picks, int64_t k, int64_t* ranks_host,
                   double* d2_host, int64_t* count_host);

/* ---- k-medoids, method "alternate" (the clustering choice for the initial, non-Bayesian recommendation) ----
 * Replaces baybe/utils/clustering_algorithms/third_party/kmedoids.py as PAMClusteringRecommender drives it
 * (baybe/recommenders/pure/nonpredictive/clustering.py:100-132, 148-193), without the N x N matrix of pairwise_distances
 * (kmedoids.py:231).  Positions are the columns of P_dev [d, ldp] in the order given (bbh_fps_prepare with order_dev = the
 * candidates' rows: a dense matrix of live rows, no masks).  d2(x, y) = sum_k (x_k - y_k) * (x_k - y_k), k ascending from 0.0,
 * nothing contracted; dist = sqrt(d2), IEEE correctly rounded; DISTANCES are compared and summed; every deciding sum is sequential
 * in ascending position; every tie goes to the first in position / cluster order (numpy's argmin).  Limits of all four:
 * 1 <= M < 2^31 - 256, 1 <= d <= 768, 1 <= k <= M.  All four are asynchronous on the handle's stream and keep no state. */
/* D[medoid candidates, :] (kmedoids.py:481, 490): out_dev [T, M] = dist(rows_dev[t], j); a row index outside [0, M) gives a row of
 * NaN.  rows_dev [T] int64, T >= 1. */
int bbh_pam_dist_rows(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, const int64_t* rows_dev, int64_t T,
                      double* out_dev);
/* np.argmin(D[medoid_idxs, :], axis=0) (kmedoids.py:256, 302) and the distance it found: labels_dev [M] int32 = the smallest cluster
 * index among bit-equal minima of dist(medoids_dev[c], j), dist_dev [M] that distance (the column minimum behind inertia_,
 * kmedoids.py:304).  medoids_dev [k] int64; the medoids' coordinates pass through LDS in tiles, so any k <= M works. */
int bbh_pam_assign(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, const int64_t* medoids_dev, int64_t k,
                   int32_t* labels_dev, double* dist_dev);
/* np.sum(in_cluster_distances, axis=1) of every cluster at once (kmedoids.py:326-329).  Ps_dev [d, lds]: the points GROUPED by
 * label with a stable sort (position order survives inside a cluster), cluster c in the columns [starts_dev[c], starts_dev[c + 1]);
 * tile_starts_dev [k + 1]: exclusive prefix sums of ceil(n_c / 256); both int64.  cost_dev [M], by grouped column:
 * cost[i] = sum over the columns j of i's cluster, ascending, of dist(i, j) - added one by one in that order.  table_dev
 * [2 * max_tiles] int32 receives the (cluster, row tile) pairs the grid runs over; max_tiles >= M / 256 + k. */
int bbh_pam_cost(bbh_handle* h, const double* Ps_dev, int64_t M, int32_t d, int64_t lds, const int64_t* starts_dev,
                 const int64_t* tile_starts_dev, int64_t k, int32_t* table_dev, int64_t max_tiles, double* cost_dev);
/* The medoid update of every cluster (kmedoids.py:312-339), one workgroup each: the minimum cost at the smallest grouped column,
 * curr_cost = the cost at the medoid's column, or at the cluster's first column if the medoid is not a member
 * (np.argmax(cluster_k_idxs == medoid) = 0), adopted only if min_cost < curr_cost.  perm_dev [M] int64: grouped column -> position.
 * medoids_dev [k] int64 is updated in place; flags_dev [k] int32: 1 = the cluster is empty (skipped), 2 = its medoid changed. */
int bbh_pam_update(bbh_handle* h, const double* cost_dev, const int64_t* perm_dev, int64_t M, const int64_t* starts_dev, int64_t k,
                   int64_t* medoids_dev, int32_t* flags_dev);

/* ---- k-means (Lloyd) over the matrix bbh_fps_prepare leaves, batched over R restarts (bbh_kmeans.hip) ---------------------------------
 * The device side of sklearn.cluster.KMeans as KMeansClusteringRecommender drives it (nonpredictive/clustering.py:196-252), with the
 * restarts as one workload.  d2(x, c) = sum_k (x_k - c_k) * (x_k - c_k), k ascending from 0.0, nothing contracted; a label is the
 * smallest cluster index among equal minima; no floating-point atomics: every sum has a fixed order (a 256-position tile first, tiles
 * ascending), so two runs give the same bits.  Limits of all: 1 <= M < 2^31 - 256, 1 <= d <= 768, 1 <= k <= M, R <= 65535.  All are
 * asynchronous on the handle's stream and keep no state. */
/* How a pass over R restarts is tiled: *restarts_per_tile restarts' centres share LDS (a point is read once per such tile);
 * *chunks > 1: one restart per tile, its centres streamed through LDS in that many chunks (large k * d). */
int bbh_kmeans_plan(bbh_handle* h, int32_t d, int64_t k, int64_t R, int32_t* restarts_per_tile, int32_t* chunks);
/* k-means++ for R restarts at once.  idx_dev [R, k] int64: column 0 holds the first centres on entry, the rest is filled.  U_dev
 * [R, (k - 1) * T]: the uniforms of the further centres, T per centre.  Per centre: pot = the sum of closest, the T values u * pot
 * searched in the running sum of closest (first position that reaches it, clipped to M - 1), the candidate with the smallest new
 * potential, first on ties.  Work arrays: closest_dev [R, M], tilesum_dev [R, tiles], trialpart_dev [R, T, tiles], cand_dev [R, T]
 * int64, tiles = ceil(M / 256). */
int bbh_kmeans_seed(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, int64_t* idx_dev, const double* U_dev, int64_t R,
                    int64_t k, int32_t T, double* closest_dev, double* tilesum_dev, double* trialpart_dev, int64_t* cand_dev);
/* One Lloyd pass for the restarts rid_dev [n_active] int32 (indices into the [R, ...] arrays).  From C_dev [R, k, d]: labels_dev
 * [R, M] int32 (read as the previous labels, then written), d2_dev [R, M] (to the assigned centre), inertia_dev [R]; with want_sums
 * also sums_dev [R, k, d] and counts_dev [R, k] of the members, Cnew_dev [R, k, d] = sums / counts (the sum itself where the count
 * is 0), shift_dev [R] = sum |new - old|^2.  flags_dev [R]: bit 0 = no label changed, bit 1 = an empty cluster was met.  Work
 * arrays: tiles * restarts_per_tile * (k * d + 1) doubles and tiles * restarts_per_tile * (k + 1) ints (1 for k * d and k without
 * want_sums). */
int bbh_kmeans_pass(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, const double* C_dev, const int32_t* rid_dev,
                    int64_t n_active, int64_t k, int32_t want_sums, int32_t* labels_dev, double* d2_dev, double* work_f64_dev,
                    int64_t work_f64_len, int32_t* work_i32_dev, int64_t work_i32_len, double* Cnew_dev, double* sums_dev,
                    int32_t* counts_dev, double* shift_dev, double* inertia_dev, int32_t* flags_dev);
/* The reference's selection without its [N, k] matrix: out_dev [k] int64 = per cluster the member with the smallest sqrt(d2), the
 * smallest position among equal ones; 0 for a cluster without members (argmin of an all-infinite column). */
int bbh_kmeans_select(bbh_handle* h, const int32_t* labels_dev, const double* d2_dev, int64_t M, int64_t k, int64_t* out_dev);

/* ---- Gaussian mixture (EM, full covariances) over the matrix bbh_fps_prepare leaves, batched over R restarts (bbh_gmm.hip) -----------
 * The device side of sklearn.mixture.GaussianMixture(n_components=batch_size) as GaussianMixtureClusteringRecommender drives it
 * (nonpredictive/clustering.py:255-304).  Parameters live in [R, ...] arrays indexed by restart: w [R, k], mu [R, k, d], cov and prec
 * [R, k, d, d] (row-major; prec upper triangular), logdet [R, k], nk [R, k]; rid_dev [n_active] int32 lists the restarts a call works
 * on.  log_resp [G, k, M] is component-major and labels [G, M] int32; restart r uses row r - base of both.  No floating-point
 * atomics: every sum has a fixed order (positions ascending inside a strip of 256-position tiles, strips ascending, or the MFMA's own
 * order), so two runs give the same bits.  Limits of all: 1 <= M < 2^31 - 256, 1 <= d <= 64, 1 <= k <= min(M, 65535), restarts
 * <= 65535.  All are asynchronous on the handle's stream and keep no state. */
/* The form a shape takes: *comps_per_chunk components' P_c and mu_c share LDS in the E-step; a workgroup of the M-step owns
 * *tiles_per_strip consecutive tiles (at most 64 strips, whatever M is). */
int bbh_gmm_plan(bbh_handle* h, int32_t d, int64_t k, int64_t M, int32_t* comps_per_chunk, int32_t* tiles_per_strip);
/* _estimate_gaussian_parameters + the weights of _m_step (sklearn/mixture/_gaussian_mixture.py:153-179, 258-294, 819-835).  r_jc =
 * exp(log_resp_dev) or the one-hot of labels_dev (-1: a row of zeros); exactly one of the two is given.  nk_c = sum_j r_jc + 10 * 2^-52,
 * mu_c = sum_j r_jc x_j / nk_c, cov_c = sum_j r_jc (x_j - mu_c)(x_j - mu_c)^T / nk_c + reg_covar I, w_c = nk_c / M, with normalize
 * also divided by sum_c w_c (ascending c).  work_dev: strips * n_active * k * (d + 1 + 256 * b (b + 1) / 2) doubles, b = ceil(d / 16). */
int bbh_gmm_mstep(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, const double* log_resp_dev,
                  const int32_t* labels_dev, int64_t src_base, const int32_t* rid_dev, int64_t n_active, int64_t k, double reg_covar,
                  int32_t normalize, double* work_dev, int64_t work_len, double* nk_dev, double* w_dev, double* mu_dev, double* cov_dev);
/* _compute_precision_cholesky + _compute_log_det_cholesky (_gaussian_mixture.py:297-351, 362-396): cov_c = L L^T, prec_c = (L^-1)^T,
 * logdet_c = sum_i log prec_c[i][i].  A pivot that is not finite and positive sets bit 0 of flags_dev [R] (int32, zeroed by the
 * caller): the host raises scikit-learn's ValueError. */
int bbh_gmm_precision(bbh_handle* h, const double* cov_dev, const int32_t* rid_dev, int64_t n_active, int64_t k, int32_t d,
                      double* prec_dev, double* logdet_dev, int32_t* flags_dev);
/* _e_step / predict (sklearn/mixture/_base.py:296-313, 359-395; _gaussian_mixture.py:413-512): y = (x_j - mu_c) prec_c, lp_jc =
 * -0.5 (d log 2 pi + |y|^2) + logdet_c + log w_c, lpn_j = m + log sum_c exp(lp_jc - m) with m = max_c lp_jc, log_resp_dev = lp - lpn,
 * labels_dev = the smallest c among equal maxima of lp, lpn_dev [G, M] (may be null) = lpn, lower_dev [R] = sum_j lpn_j / M.  work_dev:
 * tiles * n_active doubles. */
int bbh_gmm_estep(bbh_handle* h, const double* P_dev, int64_t M, int32_t d, int64_t ldp, const double* w_dev, const double* mu_dev,
                  const double* prec_dev, const double* logdet_dev, const int32_t* rid_dev, int64_t n_active, int64_t k, int64_t dst_base,
                  double* log_resp_dev, int32_t* labels_dev, double* lpn_dev, double* work_dev, int64_t work_len, double* lower_dev);

/* ---- random forest surrogate: traversal, ensemble moments and the fused MC acquisition pass (bbh_forest.hip) ------------------------
 * The device side of RandomForestSurrogate (baybe/surrogates/random_forest.py:53-139): the forest is fitted by scikit-learn on the
 * host; these calls replace the per-tree predictor.predict(candidates), the [T, N] EnsemblePosterior and BoTorch's per-sample gather
 * from it.  A forest of T trees is meta_dev [n_nodes, 4] int32 (feature, left child, right child, unused; children counted from the
 * tree's first node, left < 0 marks a leaf), tv_dev [n_nodes] fp64 (threshold of an inner node, value of a leaf) and off_dev [T + 1]
 * int64 (first node of every tree).  order_dev [n_order] int32 lists the trees a call visits, in the order every row's sums run.  A row
 * is cast to float32 and goes left iff (double)x32[feature] <= threshold: tree.predict of scikit-learn, bit for bit.  Trees of at most
 * min(lds_nodes, bbh_forest_lds_nodes()) nodes are walked out of LDS, larger ones in global memory.  A node whose feature or child lies
 * outside its tree reads as a NaN leaf.  No atomics; a row's result does not depend on where the row sits, so equal rows get equal
 * bits.  Limits of all: 1 <= N < 2^31 - 256, 1 <= d <= ldx, and 64 float32 rows of d columns must fit into LDS next to the node
 * tables (d <= 441 with 160 KB).  All are asynchronous on the handle's stream and keep no state. */
int bbh_forest_lds_nodes(void);
/* P_dev [T, N]: the prediction of every listed tree for every row (rows of P for trees that are not listed stay untouched).  For small
 * row sets - training inputs, pending rows, read-backs; the only call that writes a [T, N] array. */
int bbh_forest_predict(bbh_handle* h, const double* X_dev, int64_t N, int32_t d, int64_t ldx, const int32_t* meta_dev,
                       const double* tv_dev, const int64_t* off_dev, int64_t T, int64_t n_nodes, const int32_t* order_dev,
                       int64_t n_order, int32_t lds_nodes, double* P_dev);
/* EnsemblePosterior.mean / .variance: mean_dev [N] = sum_t P_t / n, var_dev [N] = sum_t (P_t - mean)^2 / (n - 1) over the n listed
 * trees in their order (two passes), identically 0 for n = 1. */
int bbh_forest_moments(bbh_handle* h, const double* X_dev, int64_t N, int32_t d, int64_t ldx, const int32_t* meta_dev,
                       const double* tv_dev, const int64_t* off_dev, int64_t T, int64_t n_nodes, const int32_t* order_dev,
                       int64_t n_order, int32_t lds_nodes, double* mean_dev, double* var_dev);
/* MC acquisition values of the t-batches [x_i ; pending] under an ensemble posterior whose sample s reads tree idx_s: counts_dev [T]
 * int32 = #{s : idx_s = t} (S in total; the listed trees are those with a count > 0), pend_dev [T, k] = P_t of the k <= 63 pending
 * points.  obj = sign P_t.  BBH_ACQ_QLOGEI: li = log_fatplus(obj - best_f; 1e-6) per point, fatmax over [candidate, pending ...]
 * (tau 1e-2), score = log sum_t counts[t] exp(v_t - M) + M - log S.  BBH_ACQ_QEI ... BBH_ACQ_QPSTD: bbh_mc_utility per point with m =
 * the point's count-weighted sample mean, the maximum over the points, the count-weighted mean.  Rows with alive_dev[i] == 0 score
 * -inf (alive_dev may be null). */
int bbh_forest_mc_acq(bbh_handle* h, int32_t kind, const double* X_dev, int64_t N, int32_t d, int64_t ldx, const int32_t* meta_dev,
                      const double* tv_dev, const int64_t* off_dev, int64_t T, int64_t n_nodes, const int32_t* order_dev,
                      int64_t n_order, int32_t lds_nodes, const int32_t* counts_dev, int64_t S, const double* pend_dev, int64_t k,
                      double best_f, double sign, double beta, const uint8_t* alive_dev, double* scores_dev);

/* ---- Bayesian linear (ARD) surrogate: predictive moments of every row in one pass (bbh_linear.hip) -------------------------------------
 * The device side of BayesianLinearSurrogate (baybe/surrogates/linear.py:62-82): ARDRegression is fitted by scikit-learn on the host;
 * this call replaces model.predict(X, return_std=True) over the candidates.  Of the k <= 512 kept columns (lambda_ < threshold_lambda)
 * cols_dev [k] int32 holds the column of the rows, scale_dev [3, k] the lower bound, the range hi - lo (> 0) and coef_, and T_dev
 * [k, k] the matrix T[i][i] = Ss[i][i], T[i][j] = 2 Ss[i][j] (j < i), 0 above the diagonal, Ss = (sigma_ + sigma_^T) / 2 (entries above
 * the diagonal are not read).  With x~_j = (x[cols_j] - lo_j) / range_j:
 *   mean_dev[i] = ybar + ysd * (sum_j x~_j coef_j + intercept),  var_dev[i] = ysd^2 * (sum_i x~_i sum_{j <= i} T[i][j] x~_j + inv_alpha).
 * form: 0 = by size (register form for k <= 16, block form above: the measured crossover), 1 = register form (one thread per row,
 * k <= 32), 2 = block form
 * (16 rows per wave on v_mfma_f64_16x16x4_f64, any k >= 1).  k = 0 fills the two constants in either form.  Every sum has a fixed
 * order and nothing is contracted: equal rows get equal bits within a form.  Stateless apart from the form of the last call; the
 * launch is asynchronous on the handle's stream after the column list has been read back and checked.  N == 0 is a no-op.  Returns -1
 * with an error text for k < 0, k > 512, form 1 with k > 32, a column index outside [0, d), ldx < d, or a null pointer where one is
 * needed (the outputs; for k > 0 the rows and the tables). */
int bbh_linear_moments(bbh_handle* h, const double* X_dev, int64_t N, int32_t d, int64_t ldx, const int32_t* cols_dev,
                       const double* scale_dev, const double* T_dev, int32_t k, double intercept, double inv_alpha, double ybar, double ysd,
                       int32_t form, double* mean_dev, double* var_dev);
/* Form the last bbh_linear_moments of this handle ran as: 1 = register, 2 = block, -1 = none yet. */
int bbh_linear_last_form(bbh_handle* h);

/* The joint q'-batch and qLogNEHVI kernels split the MC samples into slices when a candidate set alone would not fill the chip; the
 * slice count - and with it the order in which a candidate's partial sums are added - follows the number of candidate rows.
 * rows > 0 fixes the row count the heuristic sees (a row shard passes the GLOBAL count: every rank then adds in the order the
 * unsharded pass uses, so scores are bit-identical across shard layouts); 0 = the rows of each call (default). */
int bbh_set_slice_rows(bbh_handle* h, int64_t rows);

/* Release what an idle handle holds above keep_bytes per buffer: the scratch workspace (bbh_qlogei_pending_big, the materialised
 * K* path), the global kernel-value cache, and the model's matrices (6 np^2 doubles; the next bbh_set_model re-creates them).  No
 * reference counterpart (BayBE holds no device state); called by the host side when a handle goes back to its pool. */
int bbh_trim(bbh_handle* h, int64_t keep_bytes);

/* ---- row-sharded selection over the GPUs of one node (RCCL over xGMI) ---------------------------
 * No reference call site (BayBE is single-process): these belong to the argmax / top-k of
 * optimize_acqf_discrete (baybe/recommenders/pure/bayesian/botorch/discrete.py:120-126) once the candidate rows are
 * sharded contiguously over the ranks.  One collective per selection step; ties resolve to the lowest GLOBAL row index,
 * which follows shard order, i.e. exactly as on a single device.  RCCL is bound at run time (dlopen): without a
 * communicator nothing here is needed. */
/* rank 0: a fresh ncclUniqueId into id_out (bytes >= 128); returns its size, < 0 on error.  Ship it to the other
 * ranks by any means (file, MPI, torch.distributed broadcast). */
int bbh_comm_unique_id(void* id_out, int64_t bytes);
int bbh_comm_init(bbh_handle* h, int32_t rank, int32_t world, const void* unique_id, int64_t bytes);
int bbh_comm_destroy(bbh_handle* h);
/* Global top-k (k <= 64) of the scores of all shards: this rank holds scores_dev [N] for the global rows
 * [row_offset, row_offset + N).  Payload k x (score, global index) built on the device, one ncclAllGather, one
 * read-back; every rank returns the same vals_host / idx_host [k] (descending; (-inf, -1) beyond the total count). */
int bbh_allgather_topk(bbh_handle* h, const double* scores_dev, int64_t N, int64_t row_offset, int64_t k,
                       double* vals_host, int64_t* idx_host);
/* One greedy step: the global first-index argmax and the winner's comp-rep row (row_host [d]; every rank appends it
 * to its pending points).  X_dev [N, ldx] are this rank's rows; an empty shard (N = 0) still takes part. */
int bbh_allgather_argmax(bbh_handle* h, const double* scores_dev, int64_t N, int64_t row_offset, const double* X_dev,
                         int64_t ldx, double* val_host, int64_t* gidx_host, double* row_host);

/* ---- instrumentation --------------------------------------------------------------- */
/* Duration (ms) and launch count of the fused posterior kernel accumulated since the
 * last reset, measured with HIP events on the handle's stream when enabled.
 * enable: 0 = off, 1 = every kernel family, 2 * m = only the families whose bit is set in m (1 << BBH_TIMED_POSTERIOR ...): an event
 * between two back-to-back kernels costs the stream ~5 us, so a timed region brackets only the kernel it reports. */
int bbh_timing_enable(bbh_handle* h, int enable);
int bbh_timing_read(bbh_handle* h, double* fused_ms_total, int64_t* fused_launches, int reset);
/* The same per kernel family: BBH_TIMED_POSTERIOR = variance passes of the fused posterior kernel (what
 * bbh_timing_read reports), BBH_TIMED_CROSS = its mean-only passes (bbh_cross_cov),
 * BBH_TIMED_PENDING = the joint q'-batch acquisition kernels (bbh_qlogei_pending, bbh_mc_acq_pending). */
/* Form of the fused posterior kernel the last variance pass of this handle ran as: 0 = windowed (one wave per 16
 * candidates, bbh_fused_posterior_kernel), 1 = cooperative (one workgroup per 16 candidates, bbh_coop_posterior_kernel),
 * 2 = materialised K* (verification path; models outside the fused forms), 3 = two-sweep cooperative (512 < n <= 1024,
 * bbh_coop2_posterior_kernel), 4 = cooperative with the generic kernel-value production (composite, RQ, piecewise, Linear,
 * Polynomial, Periodic: bbh_coopg_posterior_kernel), 5 = register- / LDS-resident (n <= 128, bbh_small_posterior_kernel),
 * 6 = feature space (BBH_KERNEL_RFF: bbh_rff_posterior_kernel), -1 = none yet. */
int bbh_last_posterior_form(bbh_handle* h);
/* 1 if the last variance pass ran the cooperative form with the seeded distance GEMM (the squared norms as the accumulator's
 * initial value, ceil(d / 4) k-steps), 0 if it ran any other form (BBH_COOP_SEED=0 keeps the augmented stream everywhere). */
int bbh_last_posterior_seeded(bbh_handle* h);
/* Form the last qNEI / qLogNEI scoring pass of this handle ran as: 1 = fused (bbh_score_nei), 2 = unfused (bbh_nei_q1),
 * -1 = none yet. */
int bbh_last_nei_form(bbh_handle* h);
/* Form the last fit evaluation (bbh_fit_value_grad) of this handle ran as, i.e. the path that produced the returned value and gradient
 * (after a give-up of a dataflow launch: the path that redid the evaluation), -1 = none yet. */
enum bbh_fit_form {
  BBH_FIT_FORM_LAUNCH = 0,           /* launch by launch: factorisation, K^-1, value and gradient kernels (bbh_chol_and_alpha + ...) */
  BBH_FIT_FORM_SMALL = 1,            /* np = 64: one workgroup (bbh_fit_small_kernel) */
  BBH_FIT_FORM_TILES_MT = 2,         /* tile-dataflow factorisation building its Gram tiles and all of K^-1's tiles, then the dataflow tail */
  BBH_FIT_FORM_TILES_MT_PARTIAL = 3, /* ... building a part of K^-1's tiles (BBH_TILE_MT=partial beyond co-residency) */
  BBH_FIT_FORM_TILES = 4,            /* ... building its Gram tiles only */
  BBH_FIT_FORM_GRAM_TILES = 5,       /* Gram launch, tile-dataflow factorisation, dataflow tail */
  BBH_FIT_FORM_ONE_LAUNCH = 6,       /* the whole evaluation as one dataflow launch (bbh_fit_flow_kernel) */
  BBH_FIT_FORM_SPLIT = 7,            /* two dataflow launches: factorisation + K^-1, then the rest (BBH_FIT_FLOW=3) */
  BBH_FIT_FORM_RFF = 8,              /* feature-space evaluation of a BBH_KERNEL_RFF model */
  BBH_FIT_FORM_STEPS_TAIL = 9        /* Gram launch, per-step factorisation launches, dataflow tail */
};
int bbh_last_fit_form(bbh_handle* h);
/* How the last bbh_factorize factorised the train covariance (its last attempt): 0 per-step launches (one diagonal-block kernel,
 * panel and trailing update per block row), 1 the one-launch tile-dataflow factorisation (np <= 1024 while its tiles are co-resident);
 * -1 before the first factorisation of a kernel-space model. */
int bbh_last_factor_form(bbh_handle* h);
enum bbh_timed_family {
  BBH_TIMED_POSTERIOR = 0, BBH_TIMED_CROSS = 1, BBH_TIMED_PENDING = 2,
  BBH_TIMED_COLUMNS = 3,  /* bbh_posterior_columns: conditional means under S target columns (qLogNEHVI) */
  BBH_TIMED_NEHVI = 4,    /* bbh_qlognehvi: the scoring kernel over the cells of the box decompositions */
  BBH_TIMED_Q1 = 5,       /* q' = 1 acquisition kernels (bbh_qlogei_q1, bbh_mc_acq_q1) */
  BBH_TIMED_SELECT = 6,   /* chunk keys + the selection kernel (bbh_topk, bbh_argmax, bbh_qlogei_q1_topk) */
  BBH_TIMED_FAMILIES = 7
};
int bbh_timing_read_family(bbh_handle* h, int32_t family, double* ms_total, int64_t* launches, int reset);

/* Diagnostics of the dataflow fit evaluation (declared because the library exports them; scripts/gpu_flow_trace.py,
 * scripts/gpu_tile_stamps.py).  With BBH_FLOW_TRACE=1 / BBH_TILE_STAMPS=1 in the environment the last launch leaves device clock
 * stamps behind: bbh_flow_trace_read copies the per-role stamps [nroles][8] and the role table and returns nroles;
 * bbh_tiles_trace_read the row heads' stamps [tiles][8] of the tile-dataflow factorisation and returns the tile count.  -1 when no
 * trace exists or cap is too small.  No reference counterpart (baybe has no native code). */
int bbh_flow_trace_read(bbh_handle* h, long long* stamps_host, int* roles_host, int cap);
int bbh_tiles_trace_read(bbh_handle* h, long long* stamps_host, int cap);

#ifdef __cplusplus
}
#endif
#endif /* BAYBE_HIP_H */
