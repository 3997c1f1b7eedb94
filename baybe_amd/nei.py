"""qNoisyExpectedImprovement / qLogNoisyExpectedImprovement on the HIP path (``baybe/acquisition/acqfs.py:226-243``; built with
``X_baseline`` = all training inputs and ``prune_baseline`` at ``baybe/acquisition/_builder.py:319-324``).

The noisy forms of expected improvement do not compare against one incumbent value: per MC sample BoTorch draws f(x) *jointly*
with the baseline values f(X_b) through a cached Cholesky root and scores the improvement over that sample's own best baseline
value.  This is qLogNEHVI (``baybe_amd/nehvi.py``) with one target and without box decompositions, and the driver is that
class with three methods replaced:

    pruning   keep a baseline row iff it is the best of at least one of 2048 joint draws (``prune_inferior_points``;
              ``bbh_best_frequency_dev`` on the same device draw as the qLogNEHVI pruning; ties go to the first index)
    set-up    extended model + ``bbh_nehvi_samples`` with m = 1 (oriented baseline samples, S weight columns), then
              ``best_s = max_b F_b,s`` on the device (``bbh_sample_best_dev``)
    scoring   ``f_s = E[f(x) | D, F_b,s] + safe_sd(Var[f(x) | D, X_b]) z_x,s``,  ``u_s = sign f_s - best_s``;
              qLogNEI = logmeanexp_s log_fatplus(u_s; 1e-6) (the q = 1 form of qLogEI), qNEI = mean_s max(u_s, 0)

The scoring pass is one fused kernel (``bbh_score_nei``: the cooperative conditional-mean kernel with a scoring epilogue) - for
S <= 512 its accumulators hold a candidate's whole sample axis, so the ``[S, N]`` matrix of conditional means that qLogNEHVI
materialises per target (4.1 GB at 1e6 candidates, S = 512) never exists.  Where that form does not apply (composite-kernel
models, S > 512, ``BBH_NEI_FUSED=0``) the candidates go through ``bbh_posterior_columns_sm`` + ``bbh_nei_q1`` in chunks of at
most ``UNFUSED_CHUNK_BYTES`` of conditional means.

Greedy batches: each pick and every pending experiment joins the baseline (BoTorch's ``set_X_pending`` with a cached root,
``HipNEHVI.greedy``) - there is no joint q' kernel and therefore no cap on the batch size.

Multi-task (ICM) surrogates: the extended model carries the task column like any other input column (``bbh_set_model_ex``), the
baseline rows keep their tasks; pinned by one parity case in ``tests/test_nei_gpu.py``."""

from __future__ import annotations

import numpy as np

from baybe_amd import _lib
from baybe_amd.engine import _native_sobol_usable, draw_sampler_seed, sobol_normal_base_samples
from baybe_amd.nehvi import PRUNE_SAMPLES, HipNEHVI, _unique_rows

UNFUSED_CHUNK_BYTES = 256 << 20  # conditional means of one chunk of the unfused form ([S, chunk] doubles)


class HipNEI(HipNEHVI):
    """qNEI / qLogNEI scorer over one HIP GP (q = 1 t-batches; pending points and picks join the baseline).  Same surface as
    ``HipNEHVI``: ``prepare`` / ``score`` / ``greedy``, ``outputs``, ``X_b_current``, ``_pruned``."""

    def __init__(self, engine, sign, X_baseline, n_mc_samples: int = 512, prune_baseline: bool = True, log: bool = True,
                 device: int = 0):
        if getattr(engine.spec, "kernel", None) == "rff":
            from baybe_amd.exceptions import IncompatibilityError

            # (the extended model conditions on noise-free latent rows, which the RFF kernel's uniform-noise feature-space form does not have)
            raise IncompatibilityError("qNEI / qLogNEI are not available with an RFFKernel surrogate on the HIP path.")
        super().__init__([engine], [sign], X_baseline, ref_point=[-np.inf], n_mc_samples=n_mc_samples,
                         prune_baseline=prune_baseline, device=device)
        self.log = bool(log)
        self.kind = _lib.ACQ_KINDS["qLogNEI" if self.log else "qNEI"]
        self.device_setup = True  # (there is no host form of this set-up)
        self._best = self._Fb = None
        self.last_form = None  # "fused" / "unfused": what the last scoring pass ran as (bbh_last_nei_form)

    # ---- set-up ----------------------------------------------------------------------------------
    def prune_points(self, Xb: np.ndarray, seed: int) -> np.ndarray:
        """Keep the baseline points that are the best in at least one of 2048 joint posterior samples (``prune_inferior_points``),
        in their original order.  Ties go to the lowest index, so of a repeated point (one latent value, ``_unique_rows``) the first
        copy is the one that can be kept."""
        Xb_all = Xb
        Xb, first, _ = _unique_rows(Xb_all)
        nb = len(Xb)
        draw_on_device = self.device_draw and _native_sobol_usable()
        if draw_on_device:
            z = self.outputs[0].ext.sobol_normal_dev(PRUNE_SAMPLES, len(Xb_all), seed)
        else:
            z = sobol_normal_base_samples(PRUNE_SAMPLES, len(Xb_all), seed).reshape(PRUNE_SAMPLES, len(Xb_all), 1)
            if nb < len(Xb_all):
                z = np.ascontiguousarray(z[:, first, :])
        obj_dev = self._baseline_samples_dev(Xb, z, want_columns=False, S=PRUNE_SAMPLES, first=first if draw_on_device else None)
        counts = np.zeros(nb, dtype=np.int64)
        h = self.outputs[0].ext
        h._check(self._lib.bbh_best_frequency_dev(h._h, obj_dev.data_ptr(), PRUNE_SAMPLES, nb, counts.ctypes.data_as(_lib.c_int64_p)),
                 "bbh_best_frequency_dev")
        return Xb_all[first[counts > 0]]

    def prepare(self, seed: int, extra_baseline: np.ndarray | None = None, prune_seed: int | None = None):
        """Sample the baseline, take the per-sample best, and condition the model (one selection step)."""
        import torch

        if self._pruned is None:  # pruning happens once, when the acquisition function is built
            Xb0 = self.X_baseline
            if self.prune and len(Xb0):
                Xb0 = self.prune_points(Xb0, draw_sampler_seed() if prune_seed is None else prune_seed)
            self._pruned = Xb0
        Xb = self._pruned
        if extra_baseline is not None and len(extra_baseline):
            Xb = np.vstack([Xb, np.atleast_2d(extra_baseline)])  # picks and pending points join the baseline
        Xb_all = Xb
        z = self._base_samples(self.S, len(Xb_all), seed)  # [S, nb + 1, 1], the candidate's column last
        self.zx = np.ascontiguousarray(z[:, len(Xb_all), 0])
        Xb, first, _ = _unique_rows(Xb_all)
        nb = len(Xb)
        if nb < len(Xb_all):  # repeated baseline points: one latent value each (their base-sample columns stay counted)
            z = np.ascontiguousarray(z[:, np.concatenate([first, [len(Xb_all)]]), :])
        self._Fb = self._baseline_samples_dev(Xb, z, want_columns=True)  # [S, nb, 1] oriented baseline samples
        h = self.outputs[0].ext
        self._best = torch.empty(self.S, dtype=torch.float64, device=self._Fb.device)
        h._check(self._lib.bbh_sample_best_dev(h._h, self._Fb.data_ptr(), self.S, nb, self._best.data_ptr()), "bbh_sample_best_dev")
        self.X_b_current = Xb_all
        self._prepared = True

    # ---- scoring ---------------------------------------------------------------------------------
    def score(self, X_dev, alive=None, sync: bool = True):
        import torch

        assert self._prepared, "call prepare() first"
        h = self.outputs[0].ext
        X_dev = h._as_dev(X_dev)
        N = X_dev.shape[0]
        _, var = h.posterior(X_dev)
        scores = torch.empty(N, dtype=torch.float64, device=X_dev.device)
        zx = _lib_dp(self.zx)
        sign = float(self.signs[0])
        alive_ptr = alive.data_ptr() if alive is not None else None
        rc = self._lib.bbh_score_nei(h._h, self.kind, X_dev.data_ptr(), N, X_dev.stride(0), var.data_ptr(), zx, self.S,
                                     self._best.data_ptr(), sign, alive_ptr, scores.data_ptr())
        keep = [var]
        if rc == 1:  # the fused form does not apply
            keep.append(self._score_unfused(X_dev, var, alive, scores))
        else:
            h._check(rc, "bbh_score_nei")
        self.last_form = {1: "fused", 2: "unfused"}.get(self._lib.bbh_last_nei_form(h._h))
        if sync:
            torch.cuda.synchronize(X_dev.device)
        else:
            self._keep = keep  # (the caller synchronises; the operands live until the next pass)
        return scores

    def _score_unfused(self, X_dev, var, alive, scores):
        """The unfused form: conditional means of one chunk of candidates at a time (``bbh_posterior_columns_sm``), then
        ``bbh_nei_q1`` on them.  One buffer of at most ``UNFUSED_CHUNK_BYTES`` serves every chunk - the handle's kernels run in
        the order they were enqueued, whichever stream the handle is bound to, so a chunk's means are scored before the next
        chunk overwrites them.  Returns that buffer: it must outlive the pass."""
        import torch

        h = self.outputs[0].ext
        N = X_dev.shape[0]
        chunk = max(1, min(N, max(1024, UNFUSED_CHUNK_BYTES // (8 * self.S))))
        buf = torch.empty(self.S * chunk, dtype=torch.float64, device=X_dev.device)  # [S, c] sample-major, c <= chunk
        zx = _lib_dp(self.zx)
        for c0 in range(0, N, chunk):
            c1 = min(N, c0 + chunk)
            Xc = X_dev[c0:c1]
            h._check(self._lib.bbh_posterior_columns_sm(h._h, Xc.data_ptr(), c1 - c0, Xc.stride(0), buf.data_ptr()),
                     "bbh_posterior_columns_sm")
            h._check(
                self._lib.bbh_nei_q1(h._h, self.kind, buf.data_ptr(), var[c0:c1].data_ptr(), c1 - c0, zx, self.S,
                                     self._best.data_ptr(), float(self.signs[0]), alive[c0:c1].data_ptr() if alive is not None else None,
                                     scores[c0:c1].data_ptr()),
                "bbh_nei_q1",
            )
        return buf


def _lib_dp(a: np.ndarray):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_lib.c_double_p)
