"""qLogNParEGO on the HIP path (``baybe/acquisition/acqfs.py:328-336``; built with ``X_baseline`` = all training inputs and
``prune_baseline`` at ``baybe/acquisition/_builder.py:319-324``).

BoTorch's qLogNParEGO is qLogNoisyExpectedImprovement under an augmented Chebyshev scalarisation of the m targets: per MC sample the
candidate is drawn *jointly* with the baseline through the cached factor, both are scalarised, and the improvement of the candidate
over that sample's best scalarised baseline value is scored.  It needs neither fantasies nor integration points - the set-up is
qLogNEHVI's (``baybe_amd/nehvi.py``: one extended model per target, device-side Sobol draw, per-target streams, greedy loop, shards)
without the box decompositions, and the finish is qLogNEI's (``baybe_amd/nei.py``).  ``HipNEHVI`` with three methods replaced:

    weights   w on the simplex: given (``scalarization_weights``), or ``draw_scalarization_weights`` when the acquisition function
              is built - BEFORE the scoring and pruning seeds are drawn
    bounds    Y = oriented posterior means of the m targets at ALL baseline rows (before pruning); lo = min_b Y, hi = max_b Y
              (one row: hi = lo + 1; a zero range counts as 1)
    g(y)      t_o = w_o (hi_o - y_o) / (hi_o - lo_o),  g = -(max_o t_o + 0.05 sum_o t_o)   (augmented Chebyshev, alpha = 0.05)
    pruning   keep a baseline row iff it is the first-index argmax of g in at least one of 2048 joint draws
              (``prune_inferior_points`` under the scalarisation; ``bbh_scalarized_best_frequency_dev`` on qLogNEHVI's pruning draw)
    set-up    extended models + ``bbh_nehvi_samples`` (oriented baseline samples F_b [S, nb, m], S weight columns per target), then
              ``best_s = max_b g(F_b[s, b, :])`` (``bbh_scalarized_best_dev``)
    scoring   ``f_s,o = sign_o (E[f_o(x) | D, F_b,s,o] + safe_sd(v_o) z_x,s,o)``,  ``u_s = g(f_s) - best_s``,
              score = logmeanexp_s log_fatplus(u_s; 1e-6)   (``bbh_nparego_q1``)

The scoring pass walks the candidates in chunks: each target's variance pass runs over all rows once, then per chunk the m
``bbh_posterior_columns_sm`` launches run on the targets' streams, are joined, and one ``bbh_nparego_q1`` scores the chunk from the m
reused ``[S, chunk]`` buffers - together at most ``CHUNK_BYTES``, so memory does not grow with the candidate count (unchunked, 1e6
rows x 512 samples x 3 targets would be 12 GB).  A row's score does not depend on the chunk it sits in (the kernel's sample slices
have a fixed length), so a chunked pass equals the one-chunk pass bit for bit.

Greedy batches: picks and pending experiments join the baseline (``HipNEHVI.greedy``): q' = 1 always, no cap on the batch size."""

from __future__ import annotations

import ctypes as C

import numpy as np

from baybe_amd import _lib
from baybe_amd.engine import _dp, _native_sobol_usable, draw_sampler_seed, sobol_normal_base_samples
from baybe_amd.nehvi import PRUNE_SAMPLES, HipNEHVI, _unique_rows

# The m [S, chunk] blocks of conditional means of one chunk, together.  An UNMEASURED placeholder from the Infinity-Cache hypothesis alone
# (KERNELS §4.4c): scripts/gpu_nparego_pass.py is the measurement that has to set it, and it has not been run on a device yet.
CHUNK_BYTES = 96 << 20


def draw_scalarization_weights(m: int, agree=None) -> np.ndarray:
    """``sample_simplex(m)``: m - 1 uniform values in double precision from torch's global generator, sorted; the differences of
    [0, ..., 1] are the weights.  ``agree`` (``RowShard.agree``): rank 0's draw on every rank, like the sampler seeds."""
    import torch

    cuts = np.sort(torch.rand(max(int(m) - 1, 0), dtype=torch.float64).numpy())
    w = np.diff(np.concatenate([[0.0], cuts, [1.0]]))
    return np.asarray(agree(w), dtype=np.float64) if agree is not None else w


def check_weights(weights, m: int) -> np.ndarray:
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if len(w) != m or not np.isfinite(w).all() or (w < 0).any() or abs(w.sum() - 1.0) > 1e-9:
        raise ValueError(f"scalarization weights must be {m} non-negative values that sum to 1, got {weights!r}")
    return w


def scalarization_bounds(Y: np.ndarray):
    """(hi [m], hi - lo [m]) of the oriented baseline means Y [nb, m]."""
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    if len(Y) == 1:
        hi = lo + 1.0
    rng = hi - lo
    rng[rng == 0.0] = 1.0
    return hi, rng


class HipNParEGO(HipNEHVI):
    """qLogNParEGO scorer over m independent HIP GPs (q = 1 t-batches; pending points and picks join the baseline).  Same surface as
    ``HipNEHVI``: ``prepare`` / ``score`` / ``greedy``, ``outputs``, ``X_b_current``, ``_pruned``."""

    def __init__(self, engines, signs, X_baseline, weights, n_mc_samples: int = 512, prune_baseline: bool = True, device: int = 0):
        if any(getattr(e.spec, "kernel", None) == "rff" for e in engines):
            from baybe_amd.exceptions import IncompatibilityError

            # (the extended models condition on noise-free latent rows, which the RFF kernel's uniform-noise feature-space form does not have)
            raise IncompatibilityError("qLogNParEGO is not available with an RFFKernel surrogate on the HIP path.")
        super().__init__(engines, signs, X_baseline, ref_point=[-np.inf] * len(engines), n_mc_samples=n_mc_samples,
                         prune_baseline=prune_baseline, device=device)
        self.weights = check_weights(weights, self.m)
        self.device_setup = True  # (there is no host form of this set-up)
        self._hi = self._inv = None
        self._best = self._Fb = self._zx_dev = None

    # ---- set-up ----------------------------------------------------------------------------------
    def _scalarization(self):
        """(w, hi, 1 / (hi - lo)) as ctypes pointers; the bounds come from the fitted models' means at all baseline rows, once."""
        if self._hi is None:
            Y = np.stack([out.sign * out.engine.posterior(self.X_baseline)[0].cpu().numpy() for out in self.outputs], axis=1)
            hi, rng = scalarization_bounds(Y)
            self._hi, self._inv = np.ascontiguousarray(hi), np.ascontiguousarray(1.0 / rng)
        return _dp(self.weights), _dp(self._hi), _dp(self._inv)

    def prune_points(self, Xb: np.ndarray, seed: int) -> np.ndarray:
        """Keep the baseline points whose scalarised value is the largest in at least one of 2048 joint posterior samples, in their
        original order.  Ties go to the lowest index, so of a repeated point (one latent value, ``_unique_rows``) the first copy is
        the one that can be kept."""
        Xb_all = Xb
        Xb, first, _ = _unique_rows(Xb_all)
        nb = len(Xb)
        draw_on_device = self.device_draw and _native_sobol_usable()
        if draw_on_device:
            z = self.outputs[0].ext.sobol_normal_dev(PRUNE_SAMPLES, len(Xb_all) * self.m, seed)
        else:
            z = sobol_normal_base_samples(PRUNE_SAMPLES, len(Xb_all) * self.m, seed).reshape(PRUNE_SAMPLES, len(Xb_all), self.m)
            if nb < len(Xb_all):
                z = np.ascontiguousarray(z[:, first, :])
        obj_dev = self._baseline_samples_dev(Xb, z, want_columns=False, S=PRUNE_SAMPLES, first=first if draw_on_device else None)
        counts = np.zeros(nb, dtype=np.int64)
        h = self.outputs[0].ext
        h._check(self._lib.bbh_scalarized_best_frequency_dev(h._h, obj_dev.data_ptr(), PRUNE_SAMPLES, nb, self.m, *self._scalarization(),
                                                             counts.ctypes.data_as(_lib.c_int64_p)), "bbh_scalarized_best_frequency_dev")
        return Xb_all[first[counts > 0]]

    def prepare(self, seed: int, extra_baseline: np.ndarray | None = None, prune_seed: int | None = None):
        """Sample the baseline, take the per-sample best scalarised value, and condition the per-target models (one selection step)."""
        import torch

        if not len(self.X_baseline):
            raise ValueError("qLogNParEGO needs at least one baseline point.")
        scal = self._scalarization()
        if self._pruned is None:  # pruning happens once, when the acquisition function is built
            Xb0 = self.X_baseline
            if self.prune:
                Xb0 = self.prune_points(Xb0, draw_sampler_seed() if prune_seed is None else prune_seed)
            self._pruned = Xb0
        Xb = self._pruned
        if extra_baseline is not None and len(extra_baseline):
            Xb = np.vstack([Xb, np.atleast_2d(extra_baseline)])  # picks and pending points join the baseline
        Xb_all = Xb
        z = self._base_samples(self.S, len(Xb_all), seed)  # [S, nb + 1, m], the candidate's row last
        self.zx = np.ascontiguousarray(z[:, len(Xb_all), :])
        Xb, first, _ = _unique_rows(Xb_all)
        nb = len(Xb)
        if nb < len(Xb_all):  # repeated baseline points: one latent value each (their base-sample columns stay counted)
            z = np.ascontiguousarray(z[:, np.concatenate([first, [len(Xb_all)]]), :])
        self._Fb = self._baseline_samples_dev(Xb, z, want_columns=True)  # [S, nb, m] oriented baseline samples
        self._zx_dev = torch.from_numpy(self.zx).to(self._Fb.device)  # [S, m]: uploaded once per step, read by every chunk's kernel
        h = self.outputs[0].ext
        self._best = torch.empty(self.S, dtype=torch.float64, device=self._Fb.device)
        h._check(self._lib.bbh_scalarized_best_dev(h._h, self._Fb.data_ptr(), self.S, nb, self.m, *scal, self._best.data_ptr()),
                 "bbh_scalarized_best_dev")
        self.X_b_current = Xb_all
        self._prepared = True

    # ---- scoring ---------------------------------------------------------------------------------
    def score(self, X_dev, alive=None, sync: bool = True):
        import torch

        assert self._prepared, "call prepare() first"
        h = self.outputs[0].ext
        X_dev = h._as_dev(X_dev)
        N = X_dev.shape[0]
        scores = torch.empty(N, dtype=torch.float64, device=X_dev.device)
        chunk = max(1, min(N, CHUNK_BYTES // (8 * self.S * self.m)))
        bufs = [torch.empty(self.S * chunk, dtype=torch.float64, device=X_dev.device) for _ in self.outputs]  # [S, c] sample-major, c <= chunk
        # Every extended model's handle is bound to its target's stream (``_target_streams``): the library calls below enqueue there,
        # whichever stream is torch's current one.  All tensors of the pass are allocated here, on the current stream.
        streams = self._target_streams(X_dev.device)
        if streams:
            cur = torch.cuda.current_stream(X_dev.device)
            for st in streams:
                st.wait_stream(cur)
        vars_ = []
        for out in self.outputs:  # each target's variance pass over all rows, once
            mean, var = (torch.empty(N, dtype=torch.float64, device=X_dev.device) for _ in range(2))
            out.ext.posterior(X_dev, out=(mean, var))
            vars_.append((mean, var))
        sg = np.ascontiguousarray(self.signs)
        w, hi, inv = self._scalarization()
        tp = (C.c_void_p * self.m)(*[b.data_ptr() for b in bufs])
        for c0 in range(0, N, chunk):
            c1 = min(N, c0 + chunk)
            Xc = X_dev[c0:c1]
            for o, out in enumerate(self.outputs):
                if streams and o:  # the scoring kernel of the previous chunk (first target's stream) has read this buffer
                    streams[o].wait_stream(streams[0])
                out.ext._check(self._lib.bbh_posterior_columns_sm(out.ext._h, Xc.data_ptr(), c1 - c0, Xc.stride(0), bufs[o].data_ptr()),
                               "bbh_posterior_columns_sm")
            for st in streams[1:]:
                streams[0].wait_stream(st)
            vp = (C.c_void_p * self.m)(*[v[c0:c1].data_ptr() for _, v in vars_])
            h._check(self._lib.bbh_nparego_q1(h._h, self.m, c1 - c0, tp, vp, _dp(sg), self._zx_dev.data_ptr(), self.S, w, hi, inv, self._best.data_ptr(),
                                              alive[c0:c1].data_ptr() if alive is not None else None, scores[c0:c1].data_ptr()),
                     "bbh_nparego_q1")
        if sync:
            torch.cuda.synchronize(X_dev.device)  # the buffers must outlive the kernels
        else:
            self._keep = (bufs, vars_)  # (the caller synchronises; the operands live until the next pass)
        return scores
