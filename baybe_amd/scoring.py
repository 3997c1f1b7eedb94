"""The one surface every acquisition scorer of the recommender has, and the scorer of the single-target paths.

``HipRecommenderImpl._setup_acqf`` puts exactly one scorer into ``_scorer`` (chosen by ``recommenders._choose_scorer``) and the
recommender asks it one question per public call:

* ``select(X, q, *, seeds, X_pending=None, alive=None, shard=None) -> GreedyResult`` - the greedy batch of ``recommend``;
* ``values(X, *, seeds, X_pending=None) -> fp64 device tensor [N]`` - ``acquisition_values``;
* ``joint_value(batch, *, seeds, X_pending=None) -> float`` - ``joint_acquisition_value`` and the subset ranking;
* ``check_request(batch_size, n_pend, acqf, program, model)`` (static, asked before anything is fitted) - the path's batch cap;
* ``supports_continuous`` - whether the hybrid / continuous search may drive the scorer (``HipSingleTargetAcq.scores``).

``seeds`` is the recommender's seed source (``_sampler_seed``): every call draws the next MC sampler seed from torch's global
generator, and with row shards returns rank 0's draw; ``seeds(agree=False)`` is the local draw, for the one draw that was never
agreed (the pruning seed of a read-back).  A scorer draws what its path needs, in a fixed order, from that callable alone - the
draws decide the recommendation, so their order is behaviour - and refuses what it cannot serve itself.  The lower-level
methods underneath (``greedy(..., seed=)``, ``prepare``, ``score``, ``gain``, ``cells``) take explicit seeds and stay public.

The scorers: ``HipSingleTargetAcq`` (here), ``nehvi.HipNEHVI`` / ``HipNEHVIPlain``, ``nparego.HipNParEGO``, ``nei.HipNEI``,
``ehvi.HipEHVI``, ``nipv.HipNIPV``, ``desirability.HipDesirability``, ``forest.HipForestAcq``, ``linear.HipLinearAcq`` /
``HipLinearAnalytic``."""

from __future__ import annotations

import numpy as np

from baybe_amd import _lib
from baybe_amd.engine import GreedyResult, sobol_normal_base_samples
from baybe_amd.exceptions import IncompatibilityError, IncompatibleAcquisitionFunctionError


def refuse_shard(shard, text: str) -> None:
    """A scorer without a row-sharded form says so (the recommender raises the same ``text`` before anything is fitted)."""
    if shard is not None:
        raise IncompatibilityError(text)


def check_joint_batch(batch_size, n_pend, acqf, program=None, model=None) -> None:
    """The joint q'-batch kernels hold 1 + (pending + earlier picks) <= 16 points; the reference has no such limit, so say so
    before any candidate is scored.  qLogEI: up to 64 points (beyond 16 through bbh_qlogei_pending_big, the factor in a global
    workspace); the other MC acquisition functions, and every one under an objective program (bbh_mc_acq_obj_pending): 16.
    Analytic functions have q = 1."""
    if getattr(acqf, "is_analytic", False):
        return
    big = getattr(acqf, "kind", None) == "qLogEI" and program is None
    cap = (_lib.MAX_PENDING_BIG if big else _lib.MAX_PENDING) + 1
    if batch_size + n_pend > cap:
        raise IncompatibilityError(
            f"batch_size ({batch_size}) + pending experiments ({n_pend}) exceeds {cap}, the largest "
            f"joint q-batch of the HIP kernels; recommend in smaller batches (marking earlier ones as pending)."
        )


def no_batch_cap(batch_size, n_pend, acqf, program=None, model=None) -> None:
    """The ``check_request`` of the scorers that cache pending points and picks into their baseline: any batch size."""


class HipSingleTargetAcq:
    """MC and analytic acquisition functions of ONE model with a Gaussian posterior per point (``HipGP``, and the moments of the
    forest / linear engines for the analytic kinds).  ``sign`` is the target's orientation, or +1 where the objective ``program``
    carries it; an affine program is the reference's posterior transform for the analytic kinds."""

    supports_continuous = True
    check_request = staticmethod(check_joint_batch)

    def __init__(self, engine, acqf, sign: float, best_f: float, program=None):
        self.engine, self.acqf, self.sign, self.best_f, self.program = engine, acqf, float(sign), best_f, program
        self.beta = getattr(acqf, "beta", 0.2)

    def analytic_scores(self, mean, var, alive=None):
        sign = self.sign
        if self.program is not None:
            # an affine objective is the reference's posterior transform (objectives/single.py:77-91): N(a mu + b, a^2 sigma^2)
            a, b = self.program.as_affine()
            mean, var, sign = a * mean + b, (a * a) * var, 1.0
        return self.engine.analytic_acq(self.acqf.kind, mean, var, self.best_f, sign, self.beta,
                                        getattr(self.acqf, "maximize", True), alive)

    def mc_scores(self, X, mean, var, pend, seed):
        """MC acquisition values of the t-batches [x_i ; pend].  Up to 15 pending rows ride on the handle's pending state; beyond
        that (qLogEI only, up to 63 - the same limit ``check_joint_batch`` admits for recommend()) the columns come from
        ``cross_cov_many`` and the joint kernel takes the pending statistics explicitly, as in the greedy loop."""
        eng, acqf, prog = self.engine, self.acqf, self.program
        okw = {} if prog is None else {"objective": prog}
        if len(pend) == 0:
            z = sobol_normal_base_samples(acqf.n_mc_samples, 1, seed)[:, 0]
            return eng.mc_acq(acqf.kind, mean, var, z, self.best_f, self.sign, self.beta, **okw)
        z = sobol_normal_base_samples(acqf.n_mc_samples, 1 + len(pend), seed)
        if len(pend) > _lib.MAX_PENDING:
            if prog is not None:
                raise IncompatibilityError(
                    f"{len(pend)} pending / batch rows exceed the largest joint q-batch of the HIP kernels for a transformed target "
                    f"({_lib.MAX_PENDING + 1} points).")
            if acqf.kind != "qLogEI" or len(pend) > _lib.MAX_PENDING_BIG:
                raise IncompatibilityError(
                    f"{len(pend)} pending / batch rows exceed the largest joint q-batch of the HIP kernels for '{type(acqf).__name__}' "
                    f"({_lib.MAX_PENDING_BIG + 1} points for qLogEI, {_lib.MAX_PENDING + 1} otherwise).")
            cross = eng.cross_cov_many(X, pend)
            s = eng.qlogei_pending_big(mean, var, cross, pend, z, self.best_f, self.sign)
        else:
            stats = eng.set_pending(pend)
            cross = eng.cross_cov(X)
            if prog is not None:
                okw["stats"] = stats
            s = eng.mc_acq(acqf.kind, mean, var, z, self.best_f, self.sign, self.beta, cross=cross, **okw)
        eng.set_pending(None)
        return s

    def scores(self, X, mean, var, pend, seed):
        """Scores of arbitrary rows ``X`` given their moments, the pending rows and the sampler seed: the step function of the
        hybrid / continuous search (same base samples for every evaluation)."""
        if self.acqf.is_analytic:
            if len(pend):
                raise IncompatibleAcquisitionFunctionError("Analytic acquisition functions score single points only.")
            return self.analytic_scores(mean, var)
        return self.mc_scores(X, mean, var, pend, seed)

    def select(self, X, q, *, seeds, X_pending=None, alive=None, shard=None) -> GreedyResult:
        eng, acqf = self.engine, self.acqf
        if acqf.is_analytic:  # q = 1 by construction (supports_batching is False); no sampler, no seed
            val, idx = eng.argmax(self.analytic_scores(*eng.posterior(X), alive))
            if shard is not None:
                val, idx, _ = shard.global_argmax(val, idx, X)
            return GreedyResult([int(idx)], [float(val)])
        return eng.greedy_qlogei(
            X, q, S=acqf.n_mc_samples, seed=seeds(), sign=self.sign, X_pending=X_pending, best_f=self.best_f, shard=shard,
            kind=acqf.kind, beta=self.beta, alive=alive, **({} if self.program is None else {"objective": self.program}),
        )

    def values(self, X, *, seeds, X_pending=None):
        mean, var = self.engine.posterior(X)
        if self.acqf.is_analytic:
            return self.analytic_scores(mean, var)
        pend = X_pending if X_pending is not None else np.zeros((0, X.shape[1]))
        return self.mc_scores(X, mean, var, pend, seeds())

    def joint_value(self, batch, *, seeds, X_pending=None) -> float:
        """The value of one q-batch (candidate = first row, the others enter as pending rows)."""
        base = X_pending if X_pending is not None else np.zeros((0, batch.shape[1]))
        pend = np.vstack([batch[1:], base])
        seed = seeds()  # (drawn for the analytic kinds too, which do not use it)
        mean, var = self.engine.posterior(batch[:1])
        return float(self.scores(batch[:1], mean, var, pend, seed).cpu().numpy()[0])
