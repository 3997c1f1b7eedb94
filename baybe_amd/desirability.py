"""``DesirabilityObjective`` with one surrogate per target (the reference's default, ``as_pre_transformation=False``) on the HIP path.

In the reference every target gets its own model (``surrogates/composite.py``) and the desirability score is computed per posterior
sample, as an MC objective in front of the acquisition utility (``objectives/desirability.py:229-264``): the oriented
transformation of every target (``_oriented_targets``: a minimised target is ``t.negate() + 1``, lines 206-215), then the weighted
arithmetic or geometric mean.  Here the objective is walked once on the host into a ``DesirabilityProgram`` - one
``ObjectiveProgram`` per target, the normalised weights, the scalariser - which ``csrc/bbh_desirability.hip`` evaluates between the
T joint draws and the utility.  ``DesirabilityProgram.apply`` is the numpy interpreter of the same description (``best_f``).

``HipDesirability`` is the scorer the recommender puts into the slot of the other device scorers: the T posterior passes stay
resident as ``[T, N]``, every greedy step adds the picks' cross-covariances per target, and one ``desirability_acq`` call scores all
candidates.  Analytic acquisition functions do not come here: an arithmetic mean of affine targets is Gaussian
(``to_botorch_posterior_transform``, lines 266-320) and goes through ``DesirabilityProgram.as_affine``."""

from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from baybe_amd.engine import GreedyResult, draw_sampler_seed, sobol_normal_base_samples
from baybe_amd.exceptions import IncompatibilityError, IncompatibleAcquisitionFunctionError
from baybe_amd.objective import MAX_OPS, ObjectiveProgram, _fold, _walk
from baybe_amd.scoring import check_joint_batch, refuse_shard

MAX_TARGETS = 8  # BBH_DES_MAX_TARGETS
SCALARIZERS = {"MEAN": 0, "GEOM_MEAN": 1}  # enum bbh_scalarizer
SHARD_TEXT = ("Row shards are not on the HIP path of desirability objectives with one model per target; score them on one "
              "device, or use 'DesirabilityObjective(as_pre_transformation=True)'.")
EPS = 2.0**-52  # torch.finfo(float64).eps: the reference's guard inside the logarithm (objectives/desirability.py:62-64)


@dataclass(frozen=True)
class DesirabilityProgram:
    """``programs``: one ``ObjectiveProgram`` per target (the oriented transformation); ``normalized_weights``; ``scalarizer``:
    "MEAN" or "GEOM_MEAN".  ``posterior_terms``: per target the (factor, shift) of ``to_botorch_posterior_transform`` - the target's
    own affine map, negated if minimised (without the + 1 of the oriented target) - or None where a target is not affine."""

    programs: tuple
    normalized_weights: tuple
    scalarizer: str
    posterior_terms: tuple | None = None

    @property
    def n_targets(self) -> int:
        return len(self.programs)

    def apply(self, Y: np.ndarray) -> np.ndarray:
        """Y [..., T] target values -> [...] desirability values; the sum runs in ascending t with rounded products, as on the device."""
        Y = np.asarray(Y, dtype=np.float64)
        acc = np.zeros(Y.shape[:-1])
        with np.errstate(all="ignore"):
            for t, (prog, w) in enumerate(zip(self.programs, self.normalized_weights)):
                g = prog.apply(Y[..., t])
                acc = acc + w * (np.log(g + EPS) if self.scalarizer == "GEOM_MEAN" else g)
            return np.exp(acc) if self.scalarizer == "GEOM_MEAN" else acc

    def as_affine(self):
        """(c [T], offset) with desirability = sum_t c_t y_t + offset if the scalariser is the arithmetic mean and every target's
        program is one affine map - the case in which the reference hands analytic acquisition functions a posterior transform
        (``to_botorch_posterior_transform``) - else None."""
        if self.scalarizer != "MEAN" or self.posterior_terms is None or any(p.as_affine() is None for p in self.programs):
            return None
        w = np.asarray(self.normalized_weights, dtype=np.float64)
        c = np.array([wt * a for wt, (a, _) in zip(w, self.posterior_terms)])
        return c, float(sum(wt * b for wt, (_, b) in zip(w, self.posterior_terms)))

    def to_struct(self):
        """``bbh_desirability`` for the C-ABI."""
        from baybe_amd import _lib

        des = _lib.Desirability()
        des.n_targets, des.scalarizer = self.n_targets, SCALARIZERS[self.scalarizer]
        for t, (prog, w) in enumerate(zip(self.programs, self.normalized_weights)):
            des.weight[t] = float(w)
            des.prog[t] = prog.to_struct()
        return des


def _target_ops(transformation, negate_plus_one: bool, name: str) -> tuple:
    ops: list = []
    if transformation is not None:
        _walk(transformation, ops)
    if negate_plus_one:
        ops.append(("AFFINE", (-1.0, 1.0)))
    ops = _fold(ops)  # (an identity comes out as the one-operation program AFFINE(1, 0))
    if len(ops) > MAX_OPS:
        raise IncompatibilityError(
            f"The transformation of target '{name}' needs {len(ops)} operations after folding; the HIP kernels evaluate at most "
            f"{MAX_OPS}. Use BotorchRecommender."
        )
    return tuple(ops)


def desirability_program(objective) -> DesirabilityProgram:
    """The ``DesirabilityProgram`` of a ``DesirabilityObjective`` (recognised by its attributes, like the transformations: no import
    of BayBE).  Each target's program comes from the transformation of the reference's oriented target alone - a minimised target
    there is ``t.negate() + 1`` and still reports ``minimize=True``, so going through ``objective_program`` would negate it a second
    time.  Stand-ins without ``_oriented_targets`` get their transformation followed by ``AFFINE(-1, 1)`` if minimised."""
    targets = tuple(objective.targets)
    T = len(targets)
    if not 2 <= T <= MAX_TARGETS:
        raise IncompatibilityError(
            f"The HIP path scores desirability objectives of 2 to {MAX_TARGETS} targets per posterior sample ({T} given). Use "
            f"BotorchRecommender, or 'DesirabilityObjective(as_pre_transformation=True)', which models the scalarised value."
        )
    scal = getattr(objective, "scalarizer", "GEOM_MEAN")
    scal = str(getattr(scal, "name", scal)).upper()
    if scal not in SCALARIZERS:
        raise IncompatibilityError(f"The scalarizer '{scal}' is not on the HIP path (MEAN, GEOM_MEAN). Use BotorchRecommender.")
    weights = getattr(objective, "normalized_weights", None)
    if weights is None:
        raw = np.asarray(getattr(objective, "weights", None) or np.ones(T), dtype=np.float64)
        weights = raw / raw.sum()
    weights = tuple(float(w) for w in weights)
    if len(weights) != T or not all(np.isfinite(w) and w > 0.0 for w in weights):
        raise IncompatibilityError(f"A desirability objective needs one positive finite weight per target, got {weights!r}.")
    oriented = getattr(objective, "_oriented_targets", None)
    programs, terms = [], []
    for i, target in enumerate(targets):
        name = str(getattr(target, "name", i))
        minimize = bool(getattr(target, "minimize", False))
        if oriented is not None:
            ops = _target_ops(getattr(oriented[i], "transformation", None), False, name)
        else:
            ops = _target_ops(getattr(target, "transformation", None), minimize, name)
        programs.append(ObjectiveProgram(ops))
        own = _target_ops(getattr(target, "transformation", None), False, name)
        if len(own) == 1 and own[0][0] == "AFFINE":
            a, b = own[0][1]
            terms.append((-a, -b) if minimize else (a, b))
        else:
            terms.append(None)
    return DesirabilityProgram(tuple(programs), weights, scal, None if any(t is None for t in terms) else tuple(terms))


class HipDesirability:
    """MC acquisition values of a desirability objective over T independent HIP GPs: ``best_f`` / ``score`` / ``greedy``.  Every call
    that reaches the device goes through the engines (``posterior``, ``set_pending``, ``cross_cov``, ``argmax``, and the first
    engine's ``desirability_acq``)."""

    def __init__(self, engines, program: DesirabilityProgram, X_all, kind: str = "qLogEI", n_mc_samples: int = 512, beta: float = 0.2,
                 device: int = 0, analytic: bool = False, maximize: bool = True):
        self.engines = list(engines)
        if len(self.engines) != program.n_targets:
            raise ValueError(f"{program.n_targets} targets need as many models, got {len(self.engines)}")
        self.outputs = [SimpleNamespace(engine=e, ext=e) for e in self.engines]
        self.program, self.kind, self.S, self.beta, self.device = program, kind, int(n_mc_samples), float(beta), int(device)
        self.analytic, self.maximize = bool(analytic), maximize  # (an analytic ``kind`` reads the combined Gaussian moments)
        self.X_all = np.ascontiguousarray(np.atleast_2d(X_all), dtype=np.float64)
        self._best_f = None

    @property
    def T(self) -> int:
        return self.program.n_targets

    def best_f(self) -> float:
        """max_i desirability(posterior means at measurement row i) over ALL measurement rows (``_builder.py:141-161, 256-265``:
        the objective of the posterior mean at the training inputs).  Every model is evaluated at all rows: with partial
        measurements each was trained on its own subset."""
        if self._best_f is None:
            mu = np.stack([e.posterior(self.X_all)[0].cpu().numpy() for e in self.engines], axis=-1)  # [n, T]
            self._best_f = float(self.program.apply(mu).max())
        return self._best_f

    def base_samples(self, q: int, seed: int) -> np.ndarray:
        """[S, q, T]: one Sobol draw over the q T normal variables (the ``[S, q', T]`` convention of ``nehvi.py``)."""
        return sobol_normal_base_samples(self.S, q * self.T, seed).reshape(self.S, q, self.T)

    def _moments(self, X):
        import torch

        X = self.engines[0]._as_dev(X)
        pairs = []
        for e in self.engines:
            e.set_pending(None)
            pairs.append(e.posterior(X))
        return X, torch.stack([m for m, _ in pairs]).contiguous(), torch.stack([v for _, v in pairs]).contiguous()

    def _pending_terms(self, X, pend):
        """(cross [T, N, p], (mean_p [T, p], cov_pp [T, p, p])) of the pending rows under every model."""
        import torch

        cross, mps, cpps = [], [], []
        for e in self.engines:
            mp, cpp = e.set_pending(pend)
            cross.append(e.cross_cov(X))
            mps.append(np.asarray(mp, dtype=np.float64)), cpps.append(np.asarray(cpp, dtype=np.float64))
        return torch.stack(cross).contiguous(), (np.stack(mps), np.stack(cpps))

    def _clear_pending(self):
        for e in self.engines:
            e.set_pending(None)

    def _score(self, X, mean, var, pend, z, alive, form=-1):
        if pend is None or len(pend) == 0:
            return self.engines[0].desirability_acq(self.program, self.kind, mean, var, z[:, 0, :], self.best_f(), self.beta, alive)
        cross, stats = self._pending_terms(X, pend)
        return self.engines[0].desirability_acq(self.program, self.kind, mean, var, z, self.best_f(), self.beta, alive, cross=cross,
                                                stats=stats, form=form)

    def score(self, X, X_pending=None, z=None, seed=None, alive=None):
        """Acquisition values [N] of the t-batches [x_i ; X_pending]; ``z`` [S, 1 + p, T] or drawn from ``seed``."""
        from baybe_amd import _lib

        pend = None if X_pending is None or len(X_pending) == 0 else np.ascontiguousarray(np.atleast_2d(X_pending), dtype=np.float64)
        p = 0 if pend is None else len(pend)
        if p > _lib.MAX_PENDING:
            raise IncompatibilityError(
                f"{p} pending / batch rows exceed the largest joint q-batch of the HIP kernels for a desirability objective "
                f"({_lib.MAX_PENDING + 1} points).")
        if z is None:
            z = self.base_samples(1 + p, draw_sampler_seed() if seed is None else seed)
        X, mean, var = self._moments(X)
        try:
            return self._score(X, mean, var, pend, np.ascontiguousarray(z, dtype=np.float64), alive)
        finally:
            if p:
                self._clear_pending()

    def greedy(self, X, q: int, seed=None, X_pending=None, alive=None) -> GreedyResult:
        """Sequential greedy of ``optimize_acqf_discrete``: the T posterior passes once, then per step the picks' cross-covariances
        and pending statistics per target and one scoring call; first index on ties, picks leave the candidate set."""
        import torch

        seed = draw_sampler_seed() if seed is None else seed
        X, mean, var = self._moments(X)
        N, d = X.shape[0], self.engines[0].spec.d
        base = np.zeros((0, d)) if X_pending is None or len(X_pending) == 0 else np.atleast_2d(np.asarray(X_pending, dtype=np.float64))[:, :d]
        alive = torch.ones(N, dtype=torch.uint8, device=X.device) if alive is None else alive.clone()
        rows, indices, values = [], [], []
        try:
            for _ in range(q):
                pend = np.vstack([base] + rows) if rows else base
                scores = self._score(X, mean, var, pend, self.base_samples(1 + len(pend), seed), alive)
                val, idx = self.engines[0].argmax(scores)
                indices.append(int(idx)), values.append(float(val))
                alive[idx] = 0
                rows.append(X[idx, :d].cpu().numpy().reshape(1, d))
        finally:
            self._clear_pending()
        return GreedyResult(indices, values)

    # ---- the recommender's surface (``baybe_amd.scoring``): ONE sampler seed per call, none for the analytic kinds ---------------
    supports_continuous = False
    check_request = staticmethod(check_joint_batch)

    def _analytic_scores(self, X, alive=None):
        """The analytic ``kind`` on the Gaussian desirability N(sum_t c_t mu_t + offset, sum_t c_t^2 sigma_t^2) of an arithmetic mean
        of affine targets (``DesirabilityProgram.as_affine``; to_botorch_posterior_transform, objectives/desirability.py:266-320)."""
        c, offset = self.program.as_affine()
        mean = var = None
        for ct, e in zip(c, self.engines):
            m, v = e.posterior(X)
            mean = ct * m + offset if mean is None else mean + ct * m
            var = (ct * ct) * v if var is None else var + (ct * ct) * v
        return self.engines[0].analytic_acq(self.kind, mean, var, self.best_f(), 1.0, self.beta, self.maximize, alive)

    def select(self, X, q, *, seeds, X_pending=None, alive=None, shard=None) -> GreedyResult:
        refuse_shard(shard, SHARD_TEXT)
        if self.analytic:  # q = 1 by construction
            val, idx = self.engines[0].argmax(self._analytic_scores(X, alive))
            return GreedyResult([int(idx)], [float(val)])
        return self.greedy(X, q, seed=seeds(), X_pending=X_pending, alive=alive)

    def values(self, X, *, seeds, X_pending=None):
        return self._analytic_scores(X) if self.analytic else self.score(X, X_pending=X_pending, seed=seeds())

    def joint_value(self, batch, *, seeds, X_pending=None) -> float:
        """The value of one q-batch (candidate = first row, the others enter as pending rows)."""
        if self.analytic:
            if len(batch) != 1 or X_pending is not None:
                raise IncompatibleAcquisitionFunctionError("Analytic acquisition functions score single points only.")
            return float(self._analytic_scores(batch).cpu().numpy()[0])
        base = X_pending if X_pending is not None else np.zeros((0, batch.shape[1]))
        return float(self.score(batch[:1], X_pending=np.vstack([batch[1:], base]), seed=seeds()).cpu().numpy()[0])
