"""qNegIntegratedPosteriorVariance (``baybe/acquisition/acqfs.py:29-138``) on the HIP path: active learning over discrete spaces.

[UPSTREAM] BoTorch is restated from memory, parity unpinned: for a t-batch ``[x ; B]`` (B = pending experiments + the batch's
earlier picks) ``qNegIntegratedPosteriorVariance`` conditions the GP on the batch through ``model.fantasize`` - the likelihood's
homoskedastic noise is added at the new points, the fantasised values do not enter a variance - evaluates the latent posterior
variance at the integration points ``p_1 .. p_M`` and returns ``-mean_j var_j``.  The target's direction does not enter, and no
sample does: with ``cov`` the posterior covariance given the training data and ``s2`` the noise,

    G = cov(B, B) + s2 I,   H = G^-1 cov(B, P),
    C_j(x)  = cov(x, p_j) - cov(x, B) H[:, j]                      (= cov(p_j, x | B))
    gain(x) = sum_j C_j(x)^2 / (max(var(x) - cov(x, B) G^-1 cov(B, x), 0) + s2)
    V_B     = mean_j (var(p_j) - cov(p_j, B) H[:, j])              (once per greedy step)
    qNIPV([x ; B]) = gain(x) / M - V_B.

``csrc/bbh_nipv.hip`` computes ``gain`` for all candidates in one pass.  The selection runs on ``gain``: adding the constant
``-V_B`` would only throw away low bits and manufacture ties; the value is formed on the host for what is reported.

Per greedy step the host needs ``G``, ``H`` and ``V_B``.  They come from what ``set_pending`` returns (``cov(B, B)``), what
``nipv_set_points`` returned (``var(p_j)``), and ONE small cross-covariance pass over the M integration points (``cov(P, B)``,
[M, b]) - not from ``posterior_joint`` over ``[B ; P]``, which would factor an (b + M)-point covariance on the host."""

from __future__ import annotations

import math

import numpy as np
import pandas as pd

from baybe_amd.engine import GreedyResult, draw_sampler_seed
from baybe_amd.exceptions import IncompatibilityError
from baybe_amd.scoring import refuse_shard

MAX_TRAINING_POINTS = 512  # csrc/bbh_nipv.hip
NIPV_KERNELS = ("matern12", "matern32", "matern52", "rbf")


def integration_ilocs(n_rows: int, n_points: int, method: str, values=None, device: int = 0) -> list:
    """``sample_numerical_df`` (utils/sampling_algorithms.py:185-227) as positional indices: the whole frame as often as it fits
    into ``n_points``, the sampling method for the remainder.  ``Random`` consumes ``np.random``'s global state exactly as
    ``DataFrame.sample`` does (the draw depends on the length alone, so pandas is called on an index-only frame); ``FPS`` is the
    device's ``farthest_point_sampling`` with the reference's defaults."""
    n_trivial, n_sampled = divmod(int(n_points), int(n_rows))
    ilocs = list(range(n_rows)) * n_trivial
    if n_sampled > 0:
        if method == "FPS":
            from baybe_amd.sampling import farthest_point_sampling

            ilocs += [int(i) for i in farthest_point_sampling(values, n_sampled, device=device)]
        elif method == "Random":
            ilocs += pd.DataFrame(index=pd.RangeIndex(n_rows)).sample(n_sampled).index.tolist()
        else:
            raise ValueError(f"Unrecognized sampling method: '{method}'.")
    return ilocs


def integration_points(acqf, searchspace, device: int = 0) -> pd.DataFrame:
    """``qNegIntegratedPosteriorVariance.get_integration_points`` for the discrete part: rows of ALL of
    ``searchspace.discrete.comp_rep`` (not of the candidates left); repeats stay repeated rows."""
    comp = searchspace.discrete.comp_rep
    n = acqf.sampling_n_points or math.ceil(acqf.sampling_fraction * len(comp))
    method = str(getattr(acqf.sampling_method, "value", acqf.sampling_method))
    values = comp.values if method == "FPS" else None
    return comp.iloc[integration_ilocs(len(comp), n, method, values, device)]


SHARD_TEXT = "Row shards are not on the HIP path of qNIPV; score the candidates on one device."


def check_batch(n_points: int) -> None:
    """pending + picks must fit the handle's pending state (the last step conditions on pending + batch_size - 1 points; the
    recommender's rule keeps one point of headroom, as for qEHVI)."""
    from baybe_amd import _lib

    if n_points > _lib.MAX_PENDING:
        raise IncompatibilityError(
            f"qNIPV conditions the model on the pending experiments and the batch's picks; {n_points} points exceed the HIP "
            f"kernel's limit of {_lib.MAX_PENDING}. Recommend in smaller batches, or use BotorchRecommender."
        )


class HipNIPV:
    """qNIPV values over one HIP GP: ``score`` / ``gain`` / ``greedy`` / ``joint_value``.  Every call that reaches the device goes
    through the engine (``nipv_set_points`` once, ``posterior`` once per call, then per step ``set_pending``, ``cross_cov``,
    ``nipv_gain``, ``argmax``)."""

    def __init__(self, engine, P, device: int = 0):
        self.engine = engine
        self.device = int(device)
        d = engine.spec.d
        self.P = np.ascontiguousarray(np.atleast_2d(np.asarray(P, dtype=np.float64))[:, :d])
        self.M = len(self.P)
        self._var_p = None
        self._P_dev = None

    def _prepare(self):
        if self._var_p is None:
            self._var_p = self.engine.nipv_set_points(self.P)
            self._P_dev = self.engine._as_dev(self.P)

    @property
    def s2(self) -> float:
        """The likelihood's noise in the target's original scale."""
        return float(self.engine.ysd) ** 2 * float(self.engine.params.noise)

    def _pend(self, X_pending):
        d = self.engine.spec.d
        if X_pending is None or len(X_pending) == 0:
            return np.zeros((0, d))
        return np.ascontiguousarray(np.atleast_2d(np.asarray(X_pending, dtype=np.float64))[:, :d])

    def conditioning_terms(self, pend):
        """(H [b, M], G^-1 [b, b], V_B) of the pending rows; leaves them as the handle's pending state.  b = 0: (None, None, V_0)."""
        self._prepare()
        if len(pend) == 0:
            self.engine.set_pending(None)
            return None, None, float(np.mean(self._var_p))
        _, cpp = self.engine.set_pending(pend)
        cov_pb = self.engine.cross_cov(self._P_dev).cpu().numpy()  # [M, b]
        G = np.asarray(cpp, dtype=np.float64) + self.s2 * np.eye(len(pend))
        ginv = np.linalg.inv(G)
        ginv = 0.5 * (ginv + ginv.T)
        H = ginv @ cov_pb.T  # [b, M]
        v_b = float(np.mean(self._var_p - np.einsum("jl,lj->j", cov_pb, H)))
        return np.ascontiguousarray(H), np.ascontiguousarray(ginv), v_b

    def _variance(self, X):
        X = self.engine._as_dev(X)
        self.engine.set_pending(None)
        return X, self.engine.posterior(X)[1]

    def _gain(self, X, var, pend, alive):
        H, ginv, v_b = self.conditioning_terms(pend)
        cross = self.engine.cross_cov(X) if len(pend) else None
        return self.engine.nipv_gain(X, var, cross, H, ginv, alive), v_b

    def gain(self, X, X_pending=None, alive=None):
        """(gain [N] device tensor, V_B) of the t-batches [x_i ; X_pending]."""
        pend = self._pend(X_pending)
        check_batch(len(pend))
        self._prepare()
        X, var = self._variance(X)
        try:
            return self._gain(X, var, pend, alive)
        finally:
            self.engine.set_pending(None)

    def score(self, X, X_pending=None, seed=None, alive=None):
        """Acquisition values [N] of the t-batches [x_i ; X_pending] (device tensor); ``seed`` is accepted and unused."""
        g, v_b = self.gain(X, X_pending, alive)
        return g / self.M - v_b

    # ---- the recommender's surface (``baybe_amd.scoring``): one seed per call, drawn and unused ---------------------------------
    supports_continuous = False

    @staticmethod
    def check_request(batch_size, n_pend, acqf=None, program=None, model=None) -> None:
        """The model is conditioned on the pending experiments and the picks through the handle's pending state."""
        check_batch(n_pend + batch_size)

    def select(self, X, q, *, seeds, X_pending=None, alive=None, shard=None) -> GreedyResult:
        refuse_shard(shard, SHARD_TEXT)
        return self.greedy(X, q, seed=seeds(), X_pending=X_pending, alive=alive)

    def values(self, X, *, seeds, X_pending=None):
        return self.score(X, X_pending=X_pending, seed=seeds())

    def joint_value(self, batch, *, seeds, X_pending=None) -> float:
        """The value of the whole batch ``[batch ; X_pending]``: its first point scored with the others pending (the value is
        symmetric in the points)."""
        seeds()
        batch = np.atleast_2d(np.asarray(batch, dtype=np.float64))
        rest = np.vstack([self._pend(batch[1:]), self._pend(X_pending)])
        return float(self.score(batch[:1], X_pending=rest).cpu().numpy()[0])

    def greedy(self, X, q: int, seed=None, X_pending=None, alive=None) -> GreedyResult:
        """Sequential greedy of ``optimize_acqf_discrete``: the posterior pass once, then per step the conditioning terms, the
        picks' cross-covariances and one gain pass; argmax on the gain, first index on ties; picks leave the candidate set.
        The reference constructs a sampler whose draw it never uses: one seed is drawn per recommendation ([UPSTREAM], unpinned),
        which keeps torch's global stream where the other MC functions leave it."""
        import torch

        if seed is None:
            draw_sampler_seed()
        base = self._pend(X_pending)
        check_batch(len(base) + q)
        self._prepare()
        X, var = self._variance(X)
        d = self.engine.spec.d
        N = X.shape[0]
        alive = torch.ones(N, dtype=torch.uint8, device=X.device) if alive is None else alive.clone()
        rows, indices, values = [], [], []
        try:
            for _ in range(q):
                pend = np.vstack([base] + rows) if rows else base
                g, v_b = self._gain(X, var, pend, alive)
                val, idx = self.engine.argmax(g)
                indices.append(int(idx)), values.append(float(val) / self.M - v_b)
                alive[idx] = 0
                rows.append(X[idx, :d].cpu().numpy().reshape(1, d))
        finally:
            self.engine.set_pending(None)
        return GreedyResult(indices, values)
