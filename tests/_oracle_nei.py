"""TEST INFRASTRUCTURE - CPU double of ``baybe_amd.nei.HipNEI`` on the restatement ``tests/_nei_reference.py`` (same constructor /
``prepare`` / ``score`` / ``greedy`` surface; pending points and picks join the baseline), for the plug-in classes under
``_oracle_engine.install`` where there is no device."""

from types import SimpleNamespace

import numpy as np
import torch

import _nei_reference as ref
from baybe_amd import engine as engine_mod
from baybe_amd.engine import GreedyResult
from baybe_amd.nehvi import HipNEHVI


class OracleNEI:
    def __init__(self, engine, sign, X_baseline, n_mc_samples=512, prune_baseline=True, log=True, device=0):
        self.engine, self.sign, self.log = engine, float(sign), bool(log)
        self.outputs = [SimpleNamespace(engine=engine, ext=engine, sign=float(sign))]
        self.X_baseline = np.ascontiguousarray(np.atleast_2d(X_baseline), dtype=np.float64)
        self.S, self.prune = int(n_mc_samples), bool(prune_baseline)
        self._pruned = self.X_b_current = self._z = None

    def prepare(self, seed, extra_baseline=None, prune_seed=None):
        if self._pruned is None:
            Xb0 = self.X_baseline
            if self.prune and len(Xb0):
                Xb0 = Xb0[ref.prune(self.engine._model, self.sign, Xb0, engine_mod.draw_sampler_seed() if prune_seed is None else prune_seed)[0]]
            self._pruned = Xb0
        Xb = self._pruned
        if extra_baseline is not None and len(extra_baseline):
            Xb = np.vstack([Xb, np.atleast_2d(extra_baseline)])
        self.X_b_current, self._z = Xb, ref.base_samples(self.S, len(Xb), seed)

    def score(self, X_dev, alive=None, sync=True):
        X = self.engine._np(X_dev)
        live = np.ones(len(X), bool) if alive is None else alive.numpy().astype(bool)
        out = np.full(len(X), -np.inf)
        out[live] = ref.scores(self.engine._model, self.sign, self.X_b_current, self._z, X[live], self.log)[0]
        return torch.from_numpy(out)

    def greedy(self, X_dev, q, seed=None, prune_seed=None, X_pending=None, alive=None, shard=None):
        X_dev = self.engine._as_dev(X_dev)
        d = self.engine.spec.d
        seed = engine_mod.draw_sampler_seed() if seed is None else seed
        alive = torch.ones(X_dev.shape[0], dtype=torch.uint8) if alive is None else alive.clone()
        picks = [np.atleast_2d(np.asarray(X_pending, dtype=np.float64))] if X_pending is not None and len(X_pending) else []
        indices, values = [], []
        for _ in range(q):
            self.prepare(seed, np.vstack(picks) if picks else None, prune_seed)
            s = self.score(X_dev, alive).numpy()
            idx = int(np.argmax(s))
            indices.append(idx), values.append(float(s[idx]))
            alive[idx] = 0
            picks.append(X_dev[idx, :d].numpy().reshape(1, d))
        return GreedyResult(indices, values)

    # the recommender's surface is the PRODUCT's (baybe_amd.scoring): the seeds a path draws, and their order, are under test
    supports_continuous, check_request = HipNEHVI.supports_continuous, staticmethod(HipNEHVI.check_request)
    select, values, joint_value, _prepare_drawing = HipNEHVI.select, HipNEHVI.values, HipNEHVI.joint_value, HipNEHVI._prepare_drawing


def install(monkeypatch):
    """On top of ``_oracle_engine.install``: ``nei.HipNEI`` -> ``OracleNEI``."""
    import baybe_amd.nei as nei_mod

    monkeypatch.setattr(nei_mod, "HipNEI", OracleNEI)
