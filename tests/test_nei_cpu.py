"""qNEI / qLogNEI without a device: the declarative classes and ``convert_acqf``, the formulation the device kernels implement
(conditional mean under the extended noise-free model + conditional sd * z_x) against the restatement on the frozen oracle
(``tests/_nei_reference.py``), and the plug-in classes driving ``HipNEI``'s surface over a CPU double (``tests/_oracle_nei.py``)."""

import numpy as np
import pytest
import torch

import _nei_reference as ref
from _problems import make_grid
from oracle import gp_oracle as go


def _case(n, N, d, seed, sign):
    """The ``make_grid`` problems of tests/test_nei_gpu.py (case A: 24, 150, 3, 0, +1) with the oracle's own fit."""
    rng = np.random.default_rng(seed)
    X = make_grid(N, d, seed)
    Xt = make_grid(4 * n, d, seed + 1)[:n]
    y = sign * (-((Xt - 0.25) ** 2).sum(1) + 0.05 * rng.standard_normal(n))
    spec = go.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    return X, Xt, y, spec, go.fit_gp(spec, Xt, y)


def test_convert_acqf_and_class_attributes():
    from baybe_amd import acquisition as A

    for abbr, name, cls in (("qNEI", "qNoisyExpectedImprovement", A.qNoisyExpectedImprovement),
                            ("qLogNEI", "qLogNoisyExpectedImprovement", A.qLogNoisyExpectedImprovement)):
        assert getattr(A, abbr) is cls and cls.__name__ == name
        want = cls()
        assert want.prune_baseline is True and want.n_mc_samples == 512
        assert A.convert_acqf(abbr) == want and A.convert_acqf(name) == want
        own = cls(prune_baseline=False, n_mc_samples=64)
        assert A.convert_acqf(own) is own
        stand_in = type(name, (), {"prune_baseline": False})()  # BayBE's own object: mapped by class name, prune_baseline copied
        got = A.convert_acqf(stand_in)
        assert type(got) is cls and got.prune_baseline is False and got.n_mc_samples == 512
        assert (cls.abbreviation, cls.kind) == (abbr, abbr)
        assert cls.supports_batching and cls.supports_pending_experiments and cls.is_mc
        assert not cls.supports_multi_output and not cls.is_analytic
        with pytest.raises(TypeError):
            cls(prune_baseline=1)


def test_device_formulation_equals_the_joint_draw():
    """What ``bbh_nehvi_samples`` + the scoring kernels compute, in numpy on case A: with the model extended by the baseline rows
    as noise-free observations of the sampled values F_b,s, the joint draw of f(x) through the cached baseline factor is
    E[f(x) | D, F_b,s] + sd[f(x) | D, X_b] * z_x,s - to 1e-10 (the oracle's own joint covariance carries rounding of that size)."""
    from scipy import linalg as sla

    X, Xt, y, spec, model = _case(24, 150, 3, 0, +1.0)
    S = 32
    z = ref.base_samples(S, len(Xt), 11)
    _, best, f_joint = ref.scores(model, 1.0, Xt, z, X[:60])
    p = model.params
    Xe = np.vstack([model.Xn, go.normalize_inputs(spec, Xt)])
    Ke = go.cross_cov(spec, p, Xe, Xe)
    n = len(Xt)
    Ke[:n, :n] += p.noise * np.eye(n)
    # the extended factor draws the baseline sample itself: y_ext,s = c + L_ext [t; z_s]
    L = _extended_factor(Ke, n)
    t = sla.solve_triangular(L[:n, :n], model.ystd - p.mean, lower=True)
    dup = np.array([(np.abs(Xt - x).sum(1) < 1e-12).any() for x in X[:60]])
    worst = 0.0
    for i in np.nonzero(~dup)[0]:
        kx = go.cross_cov(spec, p, go.normalize_inputs(spec, X[i][None, :]), Xe)[0]
        v = sla.solve_triangular(L, kx, lower=True)
        sd = model.ysd * np.sqrt(max(1.0 - v @ v, 0.0))
        for s in range(S):
            w = sla.solve_triangular(L.T, np.r_[t, z[s, :n, 0]], lower=False)  # weight column L_ext^-T [t; z_s]
            mean_s = model.ybar + model.ysd * (p.mean + kx @ w)
            worst = max(worst, abs(mean_s + sd * z[s, n, 0] - f_joint[i, s]))
    assert worst < 1e-10, worst
    # ... and the baseline rows of the same generative form are the oracle's baseline draw, whose row maximum is best_s
    Fb = model.ybar + model.ysd * (p.mean + (L[n:, :] @ np.vstack([np.tile(t[:, None], (1, S)), z[:, :n, 0].T])).T)
    assert np.abs(Fb.max(1) - best).max() < 1e-10


def _extended_factor(Ke, n):
    """Cholesky factor of the extended covariance; the latent block takes the jitter psd_safe_cholesky would add (none is needed
    on case A: the training rows carry noise, the baseline rows do not coincide beyond the training set's own rows)."""
    from scipy import linalg as sla

    jit = 0.0
    for attempt in range(4):
        try:
            return sla.cholesky(Ke + jit * np.diag(np.r_[np.zeros(n), np.ones(len(Ke) - n)]), lower=True)
        except np.linalg.LinAlgError:
            jit = 1e-8 * 10**attempt
    raise AssertionError("extended covariance not positive definite")


def test_recommend_through_the_plugin_classes(monkeypatch):
    """``recommend(3, ...)`` with ``acquisition_function="qLogNEI"`` and one pending experiment over the CPU doubles: the batch is the
    restatement's greedy batch (scoring seed drawn first, then the pruning seed), and a batch of 20 is not refused."""
    import _oracle_engine
    import _oracle_nei
    from _baybe_shim import NumericalDiscreteParameter, NumericalTarget, SearchSpace, SingleTargetObjective
    from baybe_amd.engine import draw_sampler_seed

    _oracle_engine.install(monkeypatch)
    _oracle_nei.install(monkeypatch)
    from baybe_amd.recommenders import HipBotorchRecommender

    rng = np.random.default_rng(5)
    vals = np.arange(6) / 5.0
    space = SearchSpace.from_product([NumericalDiscreteParameter(f"x{i}", vals) for i in range(3)])
    exp = space.discrete.exp_rep
    meas = exp.iloc[rng.choice(len(exp), 12, replace=False)].copy()
    Xm = meas[["x0", "x1", "x2"]].to_numpy(float)
    meas["y"] = -((Xm - 0.25) ** 2).sum(1) + 0.05 * rng.standard_normal(len(Xm))
    obj = SingleTargetObjective(NumericalTarget("y"))
    pending = exp.iloc[[7]]
    rec = HipBotorchRecommender(acquisition_function="qLogNEI")
    torch.manual_seed(17)
    got = rec.recommend(3, space, obj, meas, pending_experiments=pending)
    assert type(rec._scorer).__name__ == "OracleNEI" and rec._best_f is None
    torch.manual_seed(17)
    seed, pseed = draw_sampler_seed(), draw_sampler_seed()
    model = rec._surrogate_model.engine._model
    Xb = space.transform(meas, allow_extra=True).to_numpy(dtype=np.float64)
    keep, _ = ref.prune(model, 1.0, Xb, pseed)
    comp = space.discrete.comp_rep.to_numpy(dtype=np.float64)
    picks, _ = ref.greedy(model, 1.0, Xb[keep], comp, 3, 512, seed, X_pending=space.transform(pending).to_numpy(dtype=np.float64))
    assert list(got.index) == list(exp.index[picks])
    assert np.array_equal(rec._scorer._pruned, Xb[keep])
    small = HipBotorchRecommender(acquisition_function=type("qNoisyExpectedImprovement", (), {"prune_baseline": False})())
    many = small.recommend(20, space, obj, meas)  # no joint q' kernel, so no 16 / 64-point cap
    assert len(set(many.index)) == 20 and small._acqf_in_use.kind == "qNEI" and small._acqf_in_use.prune_baseline is False
