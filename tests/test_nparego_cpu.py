"""qLogNParEGO and plain qNEHVI without a device: the declarative classes and ``convert_acqf``, the scalarisation and its weights,
the restatement on the frozen oracle (``tests/_nparego_reference.py``) against the qNEI restatement, and the plug-in classes driving
the scorers' surface over CPU doubles (``tests/_oracle_nparego.py``)."""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _nei_reference as nei_ref
import _nparego_reference as ref
from _problems import make_grid
from oracle import gp_oracle as go


def _targets(X, rng, noise=0.05):  # tests/test_nehvi_gpu.py::_targets
    f1 = -((X - 0.25) ** 2).sum(1) + noise * rng.standard_normal(len(X))
    f2 = -((X - 0.75) ** 2).sum(1) + noise * rng.standard_normal(len(X))
    f3 = -np.abs(X - 0.5).sum(1) + noise * rng.standard_normal(len(X))
    return np.stack([f1, f2, f3], 1)


def _case(m, n=24, N=150, d=3, seed=0):
    """The ``make_grid`` problems of tests/test_nehvi_gpu.py::_setup with the oracle's own fit."""
    rng = np.random.default_rng(seed)
    X = make_grid(N, d, seed)
    Xt = make_grid(4 * n, d, seed + 1)[:n]
    Y = _targets(Xt, rng)[:, :m]
    spec = go.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    return X, Xt, [go.fit_gp(spec, Xt, Y[:, o]) for o in range(m)]


# ---- declarative classes ----------------------------------------------------------------------------------------------------------
def test_convert_acqf_accepts_both_functions():
    from baybe_amd import acquisition as A
    from baybe_amd.exceptions import IncompatibleAcquisitionFunctionError

    par = A.convert_acqf("qLogNParEGO")
    assert type(par) is A.qLogNParEGO and par == A.qLogNParEGO() == A.convert_acqf(A.qLogNParEGO.__name__)
    assert (par.prune_baseline, par.n_mc_samples, par.scalarization_weights) == (True, 512, None)
    assert A.qLogNParEGO.supports_multi_output and A.qLogNParEGO.supports_batching and A.qLogNParEGO.supports_pending_experiments
    assert (A.qLogNParEGO.abbreviation, A.qLogNParEGO.kind) == ("qLogNParEGO", "qLogNParEGO") and not A.qLogNParEGO.is_analytic
    own = A.qLogNParEGO(prune_baseline=False, n_mc_samples=64, scalarization_weights=[0.25, 0.75])
    assert A.convert_acqf(own) is own and own.scalarization_weights == (0.25, 0.75)
    got = A.convert_acqf(type("qLogNParEGO", (), {"prune_baseline": False})())  # BayBE's own object: by class name, prune_baseline copied
    assert type(got) is A.qLogNParEGO and got.prune_baseline is False and got.scalarization_weights is None
    for bad in ([0.5, 0.6], [-0.5, 1.5]):
        with pytest.raises(ValueError):
            A.qLogNParEGO(scalarization_weights=bad)

    cls = A.qNoisyExpectedHypervolumeImprovement
    assert A.qNEHVI is cls and (cls.abbreviation, cls.kind) == ("qNEHVI", "qNEHVI") and cls.supports_multi_output
    want = cls()
    assert (want.reference_point, want.prune_baseline, want.n_mc_samples) == (None, True, 128)
    assert A.convert_acqf("qNEHVI") == want and A.convert_acqf("qNoisyExpectedHypervolumeImprovement") == want
    stand_in = type("qNoisyExpectedHypervolumeImprovement", (), {"prune_baseline": False, "reference_point": (0.5, -1.0)})()
    got = A.convert_acqf(stand_in)
    assert type(got) is cls and got.prune_baseline is False and got.reference_point == (0.5, -1.0)
    # qLogNEHVI's own conversion is what it was
    log = A.convert_acqf(type("qLogNoisyExpectedHypervolumeImprovement", (), {"prune_baseline": False, "reference_point": 0.2})())
    assert type(log) is A.qLogNoisyExpectedHypervolumeImprovement and log.reference_point == 0.2 and log.prune_baseline is False
    # what stays refused
    for name in ("qLogEHVI", "qEHVI", "qKG", "qNIPV", "qTS"):
        with pytest.raises(IncompatibleAcquisitionFunctionError):
            A.convert_acqf(name)


def test_convert_acqf_accepts_the_references_own_objects():
    from _reference import reference_baybe

    reference_baybe()
    from baybe.acquisition import qLogNParEGO, qNoisyExpectedHypervolumeImprovement

    from baybe_amd import acquisition as A

    got = A.convert_acqf(qLogNParEGO(prune_baseline=False))
    assert type(got) is A.qLogNParEGO and got.prune_baseline is False
    got = A.convert_acqf(qNoisyExpectedHypervolumeImprovement(reference_point=[0.5, -1.0], prune_baseline=False))
    assert type(got) is A.qNoisyExpectedHypervolumeImprovement and got.reference_point == (0.5, -1.0) and got.prune_baseline is False


# ---- scalarisation and weights -------------------------------------------------------------------------------------------------------
def test_scalarisation_against_a_hand_written_evaluation():
    from baybe_amd import nparego as P

    Y = np.array([[1.0, 10.0, 3.0], [3.0, 14.0, 3.0], [2.0, 12.0, 3.0]])  # the third target has a zero range
    hi, rng = P.scalarization_bounds(Y)
    assert np.array_equal(hi, [3.0, 14.0, 3.0]) and np.array_equal(rng, [2.0, 4.0, 1.0])
    w = np.array([0.5, 0.3, 0.2])
    y = np.array([2.5, 11.0, 2.0])
    t = [0.5 * (3.0 - 2.5) / 2.0, 0.3 * (14.0 - 11.0) / 4.0, 0.2 * (3.0 - 2.0) / 1.0]  # 0.125, 0.225, 0.2
    want = -(0.225 + 0.05 * (0.125 + 0.225 + 0.2))
    lo = hi - np.array([2.0, 4.0, 0.0])  # (the restatement takes lo and counts the zero range as 1 itself)
    assert ref.scalarize(y, w, lo, hi) == pytest.approx(want, rel=0, abs=1e-15) and max(t) == t[1]
    assert np.array_equal(ref.scalarize(np.stack([y, Y[1]]), w, lo, hi), [ref.scalarize(y, w, lo, hi), 0.0])  # Y[1] is the ideal point
    hi1, rng1 = P.scalarization_bounds(Y[:1])  # one row: hi = lo + 1
    assert np.array_equal(hi1, Y[0] + 1.0) and np.array_equal(rng1, [1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        P.check_weights([0.5, 0.6], 2)
    with pytest.raises(ValueError):
        P.check_weights([0.5, 0.5], 3)


def test_drawn_weights_lie_on_the_simplex_and_follow_the_global_generator():
    from baybe_amd.nparego import draw_scalarization_weights

    for m in (1, 2, 3, 4):
        torch.manual_seed(100 + m)
        w = draw_scalarization_weights(m)
        after = torch.rand(1, dtype=torch.float64)
        assert w.shape == (m,) and (w >= 0).all() and abs(w.sum() - 1.0) < 1e-15
        torch.manual_seed(100 + m)
        u = torch.rand(m - 1, dtype=torch.float64).numpy()  # exactly m - 1 double-precision values were consumed
        assert torch.equal(after, torch.rand(1, dtype=torch.float64))
        assert np.allclose(np.cumsum(w)[:-1], np.sort(u), rtol=0, atol=1e-15)
        torch.manual_seed(100 + m)
        assert np.array_equal(ref.sample_simplex(m), w)
    seen = []
    w = draw_scalarization_weights(3, agree=lambda v: seen.append(v) or np.array([0.2, 0.3, 0.5]))
    assert np.array_equal(w, [0.2, 0.3, 0.5]) and len(seen) == 1 and abs(seen[0].sum() - 1.0) < 1e-15


# ---- the restatement against qNEI's ----------------------------------------------------------------------------------------------------
def test_unit_weight_reduces_to_noisy_expected_improvement_of_that_target():
    """w = (1, 0): t_1 = 0, so g is a monotone piecewise-linear function of the first target alone,
        g = (1 + alpha) (y_0 - hi_0) / r_0  for y_0 <= hi_0   (max_o t_o = t_0),
        g =      alpha  (y_0 - hi_0) / r_0  for y_0 >  hi_0   (max_o t_o = t_1 = 0),      r_0 = hi_0 - lo_0,
    hence best_s = g(best0_s) with the qNEI restatement's best0_s = max_b F_b,s,0 and u_s = g(f_s,0) - g(best0_s), sample by sample.
    Where neither value exceeds hi_0 this is (1 + alpha) / r_0 times qNEI's improvement f_s,0 - best0_s - the factor between the two
    acquisition functions' non-log means; sampled values above hi_0 (the largest posterior MEAN) take the flatter branch, so the
    factor is checked on the samples below hi_0 and the piecewise form on all of them, and the non-log means agree through it."""
    X, Xt, models = _case(2)
    signs = [1.0, 1.0]
    S = 32
    z = ref.base_samples(S, len(Xt), 2, 11)
    lo, hi = ref.bounds(models, signs, Xt)
    w = np.array([1.0, 0.0])
    _, best, u = ref.scores(models, signs, Xt, z, X[:20], w, lo, hi)
    nei_mean, best0, f0 = nei_ref.scores(models[0], 1.0, Xt, np.ascontiguousarray(z[:, :, :1]), X[:20], log=False)
    r0 = hi[0] - lo[0]

    def g(y):
        return np.where(y <= hi[0], (1 + ref.ALPHA) * (y - hi[0]) / r0, ref.ALPHA * (y - hi[0]) / r0)

    assert np.allclose(best, g(best0), rtol=0, atol=1e-13)
    assert np.allclose(u, g(f0) - g(best0)[None, :], rtol=0, atol=1e-13)
    assert np.allclose(np.maximum(u, 0).mean(1), np.maximum(g(f0) - g(best0)[None, :], 0).mean(1), rtol=0, atol=1e-13)
    below = (f0 <= hi[0]) & (best0 <= hi[0])[None, :]
    assert below.sum() > 100 and (~below).sum() > 100  # both branches occur
    factor = (1 + ref.ALPHA) / r0
    assert np.allclose(np.maximum(u, 0)[below], factor * np.maximum(f0 - best0[None, :], 0)[below], rtol=0, atol=1e-13)
    every = below.all(axis=0)  # samples in which no candidate and no baseline value exceeds hi_0
    if every.any():
        assert np.allclose(np.maximum(u, 0)[:, every].mean(1), factor * np.maximum(f0 - best0[None, :], 0)[:, every].mean(1), rtol=0, atol=1e-13)
    # qNEI's own (non-log) score is the mean of its improvements: the per-sample identities above are statements about that score
    assert np.array_equal(nei_mean, np.maximum(f0 - best0[None, :], 0).mean(1))
    for i in np.flatnonzero(below.all(axis=1)):  # candidates none of whose samples leaves the steeper branch: the issue's identity
        assert np.maximum(u[i], 0).mean() == pytest.approx(factor * nei_mean[i], rel=0, abs=1e-13)
    slack = factor * nei_mean - np.maximum(u, 0).mean(1)  # elsewhere the flatter branch can only lower the improvement
    assert (slack >= -1e-13).all()


def test_an_rff_surrogate_is_refused_under_the_function_asked_for():
    from baybe_amd.exceptions import IncompatibilityError
    from baybe_amd.nehvi import HipNEHVI, HipNEHVIPlain
    from baybe_amd.nparego import HipNParEGO

    rff = [SimpleNamespace(spec=SimpleNamespace(kernel="rff"))] * 2
    for cls, args, name in ((HipNEHVI, ([0.0, 0.0],), "qLogNEHVI"), (HipNEHVIPlain, ([0.0, 0.0],), "qNEHVI"), (HipNParEGO, ([0.5, 0.5],), "qLogNParEGO")):
        with pytest.raises(IncompatibilityError) as err:
            cls(rff, [1.0, 1.0], np.zeros((1, 3)), *args)
        assert str(err.value).startswith(name + " ")


# ---- the plug-in classes over the CPU doubles --------------------------------------------------------------------------------------------
def _pareto_problem():
    from _baybe_shim import NumericalDiscreteParameter, NumericalTarget, ParetoObjective, SearchSpace

    rng = np.random.default_rng(5)
    vals = np.arange(6) / 5.0
    space = SearchSpace.from_product([NumericalDiscreteParameter(f"x{i}", vals) for i in range(3)])
    exp = space.discrete.exp_rep
    meas = exp.iloc[rng.choice(len(exp), 12, replace=False)].copy()
    T = _targets(meas[["x0", "x1", "x2"]].to_numpy(float), rng)
    meas["t1"], meas["t2"] = T[:, 0], -T[:, 1]
    obj = ParetoObjective([NumericalTarget("t1"), NumericalTarget("t2", minimize=True)])
    return space, exp, meas, obj


def _install(monkeypatch):
    import _oracle_engine
    import _oracle_nparego

    _oracle_engine.install(monkeypatch)
    _oracle_nparego.install(monkeypatch)


def test_recommend_through_the_plugin_classes(monkeypatch):
    """``recommend(3, ...)`` with ``"qLogNParEGO"`` on a two-target ``ParetoObjective`` and one pending experiment over the CPU doubles:
    the weights are drawn first, then the scoring seed, then the pruning seed; the batch is the restatement's greedy batch; a batch of
    20 is not refused; a stub shard sees the weights pass through ``agree``."""
    from baybe_amd import acquisition as A
    from baybe_amd.engine import draw_sampler_seed

    _install(monkeypatch)
    from baybe_amd.recommenders import HipBotorchRecommender

    space, exp, meas, obj = _pareto_problem()
    pending = exp.iloc[[7]]
    rec = HipBotorchRecommender(acquisition_function="qLogNParEGO")
    torch.manual_seed(17)
    got = rec.recommend(3, space, obj, meas, pending_experiments=pending)
    assert type(rec._scorer).__name__ == "OracleNParEGO" and rec._best_f is None
    torch.manual_seed(17)
    w = ref.sample_simplex(2)
    seed, pseed = draw_sampler_seed(), draw_sampler_seed()
    assert np.array_equal(rec._scorer.weights, w) and (w >= 0).all() and abs(w.sum() - 1) < 1e-15
    models = [m.engine._model for m in rec._surrogate_model.models]
    signs = np.array([1.0, -1.0])
    Xb = space.transform(meas, allow_extra=True).to_numpy(dtype=np.float64)
    lo, hi = ref.bounds(models, signs, Xb)
    keep, _ = ref.prune(models, signs, Xb, pseed, w, lo, hi)
    comp = space.discrete.comp_rep.to_numpy(dtype=np.float64)
    picks, _ = ref.greedy(models, signs, Xb[keep], comp, 3, 512, seed, w, lo, hi, X_pending=space.transform(pending).to_numpy(dtype=np.float64))
    assert list(got.index) == list(exp.index[picks])
    assert np.array_equal(rec._scorer._pruned, Xb[keep])
    # the read-backs go through the same prepare / score surface
    acq = rec.acquisition_values(exp.iloc[:5], space, obj, meas)
    assert np.isfinite(acq.to_numpy()).all()

    given = HipBotorchRecommender(acquisition_function=A.qLogNParEGO(prune_baseline=False, n_mc_samples=32))
    many = given.recommend(20, space, obj, meas)  # no joint q' kernel, so no 16 / 64-point cap
    assert len(set(many.index)) == 20 and given._acqf_in_use.kind == "qLogNParEGO" and len(given._scorer._pruned) == len(meas)

    calls = []

    def agree(value):
        calls.append(value)
        return np.array([0.25, 0.75]) if isinstance(value, np.ndarray) else value

    n = len(exp)
    sharded = HipBotorchRecommender(acquisition_function="qLogNParEGO",
                                    shard=SimpleNamespace(world=1, rank=0, N_total=n, start=0, stop=n, agree=agree))
    torch.manual_seed(17)
    sharded.recommend(1, space, obj, meas)
    assert np.array_equal(sharded._scorer.weights, [0.25, 0.75])
    assert isinstance(calls[0], np.ndarray) and np.array_equal(calls[0], w)  # rank 0's draw goes in first, before the two seeds
    assert calls[1:] == [seed, pseed]

    del calls[:]
    explicit = HipBotorchRecommender(acquisition_function=A.qLogNParEGO(scalarization_weights=[0.3, 0.7], n_mc_samples=32),
                                     shard=SimpleNamespace(world=1, rank=0, N_total=n, start=0, stop=n, agree=agree))
    torch.manual_seed(17)
    explicit.recommend(1, space, obj, meas)
    torch.manual_seed(17)
    assert calls == [draw_sampler_seed(), draw_sampler_seed()]  # given weights consume nothing from the generator
    assert np.array_equal(explicit._scorer.weights, [0.3, 0.7]) and explicit._scorer.S == 32


def test_plain_qnehvi_through_the_plugin_classes(monkeypatch):
    """``"qNEHVI"`` builds ``HipNEHVIPlain`` with the reference point qLogNEHVI would get; its batch is the restatement's."""
    from baybe_amd import acquisition as A
    from baybe_amd.engine import draw_sampler_seed
    from oracle import nehvi_oracle as no

    _install(monkeypatch)
    from baybe_amd.recommenders import HipBotorchRecommender

    space, exp, meas, obj = _pareto_problem()
    rec = HipBotorchRecommender(acquisition_function=A.qNEHVI(n_mc_samples=16))
    torch.manual_seed(23)
    got = rec.recommend(2, space, obj, meas)
    assert type(rec._scorer).__name__ == "OracleNEHVIPlain"
    torch.manual_seed(23)
    seed, pseed = draw_sampler_seed(), draw_sampler_seed()
    models = [m.engine._model for m in rec._surrogate_model.models]
    signs = np.array([1.0, -1.0])
    Xb = space.transform(meas, allow_extra=True).to_numpy(dtype=np.float64)
    ref_point = no.compute_ref_point(meas[["t1", "t2"]].to_numpy() * signs[None, :])
    assert np.allclose(rec._scorer.ref, ref_point, rtol=1e-15, atol=0)
    keep = no.prune_baseline(models, signs, Xb, ref_point, pseed)
    comp = space.discrete.comp_rep.to_numpy(dtype=np.float64)
    picks, vals = ref.qnehvi_greedy(models, signs, Xb[keep], ref_point, comp, 2, 16, seed)
    assert list(got.index) == list(exp.index[picks]) and vals[0] > 0
    log = HipBotorchRecommender()  # the default for a Pareto objective is still qLogNEHVI with today's arguments
    log.recommend(1, space, obj, meas)
    assert type(log._scorer).__name__ == "OracleNEHVI" and log._scorer.S == 128


def test_single_target_objective_is_refused(monkeypatch):
    from _baybe_shim import NumericalTarget, SingleTargetObjective
    from baybe_amd.exceptions import IncompatibleAcquisitionFunctionError

    _install(monkeypatch)
    from baybe_amd.recommenders import HipBotorchRecommender

    space, exp, meas, _ = _pareto_problem()
    for name in ("qLogNParEGO", "qNEHVI"):
        with pytest.raises(IncompatibleAcquisitionFunctionError, match="needs a multi-output objective"):
            HipBotorchRecommender(acquisition_function=name).recommend(1, space, SingleTargetObjective(NumericalTarget("t1")), meas)
