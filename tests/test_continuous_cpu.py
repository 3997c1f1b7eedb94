"""Gradient-based continuous refinement without a device: the batched box optimiser, the ``continuous_optimizer`` option and its
refusals (each raised before anything is fitted), and the closed-form derivative oracle against finite differences."""

from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

from _continuous_cases import make_case, oracle_model, random_rows
from _oracle_continuous import central_difference, posterior_grad_oracle, two_step_ok


# ---- maximize_box ----------------------------------------------------------------------------------------------------------
def _quadratic():
    rng = np.random.default_rng(0)
    d = 6
    A = rng.normal(size=(d, d))
    Q = A @ A.T + np.eye(d)
    c = np.array([1.5, -0.7, 0.3, 0.5, 0.2, 0.8])  # the unconstrained maximum: outside [0, 1]^6 in the first two coordinates
    return d, Q, c


def _projected_solution(Q, c, d):
    """The maximiser of -1/2 (x - c)^T Q (x - c) over [0, 1]^d by enumerating the active sets (KKT)."""
    import itertools

    best = (-np.inf, None)
    for pattern in itertools.product((None, 0.0, 1.0), repeat=d):
        fixed = np.array([v is not None for v in pattern])
        x = np.array([0.0 if v is None else v for v in pattern])
        free = ~fixed
        if free.any():  # stationarity on the free coordinates
            x[free] = c[free] - np.linalg.solve(Q[np.ix_(free, free)], Q[np.ix_(free, fixed)] @ (x[fixed] - c[fixed]))
        if (x < -1e-12).any() or (x > 1 + 1e-12).any():
            continue
        val = -0.5 * (x - c) @ Q @ (x - c)
        if val > best[0]:
            best = (val, x)
    return best


def test_maximize_box_reaches_the_projected_solution_from_every_start():
    from baybe_amd.continuous import maximize_box

    d, Q, c = _quadratic()
    calls = []

    def value_and_grad(X):
        calls.append(len(X))
        D = X - c
        return -0.5 * np.einsum("kd,de,ke->k", D, Q, D), -D @ Q, np.ones(len(X), dtype=np.uint8)

    starts = np.random.default_rng(1).random((5, d))
    starts[0] = 0.0  # a corner of the box
    res = maximize_box(value_and_grad, starts, np.zeros(d), np.ones(d))
    v_opt, x_opt = _projected_solution(Q, c, d)
    assert x_opt[0] == 1.0 and x_opt[1] == 0.0  # the two coordinates whose unconstrained optimum lies outside
    assert np.abs(res.values - v_opt).max() <= 1e-9, res.values - v_opt
    assert np.abs(res.x - x_opt).max() <= 1e-4
    assert res.converged.all() and res.ok.all()
    assert res.calls == len(calls) == res.iterations + res.backtracks
    assert all(k == 5 for k in calls)  # every start in every call: one callback call per trial


def test_maximize_box_freezes_a_start_the_callback_flags():
    from baybe_amd.continuous import maximize_box

    d, Q, c = _quadratic()

    def value_and_grad(X):
        D = X - c
        ok = np.ones(len(X), dtype=np.uint8)
        ok[2] = 0  # e.g. a candidate whose joint factor needed jitter
        return -0.5 * np.einsum("kd,de,ke->k", D, Q, D), -D @ Q, ok

    starts = np.random.default_rng(2).random((4, d))
    res = maximize_box(value_and_grad, starts, np.zeros(d), np.ones(d))
    assert np.array_equal(res.x[2], starts[2]) and res.values[2] == value_and_grad(starts)[0][2] and not res.ok[2]
    v_opt, _ = _projected_solution(Q, c, d)
    assert np.abs(np.delete(res.values, 2) - v_opt).max() <= 1e-9


def test_maximize_box_counts_backtracking_evaluations():
    from baybe_amd.continuous import maximize_box

    calls = []

    def value_and_grad(X):  # the first steepest-ascent trial (a tenth of the box) overshoots the maximum from this close
        calls.append(1)
        return -1e4 * (X**2).sum(axis=1), -2e4 * X, np.ones(len(X))

    res = maximize_box(value_and_grad, np.array([[0.01, -0.02]]), -np.ones(2), np.ones(2))
    assert res.backtracks > 0 and res.calls == len(calls) == res.iterations + res.backtracks
    assert abs(res.values[0]) <= 1e-9


# ---- the option and its refusals -----------------------------------------------------------------------------------------------
class _UntouchableSurrogate:
    """Stands in for the GP surrogate: its settings can be read, any use is an error."""

    kernel = "matern52"
    kernel_or_factory = None
    preset = "BAYBE"
    use_outputscale = False
    supports_multi_output = False

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def fit(self, *a, **k):
        raise AssertionError("the surrogate was fitted")

    @property
    def engine(self):
        raise AssertionError("the engine was used")


def _space(dc: int, task: bool = False):
    from _replay import HybridSpace

    disc = pd.DataFrame({"d0": [0.0, 0.5, 1.0]})
    bounds = pd.DataFrame(np.array([[0.0] * dc, [1.0] * dc]), index=["min", "max"], columns=[f"c{a}" for a in range(dc)])
    space = HybridSpace(disc, bounds)
    if task:
        space.task_idx, space.n_tasks = 0, 2
    rng = np.random.default_rng(0)
    return space, rng


def _measurements(space, rng, n: int = 8):
    dc = len(space.comp_rep_columns) - 1
    M = np.hstack([rng.choice([0.0, 0.5, 1.0], (n, 1)), rng.random((n, dc))])
    return pd.DataFrame(M, columns=list(space.comp_rep_columns)).assign(y=-((M - 0.4) ** 2).sum(1))


def _objective(transformation=None, multi=False):
    t = SimpleNamespace(name="y", minimize=False, transformation=transformation)
    if multi:
        return SimpleNamespace(targets=(t, SimpleNamespace(name="y2", minimize=False, transformation=None)), is_multi_output=True)
    return SimpleNamespace(targets=(t,), is_multi_output=False)


def test_continuous_optimizer_option_is_validated_and_defaults_to_compass():
    from baybe_amd import _lib
    from baybe_amd.recommenders import HipBotorchRecommender

    assert HipBotorchRecommender().continuous_optimizer == "compass"
    assert HipBotorchRecommender(continuous_optimizer="gradient").continuous_optimizer == "gradient"  # a TypeError without the feature
    with pytest.raises(ValueError, match="continuous_optimizer"):
        HipBotorchRecommender(continuous_optimizer="lbfgs")
    with pytest.raises(TypeError):
        HipBotorchRecommender(None, "gradient")  # keyword-only
    assert "bbh_posterior_grad" in _lib.SIGNATURES and "bbh_qlogei_partials" in _lib.SIGNATURES


def test_plugin_recommender_fields_carry_the_option():
    import attrs

    from baybe_amd.recommenders import recommender_fields

    f = recommender_fields(with_base_fields=False)
    cls = attrs.make_class("R", {"continuous_optimizer": f["continuous_optimizer"]})
    assert cls().continuous_optimizer == "compass" and cls(continuous_optimizer="gradient").continuous_optimizer == "gradient"


def test_default_recommender_still_refuses_five_continuous_parameters():
    from baybe_amd.exceptions import IncompatibilityError
    from baybe_amd.recommenders import HipBotorchRecommender

    space, rng = _space(5)
    with pytest.raises(IncompatibilityError, match="continuous parameters"):
        HipBotorchRecommender(surrogate_model=_UntouchableSurrogate()).recommend(1, space, _objective(), _measurements(space, rng))


def test_gradient_admits_up_to_32_continuous_parameters_and_then_reaches_the_fit():
    from baybe_amd.exceptions import IncompatibilityError
    from baybe_amd.recommenders import HipBotorchRecommender

    for dc in (5, 32):
        space, rng = _space(dc)
        rec = HipBotorchRecommender(surrogate_model=_UntouchableSurrogate(), continuous_optimizer="gradient")
        with pytest.raises(AssertionError, match="the surrogate was fitted"):  # nothing refused: the fit is the next thing
            rec.recommend(1, space, _objective(), _measurements(space, rng))
    space, rng = _space(33)
    with pytest.raises(IncompatibilityError, match="33 continuous parameters"):
        HipBotorchRecommender(surrogate_model=_UntouchableSurrogate(), continuous_optimizer="gradient").recommend(
            1, space, _objective(), _measurements(space, rng))


def _stub(name, **fields):
    return type(name, (), fields)()


def _refusal_cases():
    from baybe_amd.acquisition import qUpperConfidenceBound
    from baybe_amd.exceptions import IncompatibilityError, IncompatibleAcquisitionFunctionError
    from baybe_amd.kernels import MaternKernel, ProductKernel, RBFKernel

    I, A = IncompatibilityError, IncompatibleAcquisitionFunctionError
    return {
        "acquisition function": (A, "qLogExpectedImprovement only", dict(rec=dict(acquisition_function=qUpperConfidenceBound()))),
        "transformed target": (I, "transformed target", dict(objective=_objective(_stub("AffineTransformation", factor=2.0, shift=1.0)))),
        "multi-output objective": (I, "multi-output", dict(objective=_objective(multi=True))),
        "task parameter": (I, "task parameters", dict(task=True)),
        "composite kernel": (I, "composite kernel", dict(surrogate=dict(kernel=ProductKernel([MaternKernel(), RBFKernel()])))),
        "RFF kernel": (I, "no derivative on the device", dict(surrogate=dict(kernel="rff"))),
        "other kernel kind": (I, "no derivative on the device", dict(surrogate=dict(kernel="matern12"))),
        "more than 512 training points": (I, "512 training points", dict(n=513)),
        "row shards": (I, "row shards", dict(rec=dict(shard=SimpleNamespace(world=2, rank=0, agree=lambda v: v)))),
    }


@pytest.mark.parametrize("case", ["acquisition function", "transformed target", "multi-output objective", "task parameter",
                                  "composite kernel", "RFF kernel", "other kernel kind", "more than 512 training points", "row shards"])
def test_gradient_refuses_what_it_cannot_differentiate_before_the_fit(case):
    from baybe_amd.recommenders import HipBotorchRecommender

    error, text, how = _refusal_cases()[case]
    space, rng = _space(6, task=how.get("task", False))
    rec = HipBotorchRecommender(surrogate_model=_UntouchableSurrogate(**how.get("surrogate", {})), continuous_optimizer="gradient",
                                **how.get("rec", {}))
    with pytest.raises(error, match=text) as info:
        rec.recommend(1, space, how.get("objective", _objective()), _measurements(space, rng, how.get("n", 8)))
    assert "BotorchRecommender" in str(info.value)  # says what to use instead


# ---- the closed-form oracle against finite differences -----------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["matern32", "matern52", "rbf"])
def test_posterior_grad_oracle_against_central_differences(kernel):
    """n = 24, two discrete and six continuous columns.  |g - FD_{h/2}| <= |FD_h - FD_{h/2}| + 16 eps |f| / h at h = 1e-4 for the
    derivatives of ``GPModel.posterior`` and of the cross-covariance row of the joint posterior (the cross term of
    ``qlogei_with_pending``'s block form).  The case sits in the h^2 regime (observed |g - FD_{h/2}| about 1/3 of the bound,
    |FD_h - FD_{h/2}| about 4e-8 on gradients of 0.3 to 1.5): scaling ranges near 1, lengthscales about 0.4 of the box, rows within
    0.3 of the box of each other (tests/_continuous_cases.py says why)."""
    spec, prm, Xt, y, lo, hi = make_case(kernel, True, 24, 6, seed=3)
    om = oracle_model(spec, prm, Xt, y)
    X = random_rows(lo, hi, 5, seed=9, spread=0.3)
    pend = random_rows(lo, hi, 3, seed=11, spread=0.3)
    cols = [2, 3, 4, 5, 6, 7]
    ref = posterior_grad_oracle(om, X, cols, pend)
    mu, var = om.posterior(X)
    assert np.allclose(ref["mean"], mu, rtol=1e-13) and np.allclose(ref["var"], var, rtol=1e-10)
    h = 1e-4

    def cross_row(x):
        return om.posterior_joint(np.vstack([x[None, :], pend]))[1][0, 1:]

    functions = {"dmean": lambda x: om.posterior(x[None, :])[0][0], "dvar": lambda x: om.posterior(x[None, :])[1][0], "dcross": cross_row}
    worst = 0.0
    for i in range(len(X)):
        assert np.allclose(ref["cross"][i], cross_row(X[i]), rtol=1e-9)
        for k, c in enumerate(cols):
            for key, fun in functions.items():
                g = ref[key][i, k] if key != "dcross" else ref[key][i, :, k]
                holds, err, bound = two_step_ok(g, central_difference(fun, X[i], c, h), central_difference(fun, X[i], c, h / 2), fun(X[i]), h)
                worst = max(worst, float(np.max(err / bound)))
                assert np.all(holds), (key, i, c, err, bound)
    print(f"{kernel}: worst |g - FD_h/2| / bound = {worst:.3f}")
