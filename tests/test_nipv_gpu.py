"""qNIPV on the device against the oracle's DIRECT form (tests/_oracle_nipv.py (a): the GP conditioned on X u B u {x} by Cholesky), per
candidate, through the C-ABI (``bbh_nipv_set_points`` / ``bbh_nipv_gain`` behind ``HipGP.nipv_set_points`` / ``nipv_gain``; the
variance and cross-covariance operands come from the device's own ``bbh_posterior`` / ``bbh_cross_cov`` passes and the conditioning
terms from ``HipNIPV.conditioning_terms``, i.e. the path a recommendation takes).  Cases, special rows and the guard of both:
tests/_nipv_cases.py, tests/test_nipv_cpu.py.

Bound per candidate (the issue's, from oracle quantities): ``C_BOUND (n + b + 16) eps [2 sum_j |C_j| S_j + gain D] / den`` with
``C_BOUND`` from ``profiles/nipv_observed_deviations.json`` (tests/_nipv_cases.py).  Bounds this file sets itself: ``var(p_j)`` is a
posterior variance from the same factorisation as ``bbh_posterior``'s and is held to what tests/_pending_cases.py holds that to,
1e-11 of the prior variance; the reported value ``gain / M - V_B`` adds ``V_B``, a mean of such variances and covariances, so it is
held to ``C_BOUND tol / M`` plus 1e-11 of the prior variance."""

import os

import numpy as np
import pytest

import _nipv_cases as nc
import _oracle_nipv as on

pytestmark = pytest.mark.gpu

SWITCHES = ("BBH_NIPV_TILE", "BBH_NIPV_SLICE")
VARIANTS = {"default": {}, "tile16": {"BBH_NIPV_TILE": "16"}, "tile32": {"BBH_NIPV_TILE": "32"}, "unsliced": {"BBH_NIPV_SLICE": "0"}}
FORM_OF = {"tile16": 0, "tile32": 1}
VAR_TOL = 1e-11  # posterior variances scaled to the prior variance (tests/_pending_cases.py TOL)


@pytest.fixture(scope="module")
def handles():
    from baybe_amd import engine

    keep = {k: os.environ.get(k) for k in SWITCHES}
    made = {}
    try:
        for name, env in VARIANTS.items():
            for k in SWITCHES:
                os.environ.pop(k, None)
            os.environ.update(env)
            made[name] = engine.HipGP(0)  # (a handle reads the BBH_* switches when it is created)
    finally:
        for k, val in keep.items():
            os.environ.pop(k, None) if val is None else os.environ.__setitem__(k, val)
    yield made
    for g in made.values():
        g.close()


def _load(g, case, params=None):
    c = case.build()
    spec, prm = nc.device_spec(case)
    g.set_model(spec, np.array(c.Xt), np.array(c.y))
    g.factorize(prm if params is None else params)
    assert abs(g.ysd - c.om.ysd) <= 1e-13 * c.om.ysd and g.jitter == 0.0, (case.id, g.ysd, c.om.ysd, g.jitter)
    return c


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


def _record(name, ratio):
    from conftest import record_deviation

    print(f"{name}: observed |device - oracle| / tol(c = 1) = {ratio:.3f} (held to C_BOUND = {nc.C_BOUND})")
    record_deviation(f"nipv/{name}", ratio, float(nc.C_BOUND))


def _ratio(got, ref, tol, rows):
    return float((np.abs(got[rows] - ref[rows]) / tol[rows]).max())


# (one row and one column: nothing a tile width or a slice width changes - those cases run under the default only)
CASE_VARIANTS = [(c, v) for c in nc.CASES for v in VARIANTS if v == "default" or not (c.N == 1 and c.M == 1)]


@pytest.mark.parametrize("case,variant", CASE_VARIANTS, ids=lambda p: getattr(p, "id", p))
def test_gain_against_oracle(handles, case, variant):
    from baybe_amd.nipv import HipNIPV

    g = handles[variant]
    c = _load(g, case)
    a, s = case.reference()
    hn = HipNIPV(g, np.array(c.P))
    X, alive = _dev(c.X), _dev(c.alive)
    gain_t, v_b = hn.gain(X, np.array(c.B), alive)
    gain = gain_t.cpu().numpy()
    live = c.alive.astype(bool)
    prior = c.om.ysd**2
    # var(p_j) as bbh_nipv_set_points returns it, V_B, the gain and the reported value
    assert np.abs(hn._var_p - s.var_p).max() <= VAR_TOL * prior, case.id
    assert abs(v_b - a.v_b) <= VAR_TOL * prior, (case.id, v_b, a.v_b)
    ratio = _ratio(gain, a.gain, s.tol, live)
    _record(f"gain[{case.id},{variant}]", ratio)
    assert np.all(np.isneginf(gain[~live])) and np.all(np.isfinite(gain[live])), case.id
    value = hn.score(X, np.array(c.B), alive=alive).cpu().numpy()
    dev_v = np.abs(value[live] - a.value[live]) - nc.C_BOUND * s.tol[live] / case.M
    assert ratio <= nc.C_BOUND, (case.id, variant, ratio)
    assert dev_v.max() <= VAR_TOL * prior, (case.id, dev_v.max())
    if variant in FORM_OF:
        assert g.nipv_last_form() == FORM_OF[variant], (variant, g.nipv_last_form())
    # two runs give equal bits; equal rows at different positions give equal bits
    again = hn.gain(X, np.array(c.B), alive)[0].cpu().numpy()
    assert np.array_equal(gain, again, equal_nan=True), case.id
    if case.N >= 17:
        assert gain[3] == gain[-1], (case.id, gain[3], gain[-1])
        # ... and whatever else is scored with them: the row alone, at position 0 of a one-row call
        alone = hn.gain(_dev(c.X[3:4]), np.array(c.B))[0].cpu().numpy()
        assert alone[0] == gain[3], (case.id, alone[0], gain[3])


def test_fused_pass_against_existing_passes(handles):
    """The gain assembled on the device from the passes the library already had - ``cross_cov_many`` for cov(x, P), cov(x, B) and
    cov(B, P), ``posterior`` for var(x), ``set_pending`` for cov(B, B), torch reductions - against the fused pass, under the bound."""
    import torch

    case = nc.ASSEMBLY_CASE
    g = handles["default"]
    c = _load(g, case)
    a, s = case.reference()
    from baybe_amd.nipv import HipNIPV

    hn = HipNIPV(g, np.array(c.P))
    X = _dev(c.X)
    fused = hn.gain(X, np.array(c.B))[0]
    s2 = g.ysd**2 * c.noise
    g.set_pending(None)
    var = g.posterior(X)[1]
    cov_xp = g.cross_cov_many(X, np.array(c.P))  # [N, M]
    cov_bp = g.cross_cov_many(_dev(c.B), np.array(c.P))  # [b, M]
    _, cpp = g.set_pending(np.array(c.B))
    cov_xb = g.cross_cov(X)  # [N, b]
    g.set_pending(None)
    ginv = torch.linalg.inv(torch.from_numpy(np.asarray(cpp)).cuda() + s2 * torch.eye(case.b, dtype=torch.float64, device="cuda"))
    C = cov_xp - cov_xb @ (ginv @ cov_bp)
    den = torch.clamp(var - ((cov_xb @ ginv) * cov_xb).sum(1), min=0.0) + s2
    assembled = (C * C).sum(1) / den
    tol = torch.from_numpy(np.array(s.tol)).cuda()
    ratio = float(((fused - assembled).abs() / tol).max())
    _record(f"assembly[{case.id}]", ratio)
    assert ratio <= nc.C_BOUND, ratio
    assert _ratio(assembled.cpu().numpy(), a.gain, s.tol, slice(None)) <= nc.C_BOUND


def test_second_factorisation_invalidates_the_operand(handles):
    """``bbh_nipv_set_points`` after a second ``bbh_factorize``: the stale A is refused, and not used once the points are set again."""
    from baybe_amd._lib import HipError
    from baybe_amd.nipv import HipNIPV
    from oracle import gp_oracle as go

    case = nc.REFACTOR_CASE
    g = handles["default"]
    c = _load(g, case)
    hn = HipNIPV(g, np.array(c.P))
    X = _dev(c.X)
    first = hn.gain(X, np.array(c.B))[0].cpu().numpy()
    spec, prm = nc.device_spec(case)
    prm2 = type(prm)(np.array(c.ls) * 1.4, c.noise * 2.0, 0.1)
    g.factorize(prm2)
    var = g.posterior(X)[1]
    with pytest.raises(HipError, match="no integration points set for the current factorisation"):
        g.nipv_gain(X, var)
    om2 = go.GPModel(c.om.spec, go.GPParams(np.array(c.ls) * 1.4, c.noise * 2.0, 0.1), np.array(c.Xt), np.array(c.y))
    a2, s2 = on.direct(om2, c.X, c.B, c.P), on.schur(om2, c.X, c.B, c.P)
    second = HipNIPV(g, np.array(c.P)).gain(X, np.array(c.B))[0].cpu().numpy()
    ratio = _ratio(second, a2.gain, s2.tol, slice(None))
    _record(f"refactorised[{case.id}]", ratio)
    assert ratio <= nc.C_BOUND, ratio
    assert np.abs(second - first).max() > 1e3 * s2.tol.max()  # (the two factorisations are told apart by far more than the bound)


def test_budget_refusal(handles):
    """An M whose resident operand exceeds the budget is refused with a text; the handle keeps working."""
    from baybe_amd._lib import HipError

    case = nc.CASES[1]  # d = 1, np = 64: (64 + 16) Mpad 8 bytes > 256 MiB beyond 419 430 columns
    g = handles["default"]
    c = _load(g, case)
    with pytest.raises(HipError, match="over the budget of 256 MiB"):
        g.nipv_set_points(np.zeros((420000, 1)))
    assert np.all(np.isfinite(g.nipv_set_points(np.array(c.P))))


@pytest.mark.parametrize("case", nc.GREEDY_CASES, ids=lambda c: c.id)
def test_greedy_against_oracle(handles, case):
    """Batches of 3 with 2 pending rows: at every step the oracle can decide (top-two gap above the sum of both rows' bounds) the
    device's argmax on the gain is the oracle's pick, every step conditioned on the oracle's earlier picks; and ``greedy`` itself
    returns the oracle's batch when every step is decidable."""
    from baybe_amd.nipv import HipNIPV

    g = handles["default"]
    c = _load(g, case)
    steps = nc.greedy_reference(case.id)
    hn = HipNIPV(g, np.array(c.P))
    X = _dev(c.X)
    alive = _dev(c.alive)
    for st in steps:
        gain, _ = hn.gain(X, st.pending, alive)
        val, idx = g.argmax(gain)
        print(f"{case.id}: oracle pick {st.index} gap {st.gap:.3e} bound {nc.C_BOUND * st.tol2:.3e}; device pick {int(idx)}")
        if nc.decidable(st):
            assert int(idx) == st.index, (case.id, int(idx), st.index)
            assert abs(float(val) - st.gain) <= nc.C_BOUND * st.tol2
        alive[st.index] = 0
    if all(nc.decidable(st) for st in steps):
        res = hn.greedy(X, nc.GREEDY_Q, X_pending=np.array(c.B), alive=_dev(c.alive))
        assert res.indices == [st.index for st in steps], (case.id, res.indices)


def test_recommender_end_to_end():
    """``HipBotorchRecommender(nipv="device", acquisition_function=qNIPV(sampling_n_points=..., sampling_method="FPS"))`` on a small
    product grid: ``recommend`` returns the oracle's greedy batch under the device's fitted hyper-parameters and the device's
    integration points, a MIN and a MAX target give the same batch, and the read-backs match the oracle's values."""
    from baybe_amd.acquisition import qNIPV
    from baybe_amd.exceptions import IncompatibleAcquisitionFunctionError
    from baybe_amd.recommenders import HipBotorchRecommender
    from oracle import gp_oracle as go

    with pytest.raises(IncompatibleAcquisitionFunctionError, match="nipv='device'"):
        HipBotorchRecommender(acquisition_function="qNIPV")
    batches = []
    for minimize in (False, True):
        space, meas, objective = nc.campaign_problem(minimize)
        exp = space.discrete.exp_rep
        Xc, X_all = exp.to_numpy(float), meas[["x0", "x1", "x2"]].to_numpy(float)
        pend_df = exp.iloc[[100]]
        rec = HipBotorchRecommender(nipv="device", acquisition_function=qNIPV(sampling_n_points=nc.CAMPAIGN_POINTS, sampling_method="FPS"))
        np.random.seed(5)  # (the tie-breaks of farthest point sampling on a grid)
        got = rec.recommend(nc.CAMPAIGN_BATCH, space, objective, meas, pending_experiments=pend_df)
        batches.append(got.index.tolist())
        P = rec._scorer.P
        assert P.shape == (nc.CAMPAIGN_POINTS, 3)
        prm = rec._surrogate_model.engine.params
        om = go.GPModel(go.GPSpec.baybe_default(3, np.zeros(3), np.ones(3)), go.GPParams(prm.lengthscale, prm.noise, prm.mean), X_all,
                        meas["t"].to_numpy())
        alive = exp.index.isin(space.discrete.get_candidates()[0].index)
        steps = on.greedy(om, Xc, nc.CAMPAIGN_BATCH, P, pending=Xc[[100]], alive=alive)
        assert all(st.gap > 100 * nc.C_BOUND * st.tol2 for st in steps), [(st.gap, st.tol2) for st in steps]
        assert got.index.tolist() == exp.index[[st.index for st in steps]].tolist()
        np.random.seed(6)
        acq = rec.acquisition_values(exp.iloc[:60], space, objective, meas, pending_experiments=pend_df).to_numpy()
        P = rec._scorer.P
        a, s = on.direct(om, Xc[:60], Xc[[100]], P), on.schur(om, Xc[:60], Xc[[100]], P)
        dev = np.abs(acq - a.value) - nc.C_BOUND * s.tol / len(P)
        assert dev.max() <= VAR_TOL * om.ysd**2, dev.max()
        np.random.seed(7)
        jv = rec.joint_acquisition_value(exp.iloc[[3, 140, 77]], space, objective, meas, pending_experiments=pend_df)
        P = rec._scorer.P
        rest = Xc[[140, 77, 100]]
        aj, sj = on.direct(om, Xc[[3]], rest, P), on.schur(om, Xc[[3]], rest, P)
        assert abs(jv - aj.value[0]) <= nc.C_BOUND * sj.tol[0] / len(P) + VAR_TOL * om.ysd**2, (jv, aj.value[0])
    assert batches[0] == batches[1], batches
