"""Plain qNEHVI on the device against the restatement on the frozen oracle (``tests/_nparego_reference.py::qnehvi_scores``: the mean
over samples of ``oracle/nehvi_oracle.py::hvi_from_cells`` with qLogNEHVI's per-sample cells): scores, a greedy batch with a pending
row, device cells against host cells, the plug-in surface.  Problems: ``tests/_pareto_cases.py`` (n = 24, N = 150, d = 3).

Tolerance: ``rtol = 1e-9`` (the qNEI bound) plus ``atol = 1e-9 prod_o (max_b y_o - ref_o)`` - the conditional means are held to 1e-9 of
the outputs' scale, and a score is a sum of products of m clipped lengths each at most about ``max_b y_o - ref_o``."""

import numpy as np
import pytest

import _nparego_reference as ref
from _pareto_cases import coincides_with_baseline, setup

pytestmark = pytest.mark.gpu
RTOL = 1e-9
COMBOS = [(2, None), (3, None), (2, [1.0, -1.0])]  # the sign / m combinations of tests/test_nehvi_gpu.py::test_scores_match_oracle


def _problem(m, signs):
    from baybe_amd.nehvi import compute_ref_point

    X, Xt, Y, signs, engines, models = setup(m, signs)
    obj = Y * signs[None, :]
    ref_point = compute_ref_point(obj)
    atol = 1e-9 * float(np.prod(obj.max(0) - ref_point))
    return X, Xt, signs, engines, models, ref_point, atol


def _tag(m, signs):
    return f"m={m},signs={'mixed' if (signs < 0).any() else 'max'}"


@pytest.mark.parametrize("m,signs", COMBOS)
def test_scores_match_the_restatement(m, signs):
    """S = 32, sampler seed 11, no pruning, the first 60 candidates without those that coincide with a baseline row (57 compared).  A
    copy of a baseline point is that point's sampled value + sd z_x with sd <= 1e-4 per target (jitter 1e-8): its improvement is at
    most a 1e-4-wide shell around the sampled front - below 1e-3 for targets of unit scale on either side."""
    import torch

    from baybe_amd.nehvi import HipNEHVIPlain
    from conftest import record_deviation

    X, Xt, signs, engines, models, ref_point, atol = _problem(m, signs)
    S, seed = 32, 11
    dup = coincides_with_baseline(X[:60], Xt)
    so = ref.qnehvi_scores(models, signs, Xt, ref_point, ref.base_samples(S, len(Xt), m, seed), X[:60])
    top2 = np.sort(so[~dup])[-2:]
    print(f"{_tag(m, signs)}: {(so[~dup] > 0).sum()} of {(~dup).sum()} reference scores are non-zero, best two {top2[1]:.4e} / {top2[0]:.4e}")
    assert (so[~dup] > 0).sum() >= 10 and top2[1] - top2[0] > 1e-3
    hv = HipNEHVIPlain(engines, signs, Xt, ref_point, n_mc_samples=S, prune_baseline=False)
    hv.prepare(seed)
    assert hv._cells_on_device
    sg = hv.score(torch.from_numpy(X).cuda()).cpu().numpy()[:60]
    dev = np.abs(sg - so)[~dup]
    excess = (dev - RTOL * np.abs(so[~dup])).max()
    print(f"{_tag(m, signs)}: max |device - restatement| = {dev.max():.3e}, beyond rtol {excess:.3e} (atol {atol:.3e})")
    record_deviation(f"qnehvi_scores_small_beyond_rtol[{_tag(m, signs)}]", max(excess, 0.0), atol)
    assert np.allclose(sg[~dup], so[~dup], rtol=RTOL, atol=atol), dev.max()
    assert (sg[~dup][so[~dup] == 0.0] <= atol).all() and (sg >= 0).all()
    assert (sg[dup] < 1e-3).all() and (so[dup] < 1e-3).all()
    assert int(np.argmax(sg)) == int(np.argmax(so))


def test_greedy_with_a_pending_row_matches_the_restatement():
    """q = 3, S = 32, sampler seed 5, prune seed 9, candidate row 100 pending; pruning, cells and the greedy loop are qLogNEHVI's."""
    import torch

    from baybe_amd.nehvi import HipNEHVIPlain
    from conftest import record_deviation
    from oracle import nehvi_oracle as no

    m = 2
    X, Xt, signs, engines, models, ref_point, atol = _problem(m, None)
    S, seed, pseed = 32, 5, 9
    pending = X[100:101]
    Xd = torch.from_numpy(X).cuda()
    hv = HipNEHVIPlain(engines, signs, Xt, ref_point, n_mc_samples=S, prune_baseline=True)
    res = hv.greedy(Xd, 3, seed=seed, prune_seed=pseed, X_pending=pending)
    keep = no.prune_baseline(models, signs, Xt, ref_point, pseed)
    assert np.array_equal(hv._pruned, Xt[keep])
    picks, vals = ref.qnehvi_greedy(models, signs, Xt[keep], ref_point, X, 3, S, seed, X_pending=pending)
    dev = np.abs(np.array(res.values) - np.array(vals))
    print(f"greedy picks {res.indices} (restatement {picks}), values {vals}, max deviation {dev.max():.3e}")
    record_deviation("qnehvi_greedy_values_beyond_rtol", max(float((dev - RTOL * np.abs(vals)).max()), 0.0), atol)
    assert min(vals) > 0  # (a step whose best value is 0 would be decided by ties alone)
    assert res.indices == picks
    assert np.allclose(res.values, vals, rtol=RTOL, atol=atol)
    assert len(hv.X_b_current) == len(keep) + 1 + 2
    alive = torch.ones(len(X), dtype=torch.uint8, device="cuda")
    alive[[3, 149]] = 0
    sc = hv.score(Xd, alive).cpu().numpy()
    assert np.isneginf(sc[[3, 149]]).all() and np.isfinite(np.delete(sc, [3, 149])).all()


@pytest.mark.parametrize("m,signs", COMBOS)
def test_device_cells_equal_host_cells(m, signs):
    """``bbh_qnehvi_cells`` on the device-resident cell lists against ``bbh_qnehvi_sm`` on the host set-up's cells (baseline posterior ->
    host Cholesky -> host samples / decompositions): the same pruned baseline, the same scores."""
    import torch

    from baybe_amd.nehvi import HipNEHVIPlain
    from conftest import record_deviation

    X, Xt, signs, engines, models, ref_point, atol = _problem(m, signs)
    Xd = torch.from_numpy(X).cuda()
    out = {}
    for mode in ("device", "host"):
        hv = HipNEHVIPlain(engines, signs, Xt, ref_point, n_mc_samples=33, prune_baseline=True)
        hv.device_setup = mode == "device"
        hv.prepare(21, prune_seed=22)
        assert hv._cells_on_device == (mode == "device")
        out[mode] = (hv._pruned.copy(), hv.score(Xd).cpu().numpy())
        if mode == "device":  # ... and the host-cell entry point on the very same cells, read back (side lengths as exp(log(len)))
            hv.cell_off, hv.cell_lo, hv.cell_ll = hv.cells()
            hv._cells_on_device = False
            assert np.allclose(hv.score(Xd).cpu().numpy(), out[mode][1], rtol=1e-12, atol=atol)
    assert np.array_equal(out["device"][0], out["host"][0])
    sd, sh = out["device"][1], out["host"][1]
    dup = coincides_with_baseline(X, Xt)
    dev = np.abs(sd - sh)[~dup]
    record_deviation(f"qnehvi_device_vs_host_cells_beyond_rtol[{_tag(m, signs)}]", max(float((dev - RTOL * np.abs(sh[~dup])).max()), 0.0), atol)
    assert (sh[~dup] > 0).any()
    assert np.allclose(sd[~dup], sh[~dup], rtol=RTOL, atol=atol), dev.max()
    assert int(np.argmax(sd)) == int(np.argmax(sh))


def test_recommend_through_the_plugin_surface():
    """``recommend()`` with ``"qNEHVI"`` on a two-target ``ParetoObjective`` over a 512-row space: the restatement's greedy batch for the
    hyper-parameters the device fitted (scoring seed drawn first, then the pruning seed; reference point from the measurements)."""
    import torch
    from _baybe_shim import NumericalDiscreteParameter, NumericalTarget, ParetoObjective, SearchSpace
    from _pareto_cases import targets
    from _problems import oracle_params, oracle_spec
    from baybe_amd import acquisition as A
    from baybe_amd.engine import draw_sampler_seed
    from baybe_amd.recommenders import HipBotorchRecommender
    from oracle import gp_oracle as go
    from oracle import nehvi_oracle as no

    rng = np.random.default_rng(2)
    vals = np.arange(8) / 7.0
    space = SearchSpace.from_product([NumericalDiscreteParameter(f"x{i}", vals) for i in range(3)])
    exp = space.discrete.exp_rep
    meas = exp.iloc[rng.choice(len(exp), 18, replace=False)].copy()
    T = targets(meas[["x0", "x1", "x2"]].to_numpy(float), rng)
    meas["t1"], meas["t2"] = T[:, 0], -T[:, 1]
    obj = ParetoObjective([NumericalTarget("t1"), NumericalTarget("t2", minimize=True)])
    rec = HipBotorchRecommender(acquisition_function=A.qNEHVI(n_mc_samples=32))
    torch.manual_seed(31)
    got = rec.recommend(2, space, obj, meas)
    assert type(rec._scorer).__name__ == "HipNEHVIPlain"
    torch.manual_seed(31)
    seed, pseed = draw_sampler_seed(), draw_sampler_seed()
    models = []
    for sub in rec._surrogate_model.models:
        eng = sub.engine
        models.append(go.GPModel(oracle_spec(eng.spec), oracle_params(eng.spec, eng.params), eng._X_train, eng._y_train))
    signs = np.array([1.0, -1.0])
    Xb = space.transform(meas, allow_extra=True).to_numpy(dtype=np.float64)
    ref_point = no.compute_ref_point(meas[["t1", "t2"]].to_numpy() * signs[None, :])
    keep = no.prune_baseline(models, signs, Xb, ref_point, pseed)
    comp = space.discrete.comp_rep.to_numpy(dtype=np.float64)
    picks, vals = ref.qnehvi_greedy(models, signs, Xb[keep], ref_point, comp, 2, 32, seed)
    assert min(vals) > 0
    assert list(got.index) == list(exp.index[picks]), (list(got.index), picks)
    acq = rec.acquisition_values(exp.iloc[:50], space, obj, meas)
    assert np.isfinite(acq.to_numpy()).all() and (acq.to_numpy() >= 0).all()


# ---- the sample-slice scaffold (csrc/bbh_slices.h) at its edges -------------------------------------------------------------------
EDGE_ROWS = np.r_[0:60, 250:257]  # of N = 257: the second 256-row block of the scoring grid holds one row


@pytest.mark.parametrize("S", [1, 9, 33])
@pytest.mark.parametrize("m,signs", [(2, [1.0, -1.0]), (3, None)])
def test_scores_match_the_restatement_at_the_slice_edges(m, signs, S):
    """``bbh_qnehvi_kernel`` (fixed slices of 8 samples) and the shared finish kernel at N = 257 (two blocks of candidates): S = 1 is
    less than one slice, S = 9 and S = 33 leave one sample in the last slice.  Rows 0 ... 59 and 250 ... 256 against the restatement
    under the tolerance rule of this module (rows coinciding with a baseline row excluded); one compared row is masked and scores
    -inf.  From S = 9 on at least one compared reference score is non-zero (an all-zero comparison would pass a kernel that adds
    nothing)."""
    import torch

    from baybe_amd.nehvi import HipNEHVIPlain, compute_ref_point
    from conftest import record_deviation

    X, Xt, Y, signs, engines, models = setup(m, signs, N=257)
    obj = Y * signs[None, :]
    ref_point = compute_ref_point(obj)
    atol = 1e-9 * float(np.prod(obj.max(0) - ref_point))
    seed = 11
    dup = coincides_with_baseline(X[EDGE_ROWS], Xt)
    masked = int(EDGE_ROWS[~dup][3])
    held = ~dup & (EDGE_ROWS != masked)
    so = ref.qnehvi_scores(models, signs, Xt, ref_point, ref.base_samples(S, len(Xt), m, seed), X[EDGE_ROWS])
    tag = f"{_tag(m, signs)},S={S}"
    print(f"{tag}: {(so[held] > 0).sum()} of {held.sum()} compared reference scores are non-zero")
    assert held.sum() >= 60 and held[-1] and np.isfinite(so).all()
    assert S < 9 or (so[held] > 0).sum() >= 1
    hv = HipNEHVIPlain(engines, signs, Xt, ref_point, n_mc_samples=S, prune_baseline=False)
    hv.prepare(seed)
    alive = torch.ones(len(X), dtype=torch.uint8, device="cuda")
    alive[masked] = 0
    sg = hv.score(torch.from_numpy(X).cuda(), alive).cpu().numpy()
    assert np.isneginf(sg[masked]) and (np.delete(sg, masked) >= 0).all() and np.isfinite(np.delete(sg, masked)).all()
    dev = np.abs(sg[EDGE_ROWS] - so)[held]
    excess = (dev - RTOL * np.abs(so[held])).max()
    print(f"{tag}: max |device - restatement| = {dev.max():.3e}, beyond rtol {excess:.3e} (atol {atol:.3e})")
    record_deviation(f"qnehvi_scores_slice_edges_beyond_rtol[{tag}]", max(excess, 0.0), atol)
    assert np.allclose(sg[EDGE_ROWS][held], so[held], rtol=RTOL, atol=atol), dev.max()
