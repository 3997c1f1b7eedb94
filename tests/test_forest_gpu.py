"""The forest kernels against scikit-learn's recorded predictions and the numpy oracle (tests/_oracle_forest.py), on the fixtures of
tests/_forest_cases.py.

Held to:
  bbh_forest_predict, LDS and global path      np.array_equal with the recorded ``estimator.predict`` outputs
  moments, mean                                <= 2 T 2^-53 max|P| absolute     (fp64 summation of T terms)
  moments, variance                            <= 8 T 2^-53 max|P|^2 absolute, exactly 0 for T = 1
  fused scores, every MC kind, k in {0, 1, 15}, with and without ``alive``: rtol 1e-9, atol 1e-10 (the GP family's bounds)
  duplicated rows: equal bits, first index; two runs: equal bits; greedy batches of 1, 3, 5: the oracle's indices on every case.
``MIXED`` (trees of 199 to 1399 nodes in one forest) holds the same calls to the same bounds with the LDS / global border at
{default, 0, 198, 199, 658, 659, 1022, 1023} nodes - equal bits across all of them -, each tree as a pass's first, k = 63 pending points,
rows read through a stride of 7, and the device's node guard on a table the host check never saw.
Observed maxima are printed and recorded (conftest.record_deviation)."""

import functools

import numpy as np
import pytest

import _forest_cases as fc
import _oracle_forest as of
from conftest import record_deviation

pytestmark = pytest.mark.gpu

STORED = [n for n in fc.CASES if "like" not in fc.CASES[n]]
EPS = 2.0**-53


@functools.lru_cache(maxsize=None)
def golden():
    return fc.load_golden()


@functools.lru_cache(maxsize=None)
def engine_of(name):
    """The device forest of a stored case (one handle per case for the whole module)."""
    from baybe_amd.forest import HipForestEngine

    g = golden()[name]
    eng = HipForestEngine(0)
    eng._X_train = g["train_x"]
    eng.set_forest(g["packed"], g["X"].shape[1])
    return eng


@functools.lru_cache(maxsize=None)
def context(name):
    """(case, engine, X, P [T, N] = scikit-learn's recorded predictions, idx, counts, best_f) - computed once, never modified."""
    from baybe_amd.forest import ensemble_member_indices

    c = fc.case(name)
    g = golden()[fc.stored_name(name)]
    P = g["pred"]
    idx = ensemble_member_indices(c["S"], P.shape[0], c["sampler"])
    return c, engine_of(fc.stored_name(name)), g["X"], P, idx, of.best_f(g["pred_train"], c["sign"])


class _Holder:
    """What HipForestAcq reads of a surrogate."""

    def __init__(self, engine):
        self.engine = engine


def _acq(name, kind):
    from baybe_amd.forest import HipForestAcq

    c, eng, X, P, idx, best = context(name)
    return HipForestAcq(_Holder(eng), kind, c["sign"], best, c["S"])


@pytest.mark.parametrize("name", STORED)
def test_predict_equals_scikit_learn_on_both_paths(name):
    g = golden()[name]
    eng = engine_of(name)
    assert eng.forest["max_nodes"] <= eng.forest_lds_nodes()
    for rows, want in ((g["X"], g["pred"]), (g["train_x"], g["pred_train"])):
        Xd = eng._as_dev(rows)
        assert np.array_equal(eng.forest_predict(eng.forest, Xd).cpu().numpy(), want), "LDS path"
        assert np.array_equal(eng.forest_predict(eng.forest, Xd, lds_nodes=0).cpu().numpy(), want), "global path"


def test_tree_above_the_lds_budget_takes_the_global_path():
    """3 trees on 5000 x 2 rows: more nodes per tree than the LDS tables hold, so the default call walks them in global memory -
    predictions equal scikit-learn's, moments and a fused score equal the oracle's."""
    pytest.importorskip("sklearn")
    from baybe_amd.forest import HipForestEngine, ensemble_member_counts, ensemble_member_indices, pack_forest

    c = fc.BIG
    estimators, X, train_x, _ = fc.fit_case("big", c)
    packed = pack_forest(estimators)
    eng = HipForestEngine(0)
    eng.set_forest(packed, c["d"])
    assert np.diff(packed["offsets"]).min() > eng.forest_lds_nodes()
    want = np.stack([e.predict(X) for e in estimators])
    Xd = eng._as_dev(X)
    assert np.array_equal(eng.forest_predict(eng.forest, Xd).cpu().numpy(), want)
    mean, var = eng.forest_moments(eng.forest, Xd)
    mo, vo = of.moments(want)
    T, big = want.shape[0], np.abs(want).max()
    assert np.abs(mean.cpu().numpy() - mo).max() <= 2 * T * EPS * big and np.abs(var.cpu().numpy() - vo).max() <= 8 * T * EPS * big * big
    import torch

    idx = ensemble_member_indices(c["S"], T, c["sampler"])
    counts = ensemble_member_counts(c["S"], T, c["sampler"])
    best = of.best_f(np.stack([e.predict(train_x) for e in estimators]), 1.0)
    dev = eng._dev()
    got = eng.forest_mc_acq(eng.forest, "qLogEI", Xd, torch.from_numpy(counts).to(dev),
                            torch.from_numpy(np.nonzero(counts)[0].astype(np.int32)).to(dev), c["S"], None, best, 1.0)
    assert np.allclose(got.cpu().numpy(), of.scores("qLogEI", want, None, idx, best, 1.0), rtol=1e-9, atol=1e-10)
    eng.close()


@pytest.mark.parametrize("name", list(fc.WIDE))
def test_wide_rows_take_the_smaller_tiles(name):
    """d = 121 and d = 231: the tile of a workgroup is 128 and 64 rows (130 rows: more than one tile either way) - same predictions,
    moments and scores."""
    pytest.importorskip("sklearn")
    import torch

    from baybe_amd.forest import HipForestEngine, ensemble_member_counts, ensemble_member_indices, pack_forest

    c = fc.WIDE[name]
    estimators, X, train_x, _ = fc.fit_case(name, c)
    eng = HipForestEngine(0)
    eng.set_forest(pack_forest(estimators), c["d"])
    want = np.stack([e.predict(X) for e in estimators])
    Xd = eng._as_dev(X)
    assert np.array_equal(eng.forest_predict(eng.forest, Xd).cpu().numpy(), want)
    mean, var = eng.forest_moments(eng.forest, Xd)
    mo, vo = of.moments(want)
    T, big = want.shape[0], np.abs(want).max()
    assert np.abs(mean.cpu().numpy() - mo).max() <= 2 * T * EPS * big and np.abs(var.cpu().numpy() - vo).max() <= 8 * T * EPS * big * big
    idx = ensemble_member_indices(c["S"], T, c["sampler"])
    counts = ensemble_member_counts(c["S"], T, c["sampler"])
    best = of.best_f(np.stack([e.predict(train_x) for e in estimators]), c["sign"])
    dev = eng._dev()
    pend = torch.from_numpy(np.ascontiguousarray(want[:, :2])).to(dev)
    for kind in ("qLogEI", "qUCB"):
        got = eng.forest_mc_acq(eng.forest, kind, Xd, torch.from_numpy(counts).to(dev),
                                torch.from_numpy(np.nonzero(counts)[0].astype(np.int32)).to(dev), c["S"], pend, best, c["sign"])
        assert np.allclose(got.cpu().numpy(), of.scores(kind, want, want[:, :2], idx, best, c["sign"]), rtol=1e-9, atol=1e-10)
    eng.close()


@pytest.mark.parametrize("name", STORED)
def test_moments_within_the_summation_bounds(name):
    g = golden()[name]
    eng = engine_of(name)
    P = g["pred"]
    T, big = P.shape[0], np.abs(P).max()
    mo, vo = of.moments(P)
    worst = [0.0, 0.0]
    for lds_nodes in (None, 0):
        mean, var = eng.forest_moments(eng.forest, eng._as_dev(g["X"]), lds_nodes=lds_nodes)
        mean, var = mean.cpu().numpy(), var.cpu().numpy()
        worst = [max(worst[0], np.abs(mean - mo).max()), max(worst[1], np.abs(var - vo).max())]
        if T == 1:
            assert np.array_equal(var, np.zeros_like(var)) and np.array_equal(mean, P[0])
    print(f"forest moments {name}: mean dev {worst[0]:.3e} (bound {2 * T * EPS * big:.3e}), var dev {worst[1]:.3e} "
          f"(bound {8 * T * EPS * big * big:.3e})")
    record_deviation(f"forest_moments_mean[{name}]", worst[0], 2 * T * EPS * big)
    record_deviation(f"forest_moments_var[{name}]", worst[1], 8 * T * EPS * big * big)
    assert worst[0] <= 2 * T * EPS * big
    assert worst[1] <= 8 * T * EPS * big * big


@pytest.mark.parametrize("name", list(fc.CASES))
def test_fused_scores_every_kind_pending_and_mask(name):
    import torch

    c, eng, X, P, idx, best = context(name)
    Xd = eng._as_dev(X)
    worst = 0.0
    for kind in fc.MC_KINDS:
        acq = _acq(name, kind)
        for k in fc.PENDING:
            rows = fc.pending_rows(c["N"], k)
            pend = P[:, rows] if k else None
            acq.prepare(c["sampler"], X[rows] if k else None)
            assert np.array_equal(acq.counts_host, np.bincount(idx, minlength=P.shape[0]))
            want = of.scores(kind, P, pend, idx, best, c["sign"])
            got = acq.score(Xd).cpu().numpy()
            assert np.allclose(got, want, rtol=1e-9, atol=1e-10), (name, kind, k, np.abs(got - want).max())
            worst = max(worst, float((np.abs(got - want) / (1e-10 + 1e-9 * np.abs(want))).max()))  # share of the allowance used
            # a mask that removes the unmasked winner: masked rows score -inf and never win
            alive = np.ones(c["N"], dtype=np.uint8)
            alive[int(np.argmax(want))] = 0
            masked = acq.score(Xd, torch.from_numpy(alive).to(Xd.device))
            m = masked.cpu().numpy()
            live = alive.astype(bool)
            assert np.all(np.isneginf(m[~live])) and np.array_equal(m[live], got[live])
            if live.any():
                val, i = eng.argmax(masked)
                assert live[i] and i == int(np.argmax(m)) and val == m[i]
    # the global-memory path computes the same bits as the LDS path
    acq = _acq(name, "qLogEI")
    acq.prepare(c["sampler"], X[fc.pending_rows(c["N"], 1)])
    a = acq.score(Xd)
    b = eng.forest_mc_acq(eng.forest, "qLogEI", Xd, acq._counts, acq._order, c["S"], acq._pend, best, c["sign"], lds_nodes=0)
    assert torch.equal(a, b)
    print(f"forest fused scores {name}: worst deviation = {worst:.3e} of the allowance (atol 1e-10 + rtol 1e-9 |oracle|)")
    record_deviation(f"forest_fused_scores_share_of_allowance[{name}]", worst, 1.0)


def test_duplicated_rows_get_equal_bits_and_the_first_index_wins():
    import torch

    c, eng, X, P, idx, best = context("dups")
    Xd = eng._as_dev(X)
    first_of = {}
    for i, row in enumerate(map(bytes, X)):
        first_of.setdefault(row, i)
    twins = [(first_of[bytes(r)], i) for i, r in enumerate(X) if first_of[bytes(r)] != i]
    assert len(twins) >= c["N"] // 2 - 1
    for kind in fc.MC_KINDS:
        acq = _acq("dups", kind)
        acq.prepare(c["sampler"], X[fc.pending_rows(c["N"], 1)])
        s1, s2 = acq.score(Xd), acq.score(Xd)
        assert torch.equal(s1, s2), "two runs of the same call differ"
        s = s1.cpu().numpy()
        for a, b in twins:
            assert s[a] == s[b], (kind, a, b)
        val, i = eng.argmax(s1)
        assert i == int(np.argmax(s)) and i == min(j for j in range(len(s)) if s[j] == s.max())
    mean, var = eng.forest_moments(eng.forest, Xd)
    mean, var = mean.cpu().numpy(), var.cpu().numpy()
    for a, b in twins:
        assert mean[a] == mean[b] and var[a] == var[b]


@pytest.mark.parametrize("name", list(fc.CASES))
def test_greedy_batches_return_the_oracles_indices(name):
    """Batches of 1, 3 and 5, every MC kind, without and with a pending point - nothing is skipped: every step of these runs clears a
    margin of 1e-8 in the oracle (tests/test_forest_cpu.py::test_every_greedy_step_of_every_case_clears_the_margin)."""
    c, eng, X, P, idx, best = context(name)
    Xd = eng._as_dev(X)
    for kind in fc.MC_KINDS:
        acq = _acq(name, kind)
        for k in (0, 1):
            rows = fc.pending_rows(c["N"], k)
            for batch in fc.BATCHES:
                batch = min(batch, c["N"])
                want, values, _ = of.greedy(kind, P, idx, best, c["sign"], batch, P[:, rows] if k else None)
                res = acq.greedy(Xd, batch, seed=c["sampler"], X_pending=X[rows] if k else None)
                assert res.indices == want, (name, kind, k, batch, res.indices, want)
                assert np.allclose(res.values, values, rtol=1e-9, atol=1e-10)


def test_nan_rows_are_refused_whatever_was_checked_before():
    """The guard holds across calls: a clean host array and then one of the same shape with a NaN (the allocator hands the second
    upload the first one's block), pending rows, a fresh device tensor in a freed block, and a checked device tensor written to in
    place.  Only a tensor the caller keeps alive and unchanged is taken as checked."""
    import torch

    c, eng, X, P, idx, best = context("n65_d3_t7")
    clean = np.array(X[:8])
    dirty = clean.copy()
    dirty[5, 1] = np.nan
    for _ in range(2):
        eng.posterior(clean)
        with pytest.raises(ValueError, match="NaN"):
            eng.posterior(dirty)
        with pytest.raises(ValueError, match="NaN"):
            eng.predict(dirty)
    acq = _acq("n65_d3_t7", "qLogEI")
    acq.prepare(c["sampler"], clean)
    with pytest.raises(ValueError, match="NaN"):
        acq.prepare(c["sampler"], dirty)
    dev = eng._dev()
    t = torch.from_numpy(clean).to(dev)
    eng.posterior(t)
    assert eng._nan_free[0]() is t
    del t
    t2 = torch.from_numpy(dirty).to(dev)  # same shape, very likely the same block
    with pytest.raises(ValueError, match="NaN"):
        eng.posterior(t2)
    t3 = torch.from_numpy(clean).to(dev)
    eng.posterior(t3)
    eng.posterior(t3)
    t3[2, 0] = float("nan")  # (bumps the version counter)
    with pytest.raises(ValueError, match="NaN"):
        eng.posterior(t3)
    with pytest.raises(ValueError, match="NaN"):
        acq.score(t3)
    # the resident matrix is looked at once per recommendation: the pending rows' and the pick's predictions do not displace it
    Xd = eng._as_dev(X)
    acq.greedy(Xd, 2, seed=c["sampler"], X_pending=clean[:1])
    assert eng._nan_free[0]() is Xd and eng._nan_free[1] == Xd._version


def test_a_closed_engine_stays_closed_and_a_copy_opens_its_own_handle():
    import copy

    from baybe_amd.forest import HipForestEngine

    g = golden()["stumps"]
    eng = HipForestEngine(0)
    eng.set_forest(g["packed"], g["X"].shape[1])
    want = eng.predict(g["X"]).cpu().numpy()
    twin = copy.deepcopy(eng)
    assert twin._handle is None
    assert np.array_equal(twin.predict(g["X"]).cpu().numpy(), want) and twin._handle is not None
    eng.close(), twin.close()
    assert eng._h is None and twin._h is None  # (no handle is taken from the pool behind the caller's back)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _grid_context(minimize):
    from _baybe_shim import NumericalDiscreteParameter, NumericalTarget, SearchSpace, SingleTargetObjective

    vals = np.arange(6) / 5.0
    space = SearchSpace.from_product([NumericalDiscreteParameter(f"x{i}", vals) for i in range(3)])
    rng = np.random.default_rng(8)  # (a seed under which every greedy step and the EI pick below clear their margin, both orientations)
    base = rng.choice(len(space.discrete.exp_rep), 8, replace=False)
    meas = space.discrete.exp_rep.iloc[np.repeat(base, 3)].reset_index(drop=True)
    x = meas.to_numpy()
    meas["y"] = np.sin(4 * x[:, 0]) + (x[:, 1] - 0.3) ** 2 - 0.5 * x[:, 2] + 0.3 * rng.standard_normal(len(x))
    return space, SingleTargetObjective(NumericalTarget("y", minimize=minimize)), meas


@pytest.mark.parametrize("minimize", [False, True])
def test_recommend_end_to_end_returns_the_oracles_labels(minimize):
    pytest.importorskip("sklearn")
    import torch
    from sklearn.ensemble import RandomForestRegressor

    from baybe_amd.engine import draw_sampler_seed
    from baybe_amd.forest import HipRandomForestSurrogate, ensemble_member_indices, pack_forest
    from baybe_amd.recommenders import HipBotorchRecommender

    params = {"n_estimators": 7, "random_state": 3}
    space, obj, meas = _grid_context(minimize)
    sign = -1.0 if minimize else 1.0
    comp = space.discrete.comp_rep.to_numpy(dtype=np.float64)
    train_x = space.transform(meas).to_numpy(dtype=np.float64)
    model = RandomForestRegressor(**params).fit(train_x, meas["y"].to_numpy())
    packed = pack_forest(model.estimators_)
    P, Ptrain = of.traverse(packed, comp), of.traverse(packed, train_x)
    assert np.array_equal(P, np.stack([e.predict(comp) for e in model.estimators_]))
    best = of.best_f(Ptrain, sign)
    pending = space.discrete.exp_rep.iloc[[10, 100]]
    Ppend = P[:, [10, 100]]

    def oracle_batch(seed, pend, alive=None):
        idx = ensemble_member_indices(512, 7, seed)
        picks, values, margins = of.greedy("qLogEI", P, idx, best, sign, 3, pend, alive)
        assert min(margins) >= 1e-8, margins  # (a condition on this fixture)
        return picks, values

    sur = HipRandomForestSurrogate(model_params=params)
    rec = HipBotorchRecommender(surrogate_model=sur)
    # plain
    torch.manual_seed(1)
    got = rec.recommend(3, space, obj, meas)
    torch.manual_seed(1)
    picks, _ = oracle_batch(draw_sampler_seed(), None)
    assert list(got.index) == picks
    # with pending experiments
    torch.manual_seed(2)
    got = rec.recommend(3, space, obj, meas, pending_experiments=pending)
    torch.manual_seed(2)
    picks, _ = oracle_batch(draw_sampler_seed(), Ppend)
    assert list(got.index) == picks
    # acquisition_values, then recommend again (the read-back leaves nothing behind that changes a batch)
    torch.manual_seed(3)
    some = space.discrete.exp_rep.iloc[::7]
    acq = rec.acquisition_values(some, space, obj, meas)
    torch.manual_seed(3)
    idx = ensemble_member_indices(512, 7, draw_sampler_seed())
    assert np.allclose(acq.to_numpy(), of.scores("qLogEI", P[:, ::7], None, idx, best, sign), rtol=1e-9, atol=1e-10)
    torch.manual_seed(4)
    joint = rec.joint_acquisition_value(space.discrete.exp_rep.iloc[[5, 50, 150]], space, obj, meas)
    torch.manual_seed(4)
    idx = ensemble_member_indices(512, 7, draw_sampler_seed())
    assert np.isclose(joint, of.scores("qLogEI", P[:, [150]], P[:, [5, 50]], idx, best, sign)[0], rtol=1e-9, atol=1e-10)
    torch.manual_seed(1)
    again = rec.recommend(3, space, obj, meas)
    torch.manual_seed(1)
    picks, _ = oracle_batch(draw_sampler_seed(), None)
    assert list(again.index) == picks
    # read-backs: mean and std within the moment bounds; no quantile
    stats = sur.posterior_stats(some, ("mean", "std", "var"))
    mo, vo = of.moments(P[:, ::7])
    T, big = 7, np.abs(P).max()
    assert list(stats.columns) == ["y_mean", "y_std", "y_var"]
    assert np.abs(stats["y_mean"].to_numpy() - mo).max() <= 2 * T * EPS * big
    assert np.abs(stats["y_var"].to_numpy() - vo).max() <= 8 * T * EPS * big * big
    assert np.abs(stats["y_std"].to_numpy() ** 2 - vo).max() <= 16 * T * EPS * big * big
    with pytest.raises(TypeError, match="EnsemblePosterior"):
        sur.posterior_stats(some, (0.5,))
    # copies and pickles carry the packed forest and rebuild their device state on first use (backtesting drivers deep-copy campaigns)
    import copy
    import pickle

    rows = comp[::7]
    m0, v0 = (t.cpu().numpy() for t in sur.posterior_mean_var(rows))
    for twin in (copy.deepcopy(sur), pickle.loads(pickle.dumps(sur))):
        m1, v1 = (t.cpu().numpy() for t in twin.posterior_mean_var(rows))
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    with pytest.raises(ValueError, match="NaN"):
        sur.posterior_mean_var(np.full((1, 3), np.nan))
    # an analytic acquisition function reads the ensemble moments
    from oracle import gp_oracle as go

    mean_o, var_o = of.moments(P)
    ei = go.analytic_acq("EI", mean_o, var_o, best, sign)
    top = np.sort(ei)[::-1]
    assert top[0] - top[top != top[0]].max() >= 1e-8
    got = HipBotorchRecommender(surrogate_model=sur, acquisition_function="EI").recommend(1, space, obj, meas)
    assert list(got.index) == [int(np.argmax(ei))]


def test_constant_targets_recommend_the_first_rows():
    """One leaf: every acquisition value ties across all candidates, the first indices win."""
    from baybe_amd.forest import HipRandomForestSurrogate
    from baybe_amd.recommenders import HipBotorchRecommender

    space, obj, meas = _grid_context(False)
    meas = meas.copy()
    meas["y"] = 1.25
    sur = HipRandomForestSurrogate(model_params={"n_estimators": 7})
    got = HipBotorchRecommender(surrogate_model=sur).recommend(3, space, obj, meas)
    assert list(got.index) == [0, 1, 2] and sur._model is None and sur.engine.n_trees == 1
    mean, var = sur.posterior_mean_var(space.discrete.comp_rep.to_numpy(dtype=np.float64)[:5])
    assert np.array_equal(mean.cpu().numpy(), np.full(5, 1.25)) and np.array_equal(var.cpu().numpy(), np.zeros(5))


# ---- trees of the size the kernels were laid out for (MIXED: 199 ... 1399 nodes, LDS and global trees in one pass) ---------------------
@functools.lru_cache(maxsize=None)
def mixed():
    """(fixture, engine) of ``MIXED`` - loaded and uploaded once, never modified."""
    from baybe_amd.forest import HipForestEngine

    g = fc.load_mixed()
    eng = HipForestEngine(0)
    eng._X_train = g["train_x"]
    eng.set_forest(g["packed"], g["X"].shape[1])
    assert tuple(int(n) for n in np.diff(g["packed"]["offsets"])) == fc.MIXED_NODES
    return g, eng


def _listed(eng, trees):
    """The forest of an engine with another list of trees to visit."""
    import torch

    return dict(eng.forest, order=torch.tensor(list(trees), dtype=torch.int32, device=eng._dev()))


@functools.lru_cache(maxsize=None)
def mixed_draw(S):
    from baybe_amd.forest import ensemble_member_counts, ensemble_member_indices

    T = len(fc.MIXED_NODES)
    return ensemble_member_indices(S, T, fc.MIXED["sampler"]), ensemble_member_counts(S, T, fc.MIXED["sampler"])


@pytest.mark.parametrize("lds_nodes", fc.MIXED_LDS_NODES)
def test_mixed_predict_equals_scikit_learn_on_every_path_split(lds_nodes):
    """The LDS / global border directly below and at 199, 659 and 1023 nodes, all-global and the default: every neighbour pattern of
    staged and unstaged trees in this order (a global first tree, a staged tree behind a global one and the reverse, the buffer parity
    carried across trees that were never staged), every staging slot, two row tiles."""
    g, eng = mixed()
    for rows, want in ((g["X"], g["pred"]), (g["train_x"][:65], g["pred_train"][:, :65])):
        got = eng.forest_predict(eng.forest, eng._as_dev(rows), lds_nodes=lds_nodes).cpu().numpy()
        assert np.array_equal(got, want), (lds_nodes, np.argwhere(got != want)[:8])


@pytest.mark.parametrize("lds_nodes", [None, 659])
def test_mixed_each_tree_as_the_first_tree(lds_nodes):
    """A pass that lists one tree stages it through the first-tree loop (up to four trips) or walks it in global memory; the reversed
    and the rotated order put every tree behind another neighbour."""
    g, eng = mixed()
    Xd = eng._as_dev(g["X"])
    for t in range(len(fc.MIXED_NODES)):
        got = eng.forest_predict(_listed(eng, [t]), Xd, lds_nodes=lds_nodes)[t].cpu().numpy()  # (the other rows are not written)
        assert np.array_equal(got, g["pred"][t]), (lds_nodes, t)
    for name, trees in fc.mixed_orders().items():
        got = eng.forest_predict(_listed(eng, trees), Xd, lds_nodes=lds_nodes).cpu().numpy()
        assert np.array_equal(got, g["pred"]), (lds_nodes, name)


def test_mixed_moments_within_the_summation_bounds_on_every_path_split():
    g, eng = mixed()
    P = g["pred"]
    Xd = eng._as_dev(g["X"])
    T, big = P.shape[0], np.abs(P).max()
    worst = [0.0, 0.0]
    for name, trees in fc.mixed_orders().items():
        mo, vo = of.moments(P[trees])
        F = _listed(eng, trees)
        first = None
        for lds_nodes in fc.MIXED_LDS_NODES:
            mean, var = (v.cpu().numpy() for v in eng.forest_moments(F, Xd, lds_nodes=lds_nodes))
            worst = [max(worst[0], np.abs(mean - mo).max()), max(worst[1], np.abs(var - vo).max())]
            if first is None:
                first = (mean, var)
            assert np.array_equal(mean, first[0]) and np.array_equal(var, first[1]), (name, lds_nodes, "differs from the default path")
    print(f"forest moments MIXED: mean dev {worst[0]:.3e} (bound {2 * T * EPS * big:.3e}), var dev {worst[1]:.3e} "
          f"(bound {8 * T * EPS * big * big:.3e})")
    record_deviation("forest_moments_mean[mixed]", worst[0], 2 * T * EPS * big)
    record_deviation("forest_moments_var[mixed]", worst[1], 8 * T * EPS * big * big)
    assert worst[0] <= 2 * T * EPS * big
    assert worst[1] <= 8 * T * EPS * big * big
    for lds_nodes in (None, 659):
        for t in range(T):
            mean, var = (v.cpu().numpy() for v in eng.forest_moments(_listed(eng, [t]), Xd, lds_nodes=lds_nodes))
            assert np.array_equal(var, np.zeros_like(var)) and np.array_equal(mean, P[t]), (lds_nodes, t)


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("kind", fc.MC_KINDS)
def test_mixed_fused_scores_with_63_pending_points(kind, sign):
    """k = 0 and the two k = 63 blocks (the last slot of the pending block in use), S = 5 (fewer samples than trees: some are skipped)
    and 512, against the per-sample oracle; the same bits on every path split; the oracle's winner masked."""
    import torch

    g, eng = mixed()
    P, X = g["pred"], g["X"]
    Xd = eng._as_dev(X)
    dev = eng._dev()
    best = of.best_f(g["pred_train"], sign)
    worst = 0.0
    for S in fc.MIXED_SAMPLES:
        idx, counts = mixed_draw(S)
        counts_d = torch.from_numpy(counts).to(dev)
        order = torch.from_numpy(np.nonzero(counts)[0].astype(np.int32)).to(dev)
        for block in (None, "a", "b"):
            pend = None if block is None else np.ascontiguousarray(P[:, fc.mixed_pending_rows(P, sign, block)])
            pend_d = None if pend is None else torch.from_numpy(pend).to(dev)
            assert (0 if pend is None else pend.shape[1]) in fc.MIXED_PENDING
            want = of.scores(kind, P, pend, idx, best, sign)
            first = None
            for lds_nodes in fc.MIXED_LDS_NODES:
                got = eng.forest_mc_acq(eng.forest, kind, Xd, counts_d, order, S, pend_d, best, sign, lds_nodes=lds_nodes).cpu().numpy()
                if first is None:
                    first = got
                    assert np.allclose(got, want, rtol=1e-9, atol=1e-10), (kind, sign, S, block, np.abs(got - want).max())
                    worst = max(worst, float((np.abs(got - want) / (1e-10 + 1e-9 * np.abs(want))).max()))
                assert np.array_equal(got, first), (kind, sign, S, block, lds_nodes, "differs from the default path")
            alive = np.ones(len(X), dtype=np.uint8)
            alive[int(np.argmax(want))] = 0
            m = eng.forest_mc_acq(eng.forest, kind, Xd, counts_d, order, S, pend_d, best, sign,
                                  alive=torch.from_numpy(alive).to(dev)).cpu().numpy()
            live = alive.astype(bool)
            assert np.all(np.isneginf(m[~live])) and np.array_equal(m[live], first[live])
            if S == 512 and block == "b":  # a pass that starts at the 1399-node tree: other summation order, same allowance
                rot = torch.tensor(fc.mixed_orders()["rotated"], dtype=torch.int32, device=dev)
                got = eng.forest_mc_acq(eng.forest, kind, Xd, counts_d, rot, S, pend_d, best, sign).cpu().numpy()
                assert np.allclose(got, want, rtol=1e-9, atol=1e-10), (kind, sign, "rotated", np.abs(got - want).max())
                worst = max(worst, float((np.abs(got - want) / (1e-10 + 1e-9 * np.abs(want))).max()))
    print(f"forest fused scores MIXED {kind} sign {sign:+.0f}: worst deviation = {worst:.3e} of the allowance")
    record_deviation(f"forest_fused_scores_share_of_allowance[mixed-{kind}-{'max' if sign > 0 else 'min'}]", worst, 1.0)


def test_64_pending_points_are_refused():
    """One more than the pending slot holds: refused on the host, nothing is launched."""
    import torch

    from baybe_amd.engine import HipError

    g, eng = mixed()
    _, counts = mixed_draw(512)
    dev = eng._dev()
    pend = torch.zeros((len(fc.MIXED_NODES), 64), dtype=torch.float64, device=dev)
    with pytest.raises(HipError, match="63"):
        eng.forest_mc_acq(eng.forest, "qLogEI", eng._as_dev(g["X"]), torch.from_numpy(counts).to(dev), eng.forest["order"], 512, pend)


def test_mixed_strided_rows_give_the_bits_of_contiguous_rows():
    """Rows inside a wider matrix (row stride 7, every other row off the 16-byte grid) and with columns behind the d the forest reads:
    the surroundings hold 1e30, so a column or row taken from them changes a walk."""
    import torch

    g, eng = mixed()
    P, X = g["pred"], g["X"]
    dev = eng._dev()
    Xd = eng._as_dev(X)
    idx, counts = mixed_draw(512)
    counts_d = torch.from_numpy(counts).to(dev)
    pend_d = torch.from_numpy(np.ascontiguousarray(P[:, fc.mixed_pending_rows(P, 1.0, "a")])).to(dev)
    best = of.best_f(g["pred_train"], 1.0)

    def results(rows):
        mean, var = eng.forest_moments(eng.forest, rows)
        return (eng.forest_predict(eng.forest, rows), mean, var,
                eng.forest_mc_acq(eng.forest, "qLogEI", rows, counts_d, eng.forest["order"], 512, pend_d, best, 1.0))

    ref = results(Xd)
    assert np.array_equal(ref[0].cpu().numpy(), P)
    W = torch.full((260, 7), 1e30, dtype=torch.float64, device=dev)
    W[3:, 1:5] = Xd
    W2 = torch.full((260, 7), 1e30, dtype=torch.float64, device=dev)  # the same rows, the first element off the 16-byte grid too
    W2[2:259, 1:5] = Xd
    assert W2[2:259, 1:5].data_ptr() % 16 == 8
    for view in (W[3:, 1:5], W[3:, 1:], W2[2:259, 1:5], W2[2:259, 1:]):
        assert view.stride(0) == 7 and view.shape[1] in (4, 6) and not view.is_contiguous()
        for got, want in zip(results(view), ref):
            assert torch.equal(got, want)
    for view in (W[3:4, 1:5], W2[2:3, 1:5]):
        assert view.shape == (1, 4)
        p, mean, var, score = results(view)
        assert torch.equal(p, ref[0][:, :1]) and torch.equal(mean, ref[1][:1]) and torch.equal(var, ref[2][:1])
        assert torch.equal(score, ref[3][:1])


def test_mixed_greedy_batches_return_the_oracles_indices():
    """Nothing is skipped: every step clears 1e-8 in the oracle
    (tests/test_forest_cpu.py::test_every_greedy_step_of_the_mixed_forest_clears_the_margin)."""
    from baybe_amd.forest import HipForestAcq

    from baybe_amd.forest import ensemble_member_indices

    g, eng = mixed()
    c = dict(fc.MIXED, **fc.MIXED["greedy"])
    P, X = g["pred"], g["X"]
    Xd = eng._as_dev(X)
    idx = ensemble_member_indices(c["S"], P.shape[0], c["sampler"])
    best = of.best_f(g["pred_train"], c["sign"])
    for kind in fc.MIXED_GREEDY_KINDS:
        acq = HipForestAcq(_Holder(eng), kind, c["sign"], best, c["S"])
        for k in (0, 1):
            rows = fc.pending_rows(c["N"], k)
            for batch in fc.MIXED_BATCHES:
                want, values, _ = of.greedy(kind, P, idx, best, c["sign"], batch, P[:, rows] if k else None)
                res = acq.greedy(Xd, batch, seed=c["sampler"], X_pending=X[rows] if k else None)
                assert res.indices == want, (kind, k, batch, res.indices, want)
                assert np.allclose(res.values, values, rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("lds_nodes", [None, 0])
def test_a_node_pointing_outside_its_tree_becomes_a_nan_leaf(lds_nodes):
    """The device guard (``check_packed`` refuses such tables on the host; ``forest_upload`` does not look): an inner node of the
    659-node tree, in the third staging slot, gets a child equal to the tree's node count - the next tree's first node in global
    memory, an unstaged entry of the LDS table - and, separately, the feature d = 4 - the padding column of the LDS row.  Neither
    leaves an allocation.  Rows whose walk reaches the node get NaN from that tree; everything else keeps scikit-learn's bits."""
    g, eng = mixed()
    packed, d, t = g["packed"], g["X"].shape[1], 4
    off = packed["offsets"]
    first, nn = int(off[t]), int(off[t + 1] - off[t])
    assert nn == 659 and t + 1 < len(fc.MIXED_NODES)
    rows = np.concatenate([g["X"], g["train_x"]])
    recorded = np.concatenate([g["pred"], g["pred_train"]], axis=1)
    tree = {k: packed[k][first:first + nn] for k in fc.PACKED_KEYS if k != "offsets"}
    tree["offsets"] = np.array([0, nn], dtype=np.int64)

    def reached(node):  # the oracle's walk on the unaltered tree, cut at the node
        cut = {k: v.copy() for k, v in tree.items()}
        cut["children_left"][node] = cut["children_right"][node] = -1
        cut["value"][node] = np.nan
        return np.isnan(of.traverse(cut, rows)[0])

    inner = [n for n in range(512, nn) if tree["children_left"][n] >= 0]
    hit = {n: reached(n) for n in inner}
    node = max(inner, key=lambda n: int(hit[n].sum()))
    assert 2 <= hit[node].sum() < len(rows)
    want = recorded.copy()
    want[t, hit[node]] = np.nan
    Xd = eng._as_dev(rows)
    for key, value in (("children_left", nn), ("children_right", nn), ("feature", d)):
        bad = {k: v.copy() for k, v in packed.items()}
        bad[key][first + node] = value
        got = eng.forest_predict(eng.forest_upload(bad, d), Xd, lds_nodes=lds_nodes).cpu().numpy()
        assert np.array_equal(got, want, equal_nan=True), (key, lds_nodes)
