"""qNEI / qLogNEI on the device against the restatement on the frozen oracle (``tests/_nei_reference.py``): scores of q = 1
t-batches, baseline pruning, greedy batches with a pending row, the fused scoring pass against the unfused form, its memory
footprint, and the plug-in surface."""

import numpy as np
import pytest

import _nei_reference as ref
from _problems import make_grid

pytestmark = pytest.mark.gpu
NEI_ATOL = 1e-8  # qLogNEI scores, absolute (NEHVI_ATOL: the project's tolerance for qLogEI-type scores)
CASES = {"A": (24, 150, 3, 0, +1.0), "B": (20, 120, 3, 3, -1.0), "C": (40, 200, 5, 7, +1.0)}  # n, N, d, seed, sign


@pytest.fixture(scope="module")
def cases():
    """The ``make_grid`` problems of tests/test_nehvi_gpu.py::_setup with the target -|x - 0.25|^2 + 0.05 N(0, 1): the device's
    fitted engine and the oracle model carrying the device fit's hyper-parameters.  Built once per case."""
    from baybe_amd import engine, gp_spec
    from oracle import gp_oracle as go

    built = {}

    def get(name):
        if name not in built:
            n, N, d, seed, sign = CASES[name]
            rng = np.random.default_rng(seed)
            X = make_grid(N, d, seed)
            Xt = make_grid(4 * n, d, seed + 1)[:n]
            y = -((Xt - 0.25) ** 2).sum(1) + 0.05 * rng.standard_normal(n)
            g = engine.HipGP(0)
            g.set_model(gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d)), Xt, y)
            fi = g.fit()
            model = go.fit_gp(go.GPSpec.baybe_default(d, np.zeros(d), np.ones(d)), Xt, y,
                              params=go.GPParams(fi.params.lengthscale, fi.params.noise, fi.params.mean))
            built[name] = (X, Xt, sign, g, model)
        return built[name]

    yield get
    for _, _, _, g, _ in built.values():
        g.close()


@pytest.mark.parametrize("name", list(CASES))
def test_scores_match_the_restatement(cases, name):
    """S = 32, sampler seed 11, no pruning, the first 60 candidates.  Candidates that coincide with a baseline row have a
    conditional variance that is rounding noise around zero, and whether the 1e-8 jitter applies depends on its sign (see
    tests/test_nehvi_gpu.py::test_scores_match_oracle): they are excluded and held to "no improvement" - at most 3 of 60."""
    import torch

    from baybe_amd.nei import HipNEI
    from conftest import record_deviation

    X, Xt, sign, g, model = cases(name)
    S, seed = 32, 11
    z = ref.base_samples(S, len(Xt), seed)
    dup = np.array([(np.abs(Xt - x).sum(1) < 1e-12).any() for x in X[:60]])
    assert dup.sum() <= 3
    Xd = torch.from_numpy(X).cuda()
    for log in (True, False):
        hv = HipNEI(g, sign, Xt, n_mc_samples=S, prune_baseline=False, log=log)
        hv.prepare(seed)
        sg = hv.score(Xd).cpu().numpy()[:60]
        assert hv.last_form == "fused"
        so = ref.scores(model, sign, Xt, z, X[:60], log=log)[0]
        dev = np.abs(sg - so)[~dup]
        print(f"case {name} {'qLogNEI' if log else 'qNEI'}: max |device - restatement| = {dev.max():.3e} over {len(dev)} rows, "
              f"reference gap of the best two = {np.diff(np.sort(so[~dup])[-2:])[0]:.3f}")
        if log:
            record_deviation(f"qlognei_scores_small[{name}]", dev.max(), NEI_ATOL)
            assert np.allclose(sg[~dup], so[~dup], rtol=0, atol=NEI_ATOL), dev.max()
            assert (sg[dup] < so[~dup].max() - 5).all() and (so[dup] < so[~dup].max() - 5).all()
        else:
            record_deviation(f"qnei_scores_small_rel[{name}]", float((dev / np.maximum(np.abs(so[~dup]), 1e-300)).max()), 1e-9)
            assert np.allclose(sg[~dup], so[~dup], rtol=1e-9, atol=1e-12), dev.max()
            # a copy of a baseline point is that point's sampled value + sd z_x with sd <= 1e-4 (jitter 1e-8): its improvement
            # over the sample's best is at most 1e-4 E[max(z, 0)] = 4e-5
            assert (sg[dup] < 1e-4).all() and (so[dup] < 1e-4).all()
        assert int(np.argmax(sg)) == int(np.argmax(so))


@pytest.mark.parametrize("name", list(CASES))
def test_pruning_matches_the_restatement(cases, name):
    """Prune seed 9: the kept rows are the per-sample maxima of 2048 joint draws, in their original order.  The smallest gap
    between a sample's best and second-best value must lie far above the samples' agreement (1e-9), or the kept set could flip
    on rounding."""
    from baybe_amd.nei import HipNEI

    X, Xt, sign, g, model = cases(name)
    keep, gap = ref.prune(model, sign, Xt, 9)
    print(f"case {name}: reference keeps {len(keep)} of {len(Xt)} points, smallest best / second-best gap {gap:.2e}")
    assert gap > 1e-7
    hv = HipNEI(g, sign, Xt, n_mc_samples=32, prune_baseline=True)
    hv.prepare(11, prune_seed=9)
    assert np.array_equal(hv._pruned, Xt[keep])
    assert np.array_equal(hv.X_b_current, Xt[keep])


@pytest.mark.parametrize("name", list(CASES))
def test_greedy_with_a_pending_row_matches_the_restatement(cases, name):
    """q = 3, S = 32, sampler seed 5, prune seed 9, candidate row 100 pending.  ``make_grid`` repeats rows (150 draws from a grid
    of 11^3 points), and the copies of a row tie exactly in the restatement - in case A the third step's best two are such a pair.
    The indices then agree because both sides break ties the same way: ``np.argmax`` and the device argmax (``bbh_argmax``:
    score descending, index ascending) take the first index, and the device scores identical rows bit-identically - every
    candidate's contraction and sample reduction run in the same order wherever its row sits in a tile.  The last assertion pins
    that premise on the final step's scores."""
    import torch

    from baybe_amd.nei import HipNEI
    from conftest import record_deviation

    X, Xt, sign, g, model = cases(name)
    S, seed, pseed = 32, 5, 9
    pending = X[100:101]
    Xd = torch.from_numpy(X).cuda()
    hv = HipNEI(g, sign, Xt, n_mc_samples=S, prune_baseline=True)
    res = hv.greedy(Xd, 3, seed=seed, prune_seed=pseed, X_pending=pending)
    keep, _ = ref.prune(model, sign, Xt, pseed)
    picks, vals = ref.greedy(model, sign, Xt[keep], X, 3, S, seed, X_pending=pending)
    dev = np.abs(np.array(res.values) - np.array(vals)).max()
    print(f"case {name}: greedy picks {res.indices} (restatement {picks}), max value deviation {dev:.3e}")
    record_deviation(f"qlognei_greedy_values[{name}]", dev, NEI_ATOL)
    assert res.indices == picks
    assert np.allclose(res.values, vals, rtol=0, atol=NEI_ATOL)
    assert len(hv.X_b_current) == len(keep) + 1 + 2  # the pending row and the first two picks joined the baseline
    sc = hv.score(Xd).cpu().numpy()  # the third step's scores (no row masked)
    _, first, inverse = np.unique(X, axis=0, return_index=True, return_inverse=True)
    assert np.array_equal(sc, sc[first[np.ravel(inverse)]])  # every copy of a row scores exactly what its first copy scores


def test_multi_task_surrogate_matches_the_restatement():
    """An ICM model (3 tasks, candidates on task 0, baseline rows on all tasks): the extended model carries the task column - scores,
    pruning and a greedy batch with a pending row against the restatement, as for the single-task cases."""
    import torch
    from _problems import make_tl_problem, oracle_params, oracle_spec

    from baybe_amd import engine, gp_spec
    from baybe_amd.nei import HipNEI
    from conftest import record_deviation
    from oracle import gp_oracle as go

    d, T = 3, 3
    X, Xt, y = make_tl_problem(300, d, 10, T=T, seed=4)
    spec = gp_spec.GPSpec.baybe_default(d + 1, np.zeros(d + 1), np.ones(d + 1), task_idx=d, n_tasks=T)
    g = engine.HipGP(0)
    g.set_model(spec, Xt, y)
    fi = g.fit()
    model = go.GPModel(oracle_spec(spec), oracle_params(spec, fi.params), Xt, y)
    Xd = torch.from_numpy(X).cuda()
    S, seed = 32, 11
    z = ref.base_samples(S, len(Xt), seed)
    dup = np.array([(np.abs(Xt - x).sum(1) < 1e-12).any() for x in X[:60]])
    assert dup.sum() <= 3
    hv = HipNEI(g, 1.0, Xt, n_mc_samples=S, prune_baseline=False)
    hv.prepare(seed)
    sg = hv.score(Xd).cpu().numpy()[:60]
    so = ref.scores(model, 1.0, Xt, z, X[:60])[0]
    dev = np.abs(sg - so)[~dup].max()
    print(f"multi-task qLogNEI: max |device - restatement| = {dev:.3e}")
    record_deviation("qlognei_scores_multitask", dev, NEI_ATOL)
    assert hv.last_form == "fused"
    assert np.allclose(sg[~dup], so[~dup], rtol=0, atol=NEI_ATOL) and int(np.argmax(sg)) == int(np.argmax(so))
    keep, gap = ref.prune(model, 1.0, Xt, 9)
    assert gap > 1e-7
    hv = HipNEI(g, 1.0, Xt, n_mc_samples=S, prune_baseline=True)
    res = hv.greedy(Xd, 3, seed=5, prune_seed=9, X_pending=X[100:101])
    picks, vals = ref.greedy(model, 1.0, Xt[keep], X, 3, S, 5, X_pending=X[100:101])
    assert np.array_equal(hv._pruned, Xt[keep])
    assert res.indices == picks and np.allclose(res.values, vals, rtol=0, atol=NEI_ATOL)
    g.close()


def _big_model(composite=False):
    from baybe_amd import engine, gp_spec

    rng = np.random.default_rng(42)
    d, n = 20, 128
    Xt = rng.random((n, d))
    y = -((Xt - 0.25) ** 2).sum(1) + 0.05 * rng.standard_normal(n)
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    if composite:
        from baybe_amd.kernels import GammaPrior, MaternKernel, ProductKernel, RBFKernel, ScaleKernel, apply_kernel_spec

        apply_kernel_spec(spec, ProductKernel([MaternKernel(2.5, GammaPrior(3, 1)), ScaleKernel(RBFKernel(), GammaPrior(2, 0.5))]))
        params = gp_spec.initial_params(spec)
        params.noise = 0.02
    else:
        params = gp_spec.GPParams(np.full(d, 1.2), 0.02, 0.0)
    g = engine.HipGP(0)
    g.set_model(spec, Xt, y)
    g.factorize(params)
    return g, Xt


@pytest.mark.parametrize("S", [100, 512])
def test_fused_pass_equals_the_unfused_form(monkeypatch, S):
    """N = 20 000, d = 20, n = 128, the same fitted model under BBH_NEI_FUSED = 1 and 0 (a handle reads the switch when it is
    created).  Both forms evaluate the same per-sample terms; only the order of the S-term sums differs: S eps 50 ~ 3e-12."""
    import torch

    from baybe_amd.nei import HipNEI
    from conftest import record_deviation

    g, Xt = _big_model()
    Xd = torch.from_numpy(np.random.default_rng(1).random((20000, 20))).cuda()
    alive = torch.ones(20000, dtype=torch.uint8, device="cuda")
    alive[[3, 19999]] = 0
    out = {}
    for log in (True, False):
        for fused in ("1", "0"):
            monkeypatch.setenv("BBH_NEI_FUSED", fused)
            hv = HipNEI(g, 1.0, Xt, n_mc_samples=S, prune_baseline=False, log=log)
            hv.prepare(7)
            out[fused] = hv.score(Xd, alive).cpu().numpy()
            assert hv.last_form == ("fused" if fused == "1" else "unfused")
            assert hv._lib.bbh_last_nei_form(hv.outputs[0].ext._h) == (1 if fused == "1" else 2)
            for o in hv.outputs:
                o.ext.close()
        live = np.isfinite(out["1"])
        assert (~live).sum() == 2 and not live[3] and not live[19999] and np.array_equal(live, np.isfinite(out["0"]))
        dev = np.abs(out["1"][live] - out["0"][live]).max()
        print(f"S = {S} {'qLogNEI' if log else 'qNEI'}: max |fused - unfused| = {dev:.3e}, scores in [{out['1'][live].min():.3f}, {out['1'][live].max():.3f}]")
        record_deviation(f"nei_fused_vs_unfused[S={S},{'log' if log else 'plain'}]", dev, 1e-11)
        assert dev <= 1e-11
    g.close()


def test_composite_kernel_model_takes_the_unfused_form():
    import torch

    from baybe_amd.nei import HipNEI

    g, Xt = _big_model(composite=True)
    hv = HipNEI(g, 1.0, Xt[:40], n_mc_samples=64, prune_baseline=False)
    hv.prepare(7)
    sc = hv.score(torch.from_numpy(np.random.default_rng(2).random((3000, 20))).cuda()).cpu().numpy()
    assert hv._lib.bbh_last_nei_form(hv.outputs[0].ext._h) == 2 and hv.last_form == "unfused"
    assert np.isfinite(sc).all()
    g.close()


def test_fused_pass_allocates_no_sample_matrix():
    """N = 200 000, S = 512: across one fused ``score`` the peak of torch's allocator rises by the variance pass's two vectors and
    the scores (24 N bytes; bound 32 N + 16 MB) - the [S, N] matrix of conditional means would be 819 MB.  (The library itself
    takes no workspace in ``bbh_score_nei``.)"""
    import torch

    from baybe_amd.nei import HipNEI

    g, Xt = _big_model()
    N = 200_000
    Xd = torch.from_numpy(np.random.default_rng(3).random((N, 20))).cuda()
    hv = HipNEI(g, 1.0, Xt, n_mc_samples=512, prune_baseline=True)
    hv.prepare(7, prune_seed=8)
    hv.score(Xd[:4096])  # (first use: handle workspaces, kernel-value cache)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    sc = hv.score(Xd)
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise across one fused score at N = {N}, S = 512: {rise / 2**20:.1f} MB (bound {(32 * N + (16 << 20)) / 2**20:.1f} MB)")
    assert hv.last_form == "fused" and bool(torch.isfinite(sc).all())
    assert rise <= 32 * N + (16 << 20)
    g.close()


def test_recommend_through_the_plugin_surface():
    """``recommend()`` with ``"qLogNEI"`` on a 1000-row space: the restatement's greedy batch for the hyper-parameters the device
    fitted (scoring seed drawn first, then the pruning seed); an RFF surrogate is refused."""
    import torch
    from _baybe_shim import NumericalDiscreteParameter, NumericalTarget, SearchSpace, SingleTargetObjective
    from _problems import oracle_params, oracle_spec
    from baybe_amd.engine import draw_sampler_seed
    from baybe_amd.exceptions import IncompatibilityError
    from baybe_amd.kernels import GammaPrior, RFFKernel, ScaleKernel
    from baybe_amd.recommenders import HipBotorchRecommender
    from baybe_amd.surrogates import HipGaussianProcessSurrogate
    from oracle import gp_oracle as go

    rng = np.random.default_rng(5)
    vals = np.arange(10) / 9.0
    space = SearchSpace.from_product([NumericalDiscreteParameter(f"x{i}", vals) for i in range(3)])
    exp = space.discrete.exp_rep
    assert len(exp) == 1000
    meas = exp.iloc[rng.choice(len(exp), 20, replace=False)].copy()
    Xm = meas[["x0", "x1", "x2"]].to_numpy(float)
    meas["y"] = -((Xm - 0.25) ** 2).sum(1) + 0.05 * rng.standard_normal(len(Xm))
    obj = SingleTargetObjective(NumericalTarget("y"))
    rec = HipBotorchRecommender(acquisition_function="qLogNEI")
    torch.manual_seed(31)
    got = rec.recommend(2, space, obj, meas)
    assert type(rec._scorer).__name__ == "HipNEI" and rec._scorer.last_form == "fused"
    eng = rec._surrogate_model.engine
    model = go.GPModel(oracle_spec(eng.spec), oracle_params(eng.spec, eng.params), eng._X_train, eng._y_train)
    torch.manual_seed(31)
    seed, pseed = draw_sampler_seed(), draw_sampler_seed()
    Xb = space.transform(meas, allow_extra=True).to_numpy(dtype=np.float64)
    keep, gap = ref.prune(model, 1.0, Xb, pseed)
    assert gap > 1e-7
    comp = space.discrete.comp_rep.to_numpy(dtype=np.float64)
    picks, _ = ref.greedy(model, 1.0, Xb[keep], comp, 2, 512, seed)
    assert list(got.index) == list(exp.index[picks]), (list(got.index), picks)
    acq = rec.acquisition_values(exp.iloc[:50], space, obj, meas)
    assert np.isfinite(acq.to_numpy()).all()
    rff = HipBotorchRecommender(acquisition_function="qLogNEI", surrogate_model=HipGaussianProcessSurrogate(
        kernel_or_factory=ScaleKernel(RFFKernel(16, GammaPrior(3, 2)), GammaPrior(2, 0.5))))
    with pytest.raises(IncompatibilityError):
        rff.recommend(1, space, obj, meas)
