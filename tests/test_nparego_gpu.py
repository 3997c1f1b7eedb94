"""qLogNParEGO on the device against the restatement on the frozen oracle (``tests/_nparego_reference.py``): scores of q = 1 t-batches
(with a ragged last sample slice), the chunked pass and its memory footprint, the ``alive`` mask, baseline pruning, greedy batches with
a pending row, baseline edge cases, and the plug-in surface.  Problems: ``tests/_pareto_cases.py`` (n = 24, N = 150, d = 3)."""

import numpy as np
import pytest

import _nparego_reference as ref
from _pareto_cases import coincides_with_baseline, setup

pytestmark = pytest.mark.gpu
ATOL = 1e-8  # qLogNParEGO scores, absolute (NEI_ATOL: the project's tolerance for qLogEI-type scores)
# m, signs, weights, prune seed
CASES = {"i": (2, (1.0, 1.0), (0.3, 0.7), 9), "ii": (3, (1.0, 1.0, 1.0), (1 / 3, 1 / 3, 1 / 3), 3), "iii": (2, (1.0, -1.0), (0.5, 0.5), 9)}


def _case(name):
    m, signs, w, pseed = CASES[name]
    X, Xt, _, signs, engines, models = setup(m, signs)
    w = np.array(w) / np.sum(w)
    lo, hi = ref.bounds(models, signs, Xt)
    return X, Xt, signs, engines, models, w, lo, hi, pseed


@pytest.mark.parametrize("S", [32, 33])
@pytest.mark.parametrize("name", list(CASES))
def test_scores_match_the_restatement(name, S):
    """Sampler seed 11, no pruning, the first 60 candidates; S = 33 leaves the last sample slice (16 samples each) with one sample.
    Candidates that coincide with a baseline row (3 of 60) are excluded and held to "no improvement"."""
    import torch

    from baybe_amd.nparego import HipNParEGO
    from conftest import record_deviation

    X, Xt, signs, engines, models, w, lo, hi, _ = _case(name)
    seed = 11
    dup = coincides_with_baseline(X[:60], Xt)
    assert dup.sum() <= 3
    so = ref.scores(models, signs, Xt, ref.base_samples(S, len(Xt), len(models), seed), X[:60], w, lo, hi)[0]
    gap = np.diff(np.sort(so[~dup])[-2:])[0]
    assert gap > 1e-3, gap
    hv = HipNParEGO(engines, signs, Xt, w, n_mc_samples=S, prune_baseline=False)
    hv.prepare(seed)
    sg = hv.score(torch.from_numpy(X).cuda()).cpu().numpy()[:60]
    dev = np.abs(sg - so)[~dup]
    print(f"case {name} S = {S}: max |device - restatement| = {dev.max():.3e} over {len(dev)} rows, reference gap of the best two = {gap:.3f}")
    record_deviation(f"qlognparego_scores_small[{name},S={S}]", dev.max(), ATOL)
    assert np.allclose(sg[~dup], so[~dup], rtol=0, atol=ATOL), dev.max()
    assert (sg[dup] < so[~dup].max() - 5).all() and (so[dup] < so[~dup].max() - 5).all()
    assert int(np.argmax(sg)) == int(np.argmax(so))


def test_unit_weight_scores_the_first_target_alone():
    """w = (1, 0): t_1 = 0 takes part in the maximum, so g is piecewise linear in the first target (tests/test_nparego_cpu.py pins the
    restatement's form against the qNEI restatement); the device is held to the restatement as for any other weights."""
    import torch

    from baybe_amd.nparego import HipNParEGO
    from conftest import record_deviation

    X, Xt, signs, engines, models, _, lo, hi, _ = _case("i")
    w, S, seed = np.array([1.0, 0.0]), 32, 11
    dup = coincides_with_baseline(X[:60], Xt)
    so = ref.scores(models, signs, Xt, ref.base_samples(S, len(Xt), 2, seed), X[:60], w, lo, hi)[0]
    hv = HipNParEGO(engines, signs, Xt, w, n_mc_samples=S, prune_baseline=False)
    hv.prepare(seed)
    sg = hv.score(torch.from_numpy(X).cuda()).cpu().numpy()[:60]
    dev = np.abs(sg - so)[~dup].max()
    print(f"w = (1, 0): max |device - restatement| = {dev:.3e}")
    record_deviation("qlognparego_scores_unit_weight", dev, ATOL)
    assert dev <= ATOL and int(np.argmax(np.where(dup, -np.inf, sg))) == int(np.argmax(np.where(dup, -np.inf, so)))


class _CountingLib:
    """The library with the row count of every ``bbh_nparego_q1`` launch recorded."""

    def __init__(self, lib):
        self._lib, self.rows = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "bbh_nparego_q1":
            return fn

        def counted(h, m, n, *rest):
            self.rows.append(n)
            return fn(h, m, n, *rest)

        return counted


def test_chunked_pass_equals_the_one_chunk_pass(monkeypatch):
    """Case ii (three targets), S = 33: 150 rows in chunks of 40 (40, 40, 40, 30) against one chunk - bit for bit, also under a mask."""
    import torch

    from baybe_amd import nparego
    from baybe_amd.nparego import HipNParEGO

    X, Xt, signs, engines, models, w, lo, hi, _ = _case("ii")
    S, m = 33, len(engines)
    Xd = torch.from_numpy(X).cuda()
    alive = torch.ones(len(X), dtype=torch.uint8, device="cuda")
    alive[[0, 39, 40, 149]] = 0
    hv = HipNParEGO(engines, signs, Xt, w, n_mc_samples=S, prune_baseline=False)
    hv.prepare(11)
    whole, whole_masked = hv.score(Xd).cpu().numpy(), hv.score(Xd, alive).cpu().numpy()
    monkeypatch.setattr(nparego, "CHUNK_BYTES", 8 * S * m * 40)
    hv._lib = _CountingLib(hv._lib)
    parts, parts_masked = hv.score(Xd).cpu().numpy(), hv.score(Xd, alive).cpu().numpy()
    assert hv._lib.rows == [40, 40, 40, 30] * 2
    assert np.array_equal(parts, whole) and np.array_equal(parts_masked, whole_masked)
    assert np.isfinite(whole).all()


def test_masked_rows_score_minus_infinity_and_never_win():
    import torch

    from baybe_amd.nparego import HipNParEGO

    X, Xt, signs, engines, models, w, lo, hi, _ = _case("i")
    Xd = torch.from_numpy(X).cuda()
    hv = HipNParEGO(engines, signs, Xt, w, n_mc_samples=32, prune_baseline=False)
    hv.prepare(11)
    free = hv.score(Xd).cpu().numpy()
    top = int(np.argmax(free))
    alive = torch.ones(len(X), dtype=torch.uint8, device="cuda")
    gone = sorted({top, 0, 149})
    alive[gone] = 0
    masked = hv.score(Xd, alive).cpu().numpy()
    live = np.ones(len(X), bool)
    live[gone] = False
    assert np.isneginf(masked[gone]).all() and np.array_equal(masked[live], free[live])
    val, idx = hv.outputs[0].ext.argmax(torch.from_numpy(masked).cuda())
    assert idx not in gone and val == masked[live].max()


@pytest.mark.parametrize("name", list(CASES))
def test_pruning_matches_the_restatement(name):
    """The kept rows are the first-index argmax of g in at least one of 2048 joint draws, in their original order.  The smallest gap
    between a sample's best and second-best scalarised value must lie far above the samples' agreement (1e-9), or the kept set could
    flip on rounding."""
    from baybe_amd.nparego import HipNParEGO

    X, Xt, signs, engines, models, w, lo, hi, pseed = _case(name)
    keep, gap = ref.prune(models, signs, Xt, pseed, w, lo, hi)
    print(f"case {name}: reference keeps {len(keep)} of {len(Xt)} points, smallest best / second-best gap {gap:.2e}")
    assert gap > 1e-7
    hv = HipNParEGO(engines, signs, Xt, w, n_mc_samples=32, prune_baseline=True)
    hv.prepare(11, prune_seed=pseed)
    assert np.array_equal(hv._pruned, Xt[keep])
    assert np.array_equal(hv.X_b_current, Xt[keep])


@pytest.mark.parametrize("name", list(CASES))
def test_greedy_with_a_pending_row_matches_the_restatement(name):
    """q = 3, S = 32, sampler seed 5, candidate row 100 pending.  ``make_grid`` repeats rows, and the copies of a row tie exactly in the
    restatement; the indices agree because both sides take the first index and the device scores identical rows bit-identically
    (fixed-length sample slices summed in a fixed order, no atomics) - the last assertion pins that premise."""
    import torch

    from baybe_amd.nparego import HipNParEGO
    from conftest import record_deviation

    X, Xt, signs, engines, models, w, lo, hi, pseed = _case(name)
    S, seed = 32, 5
    pending = X[100:101]
    Xd = torch.from_numpy(X).cuda()
    hv = HipNParEGO(engines, signs, Xt, w, n_mc_samples=S, prune_baseline=True)
    res = hv.greedy(Xd, 3, seed=seed, prune_seed=pseed, X_pending=pending)
    keep, gap = ref.prune(models, signs, Xt, pseed, w, lo, hi)
    assert gap > 1e-7
    picks, vals = ref.greedy(models, signs, Xt[keep], X, 3, S, seed, w, lo, hi, X_pending=pending)
    dev = np.abs(np.array(res.values) - np.array(vals)).max()
    print(f"case {name}: greedy picks {res.indices} (restatement {picks}), max value deviation {dev:.3e}")
    record_deviation(f"qlognparego_greedy_values[{name}]", dev, ATOL)
    assert res.indices == picks
    assert np.allclose(res.values, vals, rtol=0, atol=ATOL)
    assert len(hv.X_b_current) == len(keep) + 1 + 2  # the pending row and the first two picks joined the baseline
    sc = hv.score(Xd).cpu().numpy()  # the third step's scores (no row masked)
    _, first, inverse = np.unique(X, axis=0, return_index=True, return_inverse=True)
    assert np.array_equal(sc, sc[first[np.ravel(inverse)]])  # every copy of a row scores exactly what its first copy scores


def test_baseline_with_a_repeated_row_and_a_one_row_baseline():
    """A repeated baseline row carries one latent value (BoTorch's joint draw gives the copies the same sample up to sqrt(jitter)): it
    enters the extended models once, its copy keeps its base-sample columns - the restatement on the unique rows with the copy's columns
    taken out of the draw.  One baseline row: hi = lo + 1."""
    import torch

    from baybe_amd.nparego import HipNParEGO
    from conftest import record_deviation

    X, Xt, signs, engines, models, w, lo, hi, _ = _case("i")
    S, seed, m = 32, 11, 2
    Xd = torch.from_numpy(X).cuda()
    dup = coincides_with_baseline(X[:60], Xt)
    Xb = np.vstack([Xt, Xt[3:4]])
    z = ref.base_samples(S, len(Xb), m, seed)  # [S, 26, m]: 24 rows, the copy, the candidate
    so = ref.scores(models, signs, Xt, np.ascontiguousarray(z[:, list(range(24)) + [25], :]), X[:60], w, *ref.bounds(models, signs, Xb))[0]
    hv = HipNParEGO(engines, signs, Xb, w, n_mc_samples=S, prune_baseline=False)
    hv.prepare(seed)
    sg = hv.score(Xd).cpu().numpy()[:60]
    dev = np.abs(sg - so)[~dup].max()
    record_deviation("qlognparego_scores_repeated_baseline_row", dev, ATOL)
    assert dev <= ATOL and int(np.argmax(sg)) == int(np.argmax(so)) and len(hv.X_b_current) == 25
    kept = HipNParEGO(engines, signs, Xb, w, n_mc_samples=S, prune_baseline=True).prune_points(Xb, 9)
    assert len(kept) and all((Xt == row).all(1).any() for row in kept) and len(np.unique(kept, axis=0)) == len(kept)

    one = Xt[5:6]
    lo1, hi1 = ref.bounds(models, signs, one)
    assert np.array_equal(hi1, lo1 + 1.0)
    far = ~coincides_with_baseline(X[:60], one)
    so = ref.scores(models, signs, one, ref.base_samples(S, 1, m, seed), X[:60], w, lo1, hi1)[0]
    for prune in (False, True):  # (a single row is the argmax of every draw)
        hv = HipNParEGO(engines, signs, one, w, n_mc_samples=S, prune_baseline=prune)
        hv.prepare(seed, prune_seed=9)
        sg = hv.score(Xd).cpu().numpy()[:60]
        dev = np.abs(sg - so)[far].max()
        record_deviation(f"qlognparego_scores_one_row_baseline[prune={prune}]", dev, ATOL)
        assert dev <= ATOL and len(hv._pruned) == 1
        assert int(np.argmax(np.where(far, sg, -np.inf))) == int(np.argmax(np.where(far, so, -np.inf)))


def _big_models(m):
    from baybe_amd import engine, gp_spec

    rng = np.random.default_rng(42)
    d, n = 20, 128
    Xt = rng.random((n, d))
    engines = []
    for o in range(m):
        y = -((Xt - 0.25 - 0.5 * o) ** 2).sum(1) + 0.05 * rng.standard_normal(n)
        g = engine.HipGP(0)
        g.set_model(gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d)), Xt, y)
        g.factorize(gp_spec.GPParams(np.full(d, 1.2), 0.02, 0.0))
        engines.append(g)
    return engines, Xt


def test_scoring_pass_allocates_no_sample_matrix():
    """N = 200 000, S = 512, two targets: across one ``score`` the peak of torch's allocator rises by the scores, each target's
    (mean, variance) pair and the chunk buffers - (8 + 16 m) N + CHUNK_BYTES, bound + 16 MB.  The two [S, N] matrices of conditional
    means would be 1.6 GB.  (The library's own workspace is S / 16 doubles per row of ONE chunk.)"""
    import torch

    from baybe_amd import nparego
    from baybe_amd.nparego import HipNParEGO

    m = 2
    engines, Xt = _big_models(m)
    N = 200_000
    Xd = torch.from_numpy(np.random.default_rng(3).random((N, 20))).cuda()
    hv = HipNParEGO(engines, [1.0, 1.0], Xt, [0.4, 0.6], n_mc_samples=512, prune_baseline=True)
    hv.prepare(7, prune_seed=8)
    hv.score(Xd[:4096])  # (first use: handle workspaces, kernel-value cache)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    sc = hv.score(Xd)
    rise = torch.cuda.max_memory_allocated() - before
    bound = (8 + 16 * m) * N + nparego.CHUNK_BYTES + (16 << 20)
    print(f"peak rise across one score at N = {N}, S = 512, m = {m}: {rise / 2**20:.1f} MB (bound {bound / 2**20:.1f} MB)")
    assert N > nparego.CHUNK_BYTES // (8 * 512 * m)  # more than one chunk
    assert bool(torch.isfinite(sc).all()) and rise <= bound
    for g in engines:
        g.close()


def test_recommend_through_the_plugin_surface():
    """``recommend()`` with ``"qLogNParEGO"`` on a two-target ``ParetoObjective`` over a 512-row space: the restatement's greedy batch for
    the hyper-parameters the device fitted (weights drawn first, then the scoring seed, then the pruning seed)."""
    import torch
    from _baybe_shim import NumericalDiscreteParameter, NumericalTarget, ParetoObjective, SearchSpace
    from _pareto_cases import targets
    from _problems import oracle_params, oracle_spec
    from baybe_amd.engine import draw_sampler_seed
    from baybe_amd.recommenders import HipBotorchRecommender
    from oracle import gp_oracle as go

    rng = np.random.default_rng(2)
    vals = np.arange(8) / 7.0
    space = SearchSpace.from_product([NumericalDiscreteParameter(f"x{i}", vals) for i in range(3)])
    exp = space.discrete.exp_rep
    meas = exp.iloc[rng.choice(len(exp), 18, replace=False)].copy()
    T = targets(meas[["x0", "x1", "x2"]].to_numpy(float), rng)
    meas["t1"], meas["t2"] = T[:, 0], -T[:, 1]
    obj = ParetoObjective([NumericalTarget("t1"), NumericalTarget("t2", minimize=True)])
    rec = HipBotorchRecommender(acquisition_function="qLogNParEGO")
    torch.manual_seed(31)
    got = rec.recommend(2, space, obj, meas)
    assert type(rec._scorer).__name__ == "HipNParEGO"
    torch.manual_seed(31)
    w = ref.sample_simplex(2)
    seed, pseed = draw_sampler_seed(), draw_sampler_seed()
    assert np.array_equal(rec._scorer.weights, w)
    models = []
    for sub in rec._surrogate_model.models:
        eng = sub.engine
        models.append(go.GPModel(oracle_spec(eng.spec), oracle_params(eng.spec, eng.params), eng._X_train, eng._y_train))
    signs = np.array([1.0, -1.0])
    Xb = space.transform(meas, allow_extra=True).to_numpy(dtype=np.float64)
    lo, hi = ref.bounds(models, signs, Xb)
    keep, gap = ref.prune(models, signs, Xb, pseed, w, lo, hi)
    assert gap > 1e-7
    comp = space.discrete.comp_rep.to_numpy(dtype=np.float64)
    picks, _ = ref.greedy(models, signs, Xb[keep], comp, 2, 512, seed, w, lo, hi)
    assert list(got.index) == list(exp.index[picks]), (list(got.index), picks)
    acq = rec.acquisition_values(exp.iloc[:50], space, obj, meas)
    assert np.isfinite(acq.to_numpy()).all()
