"""GPU parity tests: the HIP path (through the C-ABI) against the oracle on seeded inputs and
against the committed golden fixtures; at BASELINE sizes through size-independent properties.

Tolerances (fp64 everywhere): posterior mean/variance 1e-9 relative here (north_star allows
1e-5), scores 1e-8 absolute on values of magnitude 1..50, indices identical.
"""

import math
import os
from pathlib import Path

import numpy as np
import pytest

from _problems import fixed_theta, make_problem, make_tl_problem, oracle_spec

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"

MEAN_RTOL = 1e-9
VAR_RTOL = 1e-8
SCORE_ATOL = 1e-8


@pytest.fixture(scope="module")
def gp():
    from baybe_amd import engine

    g = engine.HipGP(0)
    g.selftest()
    yield g
    g.close()


def _ospec(spec):
    return oracle_spec(spec)


def _oparams(p):
    from oracle import gp_oracle as go

    return go.GPParams(np.array(p.lengthscale, dtype=float), p.noise, p.mean, p.outputscale,
                       None if p.task_W is None else p.task_W.copy(), None if p.task_v is None else p.task_v.copy(),
                       bool(getattr(p, "task_unit_scale", False)),
                       None if p.factor_ls is None else [np.array(p.lengthscale, dtype=float)] + [np.array(a, dtype=float) for a in p.factor_ls],
                       None if p.factor_os is None else np.array(p.factor_os, dtype=float),
                       None if getattr(p, "alpha", None) is None else np.array(p.alpha, dtype=float))


def _np(t):
    return t.cpu().numpy()


def test_library_loaded_and_device_present():
    from baybe_amd import _lib

    assert _lib.is_available()


# ---- fit objective -------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,criterion,tl,n", [
    ("matern52", "mll", False, 40), ("rbf", "mll", False, 100), ("matern32", "loo", True, 90),
    ("matern12", "mll", False, 130), ("matern52", "loo", True, 200), ("matern52", "mll", False, 300),
])
def test_data_term_value_and_gradient(gp, kernel, criterion, tl, n):
    from baybe_amd import gp_spec
    from oracle import gp_oracle as go

    d = 5
    if tl:
        X, Xt, y = make_tl_problem(500, d, n // 3, T=3, seed=3)
        spec = gp_spec.GPSpec.baybe_default(d + 1, np.zeros(d + 1), np.ones(d + 1), task_idx=d, n_tasks=3, kernel=kernel)
        spec.use_outputscale = True
    else:
        X, Xt, y = make_problem(500, d, n, seed=1)
        spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d), kernel=kernel)
    spec.criterion = criterion
    p = gp_spec.initial_params(spec)
    rng = np.random.default_rng(5)
    p.lengthscale = p.lengthscale * (0.7 + 0.6 * rng.random(spec.dn))
    p.mean = 0.1
    if tl:
        p.task_W = 0.3 + rng.random((3, 3))
        p.outputscale = 1.3
    gp.set_model(spec, Xt, y)
    val, g = gp.data_term(p)
    ospec = _ospec(spec)
    dt = go.data_term(ospec, _oparams(p), go.normalize_inputs(ospec, Xt), go.standardize_targets(y)[0])
    gref = np.concatenate([[dt.g_noise, dt.g_mean, dt.g_outputscale], dt.g_ls] + ([dt.g_task_B.reshape(-1)] if tl else []))
    assert math.isclose(val, dt.value, rel_tol=1e-11)
    assert np.allclose(g, gref, rtol=1e-9, atol=1e-10 * np.abs(gref).max())


def test_non_positive_definite_is_reported_not_hidden(gp):
    from baybe_amd import gp_spec

    X, Xt, y = make_problem(200, 3, 30, seed=2)
    Xt = np.vstack([Xt, Xt[:5]])  # exact duplicates
    y = np.concatenate([y, y[:5]])
    spec = gp_spec.GPSpec.baybe_default(3, np.zeros(3), np.ones(3), kernel="rbf")
    gp.set_model(spec, Xt, y)
    p = gp_spec.GPParams(np.full(3, 50.0), -1.0, 0.0)  # negative "noise": K - I is not PD
    val, g = gp.data_term(p)
    assert val is None and g is None


@pytest.mark.parametrize("n,d", [(60, 5), (128, 10)])
def test_device_fit_reaches_the_oracle_optimum(gp, n, d):
    from baybe_amd import gp_spec
    from oracle import gp_oracle as go

    X, Xt, y = make_problem(1000, d, n, seed=6)
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    gp.set_model(spec, Xt, y)
    fi = gp.fit()
    ospec = _ospec(spec)
    fo = go.fit_hyperparameters(ospec, go.normalize_inputs(ospec, Xt), go.standardize_targets(y)[0])
    assert math.isclose(fi.fun, fo.fun, rel_tol=1e-8)
    assert np.allclose(fi.params.lengthscale, fo.params.lengthscale, rtol=1e-4)
    assert math.isclose(fi.params.noise, fo.params.noise, rel_tol=1e-4)


@pytest.mark.parametrize("preset", ["EDBO", "EDBO_SMOOTHED", "CHEN", "HVARFNER"])
def test_preset_fit_on_device_reaches_the_oracle_optimum(gp, preset):
    """The reference's other GP presets are data for the same kernels: ScaleKernel +
    softplus-constrained lengthscales / noise (EDBO family, CHEN), RBF with LogNormal priors (HVARFNER)."""
    from baybe_amd import gp_spec
    from oracle import gp_oracle as go

    n, d = 50, 6
    X, Xt, y = make_problem(500, d, n, seed=8)
    spec = gp_spec.from_preset(preset, d, np.zeros(d), np.ones(d))
    gp.set_model(spec, Xt, y)
    fi = gp.fit()
    ospec = _ospec(spec)
    fo = go.fit_hyperparameters(ospec, go.normalize_inputs(ospec, Xt), go.standardize_targets(y)[0])
    # strong priors make these objectives flat near the optimum: L-BFGS-B may stop a few 1e-7 apart
    assert math.isclose(fi.fun, fo.fun, rel_tol=1e-6)
    assert np.allclose(fi.params.lengthscale, fo.params.lengthscale, rtol=2e-2)
    assert math.isclose(fi.params.noise, fo.params.noise, rel_tol=2e-2)
    assert math.isclose(fi.params.outputscale, fo.params.outputscale, rel_tol=2e-2)
    m, v = gp.posterior(X)
    mo, vo = go.GPModel(ospec, _oparams(fi.params), Xt, y).posterior(X)
    assert np.allclose(_np(m), mo, rtol=MEAN_RTOL, atol=1e-12) and np.allclose(_np(v), vo, rtol=VAR_RTOL)


# ---- posterior -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,n", [(3000, 5, 40), (3000, 15, 200), (3000, 20, 300), (5000, 20, 512),
                                   (2000, 3, 20), (1000, 9, 700), (777, 2, 1), (513, 30, 65), (64, 4, 1030),
                                   (600, 45, 300), (300, 62, 280), (200, 70, 100)])  # 12 / 16 k-steps, plain form
def test_posterior_fused_and_unfused_match_oracle(gp, N, d, n):
    from baybe_amd import gp_spec
    from oracle import gp_oracle as go

    X, Xt, y = make_problem(max(N, n + 1), d, n, seed=2)
    X = X[:N]
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    ls, nz, _ = fixed_theta(d)
    p = gp_spec.GPParams(np.full(d, ls) * (0.8 + 0.4 * np.random.default_rng(7).random(d)), nz, 0.05)
    gp.set_model(spec, Xt, y)
    gp.factorize(p)
    om = go.GPModel(_ospec(spec), _oparams(p), Xt, y)
    mo, vo = om.posterior(X)
    for unfused in (False, True):
        m, v = gp.posterior(X, unfused=unfused)
        assert np.allclose(_np(m), mo, rtol=MEAN_RTOL, atol=1e-12)
        assert np.allclose(_np(v), vo, rtol=VAR_RTOL)
    assert np.allclose(gp.train_posterior_mean(), om.posterior(Xt)[0], rtol=MEAN_RTOL, atol=1e-12)
    assert math.isclose(gp.best_f(-1.0), go.best_f_from_model(om, -1.0), rel_tol=1e-9, abs_tol=1e-12)


@pytest.mark.parametrize("N,d,n,kernel", [(20_000, 20, 600, "matern52"), (30_000, 6, 1100, "matern52"),
                                          (4_000, 28, 300, "matern52"), (20_000, 12, 600, "rbf"), (5_000, 40, 520, "rbf"),
                                          (20_000, 9, 600, "matern32")])
def test_pipelined_kernel_matches_plain_form(monkeypatch, N, d, n, kernel):
    """The software-pipelined fused kernel (staged rsq/Taylor Matérn evaluation, kernel-value cache
    in wave-private LDS and in global slabs claimed per wave) against the same launch with libm sqrt/exp and
    no cache; the switches are
    read when the handle is created.  Enough candidates to keep every CU busy, several passes."""
    from baybe_amd import engine, gp_spec

    X, Xt, y = make_problem(N, d, n, seed=11)
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d), kernel=kernel)
    ls, nz, _ = fixed_theta(d)
    p = gp_spec.GPParams(np.full(d, ls), nz, 0.0)
    out = {}
    for name, env in (("pipelined", {}), ("slabs", {"BBH_KV_GLOBAL": "1", "BBH_KV_LDS": "3"}),
                      ("no_cache", {"BBH_KVCACHE": "0"}), ("plain", {"BBH_PIPELINE": "0"})):
        for k in ("BBH_KVCACHE", "BBH_PIPELINE", "BBH_KV_GLOBAL", "BBH_KV_LDS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g = engine.HipGP(0)
        try:
            g.set_model(spec, Xt, y)
            g.factorize(p)
            for _ in range(3):  # slabs are re-claimed on every launch
                m, v = g.posterior(X)
            out[name] = (_np(m), _np(v))
        finally:
            g.close()
    scale = float(np.std(y))
    for name in ("pipelined", "slabs", "no_cache"):
        assert np.max(np.abs(out[name][0] - out["plain"][0])) <= 1e-11 * scale
        assert np.max(np.abs(out[name][1] - out["plain"][1])) <= 1e-11 * scale**2
    for name in ("pipelined", "slabs"):  # cached values (LDS / global slabs) are the computed ones
        assert np.array_equal(out[name][0], out["no_cache"][0])
        assert np.array_equal(out[name][1], out["no_cache"][1])


@pytest.mark.parametrize("N,d,n", [(1, 4, 300), (63, 6, 257), (65, 3, 320), (1000, 7, 513), (130, 20, 777),
                                   (4097, 14, 272), (17, 30, 1041), (333, 15, 1024), (49, 9, 600)])
def test_multi_pass_edges_fused_matches_unfused(gp, N, d, n):
    """Ragged candidate counts (partial tiles, partial workgroups) against every pass layout of the
    fused kernel (last-pass widths 4/8/12/16, 2-5 passes, slab cache in use): the fused launch must agree
    with the unfused reference path (explicit K*, GEMM with L^-1, row reductions)."""
    from baybe_amd import gp_spec

    X, Xt, y = make_problem(max(N, n + 1), d, n, seed=13)
    X = X[:N]
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    ls, nz, _ = fixed_theta(d)
    gp.set_model(spec, Xt, y)
    gp.factorize(gp_spec.GPParams(np.full(d, ls), nz, 0.1))
    m, v = gp.posterior(X)
    mu, vu = gp.posterior(X, unfused=True)
    assert np.allclose(_np(m), _np(mu), rtol=1e-10, atol=1e-12)
    assert np.allclose(_np(v), _np(vu), rtol=1e-8, atol=1e-13)


def test_posterior_scaling_bounds_and_strided_input(gp):
    """Normalize uses the search-space bounds (not the candidate range) and honours ldx > d."""
    import torch

    from baybe_amd import gp_spec
    from oracle import gp_oracle as go

    rng = np.random.default_rng(3)
    d, n, N = 4, 50, 1000
    lo, hi = np.array([-2.0, 10.0, 0.0, 100.0]), np.array([3.0, 20.0, 0.5, 400.0])
    X = lo + (hi - lo) * rng.random((N, d))
    Xt = lo + (hi - lo) * rng.random((n, d))
    y = np.sin(Xt[:, 0]) + 0.01 * Xt[:, 3]
    spec = gp_spec.GPSpec.baybe_default(d, lo, hi)
    gp.set_model(spec, Xt, y)
    p = gp_spec.GPParams(np.array([0.3, 0.5, 0.7, 0.4]), 1e-3, -0.2)
    gp.factorize(p)
    om = go.GPModel(_ospec(spec), _oparams(p), Xt, y)
    mo, vo = om.posterior(X)
    wide = torch.zeros((N, d + 3), dtype=torch.float64, device="cuda")
    wide[:, :d] = torch.from_numpy(X).cuda()
    m, v = gp.posterior(wide)
    assert np.allclose(_np(m), mo, rtol=MEAN_RTOL, atol=1e-12) and np.allclose(_np(v), vo, rtol=VAR_RTOL)


def test_multitask_icm_posterior_and_loo(gp):
    from baybe_amd import gp_spec

    g = np.load(GOLD / "tl_4tasks.npz")
    T = int(g["T"])
    d = g["X"].shape[1]
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d), task_idx=d - 1, n_tasks=T)
    p = gp_spec.GPParams(g["ls"], float(g["noise"]), float(g["mean_const"]), 1.0, g["task_W"], g["task_v"])
    gp.set_model(spec, g["Xt"], g["y"])
    val, grad = gp.data_term(p)
    assert math.isclose(val, float(g["dt_value"]), rel_tol=1e-10)
    assert np.allclose(grad, g["dt_grad"], rtol=1e-8, atol=1e-9 * np.abs(g["dt_grad"]).max())
    gp.factorize(p)
    for unfused in (False, True):
        m, v = gp.posterior(g["X"], unfused=unfused)
        assert np.allclose(_np(m), g["post_mean"], rtol=MEAN_RTOL, atol=1e-12)
        assert np.allclose(_np(v), g["post_var"], rtol=VAR_RTOL)


# ---- golden fixtures -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg1_plumbing", "small_matern52_max", "small_matern52_min", "small_rbf",
                                  "small_matern32", "small_matern12", "mid_320"])
def test_golden_fixture(gp, name):
    import torch

    from baybe_amd import gp_spec

    g = np.load(GOLD / f"{name}.npz")
    d = g["X"].shape[1]
    sign = float(g["sign"])
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d), kernel=str(g["kernel"]))
    gp.set_model(spec, g["Xt"], g["y"])
    val, grad = gp.data_term(gp_spec.initial_params(spec))
    assert math.isclose(val, float(g["dt_value"]), rel_tol=1e-10)
    assert np.allclose(grad, g["dt_grad"], rtol=1e-8, atol=1e-9 * np.abs(g["dt_grad"]).max())
    gp.factorize(gp_spec.GPParams(g["ls"], float(g["noise"]), float(g["mean_const"])))
    m, v = gp.posterior(g["X"])
    assert np.allclose(_np(m), g["post_mean"], rtol=MEAN_RTOL, atol=1e-12)
    assert np.allclose(_np(v), g["post_var"], rtol=VAR_RTOL)
    bf = gp.best_f(sign)
    assert math.isclose(bf, float(g["best_f"]), rel_tol=1e-9, abs_tol=1e-12)
    s = gp.qlogei(m, v, g["z1"], float(g["best_f"]), sign)
    assert np.allclose(_np(s), g["scores"], rtol=0, atol=SCORE_ATOL)
    sf, mf, vf = gp.score_qlogei(g["X"], g["z1"], float(g["best_f"]), sign)  # fused posterior + qLogEI
    assert np.allclose(_np(sf), g["scores"], rtol=0, atol=SCORE_ATOL)
    # (the stand-alone posterior may run the cooperative kernel form, the fused epilogue always runs the windowed one:
    #  same values up to the summation order of ||v||^2)
    assert torch.allclose(mf, m, rtol=1e-12, atol=1e-13) and torch.allclose(vf, v, rtol=1e-11, atol=1e-15)
    sf2, none_m, _ = gp.score_qlogei(g["X"], g["z1"], float(g["best_f"]), sign, want_posterior=False)
    assert none_m is None and torch.equal(sf2, sf)
    assert gp.argmax(s)[1] == int(np.argmax(g["scores"]))
    k = 8
    assert gp.topk(s, k)[1].tolist() == np.argsort(-g["scores"], kind="stable")[:k].tolist()
    if name != "mid_320":
        r = gp.greedy_qlogei(g["X"], int(g["q"]), seed=4321, sign=sign, X_pending=g["pend"], best_f=float(g["best_f"]))
        assert r.indices == g["greedy_idx"].tolist()
        assert np.allclose(r.values, g["greedy_val"], rtol=0, atol=SCORE_ATOL)


def test_cfg1_fit_on_device_reproduces_oracle_fit(gp):
    from baybe_amd import gp_spec

    g = np.load(GOLD / "cfg1_plumbing.npz")
    spec = gp_spec.GPSpec.baybe_default(3, np.zeros(3), np.ones(3))
    gp.set_model(spec, g["Xt"], g["y"])
    fi = gp.fit()
    assert np.allclose(fi.params.lengthscale, g["ls"], rtol=1e-4)
    assert math.isclose(fi.params.noise, float(g["noise"]), rel_tol=1e-4)
    r = gp.greedy_qlogei(g["X"], int(g["q"]), seed=4321, X_pending=g["pend"])
    assert r.indices == g["greedy_idx"].tolist()


# ---- acquisition edge cases ----------------------------------------------------------------------
def test_qlogei_edge_cases(gp):
    import torch

    from oracle import gp_oracle as go

    z = go.sobol_normal_base_samples(512, 1, 3)[:, 0]
    mu = np.array([0.0, 5.0, -5.0, 1.0, 1.0, 0.3])
    var = np.array([1.0, 1e-12, 4.0, 0.0, -1e-13, 1e-9])  # zero / negative variance -> jitter rule
    for sign, bf in ((1.0, 0.9), (-1.0, 0.2)):
        so = go.qlogei_q1(mu, var, z, bf, sign)
        s = gp.qlogei(torch.from_numpy(mu).cuda(), torch.from_numpy(var).cuda(), z, bf, sign)
        assert np.allclose(_np(s), so, rtol=0, atol=1e-9)
    alive = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8, device="cuda")
    s = _np(gp.qlogei(torch.from_numpy(mu).cuda(), torch.from_numpy(var).cuda(), z, 0.9, 1.0, alive))
    assert np.isneginf(s[1]) and np.isneginf(s[4]) and np.isfinite(s[[0, 2, 3, 5]]).all()


def test_argmax_ties_nan_and_all_masked(gp):
    import torch

    s = torch.tensor([1.0, 3.0, float("nan"), 3.0, 2.0], dtype=torch.float64, device="cuda")
    assert gp.argmax(s) == (3.0, 1)
    s = torch.full((5000,), -math.inf, dtype=torch.float64, device="cuda")
    assert gp.argmax(s)[1] == 0
    big = torch.zeros(300001, dtype=torch.float64, device="cuda")
    big[[123456, 299999, 70000]] = 7.0
    assert gp.argmax(big) == (7.0, 70000)
    v, i = gp.topk(big, 4)
    assert i.tolist() == [70000, 123456, 299999, 0]
    rng = np.random.default_rng(0)
    for N, k in ((1, 1), (5, 5), (4097, 64), (100_000, 17), (1_000_000, 8)):
        x = rng.integers(0, 50, size=N).astype(np.float64)  # many ties
        x[rng.integers(0, N, size=max(1, N // 100))] = np.nan
        xs = np.where(np.isnan(x), -np.inf, x)
        order = np.argsort(-xs, kind="stable")[:k]
        valid = int((~np.isnan(x)).sum())
        v, i = gp.topk(torch.from_numpy(x).cuda(), k)
        kk = min(k, valid)
        assert i[:kk].tolist() == order[:kk].tolist() and np.array_equal(v[:kk], xs[order[:kk]])


@pytest.mark.parametrize("N,d,n,q,minimize", [(2000, 5, 40, 4, False), (3000, 8, 100, 3, True),
                                               (700, 4, 30, 10, False)])  # q' = 9, 10: generic LDS form
def test_greedy_with_pending_matches_oracle(gp, N, d, n, q, minimize):
    from baybe_amd import gp_spec
    from oracle import gp_oracle as go

    X, Xt, y = make_problem(N, d, n, seed=4, minimize=minimize)
    sign = -1.0 if minimize else 1.0
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    ls, nz, _ = fixed_theta(d)
    p = gp_spec.GPParams(np.full(d, ls), nz, 0.0)
    gp.set_model(spec, Xt, y)
    gp.factorize(p)
    om = go.GPModel(_ospec(spec), _oparams(p), Xt, y)
    ro = go.optimize_acqf_discrete_qlogei(om, X, q, seed=77, sign=sign, X_pending=X[:1])
    rg = gp.greedy_qlogei(X, q, seed=77, sign=sign, X_pending=X[:1])
    assert rg.indices == ro.indices
    assert np.allclose(rg.values, ro.values, rtol=0, atol=SCORE_ATOL)
    # per-candidate scores with two pending points (candidates distinct from the pending rows)
    pend = X[[3, 10]]
    keep = np.ones(600, bool)
    keep[[3, 10]] = False
    Xc = X[:600][keep]
    z = go.sobol_normal_base_samples(512, 3, 5)
    bf = go.best_f_from_model(om, sign)
    so = go.qlogei_with_pending(om, Xc, pend, z, bf, sign)
    mp_, cpp = gp.set_pending(pend)
    mo_p, co_p = om.posterior_joint(pend)
    assert np.allclose(mp_, mo_p, rtol=1e-10) and np.allclose(cpp, co_p, rtol=1e-8, atol=1e-14)
    m, v = gp.posterior(Xc)
    cr = gp.cross_cov(Xc)
    sg = _np(gp.qlogei_pending(m, v, cr, z, bf, sign))
    assert np.allclose(sg, so, rtol=0, atol=SCORE_ATOL)
    gp.set_pending(None)


def test_pending_points_are_not_recommended_again_on_device(gp):
    from baybe_amd import gp_spec

    X, Xt, y = make_problem(600, 4, 30, seed=7)
    spec = gp_spec.GPSpec.baybe_default(4, np.zeros(4), np.ones(4))
    gp.set_model(spec, Xt, y)
    gp.fit()
    r1 = gp.greedy_qlogei(X, 3, seed=1337)
    mask = np.ones(len(X), bool)
    mask[r1.indices] = False
    r2 = gp.greedy_qlogei(X[mask], 3, seed=1337, X_pending=X[r1.indices])
    first = {tuple(np.round(X[i], 3)) for i in r1.indices}
    second = {tuple(np.round(X[mask][i], 3)) for i in r2.indices}
    assert not (first & second) and len(set(r1.indices)) == 3


# ---- BASELINE sizes: size-independent properties ----------------------------------------------
@pytest.mark.parametrize("N,d,n", [(100_000, 15, 256), (1_000_000, 20, 512)])
def test_full_size_properties(gp, N, d, n):
    """cfg2 / cfg3 of BASELINE.json.  (i) fused == unfused posterior on a 20k slice; (ii) the
    oracle agrees on a 4k sample and on the global top candidates; (iii) minimise(-y) mirrors
    maximise(y) exactly (reference tests/integration/test_minimization.py:41-78); (iv) scoring is
    idempotent and permutation-equivariant."""
    import torch

    from baybe_amd import gp_spec
    from oracle import gp_oracle as go

    X, Xt, y = make_problem(N, d, n, seed=0)
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    ls, nz, _ = fixed_theta(d)
    p = gp_spec.GPParams(np.full(d, ls), nz, 0.0)
    gp.set_model(spec, Xt, y)
    gp.factorize(p)
    Xd = torch.from_numpy(X).cuda()
    m, v = gp.posterior(Xd)
    z = go.sobol_normal_base_samples(512, 1, 1234)[:, 0]
    bf = gp.best_f()
    s = gp.qlogei(m, v, z, bf)
    # (i)
    m2, v2 = gp.posterior(Xd[:20000], unfused=True)
    assert torch.allclose(m[:20000], m2, rtol=MEAN_RTOL, atol=1e-12) and torch.allclose(v[:20000], v2, rtol=VAR_RTOL)
    # (ii)
    om = go.GPModel(_ospec(spec), _oparams(p), Xt, y)
    vals, top = gp.topk(s, 10)
    pick = np.concatenate([np.random.default_rng(1).choice(N, 4000, replace=False), top])
    mo, vo = om.posterior(X[pick])
    assert np.allclose(_np(m)[pick], mo, rtol=MEAN_RTOL, atol=1e-12) and np.allclose(_np(v)[pick], vo, rtol=VAR_RTOL)
    so = go.qlogei_q1(mo, vo, z, go.best_f_from_model(om))
    assert np.allclose(_np(s)[pick], so, rtol=0, atol=SCORE_ATOL)
    assert math.isclose(bf, go.best_f_from_model(om), rel_tol=1e-9)
    # (iv) idempotent, and scoring a permuted candidate set permutes the scores
    m3, v3 = gp.posterior(Xd)
    assert torch.equal(m, m3) and torch.equal(v, v3)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(0)).cuda()
    mp_, vp_ = gp.posterior(Xd[perm].contiguous())
    assert torch.allclose(mp_, m[perm], rtol=1e-12, atol=1e-13) and torch.allclose(vp_, v[perm], rtol=1e-10)
    # (iii)
    gp.set_model(spec, Xt, -y)
    gp.factorize(p)
    mn, vn = gp.posterior(Xd)
    assert torch.allclose(mn, -m, rtol=0, atol=1e-12) and torch.allclose(vn, v, rtol=1e-12)
    sn = gp.qlogei(mn, vn, -z, gp.best_f(-1.0), -1.0)
    assert torch.allclose(sn, s, rtol=1e-9, atol=1e-9)
    assert gp.argmax(sn)[1] == gp.argmax(s)[1]


# ---- multi-task HVARFNER / BOTORCH presets ----------------------------------------------------------
@pytest.mark.parametrize("preset,n_per_task,T", [("HVARFNER", 30, 3), ("BOTORCH", 25, 2), ("BOTORCH", 170, 3)])
def test_multitask_botorch_presets_data_term_posterior_and_fit(gp, preset, n_per_task, T):
    """Multi-task HVARFNER / BOTORCH (presets/hvarfner.py:72-137, presets/botorch.py:80-92): RBF x target-scaled index
    kernel, one noise variance and one constant mean per task (theta tail, ``bbh_model_desc.hadamard``), plain MLL.
    Data term + gradient, posterior (per-task mean in every kernel form's epilogue, joint and pending paths) and the
    device fit against the oracle."""
    from baybe_amd import gp_spec
    from oracle import gp_oracle as go

    d = 6
    X, Xt, y = make_tl_problem(4000, d, n_per_task, T=T, seed=13)
    spec = gp_spec.from_preset(preset, d + 1, np.zeros(d + 1), np.ones(d + 1), task_idx=d, n_tasks=T)
    ospec = _ospec(spec)
    rng = np.random.default_rng(2)
    p = gp_spec.initial_params(spec)
    p.lengthscale = p.lengthscale * (0.6 + 0.8 * rng.random(spec.dn)) * 0.3
    p.noise = 1e-3 + 0.05 * rng.random(T)
    p.mean = 0.4 * rng.standard_normal(T)
    p.task_W = 0.2 + rng.random((T, T))
    gp.set_model(spec, Xt, y)
    val, g = gp.data_term(p)
    Xn, ys = go.normalize_inputs(ospec, Xt), go.standardize_targets(y)[0]
    dt = go.data_term(ospec, _oparams(p), Xn, ys)
    gref = np.concatenate([[0.0, 0.0, dt.g_outputscale], dt.g_ls, dt.g_task_B.reshape(-1), dt.g_noise, dt.g_mean])
    assert len(g) == 3 + spec.dn + T * T + 2 * T
    assert math.isclose(val, dt.value, rel_tol=1e-11)
    assert np.allclose(g, gref, rtol=1e-9, atol=1e-10 * np.abs(gref).max())
    # posterior: fused (cooperative / windowed) and unfused forms, joint form, pending points
    gp.factorize(p)
    om = go.GPModel(ospec, _oparams(p), Xt, y)
    mo, vo = om.posterior(X)
    for unfused in (False, True):
        m, v = gp.posterior(X, unfused=unfused)
        assert np.allclose(_np(m), mo, rtol=MEAN_RTOL, atol=1e-12) and np.allclose(_np(v), vo, rtol=VAR_RTOL, atol=1e-14)
    if n_per_task * T <= 512:
        gp.posterior(X)
        assert gp.posterior_kernel_form() in ("cooperative", "register-resident")  # (n <= 128: the small-model form, bbh_small.h)
    mj, cj = gp.posterior_joint(X[:7])
    moj, coj = om.posterior_joint(X[:7])
    assert np.allclose(mj, moj, rtol=MEAN_RTOL, atol=1e-12) and np.allclose(cj, coj, rtol=1e-7, atol=1e-12)
    pm, pc = gp.set_pending(X[[3, 11]])
    assert np.allclose(pm, om.posterior(X[[3, 11]])[0], rtol=MEAN_RTOL, atol=1e-12)
    gp.set_pending(None)
    assert np.allclose(gp.train_posterior_mean(), om.posterior(Xt)[0], rtol=MEAN_RTOL, atol=1e-12)
    if n_per_task > 100 or preset == "HVARFNER":
        return  # the fit below runs for BOTORCH at the small size (HVARFNER's: tests/test_plugin_gpu.py, through the surrogate)
    # The target-scaled index kernel leaves the overall scale of (covar_factor, var) without any effect on the model: the
    # objective has an exactly flat direction, L-BFGS-B runs 500 - 700 iterations along a near-flat valley and two runs whose
    # gradients differ in the last bits stop a few 1e-6 apart.  Compared: the value reached, the identifiable quantities,
    # and the posteriors of the two fitted models.
    fi = gp.fit()
    fo = go.fit_hyperparameters(ospec, Xn, ys)
    assert math.isclose(fi.fun, fo.fun, rel_tol=5e-5)
    assert np.allclose(fi.params.task_B(), fo.params.task_B(), rtol=0.1, atol=2e-2)
    assert np.allclose(fi.params.noise, fo.params.noise, rtol=0.2, atol=5e-4)
    assert np.allclose(fi.params.mean, fo.params.mean, rtol=0.1, atol=5e-2)
    m, v = gp.posterior(X)
    mo, vo = go.GPModel(ospec, _oparams(fi.params), Xt, y).posterior(X)
    assert np.allclose(_np(m), mo, rtol=MEAN_RTOL, atol=1e-12) and np.allclose(_np(v), vo, rtol=VAR_RTOL, atol=1e-14)
    mf, _ = go.GPModel(ospec, fo.params, Xt, y).posterior(X)
    assert np.max(np.abs(mf - mo)) < 0.05 * np.std(y)


# ---- user ProductKernel / AdditiveKernel / PiecewisePolynomialKernel ---------------------------------
def _composite_kernels():
    from baybe_amd.kernels import (AdditiveKernel, GammaPrior, LogNormalPrior, MaternKernel, PiecewisePolynomialKernel, ProductKernel,
                                   RBFKernel, ScaleKernel)

    return {
        "product": ProductKernel([MaternKernel(2.5, GammaPrior(3, 1)), ScaleKernel(RBFKernel(), GammaPrior(2, 0.5))]),
        "scaled_sum": ScaleKernel(AdditiveKernel([ScaleKernel(MaternKernel(1.5)), ScaleKernel(RBFKernel(LogNormalPrior(0, 1))),
                                                  MaternKernel(0.5)]), GammaPrior(2, 0.15)),
        "product4": ProductKernel([RBFKernel(), MaternKernel(1.5), MaternKernel(2.5), ScaleKernel(MaternKernel(0.5))]),
        "piecewise_x_rbf": ProductKernel([PiecewisePolynomialKernel(2, None, 3.0), ScaleKernel(RBFKernel())]),
        # the nested entry of the reference's kernel matrix (tests/test_iterations.py:294-296): (Matern * Matern) + (Matern + Matern)
        "sum_of_products": AdditiveKernel([ProductKernel([MaternKernel(2.5, GammaPrior(3, 1)), MaternKernel(1.5)]),
                                           AdditiveKernel([ScaleKernel(MaternKernel(2.5), GammaPrior(2, 0.5)), RBFKernel()])]),
    }


@pytest.mark.parametrize("name,tl", [("product", False), ("scaled_sum", False), ("product4", False), ("product", True),
                                     ("piecewise_x_rbf", False), ("sum_of_products", False), ("sum_of_products", True)])
def test_composite_kernels_data_term_posterior_and_greedy(gp, name, tl):
    """User ``ProductKernel`` / ``AdditiveKernel`` (baybe/kernels/composite.py:60-91) of 2..4 stationary factors, each with
    its own ARD lengthscales and optionally its own ScaleKernel (``bbh_model_desc.n_factors``): Gram matrix and gradient
    slots, the materialised-K* posterior (mean, variance, pending cross-covariances, joint form) and a greedy batch with
    pending points against the oracle; with the ICM task factor on top as well."""
    from baybe_amd import gp_spec
    from baybe_amd.kernels import apply_kernel_spec
    from oracle import gp_oracle as go

    d = 5
    if tl:
        X, Xt, y = make_tl_problem(3000, d, 25, T=3, seed=21)
        spec = gp_spec.GPSpec.baybe_default(d + 1, np.zeros(d + 1), np.ones(d + 1), task_idx=d, n_tasks=3)
    else:
        X, Xt, y = make_problem(3000, d, 70, seed=21)
        spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    apply_kernel_spec(spec, _composite_kernels()[name])
    spec.criterion = "loo" if tl else "mll"
    F = spec.n_factors
    ospec = _ospec(spec)
    rng = np.random.default_rng(7)
    p = gp_spec.initial_params(spec)
    p.lengthscale = p.lengthscale * (0.5 + rng.random(spec.dn))
    p.factor_ls = [l * (0.5 + rng.random(spec.dn)) * (1.5 if name == "product4" else 1.0) for l in p.factor_ls]
    p.factor_os = np.where(np.array([f.scaled for f in spec.factors]), 0.5 + rng.random(F), 1.0)
    p.noise, p.mean = 0.02, 0.15
    if spec.use_outputscale:
        p.outputscale = 1.7
    if tl:
        p.task_W = 0.3 + rng.random((3, 3))
    gp.set_model(spec, Xt, y)
    val, g = gp.data_term(p)
    Xn, ys = go.normalize_inputs(ospec, Xt), go.standardize_targets(y)[0]
    dt = go.data_term(ospec, _oparams(p), Xn, ys)
    gref = np.concatenate([[dt.g_noise, dt.g_mean, dt.g_outputscale], dt.g_member_ls[0]] + ([dt.g_task_B.reshape(-1)] if tl else [])
                          + dt.g_member_ls[1:] + [dt.g_member_scale])
    assert len(g) == len(gref) == 3 + F * spec.dn + F + (9 if tl else 0)
    assert math.isclose(val, dt.value, rel_tol=1e-11)
    assert np.allclose(g, gref, rtol=1e-9, atol=1e-10 * np.abs(gref).max())
    gp.factorize(p)
    om = go.GPModel(ospec, _oparams(p), Xt, y)
    mo, vo = om.posterior(X)
    for unfused in (False, True):
        m, v = gp.posterior(X, unfused=unfused)
        assert np.allclose(_np(m), mo, rtol=MEAN_RTOL, atol=1e-12) and np.allclose(_np(v), vo, rtol=VAR_RTOL, atol=1e-14)
    gp.posterior(X)
    # variance passes: the cooperative kernel with the generic production (bbh_coopg.h) unless a Matérn-1/2 factor is present
    # (direct-difference distances near r = 0: materialised-K* path)
    assert gp.posterior_kernel_form() == ("materialised" if name in ("scaled_sum", "product4") else "cooperative-generic")
    mj, cj = gp.posterior_joint(X[:6])
    moj, coj = om.posterior_joint(X[:6])
    assert np.allclose(mj, moj, rtol=MEAN_RTOL, atol=1e-12) and np.allclose(cj, coj, rtol=1e-7, atol=1e-12)
    assert np.allclose(gp.train_posterior_mean(), om.posterior(Xt)[0], rtol=MEAN_RTOL, atol=1e-12)
    # greedy batch with pending points: same picks, same joint values as the oracle loop
    cand = np.ascontiguousarray((X[X[:, d] == 0] if tl else X)[:800])
    res = gp.greedy_qlogei(cand, 3, seed=5)
    ref = go.optimize_acqf_discrete_qlogei(om, cand, 3, seed=5)
    assert list(res.indices) == list(ref.indices)
    assert np.allclose(res.values, ref.values, rtol=0, atol=SCORE_ATOL)
    # mean-only / cross-covariance passes (steps >= 2 of a greedy batch; round 4: bbh_coopg_cross_kernel where the generic production
    # applies): against the oracle's joint posterior, and against the materialised-K* path on a handle created under BBH_COOPG_CROSS=0
    from baybe_amd import engine

    P = cand[[5, 77, 300]]
    gp.set_pending(P)
    cr = _np(gp.cross_cov(cand[:600]))
    gp.set_pending(None)
    for i in (0, 17, 599):
        _, cov = om.posterior_joint(np.vstack([cand[i:i + 1], P]))
        assert np.allclose(cr[i], cov[0, 1:], rtol=1e-7, atol=1e-12), (i, cr[i], cov[0, 1:])
    from _pending_cases import batched_cross  # every row (the batched form is pinned to posterior_joint in test_pending_cases_cpu.py)

    assert np.allclose(cr, batched_cross(om, cand[:600], P), rtol=1e-7, atol=1e-12)
    os.environ["BBH_COOPG_CROSS"] = "0"
    try:
        g2 = engine.HipGP(0)
        g2.set_model(spec, Xt, y)
        g2.factorize(p)
        g2.set_pending(P)
        cr2 = _np(g2.cross_cov(cand[:600]))
        assert np.allclose(g2.train_posterior_mean(), gp.train_posterior_mean(), rtol=1e-11, atol=1e-13)
        g2.close()
    finally:
        del os.environ["BBH_COOPG_CROSS"]
    assert np.allclose(cr, cr2, rtol=1e-9, atol=1e-13), np.abs(cr - cr2).max()


@pytest.mark.parametrize("q", [0, 1, 2, 3])
def test_piecewise_polynomial_kernels(gp, q):
    """``PiecewisePolynomialKernel(q)`` (baybe/kernels/basic.py:114-131; gpytorch: (1 - r)_+^(j + q) P_q(r), j = floor(d / 2) + q
    + 1): value and the closed-form lengthscale derivative on the device against the oracle's product-rule form, the
    materialised-K* posterior (compact support: exact zeros in K*), a greedy batch and the device fit."""
    from baybe_amd import gp_spec
    from baybe_amd.kernels import GammaPrior, PiecewisePolynomialKernel, ScaleKernel, apply_kernel_spec
    from oracle import gp_oracle as go

    d = 5
    X, Xt, y = make_problem(2000, d, 60, seed=40 + q)
    spec = apply_kernel_spec(gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d)),
                             ScaleKernel(PiecewisePolynomialKernel(q, GammaPrior(3.0, 1.0), 1.5), GammaPrior(2.0, 0.5)))
    assert spec.kernel == f"piecewise{q}" and spec.use_outputscale
    ospec = _ospec(spec)
    rng = np.random.default_rng(q)
    p = gp_spec.initial_params(spec)
    p.lengthscale = p.lengthscale * (0.6 + 0.8 * rng.random(d))  # support radius ~ 1 - 2 in the unit cube: zeros and non-zeros
    p.noise, p.mean, p.outputscale = 0.03, -0.1, 1.4
    gp.set_model(spec, Xt, y)
    val, g = gp.data_term(p)
    Xn, ys = go.normalize_inputs(ospec, Xt), go.standardize_targets(y)[0]
    dt = go.data_term(ospec, _oparams(p), Xn, ys)
    gref = np.concatenate([[dt.g_noise, dt.g_mean, dt.g_outputscale], dt.g_ls])
    assert math.isclose(val, dt.value, rel_tol=1e-11)
    assert np.allclose(g, gref, rtol=1e-9, atol=1e-10 * np.abs(gref).max())
    gp.factorize(p)
    om = go.GPModel(ospec, _oparams(p), Xt, y)
    mo, vo = om.posterior(X)
    for unfused in (False, True):
        m, v = gp.posterior(X, unfused=unfused)
        assert np.allclose(_np(m), mo, rtol=MEAN_RTOL, atol=1e-12) and np.allclose(_np(v), vo, rtol=VAR_RTOL, atol=1e-14)
    gp.posterior(X)
    # q = 0, (1 - r)^j, is not smooth at r = 0 (as Matérn-1/2): direct-difference distances, i.e. the materialised-K* path
    assert gp.posterior_kernel_form() == ("materialised" if q == 0 else "cooperative-generic")
    cand = np.ascontiguousarray(X[:600])
    res = gp.greedy_qlogei(cand, 3, seed=8)
    ref = go.optimize_acqf_discrete_qlogei(om, cand, 3, seed=8)
    assert list(res.indices) == list(ref.indices) and np.allclose(res.values, ref.values, rtol=0, atol=SCORE_ATOL)
    if q in (1, 2):
        fi = gp.fit()
        fo = go.fit_hyperparameters(ospec, Xn, ys)
        assert math.isclose(fi.fun, fo.fun, rel_tol=1e-6)
        assert np.allclose(fi.params.lengthscale, fo.params.lengthscale, rtol=2e-2)


@pytest.mark.parametrize("name", ["scaled_rq", "rq_x_matern", "rq_plus_rbf"])
def test_rational_quadratic_kernels(gp, name):
    """``RQKernel`` (baybe/kernels/basic.py:202-216; gpytorch: (1 + r^2 / (2 alpha))^-alpha with a learnable alpha, one theta
    slot per factor): value, lengthscale and alpha derivatives on the device against the oracle, materialised-K* posterior,
    greedy batch, device fit - alone and as a factor of a product / sum."""
    from baybe_amd import gp_spec
    from baybe_amd.kernels import AdditiveKernel, GammaPrior, MaternKernel, ProductKernel, RBFKernel, RQKernel, ScaleKernel, apply_kernel_spec
    from oracle import gp_oracle as go

    kern = {"scaled_rq": ScaleKernel(RQKernel(GammaPrior(3.0, 1.0), 0.8), GammaPrior(2.0, 0.5)),
            "rq_x_matern": ProductKernel([RQKernel(None, 1.2), ScaleKernel(MaternKernel(2.5))]),
            "rq_plus_rbf": AdditiveKernel([ScaleKernel(RQKernel()), ScaleKernel(RBFKernel(GammaPrior(3.0, 2.0)))])}[name]
    d = 5
    X, Xt, y = make_problem(2000, d, 60, seed=50)
    spec = apply_kernel_spec(gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d)), kern)
    assert spec.has_rq
    ospec = _ospec(spec)
    rng = np.random.default_rng(3)
    p = gp_spec.initial_params(spec)
    p.lengthscale = p.lengthscale * (0.6 + 0.8 * rng.random(d))
    p.alpha = np.where(np.array(spec.factor_kinds) == "rq", 0.4 + 2.0 * rng.random(len(p.alpha)), 1.0)
    p.noise, p.mean = 0.03, 0.05
    gp.set_model(spec, Xt, y)
    val, g = gp.data_term(p)
    Xn, ys = go.normalize_inputs(ospec, Xt), go.standardize_targets(y)[0]
    dt = go.data_term(ospec, _oparams(p), Xn, ys)
    if spec.factors:
        gref = np.concatenate([[dt.g_noise, dt.g_mean, dt.g_outputscale]] + dt.g_member_ls + [dt.g_member_scale, dt.g_alpha])
    else:
        gref = np.concatenate([[dt.g_noise, dt.g_mean, dt.g_outputscale], dt.g_ls, dt.g_alpha])
    assert len(g) == len(gref)
    assert math.isclose(val, dt.value, rel_tol=1e-11)
    assert np.allclose(g, gref, rtol=1e-9, atol=1e-10 * np.abs(gref).max())
    gp.factorize(p)
    om = go.GPModel(ospec, _oparams(p), Xt, y)
    mo, vo = om.posterior(X)
    for unfused in (False, True):
        m, v = gp.posterior(X, unfused=unfused)
        assert np.allclose(_np(m), mo, rtol=MEAN_RTOL, atol=1e-12) and np.allclose(_np(v), vo, rtol=VAR_RTOL, atol=1e-14)
    cand = np.ascontiguousarray(X[:600])
    res = gp.greedy_qlogei(cand, 3, seed=9)
    ref = go.optimize_acqf_discrete_qlogei(om, cand, 3, seed=9)
    assert list(res.indices) == list(ref.indices) and np.allclose(res.values, ref.values, rtol=0, atol=SCORE_ATOL)
    if name == "scaled_rq":
        fi = gp.fit()
        fo = go.fit_hyperparameters(ospec, Xn, ys)
        assert math.isclose(fi.fun, fo.fun, rel_tol=2e-5)  # alpha against the lengthscales: a shallow valley
        m, v = gp.posterior(X)
        mf, vf = go.GPModel(ospec, fo.params, Xt, y).posterior(X)
        assert np.max(np.abs(_np(m) - mf)) < 0.02 * np.std(y)


def test_tile_dataflow_factorisation_and_its_fallback(monkeypatch):
    """The one-launch tile-dataflow Cholesky + inverse (bbh_potrf_tiles_kernel, np <= 1024) against the per-step launches
    (BBH_POTRF_TILES=0): same data term / gradient / posterior to rounding; and with a poll budget of zero the waiting tiles
    give up at once, the launch reports -7 and the handle falls back to the per-step path with the same results."""
    from baybe_amd import engine, gp_spec

    d, n = 8, 300
    X, Xt, y = make_problem(3000, d, n, seed=61)
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    ls, nz, _ = fixed_theta(d)
    p = gp_spec.GPParams(np.full(d, ls), nz, 0.1)
    out = {}
    for mode, env in (("tiles", {"BBH_POTRF_TILES": "1"}), ("steps", {"BBH_POTRF_TILES": "0"}),
                      ("fallback", {"BBH_POTRF_TILES": "1", "BBH_TILE_SPIN": "0"})):
        for k in ("BBH_POTRF_TILES", "BBH_TILE_SPIN"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g = engine.HipGP(0)
        g.set_model(spec, Xt, y)
        val, grad = g.data_term(p)
        g.factorize(p)
        m, v = g.posterior(X)
        out[mode] = (val, grad, m.cpu().numpy(), v.cpu().numpy())
        g.close()
    for mode in ("steps", "fallback"):
        assert math.isclose(out["tiles"][0], out[mode][0], rel_tol=1e-12)
        assert np.allclose(out["tiles"][1], out[mode][1], rtol=1e-9, atol=1e-11 * np.abs(out["tiles"][1]).max())
        assert np.allclose(out["tiles"][2], out[mode][2], rtol=1e-10, atol=1e-12) and np.allclose(out["tiles"][3], out[mode][3], rtol=1e-8)
    assert out["steps"][0] == out["fallback"][0]  # the fallback IS the per-step path


def test_fit_through_the_captured_graph_matches_the_launch_path(monkeypatch):
    """BBH_FIT_GRAPH=1 replays one captured evaluation per objective call (the tile-dataflow factorisation took its
    epoch as a by-value kernel argument, so from the second replay on every wait passed at once).  The captured evaluation
    now uses the per-step launches; value, gradient at several points and the whole fit must equal the launch path."""
    from baybe_amd import engine, gp_spec

    d, n = 6, 200
    X, Xt, y = make_problem(2000, d, n, seed=77)
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    ls, nz, _ = fixed_theta(d)
    points = [gp_spec.GPParams(np.full(d, ls * f), nz * f, 0.05 * f) for f in (1.0, 0.7, 1.4, 0.9)]
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("BBH_FIT_GRAPH", mode)
        g = engine.HipGP(0)
        g.set_model(spec, Xt, y)
        evals = [g.data_term(p) for p in points]  # the graph is replayed from the second evaluation on
        fi = g.fit()
        out[mode] = (evals, fi)
        g.close()
    for (v0, g0), (v1, g1) in zip(out["0"][0], out["1"][0]):
        assert math.isclose(v0, v1, rel_tol=1e-11)
        assert np.allclose(g0, g1, rtol=1e-8, atol=1e-10 * np.abs(g0).max())
    assert math.isclose(out["0"][1].fun, out["1"][1].fun, rel_tol=1e-8)
    assert np.allclose(out["0"][1].params.lengthscale, out["1"][1].params.lengthscale, rtol=1e-4)


def test_small_model_evaluation_in_one_workgroup_matches_the_launch_path(monkeypatch):
    """np = 64 (n <= 64), one task, one kernel, MLL: ``bbh_fit_small_kernel`` does a whole objective evaluation - Gram matrix,
    factorisation and inverse, alpha, K^-1, value, every gradient slot - in one workgroup (``BBH_FIT_SMALL=0``: launch by launch).
    Value and gradient at several points for every kernel kind the fused kernel accepts (incl. the alpha slot of RQ / Polynomial,
    the weights of Linear, pinned slots of a subset), a failed factorisation, the whole fit against the launch path and against the
    oracle; models it does not accept (two factors, n > 64) are unaffected."""
    import time

    from _problems import oracle_params
    from baybe_amd import engine, gp_spec
    from baybe_amd.kernels import (GammaPrior, LinearKernel, MaternKernel, PiecewisePolynomialKernel, PolynomialKernel, ProductKernel,
                                   RBFKernel, RQKernel, ScaleKernel, apply_kernel_spec)
    from oracle import gp_oracle as go

    class Space:
        comp_rep_columns = tuple(f"x{j}" for j in range(8))

    rng = np.random.default_rng(3)
    cases = [(None, 3, 20), (None, 8, 64), (ScaleKernel(RBFKernel(GammaPrior(3, 1)), GammaPrior(2, 0.5)), 8, 50),
             (RQKernel(GammaPrior(3, 1)), 4, 33), (ScaleKernel(LinearKernel(GammaPrior(2, 1))), 4, 40), (PolynomialKernel(2, GammaPrior(2, 2)), 5, 45),
             (PiecewisePolynomialKernel(2, GammaPrior(3, 1)), 3, 30), (MaternKernel(0.5, GammaPrior(3, 1)), 3, 25),
             (ScaleKernel(MaternKernel(1.5, GammaPrior(3, 1), parameter_names=["x0", "x2", "x3"])), 5, 37)]
    for kern, d, n in cases:
        X, Xt, y = make_problem(500, d, n, seed=100 + n)
        spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
        if kern is not None:
            apply_kernel_spec(spec, kern, Space())
        bounds = gp_spec.raw_bounds(spec)
        free = np.array([not (b[0] is not None and b[0] == b[1]) for b in bounds])
        raw0 = gp_spec.pack_raw(spec, gp_spec.initial_params(spec))
        points = []
        for _ in range(3):
            raw = np.where(free, raw0 + 0.3 * rng.standard_normal(raw0.shape), raw0)
            raw[0] = abs(raw[0]) + 0.01
            points.append(gp_spec.unpack_raw(spec, raw))
        out = {}
        for mode in ("0", "1"):
            monkeypatch.setenv("BBH_FIT_SMALL", mode)
            g = engine.HipGP(0)
            g.set_model(spec, Xt, y)
            evals = [g.data_term(p) for p in points]
            t0 = time.perf_counter()
            fi = g.fit()
            out[mode] = (evals, fi, (time.perf_counter() - t0) * 1e3)
            m_, v_ = g.posterior(X)  # the posterior path is untouched by the switch
            out[mode] += (m_.cpu().numpy(), v_.cpu().numpy())
            g.close()
        for (v0, g0), (v1, g1) in zip(out["0"][0], out["1"][0]):
            assert math.isclose(v0, v1, rel_tol=1e-11, abs_tol=1e-11), (kern, v0, v1)
            assert np.allclose(g0, g1, rtol=1e-8, atol=1e-10 * np.abs(g0).max()), (kern, g0, g1)
        f0, f1 = out["0"][1], out["1"][1]
        assert abs(f0.fun - f1.fun) <= 2e-6 * max(1.0, abs(f0.fun)), (kern, f0.fun, f1.fun)
        ospec = _ospec(spec)
        Xn, ys = go.normalize_inputs(ospec, Xt), go.standardize_targets(y)[0]
        f_at, _ = go.fit_objective(ospec, go.pack_raw(ospec, oracle_params(spec, f1.params)), Xn, ys)
        assert math.isclose(f_at, f1.fun, rel_tol=1e-9, abs_tol=1e-11), (kern, f_at, f1.fun)
        print(f"   {type(kern).__name__ if kern is not None else 'BAYBE preset'} d={d} n={n}: fit launch by launch {out['0'][2]:.2f} ms ({f0.nfev} evaluations), "
              f"one workgroup {out['1'][2]:.2f} ms ({f1.nfev})")
    # not positive definite: the flag comes back through the same channel (zero noise, duplicated rows)
    monkeypatch.setenv("BBH_FIT_SMALL", "1")
    X, Xt, y = make_problem(300, 3, 20, seed=5)
    Xt[1] = Xt[0]
    spec = gp_spec.GPSpec.baybe_default(3, np.zeros(3), np.ones(3))
    g = engine.HipGP(0)
    g.set_model(spec, Xt, y)
    assert g.data_term(gp_spec.GPParams(np.full(3, 1.0), 0.0, 0.0)) == (None, None)
    fi = g.fit()  # the fit itself survives (the objective reports +inf there)
    assert np.isfinite(fi.fun)
    g.close()


@pytest.mark.parametrize("which", ["single", "product", "sum_icm"])
def test_kernels_on_parameter_subsets(gp, which):
    """``BasicKernel.parameter_names`` (baybe/kernels/base.py:198-240; gpytorch ``active_dims``): kernels acting on a subset of the
    parameters - alone, as factors of a ``ProductKernel`` on (overlapping) subsets, and under the ICM task factor.  The device
    kernels know nothing about subsets: a column a kernel does not act on gets the pinned lengthscale ``INACTIVE_LS``; the
    oracle drops the column (a lengthscale of ``len(active_dims)`` entries, as gpytorch).  Checked: the fit objective and its
    gradient against the oracle's autograd objective (active slots; zero in the pinned ones), the whole fit, the posterior
    (fused and unfused paths) and a greedy batch."""
    from _problems import oracle_params
    from baybe_amd import gp_spec
    from baybe_amd.kernels import AdditiveKernel, GammaPrior, MaternKernel, ProductKernel, RBFKernel, ScaleKernel, apply_kernel_spec
    from oracle import gp_oracle as go

    d = 5

    class Space:
        comp_rep_columns = tuple(f"x{j}" for j in range(d)) + (("task",) if which == "sum_icm" else ())

    if which == "sum_icm":
        X, Xt, y = make_tl_problem(2500, d, 24, T=3, seed=33)
        spec = gp_spec.GPSpec.baybe_default(d + 1, np.zeros(d + 1), np.ones(d + 1), task_idx=d, n_tasks=3)
        kern = AdditiveKernel([ScaleKernel(MaternKernel(2.5, GammaPrior(3, 1), parameter_names=["x0", "x1", "x2"]), GammaPrior(2, 0.5)),
                               ScaleKernel(RBFKernel(GammaPrior(3, 1), parameter_names=["x3", "x4"]), GammaPrior(2, 0.5))])
    else:
        X, Xt, y = make_problem(2500, d, 60, seed=33)
        spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
        kern = (ScaleKernel(MaternKernel(2.5, GammaPrior(3, 1), parameter_names=["x1", "x3", "x4"]), GammaPrior(2, 0.5)) if which == "single"
                else ProductKernel([MaternKernel(2.5, GammaPrior(3, 1), parameter_names=["x0", "x1"]),
                                    ScaleKernel(RBFKernel(GammaPrior(2, 1), parameter_names=["x1", "x2", "x3", "x4"]), GammaPrior(2, 0.5))]))
    apply_kernel_spec(spec, kern, Space())
    assert spec.has_subsets
    ospec = _ospec(spec)
    gp.set_model(spec, Xt, y)
    Xn, ys = go.normalize_inputs(ospec, Xt), go.standardize_targets(y)[0]
    rng = np.random.default_rng(4)
    p = gp_spec.initial_params(spec)
    for k in range(spec.n_factors):  # perturb the active lengthscales only; the pinned ones stay pinned
        arr = p.lengthscale if k == 0 else p.factor_ls[k - 1]
        m = spec.active_mask(k)
        arr[m] *= 0.6 + 0.8 * rng.random(int(m.sum()))
    p.noise = 0.02
    raw = gp_spec.pack_raw(spec, p)
    val, g_theta = gp.data_term(p)
    f_dev, g_dev = gp_spec.objective_from_data_term(spec, raw, len(y), val, g_theta)
    raw_o = go.pack_raw(ospec, oracle_params(spec, p))
    f_orc, g_orc = go.fit_objective(ospec, raw_o, Xn, ys)
    bounds = gp_spec.raw_bounds(spec)
    free = np.array([not (b[0] is not None and b[0] == b[1]) for b in bounds])
    assert free.sum() == len(raw_o) and (g_dev[~free] == 0.0).all()
    assert math.isclose(f_dev, f_orc, rel_tol=1e-10)
    assert np.allclose(g_dev[free], g_orc, rtol=1e-7, atol=1e-9 * np.abs(g_orc).max())
    # the whole fit (ICM case: the LOO surface of the task covariance is flat - two complete runs stop ~1e-5 apart after > 1000
    # evaluations, see test_device_fit_reaches_the_oracle_optimum_at_n1024_icm - so there a capped device fit is checked through the
    # oracle's objective at its end point)
    if which == "sum_icm":
        fi = gp.fit(maxiter=80)
        f_at, _ = go.fit_objective(ospec, go.pack_raw(ospec, oracle_params(spec, fi.params)), Xn, ys)
        assert math.isclose(f_at, fi.fun, rel_tol=1e-9, abs_tol=1e-11) and fi.fun < f_dev
    else:
        fi = gp.fit()
        fo = go.fit_hyperparameters(ospec, Xn, ys)
        assert abs(fi.fun - fo.fun) <= 2e-5 * max(1.0, abs(fo.fun)), (fi.fun, fo.fun)
    for k in range(spec.n_factors):
        arr = fi.params.lengthscale if k == 0 else fi.params.factor_ls[k - 1]
        assert (arr[~spec.active_mask(k)] == gp_spec.INACTIVE_LS).all()
    # posterior and a greedy batch at the device's optimum, against the oracle's model at the same hyper-parameters
    om = go.GPModel(ospec, oracle_params(spec, fi.params), Xt, y)
    mo, vo = om.posterior(X)
    for unfused in (False, True):
        m_, v_ = gp.posterior(X, unfused=unfused)
        assert np.allclose(_np(m_), mo, rtol=MEAN_RTOL, atol=1e-12) and np.allclose(_np(v_), vo, rtol=VAR_RTOL, atol=1e-14)
    cand = np.ascontiguousarray(X[:800])
    res = gp.greedy_qlogei(cand, 3, seed=12)
    ref = go.optimize_acqf_discrete_qlogei(om, cand, 3, seed=12)
    assert list(res.indices) == list(ref.indices) and np.allclose(res.values, ref.values, rtol=0, atol=SCORE_ATOL)


@pytest.mark.parametrize("which", ["linear", "poly", "sum", "product_subsets", "periodic", "periodic_sum_subsets"])
def test_linear_polynomial_and_periodic_kernels(gp, which):
    """``LinearKernel`` / ``PolynomialKernel`` (baybe/kernels/basic.py:20-46, 135-163; the reference iterates them alone and in sums,
    tests/test_iterations.py:277-295).  On the device they are functions of s = sum_j x_j x'_j / w_j^2 (BBH_KERNEL_LINEAR ..): the
    Linear kernel's ARD variances are v_j = w_j^-2, the Polynomial kernel's weights are pinned to 1 and its offset sits in the alpha
    slot; k(x, x) varies per candidate, so the posterior goes through the materialised-K* path with a per-candidate prior variance.
    ``PeriodicKernel`` (basic.py:73-112): exp(-2 sum_j sin^2(pi Delta_j / p_j) / l_j), period lengths in a block at the end of theta.
    Checked against the oracle (gpytorch's own parameterisation): fit objective + gradient, the whole fit, posterior, greedy batch."""
    from _problems import oracle_params
    from baybe_amd import gp_spec
    from baybe_amd.kernels import (AdditiveKernel, GammaPrior, LinearKernel, LogNormalPrior, MaternKernel, PeriodicKernel, PolynomialKernel,
                                   ProductKernel, RBFKernel, ScaleKernel, apply_kernel_spec)
    from oracle import gp_oracle as go

    d = 4

    class Space:
        comp_rep_columns = tuple(f"x{j}" for j in range(d))

    X, Xt, y = make_problem(2500, d, 50, seed=57)
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    kern = {"linear": ScaleKernel(LinearKernel(GammaPrior(2, 1)), GammaPrior(2, 0.5)),
            "poly": PolynomialKernel(2, GammaPrior(2, 2)),
            "sum": AdditiveKernel([RBFKernel(GammaPrior(3, 1)), ScaleKernel(LinearKernel(GammaPrior(3, 2))), PolynomialKernel(1, GammaPrior(2, 1))]),
            "periodic": ScaleKernel(PeriodicKernel(GammaPrior(3, 2), 1.0, LogNormalPrior(0.3, 0.4), 1.5), GammaPrior(2, 0.5)),
            "periodic_sum_subsets": AdditiveKernel([ScaleKernel(PeriodicKernel(GammaPrior(3, 2), None, GammaPrior(4, 3), 1.2, parameter_names=["x0", "x2"])),
                                                    ScaleKernel(MaternKernel(2.5, GammaPrior(3, 1), parameter_names=["x1", "x2", "x3"]))]),
            "product_subsets": ProductKernel([MaternKernel(2.5, GammaPrior(3, 1), parameter_names=["x0", "x1"]),
                                              ScaleKernel(PolynomialKernel(3, GammaPrior(2, 1), 1.5, parameter_names=["x1", "x2", "x3"]))])}[which]
    apply_kernel_spec(spec, kern, Space())
    ospec = _ospec(spec)
    gp.set_model(spec, Xt, y)
    Xn, ys = go.normalize_inputs(ospec, Xt), go.standardize_targets(y)[0]
    rng = np.random.default_rng(9)
    bounds = gp_spec.raw_bounds(spec)
    free = np.array([not (b[0] is not None and b[0] == b[1]) for b in bounds])
    raw = gp_spec.pack_raw(spec, gp_spec.initial_params(spec))
    raw = np.where(free, raw + 0.3 * rng.standard_normal(raw.shape), raw)
    raw[0] = 0.03
    p = gp_spec.unpack_raw(spec, raw)
    val, g_theta = gp.data_term(p)
    f_dev, g_dev = gp_spec.objective_from_data_term(spec, raw, len(y), val, g_theta)
    raw_o = go.pack_raw(ospec, oracle_params(spec, p))
    assert np.allclose(raw_o, raw[free], rtol=1e-12, atol=1e-12)
    f_orc, g_orc = go.fit_objective(ospec, raw_o, Xn, ys)
    assert math.isclose(f_dev, f_orc, rel_tol=1e-10), (f_dev, f_orc)
    assert np.allclose(g_dev[free], g_orc, rtol=1e-7, atol=1e-9 * np.abs(g_orc).max()), (g_dev[free], g_orc)
    assert (g_dev[~free] == 0.0).all()
    fi = gp.fit()
    fo = go.fit_hyperparameters(ospec, Xn, ys)
    assert abs(fi.fun - fo.fun) <= 2e-5 * max(1.0, abs(fo.fun)), (fi.fun, fo.fun)
    om = go.GPModel(ospec, oracle_params(spec, fi.params), Xt, y)
    mo, vo = om.posterior(X)
    m_, v_ = gp.posterior(X)
    # fused: the cooperative form with the generic production - dot products / the cos-sin expansion of the periodic metric through
    # the same MFMA as the distances (csrc/bbh_coopg.h); the materialised-K* path stays as the second opinion
    assert gp.posterior_kernel_form() == "cooperative-generic"
    assert np.allclose(_np(m_), mo, rtol=MEAN_RTOL, atol=1e-12) and np.allclose(_np(v_), vo, rtol=VAR_RTOL, atol=1e-13)
    mu_, vu_ = gp.posterior(X, unfused=True)
    assert np.allclose(_np(mu_), mo, rtol=MEAN_RTOL, atol=1e-12) and np.allclose(_np(vu_), vo, rtol=VAR_RTOL, atol=1e-13)
    if spec.has_dot_kind:
        assert np.ptp(go.prior_var(ospec, oracle_params(spec, fi.params), go.normalize_inputs(ospec, X))) > 0  # k(x, x) is not constant
    cand = np.ascontiguousarray(X[:800])
    res = gp.greedy_qlogei(cand, 3, seed=12)
    ref = go.optimize_acqf_discrete_qlogei(om, cand, 3, seed=12)
    assert list(res.indices) == list(ref.indices) and np.allclose(res.values, ref.values, rtol=0, atol=SCORE_ATOL)
    # the cross-covariance columns of steps >= 2 (bbh_coopg_cross_kernel: same feature maps, pending points in block nb) vs the oracle
    P = cand[[3, 410]]
    gp.set_pending(P)
    cr = _np(gp.cross_cov(cand[:300]))
    gp.set_pending(None)
    for i in (0, 151, 299):
        _, cov = om.posterior_joint(np.vstack([cand[i:i + 1], P]))
        assert np.allclose(cr[i], cov[0, 1:], rtol=1e-7, atol=1e-11), (i, cr[i], cov[0, 1:])
    from _pending_cases import batched_cross  # every row (the batched form is pinned to posterior_joint in test_pending_cases_cpu.py)

    assert np.allclose(cr, batched_cross(om, cand[:300], P), rtol=1e-7, atol=1e-11)


def test_joint_batches_beyond_sixteen_points(gp):
    """``optimize_acqf_discrete`` has no cap on batch_size + pending experiments (botorch/discrete.py:120-126); the register / LDS
    kernels hold 16 points.  Beyond that ``bbh_qlogei_pending_big`` keeps the per-candidate Cholesky factors in a global
    workspace: a greedy batch of 19 with 3 pending experiments (q' up to 22) must be the oracle's, step by step - including the
    steps on either side of the hand-over at 16 points - and the recommender accepts the batch."""
    from baybe_amd import gp_spec
    from oracle import gp_oracle as go

    d, n, N, q = 4, 30, 500, 19
    X, Xt, y = make_problem(N + 3, d, n, seed=71)
    pend, X = X[N:], np.ascontiguousarray(X[:N])
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    gp.set_model(spec, Xt, y)
    fi = gp.fit()
    om = go.GPModel(_ospec(spec), _oparams(fi.params), Xt, y)
    res = gp.greedy_qlogei(X, q, S=128, seed=21, X_pending=pend)
    ref = go.optimize_acqf_discrete_qlogei(om, X, q, S=128, seed=21, X_pending=pend)
    assert list(res.indices) == list(ref.indices), (res.indices, ref.indices)
    assert np.allclose(res.values, ref.values, rtol=0, atol=SCORE_ATOL), np.abs(np.array(res.values) - np.array(ref.values)).max()
    assert len(set(res.indices)) == q
    # the many-point cross-covariance helper: columns are independent of the chunking
    P = X[res.indices[:17]]
    many = _np(gp.cross_cov_many(X, P))
    gp.set_pending(P[:15]); first = _np(gp.cross_cov(X))
    gp.set_pending(P[15:]); rest = _np(gp.cross_cov(X))
    gp.set_pending(None)
    assert np.array_equal(many, np.hstack([first, rest]))
    # the factor workspace is bounded (16 GB at 1e6 candidates and q' = 64): candidates go through it in chunks, and the
    # scores do not depend on the chunking (BBH_QBIG_WS_MB=1: 512-row chunks at q' = 22, masked rows and the ragged last chunk included)
    import torch

    from baybe_amd import engine

    rng = np.random.default_rng(5)
    Xl = np.ascontiguousarray(rng.random((3003, d)))
    P21 = X[res.indices[:18]].tolist() + pend.tolist()
    P21 = np.asarray(P21)
    z = engine.sobol_normal_base_samples(64, len(P21) + 1, 3)
    m, v = gp.posterior(Xl)
    cr = gp.cross_cov_many(Xl, P21)
    alive = torch.from_numpy((rng.random(3003) > 0.1).astype(np.uint8)).to(m.device)
    stats, best_f = gp.posterior_joint(P21), gp.best_f(1.0)
    one = _np(gp.qlogei_pending_big(m, v, cr, P21, z, best_f, alive=alive, stats=stats))
    # (a handle reads its switches when it is created: the many-chunk run is a second handle's, on the same model, theta and inputs)
    os.environ["BBH_QBIG_WS_MB"] = "1"
    try:
        g2 = engine.HipGP(0)
    finally:
        del os.environ["BBH_QBIG_WS_MB"]
    try:
        g2.set_model(spec, Xt, y)
        g2.factorize(fi.params)
        many_chunks = _np(g2.qlogei_pending_big(m, v, cr, P21, z, best_f, alive=alive, stats=stats))
    finally:
        g2.close()
    assert np.array_equal(one, many_chunks) and np.isfinite(one[_np(alive).astype(bool)]).all() and np.isneginf(one[~_np(alive).astype(bool)]).all()
    with pytest.raises(ValueError):
        gp.greedy_qlogei(X, 5, S=64, seed=1, X_pending=X[:62])  # 62 + 4 picks > 63 pending points
    with pytest.raises(ValueError):
        gp.greedy_qlogei(X, 18, S=64, seed=1, kind="qEI")  # the other MC functions stop at 16 points


def test_fit_evaluation_in_one_launch_matches_the_launch_path(monkeypatch):
    """64 < np <= 1024, one kernel, <= 4 tasks: ``bbh_fit_flow_kernel`` does everything after the factorisation - K^-1, alpha, value,
    every gradient slot - as one dataflow launch that writes into the pinned result buffers (``BBH_FIT_FLOW=1``, the default), or
    the whole objective evaluation incl. Gram tiles, factor and inverse (``BBH_FIT_FLOW=2``); ``BBH_FIT_FLOW=0``: launch by launch.  Value 1e-11 / gradient 1e-8 between the two at several points for MLL models of n = 70 ... 1024 (incl. sizes that are
    not multiples of 64, the alpha slot of RQ, Matern-1/2, a pinned subset), ICM models with the leave-one-out criterion (the
    configs[3] model) and with the marginal likelihood; a failed factorisation; whole fits end at the same objective value;
    models the form does not take (two factors) are unaffected."""
    import time

    from _problems import make_tl_problem
    from baybe_amd import engine, gp_spec
    from baybe_amd.kernels import GammaPrior, MaternKernel, ProductKernel, RBFKernel, RQKernel, ScaleKernel, apply_kernel_spec

    class Space:
        comp_rep_columns = tuple(f"x{j}" for j in range(20))

    rng = np.random.default_rng(11)
    cases = [("preset", None, 6, 70, 1), ("preset", None, 20, 512, 1), ("preset", None, 15, 300, 1), ("preset", None, 20, 1024, 1),
             ("rbf", ScaleKernel(RBFKernel(GammaPrior(3, 1)), GammaPrior(2, 0.5)), 8, 130, 1), ("rq", RQKernel(GammaPrior(3, 1)), 4, 200, 1),
             ("m12", MaternKernel(0.5, GammaPrior(3, 1)), 3, 100, 1),
             ("subset", ScaleKernel(MaternKernel(1.5, GammaPrior(3, 1), parameter_names=["x0", "x2", "x3"])), 5, 150, 1),
             ("icm-loo", None, 15, 256, 4), ("icm-loo", None, 15, 1024, 4), ("icm-mll", None, 6, 200, 3),
             # round 6: 1024 < np <= 2048 - the one-launch form is the default there (its ticketed roles need no co-residency; the
             # tile-dataflow factorisation of the two-launch form ends at 16 block rows), configs[3] one batch of measurements later
             ("preset", None, 20, 1088, 1), ("preset", None, 12, 1500, 1), ("icm-loo", None, 15, 1040, 4), ("preset", None, 8, 2048, 1)]
    for tag, kern, d, n, T in cases:
        if T == 1:
            X, Xt, y = make_problem(4096, d, n, seed=100 + n)
            spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
        else:
            X, Xt, y = make_tl_problem(500, d, n // T, T, seed=n)
            spec = gp_spec.GPSpec.baybe_default(d + 1, np.zeros(d + 1), np.ones(d + 1), task_idx=d, n_tasks=T)
            if tag == "icm-mll":
                spec.criterion = "mll"
        if kern is not None:
            apply_kernel_spec(spec, kern, Space())
        bounds = gp_spec.raw_bounds(spec)
        free = np.array([not (b[0] is not None and b[0] == b[1]) for b in bounds])
        raw0 = gp_spec.pack_raw(spec, gp_spec.initial_params(spec))
        points = []
        for _ in range(3):
            raw = np.where(free, raw0 + 0.3 * rng.standard_normal(raw0.shape), raw0)
            raw[0] = abs(raw[0]) + 0.01
            points.append(gp_spec.unpack_raw(spec, raw))
        out = {}
        # "1": Gram tiles and (n <= 832) K^-1's tiles inside the factorisation launch, theta as kernel arguments, write-through hand-offs;
        # the suffixed forms switch one of these off each; "3": the split form (factorisation + K^-1 as one ticketed launch, then the rest)
        variants = {"0": {}, "1": {}, "2": {}, "3": {}, "1-mt0": {"BBH_TILE_MT": "0"}, "1-gram0": {"BBH_TILE_GRAM": "0"},
                    "1-wt0": {"BBH_TILE_WT": "0"}, "1-copy": {"BBH_TILE_GRAM_THETA": "copy"}}
        if n > 1024:  # (forms 2 / 3 are A/B switches for np <= 1024; beyond it the default IS the one-launch form)
            variants = {"0": {}, "1": {}}
        for mode, extra in variants.items():
            monkeypatch.setenv("BBH_FIT_FLOW", mode[0])
            for k_, v_ in extra.items():
                monkeypatch.setenv(k_, v_)
            g = engine.HipGP(0)
            g.set_model(spec, Xt, y)
            evals = [g.data_term(p) for p in points]
            evals += [g.data_term(points[0])]  # (a repeated point: the epoch-stamped flags and cumulative counters carry over)
            t0 = time.perf_counter()
            for _ in range(20):
                g.data_term(points[1])
            per_eval = (time.perf_counter() - t0) / 20 * 1e3
            fi = g.fit() if n <= 512 and T == 1 else None
            out[mode] = (evals, fi, per_eval)
            g.close()
            for k_ in extra:
                monkeypatch.delenv(k_)
        for mode in [m for m in variants if m != "0"]:
            for (v0, g0), (v1, g1) in zip(out["0"][0], out[mode][0]):
                assert v0 is not None and v1 is not None
                assert math.isclose(v0, v1, rel_tol=1e-11, abs_tol=1e-11), (tag, n, mode, v0, v1)
                assert np.allclose(g0, g1, rtol=1e-8, atol=1e-10 * np.abs(g0).max()), (tag, n, mode, g0, g1)
            assert out[mode][0][0][0] == out[mode][0][3][0] and np.array_equal(out[mode][0][0][1], out[mode][0][3][1])  # reproducible
        if out["0"][1] is not None:
            f0, f1 = out["0"][1], out["1"][1]
            assert abs(f0.fun - f1.fun) <= 2e-6 * max(1.0, abs(f0.fun)), (tag, f0.fun, f1.fun)
        print(f"   {tag} d={d} n={n} T={T}: evaluation launch by launch {out['0'][2]:.3f} ms, default dataflow form {out['1'][2]:.3f} ms"
              + (f", one launch {out['2'][2]:.3f} ms" if "2" in out else ""))
        if n > 1024:
            assert out["1"][2] < 0.8 * out["0"][2], (tag, n, out["0"][2], out["1"][2])  # (it is the dataflow form that ran)
    # a poll budget of zero: the waiting roles give up at once, the launch never reports, the handle falls back to the launch path
    for mode in ("1", "2", "3"):
        monkeypatch.setenv("BBH_FIT_FLOW", mode)
        monkeypatch.setenv("BBH_FLOW_SPIN", "0")
        X, Xt, y = make_problem(4096, 6, 200, seed=8)
        spec = gp_spec.GPSpec.baybe_default(6, np.zeros(6), np.ones(6))
        g = engine.HipGP(0)
        g.set_model(spec, Xt, y)
        p0 = gp_spec.initial_params(spec)
        va, ga_ = g.data_term(p0)
        monkeypatch.setenv("BBH_FIT_FLOW", "0")
        monkeypatch.delenv("BBH_FLOW_SPIN")
        g0 = engine.HipGP(0)
        g0.set_model(spec, Xt, y)
        vb, gb_ = g0.data_term(p0)
        assert va == vb and np.array_equal(ga_, gb_)  # (after the give-up it IS the launch path)
        g.close()
        g0.close()
    monkeypatch.delenv("BBH_FLOW_SPIN", raising=False)
    # not positive definite (a negative noise variance: the first pivots fail): the flag comes back through the same channel
    for mode in ("1", "2", "3"):
        monkeypatch.setenv("BBH_FIT_FLOW", mode)
        X, Xt, y = make_problem(600, 3, 100, seed=5)
        spec = gp_spec.GPSpec.baybe_default(3, np.zeros(3), np.ones(3))
        g = engine.HipGP(0)
        g.set_model(spec, Xt, y)
        assert g.data_term(gp_spec.GPParams(np.full(3, 1.0), -2.0, 0.0)) == (None, None)
        v, gr = g.data_term(gp_spec.GPParams(np.full(3, 1.0), 0.1, 0.0))  # ... and the next evaluation is clean
        assert v is not None and np.isfinite(v) and np.isfinite(gr).all()
        g.close()
