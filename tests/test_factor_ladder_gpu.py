"""The failure flag of the train-covariance factorisation and the jitter ladder of ``bbh_factorize`` against the oracle (cases,
references and the scaled metric: tests/_factor_cases.py; their CPU guard: tests/test_factor_cases_cpu.py).

Five kernels write ``info = 64 J + j + 1`` at the first non-positive pivot.  Which test reaches a failing pivot behind the first
rows in which of them:

  bbh_potrf_tiles_kernel     test_factorize_takes_the_reference_level / test_exhausted_ladder on the "default" handle up to n = 200
                             (<false, *>: the Gram matrix is built by a launch in front); test_fit_evaluation_flag under "1"
                             (<true, *>: builds its own Gram tiles), "1-gram0" and "0" at n = 70, 200
  bbh_potrf_diag16_kernel    (pd_factor_block4) the "steps" handle at every size, every handle at n = 1030 (17 block rows: per-step
                             launches by itself); the fit evaluation under "1-steps" at n = 70, 200 and under "0" at n = 1030
  bbh_potrf_diag_kernel      the "reg" handle (BBH_POTRF_TILES=0 BBH_POTRF_REG=1: the one-wave register form) at every size; the fit
                             evaluation under "reg" at n = 70, 200
  bbh_fit_small_kernel       (pd_factor_block) the fit evaluation under "small1" at n = 64: b = 1, 15, 16, 17, 63
  bbh_fitflow.hip            (the ticketed one-launch form) the fit evaluation under "2" and "3" at n = 70, 200 and under "1" at n = 1030

``HipGP.factorization_form()`` / ``fit_evaluation_form()`` say which path produced the numbers; every case asserts the path its handle
was built for, so that a silent give-up of a dataflow launch cannot let three handles test one kernel.

The flag itself never leaves the library: it shows as the branch the ladder takes for masked models (``jitter`` = j_k against
j_k / ysd^2 = 16 j_k), as the level where a NaN from the failed attempt survives, and as ``data_term`` returning (None, None)."""

import os

import numpy as np
import pytest

import _factor_cases as fc
from _factor_cases import EXHAUSTED, TOL
from _fit_cases import VARIANTS as FIT_SWITCHES

pytestmark = pytest.mark.gpu

# a handle reads the BBH_* switches when it is created
FACTOR_SWITCHES = {"default": {}, "steps": {"BBH_POTRF_TILES": "0"}, "reg": {"BBH_POTRF_TILES": "0", "BBH_POTRF_REG": "1"}}
SWITCH_SETS = {**{f"fit:{k}": v for k, v in FIT_SWITCHES.items()}, "fit:reg": FACTOR_SWITCHES["reg"], **FACTOR_SWITCHES}
SWITCH_NAMES = sorted({k for v in SWITCH_SETS.values() for k in v})


@pytest.fixture(scope="module")
def handles():
    """``get(name, second=False)``: the handle of a switch set, created on first use; ``second``: another handle of the same set - the
    "fresh" one a handle's state is compared with."""
    from baybe_amd import engine

    made = {}

    def get(name, second=False):
        if (name, second) not in made:
            keep = {k: os.environ.get(k) for k in SWITCH_NAMES}
            try:
                for k in SWITCH_NAMES:
                    os.environ.pop(k, None)
                os.environ.update(SWITCH_SETS[name])
                made[name, second] = engine.HipGP(0)
            finally:
                for k, val in keep.items():
                    os.environ.pop(k, None) if val is None else os.environ.__setitem__(k, val)
        return made[name, second]

    yield get
    for g in made.values():
        g.close()


def _np(t):
    return t.cpu().numpy()


def _rows(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


def _set_model(g, md):
    g.set_model(md.spec, md.Xt, md.y, noise_mask=md.mask, standardization=md.standardization)


def _expected_factor_form(name, n):
    return "tiles" if name == "default" and n <= 1024 else "steps"


def _measure(g, md):
    """Everything compared with the reference, from a factorised handle."""
    cand = _rows(md.cand)
    m, v = (_np(t) for t in g.posterior(cand))
    mu, vu = (_np(t) for t in g.posterior(cand, unfused=True))
    jm, jc = g.posterior_joint(md.joint)
    return {"fused": (m, v), "unfused": (mu, vu), "joint": (jm, jc), "train": g.train_posterior_mean()}


def _deviations(ref, got):
    out = {f"fused:{k}": val for k, val in fc.deviations(ref, mean=got["fused"][0], var=got["fused"][1]).items()}
    out.update({f"unfused:{k}": val for k, val in fc.deviations(ref, mean=got["unfused"][0], var=got["unfused"][1]).items()})
    out.update(fc.deviations(ref, jmean=got["joint"][0], jcov=got["joint"][1], train=got["train"]))
    return out


def _hold(tag, devs, tol=TOL):
    from conftest import record_deviation

    for what, value in devs.items():
        print(f"{tag} {what}: observed {value:.3e} (tolerance {tol:.1e})")
    record_deviation(f"factor_ladder/{tag}", max(devs.values()), tol)
    failures = [(what, value) for what, value in devs.items() if not value <= tol]
    assert not failures, (tag, failures)


def _flat(v):
    return v if isinstance(v, tuple) else (v,)


def _same_bits(a, b):
    """Two ``_measure`` results, array by array."""
    return all(np.array_equal(x, y) for k in a for x, y in zip(_flat(a[k]), _flat(b[k])))


LADDER = [c for c in fc.ladder_cases() if c.k != EXHAUSTED]


@pytest.mark.parametrize("case", LADDER, ids=[c.id for c in LADDER])
def test_factorize_takes_the_reference_level(handles, case):
    """``jitter`` equals the reference level exactly - through both branches for masked models -, and the posterior behind it (fused
    and unfused, every candidate row; the joint block of three rows with the duplicated one; the training rows' means) holds to the
    reference at 1e-11 scaled, on the tile-dataflow launch, the per-step launches and the per-step launches with the register kernel."""
    md, ref, n = case.model.build(), case.reference(), case.model.n
    got = {}
    for name in FACTOR_SWITCHES:
        g = handles(name)
        _set_model(g, md)
        g.factorize(case.params())
        assert g.factorization_form() == _expected_factor_form(name, n), (case.id, name, g.factorization_form())
        assert g.jitter == ref.level, (case.id, name, g.jitter, ref.level)
        assert abs(g.ysd - ref.ysd) <= 1e-13 * ref.ysd, (case.id, name, g.ysd, ref.ysd)
        got[name] = _measure(g, md)
        _hold(f"{case.id}:{name}", _deviations(ref, got[name]))
    if n > 1024:  # the default handle runs the per-step launches itself there: the same kernels, the same bits
        assert _same_bits(got["default"], got["steps"]), (case.id, "default and steps handles differ at n > 1024")


EXHAUSTED_CASES = [c for c in fc.ladder_cases() if c.k == EXHAUSTED]


@pytest.mark.parametrize("case", EXHAUSTED_CASES, ids=[c.id for c in EXHAUSTED_CASES])
def test_exhausted_ladder(handles, case):
    """No level rescues the matrix: ``ModelFittingError`` with the handle's message, no posterior from the failed factorisation, and a
    following ``factorize`` at sound parameters gives the oracle's numbers and a fresh handle's bits."""
    from baybe_amd import HipError
    from baybe_amd.engine import ModelFittingError

    md, n = case.model.build(), case.model.n
    assert case.reference().level is None
    sound = fc.FactorCase(case.model, 0)
    ref = sound.reference()
    assert ref.level == 0.0
    for name in FACTOR_SWITCHES:
        g, fresh = handles(name), handles(name, second=True)
        _set_model(g, md)
        g.factorize(sound.params())  # (something to be stale: a posterior the failed factorisation must not leave reachable)
        with pytest.raises(ModelFittingError, match=r"train covariance not positive definite \(even with jitter 1e-6\)"):
            g.factorize(case.params())
        assert g.factorization_form() == _expected_factor_form(name, n), (case.id, name, g.factorization_form())
        with pytest.raises(HipError, match="before bbh_factorize"):
            g.posterior(_rows(md.cand))
        with pytest.raises(HipError, match="not factorised"):
            g.train_posterior_mean()
        g.factorize(sound.params())
        assert g.jitter == 0.0 and g.factorization_form() == _expected_factor_form(name, n), (case.id, name, g.jitter)
        got = _measure(g, md)
        _hold(f"{case.id}:{name}:after", _deviations(ref, got))
        _set_model(fresh, md)
        fresh.factorize(sound.params())
        assert _same_bits(got, _measure(fresh, md)), (case.id, name, "differs from a fresh handle after the exhausted ladder")


FIT_MODELS = fc.PLAIN_MODELS
_FIT_REFS: dict = {}


def _fit_reference(model):
    """The oracle's data term at the sound point of the model, once."""
    if model not in _FIT_REFS:
        from _fit_cases import FitCase, oracle_inputs, oracle_reference

        md = model.build()
        ospec, Xn, ys = oracle_inputs(md.spec, md.Xt, md.y)
        p = fc.fit_point(model)
        _FIT_REFS[model] = (p, oracle_reference(FitCase("factor", model.n, d=model.d), md.spec, p, ospec, Xn, ys))
    return _FIT_REFS[model]


@pytest.mark.parametrize("model", FIT_MODELS, ids=[m.id for m in FIT_MODELS])
def test_fit_evaluation_flag(handles, model):
    """``data_term`` is (None, None) exactly where the jitter-free Cholesky fails (noise -0.3e-8: the pivot of row b) and a number at
    +0.7e-8, under every form of the evaluation reachable at the size; the evaluation behind a failed one, at a sound point, meets
    the oracle at the fit tests' tolerances and has a fresh handle's bits (the flag a late failure left behind is reset)."""
    from _fit_cases import device_in_reference_terms, mismatch

    md, n = model.build(), model.n
    base = fc.FactorCase(model, 1).params()

    def at(noise):
        from baybe_amd import gp_spec

        return gp_spec.GPParams(base.lengthscale, noise, base.mean)

    p_sound, (kind, rv, rg) = _fit_reference(model)
    worst = {}
    for variant in fc.FIT_VARIANTS[n]:
        g, fresh = handles(f"fit:{variant}"), handles(f"fit:{variant}", second=True)
        forms = fc.fit_expected_form(n, variant)
        g.set_model(md.spec, md.Xt, md.y)
        where = (model.id, variant)
        for step, noise in enumerate((fc.FIT_NOISE_FAILS, fc.FIT_NOISE_HOLDS, fc.FIT_NOISE_FAILS)):
            val, grad = g.data_term(at(noise))
            assert g.fit_evaluation_form() in forms, (where, step, g.fit_evaluation_form(), sorted(forms))
            if noise < 0.0:
                assert val is None and grad is None, (where, step, "a failing pivot at row b went unreported", val)
            else:
                assert val is not None and np.isfinite(val) and np.isfinite(grad).all(), (where, step, val)
        val, grad = g.data_term(p_sound)
        assert g.fit_evaluation_form() in forms, (where, g.fit_evaluation_form())
        assert val is not None, (where, "sound point reported as not positive definite after a failed evaluation")
        dv, dg = device_in_reference_terms(kind, md.spec, p_sound, n, val, grad)
        worst[variant] = mismatch(kind, rv, rg, dv, dg)
        fresh.set_model(md.spec, md.Xt, md.y)
        fval, fgrad = fresh.data_term(p_sound)
        assert fresh.fit_evaluation_form() == g.fit_evaluation_form(), (where, fresh.fit_evaluation_form(), g.fit_evaluation_form())
        assert val == fval and np.array_equal(grad, fgrad), (where, "differs from a fresh handle", val - fval)
    _hold(f"fit/{model.id}", worst, tol=1.0)  # (deviation / tolerance of tests/_fit_cases.py: value and every gradient slot)
