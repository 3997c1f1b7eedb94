"""The variance pass of the cooperative form with the generic production against the oracle, every row:
``bbh_coopg_posterior_kernel<KD, F>`` (csrc/bbh_coopg.h) - what ``posterior()`` runs for every Product / Additive kernel of up to four
factors, RQ, piecewise polynomial, Linear, Polynomial and Periodic model with n <= 512 and no pending points.  Cases, references and the
scaled metric: tests/_generic_variance_cases.py (on tests/_pending_cases.py); the CPU guard of the cases - that the float64 oracle is
within 1e-13 of a long-double restatement in mean and variance for every one of them, and that each would notice a padding row that
contributes, a constant k(x, x) for a dot kind, a flattened grouped combine, exchanged factor scales, a dropped feature slot and far
rows taken for padding: tests/test_generic_variance_cases_cpu.py.

Every comparison with the oracle is scaled and absolute and held to 1e-11: |var - ref| / (ysd^2 k(x, x)), |mean - ref| / ysd,
|cross - ref| / (ysd^2 sqrt(k(x, x) k(p_j, p_j))).  Every observed maximum is recorded under ``generic_variance/<case id>``.

  test_every_instantiation (V1)   all 16 (F, KD), every kind, the ICM table, every first round g0 twice, 257 rows; the materialised K*
                                  (``unfused=True``) held to the same tolerance, so that a failure names the side that is wrong
  test_rounds (V2)                n = 1 ... 512 of a table model in the mixed layout and of the widest instantiation; n = 513: materialised
  test_ragged_tiles_and_layout (V3)  N = 1 ... 257 rows of a strided view, outputs into views with sentinels behind row N; the bits of
                                  the 257-row launch
  test_feature_slots (V4)         full and just-started k-steps of the metric GEMM; d = 31 / periodic d = 16: materialised
  test_far_rows (V5)              RQ at lengthscales 1e-4 and alpha 0.4, r^2 > 1e7 for nearly every pair: variance pass, materialised
                                  K*, and ``bbh_coopg_cross_kernel`` with two pending points
  test_handle_state (V6)          five loads on one handle, each the oracle's values and a fresh handle's bits"""

import numpy as np
import pytest

import _generic_variance_cases as gv
import _pending_cases as pc
from _pending_cases import TOL

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


@pytest.fixture(scope="module")
def handles():
    from baybe_amd import engine

    made = {"default": engine.HipGP(0), "fresh": engine.HipGP(0)}
    yield made
    for g in made.values():
        g.close()


def _np(t):
    return t.cpu().numpy()


def _rows(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


def _load(g, model, params=None):
    md = model.build()
    g.set_model(md.spec, md.Xt, md.y)
    g.factorize(md.params if params is None else params)
    assert abs(g.ysd - md.om.ysd) <= 1e-13 * md.om.ysd and g.jitter == 0.0, (model.id, g.ysd, md.om.ysd, g.jitter)
    return md


def _hold(case, devs):
    from conftest import record_deviation

    for what, value in devs.items():
        print(f"{case.id} {what}: observed {value:.3e} (tolerance {TOL:.1e})")
    record_deviation(f"generic_variance/{case.id}", max(devs.values()), TOL)
    failures = [(what, value) for what, value in devs.items() if not value <= TOL]
    assert not failures, (case.id, failures)


def _posterior_devs(g, case, unfused=False, tag=""):
    ref = case.reference()
    m, v = (_np(t) for t in g.posterior(_rows(case.build().cand), unfused=unfused))
    if not unfused:  # (``unfused=True`` asks for the materialised K* by name and leaves the recorded form alone)
        form, want = g.posterior_kernel_form(), pc.expected_p0_form(case.model, case.N)
        assert form == want, (case.id, tag, form, want)
    return {tag + "mean": pc.scaled_mean(m, ref), tag + "var": pc.scaled_var(v, ref)}, (m, v)


V1_CASES = gv.family_v1()


@pytest.mark.parametrize("case", V1_CASES, ids=[c.id for c in V1_CASES])
def test_every_instantiation(handles, case):
    g = handles["default"]
    _load(g, case.model)
    devs, _ = _posterior_devs(g, case)
    devs.update(_posterior_devs(g, case, unfused=True, tag="materialised:")[0])
    _hold(case, devs)


V2_CASES = gv.family_v2()


@pytest.mark.parametrize("case", V2_CASES, ids=[c.id for c in V2_CASES])
def test_rounds(handles, case):
    g = handles["default"]
    _load(g, case.model)
    _hold(case, _posterior_devs(g, case)[0])


V3_FULL = {}  # model -> the N = 257 launch
V3_CASES = gv.family_v3()


def _raw_posterior(g, wide, N, dtot):
    """``posterior(X, out=...)`` on the first N rows of a strided view, into views of buffers with 64 sentinels behind row N."""
    import torch

    bm, bv = (torch.full((N + 64,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(2))
    X = wide[:N, :dtot]
    assert N == 1 or (X.stride(0) == dtot + 3 and not X.is_contiguous())
    g.posterior(X, out=(bm[:N], bv[:N]))
    bm, bv = _np(bm), _np(bv)
    return bm[:N], bv[:N], np.concatenate([bm[N:], bv[N:]])


@pytest.mark.parametrize("case", V3_CASES, ids=[c.id for c in V3_CASES])
def test_ragged_tiles_and_layout(handles, case):
    import torch

    g, model = handles["default"], case.model
    d = gv.VarCase("V3", model, 0, pc.N_FULL).build()
    _load(g, model)
    wide = torch.full((pc.N_FULL, model.dtot + 3), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, : model.dtot] = _rows(d.cand)
    if model not in V3_FULL:
        V3_FULL[model] = _raw_posterior(g, wide, pc.N_FULL, model.dtot)[:2]
        assert g.posterior_kernel_form() == "cooperative-generic"
    m, v, tail = _raw_posterior(g, wide, case.N, model.dtot)
    assert g.posterior_kernel_form() == "cooperative-generic", (case.id, g.posterior_kernel_form())
    assert np.array_equal(tail, np.full(128, SENTINEL)), (case.id, "written behind row N", np.nonzero(tail != SENTINEL)[0][:8])
    fm, fv = V3_FULL[model]
    assert np.array_equal(m, fm[: case.N]) and np.array_equal(v, fv[: case.N]), (case.id, np.abs(m - fm[: case.N]).max(),
                                                                                 np.abs(v - fv[: case.N]).max())
    ref = case.reference()
    _hold(case, {"mean": pc.scaled_mean(m, ref), "var": pc.scaled_var(v, ref)})


V4_CASES = gv.family_v4()


@pytest.mark.parametrize("case", V4_CASES, ids=[c.id for c in V4_CASES])
def test_feature_slots(handles, case):
    g = handles["default"]
    _load(g, case.model)
    _hold(case, _posterior_devs(g, case)[0])


V5_CASES = gv.family_v5()


@pytest.mark.parametrize("case", V5_CASES, ids=[c.id for c in V5_CASES])
def test_far_rows(handles, case):
    g = handles["default"]
    d, ref = case.build(), case.reference()
    _load(g, case.model)
    devs, _ = _posterior_devs(g, case)
    devs.update(_posterior_devs(g, case, unfused=True, tag="materialised:")[0])
    if case.p:
        g.set_pending(d.P)
        cr = _np(g.cross_cov(_rows(d.cand)))
        g.set_pending(None)
        assert cr.shape == (case.N, case.p)
        devs["cross"] = pc.scaled_cross(cr, ref)
    _hold(case, devs)


def test_handle_state(handles):
    """V6: a two-factor model, a four-factor model in the same buffers, a single Matérn kernel (the generic production goes away), the
    first model again, a new factorisation of it - after each step the oracle's values and the bits of a fresh handle."""
    g, fresh = handles["default"], handles["fresh"]
    first = gv.V6_STEPS[0]
    for step, model in enumerate(gv.V6_STEPS):
        case = gv.VarCase("V6", model, 0, gv.N_SMALL)
        if step == 4:  # the model of step 3 stays; only the hyper-parameters change
            g.factorize(model.build().params)
            assert abs(g.ysd - model.build().om.ysd) <= 1e-13 * g.ysd and g.jitter == 0.0
            assert np.array_equal(model.build().Xt, first.build().Xt)
        else:
            _load(g, model)
        devs, (m, v) = _posterior_devs(g, case)
        _load(fresh, model)
        _, (mf, vf) = _posterior_devs(fresh, case)
        assert np.array_equal(m, mf) and np.array_equal(v, vf), (step, case.id, np.abs(m - mf).max(), np.abs(v - vf).max())
        case = gv.VarCase("V6", model, 0, gv.N_SMALL, handle=f"step{step + 1}")
        _hold(case, devs)
