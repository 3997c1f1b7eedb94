"""Every form of one fit evaluation (value + gradient of the MLL / LOO data term) against the fp64 oracle, at the size and model
edges where ``bbh_fit_enqueue`` switches between them (case table: tests/_fit_cases.py).  The gradient is checked slot by slot:
a bug in the padding rows of the last 64-block leaves the value untouched but shows in the noise, mean and LOO slots.
``HipGP.fit_evaluation_form`` says which path produced the numbers; every case asserts the path it was built for."""

import math
import os

import numpy as np
import pytest

from _fit_cases import CASES, FORMS, VARIANTS, FitCase, device_in_reference_terms, mismatch, oracle_inputs, oracle_reference
from _problems import oracle_params

pytestmark = pytest.mark.gpu

SEEN: dict = {}  # form -> case ids that ran as it


def _handle(monkeypatch, variant):
    from baybe_amd import engine

    for k in {k for v in VARIANTS.values() for k in v}:
        monkeypatch.delenv(k, raising=False)
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    return engine.HipGP(0)


def _check_point(case, spec, p, n, val, g, ref, where):
    kind, rv, rg = ref
    assert val is not None, (where, "not positive definite on the device")
    dv, dg = device_in_reference_terms(kind, spec, p, n, val, g)
    assert len(dg) == len(rg), (where, len(dg), len(rg))
    worst = mismatch(kind, rv, rg, dv, dg)
    assert worst <= 1.0, (where, kind, "deviation / tolerance", worst, dv, rv, np.asarray(dg) - rg)
    return worst


def _check_objective(spec, p, n, val, g, ospec, Xn, ys, where):
    """Through the host's chain rules against the oracle's autograd objective (tolerances of test_cfg4_loo_data_term_and_gradient_at_n1024)."""
    from baybe_amd import gp_spec
    from oracle import gp_oracle as go

    raw = gp_spec.pack_raw(spec, p)
    f, gr = gp_spec.objective_from_data_term(spec, raw, n, val, g)
    fo, gro = go.fit_objective(ospec, go.pack_raw(ospec, oracle_params(spec, p)), Xn, ys)
    bounds = gp_spec.raw_bounds(spec)
    free = np.array([not (b[0] is not None and b[0] == b[1]) for b in bounds])
    gr = np.asarray(gr)[free]
    assert math.isclose(f, fo, rel_tol=1e-10), (where, f, fo)
    assert np.allclose(gr, gro, rtol=1e-7, atol=1e-9 * np.abs(gro).max()), (where, gr - gro)


def _run_case(monkeypatch, case: FitCase, variants=None):
    spec, Xt, y, points = case.problem()
    ospec, Xn, ys = oracle_inputs(spec, Xt, y)
    refs = [oracle_reference(case, spec, p, ospec, Xn, ys) for p in points]
    forms = {}
    for variant in variants or case.variants:
        gp = _handle(monkeypatch, variant)
        try:
            gp.set_model(spec, Xt, y)
            worst = 0.0
            for k, (p, ref) in enumerate(zip(points, refs)):
                val, g = gp.data_term(p)
                form = gp.fit_evaluation_form()
                where = (case.id, variant, k, form)
                assert form in case.expected_forms(spec, variant), (where, sorted(case.expected_forms(spec, variant)))
                worst = max(worst, _check_point(case, spec, p, len(y), val, g, ref, where))
                if k == 0 and refs[0][0] == "analytic":
                    _check_objective(spec, p, len(y), val, g, ospec, Xn, ys, where)
            forms[variant] = form
            SEEN.setdefault(form, []).append(f"{case.id}/{variant}")
            print(f"   {case.id:>16} {variant:>7}: {form:<17} worst deviation / tolerance {worst:.2e}")
        finally:
            gp.close()
    return forms


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_fit_evaluation_form_matches_the_oracle(monkeypatch, case):
    _run_case(monkeypatch, case)


def test_m_tile_edge(monkeypatch):
    """K^-1's tiles ride in the factorisation launch only while they are co-resident with its own: the block row where the read-back
    drops from ``tiles+mt`` (found, not assumed), and the sizes on either side of it against the oracle, with the default switches and
    with BBH_TILE_MT=partial."""
    from baybe_amd import gp_spec

    edge = None
    gp = _handle(monkeypatch, "1")
    try:
        for nbk in range(9, 17):
            case = FitCase("baybe", 64 * nbk)
            spec, Xt, y, points = case.problem()
            gp.set_model(spec, Xt, y)
            assert gp.data_term(gp_spec.initial_params(spec))[0] is not None
            if gp.fit_evaluation_form() != "tiles+mt":
                assert gp.fit_evaluation_form() == "tiles", (nbk, gp.fit_evaluation_form())
                edge = nbk
                break
    finally:
        gp.close()
    assert edge is not None, "K^-1's tiles rode in the factorisation launch up to np = 1024"
    print(f"   M-tile edge: tiles+mt up to {64 * (edge - 1)} rows, not from {64 * (edge - 1) + 1}")
    below = _run_case(monkeypatch, FitCase("mt-edge", 64 * (edge - 1)), ("1", "1-mtp"))
    above = _run_case(monkeypatch, FitCase("mt-edge", 64 * (edge - 1) + 1), ("1", "1-mtp"))
    assert below == {"1": "tiles+mt", "1-mtp": "tiles+mt"}, below
    assert above == {"1": "tiles", "1-mtp": "tiles+mt-partial"}, above


def test_handle_reuse_across_models_and_the_pool(monkeypatch):
    """One handle through models that switch path while np stays or returns (the dataflow state is keyed on np / criterion / form
    only), then the same sequence on the handle the pool hands back; a repeated point is bit-identical."""
    # (rq -> pp0 at np = 1088: the same one-launch state over a model of another theta length, whose buffers - the Cholesky flag among
    # them - are fresh allocations; that evaluation once read an uncleared flag as "not positive definite")
    seq = [FitCase("baybe", 1024), FitCase("rq", 1088, d=6, kernel="rq"), FitCase("pp0", 1088, d=6, kernel="pp0"), FitCase("baybe", 1088),
           FitCase("icm-loo", 1024, d=6, criterion="loo", rows=(400, 300, 200, 124)),
           FitCase("baybe", 64, d=5), FitCase("baybe", 2049), FitCase("baybe", 512), FitCase("icm-mll", 512, d=6, rows=(300, 212))]
    prepared = []
    for case in seq:
        spec, Xt, y, points = case.problem()
        ospec, Xn, ys = oracle_inputs(spec, Xt, y)
        prepared.append((case, spec, Xt, y, points[:2], [oracle_reference(case, spec, p, ospec, Xn, ys) for p in points[:2]]))
    from baybe_amd import engine

    created = engine.pool_stats["created"]
    for rnd in range(2):
        gp = _handle(monkeypatch, "1")
        try:
            for case, spec, Xt, y, points, refs in prepared:
                gp.set_model(spec, Xt, y)
                first = None
                for k, (p, ref) in enumerate(zip(points, refs)):
                    val, g = gp.data_term(p)
                    form = gp.fit_evaluation_form()
                    assert form in case.expected_forms(spec, "1"), (case.id, form)
                    _check_point(case, spec, p, len(y), val, g, ref, ("reuse", rnd, case.id, k, form))
                    if first is None:
                        first = (val, g.copy())
                val, g = gp.data_term(points[0])  # the same point again, after another one
                assert val == first[0] and np.array_equal(g, first[1]), (case.id, val - first[0])
        finally:
            gp.close()
    assert engine.pool_stats["created"] <= created + 1  # the second round ran on the pooled handle


@pytest.mark.parametrize("n,icm", [(64, False), (65, False), (513, False), (1025, False), (2048, False), (1040, True)])
def test_whole_fit_ends_where_the_oracle_objective_agrees(monkeypatch, n, icm):
    """~100 back-to-back evaluations of a whole device fit: the oracle's objective at the device's end point equals the device's."""
    from oracle import gp_oracle as go

    case = (FitCase("icm-loo", n, d=6, criterion="loo", rows=(n // 2, n // 4, n // 8, n - n // 2 - n // 4 - n // 8)) if icm
            else FitCase("baybe", n))
    spec, Xt, y, _ = case.problem()
    ospec, Xn, ys = oracle_inputs(spec, Xt, y)
    gp = _handle(monkeypatch, "1")
    try:
        gp.set_model(spec, Xt, y)
        fi = gp.fit(maxiter=80) if icm else gp.fit()
        form = gp.fit_evaluation_form()
    finally:
        gp.close()
    f_at, _ = go.fit_objective(ospec, go.pack_raw(ospec, oracle_params(spec, fi.params)), Xn, ys)
    print(f"   fit n={n} icm={icm}: {fi.nfev} evaluations as {form}, objective {fi.fun:.12f}")
    assert math.isclose(f_at, fi.fun, rel_tol=1e-9, abs_tol=1e-11), (f_at, fi.fun)


def test_every_form_was_hit():
    """After the table: every path of the evaluation ran at least once (``rff``: tests/test_rff_gpu.py)."""
    print("\n   form table:")
    for form in FORMS:
        ids = SEEN.get(form, [])
        print(f"   {form:<17} {len(ids):>4}  {', '.join(ids[:4])}{' ...' if len(ids) > 4 else ''}")
    missing = [f for f in FORMS if f != "rff" and f not in SEEN]
    assert not missing, missing
    assert os.environ.get("BBH_FIT_FLOW") is None  # (monkeypatch left no switch behind)
