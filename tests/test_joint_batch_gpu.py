"""Every joint q'-batch acquisition kernel of baybe_amd/csrc/bbh_acq.hip against the oracle, per candidate.

qLogEI: ``HipGP.qlogei_pending_big(..., stats=...)`` takes every statistic from the caller, so the kernels are fed the synthetic
joint statistics of tests/_joint_cases.py (ordinary rows in four mean families, rows that need each jitter level of
psd_safe_cholesky, rows that are not positive definite, masked rows) and compared row by row with ``qlogei_joint``:

  register form   Q = 2 ... 14, S = 33 / 100 / 512 (1, 3 ragged and 16 sample slices at 777 rows), both signs; one slice and five
                  ragged slices through BBH_PENDING_SLICES
  LDS form        q' = 15, 16; both sides of the 60 KB hand-over at q' = 14; S = 1024 at q' = 8; BBH_PENDING_LDS=1 at Q = 2, 7, 14
  q' > 16         p = 16, 32, 63 with the factor in a global workspace, in one chunk and in several (BBH_QBIG_WS_MB=1)

qEI / qPI / qSR / qUCB / qPSTD read the handle's own pending statistics, so they run on a real model with 1 ... 15 pending points
against ``mc_acq_joint`` on the oracle's joint posterior of every [candidate ; pending]; every seventh candidate is masked and must
score -inf.

tests/test_joint_cases_cpu.py checks the cases themselves (that the regimes are what their labels say, that a wrong jitter level
moves the reference by more than 100 tolerances, that the reference agrees with an independent restatement)."""

import os

import numpy as np
import pytest

from _joint_cases import (BIG_CASES, HANDOVER_CASES, LDS_CASES, LDS_SWITCH_P, ONE_ROW_CASE, REGISTER_P, S1024_CASE, SCORE_ATOL, compare,
                          form_bytes, lds_switch_cases, register_cases)
from _problems import fixed_theta, make_problem

pytestmark = pytest.mark.gpu

# a handle reads the BBH_* switches when it is created
SWITCHES = ("BBH_PENDING_SLICES", "BBH_PENDING_LDS", "BBH_QBIG_WS_MB")
VARIANTS = {
    "default": {},
    "slices1": {"BBH_PENDING_SLICES": "1"},
    "slices5": {"BBH_PENDING_SLICES": "5"},
    "lds": {"BBH_PENDING_LDS": "1"},
    "ws1": {"BBH_QBIG_WS_MB": "1"},
}
SLICE_ORDER_ATOL = 1e-12  # the same terms added in another order
MC_RTOL, MC_ATOL = 1e-8, 1e-9  # tests/test_acqfs_gpu.py::test_mc_family_q1_and_pending
MC_KINDS = ("qEI", "qPI", "qSR", "qUCB", "qPSTD")


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
            made[name] = engine.HipGP(0)
    finally:
        for k, val in keep.items():
            os.environ.pop(k, None) if val is None else os.environ.__setitem__(k, val)
    yield made
    for g in made.values():
        g.close()


def _score(g, case):
    """The device's scores of the case's rows: every statistic is the caller's (X_pending gives the row count only)."""
    import torch

    d = case.build()
    dev = lambda a: torch.tensor(a, device="cuda")  # noqa: E731
    out = g.qlogei_pending_big(dev(d.mean), dev(d.var), dev(d.cross), np.zeros((case.p, 1)), d.z, d.best_f, case.sign,
                               alive=dev(d.alive), stats=(d.mean_p, d.cov_pp))
    return out.cpu().numpy()


def _agree(a, b, case):
    """Largest |a - b| over the scored rows of two device results (which mark the other rows alike)."""
    live = case.build().scored
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)), case.id
    return float(np.abs(a[live] - b[live]).max()) if live.any() else 0.0


def _record(name, value, tol):
    from conftest import record_deviation

    print(f"{name}: observed {value:.3e} (tolerance {tol:.1e})")
    record_deviation(f"joint_batch/{name}", value, tol)


@pytest.mark.parametrize("p", REGISTER_P, ids=[f"Q{p + 1}" for p in REGISTER_P])
def test_register_form_every_instantiation(handles, p):
    """``bbh_qlogei_pending_q_kernel<Q>``, Q = p + 1: 1, 3 (34 / 34 / 32 samples) and 16 sample slices on the default handle, the
    one-slice path (``partial == nullptr``) at every S, five slices of 103 / 103 / 103 / 103 / 100 samples at S = 512."""
    worst = {"default": 0.0, "slices1": 0.0, "slices5": 0.0, "order": 0.0}
    failures = []
    for case in register_cases(p):
        assert form_bytes(case) <= 60 * 1024  # (the register form's side of the hand-over)
        base = _score(handles["default"], case)
        dev = compare(base, case)
        worst["default"] = max(worst["default"], dev)
        if dev > SCORE_ATOL:
            failures.append((case.id, "default", dev))
        for name in ("slices1", "slices5") if case.S == 512 else ("slices1",):
            got = _score(handles[name], case)
            dev, order = compare(got, case), _agree(got, base, case)
            worst[name], worst["order"] = max(worst[name], dev), max(worst["order"], order)
            if dev > SCORE_ATOL or order > SLICE_ORDER_ATOL:
                failures.append((case.id, name, dev, order))
    for name in ("default", "slices1", "slices5"):
        _record(f"register[Q={p + 1},{name}]", worst[name], SCORE_ATOL)
    _record(f"register_slice_order[Q={p + 1}]", worst["order"], SLICE_ORDER_ATOL)
    assert not failures, failures


def test_single_candidate(handles):
    """N = 1: one thread of one workgroup does any work, in every form (three slices on the default handle)."""
    case = ONE_ROW_CASE
    worst = max(compare(_score(handles[name], case), case) for name in ("default", "slices1", "lds"))
    _record("single_candidate", worst, SCORE_ATOL)
    assert worst <= SCORE_ATOL


@pytest.mark.parametrize("case", LDS_CASES, ids=[c.id for c in LDS_CASES])
def test_lds_form_fifteen_and_sixteen_points(handles, case):
    """q' = 15, 16: ``bbh_qlogei_pending_kernel`` whatever the sample count."""
    dev = compare(_score(handles["default"], case), case)
    _record(f"lds[{case.id}]", dev, SCORE_ATOL)
    assert dev <= SCORE_ATOL, (case.id, dev)


def test_sixty_kb_hand_over(handles):
    """8 (S q' + p + p^2) bytes against 60 KB.  q' = 14 with one slice: S = 535 is the register form's largest dynamic-LDS launch
    (61 376 B), S = 536 the LDS form's first (61 488 B); the default handle takes 16 slices at S = 535.  S = 1024 at q' = 8 is the LDS
    form on every handle.  The register and the LDS form of S = 535 agree to two tolerances."""
    below, above = HANDOVER_CASES
    assert form_bytes(below) <= 60 * 1024 < form_bytes(above) and form_bytes(S1024_CASE) > 60 * 1024
    out = {}
    for case in (below, above, S1024_CASE):
        for name in ("slices1", "default"):
            out[case, name] = _score(handles[name], case)
            dev = compare(out[case, name], case)
            _record(f"hand_over[{case.id},{name}]", dev, SCORE_ATOL)
            assert dev <= SCORE_ATOL, (case.id, name, dev)
    lds = _score(handles["lds"], below)
    assert compare(lds, below) <= SCORE_ATOL
    forms = _agree(lds, out[below, "slices1"], below)
    _record(f"hand_over_register_vs_lds[{below.id}]", forms, 2 * SCORE_ATOL)
    assert forms <= 2 * SCORE_ATOL


@pytest.mark.parametrize("p", LDS_SWITCH_P, ids=[f"Q{p + 1}" for p in LDS_SWITCH_P])
def test_lds_form_under_its_switch(handles, p):
    """BBH_PENDING_LDS=1: the generic LDS form (double-precision streaming log-sum-exp) at sizes the register form otherwise takes;
    it holds to the oracle, and the reduced-precision register form is within two tolerances of it."""
    worst, forms = 0.0, 0.0
    for case in lds_switch_cases(p):
        lds = _score(handles["lds"], case)
        worst = max(worst, compare(lds, case))
        forms = max(forms, _agree(lds, _score(handles["default"], case), case))
    _record(f"lds_switch[Q={p + 1}]", worst, SCORE_ATOL)
    _record(f"lds_switch_vs_register[Q={p + 1}]", forms, 2 * SCORE_ATOL)
    assert worst <= SCORE_ATOL and forms <= 2 * SCORE_ATOL, (p, worst, forms)


@pytest.mark.parametrize("case", BIG_CASES, ids=[c.id for c in BIG_CASES])
def test_beyond_sixteen_points(handles, case):
    """``bbh_qlogei_pending_big_kernel`` in all regimes: the factor workspace in one chunk and under BBH_QBIG_WS_MB=1 (two chunks of
    the 300 rows at q' = 33, five at q' = 64) - the same bits, and the oracle's scores."""
    one, many = _score(handles["default"], case), _score(handles["ws1"], case)
    dev = compare(one, case)
    _record(f"beyond_sixteen[{case.id}]", dev, SCORE_ATOL)
    assert np.array_equal(one, many, equal_nan=True), (case.id, _agree(one, many, case))
    assert dev <= SCORE_ATOL, (case.id, dev)


# ---- the other MC functions: the handle's own pending statistics, so a real model -----------------------
MC_D, MC_N_TRAIN, MC_CANDIDATES, MC_BETA = 3, 20, 300, 0.4


@pytest.fixture(scope="module")
def mc_setup(handles):
    from baybe_amd import gp_spec
    from oracle import gp_oracle as go

    d = MC_D
    X, Xt, y = make_problem(2000, d, MC_N_TRAIN, seed=11)
    rows = np.unique(X, axis=0)  # distinct rows: a candidate never coincides with a pending point
    rows = rows[np.random.default_rng(3).permutation(len(rows))]
    pool, cand = rows[:15], np.ascontiguousarray(rows[15:15 + MC_CANDIDATES])
    assert len(cand) == MC_CANDIDATES
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    ls, nz, _ = fixed_theta(d)
    prm = gp_spec.GPParams(np.full(d, ls), nz, 0.02)
    for name in ("default", "lds"):
        handles[name].set_model(spec, Xt, y)
        handles[name].factorize(prm)
    om = go.GPModel(go.GPSpec.baybe_default(d, np.zeros(d), np.ones(d)), go.GPParams(prm.lengthscale, prm.noise, prm.mean), Xt, y)
    return om, pool, cand


def _mc_compare(handles, names, om, pend, cand, S, tag):
    import torch

    from oracle import gp_oracle as go

    p = len(pend)
    z = go.sobol_normal_base_samples(S, p + 1, 3)
    live = np.ones(len(cand), dtype=bool)
    live[::7] = False  # every seventh candidate is masked: the kernels score it -inf
    alive = torch.tensor(live.astype(np.uint8), device="cuda")
    joint = [om.posterior_joint(np.vstack([x[None, :], pend])) for x in cand]
    dev_in = {}
    for name in names:
        g = handles[name]
        g.set_pending(pend)
        dev_in[name] = (*g.posterior(cand), g.cross_cov(cand))
    worst, failures = 0.0, []
    for sign in (1.0, -1.0):
        bf = go.best_f_from_model(om, sign)
        for kind in MC_KINDS:
            ref = np.array([go.mc_acq_joint(kind, m, C, z, bf, sign, beta=MC_BETA) for m, C in joint])
            for name in names:
                m, v, cross = dev_in[name]
                got = handles[name].mc_acq(kind, m, v, z, bf, sign, beta=MC_BETA, alive=alive, cross=cross).cpu().numpy()
                if not np.all(np.isneginf(got[~live])):
                    failures.append((kind, sign, name, "masked rows", got[~live]))
                ratio = float((np.abs(got[live] - ref[live]) / (MC_ATOL + MC_RTOL * np.abs(ref[live]))).max())
                worst = max(worst, ratio)
                if not ratio <= 1.0:
                    failures.append((kind, sign, name, ratio, float(np.abs(got[live] - ref[live]).max())))
    for name in names:
        handles[name].set_pending(None)
    _record(f"mc_family_over_tolerance[{tag}]", worst, 1.0)
    assert not failures, failures


@pytest.mark.parametrize("p", range(1, 16), ids=[f"q{p + 1}" for p in range(1, 16)])
def test_other_mc_functions_every_instantiation(handles, mc_setup, p):
    """``bbh_mc_pending_q_kernel<Q>`` (q' = 2 ... 14) and ``bbh_mc_pending_kernel`` (q' = 15, 16): all five functions, both signs, every
    candidate; under BBH_PENDING_LDS=1 the generic form at q' = 2, 7, 14 as well."""
    om, pool, cand = mc_setup
    names = ("default", "lds") if p in LDS_SWITCH_P else ("default",)
    _mc_compare(handles, names, om, pool[:p], cand, 64, f"q'={p + 1},S=64")


def test_other_mc_functions_past_the_hand_over(handles, mc_setup):
    """S = 1024 at q' = 8: 8 (S q' + q' + p + p^2) = 66 048 bytes, past 60 KB - the generic form."""
    om, pool, cand = mc_setup
    _mc_compare(handles, ("default",), om, pool[:7], cand, 1024, "q'=8,S=1024")
