"""The passes behind the pending columns of a greedy batch against the oracle, every row: ``set_pending`` + ``cross_cov`` (steps 2 ... q
of every greedy batch, every ``acquisition_values(..., pending_experiments=...)``), ``posterior()`` while pending points are set, and
the handle's pending state.  Cases, references and the scaled metric: tests/_pending_cases.py; the CPU guard of the cases (that the
float64 oracle is within 1e-13 of a long-double restatement for every one of them, that they would notice a shifted, stale or
mis-tasked column and a padding row that contributes): tests/test_pending_cases_cpu.py.

Every comparison with the oracle is scaled and absolute and held to 1e-11: |cross - ref| / (ysd^2 sqrt(k(x, x) k(p_j, p_j))),
|var - ref| / (ysd^2 k(x, x)), |mean - ref| / ysd.

WHICH CODE EVERY TEST REACHES, read off ``bbh_launch_fused`` (csrc/bbh_panel.hip): a mean-only pass (``with_var`` false) skips the
cooperative, two-sweep and register-resident forms (they require ``with_var``), so for a single Matérn / RBF kernel it is always
``bbh_fused_posterior_kernel`` - the pipelined instantiation <table, kind, KD> where ``kdp`` is non-zero (Matérn-5/2; RBF / Matérn-3/2
without a table; kd in 2 ... 16; BBH_PIPELINE on), else ``bbh_fused_launch_kd0``'s plain one.  A variance pass with p > 0 fails
``coop_mean_valu`` and the register-resident form's ``p == 0``, so it is the same kernel's ``with_var`` branch with the MFMA mean and
the trailing pending-block loop, with the kernel-value cache (LDS, or global slabs under BBH_KV_GLOBAL=1 BBH_KV_LDS=3) once there is
more than one pass.  Composite / RQ / piecewise / dot-product / periodic models take ``bbh_coopg_cross_kernel<KD, F>`` for mean-only
passes where the generic production is packed (``coopg_ready``) and BBH_COOPG_CROSS is on, else ``bbh_launch_unfused_ext`` (the
materialised K*); RFF models ``bbh_rff_posterior_launch``.

  test_mean_only_pass (family A)        bbh_fused_posterior_kernel<false | true, Matérn-5/2 | RBF | Matérn-3/2, KD>, KD = 2, 4, 6, 8, 12,
                                        16: kvp_load / kvp_dist / kv_all over nb_ext blocks, every instantiation with a ragged n and
                                        p = 15 (the table in tests/_pending_cases.py); the plain branch (compute_kv) at kd = 18, for
                                        Matérn-1/2, RBF / Matérn-3/2 with a table and under BBH_PIPELINE=0; n = 1 ... 513
  test_ragged_rows_and_layout (B)       the same pass through the C entry ``bbh_cross_cov`` at N = 1 ... 257 rows with ldx = d + 3, non-unit
                                        bounds, the task column in the middle (numcol_identity = 0); nothing written past row N
  test_variance_pass_with_pending (C)   the with_var branch + pending block(s) at nb = 4 ... 68 (one to five passes, every last-pass
                                        width), KD 2 ... 16 and plain, RBF, Matérn-3/2, the ICM table; BBH_KVCACHE=0 and global slabs
                                        bit-identical to the default; ``posterior_kernel_form()`` "windowed" against another form at p = 0
  test_generic_and_other_paths (D)      bbh_coopg_cross_kernel<KD, F> for every (F, KD) of bbh_coopg_cross_launch and every kind of the
                                        generic production; the same models under BBH_COOPG_CROSS=0 and the materialised-only models
                                        (bbh_launch_unfused_ext); bbh_rff_posterior_kernel<32> (D = 16) and <64> (D = 64)
  test_state_transitions (E)            bbh_pending_set / bbh_rff_pending_set rewriting d_meanB, the fragment block nb, d_taskext and
                                        nb_ext in place: p = 15 -> 2 -> 0 -> 1, then bbh_factorize, which drops the pending points"""

import os

import numpy as np
import pytest

import _pending_cases as pc
from _pending_cases import PEND_MEAN_ATOL, TOL

pytestmark = pytest.mark.gpu

# a handle reads the BBH_* switches when it is created
SWITCHES = ("BBH_PIPELINE", "BBH_KVCACHE", "BBH_KV_GLOBAL", "BBH_KV_LDS", "BBH_COOPG_CROSS", "BBH_COOP", "BBH_SMALL", "BBH_MEAN_VALU")
VARIANTS = {
    "default": {},
    "nopipe": {"BBH_PIPELINE": "0"},
    "nokv": {"BBH_KVCACHE": "0"},
    "kvglobal": {"BBH_KV_GLOBAL": "1", "BBH_KV_LDS": "3"},
    "nocoopgcross": {"BBH_COOPG_CROSS": "0"},
}
SENTINEL = -777.25


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
        for k in SWITCHES:
            os.environ.pop(k, None)
        made["fresh"] = engine.HipGP(0)  # a second default handle: what a pending state is compared with
    finally:
        for k, val in keep.items():
            os.environ.pop(k, None) if val is None else os.environ.__setitem__(k, val)
    yield made
    for g in made.values():
        g.close()


def _np(t):
    return t.cpu().numpy()


def _rows(a):
    """A device copy of (read-only, shared) case rows."""
    import torch

    return torch.from_numpy(np.array(a)).cuda()


def _load(g, model, params=None):
    """Model and factorisation onto the handle (which drops any pending points); the device standardises like the oracle."""
    md = model.build()
    g.set_model(md.spec, md.Xt, md.y)
    g.factorize(md.params if params is None else params)
    assert abs(g.ysd - md.om.ysd) <= 1e-13 * md.om.ysd and g.jitter == 0.0, (model.id, g.ysd, md.om.ysd, g.jitter)
    return md


def _record(case, devs):
    """The observed maxima of a case next to what they are held to: everything scaled to the prior under ``pending_passes/<case>``, the
    ``set_pending`` means (1e-10 of ysd) under ``pending_passes/<case>:pend_mean``; every figure is printed."""
    from conftest import record_deviation

    for what, value in devs.items():
        print(f"{case.id} {what}: observed {value:.3e} (tolerance {_tol(what):.1e})")
    scaled = [v for k, v in devs.items() if _tol(k) == TOL]
    means = [v for k, v in devs.items() if _tol(k) == PEND_MEAN_ATOL]
    if scaled:
        record_deviation(f"pending_passes/{case.id}", max(scaled), TOL)
    if means:
        record_deviation(f"pending_passes/{case.id}:pend_mean", max(means), PEND_MEAN_ATOL)


def _tol(what):
    return PEND_MEAN_ATOL if what.endswith("pend_mean") else TOL


def _pending_devs(case, ref, cr, mp, cpp):
    """Deviations of a cross-covariance pass and of the ``set_pending`` statistics behind it: the columns against the oracle; the pending
    mean and covariance; on every row that IS pending point j, column j against the device's own cov_pp[j, j] and against the oracle's
    posterior variance of that row."""
    d = case.build()
    out = {"cross": pc.scaled_cross(cr, ref), "pend_cov": pc.scaled_cov_pp(cpp, ref),
           "pend_mean": float(np.abs(mp - ref.mean_p).max() / ref.ysd), "own_diag": 0.0, "oracle_var": 0.0}
    for i in np.nonzero(d.rows("pending"))[0]:
        j = int(d.labels[i].split(":")[1])
        scale = ref.ysd**2 * ref.kpp[j]
        assert ref.kxx[i] == ref.kpp[j]
        out["own_diag"] = max(out["own_diag"], abs(cr[i, j] - cpp[j, j]) / scale)
        out["oracle_var"] = max(out["oracle_var"], abs(cr[i, j] - ref.var[i]) / scale)
    return out


def _hold(case, devs):
    _record(case, devs)
    failures = [(what, value, _tol(what)) for what, value in devs.items() if not value <= _tol(what)]
    assert not failures, (case.id, failures)


def _cross_pass(g, case, ref):
    d = case.build()
    mp, cpp = g.set_pending(d.P)
    cr = _np(g.cross_cov(_rows(d.cand)))
    assert cr.shape == (case.N, case.p)
    return cr, _pending_devs(case, ref, cr, mp, cpp)


A_CASES = pc.family_a()


@pytest.mark.parametrize("case", A_CASES, ids=[c.id for c in A_CASES])
def test_mean_only_pass(handles, case):
    """Family A: the ``!with_var`` branches of ``bbh_fused_posterior_kernel``, all 257 rows."""
    g = handles[case.handle]
    _load(g, case.model)
    _, devs = _cross_pass(g, case, case.reference())
    g.set_pending(None)
    _hold(case, devs)


B_FULL = {}  # (model, p) -> the N = 257 launch


def _raw_cross(g, wide, N, p):
    """``bbh_cross_cov`` as ``HipGP.cross_cov`` calls it, into a buffer with 64 p sentinel doubles behind row N."""
    import torch

    buf = torch.full((N * p + 64 * p,), SENTINEL, dtype=torch.float64, device="cuda")
    g._check(g._lib.bbh_cross_cov(g._h, wide.data_ptr(), N, wide.stride(0), buf.data_ptr()), "bbh_cross_cov")
    out = _np(buf)
    return out[: N * p].reshape(N, p), out[N * p:]


B_CASES = pc.family_b()


@pytest.mark.parametrize("case", B_CASES, ids=[c.id for c in B_CASES])
def test_ragged_rows_and_layout(handles, case):
    """Family B: N = 1 ... 257 rows of a matrix with row stride d + 3 (NaN in the columns that are not the model's), bounds other than
    [0, 1], the task column in the middle.  Every launch equals the 257-row launch bit for bit on its rows and leaves the doubles
    behind row N alone; the rows hold to the oracle."""
    import torch

    g = handles["default"]
    model, p = case.model, case.p
    full = pc.PendCase("B", model, p, pc.N_FULL)
    d = full.build()
    _load(g, model)
    mp, cpp = g.set_pending(d.P)
    wide = torch.full((pc.N_FULL, model.dtot + 3), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, : model.dtot] = _rows(d.cand)
    assert wide.stride(0) == model.dtot + 3
    if (model, p) not in B_FULL:
        B_FULL[model, p] = _raw_cross(g, wide, pc.N_FULL, p)[0]
    cr, tail = _raw_cross(g, wide, case.N, p)
    g.set_pending(None)
    assert np.array_equal(tail, np.full(64 * p, SENTINEL)), (case.id, "written behind row N", np.nonzero(tail != SENTINEL)[0][:8])
    assert np.array_equal(cr, B_FULL[model, p][: case.N]), (case.id, np.abs(cr - B_FULL[model, p][: case.N]).max())
    _hold(case, _pending_devs(case, case.reference(), cr, mp, cpp))


C_CASES = pc.family_c()


@pytest.mark.parametrize("case", C_CASES, ids=[c.id for c in C_CASES])
def test_variance_pass_with_pending(handles, case):
    """Family C: ``posterior()`` after ``set_pending()`` is the windowed kernel with the MFMA mean and the pending-block loop at every n
    (``posterior_kernel_form() == "windowed"``).  Mean and variance hold to the oracle and to the same handle's p = 0 pass - another
    kernel form up to n = 1024 -, the cross pass holds on the same models; from two passes on (n >= 257) the handles without a
    kernel-value cache and with global slabs give the default handle's bits."""
    model, ref, d = case.model, case.reference(), case.build()
    names = ("default", "nokv", "kvglobal") if model.n >= 257 else ("default",)
    got, devs = {}, {}
    for name in names:
        g = handles[name]
        _load(g, model)
        m0, v0 = g.posterior(_rows(d.cand))
        form0 = g.posterior_kernel_form()
        assert form0 == pc.expected_p0_form(model, case.N), (case.id, name, form0)
        mp, cpp = g.set_pending(d.P)
        m, v = g.posterior(_rows(d.cand))
        assert g.posterior_kernel_form() == "windowed", (case.id, name, g.posterior_kernel_form())
        cr = _np(g.cross_cov(_rows(d.cand)))
        g.set_pending(None)
        m, v, m0, v0 = _np(m), _np(v), _np(m0), _np(v0)
        got[name] = (m, v, cr)
        tag = "" if name == "default" else f"{name}:"
        devs.update({tag + k: val for k, val in _pending_devs(case, ref, cr, mp, cpp).items()})
        devs.update({tag + "mean": pc.scaled_mean(m, ref), tag + "var": pc.scaled_var(v, ref),
                     tag + "mean_vs_p0": pc.scaled_mean(m, ref, m0), tag + "var_vs_p0": pc.scaled_var(v, ref, v0)})
    for name in names[1:]:
        for a, b, what in zip(got[name], got["default"], ("mean", "var", "cross")):
            assert np.array_equal(a, b), (case.id, name, what, np.abs(a - b).max())
    _hold(case, devs)


D_CASES = pc.family_d()


@pytest.mark.parametrize("case", D_CASES, ids=[c.id for c in D_CASES])
def test_generic_and_other_paths(handles, case):
    """Family D: ``bbh_coopg_cross_kernel`` in every (F, KD), the materialised-K* path (the same models under BBH_COOPG_CROSS=0; a
    Matérn-1/2 factor, d = 31, n = 513) and the feature-space pass of the RFF models, every row of 257 and of 65."""
    g = handles[case.handle]
    d = case.build()
    ref = case.reference()
    _load(g, case.model)
    m0, v0 = (_np(t) for t in g.posterior(_rows(d.cand)))
    assert g.posterior_kernel_form() == pc.expected_p0_form(case.model, case.N), (case.id, g.posterior_kernel_form())
    _, devs = _cross_pass(g, case, ref)
    g.set_pending(None)
    devs.update({"p0_mean": pc.scaled_mean(m0, ref), "p0_var": pc.scaled_var(v0, ref)})
    _hold(case, devs)


@pytest.mark.parametrize("model", pc.E_MODELS, ids=[m.id for m in pc.E_MODELS])
def test_state_transitions(handles, model):
    """Family E: p = 15 -> 2 -> 0 -> 1 on one handle, other points each time.  After every step ``cross_cov`` has exactly p columns, the
    bits a fresh handle gives for that set, and ``set_pending``'s statistics are the oracle's; with p = 0 ``cross_cov`` fails,
    ``posterior()`` gives the bits it gave before any pending point was set and is back on its p = 0 form.  ``bbh_factorize`` drops
    the pending points (``h->p = 0``): ``cross_cov`` after it fails with "no pending points set" until ``set_pending`` is called again,
    and then has the new factorisation's columns."""
    import copy

    from baybe_amd import HipError

    g, fresh = handles["default"], handles["fresh"]
    md = _load(g, model)
    steps = [pc.PendCase("E", model, p, 130, pend_seed=s) for p, s in pc.E_STEPS]
    zero = next(c for c in steps if c.p == 0)
    cand0 = zero.build().cand
    form0 = pc.expected_p0_form(model, 130)
    with_pending = "feature-space" if model.rff else ("materialised" if model.generic else "windowed")
    m0, v0 = (_np(t) for t in g.posterior(_rows(cand0)))
    assert g.posterior_kernel_form() == form0
    with pytest.raises(HipError, match="no pending points set"):
        g.cross_cov(_rows(cand0))
    for case in steps:
        d, ref = case.build(), case.reference()
        if case.p == 0:
            assert g.set_pending(None) == (None, None)
            with pytest.raises(HipError, match="no pending points set"):
                g.cross_cov(_rows(d.cand))
            m, v = (_np(t) for t in g.posterior(_rows(d.cand)))
            assert g.posterior_kernel_form() == form0, (case.id, g.posterior_kernel_form())
            assert np.array_equal(m, m0) and np.array_equal(v, v0), (case.id, np.abs(m - m0).max(), np.abs(v - v0).max())
            continue
        cr, devs = _cross_pass(g, case, ref)
        m, v = (_np(t) for t in g.posterior(_rows(d.cand)))
        assert g.posterior_kernel_form() == with_pending, (case.id, g.posterior_kernel_form())
        _load(fresh, model)
        cr_f, _ = _cross_pass(fresh, case, ref)
        m_f, v_f = (_np(t) for t in fresh.posterior(_rows(d.cand)))
        assert np.array_equal(cr, cr_f), (case.id, "cross_cov after the earlier pending sets", np.abs(cr - cr_f).max())
        assert np.array_equal(m, m_f) and np.array_equal(v, v_f), (case.id, "posterior after the earlier pending sets")
        devs.update({"mean": pc.scaled_mean(m, ref), "var": pc.scaled_var(v, ref)})
        _hold(case, devs)
    # a new factorisation: the pending points are gone with the old one
    last = steps[-1]
    d = last.build()
    p2 = copy.deepcopy(md.params)
    p2.lengthscale = np.asarray(p2.lengthscale) * 1.1
    g.factorize(p2)
    with pytest.raises(HipError, match="no pending points set"):
        g.cross_cov(_rows(d.cand))
    g.set_pending(d.P)
    cr = _np(g.cross_cov(_rows(d.cand)))
    _load(fresh, model, params=p2)
    fresh.set_pending(d.P)
    cr_f = _np(fresh.cross_cov(_rows(d.cand)))
    assert cr.shape == (130, last.p) and np.array_equal(cr, cr_f)
    g.set_pending(None)
    fresh.set_pending(None)
