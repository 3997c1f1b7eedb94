"""The seeded distance GEMM of the cooperative posterior form (``csrc/bbh_coop.h``, KVF bit 8: the squared norms enter as the
accumulator's initial value, ceil(d / 4) k-steps, the Matérn-5/2 constant folded into the operands) and the shortened exponent split
of ``kv_micro`` against the oracle's exact posterior, every row, and against the same model on a handle created under
``BBH_COOP_SEED=0`` (the augmented stream: the two differ in the rounding of r2 only).

Metric and tolerance of tests/test_pending_passes_gpu.py: |var - ref| / (ysd^2 k(x, x)) and |mean - ref| / ysd, 1e-11 against the
oracle; 1e-12 between the two forms.

Both handles are created with ``BBH_SMALL=0`` so that n <= 64 reaches the cooperative form (GMIN = 6) instead of the
register-resident one.  Shapes: d on both sides of every k-step boundary (d = 3, 4: the seeded stream has no fewer k-steps and the
dispatch keeps the augmented one - read back through ``posterior_distance_seeded()``), n with padding rows inside a k-block and in
every GMIN instantiation (n = 17, 64, 65: rounds 6 - 7, seeded for d <= 12; 129: 4 - 7; 257, 512: all), N with a partial last tile.  Rows 1 - 3 of
every candidate set are copies of training rows (t at the 1e-300 floor), rows 4 - 5 lie 30 lengthscales away (the kernel values
vanish against the prior: the variance IS the prior)."""

import os

import numpy as np
import pytest

from _problems import fixed_theta, make_problem, make_tl_problem, oracle_params, oracle_spec

pytestmark = pytest.mark.gpu

TOL = 1e-11       # device against the oracle, scaled to the prior
TOL_FORMS = 1e-12  # seeded against augmented stream, scaled to the prior
SWITCHES = ("BBH_SMALL", "BBH_COOP_SEED", "BBH_COOP", "BBH_COOP_SMALL", "BBH_PIPELINE", "BBH_MEAN_VALU", "BBH_SMALL_FORCE")

# d -> the seeded stream has fewer k-steps than the augmented one's instantiation: ceil(d / 4) (at least 2; 12 beyond 8) against
# ceil((d + 2) / 4) rounded up to 2, 4, 6, 8, 12, 16
SEEDED = {3: False, 4: False, 7: True, 8: True, 12: True, 15: True, 16: True, 19: True, 20: True, 23: True, 24: True,
          27: True, 31: True, 32: True, 48: True}

# (d, n, N, what the first row is when N == 1)
CASES = [(3, 17, 16, None), (4, 129, 40, None), (7, 65, 40, None), (8, 64, 1, "copy"), (12, 257, 40, None), (12, 64, 40, None),
         (15, 512, 40, None), (16, 129, 16, None), (19, 17, 40, None), (20, 512, 40, None), (20, 65, 16, None), (20, 257, 40, None),
         (23, 257, 1, "far"), (24, 512, 16, None),
         # k-step counts the list above does not reach: 7 (no seeded n <= 256 instantiation: the augmented stream's at n = 129), 8, 12
         (27, 257, 40, None), (27, 129, 16, None), (31, 65, 16, None), (32, 512, 40, None), (48, 512, 16, None)]


@pytest.fixture(scope="module")
def handles():
    from baybe_amd import engine

    keep = {k: os.environ.get(k) for k in SWITCHES}
    made = {}
    try:
        for name, env in (("seeded", {"BBH_SMALL": "0"}), ("augmented", {"BBH_SMALL": "0", "BBH_COOP_SEED": "0"})):
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


def _np(t):
    return t.cpu().numpy()


def _candidates(X, Xt, ls, N, first):
    """N candidate rows: grid rows, with copies of the first, a middle and the last training row (the last one sits next to the padding
    rows of its k-block) and two rows 30 lengthscales from a training row; ``first`` names what a single row is."""
    C = np.array(X[:N], dtype=np.float64)
    dnum = len(ls)
    far = Xt[0].copy()
    far[0] += 30.0 * ls[0]
    far2 = Xt[-1].copy()
    far2[:dnum] -= 30.0 * ls / np.sqrt(dnum)
    special = {"copy": [Xt[len(Xt) // 2]], "far": [far]}.get(first, [C[0], Xt[0], Xt[len(Xt) // 2], Xt[-1], far, far2])
    for i, row in enumerate(special[:N]):
        C[i] = row
    labels = {"copy": ["copy"], "far": ["far"]}.get(first, ["grid", "copy", "copy", "copy", "far", "far"])[:N]
    return C, labels


def _check(case_id, handles, spec, p, Xt, y, C, labels, expect_seeded, kxx=None):
    """Both handles against the oracle (1e-11) and against each other (1e-12), scaled to the prior; which stream ran."""
    import torch

    from conftest import record_deviation
    from oracle import gp_oracle as go

    om = go.GPModel(oracle_spec(spec), oracle_params(spec, p), Xt, y)
    mo, vo = om.posterior(C)
    kxx = np.ones(len(C)) if kxx is None else kxx
    out = {}
    for name, g in handles.items():
        g.set_model(spec, Xt, y)
        g.factorize(p)
        assert abs(g.ysd - om.ysd) <= 1e-13 * om.ysd and g.jitter == 0.0
        m, v = g.posterior(torch.from_numpy(C).cuda())
        assert g.posterior_kernel_form() == "cooperative", (case_id, name, g.posterior_kernel_form())
        assert g.posterior_distance_seeded() == (expect_seeded and name == "seeded"), (case_id, name)
        out[name] = (_np(m), _np(v))
        assert np.isfinite(out[name][0]).all() and np.isfinite(out[name][1]).all()
        dm = float((np.abs(out[name][0] - mo) / om.ysd).max())
        dv = float((np.abs(out[name][1] - vo) / (om.ysd**2 * kxx)).max())
        print(f"{case_id} {name}: mean {dm:.3e} var {dv:.3e} (tolerance {TOL:.1e})")
        record_deviation(f"seeded_distance/{case_id}:{name}", max(dm, dv), TOL)
        assert dm <= TOL and dv <= TOL, (case_id, name, dm, dv)
    (ms, vs), (ma, va) = out["seeded"], out["augmented"]
    fm = float((np.abs(ms - ma) / om.ysd).max())
    fv = float((np.abs(vs - va) / (om.ysd**2 * kxx)).max())
    print(f"{case_id} seeded against augmented: mean {fm:.3e} var {fv:.3e} (tolerance {TOL_FORMS:.1e})")
    record_deviation(f"seeded_distance/{case_id}:forms", max(fm, fv), TOL_FORMS)
    assert fm <= TOL_FORMS and fv <= TOL_FORMS, (case_id, fm, fv)
    for i, what in enumerate(labels):
        if what == "far":  # every kernel value is below 1e-20, its square vanishes against the prior: the variance IS the prior
            for _, v in out.values():  # (1e-13: what the device's and the oracle's ysd may differ by)
                assert abs(v[i] / (om.ysd**2 * kxx[i]) - 1.0) <= 1e-13, (case_id, i, v[i])
    return out


@pytest.mark.parametrize("d,n,N,first", CASES, ids=[f"d{d}-n{n}-N{N}" for d, n, N, _ in CASES])
def test_seeded_stream_matches_the_oracle_and_the_augmented_stream(d, n, N, first, handles):
    from baybe_amd import gp_spec

    X, Xt, y = make_problem(2000, d, n, seed=11)
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d))
    ls, nz, _ = fixed_theta(d)
    p = gp_spec.GPParams(np.full(d, ls) * (0.8 + 0.4 * np.random.default_rng(7).random(d)), nz, 0.05)
    C, labels = _candidates(X, Xt, p.lengthscale, N, first)
    # The small-model instantiations of the seeded stream: 2 and 3 k-steps (d <= 12) at n <= 128, 2 - 6 (d <= 24) at n <= 256.  Beyond,
    # the dispatch keeps the augmented stream's small-model instantiation where it has one (d <= 30) and takes the eight-round seeded
    # kernel otherwise (d = 31, 32).
    seeded = SEEDED[d] and not (n <= 128 and 12 < d <= 30) and not (n <= 256 and 24 < d <= 30)
    _check(f"d{d}-n{n}-N{N}", handles, spec, p, Xt, y, C, labels, seeded)


@pytest.mark.parametrize("n_per_task", [100, 200], ids=["n200", "n400"])
def test_seeded_stream_with_the_task_table(n_per_task, handles):
    """Two tasks (KVF = 1 | 8): the table row is the candidate's own task; n = 200 (rounds 4 - 7) and 400 (all rounds)."""
    from baybe_amd import gp_spec
    from oracle import gp_oracle as go

    d, T = 12, 2
    X, Xt, y = make_tl_problem(2000, d, n_per_task, T=T, seed=6)
    X[:, d] = np.random.default_rng(0).integers(0, T, len(X))  # candidates of both tasks
    spec = gp_spec.GPSpec.baybe_default(d + 1, np.zeros(d + 1), np.ones(d + 1), task_idx=d, n_tasks=T)
    p = gp_spec.initial_params(spec)
    p.task_W = p.task_W * np.array([[1.0, 0.6], [0.5, 1.1]])
    p.lengthscale = p.lengthscale * np.linspace(0.8, 1.3, d)
    C, labels = _candidates(X, Xt, p.lengthscale, 40, None)
    # k(x, x) of a candidate is its task's diagonal table entry: the oracle's variance of a row 1e3 lengthscales from everything
    om = go.GPModel(oracle_spec(spec), oracle_params(spec, p), Xt, y)
    probe = np.tile(Xt[0], (T, 1))
    probe[:, 0] += 1e3 * p.lengthscale[0]
    probe[:, d] = np.arange(T)
    ktt = om.posterior(probe)[1] / om.ysd**2
    kxx = ktt[C[:, d].astype(int)]
    _check(f"tasks-n{T * n_per_task}", handles, spec, p, Xt, y, C, labels, True, kxx=kxx)


@pytest.mark.parametrize("kernel", ["rbf", "matern32"])
def test_other_kinds_keep_the_augmented_stream(kernel, handles):
    """RBF and Matérn-3/2 have no seeded instantiation; they pin the exponent split of ``kv_micro`` where the seeded stream does not apply."""
    from baybe_amd import gp_spec

    d, n, N = 12, 129, 40
    X, Xt, y = make_problem(2000, d, n, seed=12)
    spec = gp_spec.GPSpec.baybe_default(d, np.zeros(d), np.ones(d), kernel=kernel)
    ls, nz, _ = fixed_theta(d)
    p = gp_spec.GPParams(np.full(d, ls) * (0.8 + 0.4 * np.random.default_rng(8).random(d)), nz, 0.05)
    C, labels = _candidates(X, Xt, p.lengthscale, N, None)
    _check(f"{kernel}-d{d}-n{n}", handles, spec, p, Xt, y, C, labels, False)
