"""The per-tile set-up of the cooperative posterior kernel (``bbh_coop_posterior_kernel``, csrc/bbh_coop.h) against the oracle, every
row: the candidate fragments that the four waves of a workgroup build once and exchange through LDS, the seeded stream's training
fragments in pairs of k-steps and its contiguous alpha / |a|^2 image.  Models, candidate rows (ordinary grid rows, training rows -
r^2 = 0 -, both corners of the cube), references and the scaled metric: tests/_pending_cases.py.  The handle is created with
``BBH_SMALL=0`` so that n <= 64 reaches the cooperative form (its two-round instantiations) instead of the register-resident one.

Every comparison is scaled and absolute and held to 1e-11: |var - ref| / (ysd^2 k(x, x)), |mean - ref| / ysd.  Every observed maximum
is recorded under ``coop_setup/<case id>``.

  test_rounds   n = 1 ... 512: every first round g0 and the two- and four-round instantiations, of a plain d = 20 model (five k-steps:
                two pairs and a single) and of a d = 9 table model in the mixed column layout (three k-steps, the task column in the
                middle, ``numcol`` not the identity)
  test_k_steps  d = 5 ... 32: 2 - 8 k-steps of the seeded stream, odd and even pair counts, full and just-started last k-steps, at
                n = 300 (eight rounds) and n = 200 (four); d = 4, 5, 13 and 33 keep the augmented stream (no k-step saved)
  test_ragged_tiles_and_layout  N = 1, 15, 16, 17, 33 rows of a strided view (``ldx > d``), outputs into views with sentinels behind
                row N; the bits of the 33-row launch"""

import os

import numpy as np
import pytest

import _pending_cases as pc
from _pending_cases import TOL, PendCase, PendModel

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
SWITCHES = ("BBH_SMALL", "BBH_COOP_SEED", "BBH_COOP", "BBH_COOP_SMALL", "BBH_PIPELINE", "BBH_MEAN_VALU", "BBH_SMALL_FORCE")
N_ROWS = 33  # two full tiles of 16 candidates and one row of a third


def seeded_k_steps(model: PendModel) -> int:
    """k-steps of the seeded distance GEMM ``bbh_coop_seed_kds`` gives a Matérn-5/2 model, 0 where it keeps the augmented stream: the
    seeded count must be smaller than the augmented one, and an n <= 256 model takes a four- or two-round instantiation of the
    augmented stream before an eight-round one of the seeded stream."""
    kds = (model.d + 3) // 4
    kds = max(kds, 2) if kds <= 8 else 12
    if kds >= model.kd or 4 * kds < model.d:
        return 0
    if model.nb <= 16:
        if kds <= 3 or (kds <= 6 and model.nb > 8):
            return kds
        if model.kd <= 8:
            return 0
    return kds


@pytest.fixture(scope="module")
def gp():
    from baybe_amd import engine

    keep = {k: os.environ.get(k) for k in SWITCHES}
    try:  # (the switches are read when the handle is created)
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ["BBH_SMALL"] = "0"
        g = engine.HipGP(0)
    finally:
        for k, val in keep.items():
            os.environ.pop(k, None) if val is None else os.environ.__setitem__(k, val)
    yield g
    g.close()


def _np(t):
    return t.cpu().numpy()


def _load(g, model):
    md = model.build()
    g.set_model(md.spec, md.Xt, md.y)
    g.factorize(md.params)
    assert abs(g.ysd - md.om.ysd) <= 1e-13 * md.om.ysd and g.jitter == 0.0, (model.id, g.ysd, md.om.ysd, g.jitter)
    return md


def _ran_as_expected(g, case):
    assert g.posterior_kernel_form() == "cooperative", (case.id, g.posterior_kernel_form())
    assert g.posterior_distance_seeded() == (seeded_k_steps(case.model) > 0), (case.id, seeded_k_steps(case.model))


def _hold(case, devs):
    from conftest import record_deviation

    for what, value in devs.items():
        print(f"{case.id} {what}: observed {value:.3e} (tolerance {TOL:.1e})")
    record_deviation(f"coop_setup/{case.id}", max(devs.values()), TOL)
    failures = [(what, value) for what, value in devs.items() if not value <= TOL]
    assert not failures, (case.id, failures)


def _posterior_case(g, case):
    import torch

    _load(g, case.model)
    m, v = (_np(t) for t in g.posterior(torch.from_numpy(np.array(case.build().cand)).cuda()))
    _ran_as_expected(g, case)
    ref = case.reference()
    _hold(case, {"mean": pc.scaled_mean(m, ref), "var": pc.scaled_var(v, ref)})


ROUND_N = (1, 16, 17, 64, 65, 128, 129, 256, 257, 511, 512)
ROUND_CASES = [PendCase("S1", PendModel("matern52", 20, n), 0, N_ROWS) for n in ROUND_N] + [
    PendCase("S1", PendModel("matern52", 9, n, tasks=3, layout="mixed"), 0, N_ROWS) for n in ROUND_N]


@pytest.mark.parametrize("case", ROUND_CASES, ids=[c.id for c in ROUND_CASES])
def test_rounds(gp, case):
    _posterior_case(gp, case)


K_STEP_D = (4, 5, 8, 9, 12, 13, 15, 20, 23, 25, 32, 33)
K_STEP_CASES = [PendCase("S2", PendModel("matern52", d, n), 0, 17) for n in (300, 200) for d in K_STEP_D]


@pytest.mark.parametrize("case", K_STEP_CASES, ids=[c.id for c in K_STEP_CASES])
def test_k_steps(gp, case):
    _posterior_case(gp, case)


def test_k_step_cases_cover_the_seeded_counts():
    """2 - 8 k-steps of the seeded stream are all met, and d = 4 and d = 33 are not seeded."""
    assert {seeded_k_steps(c.model) for c in K_STEP_CASES} == {0, 2, 3, 4, 5, 6, 7, 8}
    assert all(seeded_k_steps(c.model) == 0 for c in K_STEP_CASES if c.model.d in (4, 33))


RAGGED_MODELS = (PendModel("matern52", 20, 512), PendModel("matern52", 9, 200, tasks=3, layout="mixed"))
RAGGED_CASES = [PendCase("S3", m, 0, N) for m in RAGGED_MODELS for N in (1, 15, 16, 17, N_ROWS)]
RAGGED_FULL = {}  # model -> the 33-row launch


def _raw_posterior(g, wide, N, dtot):
    """``posterior(X, out=...)`` on the first N rows of a strided view, into views of buffers with 64 sentinels behind row N."""
    import torch

    bm, bv = (torch.full((N + 64,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(2))
    X = wide[:N, :dtot]
    assert N == 1 or (X.stride(0) == dtot + 3 and not X.is_contiguous())
    g.posterior(X, out=(bm[:N], bv[:N]))
    bm, bv = _np(bm), _np(bv)
    return bm[:N], bv[:N], np.concatenate([bm[N:], bv[N:]])


@pytest.mark.parametrize("case", RAGGED_CASES, ids=[c.id for c in RAGGED_CASES])
def test_ragged_tiles_and_layout(gp, case):
    import torch

    g, model = gp, case.model
    _load(g, model)
    full = PendCase("S3", model, 0, N_ROWS).build()
    wide = torch.full((N_ROWS, model.dtot + 3), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, : model.dtot] = torch.from_numpy(np.array(full.cand)).cuda()
    if model not in RAGGED_FULL:
        RAGGED_FULL[model] = _raw_posterior(g, wide, N_ROWS, model.dtot)[:2]
    m, v, tail = _raw_posterior(g, wide, case.N, model.dtot)
    _ran_as_expected(g, case)
    assert np.array_equal(tail, np.full(128, SENTINEL)), (case.id, "written behind row N", np.nonzero(tail != SENTINEL)[0][:8])
    fm, fv = RAGGED_FULL[model]
    assert np.array_equal(m, fm[: case.N]) and np.array_equal(v, fv[: case.N]), (case.id, np.abs(m - fm[: case.N]).max(),
                                                                                 np.abs(v - fv[: case.N]).max())
    ref = case.reference()
    _hold(case, {"mean": pc.scaled_mean(m, ref), "var": pc.scaled_var(v, ref)})
