"""The case table of tests/test_factor_ladder_gpu.py checked with the oracle alone, for every case:

(a) the level is what the label says: ``oracle.gp_oracle.GPModel`` (plain models) and the restatement of the two-branch ladder take
    exactly the labelled level, or raise; every failed attempt fails at row b of the first planted pair; for masked models the level
    equals the one BoTorch's order gives - the noisy block through the ladder, then the latent block's Schur complement in the
    target's original scale;
(b) nothing else is near-singular: the second smallest eigenvalue of the matrix the first attempt factorises (the third where two
    pairs are planted) is >= 0.05;
(c) every attempt is decided decisively: the failing pivot of a failed attempt and the smallest pivot of the successful one have
    magnitude >= 0.2 j_k (j_k / ysd^2 in the latent branch), ten million times the rounding of a factorisation of this size;
(d) a wrong level would be seen: with the neighbouring level (10 j_k) forced on the diagonal at least one compared quantity moves by
    more than 100 x TOL;
(e) the reference is right and resolves the tolerance: the float64 reference is within REF_NOISE = 1e-13 (scaled) of a long-double
    restatement on every candidate row and the joint block;
(f) the fit evaluation's cases: the jitter-free Cholesky fails at row b at noise -0.3e-8 and holds at +0.7e-8, for every position."""

import numpy as np
import pytest
import scipy.linalg as sla

import _factor_cases as fc
from _factor_cases import EXHAUSTED, REF_NOISE, TOL

CASES = fc.ladder_cases()


def test_case_table_covers_what_it_claims():
    assert len(set(CASES)) == len(CASES)
    at = {}
    for m in fc.PLAIN_MODELS:
        at.setdefault(m.n, set()).add(m.first[1])
    assert {1, 15, 16, 17, 63} <= at[64] and {63, 64, 65, 69} <= at[70] and {127, 128, 199} <= at[200] and {1023, 1024, 1029} <= at[1030]
    assert {1, 15, 16, 17, 63, 64, 65} <= at[64] | at[70] | at[200]
    assert any(len(m.pairs) == 2 and m.pairs[0][1] // 64 != m.pairs[1][1] // 64 for m in fc.PLAIN_MODELS)
    for m in fc.PLAIN_MODELS + fc.MASKED_MODELS:
        assert {c.k for c in CASES if c.model == m} == {1, 2, 3, EXHAUSTED}
    assert {m.n for m in fc.SOUND_MODELS} == set(at)
    # masked: inside the latent block, directly in front of and directly behind the first latent row, at both sizes; 128 is a block edge
    for n, latent in ((66, 12), (200, 72)):
        bs = {m.first[1] - m.n_noisy for m in fc.MASKED_MODELS if m.n == n and m.latent == latent}
        assert {-1, 0} <= bs and max(bs) > 0, (n, bs)
    assert fc.FactorModel(200, latent=72).n_noisy == 128
    assert -(-1030 // 64) == 17
    assert set(fc.FIT_VARIANTS) == set(at)
    from baybe_amd import _lib

    assert "bbh_last_factor_form" in _lib.SIGNATURES  # (the read-back the GPU module asserts every handle's launch with)


def _first_matrix(case):
    """K = k(X, X) + diag(noise mask) of the case, its mask and ysd."""
    from oracle import gp_oracle as go

    md = case.model.build()
    om = fc.ladder_model(case, forced=np.full(case.model.n, 1e-3))  # (forced: only the kernel matrix is taken from it)
    mask = np.ones(case.model.n) if md.mask is None else md.mask.astype(np.float64)
    K = go.cross_cov(om.spec, om.params, om.Xn, om.Xn) + np.diag(case.noise * mask)
    return K, mask, float(om.ysd)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_conditions(case):
    m, md = case.model, case.model.build()
    ref = case.reference()
    K, mask, ysd = _first_matrix(case)
    diag, level, infos = fc.walk_ladder(K, mask, ysd)
    unit = fc.level_value(1, m.unit_ysd) / 1e-8  # 1, or 1 / ysd^2 in the latent branch
    # (a)
    assert ref.level == case.level and level == case.level, (case.id, ref.level, level, case.level)
    attempts = {0: 0, EXHAUSTED: 4}.get(case.k, case.k)
    assert infos == (m.first[1] + 1,) * attempts if m.pairs else infos == (), (case.id, infos)
    if not m.masked:
        try:
            lad = fc.ladder_model(case)
            assert lad.jitter == ref.level and np.array_equal(lad.L, fc.oracle_model(case).L), case.id
        except sla.LinAlgError:
            assert case.k == EXHAUSTED
    else:
        j1, j2 = fc.schur_ladder(K, mask, ysd)
        if case.k == EXHAUSTED:
            assert j1 is None or j2 is None, (case.id, j1, j2)
        elif m.latent_branch:  # the noisy block is sound; the Schur complement takes j_k in original scale: j_k / ysd^2 here
            assert j1 == 0.0 and j2 == fc.level_value(case.k) and j2 / (ysd * ysd) == case.level, (case.id, j1, j2)
        else:
            assert j1 == case.level, (case.id, j1, j2)
    # (b)
    ev = np.linalg.eigvalsh(K)
    assert ev[max(1, len(m.pairs))] >= 0.05, (case.id, ev[:3])  # (behind the planted directions, one per pair)
    if case.k:
        assert ev[0] < 0.0
    # (c)
    jit = jl = 0.0
    for attempt in range(attempts + (case.k != EXHAUSTED)):
        row, pivot = fc.deciding_pivot(K + np.diag(np.where(mask != 0, jit, jl)))
        last = attempt == attempts
        assert (row == 0) == last, (case.id, attempt, row)
        if case.k:
            assert abs(pivot) >= 0.2 * fc.level_value(min(case.k, 3)) * unit, (case.id, attempt, row, pivot)
        step = 1e-8 * 10**attempt
        if m.latent_branch:
            jl = step / (ysd * ysd)
        else:
            jit = jl = step
    if case.k == EXHAUSTED:
        return
    # (e)
    got = fc.longdouble_reference(case, diag)
    devs = fc.deviations(ref, *[np.asarray(a, dtype=np.float64) for a in got])
    rows = np.nonzero((md.cand[:, None, :] == md.Xt[None, :, :]).all(axis=2))
    devs["train"] = float(np.abs(np.asarray(got[0], dtype=np.float64)[rows[0]] - ref.train[rows[1]]).max() / ref.ysd)
    assert len(rows[0]) >= fc.N_TRAIN_ROWS + 2
    assert max(devs.values()) <= REF_NOISE, (case.id, devs)
    # (d)
    if case.k:
        forced = fc.quantities(fc.ladder_model(case, forced=10.0 * diag), md)
        moved = fc.deviations(ref, forced.mean, forced.var, forced.jmean, forced.jcov, forced.train)
        assert max(moved.values()) >= 100.0 * TOL, (case.id, moved)


FIT_MODELS = fc.PLAIN_MODELS


@pytest.mark.parametrize("model", FIT_MODELS, ids=[m.id for m in FIT_MODELS])
def test_fit_evaluation_cases(model):
    """(f)"""
    from oracle import gp_oracle as go

    case = fc.FactorCase(model, 1)
    K, _, _ = _first_matrix(case)
    K0 = K - case.noise * np.eye(model.n)
    assert fc.deciding_pivot(K0 + fc.FIT_NOISE_FAILS * np.eye(model.n))[0] == model.first[1] + 1
    assert fc.potrf_info(K0 + fc.FIT_NOISE_FAILS * np.eye(model.n))[1] == model.first[1] + 1
    row, pivot = fc.deciding_pivot(K0 + fc.FIT_NOISE_HOLDS * np.eye(model.n))
    assert row == 0 and pivot >= 0.7e-8 and fc.potrf_info(K0 + fc.FIT_NOISE_HOLDS * np.eye(model.n))[1] == 0
    # the sound point behind the failed evaluation: the oracle's data term exists there
    md = model.build()
    from _problems import oracle_params, oracle_spec

    ospec = oracle_spec(md.spec)
    dt = go.data_term(ospec, oracle_params(md.spec, fc.fit_point(model)), go.normalize_inputs(ospec, md.Xt), go.standardize_targets(md.y)[0])
    assert np.isfinite(dt.value)
    for variant in fc.FIT_VARIANTS[model.n]:
        assert len(fc.fit_expected_form(model.n, variant)) >= 1
