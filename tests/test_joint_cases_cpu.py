"""The case tables of tests/test_joint_batch_gpu.py checked with the oracle alone, for every case:

(a) the regimes are what their labels say: LAPACK's potrf (``oracle.gp_oracle._safe_cholesky``) and the kernels' unblocked
    row-by-row loop, restated in numpy, both take exactly the labelled number of attempts, and every pivot that decides an attempt
    is larger than 1e-10 in magnitude (times the covariance scale of the case: 1 except in the family scaled by 1e-10, whose
    rounding errors scale with it) - seven orders above the rounding of a factorisation of this size;
(b) a wrong jitter level would be seen: for p <= 15 and every level, the reference score of some row of that level moves by more
    than 100 x SCORE_ATOL when the factor is taken at the next level of the ladder instead (most rows move by more than SCORE_ATOL;
    a row whose candidate hardly matters to the fat maximum moves less, which is why the bound is held per level and not per row);
(c) the reference is right: ``qlogei_joint`` agrees with an independent dense restatement to 1e-12 on every scored row;
(d) a case cannot pass on -inf / NaN rows alone: every live, factorisable row has a finite reference score, and they are at least
    85 % of the rows;
(e) the reference resolves the tolerance: with every entry of a row's joint covariance moved by up to 4 ulp (the backward error of a
    factorisation of this size, whatever the order of its operations) the reference score moves by at most SCORE_ATOL / 10.  A
    near-singular pivot before the last row of the factor is divided into the rows after it; where one sample just above best_f
    carries the whole score that is enough to move it by 1e-7, and no factorisation in double precision is "the" reference."""

import numpy as np
import pytest
import scipy.linalg as sla

from _joint_cases import (ATTEMPTS, FAMILIES, JITTERS, SCORE_ATOL, all_cases, dense_score, form_bytes, lapack_attempts,
                          unblocked_attempts, HANDOVER_CASES, S1024_CASE, REGISTER_P, register_cases)

CASES = all_cases()


def test_case_table_covers_what_it_claims():
    assert len({c for c in CASES}) == len(CASES)
    for p in REGISTER_P:
        cs = register_cases(p)
        assert {c.family for c in cs} == {0, 1, 2, 3} and {c.S for c in cs} == {33, 100, 512} and {c.sign for c in cs} == {1.0, -1.0}
    assert [form_bytes(c) for c in HANDOVER_CASES] == [61376, 61488] and 61376 <= 60 * 1024 < 61488
    assert form_bytes(S1024_CASE) > 60 * 1024


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_conditions(case):
    d = case.build()
    ref = case.reference()
    N = case.N
    labelled = np.array([ATTEMPTS[lab] for lab in d.labels])
    factorisable = ~d.is_label("notpd")
    Sig = np.stack([d.sigma(i) for i in range(N)])
    # (a)
    lap = [lapack_attempts(Sig[i]) for i in range(N)]
    assert np.array_equal([a for a, _ in lap], labelled) and np.array_equal([ok for _, ok in lap], factorisable), case.id
    att, ok, deciding = unblocked_attempts(Sig)
    assert np.array_equal(att, labelled) and np.array_equal(ok, factorisable), case.id
    assert deciding.min() > 1e-10 * FAMILIES[case.family][2], (case.id, deciding.min())
    # (d)
    scored = d.scored
    assert np.isfinite(ref[scored]).all() and np.isnan(ref[d.is_label("notpd")]).all() and np.isneginf(ref[d.is_label("masked")]).all()
    assert scored.mean() >= 0.85, (case.id, scored.mean())
    # (c)
    level = labelled - 1
    own = np.array([dense_score(d.joint_mean(i), Sig[i], JITTERS[level[i]], d.z, d.best_f, case.sign) for i in np.nonzero(scored)[0]])
    assert np.abs(own - ref[scored]).max() <= 1e-12, (case.id, np.abs(own - ref[scored]).max())
    # (e)
    from oracle import gp_oracle as go

    rng = np.random.default_rng(case.seed + 99)
    moved = np.zeros(N)
    for i in np.nonzero(scored)[0]:
        R = np.tril(rng.integers(-1, 2, size=Sig[i].shape))
        R = R + np.tril(R, -1).T
        try:
            moved[i] = abs(go.qlogei_joint(d.joint_mean(i), Sig[i] * (1.0 + 4.0 * 2.0**-52 * R), d.z, d.best_f, case.sign) - ref[i])
        except sla.LinAlgError:
            moved[i] = np.inf
    assert moved.max() <= SCORE_ATOL / 10.0, (case.id, int(moved.argmax()), d.labels[int(moved.argmax())], moved.max())
    # (b)
    if case.p <= 15:
        for k in (1, 2, 3):
            rows = np.nonzero(d.is_label(f"jitter{k}"))[0]
            if not len(rows):
                continue
            moved = np.array([abs(dense_score(d.joint_mean(i), Sig[i], 10.0 * JITTERS[k], d.z, d.best_f, case.sign) - ref[i]) for i in rows])
            assert moved.max() > 100.0 * SCORE_ATOL, (case.id, k, moved.max())
            assert np.median(moved) > SCORE_ATOL, (case.id, k, np.median(moved))
