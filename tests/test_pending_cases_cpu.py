"""The case tables of tests/test_pending_passes_gpu.py checked with the oracle alone.

For every case (one per model, pending set and candidate count):

(a) the regimes are what the labels say: which candidate rows coincide with a pending point or a training row, which lie 1e-3 from a
    pending point, that no other row coincides with one; the pending set holds grid rows, training rows and rows 1e-3 from training
    rows, in at least three tasks where the model has tasks; p, the number of training blocks and the widths of the variance passes;
(b) the reference resolves the tolerance: the float64 oracle is within 1e-13 (scaled as the device comparison) of a plain
    ``np.longdouble`` restatement - kernel values, column Cholesky, forward substitution, the same formulas - for cross-covariances,
    variances and - in the families whose variance pass is compared, C and E - means (family D's p = 0 pass: a tenth of the tolerance).  The 1e-11 the device is held to is admissible
    against the oracle only under this condition;
(c) the batched reference is the oracle's joint posterior: ``posterior_joint([x; P])`` row by row on a sample of the rows;
(d) the case can fail: with columns shifted by one, with column p left at a previous pending point, with the pending tasks taken as
    0, with one padding row given a unit kernel value, the reference moves by more than 100 tolerances on some scored row.

The tables themselves: every instantiation ``bbh_fused_launch_kd*`` has appears in family A with a ragged n and p = 15; family C has
the pass widths of its table; family D has one model per (F, KD) of ``bbh_coopg_cross_launch``; every family can show every defect
that applies to it."""

import numpy as np
import pytest

import _pending_cases as pc

CASES = pc.unique_cases()


def test_family_a_covers_every_instantiation():
    """4 kinds x 6 KD of the pipelined form and the 4 of the plain form, each with n not a multiple of 16 and p = 15; every n and p of
    the issue's lists; the long nb_ext loop; the plain form under BBH_PIPELINE=0."""
    fam = pc.family_a()
    seen = {}
    for c in fam:
        inst = c.model.windowed_instantiation(pipeline=c.handle != "nopipe")
        seen.setdefault(inst, []).append(c)
    want = {(kd, k, t) for kd in pc.KD_DIMS for k, t in (("matern52", False), ("matern52", True), ("rbf", False), ("matern32", False))}
    want |= {(0, "matern52", False), (0, "matern52", True), (0, "runtime", False), (0, "runtime", True)}
    assert set(seen) == want, set(seen) ^ want
    for inst, cs in seen.items():
        assert any(c.p == 15 and c.model.n % 16 for c in cs), inst
    assert {c.model.n for c in fam} >= {1, 15, 16, 17, 64, 65, 300, 513} and {c.p for c in fam} == {1, 2, 8, 15}
    assert {c.model.d for c in fam} >= {3, 9, 20, 28, 40, 62, 70}
    assert [c.model.kd for c in fam if c.model.d == 70][0] == 18
    for kernel in ("rbf", "matern32"):
        assert {c.model.d for c in fam if c.model.kernel == kernel and not c.model.has_tbl} >= {3, 20, 40}
    assert {c.model.d for c in fam if c.model.tasks == 4 and c.model.kernel == "matern52"} == {9, 20}
    assert any(c.model.scale and not c.model.tasks for c in fam)
    for c in fam:
        if c.model.tasks:
            assert len(set(c.build().tp)) >= 3, c.id
    nopipe = [c for c in fam if c.handle == "nopipe"]
    assert {c.model.windowed_instantiation(True)[0] for c in nopipe} == {2, 4, 6} and all(c.model.windowed_instantiation(False)[0] == 0 for c in nopipe)
    assert any(c.model.n == 513 and c.model.nb + 1 == 37 for c in fam)


def test_family_b_c_d_e_tables():
    assert {c.N for c in pc.family_b()} == {1, 15, 16, 17, 63, 64, 65, 257}
    kd6, tbl = pc.B_MODELS
    assert kd6.kd == 6 and not kd6.has_tbl and tbl.has_tbl and tbl.task_col == tbl.d // 2 and 0 < tbl.task_col < tbl.dtot - 1
    for m in pc.B_MODELS:
        md = m.build()
        assert not np.array_equal(md.lo, np.zeros(m.d)) and not np.array_equal(md.hi, np.ones(m.d))
    # C: the pass widths of the table, KD 4 and 6 over the whole sweep, the other instantiations at n = 257
    models = pc.family_c_models()
    for m in models:
        assert m.pass_widths == pc.C_WIDTHS[m.n] and m.nb == sum(m.pass_widths), m.id
    for kd in (4, 6):
        assert {m.n for m in models if m.kd == kd and m.kernel == "matern52" and not m.tasks} == set(pc.C_SWEEP_N)
    assert {m.kd for m in models if m.n == 257} == {2, 4, 6, 8, 12, 16, 18}
    assert {m.kernel for m in models if m.n == 330} == {"matern52", "rbf", "matern32"} and any(m.tasks and m.n == 513 for m in models)
    assert {(c.p, c.N) for c in pc.family_c()} == {(1, 1), (15, 49), (1, 130), (15, 130)}
    # D: one model per (F, KD) of bbh_coopg_cross_launch, every kind of the generic production, one under the ICM factor
    got = {(pc.D_COOPG_FKD[k], pc.coopg_kd(pc.PendModel(k, d, 60))) for k, d, _ in pc.D_COOPG}
    assert got == {(F, kd) for F in (1, 2, 3, 4) for kd in (2, 4, 6, 8)}
    assert {k for k, _, _ in pc.D_COOPG} >= {"product", "scaled_sum", "three", "nested4", "rq", "piecewise2", "linear", "poly2", "periodic"}
    assert any(T for _, _, T in pc.D_COOPG)
    for k, d, T in pc.D_COOPG:
        m = pc.PendModel(k, d, 60, tasks=T)
        spec = m.build().spec
        assert spec.n_factors == pc.D_COOPG_FKD[k] and pc.expected_p0_form(m, 257) == "cooperative-generic", m.id
    assert [pc.expected_p0_form(m, 257) for m in pc.D_MATERIALISED] == ["materialised"] * 3
    assert pc.coopg_kd(pc.D_MATERIALISED[1]) == 0 and pc.D_MATERIALISED[2].nb > 32
    # E: 15 -> 2 -> 0 -> 1 with different points each time
    assert [p for p, _ in pc.E_STEPS] == [15, 2, 0, 1]
    for m in pc.E_MODELS:
        sets = [pc.PendCase("E", m, p, 130, pend_seed=s).build().P for p, s in pc.E_STEPS]
        assert not np.array_equal(sets[0][:2], sets[1]) and not np.array_equal(sets[1][:1], sets[3]) and not np.array_equal(sets[0][:1], sets[3])
    assert {pc.expected_p0_form(m, 130) for m in pc.E_MODELS} == {"register-resident", "cooperative", "feature-space", "cooperative-generic"}


def test_every_family_can_show_every_defect():
    """Each defect applies to at least one case of each family (the task defect: of each family that has a task model)."""
    for fam in "ABCDE":
        cs = [c for c in pc.all_cases() if c.family == fam]
        assert any(c.p >= 2 and c.N >= 15 for c in cs) and any(c.p >= 1 and c.N >= 15 for c in cs), fam
        assert any(c.model.tasks and c.p >= 1 and c.N >= 15 and c.build().tp.any() for c in cs), fam


def _rows_sample(N):
    return sorted(set(range(0, N, 16)) | set(range(min(N, 11))) | set(range(max(0, N - 11), N)))


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_conditions(case):
    model, md, d, ref = case.model, case.model.build(), case.build(), case.reference()
    N, p, T = case.N, case.p, model.tasks
    # (a)
    assert d.cand.shape == (N, model.dtot) and d.P.shape == (p, model.dtot) and ref.cross.shape == (N, p)
    assert model.nb == 4 * -(-model.n // 64) and sum(model.pass_widths) == model.nb and all(w == 16 for w in model.pass_widths[:-1])
    eq_p = (d.cand[:, None, :] == d.P[None, :, :]).all(axis=2)  # [N, p]
    eq_t = (d.cand[:, None, :] == md.Xt[None, :, :]).all(axis=2).any(axis=1)
    for i, lab in enumerate(d.labels):
        what, _, k = lab.partition(":")
        if what == "pending":
            assert eq_p[i, int(k)], (case.id, i, lab)
        elif what == "train":
            assert np.array_equal(d.cand[i], md.Xt[int(k)]), (case.id, i, lab)
        elif what == "near":
            assert np.allclose(np.abs(d.Uc[i] - d.Up[int(k)]), 1e-3, rtol=0, atol=1e-12) and d.tc[i] == d.tp[int(k)] and not eq_p[i].any()
        elif what == "corner":
            assert set(np.unique(d.Uc[i])) <= {0.0, 1.0} and len(np.unique(d.Uc[i])) == 1
        else:
            assert not eq_p[i].any() and not eq_t[i], (case.id, i, "an ordinary row coincides with a pending or training point")
    if p:
        assert d.labels[0] == "pending:0" and (N < pc.N_FULL or d.labels[-1] == f"pending:{p - 1}")
        assert len({r.tobytes() for r in d.P}) == p, (case.id, "duplicate pending points")
        on_train = (d.Up[:, None, :] == md.Ut[None, :, :]).all(axis=2).any(axis=1)  # (the numerical columns: its task is the pending point's own)
        assert on_train.sum() == sum(1 for j in range(p) if j % 3 == 1 and j // 3 < model.n), case.id
        if p >= 3:
            k = (0 + 5 * case.pend_seed) % model.n
            assert np.allclose(np.abs(d.Up[2] - md.Ut[k]), 1e-3, rtol=0, atol=1e-12), case.id
    if T and p >= 3:
        assert len(set(d.tp)) >= 3 and (N < 15 or all((d.tc != t).any() for t in set(d.tp))), case.id
    if T:
        assert set(d.tc) <= set(range(T)) and (N < T or len(set(d.tc)) == T)
    # (b)
    rows = None if (model.n <= 600 or N <= 65) else np.array(_rows_sample(N))
    sub = ref if rows is None else pc.Reference(ref.mean[rows], ref.var[rows], ref.cross[rows], ref.mean_p, ref.cov_pp, ref.kxx[rows], ref.kpp, ref.ysd)
    mean_ld, var_ld, cross_ld = pc.longdouble_reference(case, rows)
    noise = {"cross": pc.scaled_cross(cross_ld.astype(np.float64), sub), "var": pc.scaled_var(var_ld.astype(np.float64), sub),
             "mean": pc.scaled_mean(mean_ld.astype(np.float64), sub)}
    print(case.id, {k: f"{v:.1e}" for k, v in noise.items()})
    # (the mean is compared on the device in the families with a variance pass only: there its own condition holds as well)
    held = [v for k, v in noise.items() if k != "mean" or case.family in "CE"]
    assert max(held) <= pc.REF_NOISE, (case.id, noise)
    # (family D compares the mean of its p = 0 pass too.  Its models keep ``fixed_theta``'s noise e^-5, where the float64 oracle's mean
    # of the low-rank kinds - piecewise, Linear, Polynomial - is some 1e-13 from the restatement: held to a tenth of the tolerance,
    # which leaves the device nine tenths of it; tests/_generic_variance_cases.py has these kinds at noise 0.2 and within 1e-13)
    if case.family == "D":
        assert noise["mean"] <= pc.TOL / 10.0, (case.id, noise)
    # (c)
    for i in _rows_sample(N):
        mj, cj = md.om.posterior_joint(np.vstack([d.cand[i:i + 1], d.P]))
        one = pc.Reference(mj[:1], cj[:1, 0], cj[:1, 1:], mj[1:], cj[1:, 1:], ref.kxx[i:i + 1], ref.kpp, ref.ysd)
        dev = max(pc.scaled_cross(ref.cross[i:i + 1], one), pc.scaled_var(ref.var[i:i + 1], one), pc.scaled_cov_pp(ref.cov_pp, one) if p else 0.0)
        assert dev <= pc.REF_NOISE, (case.id, i, dev)
        # (means: the same products added in the order of another matrix shape; a hundredth of what the pending means are held to)
        dev = max(pc.scaled_mean(ref.mean[i:i + 1], one), float(np.abs(ref.mean_p - one.mean_p).max() / ref.ysd) if p else 0.0)
        assert dev <= pc.PEND_MEAN_ATOL / 100.0, (case.id, i, dev)
    for i in np.nonzero(d.rows("pending"))[0]:  # the cross column of a row that is a pending point: that point's posterior variance
        j = int(d.labels[i].split(":")[1])
        one = pc.Reference(ref.mean[i:i + 1], ref.var[i:i + 1], ref.cross[i:i + 1, j:j + 1], None, None, ref.kxx[i:i + 1], ref.kpp[j:j + 1], ref.ysd)
        assert pc.scaled_cross(ref.var[i:i + 1, None], one) <= pc.REF_NOISE and pc.scaled_cross(ref.cov_pp[j:j + 1, j:j + 1], one) <= pc.REF_NOISE
    # (d)
    if p and N >= 15:
        for defect in pc.DEFECTS:
            bad = pc.defective_cross(case, defect)
            if bad is None:
                assert (defect == "task0" and (not T or not d.tp.any()) or defect == "shift" and p < 2
                        or defect == "stale" and model.n == 1), (case.id, defect)
                continue
            moved = pc.scaled_cross(bad, ref)
            assert moved > 100.0 * pc.TOL, (case.id, defect, moved)
