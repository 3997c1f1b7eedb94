"""The feasible set of a continuous subspace with linear constraints, as data:

    { c in R^dc : lo <= c <= hi,  E c = e,  G c >= g }

over the continuous comp-rep columns, in the order of ``cont.comp_rep_bounds.columns``.  ``Polytope.from_subspace`` reads
``constraints_lin_eq`` / ``constraints_lin_ineq`` with the semantics of ``ContinuousLinearConstraint.to_botorch``
(baybe/constraints/continuous.py:93-203): ``"<="`` negates the coefficients and the right-hand side, ``"="`` rows go to ``E``.

Host work, O(dc^3), once per recommendation: dependent equality rows are dropped (rank by SVD), the Chebyshev centre of the set in
the reduced coordinates ``c = c0 + Z y`` (``Z`` an orthonormal basis of ``null(E)``) comes from one linear programme.  The two batch
operations - uniform samples (``bbh_polytope_sample``, replacing BoTorch's ``get_polytope_samples``) and Euclidean projections
(``bbh_polytope_project``) - run on the device (csrc/bbh_polytope.hip).
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from baybe_amd.exceptions import IncompatibilityError

MAX_COLUMNS = 32  # MAX_GRADIENT_CONTINUOUS: the columns bbh_posterior_grad differentiates
MAX_ROWS = 16  # equality + inequality rows after normalisation (the multipliers of one projection)
FEASIBILITY_C = 4.0  # BBH_POLY_FEAS_C: the projection meets C (dc + M) eps S_abs, M = 2 dc + mi
_RANK_RTOL = 1e-12


def default_n_steps(dz: int) -> int:
    """Hit-and-run steps per chain: ``max(64, dz^2)`` rounded up to a power of two (KERNELS.md 4.17 has the table it was read from)."""
    need = max(64, int(dz) * int(dz))
    return 1 << (need - 1).bit_length()


@dataclass
class Polytope:
    lo: np.ndarray  # [dc]
    hi: np.ndarray  # [dc]
    E: np.ndarray  # [me, dc] independent rows
    e: np.ndarray  # [me]
    G: np.ndarray  # [mi, dc]
    g: np.ndarray  # [mi]
    c0: np.ndarray = field(default=None)  # [dc] Chebyshev centre (reduced coordinates), an interior point
    Z: np.ndarray = field(default=None)  # [dc, dz] orthonormal basis of null(E)
    radius: float = 0.0  # Chebyshev radius in the reduced coordinates

    def __post_init__(self):
        self.lo = np.ascontiguousarray(self.lo, dtype=np.float64).reshape(-1)
        self.hi = np.ascontiguousarray(self.hi, dtype=np.float64).reshape(-1)
        dc = self.lo.shape[0]
        self.E = np.asarray(self.E, dtype=np.float64).reshape(-1, dc)
        self.e = np.asarray(self.e, dtype=np.float64).reshape(-1)
        self.G = np.ascontiguousarray(np.asarray(self.G, dtype=np.float64).reshape(-1, dc))
        self.g = np.ascontiguousarray(np.asarray(self.g, dtype=np.float64).reshape(-1))
        if self.hi.shape[0] != dc or self.E.shape[0] != self.e.shape[0] or self.G.shape[0] != self.g.shape[0]:
            raise ValueError("Polytope: lo, hi [dc]; E [me, dc], e [me]; G [mi, dc], g [mi]")
        if dc < 1:
            raise ValueError("Polytope: at least one column")
        if dc > MAX_COLUMNS:
            raise IncompatibilityError(
                f"{dc} continuous parameters under linear constraints: the device-side sampler and projection take up to {MAX_COLUMNS} "
                f"of them; use BotorchRecommender beyond that.")
        if not (np.isfinite(self.lo).all() and np.isfinite(self.hi).all()):
            raise IncompatibilityError("Linear constraints on the HIP path need finite bounds on every continuous parameter; "
                                       "use BotorchRecommender for unbounded ones.")
        self._normalise()
        if self.me + self.mi > MAX_ROWS:
            raise IncompatibilityError(
                f"{self.me + self.mi} linear constraint rows ({self.me} independent equalities, {self.mi} inequalities): the device-side "
                f"projection takes up to {MAX_ROWS}; use BotorchRecommender beyond that.")
        self._centre()

    # ---- construction ---------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_subspace(cls, cont) -> "Polytope":
        """From a ``SubspaceContinuous`` or a stand-in with the same attributes; of a constraint only ``parameters``, ``operator``,
        ``coefficients``, ``rhs`` and ``is_interpoint`` are read."""
        bounds = cont.comp_rep_bounds
        names = [str(c) for c in bounds.columns]
        cb = np.asarray(bounds.to_numpy(), dtype=np.float64)
        E, e, G, g = [], [], [], []
        for group in ("constraints_lin_eq", "constraints_lin_ineq"):
            for con in getattr(cont, group, ()) or ():
                if getattr(con, "is_interpoint", False):
                    raise IncompatibilityError(
                        "Interpoint constraints couple the points of a batch; the HIP path constrains every point separately. "
                        "Use BotorchRecommender.")
                op = str(con.operator)
                if op not in ("=", ">=", "<="):
                    raise ValueError(f"'{op}' is not a linear constraint operator (=, >=, <=)")
                coeffs = [float(v) for v in con.coefficients]
                params = [str(p) for p in con.parameters]
                if len(coeffs) != len(params):
                    raise ValueError("The given 'coefficients' list must have one floating point entry for each entry in 'parameters'.")
                mult = -1.0 if op == "<=" else 1.0
                row = np.zeros(len(names))
                for p, v in zip(params, coeffs):
                    if p not in names:
                        raise ValueError(f"The constraint names the parameter '{p}', which is not a continuous parameter of the space.")
                    row[names.index(p)] += mult * v
                (E if op == "=" else G).append(row)
                (e if op == "=" else g).append(mult * float(con.rhs))
        dc = len(names)
        return cls(cb[0], cb[1], np.array(E).reshape(-1, dc), np.array(e), np.array(G).reshape(-1, dc), np.array(g))

    @classmethod
    def from_botorch(cls, bounds, equality_constraints=None, inequality_constraints=None) -> "Polytope":
        """From the arguments of ``botorch.utils.sampling.get_polytope_samples``: ``bounds`` [2, dc] and ``(indices, coefficients,
        rhs)`` triples meaning ``sum coeff x[idx] (= | >=) rhs``."""
        cb = np.asarray(bounds, dtype=np.float64).reshape(2, -1)
        dc = cb.shape[1]

        def rows(triples):
            A, b = [], []
            for idx, coeff, rhs in triples or ():
                row = np.zeros(dc)
                for i, v in zip(np.asarray(idx).reshape(-1).tolist(), np.asarray(coeff, dtype=np.float64).reshape(-1).tolist()):
                    row[int(i)] += v
                A.append(row)
                b.append(float(rhs))
            return np.array(A).reshape(-1, dc), np.array(b)

        E, e = rows(equality_constraints)
        G, g = rows(inequality_constraints)
        return cls(cb[0], cb[1], E, e, G, g)

    @property
    def dc(self) -> int:
        return self.lo.shape[0]

    @property
    def me(self) -> int:
        return self.E.shape[0]

    @property
    def mi(self) -> int:
        return self.G.shape[0]

    @property
    def dz(self) -> int:
        return self.Z.shape[1]

    @property
    def n_rows(self) -> int:
        """M of the feasibility bound: the 2 dc box rows and the inequalities."""
        return 2 * self.dc + self.mi

    @property
    def has_rows(self) -> bool:
        return self.me + self.mi > 0

    def _normalise(self) -> None:
        """Drops dependent equality rows; an inconsistent system is an error."""
        E, e = self.E, self.e
        if E.shape[0]:
            scale = max(1.0, float(np.abs(E).max()))
            keep = []
            for i in range(E.shape[0]):  # a row stays if it raises the rank of the rows kept so far
                s = np.linalg.svd(E[keep + [i]], compute_uv=False)
                if int((s > _RANK_RTOL * scale * max(E.shape)).sum()) > len(keep):
                    keep.append(i)
            sol = np.linalg.lstsq(E[keep], e[keep], rcond=None)[0] if keep else np.zeros(E.shape[1])
            resid = np.abs(E @ sol - e)
            tol = 1e-9 * (np.abs(E) @ np.abs(sol) + np.abs(e) + 1.0)
            if (resid > tol).any():
                raise IncompatibilityError(
                    "The linear equality constraints contradict each other (no point satisfies all of them); the search space is empty.")
            E, e = E[keep], e[keep]
        self.E = np.ascontiguousarray(E.reshape(-1, self.lo.shape[0]))
        self.e = np.ascontiguousarray(e)

    def _centre(self) -> None:
        """Z, the Chebyshev centre c0 and its radius: max r s.t. A y - r |A_i| >= b over the rows of the reduced set."""
        from scipy.optimize import linprog

        dc = self.dc
        if self.me:
            _, _, Vt = np.linalg.svd(self.E, full_matrices=True)
            Z = np.ascontiguousarray(Vt[self.me:].T)
            cp = np.linalg.lstsq(self.E, self.e, rcond=None)[0]
        else:
            Z, cp = np.eye(dc), np.zeros(dc)
        self.Z = Z
        dz = Z.shape[1]
        empty = IncompatibilityError(
            "The linear constraints and the parameter bounds leave no feasible point with room around it (the polytope is empty or has "
            "no interior in the directions the equalities leave free); the HIP path samples and projects inside such a set. "
            "Use BotorchRecommender, or state a flat direction as an equality.")
        if dz == 0:  # the equalities pin the point: answered on the host
            ok = (cp >= self.lo - 1e-9).all() and (cp <= self.hi + 1e-9).all() and (self.G @ cp >= self.g - 1e-9).all()
            if not ok:
                raise empty
            self.c0, self.radius = np.clip(cp, self.lo, self.hi), 0.0
            return
        A = np.vstack([Z, -Z, self.G @ Z])
        b = np.concatenate([self.lo - cp, cp - self.hi, self.g - self.G @ cp])
        norms = np.linalg.norm(A, axis=1)
        flat = norms <= 1e-13 * max(1.0, float(np.abs(A).max()))
        if (b[flat] > 1e-12).any():
            raise empty
        A, b, norms = A[~flat], b[~flat], norms[~flat]
        cost = np.zeros(dz + 1)
        cost[-1] = -1.0
        res = linprog(cost, A_ub=np.hstack([-A, norms[:, None]]), b_ub=-b, bounds=[(None, None)] * dz + [(0.0, None)], method="highs")
        span = max(1.0, float(np.abs(self.hi - self.lo).max()))
        if res.status != 0 or not (res.x[-1] > 1e-10 * span):
            raise empty
        self.c0 = np.ascontiguousarray(cp + Z @ res.x[:dz])
        self.radius = float(res.x[-1])

    # ---- what the kernels read ---------------------------------------------------------------------------------------------------
    def reduced(self) -> dict:
        """The reduced set around c0: ``bl <= Z y <= bu``, ``GZ y >= bg`` (arrays the sampler stages once per workgroup)."""
        return {"Z": np.ascontiguousarray(self.Z), "GZ": np.ascontiguousarray(self.G @ self.Z), "c0": self.c0, "lo": self.lo, "hi": self.hi,
                "bl": self.lo - self.c0, "bu": self.hi - self.c0, "bg": self.g - self.G @ self.c0}

    def rows(self):
        """(R [me + mi, dc], t [me + mi]): the equality rows, then the inequality rows."""
        return np.ascontiguousarray(np.vstack([self.E, self.G])), np.concatenate([self.e, self.g])

    def feasibility_ratio(self, X: np.ndarray, C: float = FEASIBILITY_C) -> np.ndarray:
        """Per row of X [k, dc]: the worst violation over the bound ``C (dc + M) eps S_abs,i`` (<= 1: feasible); inf outside the box."""
        X = np.asarray(X, dtype=np.float64).reshape(-1, self.dc)
        R, t = self.rows()
        out = np.where(((X < self.lo) | (X > self.hi)).any(axis=1), np.inf, 0.0)
        if R.shape[0] == 0:
            return out
        res = X @ R.T - t
        sabs = np.abs(X[:, None, :] * R[None, :, :]).sum(axis=2) + np.abs(t)
        viol = np.abs(res)
        viol[:, self.me:] = np.maximum(-res[:, self.me:], 0.0)
        tol = C * (self.dc + self.n_rows) * np.finfo(np.float64).eps * sabs
        ratio = np.where(viol > 0, viol / np.where(tol > 0, tol, 1e-300), 0.0)
        return np.maximum(out, ratio.max(axis=1))

    # ---- the two device operations ---------------------------------------------------------------------------------------------
    def sample(self, engine, n: int, n_steps: int | None = None, seed: int = 0):
        """``n`` points [n, dc] (device tensor): one hit-and-run chain of ``n_steps`` steps per point (``HipGP.polytope_sample``)."""
        import torch

        if self.dz == 0:
            return torch.from_numpy(np.tile(self.c0, (int(n), 1))).to(engine._dev())
        return engine.polytope_sample(self.reduced(), int(n), default_n_steps(self.dz) if n_steps is None else int(n_steps), int(seed))

    def projector(self, engine):
        """``project(X [k, dc]) -> (X' [k, dc], ok [k])`` on numpy arrays, every row through ``bbh_polytope_project``; counts its calls
        on ``project.calls``."""
        import torch

        R, t = self.rows()
        mu_min = 1e-10 * float((R * R).sum(axis=1).max()) if R.shape[0] else 1.0
        tolf = FEASIBILITY_C * (self.dc + self.n_rows) * float(np.finfo(np.float64).eps)

        def project(X):
            project.calls += 1
            Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64).reshape(-1, self.dc)).to(engine._dev())
            out, status = engine.polytope_project(Xd, self.lo, self.hi, R, t, self.me, tolf, mu_min)
            return out.cpu().numpy(), status.cpu().numpy() == 0

        project.calls = 0
        return project
