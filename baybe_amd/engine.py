"""Host driver of the HIP GP engine: one handle = one single-output GP on one MI355X.

Mirrors, step by step, what BayBE triggers inside BoTorch on the recommend() path
(SURVEY.md §3.2-3.4): fit_gpytorch_mll -> posterior -> qLogEI -> optimize_acqf_discrete.
PyTorch-ROCm tensors are used purely as device containers (``data_ptr()``); all arithmetic
happens in libbaybe_hip through the C-ABI of ``include/baybe_hip.h``.
"""

from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
import threading
from dataclasses import dataclass

import numpy as np
from scipy import optimize as sopt

from baybe_amd import _lib
from baybe_amd._lib import HipError, HipUnavailableError
from baybe_amd.gp_spec import (
    FastObjective,
    GPParams,
    GPSpec,
    initial_params,
    sample_params_from_priors,
    objective_from_data_term,
    pack_raw,
    raw_bounds,
    theta_from_params,
    unpack_raw,
)

MAX_PENDING = _lib.MAX_PENDING
MAX_PENDING_BIG = _lib.MAX_PENDING_BIG


def _dp(a: np.ndarray):
    return a.ctypes.data_as(_lib.c_double_p)


_SOBOL_MAXBIT = 30
_SOBOL_STATE: dict = {}  # dimension -> unscrambled direction numbers [q, 30] (int64 numpy), as the engine initialises them
_FAST_SOBOL = None  # None: unchecked, True / False after the first use


def _sobol_uniform_engine(S: int, q: int, seed: int):
    """[S, q] scrambled Sobol points from torch's engine itself (float64 tensor)."""
    import torch

    return torch.quasirandom.SobolEngine(dimension=q, scramble=True, seed=int(seed)).draw(S, dtype=torch.float64)


def _sobol_uniform_fast(S: int, q: int, seed: int):
    """The same points without the engine's per-dimension loops: torch's generator draws the scrambling bits in the engine's
    order (``SobolEngine._scramble``: the shift bits [q, 30], then the lower-triangular matrices [q, 30, 30]), the library's
    host code scrambles the direction numbers and walks the Gray-code sequence (``bbh_sobol_scramble`` / ``bbh_sobol_draw``:
    integer arithmetic, bitwise the engine's points).  768 dimensions x 2048 points: 25 ms -> 4 ms on the GPU box's host."""
    import torch

    lib = _lib.load_library()
    state0 = _SOBOL_STATE.get(q)
    if state0 is None:
        st = torch.zeros(q, _SOBOL_MAXBIT, dtype=torch.long)
        torch._sobol_engine_initialize_state_(st, q)
        state0 = _SOBOL_STATE[q] = st.numpy().copy()
    g = torch.Generator()
    g.manual_seed(int(seed))
    shift_bits = torch.randint(2, (q, _SOBOL_MAXBIT), generator=g).numpy()
    ltm = np.ascontiguousarray(torch.randint(2, (q, _SOBOL_MAXBIT, _SOBOL_MAXBIT), generator=g).numpy())
    shift = np.ascontiguousarray(shift_bits @ (np.int64(1) << np.arange(_SOBOL_MAXBIT, dtype=np.int64)))
    state = state0.copy()
    p64 = _lib.c_int64_p
    if lib.bbh_sobol_scramble(state.ctypes.data_as(p64), ltm.ctypes.data_as(p64), q) != 0:
        raise RuntimeError("bbh_sobol_scramble failed")
    u = np.empty((S, q), dtype=np.float64)
    if lib.bbh_sobol_draw(state.ctypes.data_as(p64), shift.ctypes.data_as(p64), S, q, _dp(u)) != 0:
        raise RuntimeError("bbh_sobol_draw failed")
    return torch.from_numpy(u)


def _fast_sobol_usable() -> bool:
    """The fast path uses two private torch entry points and mirrors ``SobolEngine._scramble``: the first use compares it with
    the engine on three small cases and falls back to the engine for good on any difference (``BBH_FAST_SOBOL=0`` forces that)."""
    global _FAST_SOBOL
    if _FAST_SOBOL is None:
        import os

        import torch

        ok = os.environ.get("BBH_FAST_SOBOL", "1") != "0"
        try:
            for S, q, seed in ((9, 1, 3), (33, 7, 123456), (130, 41, 999)) if ok else ():
                ok = ok and torch.equal(_sobol_uniform_fast(S, q, seed), _sobol_uniform_engine(S, q, seed))
        except Exception:  # noqa: BLE001
            ok = False
        _FAST_SOBOL = bool(ok)
    return _FAST_SOBOL


def sobol_normal_base_samples(S: int, q: int, seed: int) -> np.ndarray:
    """Base samples of botorch's SobolQMCNormalSampler: scrambled Sobol (torch's engine, the same
    one BoTorch uses) -> v = 0.5 + (1 - eps)(u - 0.5) -> sqrt(2) erfinv(2 v - 1).  [S, q] fp64."""
    import torch

    # The engine's scrambling runs a few tiny tensor ops (tril of a [q, 30, 30] matrix ...); with torch's
    # intra-op pool at its default size each of them wakes every host thread - 17 ms per engine on the
    # 128-thread GPU box, 1.3 ms on one thread.  The values do not depend on the thread count.
    nthreads = torch.get_num_threads()
    try:
        torch.set_num_threads(1)
        u = _sobol_uniform_fast(S, q, seed) if _fast_sobol_usable() else _sobol_uniform_engine(S, q, seed)
        if S * q >= 1 << 18:  # the normal transform of a pruning draw (2048 x 768 values) on a few threads: elementwise, same values
            torch.set_num_threads(min(8, nthreads))
        v = 0.5 + (1 - torch.finfo(torch.float64).eps) * (u - 0.5)
        return (torch.erfinv(2 * v - 1) * math.sqrt(2)).numpy().copy()
    finally:
        torch.set_num_threads(nthreads)


_FIT_TLS = threading.local()  # .stream: the torch stream fits started from this thread enqueue on (private_fit_stream)
_FIT_STREAMS: dict = {}
_FIT_POOL = None


@contextlib.contextmanager
def private_fit_stream(device: int, slot: int):
    """``HipGP.fit`` calls made by this thread inside the block run on a stream of their own (one per (device, slot), created once)."""
    import torch

    key = (int(device), int(slot))
    st = _FIT_STREAMS.get(key)
    if st is None:
        st = _FIT_STREAMS[key] = torch.cuda.Stream(device=int(device))
    prev = getattr(_FIT_TLS, "stream", None)
    _FIT_TLS.stream = st
    try:
        yield st
    finally:
        _FIT_TLS.stream = prev


def fit_side_by_side(jobs, device: int = 0):
    """Run the callables ``jobs`` (each one fits one model) on host threads, each with a private stream: the results in order.
    One shared pool of four threads (``baybe/surrogates/composite.py:101-134`` fits its targets one after the other)."""
    global _FIT_POOL
    jobs = list(jobs)
    if len(jobs) <= 1 or os.environ.get("BBH_FIT_SIDE_BY_SIDE", "1") == "0":
        return [job() for job in jobs]
    import torch

    if not torch.cuda.is_available():  # (no device, no streams: the CPU test double of the handle fits in sequence)
        return [job() for job in jobs]
    if _FIT_POOL is None:
        from concurrent.futures import ThreadPoolExecutor

        _FIT_POOL = ThreadPoolExecutor(max_workers=4, thread_name_prefix="bbh-fit")

    def run(slot, job):
        _FIT_TLS.no_global_generator = True
        try:
            with private_fit_stream(device, slot):
                return job()
        finally:
            _FIT_TLS.no_global_generator = False

    futures = [_FIT_POOL.submit(run, k % 4, job) for k, job in enumerate(jobs)]
    results, rerun = [], False
    for f in futures:  # (every job is waited for before anything is decided: none may still be running when the sequence starts)
        try:
            results.append(f.result())
        except _FitNeedsTheGlobalGenerator:
            results.append(None)
            rerun = True
    if rerun:
        # a fit wants torch's global generator: side by side its state would depend on which thread draws first.  Nothing has drawn
        # from it yet (the parallel attempts started from the deterministic prior modes), so the whole group is fitted again in order
        return [job() for job in jobs]
    return results


_NATIVE_SOBOL = None  # None: unchecked, True / False after the first use


def _sobol_state0(q: int) -> np.ndarray:
    """Unscrambled direction numbers [q, 30] as torch's engine initialises them (cached per dimension count)."""
    import torch

    state0 = _SOBOL_STATE.get(q)
    if state0 is None:
        st = torch.zeros(q, _SOBOL_MAXBIT, dtype=torch.long)
        torch._sobol_engine_initialize_state_(st, q)
        state0 = _SOBOL_STATE[q] = st.numpy().copy()
    return state0


def sobol_normal_native(S: int, q: int, seed: int) -> np.ndarray:
    """``sobol_normal_base_samples`` by the library's host code alone (``bbh_sobol_normal``: MT19937 scrambling bits, Gray-code walk,
    inverse error function) - the CPU twin of the device draw, equal to the torch path up to the last bits of erfinv."""
    lib = _lib.load_library()
    state0 = _sobol_state0(q)
    out = np.empty((S, q), dtype=np.float64)
    if lib.bbh_sobol_normal(state0.ctypes.data_as(_lib.c_int64_p), int(seed) & 0xFFFFFFFFFFFFFFFF, S, q, _dp(out)) != 0:
        raise RuntimeError("bbh_sobol_normal failed")
    return out


def _native_sobol_usable() -> bool:
    """The native draw restates torch's CPU generator (MT19937, one 32-bit output per ``randint`` element) and mirrors
    ``SobolEngine._scramble``: the first use compares it with the engine path on three small cases (a wrong bit anywhere gives
    unrelated points, so 1e-13 decides) and falls back to the host path for good on any difference (``BBH_NATIVE_SOBOL=0`` forces that)."""
    global _NATIVE_SOBOL
    if _NATIVE_SOBOL is None:
        import os

        ok = os.environ.get("BBH_NATIVE_SOBOL", "1") != "0"
        try:
            for S, q, seed in ((9, 1, 3), (33, 7, 123456), (130, 41, 999)) if ok else ():
                ok = ok and bool(np.allclose(sobol_normal_native(S, q, seed), sobol_normal_base_samples(S, q, seed), rtol=1e-13, atol=0))
        except Exception:  # noqa: BLE001
            ok = False
        _NATIVE_SOBOL = bool(ok)
    return _NATIVE_SOBOL


def draw_sampler_seed() -> int:
    """MCSampler seed when none is given: ``torch.randint(0, 1000000, (1,))`` from torch's global
    RNG at the first acquisition evaluation (so ``active_settings.random_seed`` governs it)."""
    import torch

    return int(torch.randint(0, 1000000, (1,)).item())


# ---- scipy's L-BFGS-B without scipy's per-evaluation wrappers -----------------------------------------------------------------
# ``scipy.optimize.minimize(method="L-BFGS-B")`` is what ``botorch.fit.fit_gpytorch_mll`` runs, and the iterates have to stay
# scipy's.  Its driver (``_minimize_lbfgsb``) is a short loop around the compiled reverse-communication routine ``setulb``;
# around every objective evaluation it puts ``ScalarFunction`` / ``MemoizeJac`` bookkeeping (array comparisons, copies, lowest-value
# tracking): ~25 us per evaluation - a quarter of an evaluation of a small model (0.09 ms on the device).  The loop
# below is that driver with the evaluation called directly: same routine, same work arrays, same stopping logic, same messages -
# bitwise the same iterates (``tests/test_host_logic_cpu.py::test_lean_lbfgsb_driver_is_scipys``).  ``setulb`` is a private
# interface: the first use checks the lean driver against ``minimize`` on a small problem and falls back to ``minimize`` for good
# if they differ in any bit or the call fails (another scipy version).
_LEAN_LBFGSB = None  # None: unchecked, True / False after the first use


class _OptResult:
    __slots__ = ("x", "fun", "nit", "nfev", "status", "message")

    def __init__(self, x, fun, nit, nfev, status, message):
        self.x, self.fun, self.nit, self.nfev, self.status, self.message = x, fun, nit, nfev, status, message


def _lbfgsb_lean(fun, x0, bounds, maxiter, maxcor=10, ftol=2.2204460492503131e-09, gtol=1e-5, maxfun=15000, maxls=20):
    from scipy.optimize import _lbfgsb_py as lb

    m = maxcor
    factr = ftol / np.finfo(float).eps
    x0 = np.asarray(x0, dtype=np.float64).ravel()
    n = x0.shape[0]
    nbd = np.zeros(n, np.int32)
    low, up = np.zeros(n, np.float64), np.zeros(n, np.float64)
    if bounds is not None:
        lo = np.array([-np.inf if b[0] is None else b[0] for b in bounds], dtype=np.float64)
        hi = np.array([np.inf if b[1] is None else b[1] for b in bounds], dtype=np.float64)
        if (lo > hi).any():
            raise ValueError("LBFGSB - one of the lower bounds is greater than an upper bound.")
        x0 = np.clip(x0, lo, hi)
        for i in range(n):
            has_lo, has_hi = np.isfinite(lo[i]), np.isfinite(hi[i])
            if has_lo:
                low[i] = lo[i]
            if has_hi:
                up[i] = hi[i]
            nbd[i] = (2 if has_hi else 1) if has_lo else (3 if has_hi else 0)
    x = np.array(x0, dtype=np.float64)
    f = np.array(0.0, dtype=np.int32)
    g = np.zeros((n,), dtype=np.int32)
    wa = np.zeros(2 * m * n + 5 * n + 11 * m * m + 8 * m, np.float64)
    iwa = np.zeros(3 * n, dtype=np.int32)
    task, ln_task = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    lsave, isave, dsave = np.zeros(4, dtype=np.int32), np.zeros(44, dtype=np.int32), np.zeros(29, dtype=np.float64)
    nit = nfev = 0
    while True:
        g = np.asarray(g, dtype=np.float64)
        lb._lbfgsb.setulb(m, x, low, up, nbd, f, g, factr, gtol, wa, iwa, task, lsave, isave, dsave, maxls, ln_task)
        if task[0] == 3:  # f and g at the current x
            f, g = fun(np.copy(x))
            nfev += 1
        elif task[0] == 1:  # new iteration
            nit += 1
            if nit >= maxiter:
                task[0], task[1] = 5, 504
            elif nfev > maxfun:
                task[0], task[1] = 5, 502
        else:
            break
    status = 0 if task[0] == 4 else (1 if (nfev > maxfun or nit >= maxiter) else 2)
    return _OptResult(x, f, nit, nfev, status, lb.status_messages[task[0]] + ": " + lb.task_messages[task[1]])


def _lean_lbfgsb_usable() -> bool:
    global _LEAN_LBFGSB
    if _LEAN_LBFGSB is None:
        try:
            A = np.array([[3.0, 0.5, 0.1], [0.5, 2.0, 0.3], [0.1, 0.3, 1.5]])
            b = np.array([1.0, -2.0, 0.5])

            def probe(x):
                return float(0.5 * x @ A @ x - b @ x + 0.1 * np.log1p(x @ x)), A @ x - b + 0.2 * x / (1.0 + x @ x)

            bnd = [(None, None), (-0.1, None), (0.25, 0.25)]
            x0 = np.array([0.7, -0.4, 0.2])
            ref = sopt.minimize(probe, x0, jac=True, method="L-BFGS-B", bounds=bnd, options={"maxiter": 50})
            got = _lbfgsb_lean(probe, x0, bnd, 50)
            _LEAN_LBFGSB = bool(np.array_equal(ref.x, got.x) and ref.fun == got.fun and ref.nit == got.nit and ref.nfev == got.nfev
                                and ref.status == got.status and str(ref.message) == got.message)
        except Exception:  # noqa: BLE001  (another scipy: private interface changed)
            _LEAN_LBFGSB = False
    return _LEAN_LBFGSB


def lbfgsb_minimize(fun, x0, bounds, maxiter):
    """``scipy.optimize.minimize(fun, x0, jac=True, method="L-BFGS-B", bounds=bounds, options={"maxiter": maxiter})`` - through the
    lean driver above when it reproduces scipy bit for bit here (``BBH_LEAN_LBFGSB=0`` forces ``minimize``)."""
    if os.environ.get("BBH_LEAN_LBFGSB", "1") != "0" and _lean_lbfgsb_usable():
        return _lbfgsb_lean(fun, x0, bounds, maxiter)
    return sopt.minimize(fun, x0, jac=True, method="L-BFGS-B", bounds=bounds, options={"maxiter": maxiter})


@dataclass
class FitInfo:
    params: GPParams
    fun: float
    nit: int
    nfev: int
    status: int
    message: str


@dataclass
class GreedyResult:
    indices: list  # candidate positions, in selection order
    values: list  # acquisition value of each greedy step


class ModelFittingError(RuntimeError):
    """Hyper-parameter fit / factorisation failed (mirrors baybe.exceptions.ModelFittingError)."""


class _FitNeedsTheGlobalGenerator(ModelFittingError):
    """Raised inside ``fit_side_by_side`` by a fit that would have to draw from torch's global generator (a retry from re-sampled
    hyper-parameters, random start values of a free task factor): the group is then fitted in sequence, so that the generator is
    consumed in the reference's order (surrogates/composite.py:101-134 fits target by target)."""


# Device handles of closed / collected HipGP objects, per device ordinal: a backtesting run creates (and drops) one
# model per scenario case (``simulate_scenarios`` deep-copies the campaign, simulation/scenarios.py:296); re-using the
# handle keeps its streams, events, workspaces and grow-only device buffers instead of paying hipMalloc / hipFree per case.
_HANDLE_POOL: dict = {}
_HANDLE_POOL_MAX = 8  # idle handles kept per device
_POOL_KEEP_BYTES = 64 << 20  # per buffer of an idle handle (bbh_trim)
pool_stats = {"created": 0, "reused": 0}


def _pool_key(device: int):
    """A handle reads its A/B switches (``BBH_*`` environment variables) when it is created: handles are
    only handed on between objects created under the same switches."""
    import os

    return (int(device), tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("BBH_"))))


def _acquire_handle(lib, device: int):
    free = _HANDLE_POOL.get(_pool_key(device))
    if free:
        pool_stats["reused"] += 1
        return free.pop()
    h = C.c_void_p()
    rc = lib.bbh_create(int(device), C.byref(h))
    if rc != 0:
        raise HipUnavailableError(
            f"bbh_create(device={device}) failed with {rc}: no usable HIP device. "
            "This path has no CPU fallback."
        )
    pool_stats["created"] += 1
    return h


def drain_handle_pool():
    """Destroy the idle device handles (tests; before a process gives its device away)."""
    lib = _lib.load_library()
    for free in _HANDLE_POOL.values():
        while free:
            lib.bbh_destroy(free.pop())


class HipGP:
    """A GP surrogate living on one HIP device.

    The object can be copied and pickled (``copy.deepcopy`` of campaigns / surrogates is what the reference's
    backtesting drivers do: ``simulation/core.py:124``, ``scenarios.py:296``, ``transfer_learning.py:78``,
    ``surrogates/composite.py:54``): the copy carries the model description, the training data and the fitted
    hyper-parameters - not the device handle - and re-creates its device state (handle from the pool, upload,
    factorisation with the same hyper-parameters) the first time it is used."""

    def __init__(self, device: int = 0):
        self._libobj = _lib.load_library()
        self._handle = _acquire_handle(self._libobj, device)
        self._pool_key = _pool_key(device)
        self.device = int(device)
        self.spec: GPSpec | None = None
        self.params: GPParams | None = None
        self.n = 0
        self.ybar = 0.0
        self.ysd = 1.0
        self.jitter = 0.0
        self._comm = None  # (rank, world) once bbh_comm_init has run on this handle
        self._model_args = None  # (noise_mask, standardization) of the last set_model: what a copy needs to rebuild
        self._X_train = self._y_train = None

    # ---- plumbing -------------------------------------------------------------------------
    @property
    def _lib(self):
        """The bound shared library (loaded on first use in a copied / unpickled object)."""
        if self._libobj is None:
            self._libobj = _lib.load_library()
        return self._libobj

    @property
    def _h(self):
        """The device handle; a copied / unpickled object builds its device state here, on first use."""
        if self._handle is None and getattr(self, "_restorable", False):
            self._restore()
        return self._handle

    def close(self):
        if getattr(self, "_handle", None):
            key = self._pool_key
            if self._comm is not None or len(_HANDLE_POOL.setdefault(key, [])) >= _HANDLE_POOL_MAX:
                self._lib.bbh_destroy(self._handle)  # a handle that owns a communicator is not handed on
            else:  # back to its defaults: legacy stream, no timing; buffers above 64 MB are released (an idle handle must not pin HBM)
                self._lib.bbh_set_stream(self._handle, None)
                self._lib.bbh_set_slice_rows(self._handle, 0)
                self._lib.bbh_timing_enable(self._handle, 0)
                self._lib.bbh_trim(self._handle, _POOL_KEEP_BYTES)
                _HANDLE_POOL[key].append(self._handle)
            self._handle = None
        self._restorable = False

    # ---- copies ---------------------------------------------------------------------------
    def __getstate__(self):
        return {
            "device": self.device, "spec": self.spec, "params": self.params, "n": self.n, "ybar": self.ybar,
            "ysd": self.ysd, "jitter": self.jitter, "X_train": self._X_train, "y_train": self._y_train,
            "model_args": self._model_args,
        }

    def __setstate__(self, st):
        self._libobj = None
        self._handle = None
        self.device, self.spec, self.params = st["device"], st["spec"], st["params"]
        self.n, self.ybar, self.ysd, self.jitter = st["n"], st["ybar"], st["ysd"], st["jitter"]
        self._X_train, self._y_train, self._model_args = st["X_train"], st["y_train"], st["model_args"]
        self._comm = None
        self._restorable = True

    def _restore(self):
        self._restorable = False
        self._handle = _acquire_handle(self._lib, self.device)
        self._pool_key = _pool_key(self.device)
        if self.spec is not None and self._X_train is not None:
            params = self.params
            mask, std = self._model_args or (None, None)
            self.set_model(self.spec, self._X_train, self._y_train, noise_mask=mask, standardization=std)
            if params is not None:
                self.factorize(params)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc < 0:
            msg = self._lib.bbh_last_error(self._h)
            raise HipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
        return rc

    def _torch(self):
        import torch

        return torch

    def _dev(self):
        return self._torch().device("cuda", self.device)

    def use_current_torch_stream(self):
        """Enqueue on torch's current stream of this device (containers and kernels then share
        one queue; the default is the legacy null stream, which torch's default stream is)."""
        torch = self._torch()
        self._stream_ptr = int(torch.cuda.current_stream(self.device).cuda_stream)
        self._check(self._lib.bbh_set_stream(self._h, C.c_void_p(self._stream_ptr)), "bbh_set_stream")

    def selftest(self):
        self._check(self._lib.bbh_selftest(self._h), "bbh_selftest")

    # ---- model ----------------------------------------------------------------------------
    def set_model(self, spec: GPSpec, X_train: np.ndarray, y_train: np.ndarray, noise_mask: np.ndarray | None = None,
                  standardization: tuple | None = None):
        """``noise_mask`` [n] (0 = noise-free latent value) and ``standardization`` = (ybar, ysd) are
        used by the qLogNEHVI machinery (model conditioned on sampled baseline values)."""
        X = np.ascontiguousarray(X_train, dtype=np.float64)
        y = np.ascontiguousarray(np.asarray(y_train, dtype=np.float64).reshape(-1))
        if X.ndim != 2 or X.shape[1] != spec.d or X.shape[0] != y.shape[0]:
            raise ValueError("X_train must be [n, d] and y_train [n]")
        desc = _lib.ModelDesc(
            _lib.KERNEL_KINDS[spec.kernel],
            spec.d,
            -1 if spec.task_idx is None else int(spec.task_idx),
            int(spec.n_tasks),
            1 if spec.use_outputscale else 0,
            _lib.CRITERIA[spec.criterion],
            1 if (getattr(spec, "hadamard", False) and spec.n_tasks > 1) else 0,
        )
        factors = getattr(spec, "factors", None)
        if factors:  # composite kernel: ProductKernel / AdditiveKernel of stationary factors
            desc.n_factors = len(factors)
            desc.combine = {"product": 0, "sum": 1, "grouped": 2}[spec.combine]
            for k, f in enumerate(factors):
                desc.factor_kind[k] = _lib.KERNEL_KINDS[f.kernel]
                desc.factor_scaled[k] = 1 if f.scaled else 0
                desc.factor_group[k] = int(getattr(f, "group", 0))
        lo = np.ascontiguousarray(spec.lo, dtype=np.float64)
        hi = np.ascontiguousarray(spec.hi, dtype=np.float64)
        if lo.shape[0] != spec.d or hi.shape[0] != spec.d:
            raise ValueError("spec.lo / spec.hi must have one entry per comp-rep column")
        if spec.kernel == "rff":
            spec = self._with_rff_weights(spec)
        mask_p = None
        if noise_mask is not None:
            mask = np.ascontiguousarray(noise_mask, dtype=np.uint8)
            mask_p = mask.ctypes.data_as(C.POINTER(C.c_uint8))
        given, yb, ys = (1, float(standardization[0]), float(standardization[1])) if standardization else (0, 0.0, 1.0)
        with self._on_thread_stream():  # (the uploads complete inside the call: bbh_set_model_ex synchronises its stream)
            self._check(
                self._lib.bbh_set_model_ex(self._h, C.byref(desc), X.shape[0], _dp(X), _dp(y), _dp(lo), _dp(hi), mask_p,
                                           given, yb, ys),
                "bbh_set_model_ex",
            )
        a, b = C.c_double(), C.c_double()
        self._check(self._lib.bbh_get_standardization(self._h, C.byref(a), C.byref(b)), "bbh_get_standardization")
        self.spec, self.n, self.ybar, self.ysd = spec, X.shape[0], a.value, b.value
        self.params = None
        self._X_train = X
        self._y_train = y
        self._model_args = (None if noise_mask is None else np.array(noise_mask, dtype=np.uint8),
                            None if not standardization else (float(standardization[0]), float(standardization[1])))

    def _with_rff_weights(self, spec: GPSpec) -> GPSpec:
        """The frequencies of an RFF kernel go to the handle before the model: drawn here when the spec carries none - gpytorch's
        ``RFFKernel._init_weights`` draws ``torch.randn(d, D)`` (global generator, the lengthscale's dtype) at the first forward of a
        fit, over the kernel's active columns -, and kept on a copy of the spec so that copies / re-created handles use the same ones."""
        import copy

        from baybe_amd.exceptions import IncompatibleSurrogateError  # (BayBE's own class where it is importable)

        if spec.factors or spec.n_tasks > 1 or spec.task_idx is not None or spec.criterion != "mll":
            raise IncompatibleSurrogateError("On the HIP path the RFF kernel is the single kernel of a single-task model fitted by its "
                                             "marginal likelihood (alone or in a ScaleKernel).")
        D = int(spec.rff_num_samples or 0)
        if D < 1:
            raise ValueError("rff_num_samples must be at least 1")  # (kernels/basic.py:183-200 validates the same)
        if D > _lib.MAX_RFF_SAMPLES:
            raise IncompatibleSurrogateError(f"RFFKernel(num_samples={D}): the HIP path holds up to {_lib.MAX_RFF_SAMPLES} frequencies "
                                             f"(a {2 * _lib.MAX_RFF_SAMPLES} x {2 * _lib.MAX_RFF_SAMPLES} feature-space system).")
        mask = spec.active_mask(0)
        d_act = spec.dn if mask is None else int(mask.sum())
        if spec.rff_weights is None:
            spec = copy.copy(spec)
            spec.rff_weights = self._torch().randn(d_act, D, dtype=self._torch().float64).numpy().copy()
        W = np.asarray(spec.rff_weights, dtype=np.float64)
        if W.shape != (d_act, D):
            raise ValueError(f"rff_weights must be [{d_act}, {D}] (active numerical columns x num_samples)")
        full = np.zeros((spec.dn, D))  # (columns the kernel does not act on: zero frequencies - their pinned lengthscale is immaterial)
        full[np.arange(spec.dn) if mask is None else np.flatnonzero(mask)] = W
        self._check(self._lib.bbh_set_rff_weights(self._h, _dp(np.ascontiguousarray(full)), spec.dn, D), "bbh_set_rff_weights")
        return spec

    def data_term(self, params: GPParams):
        """Device data term (MLL or LOO) and its gradient in theta layout; (None, None) if the
        train covariance is not positive definite."""
        return self._data_term_theta(theta_from_params(self.spec, params))

    def _data_term_theta(self, theta: np.ndarray):
        val = C.c_double()
        grad = np.zeros_like(theta)
        rc = self._check(self._lib.bbh_fit_value_grad(self._h, _dp(theta), C.byref(val), _dp(grad)), "bbh_fit_value_grad")
        if rc == 1:
            return None, None
        return val.value, grad

    def fit(self, p0: GPParams | None = None, maxiter: int = 15000, max_attempts: int = 5) -> FitInfo:
        """scipy L-BFGS-B over the raw parameters with scipy's defaults, as
        ``botorch.fit.fit_gpytorch_mll`` does (call site gaussian_process/core.py:340-341);
        every objective evaluation is one ``bbh_fit_value_grad`` on the device.

        Like BoTorch's ``_fit_fallback`` the fit is retried (up to ``max_attempts`` times) from
        hyper-parameters re-sampled from their priors when an attempt ends abnormally or at a
        non-finite point; ``ModelFittingError`` is raised when every attempt fails."""
        with self._on_thread_stream():
            return self._fit(p0, maxiter, max_attempts)

    @contextlib.contextmanager
    def _on_thread_stream(self):
        """Fits side by side (the targets of a CompositeSurrogate, one host thread each): on the handles' default stream - the legacy
        null stream, ONE queue per device - their evaluations would run one after the other however many threads submit them (round 5:
        50.6 ms for three fits against 56.6 ms in sequence).  Inside ``private_fit_stream`` the handle enqueues on the thread's private
        stream for the duration of the block; ``set_model``, every evaluation and the final factorisation end with a synchronisation
        of that stream, so nothing is in flight on it when the handle goes back to its own."""
        st = getattr(_FIT_TLS, "stream", None)
        if st is None or getattr(self, "_thread_stream_depth", 0) > 0:
            yield
            return
        prev = getattr(self, "_stream_ptr", 0)
        self._check(self._lib.bbh_set_stream(self._h, C.c_void_p(int(st.cuda_stream))), "bbh_set_stream")
        self._thread_stream_depth = 1
        try:
            yield
        finally:
            self._thread_stream_depth = 0
            self._check(self._lib.bbh_set_stream(self._h, C.c_void_p(prev)), "bbh_set_stream")

    def _fit(self, p0, maxiter, max_attempts) -> FitInfo:
        spec = self.spec
        n = self.n

        fast = FastObjective(spec, n) if FastObjective.applies(spec) else None

        def fun(raw):
            if fast is not None:  # single-task, single-kernel models: the same maps as below in a few vectorised operations
                theta, nat = fast.theta(raw)
                val, g = self._data_term_theta(theta)
                if val is None:
                    return float("inf"), np.zeros_like(raw)
                return fast.objective(raw, nat, val, g)
            p = unpack_raw(spec, raw)
            val, g = self.data_term(p)
            if val is None:
                return float("inf"), np.zeros_like(raw)
            return objective_from_data_term(spec, raw, n, val, g, params=p)

        last_msg = ""
        no_rng = bool(getattr(_FIT_TLS, "no_global_generator", False))  # (inside fit_side_by_side: see _FitNeedsTheGlobalGenerator)
        if no_rng and p0 is None and spec.n_tasks > 1 and getattr(spec, "task_factor_constraint", "softplus") == "none":
            raise _FitNeedsTheGlobalGenerator("random start values of the task factor")
        for attempt in range(max_attempts):
            if attempt > 0 and no_rng:
                raise _FitNeedsTheGlobalGenerator(f"retry after: {last_msg}")
            start = p0 if (attempt == 0 and p0 is not None) else (
                initial_params(spec) if attempt == 0 else sample_params_from_priors(spec))
            res = lbfgsb_minimize(fun, pack_raw(spec, start), raw_bounds(spec), maxiter)
            last_msg = str(res.message)
            ok = np.all(np.isfinite(res.x)) and np.isfinite(res.fun) and "ABNORMAL" not in last_msg.upper()
            if not ok:
                continue
            params = unpack_raw(spec, res.x)
            try:
                self.factorize(params)
            except ModelFittingError as ex:
                last_msg = str(ex)
                continue
            return FitInfo(params, float(res.fun), int(res.nit), int(res.nfev), int(res.status), last_msg)
        raise ModelFittingError(f"All attempts to fit the model have failed (last: {last_msg}).")

    def factorize(self, params: GPParams):
        theta = theta_from_params(self.spec, params)
        jit = C.c_double()
        try:
            self._check(self._lib.bbh_factorize(self._h, _dp(theta), C.byref(jit)), "bbh_factorize")
        except HipError as ex:
            raise ModelFittingError(str(ex)) from ex
        self.params = params
        self.jitter = jit.value
        self._p, self._pend_stats = 0, None  # (bbh_factorize drops the pending points of the previous factorisation)

    # ---- posterior ------------------------------------------------------------------------
    def _as_dev(self, X):
        torch = self._torch()
        if isinstance(X, np.ndarray):
            X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64))
        if X.dtype != torch.float64:
            X = X.to(torch.float64)
        X = X.to(self._dev())
        if X.dim() != 2 or X.shape[1] < self.spec.d:
            raise ValueError("candidates must be [N, d]")
        if X.stride(1) != 1:
            X = X.contiguous()
        if X.shape[0] == 1 and X.stride(0) < X.shape[1]:
            # a single row that came from a column-major block (``frame.iloc[[i]].to_numpy()``) counts as contiguous with a row
            # stride of 1: give it the row stride the C-ABI asks for (ldx >= d)
            X = X.as_strided(X.shape, (X.shape[1], 1))
        return X

    def posterior(self, X, unfused: bool = False, out=None):
        """Marginal posterior (mean, var) of N candidates as device tensors [N] (fp64); ``out`` = (mean, var) tensors to write into."""
        torch = self._torch()
        X = self._as_dev(X)
        N = X.shape[0]
        if out is not None:
            mean, var = out
        else:
            mean = torch.empty(N, dtype=torch.float64, device=X.device)
            var = torch.empty(N, dtype=torch.float64, device=X.device)
        fn = self._lib.bbh_posterior_unfused if unfused else self._lib.bbh_posterior
        self._check(fn(self._h, X.data_ptr(), N, X.stride(0), mean.data_ptr(), var.data_ptr()), "bbh_posterior")
        return mean, var

    def posterior_joint(self, Xq: np.ndarray):
        """Joint posterior (mean [q], cov [q,q]) of a small point set (host arrays)."""
        Xq = np.ascontiguousarray(np.atleast_2d(Xq), dtype=np.float64)
        q = Xq.shape[0]
        mean, cov = np.empty(q), np.empty((q, q))
        self._check(self._lib.bbh_posterior_joint(self._h, _dp(Xq), q, _dp(mean), _dp(cov)), "bbh_posterior_joint")
        return mean, cov

    def set_mean_columns(self, Y: np.ndarray):
        """Alternative target columns Y [n, S] (original scale) for ``posterior_columns``."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim != 2 or Y.shape[0] != self.n:
            raise ValueError("Y must be [n, S]")
        self._ncols = Y.shape[1]
        self._check(self._lib.bbh_set_mean_columns(self._h, _dp(Y), Y.shape[1]), "bbh_set_mean_columns")

    def posterior_columns(self, X, sample_major: bool = False):
        """Posterior means of the candidates under each target column: [N, S], or [S, N] with ``sample_major`` (the layout
        the qLogNEHVI scoring kernel reads coalesced)."""
        torch = self._torch()
        X = self._as_dev(X)
        N = X.shape[0]
        tmat = torch.empty((self._ncols, N) if sample_major else (N, self._ncols), dtype=torch.float64, device=X.device)
        fn = self._lib.bbh_posterior_columns_sm if sample_major else self._lib.bbh_posterior_columns
        self._check(fn(self._h, X.data_ptr(), N, X.stride(0), tmat.data_ptr()), "bbh_posterior_columns")
        return tmat

    def train_posterior_mean(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.float64)
        self._check(self._lib.bbh_train_posterior_mean(self._h, _dp(out)), "bbh_train_posterior_mean")
        return out

    def best_f(self, sign: float = 1.0, objective=None) -> float:
        """max_i objective(posterior mean at x_i)  (baybe/acquisition/_builder.py:141-161,256-265); ``objective``: an
        ``ObjectiveProgram`` in place of ``sign``."""
        if objective is not None:
            return float(objective.apply(self.train_posterior_mean()).max())
        return float((sign * self.train_posterior_mean()).max())

    # ---- qLogEI ---------------------------------------------------------------------------
    def qlogei(self, mean, var, z: np.ndarray, best_f: float, sign: float = 1.0, alive=None):
        torch = self._torch()
        z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1)
        N = mean.shape[0]
        scores = torch.empty(N, dtype=torch.float64, device=mean.device)
        self._check(
            self._lib.bbh_qlogei_q1(
                self._h, mean.data_ptr(), var.data_ptr(), N, _dp(z), z.shape[0], float(best_f), float(sign),
                alive.data_ptr() if alive is not None else None, scores.data_ptr(),
            ),
            "bbh_qlogei_q1",
        )
        return scores

    def qlogei_topk(self, mean, var, z: np.ndarray, best_f: float, sign: float = 1.0, k: int = 1, alive=None, scores=None):
        """q' = 1 qLogEI scores AND their k best in one call (``bbh_qlogei_q1_topk``: scores kernel, one selection kernel, results
        in host-mapped memory, one synchronisation): (scores [N] device tensor, values [k], indices [k]); entries beyond the
        number of scored candidates are (-inf, -1).  ``scores``: an fp64 device tensor [N] to write into (a step loop's buffer)."""
        torch = self._torch()
        z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1)
        N = mean.shape[0]
        if scores is None:
            scores = torch.empty(N, dtype=torch.float64, device=mean.device)
        k = int(min(k, N))
        vals, idx = np.empty(k), np.empty(k, dtype=np.int64)
        self._check(
            self._lib.bbh_qlogei_q1_topk(
                self._h, mean.data_ptr(), var.data_ptr(), N, _dp(z), z.shape[0], float(best_f), float(sign),
                alive.data_ptr() if alive is not None else None, scores.data_ptr(), k, _dp(vals), idx.ctypes.data_as(_lib.c_int64_p),
            ),
            "bbh_qlogei_q1_topk",
        )
        return scores, vals, idx

    def mc_acq(self, kind: str, mean, var, z: np.ndarray, best_f: float = 0.0, sign: float = 1.0, beta: float = 0.2,
               alive=None, cross=None, objective=None, stats=None):
        """MC acquisition values (qLogEI, qEI, qPI, qSR, qUCB, qPSTD) of N t-batches [x_i ; pending].  ``objective`` (a
        ``baybe_amd.objective.ObjectiveProgram``) replaces ``sign``: every posterior sample passes through the program before the
        utility (``bbh_mc_acq_obj_q1`` / ``bbh_mc_acq_obj_pending``); with ``cross`` the pending statistics are ``stats`` =
        (mean [p], cov [p, p]), by default what the last ``set_pending`` returned."""
        torch = self._torch()
        z = np.ascontiguousarray(z, dtype=np.float64)
        N = mean.shape[0]
        scores = torch.empty(N, dtype=torch.float64, device=mean.device)
        k = _lib.ACQ_KINDS[kind]
        al = alive.data_ptr() if alive is not None else None
        if objective is not None:
            prog = objective.to_struct()
            if cross is None:
                z = z.reshape(-1)
                rc = self._lib.bbh_mc_acq_obj_q1(self._h, k, C.byref(prog), mean.data_ptr(), var.data_ptr(), N, _dp(z), z.shape[0],
                                                 float(best_f), float(beta), al, scores.data_ptr())
            else:
                stats = stats if stats is not None else getattr(self, "_pend_stats", None)
                if stats is None:
                    raise ValueError("no pending points set: call set_pending() or pass stats=(mean, cov)")
                mp, cpp = stats
                mp, cpp = np.ascontiguousarray(mp, dtype=np.float64), np.ascontiguousarray(cpp, dtype=np.float64)
                p = mp.shape[0]
                if not 1 <= p <= MAX_PENDING or cross.shape[1] != p or z.ndim != 2 or z.shape[1] != p + 1:
                    raise ValueError(f"an objective program is scored jointly with 1 ... {MAX_PENDING} pending points")
                rc = self._lib.bbh_mc_acq_obj_pending(self._h, k, C.byref(prog), mean.data_ptr(), var.data_ptr(), cross.data_ptr(), N,
                                                      p, _dp(mp), _dp(cpp), _dp(z), z.shape[0], float(best_f), float(beta), al,
                                                      scores.data_ptr())
            self._check(rc, "bbh_mc_acq_obj")
            return scores
        if cross is None:
            z = z.reshape(-1)
            rc = self._lib.bbh_mc_acq_q1(self._h, k, mean.data_ptr(), var.data_ptr(), N, _dp(z), z.shape[0], float(best_f),
                                         float(sign), float(beta), al, scores.data_ptr())
        else:
            rc = self._lib.bbh_mc_acq_pending(self._h, k, mean.data_ptr(), var.data_ptr(), cross.data_ptr(), N, _dp(z),
                                              z.shape[0], float(best_f), float(sign), float(beta), al, scores.data_ptr())
        self._check(rc, "bbh_mc_acq")
        return scores

    def desirability_acq(self, program, kind: str, mean, var, z: np.ndarray, best_f: float = 0.0, beta: float = 0.2, alive=None,
                         cross=None, stats=None, form: int = -1):
        """MC acquisition values (qLogEI ... qPSTD) of N t-batches under a desirability objective with one model per target
        (``baybe_amd.desirability.DesirabilityProgram``): ``mean`` / ``var`` [T, N] device tensors, ``z`` [S, T]; with pending points
        ``cross`` [T, N, p], ``stats`` = (mean_p [T, p], cov_pp [T, p, p]) and ``z`` [S, 1 + p, T].  ``form``: storage of the joint
        factors (0 LDS, 1 workspace, -1 LDS where it fits)."""
        torch = self._torch()
        T, N = mean.shape
        if T != program.n_targets or var.shape != mean.shape or not mean.is_contiguous() or not var.is_contiguous():
            raise ValueError("mean and var must be contiguous [T, N] tensors, one row per target")
        z = np.ascontiguousarray(z, dtype=np.float64)
        scores = torch.empty(N, dtype=torch.float64, device=mean.device)
        k = _lib.ACQ_KINDS[kind]
        al = alive.data_ptr() if alive is not None else None
        des = program.to_struct()
        if cross is None:
            if z.ndim != 2 or z.shape[1] != T:
                raise ValueError("z must be [S, T]")
            rc = self._lib.bbh_desirability_q1(self._h, k, C.byref(des), mean.data_ptr(), var.data_ptr(), N, _dp(z), z.shape[0],
                                               float(best_f), float(beta), al, scores.data_ptr())
        else:
            if stats is None:
                raise ValueError("pass stats=(mean_p [T, p], cov_pp [T, p, p]) with cross")
            mp, cpp = (np.ascontiguousarray(a, dtype=np.float64) for a in stats)
            p = mp.shape[1]
            if (not 1 <= p <= MAX_PENDING or tuple(cross.shape) != (T, N, p) or not cross.is_contiguous() or mp.shape != (T, p)
                    or cpp.shape != (T, p, p) or z.shape[1:] != (p + 1, T)):
                raise ValueError(f"a desirability objective is scored jointly with 1 ... {MAX_PENDING} pending points: cross [T, N, p], "
                                 f"stats ([T, p], [T, p, p]), z [S, p + 1, T]")
            rc = self._lib.bbh_desirability_pending(self._h, k, C.byref(des), mean.data_ptr(), var.data_ptr(), cross.data_ptr(), N, p,
                                                    _dp(mp), _dp(cpp), _dp(z), z.shape[0], float(best_f), float(beta), int(form), al,
                                                    scores.data_ptr())
        self._check(rc, "bbh_desirability")
        return scores

    def desirability_last_form(self) -> int:
        """Storage of the factors in the last joint ``desirability_acq`` launch: 0 LDS, 1 workspace, -1 none yet."""
        return int(self._lib.bbh_desirability_last_form(self._h))

    def ehvi_acq(self, log: bool, mean, var, cells, z: np.ndarray, alive=None, cross=None, stats=None, form: int = -1):
        """qEHVI (``log=False``) / qLogEHVI values of N t-batches against one fixed cell list (``acqfs.py:429-464``): ``mean`` / ``var``
        [m, N] device tensors, ``cells`` = (lower [C, m], upper [C, m]; upper bounds may be +inf), ``z`` [S, m]; with pending points
        ``cross`` [m, N, p], ``stats`` = (mean_p [m, p], cov_pp [m, p, p]) and ``z`` [S, 1 + p, m].  Everything ORIENTED: the caller
        has negated the means and the base-sample columns of minimised targets.  ``form``: storage of the joint factors (0 LDS,
        1 workspace, -1 the library's choice: the workspace, which measured faster)."""
        torch = self._torch()
        m, N = mean.shape
        if var.shape != mean.shape or not mean.is_contiguous() or not var.is_contiguous():
            raise ValueError("mean and var must be contiguous [m, N] tensors, one row per target")
        lo, up = (np.ascontiguousarray(a, dtype=np.float64) for a in cells)
        if lo.ndim != 2 or lo.shape[1] != m or up.shape != lo.shape:
            raise ValueError("cells must be (lower [C, m], upper [C, m])")
        z = np.ascontiguousarray(z, dtype=np.float64)
        scores = torch.empty(N, dtype=torch.float64, device=mean.device)
        al = alive.data_ptr() if alive is not None else None
        if cross is None:
            if z.ndim != 2 or z.shape[1] != m:
                raise ValueError("z must be [S, m]")
            rc = self._lib.bbh_ehvi_q1(self._h, int(bool(log)), m, mean.data_ptr(), var.data_ptr(), N, _dp(lo), _dp(up), lo.shape[0], _dp(z),
                                       z.shape[0], al, scores.data_ptr())
        else:
            if stats is None:
                raise ValueError("pass stats=(mean_p [m, p], cov_pp [m, p, p]) with cross")
            mp, cpp = (np.ascontiguousarray(a, dtype=np.float64) for a in stats)
            p = mp.shape[1]
            if (cross.dim() != 3 or tuple(cross.shape) != (m, N, p) or not cross.is_contiguous() or mp.shape != (m, p)
                    or cpp.shape != (m, p, p) or z.ndim != 3 or z.shape[1:] != (p + 1, m)):
                raise ValueError("a hypervolume improvement is scored jointly with cross [m, N, p], stats ([m, p], [m, p, p]), "
                                 "z [S, p + 1, m]")
            rc = self._lib.bbh_ehvi_pending(self._h, int(bool(log)), m, mean.data_ptr(), var.data_ptr(), cross.data_ptr(), N, p, _dp(mp),
                                            _dp(cpp), _dp(lo), _dp(up), lo.shape[0], _dp(z), z.shape[0], int(form), al, scores.data_ptr())
        self._check(rc, "bbh_ehvi")
        return scores

    def ehvi_last_form(self) -> int:
        """Storage of the factors in the last joint ``ehvi_acq`` launch: 0 LDS, 1 workspace, -1 none yet."""
        return int(self._lib.bbh_ehvi_last_form(self._h))

    def nipv_set_points(self, P: np.ndarray) -> np.ndarray:
        """Integration points of qNIPV, ``P`` [M, d] rows of the candidates' representation: builds A = (K + s2 I)^-1 K(X, P) from the
        current factorisation and keeps it resident until the next ``factorize``.  Returns var(p_j) [M] (original target scale)."""
        P = np.ascontiguousarray(np.atleast_2d(P), dtype=np.float64)
        if P.shape[1] < self.spec.d:
            raise ValueError("integration points must be [M, d]")
        P = np.ascontiguousarray(P[:, : self.spec.d])
        var_p = np.empty(P.shape[0])
        self._check(self._lib.bbh_nipv_set_points(self._h, _dp(P), P.shape[0], _dp(var_p)), "bbh_nipv_set_points")
        self._nipv_M = P.shape[0]
        return var_p

    def nipv_gain(self, X, var, cross=None, H=None, ginv=None, alive=None):
        """gain [N] of qNIPV (``include/baybe_hip.h``): the integrated variance that adding x to the handle's b pending points removes,
        summed over the integration points.  ``var`` [N] from ``posterior``; with pending points ``cross`` [N, b] from ``cross_cov``,
        ``H`` [b, M] = G^-1 cov(B, P) and ``ginv`` [b, b] = G^-1, G = cov(B, B) + s2 I.  -inf where ``alive`` is 0."""
        torch = self._torch()
        X = self._as_dev(X)
        N = X.shape[0]
        b = getattr(self, "_p", 0)
        if var.shape != (N,) or not var.is_contiguous():
            raise ValueError("var must be a contiguous [N] tensor")
        hp = gp = cp = None
        if b:
            if cross is None or H is None or ginv is None:
                raise ValueError("with pending points pass cross [N, b], H [b, M] and ginv [b, b]")
            H, ginv = np.ascontiguousarray(H, dtype=np.float64), np.ascontiguousarray(ginv, dtype=np.float64)
            if tuple(cross.shape) != (N, b) or not cross.is_contiguous() or H.shape != (b, getattr(self, "_nipv_M", -1)) or ginv.shape != (b, b):
                raise ValueError("with pending points pass cross [N, b], H [b, M] and ginv [b, b]")
            hp, gp, cp = _dp(H), _dp(ginv), cross.data_ptr()
        gain = torch.empty(N, dtype=torch.float64, device=X.device)
        self._check(self._lib.bbh_nipv_gain(self._h, X.data_ptr(), N, X.stride(0), var.data_ptr(), cp, hp, gp,
                                            alive.data_ptr() if alive is not None else None, gain.data_ptr()), "bbh_nipv_gain")
        return gain

    def nipv_last_form(self) -> int:
        """Row tiles per workgroup of the last ``nipv_gain`` launch: 0 one (16 candidates), 1 two (32), -1 none yet."""
        return int(self._lib.bbh_last_nipv_form(self._h))

    # ---- exact Shapley values of the posterior mean (baybe_amd/insights.py) ----------------
    SHAP_CHUNK_BYTES = 64 << 20  # composed rows one posterior pass of the generic form takes (at least one coalition's B rows)

    def shap_values(self, X, background, groups, form: str = "auto", want_v: bool = False, n_groups: int | None = None):
        """Exact interventional Shapley values of the posterior mean (``include/baybe_hip.h``): ``X`` [R, d] explained rows,
        ``background`` [B, d], ``groups`` [d] the feature (0 .. M - 1) each comp-rep column belongs to, -1 for a column in no feature
        (it keeps the background's value); ``n_groups`` = M where the last features own no column.  ``form``: ``"fused"``
        (``bbh_shap_values``: one stationary kernel, one task, n <= 512; refused with the kernel's text elsewhere), ``"composed"``
        (``bbh_shap_compose`` -> this engine's ``posterior`` -> ``bbh_shap_reduce`` -> ``bbh_shap_apply``: every model), ``"auto"``
        (fused where it applies).  Returns ``(phi [R, M] device tensor, base_value, v [R, 2^M] device tensor or None)``; bit g of a
        coalition's index stands for feature g.  ``shap_last_form`` names the form that answered."""
        if form not in ("auto", "fused", "composed"):
            raise ValueError(f"form must be 'auto', 'fused' or 'composed', not {form!r}")
        torch = self._torch()
        d = int(self.spec.d) if self.spec is not None else int(self.d)
        X, Bg = self._as_dev(X), self._as_dev(background)
        R, B = int(X.shape[0]), int(Bg.shape[0])
        grp = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
        if grp.shape[0] != d:
            raise ValueError(f"groups must name the feature of each of the {d} comp-rep columns")
        M = int(n_groups) if n_groups is not None else int(grp.max(initial=-1)) + 1
        if R < 1 or B < 1:
            raise ValueError("need at least one explained row and one background row")
        gp = grp.ctypes.data_as(C.POINTER(C.c_int32))
        fits = 1 <= M <= 16  # (beyond that the library refuses, before any device work: nothing of size 2^M is allocated here)
        phi = torch.empty((R, max(M, 1)), dtype=torch.float64, device=X.device)
        v = torch.empty((R, 1 << M), dtype=torch.float64, device=X.device) if fits else None
        if form == "fused" and self.spec is None:  # (a forest / linear engine: its handle holds no GP model of its own)
            raise HipError("bbh_shap_values failed (-1): the fused form needs a Gaussian process model; this engine answers through "
                           "form='composed'")
        if form != "composed" and self.spec is not None:
            base = C.c_double(0.0)
            rc = self._lib.bbh_shap_values(self._h, X.data_ptr(), R, X.stride(0), Bg.data_ptr(), B, Bg.stride(0), gp, M,
                                           v.data_ptr() if (fits and want_v) else None, phi.data_ptr(), C.byref(base))
            if rc == 0:
                self._shap_form = "fused"
                return phi, float(base.value), (v if want_v else None)
            msg = self._lib.bbh_last_error(self._h)
            if form == "fused" or b"the fused form" not in (msg or b""):
                self._check(rc, "bbh_shap_values")
        if not fits:  # the generic form's own refusal text
            self._check(self._lib.bbh_shap_compose(self._h, X.data_ptr(), R, X.stride(0), Bg.data_ptr(), B, Bg.stride(0), gp, d, M, 0, 0,
                                                   None), "bbh_shap_compose")
        pairs = R << M
        per = max(1, int(self.SHAP_CHUNK_BYTES // (8 * B * d)))
        vf = v.reshape(-1)
        for p0 in range(0, pairs, per):
            pc = min(per, pairs - p0)
            rows = torch.empty((pc * B, d), dtype=torch.float64, device=X.device)
            self._check(self._lib.bbh_shap_compose(self._h, X.data_ptr(), R, X.stride(0), Bg.data_ptr(), B, Bg.stride(0), gp, d, M, p0 * B,
                                                   pc * B, rows.data_ptr()), "bbh_shap_compose")
            mean = self.posterior(rows)[0].contiguous()
            self._check(self._lib.bbh_shap_reduce(self._h, mean.data_ptr(), pc, B, vf[p0:p0 + pc].data_ptr()), "bbh_shap_reduce")
        self._check(self._lib.bbh_shap_apply(self._h, v.data_ptr(), R, M, phi.data_ptr()), "bbh_shap_apply")
        self._shap_form = "composed"
        return phi, float(v[0, 0].item()), (v if want_v else None)

    def polytope_sample(self, reduced: dict, R: int, T: int, seed: int):
        """``R`` uniform samples [R, dc] (device tensor) of a polytope given by its reduced set (``Polytope.reduced()``): one
        hit-and-run chain of ``T`` steps per sample, counter-based uniforms from ``seed`` (``bbh_polytope_sample``)."""
        torch = self._torch()
        a = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in reduced.items()}
        dc, dz = a["Z"].shape
        mi = a["bg"].shape[0]
        out = torch.empty((int(R), dc), dtype=torch.float64, device=self._dev())

        def p(name):
            return a[name].ctypes.data_as(_lib.c_double_p)

        self._check(self._lib.bbh_polytope_sample(self._h, dc, dz, mi, p("Z"), p("GZ"), p("c0"), p("lo"), p("hi"), p("bl"), p("bu"), p("bg"),
                                                  int(R), int(T), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), out.data_ptr()),
                    "bbh_polytope_sample")
        return out

    def polytope_project(self, P, lo, hi, rows, rhs, me: int, tolf: float, mu_min: float):
        """Euclidean projection of every row of ``P`` [k, dc] onto {lo <= c <= hi, rows[:me] c = rhs[:me], rows[me:] c >= rhs[me:]}:
        ``(out [k, dc], status [k] int32)`` device tensors; status 1 = iteration budget exhausted (``bbh_polytope_project``)."""
        torch = self._torch()
        if isinstance(P, np.ndarray):
            P = torch.from_numpy(np.ascontiguousarray(P, dtype=np.float64))
        P = P.to(self._dev(), dtype=torch.float64)
        if P.dim() != 2 or P.stride(1) != 1:
            P = P.reshape(-1, len(lo)).contiguous()
        lo, hi, rows, rhs = (np.ascontiguousarray(v, dtype=np.float64) for v in (lo, hi, rows, rhs))
        dc = lo.shape[0]
        m = rhs.shape[0]
        k = int(P.shape[0])
        out = torch.empty((k, dc), dtype=torch.float64, device=P.device)
        status = torch.empty(k, dtype=torch.int32, device=P.device)

        def p(arr):
            return arr.ctypes.data_as(_lib.c_double_p)

        self._check(self._lib.bbh_polytope_project(self._h, dc, int(me), m - int(me), p(rows), p(rhs), p(lo), p(hi), float(tolf), float(mu_min),
                                                   P.data_ptr(), k, P.stride(0) if k > 1 else max(P.stride(0), dc), out.data_ptr(),
                                                   status.data_ptr()), "bbh_polytope_project")
        return out, status

    def shap_last_form(self):
        """``"fused"`` or ``"composed"``: the form that answered the last ``shap_values``; None before the first."""
        return getattr(self, "_shap_form", None)

    def analytic_acq(self, kind: str, mean, var, best_f: float = 0.0, sign: float = 1.0, beta: float = 0.2,
                     maximize: bool = True, alive=None):
        """Analytic acquisition values (PM, PSTD, UCB, EI, LogEI, PI) of N single candidates."""
        torch = self._torch()
        N = mean.shape[0]
        scores = torch.empty(N, dtype=torch.float64, device=mean.device)
        self._check(
            self._lib.bbh_analytic_acq(self._h, _lib.ACQ_KINDS[kind], mean.data_ptr(), var.data_ptr(), N, float(best_f),
                                       float(sign), float(beta), 1 if maximize else 0,
                                       alive.data_ptr() if alive is not None else None, scores.data_ptr()),
            "bbh_analytic_acq",
        )
        return scores

    def score_qlogei(self, X, z: np.ndarray, best_f: float, sign: float = 1.0, alive=None, want_posterior: bool = True):
        """Fused scoring pass: posterior + q'=1 qLogEI in one kernel.  Returns (scores, mean, var);
        mean/var are None unless ``want_posterior``."""
        torch = self._torch()
        X = self._as_dev(X)
        z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1)
        N = X.shape[0]
        scores = torch.empty(N, dtype=torch.float64, device=X.device)
        mean = torch.empty(N, dtype=torch.float64, device=X.device) if want_posterior else None
        var = torch.empty(N, dtype=torch.float64, device=X.device) if want_posterior else None
        self._check(
            self._lib.bbh_score_qlogei(
                self._h, X.data_ptr(), N, X.stride(0), _dp(z), z.shape[0], float(best_f), float(sign),
                alive.data_ptr() if alive is not None else None,
                mean.data_ptr() if mean is not None else None, var.data_ptr() if var is not None else None,
                scores.data_ptr(),
            ),
            "bbh_score_qlogei",
        )
        return scores, mean, var

    def set_pending(self, X_pending: np.ndarray | None):
        """Pending points = base pending + greedy picks (candidate first, then pending)."""
        if X_pending is None or len(X_pending) == 0:
            self._check(self._lib.bbh_pending_set(self._h, None, 0, None, None), "bbh_pending_set")
            self._p, self._pend_stats = 0, None
            return None, None
        P = np.ascontiguousarray(X_pending, dtype=np.float64)
        p = P.shape[0]
        if p > MAX_PENDING:
            raise ValueError(f"at most {MAX_PENDING} pending points are supported by the HIP path")
        mp = np.empty(p)
        cpp = np.empty((p, p))
        self._check(self._lib.bbh_pending_set(self._h, _dp(P), p, _dp(mp), _dp(cpp)), "bbh_pending_set")
        self._p = p
        self._pend_stats = (mp, cpp)  # (what ``mc_acq(..., objective=...)`` hands to the joint kernel)
        return mp, cpp

    def cross_cov(self, X):
        torch = self._torch()
        X = self._as_dev(X)
        N = X.shape[0]
        # (no pending points - never set, cleared, or dropped by a new factorisation: the library's own error, not an AttributeError)
        cross = torch.empty((N, getattr(self, "_p", 0)), dtype=torch.float64, device=X.device)
        self._check(self._lib.bbh_cross_cov(self._h, X.data_ptr(), N, X.stride(0), cross.data_ptr()), "bbh_cross_cov")
        return cross

    def cross_cov_many(self, X, X_pending: np.ndarray):
        """[N, p] posterior cross-covariances with ANY number of pending points: one mean-only pass per chunk of <= 15 (a column
        does not depend on the other pending points).  Leaves the handle's pending state at the last chunk."""
        torch = self._torch()
        P = np.ascontiguousarray(np.atleast_2d(X_pending), dtype=np.float64)
        cols = []
        for c0 in range(0, len(P), MAX_PENDING):
            self.set_pending(P[c0 : c0 + MAX_PENDING])
            cols.append(self.cross_cov(X))
        return cols[0] if len(cols) == 1 else torch.cat(cols, dim=1).contiguous()

    def qlogei_pending_big(self, mean, var, cross, X_pending: np.ndarray, z: np.ndarray, best_f: float, sign: float = 1.0,
                           alive=None, stats=None):
        """qLogEI of N t-batches [x_i ; pending] with explicit pending statistics (``bbh_qlogei_pending_big``), 1 ... 63
        pending points: ``stats`` = (mean [p], cov [p, p]) of the pending points, by default from ``posterior_joint``; their
        cross-covariances from ``cross_cov`` / ``cross_cov_many``."""
        torch = self._torch()
        P = np.ascontiguousarray(np.atleast_2d(X_pending), dtype=np.float64)
        p = P.shape[0]
        if not 1 <= p <= MAX_PENDING_BIG or cross.shape[1] != p:
            raise ValueError(f"qlogei_pending_big handles 1 ... {MAX_PENDING_BIG} pending points")
        mp, cpp = stats if stats is not None else self.posterior_joint(P)
        z = np.ascontiguousarray(z, dtype=np.float64)
        N = mean.shape[0]
        scores = torch.empty(N, dtype=torch.float64, device=mean.device)
        cpp = np.ascontiguousarray(cpp, dtype=np.float64)
        self._check(
            self._lib.bbh_qlogei_pending_big(
                self._h, mean.data_ptr(), var.data_ptr(), cross.data_ptr(), N, p, _dp(np.ascontiguousarray(mp)), _dp(cpp), _dp(z),
                z.shape[0], float(best_f), float(sign), alive.data_ptr() if alive is not None else None, scores.data_ptr(),
            ),
            "bbh_qlogei_pending_big",
        )
        return scores

    def qlogei_pending(self, mean, var, cross, z: np.ndarray, best_f: float, sign: float = 1.0, alive=None):
        torch = self._torch()
        z = np.ascontiguousarray(z, dtype=np.float64)
        S = z.shape[0]
        N = mean.shape[0]
        scores = torch.empty(N, dtype=torch.float64, device=mean.device)
        self._check(
            self._lib.bbh_qlogei_pending(
                self._h, mean.data_ptr(), var.data_ptr(), cross.data_ptr(), N, _dp(z), S, float(best_f), float(sign),
                alive.data_ptr() if alive is not None else None, scores.data_ptr(),
            ),
            "bbh_qlogei_pending",
        )
        return scores

    # ---- derivatives for gradient-based continuous optimisation ---------------------------
    def posterior_grad(self, X, cols):
        """Posterior of N candidates and its derivatives with respect to the raw coordinates of the comp-rep columns ``cols``
        (ascending, numerical; ``bbh_posterior_grad``): a dict of device tensors ``mean`` [N], ``var`` [N], ``cross`` [N, p],
        ``dmean`` [N, dc], ``dvar`` [N, dc], ``dcross`` [N, p, dc], p = the pending points set on the handle."""
        torch = self._torch()
        X = self._as_dev(X)
        N = X.shape[0]
        cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        dc, p = int(cols.shape[0]), getattr(self, "_p", 0)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=X.device)  # noqa: E731
        out = {"mean": new(N), "var": new(N), "cross": new(N, p), "dmean": new(N, dc), "dvar": new(N, dc), "dcross": new(N, p, dc)}
        self._check(
            self._lib.bbh_posterior_grad(
                self._h, X.data_ptr(), N, X.stride(0), cols.ctypes.data_as(C.POINTER(C.c_int32)), dc, out["mean"].data_ptr(),
                out["var"].data_ptr(), out["cross"].data_ptr() if p else None, out["dmean"].data_ptr(), out["dvar"].data_ptr(),
                out["dcross"].data_ptr() if p else None,
            ),
            "bbh_posterior_grad",
        )
        return out

    def qlogei_partials(self, mean, var, cross, z: np.ndarray, best_f: float, sign: float = 1.0):
        """qLogEI of the t-batches [x_i ; pending] and its partial derivatives with respect to (mean_i, var_i, cross_i1 .. cross_ip)
        (``bbh_qlogei_partials``): (scores [N], partials [N, 2 + p], ok [N] uint8) as device tensors; ``ok`` = 0 marks a candidate
        whose variance is not positive or whose joint factor needed jitter (zero partials)."""
        torch = self._torch()
        p = getattr(self, "_p", 0)
        z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1, 1 + p)
        N = mean.shape[0]
        scores = torch.empty(N, dtype=torch.float64, device=mean.device)
        part = torch.empty((N, 2 + p), dtype=torch.float64, device=mean.device)
        ok = torch.empty(N, dtype=torch.uint8, device=mean.device)
        self._check(
            self._lib.bbh_qlogei_partials(
                self._h, mean.data_ptr(), var.data_ptr(), cross.data_ptr() if p else None, N, _dp(z), z.shape[0], float(best_f),
                float(sign), scores.data_ptr(), part.data_ptr(), ok.data_ptr(),
            ),
            "bbh_qlogei_partials",
        )
        return scores, part, ok

    def qlogei_value_grad(self, X, cols, z: np.ndarray, best_f: float, sign: float = 1.0):
        """qLogEI of [x_i ; pending] and its gradient with respect to the columns ``cols`` of x_i: the two native calls, then the
        chain rule grad_j = a_m dmean_j + a_v dvar_j + sum_r a_r dcross_rj as one contraction on the device.  Returns
        (scores [N], grad [N, dc], ok [N] uint8) as device tensors."""
        g = self.posterior_grad(X, cols)
        scores, part, ok = self.qlogei_partials(g["mean"], g["var"], g["cross"], z, best_f, sign)
        grad = part[:, 0:1] * g["dmean"] + part[:, 1:2] * g["dvar"]
        if g["cross"].shape[1]:
            grad = grad + (part[:, 2:, None] * g["dcross"]).sum(dim=1)
        return scores, grad, ok

    def sobol_normal_dev(self, S: int, q: int, seed: int):
        """[S, q] base samples of ``SobolQMCNormalSampler`` as a device tensor, produced on the device (``bbh_sobol_normal_dev``;
        asynchronous on the handle's stream): what ``sobol_normal_base_samples`` returns, up to the last bits of erfinv."""
        torch = self._torch()
        out = torch.empty((S, q), dtype=torch.float64, device=self._dev())
        state0 = _sobol_state0(q)
        self._check(self._lib.bbh_sobol_normal_dev(self._h, state0.ctypes.data_as(_lib.c_int64_p), int(seed) & 0xFFFFFFFFFFFFFFFF, S, q,
                                                   out.data_ptr()), "bbh_sobol_normal_dev")
        return out

    # ---- selection ------------------------------------------------------------------------
    def argmax(self, scores):
        v, i = C.c_double(), C.c_int64()
        self._check(self._lib.bbh_argmax(self._h, scores.data_ptr(), scores.shape[0], C.byref(v), C.byref(i)), "bbh_argmax")
        return v.value, i.value

    def topk(self, scores, k: int):
        vals = np.empty(k)
        idx = np.empty(k, dtype=np.int64)
        self._check(
            self._lib.bbh_topk(self._h, scores.data_ptr(), scores.shape[0], k, _dp(vals), idx.ctypes.data_as(_lib.c_int64_p)),
            "bbh_topk",
        )
        return vals, idx

    # ---- farthest point sampling (baybe_amd.sampling) ------------------------------------------------------------
    def fps_prepare(self, X, mean: np.ndarray, scale: np.ndarray, order=None):
        """``P [d, ldp]`` (device, fp64): the rows ``order`` of ``X [N, d]`` (device tensor; ``None``: all rows in place) as
        ``(X - mean) / scale``, transposed (``bbh_fps_prepare``; asynchronous).  ``ldp`` = the row count padded to 256."""
        torch = self._torch()
        N, d = X.shape
        M = N if order is None else int(order.shape[0])
        ldp = -(-M // 256) * 256
        P = torch.empty((d, ldp), dtype=torch.float64, device=X.device)
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        scale = np.ascontiguousarray(scale, dtype=np.float64)
        self._check(self._lib.bbh_fps_prepare(self._h, X.data_ptr(), N, d, X.stride(0), _dp(mean), _dp(scale),
                                              None if order is None else order.data_ptr(), M, P.data_ptr(), ldp), "bbh_fps_prepare")
        return P

    def fps_farthest_pair(self, P, M: int, alive=None):
        """(d^2, a, b): the live ranks a < b of ``P [d, ldp]`` (first ``M`` columns) with the largest squared distance; bit-equal
        maxima resolve to the smallest a, then the smallest b (``bbh_fps_farthest_pair``)."""
        v, a, b = C.c_double(), C.c_int64(), C.c_int64()
        self._check(self._lib.bbh_fps_farthest_pair(self._h, P.data_ptr(), M, P.shape[0], P.stride(0),
                                                    None if alive is None else alive.data_ptr(), C.byref(v), C.byref(a), C.byref(b)),
                    "bbh_fps_farthest_pair")
        return v.value, a.value, b.value

    def fps_greedy(self, P, M: int, alive=None, starts=None, n_picks: int = 0, k: int = -1, want_count: bool = False):
        """(ranks, d2, count) of ``bbh_fps_greedy``: ``starts`` (ranks) begins a selection on ``P``, ``None`` continues the handle's;
        ``k < 0`` takes the last of the tied rows at each of ``n_picks`` picks, ``k >= 0`` the k-th at one pick; ``count`` (with
        ``want_count``) is the number of tied rows the next pick would choose from."""
        ranks = np.empty(max(n_picks, 1), dtype=np.int64)
        d2 = np.empty(max(n_picks, 1))
        count = C.c_int64(-1)
        st = None if starts is None else np.ascontiguousarray(starts, dtype=np.int64)
        self._check(self._lib.bbh_fps_greedy(
            self._h, P.data_ptr(), M, P.shape[0], P.stride(0), None if alive is None else alive.data_ptr(),
            None if st is None else st.ctypes.data_as(_lib.c_int64_p), 0 if st is None else len(st), n_picks, k,
            ranks.ctypes.data_as(_lib.c_int64_p), _dp(d2), C.byref(count) if want_count else None), "bbh_fps_greedy")
        return ranks[:n_picks], d2[:n_picks], count.value

    # ---- k-medoids (baybe_amd.clustering): stateless, asynchronous, every buffer a device tensor ------------------
    def pam_dist_rows(self, P, M: int, rows):
        """``[T, M]`` distances from the positions ``rows`` (int64 device tensor) to every position of ``P [d, ldp]``
        (``bbh_pam_dist_rows``)."""
        torch = self._torch()
        out = torch.empty((int(rows.shape[0]), M), dtype=torch.float64, device=P.device)
        self._check(self._lib.bbh_pam_dist_rows(self._h, P.data_ptr(), M, P.shape[0], P.stride(0), rows.data_ptr(), int(rows.shape[0]),
                                                out.data_ptr()), "bbh_pam_dist_rows")
        return out

    def pam_assign(self, P, M: int, medoids):
        """(labels int32 [M], dist [M]): the nearest of the ``medoids`` (int64 device tensor), first in cluster order among bit-equal
        distances, and the distance to it (``bbh_pam_assign``)."""
        torch = self._torch()
        labels = torch.empty(M, dtype=torch.int32, device=P.device)
        dist = torch.empty(M, dtype=torch.float64, device=P.device)
        self._check(self._lib.bbh_pam_assign(self._h, P.data_ptr(), M, P.shape[0], P.stride(0), medoids.data_ptr(), int(medoids.shape[0]),
                                             labels.data_ptr(), dist.data_ptr()), "bbh_pam_assign")
        return labels, dist

    def pam_cost(self, Ps, M: int, starts, tile_starts, k: int):
        """``cost [M]`` by grouped column: the sequential sum of the distances from each column of ``Ps [d, M]`` (grouped by label) to
        the columns of its own cluster (``bbh_pam_cost``).  ``starts`` / ``tile_starts``: int64 device tensors [k + 1]."""
        torch = self._torch()
        max_tiles = M // 256 + k
        table = torch.empty(2 * max_tiles, dtype=torch.int32, device=Ps.device)
        cost = torch.empty(M, dtype=torch.float64, device=Ps.device)
        self._check(self._lib.bbh_pam_cost(self._h, Ps.data_ptr(), M, Ps.shape[0], Ps.stride(0), starts.data_ptr(), tile_starts.data_ptr(),
                                           k, table.data_ptr(), max_tiles, cost.data_ptr()), "bbh_pam_cost")
        return cost

    def pam_update(self, cost, perm, M: int, starts, medoids):
        """Moves ``medoids`` (int64 device tensor, in place) to the cheapest member of each cluster where that is strictly cheaper;
        returns the flags [k] (int32 device tensor: 1 = empty cluster, 2 = medoid changed) (``bbh_pam_update``)."""
        torch = self._torch()
        k = int(medoids.shape[0])
        flags = torch.empty(k, dtype=torch.int32, device=cost.device)
        self._check(self._lib.bbh_pam_update(self._h, cost.data_ptr(), perm.data_ptr(), M, starts.data_ptr(), k, medoids.data_ptr(),
                                             flags.data_ptr()), "bbh_pam_update")
        return flags

    # ---- k-means (baybe_amd.clustering): stateless, asynchronous, every buffer a device tensor, R restarts at once -
    def kmeans_plan(self, d: int, k: int, R: int):
        """(restarts per tile, chunks) of a pass over ``R`` restarts (``bbh_kmeans_plan``): that many restarts' centres share LDS,
        so a point is read once per such tile; ``chunks > 1``: one restart per tile, its centres streamed through LDS."""
        rt, chunks = C.c_int32(), C.c_int32()
        self._check(self._lib.bbh_kmeans_plan(self._h, d, k, R, C.byref(rt), C.byref(chunks)), "bbh_kmeans_plan")
        return rt.value, chunks.value

    def kmeans_seed(self, P, M: int, idx, U, trials: int, closest=None):
        """k-means++ for all restarts: fills the columns 1.. of ``idx [R, k]`` (int64 device tensor, column 0 = the first centres)
        from the uniforms ``U [R, (k - 1) * trials]`` (``bbh_kmeans_seed``).  ``closest [R, M]``: work array (allocated if None)."""
        torch = self._torch()
        R, k = int(idx.shape[0]), int(idx.shape[1])
        tiles = -(-M // 256)
        if closest is None:
            closest = torch.empty((R, M), dtype=torch.float64, device=P.device)
        tilesum = torch.empty((R, tiles), dtype=torch.float64, device=P.device)
        trialpart = torch.empty((R, trials, tiles), dtype=torch.float64, device=P.device)
        cand = torch.empty((R, trials), dtype=torch.int64, device=P.device)
        self._check(self._lib.bbh_kmeans_seed(self._h, P.data_ptr(), M, P.shape[0], P.stride(0), idx.data_ptr(),
                                              None if U is None else U.data_ptr(), R, k, trials, closest.data_ptr(), tilesum.data_ptr(),
                                              trialpart.data_ptr(), cand.data_ptr()), "bbh_kmeans_seed")
        return idx

    def kmeans_pass(self, P, M: int, centres, rid, labels, d2, out=None, want_sums: bool = True):
        """One Lloyd pass (``bbh_kmeans_pass``) for the restarts ``rid`` (int32 device tensor) of ``centres [R, k, d]``: ``labels
        [R, M]`` (int32) and ``d2 [R, M]`` are updated in place; returns the dict ``out`` of device tensors ``new`` [R, k, d], ``sums``
        [R, k, d], ``counts`` [R, k] (int32), ``shift`` [R], ``inertia`` [R], ``flags`` [R] (int32: bit 0 = no label changed, bit 1 =
        an empty cluster was met), allocated on the first call and passed back in on later ones.  Rows of restarts not in ``rid`` are
        left as they are."""
        torch = self._torch()
        R, k, d = (int(s) for s in centres.shape)
        if out is None:
            dev = P.device
            rt, _ = self.kmeans_plan(d, k, R)
            tiles = -(-M // 256)
            out = {"new": torch.zeros((R, k, d), dtype=torch.float64, device=dev), "sums": torch.zeros((R, k, d), dtype=torch.float64, device=dev),
                   "counts": torch.zeros((R, k), dtype=torch.int32, device=dev), "shift": torch.zeros(R, dtype=torch.float64, device=dev),
                   "inertia": torch.zeros(R, dtype=torch.float64, device=dev), "flags": torch.zeros(R, dtype=torch.int32, device=dev),
                   "work_f64": torch.empty(tiles * rt * (k * d + 1), dtype=torch.float64, device=dev),
                   "work_i32": torch.empty(tiles * rt * (k + 1), dtype=torch.int32, device=dev)}
        self._check(self._lib.bbh_kmeans_pass(
            self._h, P.data_ptr(), M, P.shape[0], P.stride(0), centres.data_ptr(), rid.data_ptr(), int(rid.shape[0]), k, int(want_sums),
            labels.data_ptr(), d2.data_ptr(), out["work_f64"].data_ptr(), out["work_f64"].numel(), out["work_i32"].data_ptr(),
            out["work_i32"].numel(), out["new"].data_ptr(), out["sums"].data_ptr(), out["counts"].data_ptr(), out["shift"].data_ptr(),
            out["inertia"].data_ptr(), out["flags"].data_ptr()), "bbh_kmeans_pass")
        return out

    def kmeans_select(self, labels, d2, k: int):
        """[k] int64 device tensor: per cluster the member with the smallest ``sqrt(d2)``, first on ties; 0 for a cluster without
        members (``bbh_kmeans_select``).  ``labels`` [M] int32, ``d2`` [M]."""
        torch = self._torch()
        out = torch.empty(k, dtype=torch.int64, device=labels.device)
        self._check(self._lib.bbh_kmeans_select(self._h, labels.data_ptr(), d2.data_ptr(), int(labels.shape[0]), k, out.data_ptr()),
                    "bbh_kmeans_select")
        return out

    # ---- Gaussian mixture (baybe_amd.clustering): stateless, asynchronous, every buffer a device tensor, R restarts at once -
    def gmm_plan(self, d: int, k: int, M: int):
        """(components per LDS chunk of the E-step, tiles per strip of the M-step) for ``M`` positions (``bbh_gmm_plan``)."""
        kc, tps = C.c_int32(), C.c_int32()
        self._check(self._lib.bbh_gmm_plan(self._h, d, k, M, C.byref(kc), C.byref(tps)), "bbh_gmm_plan")
        return kc.value, tps.value

    def gmm_params(self, R: int, k: int, d: int, device):
        """The parameter arrays of ``R`` restarts, zeroed: the dict the other ``gmm_*`` calls read and write."""
        torch = self._torch()
        f = dict(dtype=torch.float64, device=device)
        return {"nk": torch.zeros((R, k), **f), "w": torch.zeros((R, k), **f), "mu": torch.zeros((R, k, d), **f),
                "cov": torch.zeros((R, k, d, d), **f), "prec": torch.zeros((R, k, d, d), **f), "logdet": torch.zeros((R, k), **f),
                "lower": torch.zeros(R, **f), "flags": torch.zeros(R, dtype=torch.int32, device=device)}

    def gmm_mstep(self, P, M: int, params, rid, reg_covar: float, log_resp=None, labels=None, base: int = 0, normalize: bool = True,
                  work_limit: int = 1 << 25):
        """The M-step (``bbh_gmm_mstep``) for the restarts ``rid`` (int32 device tensor) from ``log_resp [G, k, M]`` or ``labels
        [G, M]`` (restart r reads row r - ``base``), then the precision factors (``bbh_gmm_precision``); ``params`` is updated in place.
        The restarts are taken in groups whose strip partials stay below ``work_limit`` doubles (256 MB)."""
        torch = self._torch()
        R, k, d = (int(s) for s in params["mu"].shape)
        _, tps = self.gmm_plan(d, k, M)
        tiles = -(-M // 256)
        strips = -(-tiles // tps)
        nb = -(-d // 16)
        per = strips * k * (d + 1 + 256 * (nb * (nb + 1) // 2))
        group = max(1, work_limit // per)
        n = int(rid.shape[0])
        work = torch.empty(per * min(group, n), dtype=torch.float64, device=P.device)
        for a in range(0, n, group):
            part = rid[a: a + group]
            self._check(self._lib.bbh_gmm_mstep(
                self._h, P.data_ptr(), M, P.shape[0], P.stride(0), None if log_resp is None else log_resp.data_ptr(),
                None if labels is None else labels.data_ptr(), base, part.data_ptr(), int(part.shape[0]), k, float(reg_covar),
                int(normalize), work.data_ptr(), work.numel(), params["nk"].data_ptr(), params["w"].data_ptr(), params["mu"].data_ptr(),
                params["cov"].data_ptr()), "bbh_gmm_mstep")
        self.gmm_precision(params, rid)

    def gmm_precision(self, params, rid):
        """``prec``, ``logdet`` and ``flags`` of ``params`` from its ``cov`` for the restarts ``rid`` (``bbh_gmm_precision``)."""
        R, k, d = (int(s) for s in params["mu"].shape)
        self._check(self._lib.bbh_gmm_precision(self._h, params["cov"].data_ptr(), rid.data_ptr(), int(rid.shape[0]), k, d,
                                                params["prec"].data_ptr(), params["logdet"].data_ptr(), params["flags"].data_ptr()),
                    "bbh_gmm_precision")

    def gmm_estep(self, P, M: int, params, rid, log_resp, labels, base: int = 0, lpn=None):
        """The E-step (``bbh_gmm_estep``) for the restarts ``rid``: ``log_resp [G, k, M]``, ``labels [G, M]`` (int32) and, if given,
        ``lpn [G, M]`` are written at row r - ``base``, ``params["lower"]`` at r."""
        torch = self._torch()
        R, k, d = (int(s) for s in params["mu"].shape)
        work = torch.empty(-(-M // 256) * int(rid.shape[0]), dtype=torch.float64, device=P.device)
        self._check(self._lib.bbh_gmm_estep(
            self._h, P.data_ptr(), M, P.shape[0], P.stride(0), params["w"].data_ptr(), params["mu"].data_ptr(), params["prec"].data_ptr(),
            params["logdet"].data_ptr(), rid.data_ptr(), int(rid.shape[0]), k, base, log_resp.data_ptr(), labels.data_ptr(),
            None if lpn is None else lpn.data_ptr(), work.data_ptr(), work.numel(), params["lower"].data_ptr()), "bbh_gmm_estep")

    # ---- random forest surrogate (baybe_amd.forest) -----------------------------------------------------------------
    def forest_lds_nodes(self) -> int:
        """Nodes of the largest tree the kernels walk out of LDS (``bbh_forest_lds_nodes``); larger trees are read from global memory."""
        return int(self._lib.bbh_forest_lds_nodes())

    def forest_upload(self, packed: dict, d: int) -> dict:
        """The node tables of a packed forest (``baybe_amd.forest.pack_forest``) on the device, in the layout the ``bbh_forest_*``
        calls read: ``meta [n, 4]`` int32 (feature, left, right, 0), ``tv [n]`` (threshold of an inner node, value of a leaf),
        ``off [T + 1]`` int64, and ``order`` = every tree once, ascending."""
        torch = self._torch()
        left = np.asarray(packed["children_left"], dtype=np.int32)
        n, T = len(left), len(packed["offsets"]) - 1
        meta = np.zeros((n, 4), dtype=np.int32)
        meta[:, 0], meta[:, 1], meta[:, 2] = packed["feature"], left, packed["children_right"]
        tv = np.where(left < 0, packed["value"], packed["threshold"]).astype(np.float64)
        dev = self._dev()
        return {"meta": torch.from_numpy(meta).to(dev), "tv": torch.from_numpy(tv).to(dev),
                "off": torch.from_numpy(np.asarray(packed["offsets"], dtype=np.int64).copy()).to(dev),
                "order": torch.arange(T, dtype=torch.int32, device=dev), "T": T, "n_nodes": n, "d": int(d),
                "max_nodes": int(np.diff(packed["offsets"]).max())}

    def _forest_args(self, F, X, order, lds_nodes):
        if X.dim() != 2 or X.shape[1] < F["d"] or X.stride(1) != 1 or X.dtype != self._torch().float64:
            raise ValueError(f"rows must be fp64 [N, >= {F['d']}] with unit column stride")
        order = F["order"] if order is None else order
        lds = self.forest_lds_nodes() if lds_nodes is None else int(lds_nodes)
        return (X.data_ptr(), int(X.shape[0]), F["d"], int(X.stride(0)), F["meta"].data_ptr(), F["tv"].data_ptr(), F["off"].data_ptr(),
                F["T"], F["n_nodes"], order.data_ptr(), int(order.shape[0]), lds)

    def forest_predict(self, F, X, lds_nodes=None):
        """Per-tree predictions ``P [T, N]`` of the device rows ``X`` (``bbh_forest_predict``): for small row sets."""
        torch = self._torch()
        P = torch.empty((F["T"], X.shape[0]), dtype=torch.float64, device=X.device)
        self._check(self._lib.bbh_forest_predict(self._h, *self._forest_args(F, X, None, lds_nodes), P.data_ptr()), "bbh_forest_predict")
        return P

    def forest_moments(self, F, X, lds_nodes=None):
        """(mean, unbiased variance) over the trees for the device rows ``X``, ``[N]`` each (``bbh_forest_moments``)."""
        torch = self._torch()
        mean = torch.empty(X.shape[0], dtype=torch.float64, device=X.device)
        var = torch.empty(X.shape[0], dtype=torch.float64, device=X.device)
        self._check(self._lib.bbh_forest_moments(self._h, *self._forest_args(F, X, None, lds_nodes), mean.data_ptr(), var.data_ptr()),
                    "bbh_forest_moments")
        return mean, var

    def forest_mc_acq(self, F, kind: str, X, counts, order, S: int, pend=None, best_f: float = 0.0, sign: float = 1.0,
                      beta: float = 0.2, alive=None, lds_nodes=None):
        """MC acquisition values ``[N]`` of the t-batches [x_i ; pending] under the ensemble posterior (``bbh_forest_mc_acq``):
        ``counts [T]`` int32 samples per tree (``S`` in total), ``order`` int32 = the trees with a count, ascending, ``pend [T, k]``
        the per-tree predictions of the pending points (None: no pending points)."""
        torch = self._torch()
        k = 0 if pend is None else int(pend.shape[1])
        if counts.shape[0] != F["T"] or counts.dtype != torch.int32 or order.dtype != torch.int32:
            raise ValueError("counts must be int32 [T] and order int32")
        if pend is not None and (pend.shape[0] != F["T"] or not pend.is_contiguous() or pend.dtype != torch.float64):
            raise ValueError("pend must be a contiguous fp64 [T, k] tensor")
        if alive is not None and (alive.shape[0] != X.shape[0] or alive.dtype != torch.uint8):
            raise ValueError("alive must be uint8 [N]")
        scores = torch.empty(X.shape[0], dtype=torch.float64, device=X.device)
        self._check(self._lib.bbh_forest_mc_acq(
            self._h, _lib.ACQ_KINDS[kind], *self._forest_args(F, X, order, lds_nodes), counts.data_ptr(), int(S),
            None if pend is None else pend.data_ptr(), k, float(best_f), float(sign), float(beta),
            None if alive is None else alive.data_ptr(), scores.data_ptr()), "bbh_forest_mc_acq")
        return scores

    # ---- Bayesian linear surrogate (baybe_amd.linear) ----------------------------------------------------------------
    def linear_upload(self, packed: dict) -> dict:
        """The tables of a packed linear model (``baybe_amd.linear.pack_linear``) on the device, in the layout ``bbh_linear_moments``
        reads: ``cols [k]`` int32, ``scale [3, k]`` (lo, range, coef) and ``T [k, k]``."""
        torch = self._torch()
        dev = self._dev()
        k = int(len(packed["cols"]))
        scale = np.ascontiguousarray(np.stack([packed["lo"], packed["range"], packed["coef"]]).astype(np.float64)).reshape(3, k)
        return {"cols": torch.from_numpy(np.ascontiguousarray(packed["cols"], dtype=np.int32)).to(dev),
                "scale": torch.from_numpy(scale).to(dev),
                "T": torch.from_numpy(np.ascontiguousarray(packed["T"], dtype=np.float64).reshape(k, k)).to(dev), "k": k,
                "intercept": float(packed["intercept"]), "inv_alpha": float(packed["inv_alpha"])}

    def linear_moments(self, L, X, ybar: float = 0.0, ysd: float = 1.0, form="auto"):
        """(mean, variance) ``[N]`` of the device rows ``X`` under the uploaded linear model ``L`` (``bbh_linear_moments``);
        ``form``: "auto" (by the number of kept columns), "register" or "block"."""
        torch = self._torch()
        if X.dim() != 2 or X.stride(1) != 1 or X.dtype != torch.float64:
            raise ValueError("rows must be fp64 [N, d] with unit column stride")
        N, k = int(X.shape[0]), L["k"]
        mean = torch.empty(N, dtype=torch.float64, device=X.device)
        var = torch.empty(N, dtype=torch.float64, device=X.device)
        ptr = (lambda t: t.data_ptr()) if k else (lambda t: None)
        self._check(self._lib.bbh_linear_moments(
            self._h, X.data_ptr() if N else None, N, int(X.shape[1]), int(X.stride(0)) if N > 1 else max(int(X.stride(0)), int(X.shape[1])),
            ptr(L["cols"]), ptr(L["scale"]), ptr(L["T"]), k, L["intercept"], L["inv_alpha"], float(ybar), float(ysd),
            form if isinstance(form, int) else {"auto": 0, "register": 1, "block": 2}[form], mean.data_ptr(), var.data_ptr()),
            "bbh_linear_moments")
        return mean, var

    def linear_last_form(self) -> str:
        """Form the last ``linear_moments`` of this handle ran as (``bbh_linear_last_form``)."""
        return {1: "register", 2: "block"}.get(self._lib.bbh_linear_last_form(self._h), "none")

    # ---- row-sharded selection through the library's own RCCL communicator ---------------------------------
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(256)
        n = self._lib.bbh_comm_unique_id(buf, 256)
        if n <= 0:
            raise HipError("bbh_comm_unique_id failed: RCCL (librccl.so.1) could not be loaded")
        return buf.raw[:n]

    def comm_init(self, rank: int, world: int, unique_id: bytes):
        self._check(self._lib.bbh_comm_init(self._h, int(rank), int(world), unique_id, len(unique_id)), "bbh_comm_init")
        self._comm = (int(rank), int(world))

    def allgather_topk(self, scores, row_offset: int, k: int):
        """Global top-k over all shards (one ncclAllGather of k (score, global index) pairs per rank)."""
        vals, idx = np.empty(k), np.empty(k, dtype=np.int64)
        self._check(
            self._lib.bbh_allgather_topk(self._h, scores.data_ptr() if scores.shape[0] else None, scores.shape[0],
                                         int(row_offset), int(k), _dp(vals), idx.ctypes.data_as(_lib.c_int64_p)),
            "bbh_allgather_topk",
        )
        return vals, idx

    def allgather_argmax(self, scores, row_offset: int, X):
        """One greedy step over all shards: (score, global row index, comp-rep row [d]) of the global winner."""
        val, gidx, row = C.c_double(), C.c_int64(), np.empty(self.spec.d)
        N = scores.shape[0]
        self._check(
            self._lib.bbh_allgather_argmax(self._h, scores.data_ptr() if N else None, N, int(row_offset),
                                           X.data_ptr() if N else None, X.stride(0) if N else self.spec.d, C.byref(val),
                                           C.byref(gidx), _dp(row)),
            "bbh_allgather_argmax",
        )
        return val.value, gidx.value, row

    def set_slice_rows(self, rows: int):
        """Row count the sample-slice heuristics of the joint q'-batch / qLogNEHVI kernels use instead of each call's own N
        (``bbh_set_slice_rows``; 0 = per call).  A row shard passes the GLOBAL count to add every candidate's partial sums in the
        order the unsharded pass uses: scores are then bit-identical across shard layouts, at the price of fewer slices (less
        parallelism) per rank."""
        self._check(self._lib.bbh_set_slice_rows(self._h, int(rows)), "bbh_set_slice_rows")

    # ---- instrumentation ------------------------------------------------------------------
    def posterior_kernel_form(self) -> str:
        """Which form of the fused posterior kernel the last variance pass ran as."""
        return {0: "windowed", 1: "cooperative", 2: "materialised", 3: "cooperative-2sweep", 4: "cooperative-generic",
                5: "register-resident", 6: "feature-space"}.get(self._lib.bbh_last_posterior_form(self._h), "none")

    def posterior_distance_seeded(self) -> bool:
        """Whether the last variance pass ran the cooperative form with the seeded distance GEMM (``BBH_COOP_SEED=0``: never)."""
        return self._lib.bbh_last_posterior_seeded(self._h) == 1

    def fit_evaluation_form(self) -> str:
        """Which path the last fit evaluation (``data_term``, every objective call of ``fit``) ran as - after a give-up of a dataflow
        launch, the path that produced the returned numbers (``enum bbh_fit_form`` in include/baybe_hip.h)."""
        return {0: "launch", 1: "small", 2: "tiles+mt", 3: "tiles+mt-partial", 4: "tiles", 5: "gram+tiles", 6: "one-launch",
                7: "split", 8: "rff", 9: "steps+tail"}.get(self._lib.bbh_last_fit_form(self._h), "none")

    def factorization_form(self) -> str:
        """How the last ``factorize`` (its last attempt) factorised the train covariance: ``"steps"`` - per-step launches - or
        ``"tiles"`` - the one-launch tile-dataflow factorisation; ``"none"`` before the first one."""
        return {0: "steps", 1: "tiles"}.get(self._lib.bbh_last_factor_form(self._h), "none")

    def timing(self, enable, families=None):
        """HIP-event timing of the kernel families on / off; ``families`` (names as for ``timing_read``) restricts the events to those
        families - an event between two back-to-back kernels costs the stream ~5 us."""
        code = 0
        if enable:
            code = 1 if not families else 2 * sum(1 << _lib.TIMED_FAMILIES[f] for f in families)
        self._check(self._lib.bbh_timing_enable(self._h, code), "bbh_timing_enable")

    def timing_read(self, reset: bool = True, family: str = "posterior"):
        """(total ms, launches) of one kernel family since the last reset: ``"posterior"`` (variance passes of the fused
        kernel), ``"cross"`` (its mean-only passes), ``"pending"`` (joint q'-batch acquisition kernels)."""
        ms, cnt = C.c_double(), C.c_int64()
        self._check(self._lib.bbh_timing_read_family(self._h, _lib.TIMED_FAMILIES[family], C.byref(ms), C.byref(cnt),
                                                     1 if reset else 0), "bbh_timing_read_family")
        return ms.value, cnt.value

    # ---- optimize_acqf_discrete with qLogEI -----------------------------------------------
    def greedy_qlogei(self, *args, **kwargs) -> "GreedyResult":
        """``_greedy_qlogei`` with the shard's slice geometry set for its duration only (an exception inside the loop used
        to leave ``slice_rows`` on a handle that goes back to the pool)."""
        import inspect

        # (``shard`` may arrive positionally: read it from the bound arguments of the real signature - ADVICE r5)
        shard = inspect.signature(self._greedy_qlogei).bind(*args, **kwargs).arguments.get("shard")
        repro = shard is not None and getattr(shard, "reproducible", False)
        if repro:
            self.set_slice_rows(shard.N_total)
        try:
            return self._greedy_qlogei(*args, **kwargs)
        finally:
            if repro:
                self.set_slice_rows(0)

    def _greedy_qlogei(
        self,
        X,
        q: int,
        S: int = 512,
        seed: int | None = None,
        sign: float = 1.0,
        X_pending: np.ndarray | None = None,
        best_f: float | None = None,
        z_by_q: dict | None = None,
        shard=None,
        kind: str = "qLogEI",
        beta: float = 0.2,
        alive=None,
        speculate: bool = True,
        objective=None,
    ) -> GreedyResult:
        """Sequential greedy of ``optimize_acqf_discrete(acqf, q, choices, unique=True)``.

        Step 0 runs the fused posterior over all candidates and caches (mean, var); every later
        step only needs the cross-covariances with the points picked so far (mean-only pass).
        ``alive`` (uint8 device tensor) restricts the candidates to a subset of the resident rows.
        ``shard`` (a ``baybe_amd.distributed.RowShard``) makes every selection a global one: the
        local winner is all-gathered (score, global index, row) and the global first-index argmax
        wins on every rank.
        ``objective`` (an ``ObjectiveProgram``, in place of ``sign``): every step is one ``mc_acq`` call with the program - no
        fused first step, no speculative statistics, at most 15 pending points.
        """
        torch = self._torch()
        X = self._as_dev(X)
        N = X.shape[0]
        d = self.spec.d
        if seed is None and z_by_q is None:
            seed = draw_sampler_seed()
        if best_f is None:
            best_f = self.best_f(sign) if objective is None else self.best_f(1.0, objective)
        okw = {} if objective is None else {"objective": objective}  # (an engine double without the feature is called as before)
        base = np.zeros((0, d)) if X_pending is None or len(X_pending) == 0 else np.atleast_2d(np.asarray(X_pending, dtype=np.float64))
        alive = torch.ones(N, dtype=torch.uint8, device=X.device) if alive is None else alive.clone()
        mean = var = None
        chosen_rows: list[np.ndarray] = []
        indices, values = [], []

        def get_z(qp: int) -> np.ndarray:
            return z_by_q[qp] if z_by_q is not None else sobol_normal_base_samples(S, qp, seed)

        if q > 0 and N > 0:  # the first pass is enqueued before the host scrambles the first step's base samples (0.6 ms)
            self.set_pending(None)  # (a variance pass without pending columns: the cooperative kernel forms)
            mean, var = self.posterior(X)
        z_next = get_z(1 + base.shape[0])
        # Cross-covariance columns ahead of time.  Every later step needs cov(candidate, pending point) for the points picked
        # so far - one mean-only pass of the fused kernel over all candidates per step, whose cost does not depend on the number
        # of columns (<= 15 ride on one MFMA column block).  The picks of the later steps come almost always from the head of
        # the first step's ranking, so after the first step ONE such pass computes the columns of its top candidates; a later
        # step whose pending points are all among them gathers its columns (bit-identical values: a column is an independent
        # dot product) instead of launching its own pass, any other step falls back to its own pass.
        spec_rows, spec_pos, cross_spec, big_cross, spec_stats = None, {}, None, None, None
        first_vals = first_top = None
        b0 = base.shape[0]
        for _step in range(q):
            pend = np.vstack([base] + chosen_rows) if chosen_rows else base
            p = pend.shape[0]
            z = z_next
            if p == 0:
                if mean is None:  # first step: posterior of every candidate, cached for the later steps
                    self.set_pending(None)
                    mean, var = self.posterior(X)
                if kind == "qLogEI" and shard is None and N > 0 and objective is None:
                    # scores, the winner and (for later steps) the head of the ranking in ONE call
                    m_spec = min(MAX_PENDING - b0, N, 4 * q) if (q > 1 and speculate and N > 1 and b0 < MAX_PENDING) else 1
                    scores, first_vals, first_top = self.qlogei_topk(mean, var, z[:, 0], best_f, sign, max(1, m_spec), alive)
                else:
                    scores = self.mc_acq(kind, mean, var, z[:, 0], best_f, sign, beta, alive, **okw)
            else:
                if mean is None:
                    mean, var = self.posterior(X)
                if p > MAX_PENDING and objective is not None:
                    raise ValueError(f"joint q-batches beyond {MAX_PENDING + 1} points are not available with a transformed target")
                if p > MAX_PENDING:
                    # more than 15 pending points (the reference has no cap): columns of earlier steps are kept, the new pick's
                    # column comes from a one-point pass; the joint kernel takes the pending statistics explicitly
                    if kind != "qLogEI":
                        raise ValueError(f"joint q-batches beyond {MAX_PENDING + 1} points are available for qLogEI only")
                    if p > MAX_PENDING_BIG:
                        raise ValueError(f"at most {MAX_PENDING_BIG} pending points (batch size + pending experiments <= "
                                         f"{MAX_PENDING_BIG + 1}) are supported by the HIP path")
                    if big_cross is None or big_cross.shape[1] != p - 1:
                        big_cross = self.cross_cov_many(X, pend)
                    else:
                        big_cross = torch.cat([big_cross, self.cross_cov_many(X, pend[-1:])], dim=1).contiguous()
                    scores = self.qlogei_pending_big(mean, var, big_cross, pend, z, best_f, sign, alive)
                else:
                    cols = None
                    if cross_spec is not None:
                        cols = [spec_pos.get(ix) for ix in indices]
                        cols = None if any(c is None for c in cols) else list(range(b0)) + cols
                    if cols is not None and kind == "qLogEI" and spec_stats is not None and objective is None:
                        # columns AND pending statistics are sub-blocks of what the speculative pass left: no bbh_pending_set
                        # round trip (0.15 - 0.3 ms of host work per step)
                        cross = cross_spec[:, cols].contiguous() if len(cols) != cross_spec.shape[1] else cross_spec
                        ix = np.asarray(cols)
                        scores = self.qlogei_pending_big(mean, var, cross, pend, z, best_f, sign, alive,
                                                         stats=(spec_stats[0][ix], spec_stats[1][np.ix_(ix, ix)]))
                    else:
                        self.set_pending(pend)
                        if cols is not None:
                            cross = cross_spec[:, cols].contiguous() if len(cols) != cross_spec.shape[1] else cross_spec
                        else:
                            cross = self.cross_cov(X)
                        scores = self.mc_acq(kind, mean, var, z, best_f, sign, beta, alive, cross=cross, **okw)
                    if p == MAX_PENDING:
                        big_cross = cross  # the next step continues from these columns
            step0_global = None
            if _step == 0 and q > 1 and speculate and b0 < MAX_PENDING and (N > 1 or shard is not None):
                if shard is None:
                    m_spec = min(MAX_PENDING - b0, N, 4 * q)
                    tv, top = (first_vals, first_top) if first_top is not None and len(first_top) == m_spec else self.topk(scores, m_spec)
                    keep = [j for j, (t, v) in enumerate(zip(top, tv)) if t >= 0 and v > -math.inf]  # live candidates only
                    top = [int(top[j]) for j in keep]
                    spec_rows = X[torch.as_tensor(top, device=X.device), :d].cpu().numpy() if top else None
                else:
                    # row shards: the head of the GLOBAL ranking with its rows - one all-gather of each rank's local head; its
                    # first entry is this step's winner, so the step needs no collective of its own
                    m_spec = min(MAX_PENDING - b0, shard.N_total, 4 * q)
                    lv, li = self.topk(scores, min(m_spec, N)) if N > 0 else (np.empty(0), np.empty(0, dtype=np.int64))
                    tv, top, rows = shard.global_topk_rows(lv, li, m_spec, X, d)
                    if len(top):
                        step0_global = (float(tv[0]), int(top[0]), rows[0].copy())
                    keep = [j for j, v in enumerate(tv) if v > -math.inf]
                    top = [int(top[j]) for j in keep]
                    spec_rows = rows[keep] if keep else None
                if top:
                    spec_stats = self.set_pending(np.vstack([base, spec_rows]))  # (mean, cov) of base + speculative points
                    cross_spec = self.cross_cov(X) if N > 0 else torch.empty((0, b0 + len(top)), dtype=torch.float64, device=X.device)
                    spec_pos = {ix: b0 + j for j, ix in enumerate(top)}
            if _step + 1 < q:  # host-side Sobol scrambling of the next step overlaps the device work of this one
                z_next = get_z(2 + p)
            if step0_global is not None:  # (sharded first step: the winner came with the speculative head)
                val, gidx, row = step0_global
                if shard.owns(gidx):
                    alive[shard.to_local(gidx)] = 0
                idx = gidx
            elif shard is not None and shard.rccl_bound(self):  # payload built on the device, one ncclAllGather
                val, gidx, row = self.allgather_argmax(scores, shard.start, X)
                if shard.owns(gidx):
                    alive[shard.to_local(gidx)] = 0
                idx = gidx
            elif shard is not None:
                val, idx = self.argmax(scores) if N > 0 else (-math.inf, -1)
                val, gidx, row = shard.global_argmax(val, idx, X)
                if shard.owns(gidx):
                    alive[shard.to_local(gidx)] = 0
                idx = gidx
            else:
                if _step == 0 and first_top is not None:
                    val, idx = float(first_vals[0]), int(first_top[0])
                else:
                    val, idx = self.argmax(scores) if N > 0 else (-math.inf, -1)
                if idx in spec_pos and spec_rows is not None:  # the winner is one of the speculative heads: its row is on the host already
                    row = spec_rows[spec_pos[idx] - b0]
                else:
                    row = X[idx, :d].cpu().numpy()
                alive[idx] = 0
            indices.append(int(idx))
            values.append(float(val))
            chosen_rows.append(np.asarray(row, dtype=np.float64).reshape(1, d))
        self.set_pending(None if (base.shape[0] == 0 or base.shape[0] > MAX_PENDING) else base)
        return GreedyResult(indices, values)
