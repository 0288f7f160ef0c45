"""ctypes binding of the planner kernels' C ABI (include/plan/rp_plan.h, librp_plan.so) and `PredictiveSampler`, a
batched predictive-sampling planner (MJPC's: fork the state into K candidates, roll each out H control steps under a
perturbed action spline, keep the best) over a second, K times larger environment.

The six entry points are module functions taking raw device addresses (`fork`, `sample`, `action`, `accumulate`,
`select`, `shift`); each enqueues one kernel on the caller's HIP stream and reads nothing back.  Like the engine, the
library has no CPU fallback: a missing library is an error.
"""

from __future__ import annotations

import ctypes

import numpy as np

from robopianist_amd import _abi

EXPORTED_SYMBOLS = ("rp_plan_fork", "rp_plan_sample", "rp_plan_action", "rp_plan_accumulate", "rp_plan_select",
                    "rp_plan_shift", "rp_plan_dim", "rp_plan_last_error")

MAX_FIELDS = 64
SPLINES = {"zero": 0, "linear": 1}


class PlanError(RuntimeError):
    pass


_p, _i, _u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32


class Field(ctypes.Structure):
    """rp_plan_field."""
    _fields_ = [("src", _p), ("dst", _p), ("row_bytes", ctypes.c_longlong)]


class ForkArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("fields", ctypes.POINTER(Field)), ("n_fields", _i), ("G", _i), ("K", _i),
                ("env_first", _i), ("env_count", _i), ("hip_stream", _p)]


class SampleArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("nominal", _p), ("sigma", _p), ("lo", _p), ("hi", _p), ("knots", _p),
                ("seed_lo", _u32), ("seed_hi", _u32), ("round", _u32), ("G", _i), ("K", _i), ("P", _i), ("nu", _i),
                ("env_first", _i), ("env_count", _i), ("hip_stream", _p)]


class ActionArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("knots", _p), ("out", _p), ("precision", _i), ("spline", _i),
                ("h", _i), ("H", _i), ("P", _i), ("nu", _i), ("n_rows", _i), ("row_first", _i), ("row_count", _i),
                ("hip_stream", _p)]


class AccumulateArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("ret", _p), ("alive", _p), ("reward", _p), ("step_type", _p),
                ("precision", _i), ("weight", ctypes.c_double), ("E", _i), ("env_first", _i), ("env_count", _i),
                ("hip_stream", _p)]


class SelectArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("ret", _p), ("knots", _p), ("nominal", _p), ("best_k", _p),
                ("best_return", _p), ("G", _i), ("K", _i), ("P", _i), ("nu", _i), ("group_first", _i), ("group_count", _i),
                ("hip_stream", _p)]


class ShiftArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("nominal", _p), ("spline", _i), ("H", _i), ("P", _i), ("nu", _i),
                ("G", _i), ("group_first", _i), ("group_count", _i), ("hip_stream", _p)]


_ARGS = {"fork": ForkArgs, "sample": SampleArgs, "action": ActionArgs, "accumulate": AccumulateArgs, "select": SelectArgs,
         "shift": ShiftArgs}


_entries = _abi.EntryTable("rp_plan_", _ARGS, PlanError, "RP_PLAN_LIB", "librp_plan.so", "planner")
LIB_PATH = _entries.path
load_library, declare, make_args, call_raw, last_error, dim, _call = (
    _entries.load, _entries.declare, _entries.make_args, _entries.call_raw, _entries.last_error, _entries.dim, _entries.call)


def field_table(fields):
    """A ctypes array of rp_plan_field from (src address, dst address, row_bytes) triples."""
    fields = list(fields)
    if not 1 <= len(fields) <= MAX_FIELDS:
        raise PlanError(f"a fork takes 1 .. {MAX_FIELDS} fields per launch, got {len(fields)}")
    tab = (Field * len(fields))()
    for f, (src, dst, row_bytes) in zip(tab, fields):
        f.src, f.dst, f.row_bytes = src, dst, int(row_bytes)
    return tab


def fork(table, G, K, env_first=0, env_count=None, hip_stream=None):
    _call("fork", fields=table, n_fields=len(table), G=G, K=K, env_first=env_first,
          env_count=G * K - env_first if env_count is None else env_count, hip_stream=hip_stream)


def sample(nominal, sigma, lo, hi, knots, seed, round_, G, K, P, nu, env_first=0, env_count=None, hip_stream=None):
    _call("sample", nominal=nominal, sigma=sigma, lo=lo, hi=hi, knots=knots, G=G, K=K, P=P, nu=nu,
          env_first=env_first, env_count=G * K - env_first if env_count is None else env_count, hip_stream=hip_stream,
          **_abi.seed_args(seed, round_))


def action(knots, out, precision, spline, h, H, P, nu, n_rows, row_first=0, row_count=None, hip_stream=None):
    _call("action", knots=knots, out=out, precision=precision, spline=spline, h=h, H=H, P=P, nu=nu, n_rows=n_rows,
          row_first=row_first, row_count=n_rows - row_first if row_count is None else row_count, hip_stream=hip_stream)


def accumulate(ret, alive, reward, step_type, precision, weight, E, env_first=0, env_count=None, hip_stream=None):
    _call("accumulate", ret=ret, alive=alive, reward=reward, step_type=step_type, precision=precision, weight=float(weight),
          E=E, env_first=env_first, env_count=E - env_first if env_count is None else env_count, hip_stream=hip_stream)


def select(ret, knots, nominal, best_k, best_return, G, K, P, nu, group_first=0, group_count=None, hip_stream=None):
    _call("select", ret=ret, knots=knots, nominal=nominal, best_k=best_k, best_return=best_return, G=G, K=K, P=P, nu=nu,
          group_first=group_first, group_count=G - group_first if group_count is None else group_count,
          hip_stream=hip_stream)


def shift(nominal, spline, H, P, nu, G, group_first=0, group_count=None, hip_stream=None):
    _call("shift", nominal=nominal, spline=spline, H=H, P=P, nu=nu, G=G, group_first=group_first,
          group_count=G - group_first if group_count is None else group_count, hip_stream=hip_stream)


def check_plan_shape(spline: str, horizon: int, n_knots: int) -> int:
    """The ABI's spline code of `spline` ("zero" / "linear"); raises ValueError for what the library would refuse."""
    if spline not in SPLINES:
        raise ValueError(f"spline must be one of {sorted(SPLINES)}, got {spline!r}")
    H, P = int(horizon), int(n_knots)
    if H < 1 or P < 1:
        raise ValueError("horizon and n_knots must be >= 1")
    if spline == "linear" and P > 1 and (H < P or (H - 1) % (P - 1) != 0):
        raise ValueError(f"the linear spline needs (horizon - 1) % (n_knots - 1) == 0 with horizon >= n_knots "
                         f"(horizon = {H}, n_knots = {P})")
    return SPLINES[spline]


def match_state_views(real_views, plan_views, G: int, E: int):
    """Pairs the `state_views()` of the real (G envs) and of the planning environment (E envs): a list of
    (name, src tensor, dst tensor, row_bytes).  Refuses names, dtypes or per-row shapes that differ, rows that are not
    contiguous and tensors that share memory."""
    if list(real_views) != list(plan_views):
        raise ValueError(f"the environments' state differs: {sorted(set(real_views) ^ set(plan_views))} "
                         "(are both built with the same task arguments?)")
    out = []
    for name, src in real_views.items():
        dst = plan_views[name]
        if src.dtype != dst.dtype:
            raise ValueError(f"state {name!r}: dtype {src.dtype} in the real env, {dst.dtype} in the planning env")
        if src.shape[0] != G or dst.shape[0] != E or tuple(src.shape[1:]) != tuple(dst.shape[1:]):
            raise ValueError(f"state {name!r}: shape {tuple(src.shape)} in the real env and {tuple(dst.shape)} in the "
                             f"planning env, expected [{G}, ...] and [{E}, ...] with equal rows")
        if not src.is_contiguous() or not dst.is_contiguous():
            raise ValueError(f"state {name!r} is not contiguous")
        if src.device != dst.device:
            raise ValueError(f"state {name!r}: the environments live on different devices")
        row_bytes = int(np.prod(src.shape[1:], dtype=np.int64)) * src.element_size()
        if row_bytes < 1:
            continue
        s0, d0 = src.data_ptr(), dst.data_ptr()
        if s0 < d0 + E * row_bytes and d0 < s0 + G * row_bytes:
            raise ValueError(f"state {name!r}: the real and the planning env share memory")
        out.append((name, src, dst, row_bytes))
    return out


class PredictiveSampler:
    """Predictive sampling for every env of `real_env` at once.

    `make_env(n_envs)` builds the planning environment: the same task arguments, wrappers included where the plan is
    made in the wrapper's action space (a FingertipActionWrapper on both, or on neither).  It has G K envs, G =
    real_env.n_envs, K = `n_candidates`; row g K + k is candidate k of real env g, candidate 0 carries the nominal.
    A plan is `n_knots` knots of the action over `horizon` control steps ("linear" or "zero"-order spline); `sigma`
    (a scalar or one value per action entry, in the action's units) is the noise around the nominal, which starts at the
    spec's lower bound clamped to 0 where 0 is in range.  `gamma` discounts the rollouts' rewards.

    `plan()` launches, on torch's current stream and without reading anything back: shift (the nominal one step on,
    except right after construction or `set_nominal`), sample, fork (the real env's `state_views()` into the planning
    env's), active <- 1 and physics.forward(), H x (action, planning env step, accumulate), select, and the action of the
    winners' first step.  The real env is only read.  (A planning env of a single env -- G = K = 1 -- inherits
    Environment.step's host read of its reset flag.)"""

    def __init__(self, real_env, make_env, n_candidates: int, horizon: int, n_knots: int, spline: str = "linear",
                 sigma=0.1, gamma: float = 1.0, seed: int = 0):
        import torch
        load_library()
        self._spline = check_plan_shape(spline, horizon, n_knots)
        self.G, self.K, self.H, self.P = int(real_env.n_envs), int(n_candidates), int(horizon), int(n_knots)
        if self.K < 1:
            raise ValueError("n_candidates must be >= 1")
        self.E = self.G * self.K
        self._real = real_env
        self._plan = plan_env = make_env(self.E)
        if int(plan_env.n_envs) != self.E:
            raise ValueError(f"make_env({self.E}) returned an environment of {plan_env.n_envs} envs")
        spec, real_spec = plan_env.action_spec(), real_env.action_spec()
        if spec.shape != real_spec.shape or not (np.array_equal(spec.minimum, real_spec.minimum)
                                                 and np.array_equal(spec.maximum, real_spec.maximum)):
            raise ValueError(f"the planning env's action spec {spec.shape} differs from the real env's {real_spec.shape}")
        self.nu = int(spec.shape[0])
        phys = plan_env.physics
        self._dev, self._dtype = phys.device, phys.dtype
        if real_env.physics.dtype != phys.dtype:
            raise ValueError("the real and the planning env differ in precision")
        self._precision = 32 if phys.dtype == torch.float32 else 64
        plan_env.reset()   # (allocates every state tensor the fork writes; they are updated in place from here on)
        self._fields = match_state_views(real_env.state_views(), plan_env.state_views(), self.G, self.E)
        self._tables = [field_table([(s.data_ptr(), d.data_ptr(), rb) for _, s, d, rb in self._fields[i:i + MAX_FIELDS]])
                        for i in range(0, len(self._fields), MAX_FIELDS)]
        f64 = dict(dtype=torch.float64, device=self._dev)
        lo, hi = np.asarray(spec.minimum, np.float64), np.asarray(spec.maximum, np.float64)
        self._lo, self._hi = torch.as_tensor(lo, **f64).contiguous(), torch.as_tensor(hi, **f64).contiguous()
        sg = np.broadcast_to(np.asarray(sigma, np.float64), (self.nu,)).copy()
        if not (np.isfinite(sg).all() and (sg >= 0).all()):
            raise ValueError("sigma must be finite and >= 0")
        self._sigma = torch.as_tensor(sg, **f64).contiguous()
        self.gamma, self.seed, self._round = float(gamma), int(seed), 0
        start = np.clip(np.zeros(self.nu), lo, hi)
        self._nominal = torch.as_tensor(np.tile(start, (self.G, self.P, 1)), **f64).contiguous()
        self._knots = torch.zeros((self.E, self.P, self.nu), **f64)
        self._ret = torch.zeros(self.E, **f64)
        self._alive = torch.ones(self.E, dtype=torch.uint8, device=self._dev)
        self._best_k = torch.zeros(self.G, dtype=torch.int32, device=self._dev)
        self._best_return = torch.zeros(self.G, **f64)
        self._act = torch.zeros((self.E, self.nu), dtype=self._dtype, device=self._dev)
        self._first = torch.zeros((self.G, self.nu), dtype=self._dtype, device=self._dev)
        self._shift_pending = False
        self._keep = None

    # -- accessors ---------------------------------------------------------------------------------------------------
    @property
    def plan_env(self):
        return self._plan

    @property
    def real_env(self):
        return self._real

    @property
    def field_names(self):
        """The forked state, in table order."""
        return [name for name, *_ in self._fields]

    @property
    def nominal(self):
        """[G, P, nu] float64 (live): the plan the next `plan()` samples around, after its shift."""
        return self._nominal

    @property
    def knots(self):
        """[G K, P, nu] float64 (live): the candidates of the last `plan()`."""
        return self._knots

    @property
    def returns(self):
        """[G K] float64 (live): the candidates' returns of the last rollout."""
        return self._ret

    @property
    def best_k(self):
        return self._best_k

    @property
    def best_return(self):
        return self._best_return

    def set_nominal(self, nominal) -> None:
        """Seeds the plan: [G, P, nu], or [G, nu] / [nu] for a constant plan.  The next `plan()` samples around it as it
        is (no shift)."""
        import torch
        n = torch.as_tensor(nominal, device=self._dev).to(torch.float64)
        if n.dim() == 1:
            n = n[None, None, :]
        elif n.dim() == 2:
            n = n[:, None, :]
        self._nominal.copy_(n.expand(self.G, self.P, self.nu))
        self._shift_pending = False

    # -- the launches ------------------------------------------------------------------------------------------------
    def _stream(self):
        import torch
        return torch.cuda.current_stream(self._dev).cuda_stream

    def fork(self) -> None:
        """The real env's state into every candidate, then what `load_state_dict` does after its copies."""
        st = self._stream()
        for tab in self._tables:
            fork(tab, self.G, self.K, hip_stream=st)
        phys = self._plan.physics
        phys.active_mask.fill_(1)
        phys.forward()

    def rollout(self, knots=None):
        """Forks, then rolls `knots` ([G K, P, nu] float64 contiguous device tensor; default: the sampled candidates) out
        H control steps in the planning env.  Returns the candidates' returns [G K] (live)."""
        import torch
        knots = self._knots if knots is None else knots
        if (tuple(knots.shape) != (self.E, self.P, self.nu) or knots.dtype != torch.float64 or not knots.is_contiguous()
                or knots.device != self._dev):
            raise PlanError(f"rollout: knots must be a contiguous float64 device tensor {(self.E, self.P, self.nu)}")
        with torch.cuda.device(self._dev):
            st = self._stream()
            self.fork()
            self._ret.zero_()
            self._alive.fill_(1)
            weight, kept = 1.0, []
            for h in range(self.H):
                action(knots.data_ptr(), self._act.data_ptr(), self._precision, self._spline, h, self.H, self.P, self.nu,
                       self.E, hip_stream=st)
                ts = self._plan.step(self._act)
                if ts.reward is not None:   # (None: the reset of a single-env batch, Environment.step's dm_env case)
                    accumulate(self._ret.data_ptr(), self._alive.data_ptr(), ts.reward.data_ptr(), ts.step_type.data_ptr(),
                               self._precision, weight, self.E, hip_stream=st)
                kept.append(ts)          # alive until the kernels have run
                weight *= self.gamma
            self._keep = (knots, kept)
        return self._ret

    def plan(self):
        """One planning round; returns the [G, nu] first action of each group's winner (live, of the engine's dtype)."""
        import torch
        with torch.cuda.device(self._dev):
            st = self._stream()
            if self._shift_pending:
                shift(self._nominal.data_ptr(), self._spline, self.H, self.P, self.nu, self.G, hip_stream=st)
            sample(self._nominal.data_ptr(), self._sigma.data_ptr(), self._lo.data_ptr(), self._hi.data_ptr(),
                   self._knots.data_ptr(), self.seed, self._round, self.G, self.K, self.P, self.nu, hip_stream=st)
            self._round += 1
            self.rollout()
            select(self._ret.data_ptr(), self._knots.data_ptr(), self._nominal.data_ptr(), self._best_k.data_ptr(),
                   self._best_return.data_ptr(), self.G, self.K, self.P, self.nu, hip_stream=st)
            action(self._nominal.data_ptr(), self._first.data_ptr(), self._precision, self._spline, 0, self.H, self.P, self.nu,
                   self.G, hip_stream=st)
            self._shift_pending = True
        return self._first
