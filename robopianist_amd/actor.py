"""ctypes binding of the fused DroQ actor and temperature step's C ABI (include/learn/rp_actor.h, librp_actor.so): the
policy at the rows' observations, every live critic at the policy's action, the minimum over the ensemble, the backward
pass through the selected critic's action input, the squashed-Gaussian head and the tanh layers, Adam on the actor and on
log_alpha, and the step's statistics, in two launches.

The entry points are module functions taking raw device addresses (`step`, `workspace_bytes`); `step` enqueues its two
kernels on the caller's HIP stream and reads nothing back.  `droq.DroQ(actor_step="fused")` is the learner that uses it.
Like the engine, the library has no CPU fallback: a missing library is an error.
"""

from __future__ import annotations

import ctypes

from robopianist_amd import _abi, critic, offpolicy
from robopianist_amd.learning import LearnError

EXPORTED_SYMBOLS = ("rp_actor_step", "rp_actor_workspace", "rp_actor_dim", "rp_actor_last_error")

MAX_CRITICS = offpolicy.MAX_CRITICS
NOISE_COUNTER = 64   # the last Philox counter words of the step's draw are NOISE_COUNTER + 0 .. 2
COUNTER = 80         # the last Philox counter word of critic i, layer L is COUNTER + 2 i + L
LAUNCHES = 2
STEP, ROWS_ONLY, APPLY_ONLY = 0, 1, 2   # `launches`: a step, or one of its two launches alone (for measurement)
PARAMS = ("w1", "b1", "w2", "b2", "w3", "b3")   # the order of rp_actor_set
STATS = ("actor_loss", "alpha_loss", "alpha", "entropy", "masked")   # the order of `stats`

_p, _i, _u32, _f, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t


class Set(ctypes.Structure):
    """rp_actor_set: the six tensors of the actor, of its m or v, or of where its gradients go."""
    _fields_ = [("t", _p * len(PARAMS))]


class Adam(ctypes.Structure):
    """rp_actor_adam: Adam's scalars of one optimiser at its own step count."""
    _fields_ = [("one_minus_beta1", _f), ("beta2", _f), ("one_minus_beta2", _f), ("step_size", _f), ("bc2_sqrt", _f),
                ("eps", _f)]


class StepArgs(ctypes.Structure):
    _fields_ = [("struct_size", _sz), ("obs", _p), ("mask", _p), ("mean", _p), ("inv_std", _p), ("obs_clip", _f),
                ("p", Set), ("m", Set), ("v", Set), ("grad", Set), ("critics", ctypes.POINTER(critic.Set)),
                ("n_critics", _i), ("log_alpha", _p), ("log_alpha_m", _p), ("log_alpha_v", _p), ("log_alpha_grad", _p),
                ("target_entropy", _f), ("log_std_min", _f), ("log_std_max", _f), ("workspace", _p),
                ("workspace_bytes", _sz), ("drop_threshold", _u32), ("keep_scale", _f), ("ln_eps", _f), ("seed_lo", _u32),
                ("seed_hi", _u32), ("round", _u32), ("actor_adam", Adam), ("alpha_adam", Adam), ("action", _p),
                ("logp", _p), ("q_min", _p), ("stats", _p), ("D", _i), ("H1", _i), ("H2", _i), ("A", _i), ("B", _i),
                ("row_first", _i), ("row_count", _i), ("launches", _i), ("hip_stream", _p)]


class WorkspaceArgs(ctypes.Structure):
    _fields_ = [("struct_size", _sz), ("H1", _i), ("H2", _i), ("A", _i), ("row_count", _i), ("bytes", _sz)]


_ARGS = {"step": StepArgs, "workspace": WorkspaceArgs}


_entries = _abi.EntryTable("rp_actor_", _ARGS, LearnError, "RP_ACTOR_LIB", "librp_actor.so", "DroQ actor step")
LIB_PATH = _entries.path
load_library, declare, make_args, call_raw, last_error, dim, _call = (
    _entries.load, _entries.declare, _entries.make_args, _entries.call_raw, _entries.last_error, _entries.dim, _entries.call)


def set_entry(tensors=None):
    """An rp_actor_set from six tensors in PARAMS' order (None: a NULL pointer; no argument: all NULL, for the optional
    gradients)."""
    s = Set()
    tensors = [None] * len(PARAMS) if tensors is None else list(tensors)
    if len(tensors) != len(PARAMS):
        raise LearnError(f"the actor has {len(PARAMS)} tensors, got {len(tensors)}")
    for k, t in enumerate(tensors):
        s.t[k] = None if t is None else t.data_ptr()
    return s


def adam_entry(lr, t, betas=(0.9, 0.999), eps=1e-8):
    """An rp_actor_adam of step number t >= 1 (`critic.adam_scalars`: torch's doubles, rounded to float32 here)."""
    step_size, bc2_sqrt = critic.adam_scalars(lr, t, betas)
    return Adam(1.0 - betas[0], betas[1], 1.0 - betas[1], step_size, bc2_sqrt, float(eps))


def workspace_bytes(H1, H2, A, row_count) -> int:
    """The bytes `step` needs as its workspace for these sizes."""
    a = make_args("workspace", H1=H1, H2=H2, A=A, row_count=row_count)
    if call_raw("workspace", a) != 0:
        raise LearnError(last_error())
    return int(a.bytes)


def step(obs, mask, mean, inv_std, obs_clip, p, m, v, critics, log_alpha, log_alpha_m, log_alpha_v, target_entropy,
         log_std_bounds, workspace, workspace_bytes_, stats, D, H1, H2, A, B, actor_adam, alpha_adam, grad=None,
         log_alpha_grad=None, action=None, logp=None, q_min=None, threshold=0, keep_scale=1.0, ln_eps=1e-5, seed=0,
         round_=0, row_first=0, row_count=None, launches=STEP, hip_stream=None):
    """`p`, `m`, `v` (and `grad`, optional): `Set`.  `critics`: a sequence of `critic.Set`, read only.  `actor_adam`,
    `alpha_adam`: `adam_entry(lr, t)`.  `threshold`: `droq.drop_threshold(p)`.  The addresses `log_alpha*`, `stats`
    (five floats, STATS' order) and the optional per-row outputs are device memory."""
    tab = critic.set_table(critics)
    _call("step", obs=obs, mask=mask, mean=mean, inv_std=inv_std, obs_clip=float(obs_clip), p=p, m=m, v=v,
          grad=set_entry() if grad is None else grad, critics=tab, n_critics=len(tab), log_alpha=log_alpha,
          log_alpha_m=log_alpha_m, log_alpha_v=log_alpha_v, log_alpha_grad=log_alpha_grad,
          target_entropy=float(target_entropy), log_std_min=float(log_std_bounds[0]), log_std_max=float(log_std_bounds[1]),
          workspace=workspace, workspace_bytes=int(workspace_bytes_), drop_threshold=int(threshold),
          keep_scale=float(keep_scale), ln_eps=float(ln_eps), actor_adam=actor_adam, alpha_adam=alpha_adam, action=action,
          logp=logp, q_min=q_min, stats=stats, D=D, H1=H1, H2=H2, A=A, B=B, row_first=row_first,
          row_count=B - row_first if row_count is None else row_count, launches=int(launches), hip_stream=hip_stream,
          **_abi.seed_args(seed, round_))
