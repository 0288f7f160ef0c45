"""ctypes binding of the fused DroQ critic step's C ABI (include/learn/rp_critic.h, librp_critic.so): the forward pass of
every critic of the ensemble, the backward pass, Adam and the targets' Polyak step in two launches.

The entry points are module functions taking raw device addresses (`step`, `workspace_bytes`); `step` enqueues its two
kernels on the caller's HIP stream and reads nothing back.  `droq.DroQ(critic_step="fused")` is the learner that uses it.
Like the engine, the library has no CPU fallback: a missing library is an error.
"""

from __future__ import annotations

import ctypes
import math

from robopianist_amd import _abi, offpolicy
from robopianist_amd.learning import LearnError

EXPORTED_SYMBOLS = ("rp_critic_step", "rp_critic_workspace", "rp_critic_dim", "rp_critic_last_error")

MAX_CRITICS = offpolicy.MAX_CRITICS
COUNTER = 48   # the last Philox counter word of critic i, layer L is COUNTER + 2 i + L
STEP, ROWS_ONLY, APPLY_ONLY = 0, 1, 2   # `launches`: a step, or one of its two launches alone (for measurement)
PARAMS = ("w1", "b1", "w2", "b2", "w3", "b3", "g1", "be1", "g2", "be2")   # the order of rp_critic_set (droq.critic_entry's)

_p, _i, _u32, _f, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t


class Set(ctypes.Structure):
    """rp_critic_set: the ten tensors of one critic, of its m, v or target, or of where its gradients go."""
    _fields_ = [("t", _p * len(PARAMS))]


def step_fields(*rows):
    """The fields of a step block: the fused step's, with the block's own row dimensions `rows` between A and row_first."""
    return [("struct_size", _sz), ("obs", _p), ("action", _p), ("y", _p), ("mask", _p), ("mean", _p), ("inv_std", _p),
            ("obs_clip", _f), ("p", ctypes.POINTER(Set)), ("m", ctypes.POINTER(Set)), ("v", ctypes.POINTER(Set)),
            ("target", ctypes.POINTER(Set)), ("grad", ctypes.POINTER(Set)), ("n_critics", _i), ("q", _p),
            ("workspace", _p), ("workspace_bytes", _sz), ("drop_threshold", _u32), ("keep_scale", _f), ("ln_eps", _f),
            ("seed_lo", _u32), ("seed_hi", _u32), ("round", _u32), ("one_minus_beta1", _f), ("beta2", _f),
            ("one_minus_beta2", _f), ("step_size", _f), ("bc2_sqrt", _f), ("eps", _f), ("tau", _f), ("D", _i),
            ("H1", _i), ("H2", _i), ("A", _i), *rows, ("row_first", _i), ("row_count", _i), ("launches", _i),
            ("hip_stream", _p)]


class StepArgs(ctypes.Structure):
    _fields_ = step_fields(("B", _i))


class WorkspaceArgs(ctypes.Structure):
    _fields_ = [("struct_size", _sz), ("n_critics", _i), ("H1", _i), ("H2", _i), ("row_count", _i), ("bytes", _sz)]


_ARGS = {"step": StepArgs, "workspace": WorkspaceArgs}


_entries = _abi.EntryTable("rp_critic_", _ARGS, LearnError, "RP_CRITIC_LIB", "librp_critic.so", "DroQ critic step")
LIB_PATH = _entries.path
load_library, declare, make_args, call_raw, last_error, dim, _call = (
    _entries.load, _entries.declare, _entries.make_args, _entries.call_raw, _entries.last_error, _entries.dim, _entries.call)


def set_entry(tensors):
    """An rp_critic_set from ten tensors in PARAMS' order (None: a NULL pointer, for the optional gradients)."""
    s = Set()
    tensors = list(tensors)
    if len(tensors) != len(PARAMS):
        raise LearnError(f"a critic has {len(PARAMS)} tensors, got {len(tensors)}")
    for k, t in enumerate(tensors):
        s.t[k] = None if t is None else t.data_ptr()
    return s


def set_table(sets, n=None):
    """A ctypes array of rp_critic_set from a sequence of `Set`."""
    sets = list(sets)
    if not 1 <= len(sets) <= MAX_CRITICS or (n is not None and len(sets) != n):
        raise LearnError(f"the step takes 1 .. {MAX_CRITICS} critics per launch and as many sets of each kind, got {len(sets)}")
    tab = (Set * len(sets))()
    for i, s in enumerate(sets):
        tab[i] = s
    return tab


def workspace_bytes(n_critics, H1, H2, row_count) -> int:
    """The bytes `step` needs as its workspace for these sizes."""
    a = make_args("workspace", n_critics=n_critics, H1=H1, H2=H2, row_count=row_count)
    if call_raw("workspace", a) != 0:
        raise LearnError(last_error())
    return int(a.bytes)


def adam_scalars(lr, t, betas=(0.9, 0.999)):
    """(step_size, bc2_sqrt) of Adam's step number t >= 1, computed in double as torch computes them."""
    return float(lr) / (1.0 - betas[0] ** t), math.sqrt(1.0 - betas[1] ** t)


def step_keywords(obs, action, y, mask, mean, inv_std, obs_clip, p, m, v, target, q, workspace, workspace_bytes_, D, H1, H2, A,
                  rows, step_size, bc2_sqrt, eps=1e-8, betas=(0.9, 0.999), tau=0.005, grad=None, threshold=0, keep_scale=1.0,
                  ln_eps=1e-5, seed=0, round_=0, row_first=0, row_count=None, launches=STEP, hip_stream=None):
    """The keywords of a step block but its own row dimensions; `rows`: the rows that `row_count` defaults to the rest of."""
    tp = set_table(p)
    n = len(tp)
    tm, tv, tt = set_table(m, n), set_table(v, n), set_table(target, n)
    tg = None if grad is None else set_table(grad, n)
    return dict(obs=obs, action=action, y=y, mask=mask, mean=mean, inv_std=inv_std, obs_clip=float(obs_clip), p=tp, m=tm,
                v=tv, target=tt, grad=tg, n_critics=n, q=q, workspace=workspace, workspace_bytes=int(workspace_bytes_),
                drop_threshold=int(threshold), keep_scale=float(keep_scale), ln_eps=float(ln_eps),
                one_minus_beta1=1.0 - betas[0], beta2=betas[1], one_minus_beta2=1.0 - betas[1], step_size=float(step_size),
                bc2_sqrt=float(bc2_sqrt), eps=float(eps), tau=float(tau), D=D, H1=H1, H2=H2, A=A, row_first=row_first,
                row_count=rows - row_first if row_count is None else row_count, launches=int(launches),
                hip_stream=hip_stream, **_abi.seed_args(seed, round_))


def step(obs, action, y, mask, mean, inv_std, obs_clip, p, m, v, target, q, workspace, workspace_bytes_, D, H1, H2, A, B,
         step_size, bc2_sqrt, **options):
    """`p`, `m`, `v`, `target` (and `grad`, optional): sequences of `Set`, one per critic.  `threshold`:
    `droq.drop_threshold(p)`.  `step_size`, `bc2_sqrt`: `adam_scalars(lr, t)`.  `options`: `step_keywords`' (eps, betas,
    tau, grad, threshold, keep_scale, ln_eps, seed, round_, row_first, row_count, launches, hip_stream)."""
    _call("step", B=B, **step_keywords(obs, action, y, mask, mean, inv_std, obs_clip, p, m, v, target, q, workspace,
                                       workspace_bytes_, D, H1, H2, A, B, step_size, bc2_sqrt, **options))
