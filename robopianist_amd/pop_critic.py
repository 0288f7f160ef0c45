"""ctypes binding of the population's fused critic step (include/learn/rp_pop_critic.h, librp_pop_critic.so): `critic.step`
for every member of a population in the same two launches, on the members' blocked rows, their slices of the stacked
tensors and one workspace segment each.

The entry points are module functions taking raw device addresses (`step`, `workspace_bytes`); `step` enqueues its two
kernels on the caller's HIP stream and reads nothing back.  `population.DroQPopulation(critic_step="fused")` is the
learner that uses it.  Like the engine, the library has no CPU fallback: a missing library is an error.
"""

from __future__ import annotations

import ctypes

from robopianist_amd import _abi, critic
from robopianist_amd.critic import APPLY_ONLY, COUNTER, MAX_CRITICS, PARAMS, ROWS_ONLY, STEP, Set, adam_scalars, set_entry, set_table  # noqa: F401
from robopianist_amd.learning import LearnError

EXPORTED_SYMBOLS = ("rp_pop_critic_step", "rp_pop_critic_workspace", "rp_pop_critic_dim", "rp_pop_critic_last_error")

TILE_MAJOR, MEMBER_MAJOR = 0, 1      # the workgroup order of both launches (speed only): population's

_i, _sz = ctypes.c_int, ctypes.c_size_t


class StepArgs(ctypes.Structure):
    _fields_ = critic.step_fields(("P", _i), ("n", _i), ("grid_order", _i), ("member_first", _i), ("member_count", _i))


class WorkspaceArgs(ctypes.Structure):
    _fields_ = [("struct_size", _sz), ("n_critics", _i), ("H1", _i), ("H2", _i), ("row_count", _i), ("member_count", _i),
                ("bytes", _sz)]


_ARGS = {"step": StepArgs, "workspace": WorkspaceArgs}


_entries = _abi.EntryTable("rp_pop_critic_", _ARGS, LearnError, "RP_POP_CRITIC_LIB", "librp_pop_critic.so", "population critic step")
LIB_PATH = _entries.path
load_library, declare, make_args, call_raw, last_error, dim, _call = (
    _entries.load, _entries.declare, _entries.make_args, _entries.call_raw, _entries.last_error, _entries.dim, _entries.call)


def workspace_bytes(n_critics, H1, H2, row_count, member_count) -> int:
    """The bytes `step` needs as its workspace for these sizes: `member_count` segments of `critic.workspace_bytes`."""
    a = make_args("workspace", n_critics=n_critics, H1=H1, H2=H2, row_count=row_count, member_count=member_count)
    if call_raw("workspace", a) != 0:
        raise LearnError(last_error())
    return int(a.bytes)


def step(obs, action, y, mask, mean, inv_std, obs_clip, p, m, v, target, q, workspace, workspace_bytes_, D, H1, H2, A, P, n,
         step_size, bc2_sqrt, member_first=0, member_count=None, grid_order=None, **options):
    """`critic.step` with `p`, `m`, `v`, `target` (and `grad`, optional) the `Set`s of the bases of the stacked tensors
    [P][...].  `n`: minibatch rows per member; the arrays hold P n rows, member p's at [p n, (p + 1) n).  `step_size`,
    `bc2_sqrt`: `adam_scalars(lr, t)`, shared by the members."""
    shared = critic.step_keywords(obs, action, y, mask, mean, inv_std, obs_clip, p, m, v, target, q, workspace,
                                  workspace_bytes_, D, H1, H2, A, n, step_size, bc2_sqrt, **options)
    _call("step", P=P, n=n, grid_order=dim("default_grid_order") if grid_order is None else int(grid_order),
          member_first=member_first, member_count=P - member_first if member_count is None else member_count, **shared)
