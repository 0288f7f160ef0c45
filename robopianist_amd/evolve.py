"""ctypes binding of population-based training's C ABI (include/learn/rp_evolve.h, librp_evolve.so): the members' fitness
windows (`fold`), the decision who copies whom with the perturbed hyper-parameters (`plan`) and the copy of the members'
slices of the stacked tensors (`copy`).

The entry points are module functions taking raw device addresses; `fold` and `plan` enqueue one kernel each on the
caller's HIP stream, `copy` one per `MAX_FIELDS` fields, and nothing is read back.
`population.DroQPopulation(evolve={...})` is the learner that uses it; the library is loaded at the first call, so a
population without the option never opens it.  Like the engine, the library has no CPU fallback: a missing library is an
error.
"""

from __future__ import annotations

import ctypes

from robopianist_amd import _abi
from robopianist_amd.learning import LearnError

EXPORTED_SYMBOLS = ("rp_evolve_fold", "rp_evolve_plan", "rp_evolve_copy", "rp_evolve_dim", "rp_evolve_last_error")

MAX_MEMBERS, MAX_COPY_MEMBERS, MAX_FIELDS, CHUNK_WORDS = 256, 65535, 64, 4096
COUNTER = 96   # the last Philox counter word of the plan's draw

_p, _i, _u32, _f, _d, _ll = (ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_float, ctypes.c_double,
                             ctypes.c_longlong)


class Field(ctypes.Structure):
    """rp_evolve_field."""
    _fields_ = [("base", _p), ("slice_words", _ll)]


class FoldArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("done_return", _p), ("done_count", _p), ("fit_sum", _p),
                ("fit_count", _p), ("E", _i), ("P", _i), ("hip_stream", _p)]


class PlanArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("fit_sum", _p), ("fit_count", _p), ("source", _p), ("gamma", _p),
                ("target_entropy", _p), ("min_gap", _d), ("min_episodes", _ll), ("up", _f), ("down", _f),
                ("gamma_lo", _f), ("gamma_hi", _f), ("entropy_lo", _f), ("entropy_hi", _f), ("seed_lo", _u32),
                ("seed_hi", _u32), ("generation", _u32), ("P", _i), ("percent", _i), ("hip_stream", _p)]


class CopyArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("fields", ctypes.POINTER(Field)), ("source", _p), ("n_fields", _i),
                ("P", _i), ("launches", _i), ("hip_stream", _p)]


_ARGS = {"fold": FoldArgs, "plan": PlanArgs, "copy": CopyArgs}


_entries = _abi.EntryTable("rp_evolve_", _ARGS, LearnError, "RP_EVOLVE_LIB", "librp_evolve.so", "population-based training")
LIB_PATH = _entries.path
load_library, declare, make_args, call_raw, last_error, dim, _call = (
    _entries.load, _entries.declare, _entries.make_args, _entries.call_raw, _entries.last_error, _entries.dim, _entries.call)


def field_table(fields):
    """A ctypes array of rp_evolve_field from a sequence of (base address, slice_words)."""
    fields = list(fields)
    tab = (Field * max(len(fields), 1))()
    for i, (base, words) in enumerate(fields):
        tab[i].base, tab[i].slice_words = base, int(words)
    return tab


def launches_for(n_fields: int, P: int = 2) -> int:
    """The launches `copy` enqueues for a table of `n_fields` fields: ceil(n_fields / MAX_FIELDS); none with one member."""
    return 0 if P == 1 else -(-int(n_fields) // MAX_FIELDS)


def fold(done_return, done_count, fit_sum, fit_count, E, P, hip_stream=None):
    """The ended-episode counters [E] of every env into its member's window `fit_sum`, `fit_count` [P] (one launch)."""
    _call("fold", done_return=done_return, done_count=done_count, fit_sum=fit_sum, fit_count=fit_count, E=E, P=P,
          hip_stream=hip_stream)


def plan(fit_sum, fit_count, source, P, percent=25, min_episodes=1, min_gap=0.0, factors=(0.8, 1.25), gamma=None,
         gamma_bounds=(0.0, 1.0), target_entropy=None, entropy_bounds=(-float("inf"), float("inf")), seed=0, generation=0,
         hip_stream=None):
    """`source` [P] int32 from the windows, which are cleared; `gamma`, `target_entropy`: device addresses of [P] float32
    explored in place, or None.  `factors`: (down, up).  One launch."""
    s = _abi.seed_args(seed, generation)
    _call("plan", fit_sum=fit_sum, fit_count=fit_count, source=source, gamma=gamma, target_entropy=target_entropy,
          min_gap=float(min_gap), min_episodes=int(min_episodes), down=float(factors[0]), up=float(factors[1]),
          gamma_lo=float(gamma_bounds[0]), gamma_hi=float(gamma_bounds[1]), entropy_lo=float(entropy_bounds[0]),
          entropy_hi=float(entropy_bounds[1]), seed_lo=s["seed_lo"], seed_hi=s["seed_hi"], generation=s["round"], P=P,
          percent=int(percent), hip_stream=hip_stream)


def copy(fields, source, P, hip_stream=None) -> int:
    """Slice p of every field takes slice source[p] where the two differ.  `fields`: a sequence of (base address,
    slice_words); returns the launches enqueued (`launches_for`)."""
    fields = list(fields)
    a = make_args("copy", fields=field_table(fields) if fields else None, source=source, n_fields=len(fields), P=P,
                  hip_stream=hip_stream)
    if call_raw("copy", a) != 0:
        raise LearnError(last_error())
    return int(a.launches)
