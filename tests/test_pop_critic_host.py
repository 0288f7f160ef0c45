"""Host tests of the population's fused critic step (include/learn/rp_pop_critic.h, robopianist_amd/pop_critic.py): the
binding's symbols, struct sizes and names, the workspace query, the argument validation (refused calls return before
anything touches a device) and population.DroQPopulation's `critic_step` option with its checkpoint.  What the kernels
compute is test_gpu_pop_critic.py's.
"""

from __future__ import annotations

import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_offpolicy_host import _SpecEnv  # noqa: E402
from robopianist_amd import critic, droq, learning, pop_critic, population  # noqa: E402


# ---- the binding -------------------------------------------------------------------------------------------------------
def test_exported_symbols_dims_and_struct_sizes():
    L = pop_critic.load_library()
    assert set(pop_critic.EXPORTED_SYMBOLS) == {"rp_pop_critic_step", "rp_pop_critic_workspace", "rp_pop_critic_dim",
                                                "rp_pop_critic_last_error"}
    assert [getattr(L, s) for s in pop_critic.EXPORTED_SYMBOLS]
    # each library keeps its own symbols
    for name in critic.EXPORTED_SYMBOLS + population.EXPORTED_SYMBOLS + droq.EXPORTED_SYMBOLS:
        assert not hasattr(L, name), name
    for other in (critic.load_library(), population.load_library(), droq.load_library()):
        assert not any(hasattr(other, s) for s in pop_critic.EXPORTED_SYMBOLS)
    # the names of rp_critic_dim and the grid orders of rp_pop_dim
    for name in ("max_critics", "tile_rows", "stage_rows", "launches", "counter", "max_hidden", "max_actions"):
        assert pop_critic.dim(name) == critic.dim(name) > 0, name
    assert pop_critic.dim("launches") == 2 and pop_critic.dim("counter") == pop_critic.COUNTER == 48
    assert pop_critic.dim("max_critics") == pop_critic.MAX_CRITICS == 4 and pop_critic.dim("max_hidden") == learning.MAX_HIDDEN
    for name in ("tile_major", "member_major", "default_grid_order"):
        assert pop_critic.dim(name) == population.dim(name), name
    assert (pop_critic.TILE_MAJOR, pop_critic.MEMBER_MAJOR) == (population.TILE_MAJOR, population.MEMBER_MAJOR)
    assert pop_critic.dim("nothing") == -1 and pop_critic.dim("blocked") == -1
    assert (pop_critic.STEP, pop_critic.ROWS_ONLY, pop_critic.APPLY_ONLY) == (critic.STEP, critic.ROWS_ONLY, critic.APPLY_ONLY)
    assert pop_critic.Set is critic.Set and pop_critic.PARAMS == critic.PARAMS
    # the layouts of the header on the LP64 ABI: rp_critic_step_args with (P, n, grid_order, member_first, member_count)
    # where it has B, and the query with member_count
    assert ctypes.sizeof(pop_critic.StepArgs) == ctypes.sizeof(critic.StepArgs) + 16 == 248
    assert ctypes.sizeof(pop_critic.WorkspaceArgs) == 40
    assert [f[0] for f in pop_critic.StepArgs._fields_ if f not in critic.StepArgs._fields_] == \
        ["P", "n", "grid_order", "member_first", "member_count"]
    a = pop_critic.make_args("step")
    assert pop_critic.call_raw("step", a) != 0 and "struct_size" not in pop_critic.last_error()
    a.struct_size -= 8
    assert pop_critic.call_raw("step", a) != 0 and "struct_size" in pop_critic.last_error()
    w = pop_critic.make_args("workspace", n_critics=2, H1=16, H2=16, row_count=5, member_count=2)
    w.struct_size += 8
    assert pop_critic.call_raw("workspace", w) != 0 and "struct_size" in pop_critic.last_error()


def test_workspace_is_one_single_learner_workspace_per_member():
    for n, H1, H2, R in ((1, 16, 16, 5), (2, 256, 256, 512), (4, 48, 16, 17), (3, 32, 32, 70)):
        one = critic.workspace_bytes(n, H1, H2, R)
        assert one % 16 == 0                                                 # every member's segment stays 16-byte aligned
        for members in (0, 1, 3, 16):
            assert pop_critic.workspace_bytes(n, H1, H2, R, members) == members * one
    assert pop_critic.workspace_bytes(2, 16, 16, 0, 5) == 0
    for bad in (dict(n_critics=0), dict(n_critics=5), dict(H1=8), dict(H2=272), dict(row_count=-1), dict(member_count=-1)):
        with pytest.raises(pop_critic.LearnError, match="rp_pop_critic_workspace"):
            pop_critic.workspace_bytes(**dict(dict(n_critics=2, H1=16, H2=16, row_count=4, member_count=2), **bad))


_A = 0x1000   # a non-null address: a refused call never reads it


def _refused(match, **values):
    assert pop_critic.call_raw("step", pop_critic.make_args("step", **values)) != 0
    assert match in pop_critic.last_error(), pop_critic.last_error()
    assert pop_critic.last_error().startswith("rp_pop_critic_step: ")


def _accepted(**values):
    assert pop_critic.call_raw("step", pop_critic.make_args("step", **values)) == 0, pop_critic.last_error()


class _Fake:
    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address


def _set(hole=None):
    return critic.set_entry([None if k == hole else _Fake(_A) for k in range(10)])


def test_argument_validation_refuses_before_any_launch():
    tab = critic.set_table([_set(), _set()])
    need = pop_critic.workspace_bytes(2, 16, 32, 4, 3)
    sa = dict(obs=_A, action=_A, y=_A, mask=_A, mean=_A, inv_std=_A, obs_clip=5.0, p=tab, m=tab, v=tab, target=tab, grad=tab,
              n_critics=2, q=_A, workspace=_A, workspace_bytes=need, drop_threshold=7, keep_scale=1.0, ln_eps=1e-5,
              one_minus_beta1=0.1, beta2=0.999, one_minus_beta2=0.001, step_size=1e-3, bc2_sqrt=0.5, eps=1e-8, tau=0.005,
              D=3, H1=16, H2=32, A=2, P=3, n=8, grid_order=pop_critic.MEMBER_MAJOR, member_first=0, member_count=3,
              row_first=2, row_count=4)
    # what rp_pop_target refuses about the population
    for P in (0, -1):
        _refused("P must be >= 1", **dict(sa, P=P))
    for first, count in ((0, 4), (3, 1), (-1, 1), (2, 2), (0, -1)):
        _refused("the member range", **dict(sa, member_first=first, member_count=count))
    _refused("n must be >= 1", **dict(sa, n=0, row_first=0, row_count=0))
    _refused("the row range", **dict(sa, row_first=5))
    _refused("the row range", **dict(sa, row_first=-1, row_count=1))
    _refused("the row range", **dict(sa, row_first=0, row_count=9))
    _refused("must be < 2^31", **dict(sa, n=2 ** 30))
    for order in (2, -1):
        _refused("grid_order must be", **dict(sa, grid_order=order))
    # what rp_critic_step refuses, under this library's name
    for name in ("obs", "action", "y", "mask", "mean", "inv_std", "q"):
        _refused("a pointer is NULL", **dict(sa, **{name: None}))
    _refused("critics is NULL", **dict(sa, p=None))
    for n in (0, 5):
        _refused("n_critics", **dict(sa, n_critics=n))
    _refused("obs_clip", **dict(sa, obs_clip=-1.0))
    for bad in (0.0, -1.0, float("nan")):
        for name in ("keep_scale", "ln_eps", "step_size", "bc2_sqrt", "eps"):
            _refused(f"{name} must be > 0", **dict(sa, **{name: bad}))
    for bad in (-0.01, 1.5, float("nan")):
        _refused("tau must lie in [0, 1]", **dict(sa, tau=bad))
    _refused("D must be", **dict(sa, D=0))
    for h in (0, 8, 24, 272):
        _refused("H1 must be", **dict(sa, H1=h))
        _refused("H2 must be", **dict(sa, H2=h))
    for A in (0, 129):
        _refused("A must be", **dict(sa, A=A))
    for k in range(10):
        holed = critic.set_table([_set(), _set(k)])
        _refused("the critic 1 has a NULL", **dict(sa, p=holed))
        _refused("the m of critic 1 has a NULL", **dict(sa, m=holed))
        _refused("the v of critic 1 has a NULL", **dict(sa, v=holed))
        _refused("the target of critic 1 has a NULL", **dict(sa, target=holed))
        _accepted(**dict(sa, grad=holed, row_count=0))                       # every gradient pointer is optional
    _refused("m and v must not be NULL", **dict(sa, m=None))
    _refused("m and v must not be NULL", **dict(sa, v=None))
    _refused("target is NULL", **dict(sa, target=None))
    for bad in (-1, 3):
        _refused("launches must be", **dict(sa, launches=bad))
    # the workspace: one segment per member of the range
    _refused("workspace is NULL", **dict(sa, workspace=None))
    _refused("16-byte aligned", **dict(sa, workspace=_A + 4))
    _refused(f"is smaller than the {need} this step needs", **dict(sa, workspace_bytes=need - 1))
    _refused("is smaller than", **dict(sa, workspace_bytes=critic.workspace_bytes(2, 16, 32, 4)))   # one member's
    _refused("is smaller than", **dict(sa, workspace_bytes=0))
    two = pop_critic.workspace_bytes(2, 16, 32, 4, 2)
    _refused(f"is smaller than the {two}", **dict(sa, member_first=1, member_count=2, workspace_bytes=two - 16))
    # accepted: no row or no member (nothing is launched; the workspace may be empty), with or without gradient pointers
    _accepted(**dict(sa, row_count=0, workspace_bytes=0))
    _accepted(**dict(sa, row_first=8, row_count=0, grad=None))
    _accepted(**dict(sa, member_first=3, member_count=0, workspace_bytes=0))
    _accepted(**dict(sa, member_first=1, member_count=0, tau=1.0))
    with pytest.raises(TypeError):
        pop_critic.make_args("step", nothing=1)
    # the module function raises the library's message
    with pytest.raises(pop_critic.LearnError, match="rp_pop_critic_step: the member range"):
        pop_critic.step(_A, _A, _A, _A, _A, _A, 5.0, [_set()], [_set()], [_set()], [_set()], _A, _A, 0, 3, 16, 32, 2, 3, 8,
                        1e-3, 0.5, member_first=2, member_count=2)
    with pytest.raises(pop_critic.LearnError, match="as many sets of each kind"):
        pop_critic.step(_A, _A, _A, _A, _A, _A, 5.0, [_set(), _set()], [_set()], [_set()], [_set()], _A, _A, 0, 3, 16, 32, 2,
                        3, 8, 1e-3, 0.5)


# ---- the learner's option ------------------------------------------------------------------------------------------------
def _population(P=3, E=6, seed=5, **kw):
    args = dict(hidden=(16, 32), n_critics=2, capacity=4, batch_size=24, lr=1e-2, tau=0.25, seed=seed, dropout=0.25, utd=2)
    args.update(kw)
    return population.DroQPopulation(_SpecEnv(E, (4, 3), 3), P, **args)


# what DroQPopulation.state_dict() held before the option existed
PLAIN_KEYS = {"members", "droq", "actor", "critics", "targets", "log_alpha", "gamma", "target_entropy", "optimizers",
              "normalizer", "seed", "round", "n_written", "generator", "newest", "episodes"}


def test_the_option_its_state_and_the_cross_mode_checkpoint():
    for bad in ("nonsense", "", None, "Fused"):
        with pytest.raises(ValueError, match="critic_step must be"):
            _population(critic_step=bad)
    plain, fused = _population(), _population(critic_step="fused")
    assert plain.critic_mode == "torch" and _population(critic_step="torch").critic_mode == "torch" and fused.critic_mode == "fused"
    # torch mode: everything as it was
    assert not hasattr(plain, "_c_m") and not hasattr(plain, "_u_q")
    sd_plain = plain.state_dict()
    assert set(sd_plain) == PLAIN_KEYS and sd_plain["droq"] == {"dropout": 0.25, "utd": 2, "ln_eps": 1e-5}
    assert set(plain.state_dict(include_replay=True)) == PLAIN_KEYS | {"replay"}
    # the same seed draws the same networks in both modes
    assert all(torch.equal(x, y) for a, b in zip(plain.critics, fused.critics) for x, y in zip(a.parameters(), b.parameters()))
    # stacked m, v per tensor in the order of the ABI, zero; one step count; the workspace of P segments of one range; q
    assert len(fused._c_m) == len(fused._c_v) == 2 and fused._c_t == 0
    shapes = [tuple(t.shape) for t in fused._c_m[1]]
    assert shapes == [(3, 16, 10), (3, 16), (3, 32, 16), (3, 32), (3, 1, 32), (3, 1), (3, 16), (3, 16), (3, 32), (3, 32)]
    assert shapes == [tuple(t.shape) for t in fused._critic_tensors(fused.critics[1])]
    assert all(not bool(t.any()) for group in (fused._c_m, fused._c_v) for net in group for t in net)
    assert fused._c_bytes == 3 * critic.workspace_bytes(2, 16, 32, 24) and fused._c_ws.numel() * 4 >= fused._c_bytes
    assert tuple(fused._u_q.shape) == (2, 3 * 2 * 24)
    sd = fused.state_dict()
    assert set(sd) == PLAIN_KEYS | {"critic_adam"}
    assert sd["droq"] == {"dropout": 0.25, "utd": 2, "ln_eps": 1e-5, "critic_step": "fused"}
    assert set(sd["critic_adam"]) == {"m", "v", "t"} and sd["critic_adam"]["t"] == 0 and len(sd["critic_adam"]["m"][1]) == 10
    fused._c_m[1][3].fill_(2.0)
    fused._c_v[0][0][2].fill_(0.5)
    fused._c_t = 7
    sd = fused.state_dict()
    again = _population(critic_step="fused", seed=9)
    again.load_state_dict(sd)
    assert again._c_t == 7 and bool((again._c_m[1][3] == 2.0).all()) and not bool(again._c_m[1][2].any())
    assert bool((again._c_v[0][0][2] == 0.5).all()) and not bool(again._c_v[0][0][:2].any())
    fused._c_m[1][3].fill_(3.0)
    assert bool((sd["critic_adam"]["m"][1][3] == 2.0).all())                 # a snapshot, not a view
    with pytest.raises(ValueError, match="written with critic_step = fused, this population has critic_step = torch"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="written with critic_step = torch, this population has critic_step = fused"):
        fused.load_state_dict(sd_plain)
    # a fused step is a step on a range of the population's own minibatches
    with pytest.raises(population.LearnError, match="range of the population's own minibatches"):
        fused.critic_step({k: v.clone() for k, v in fused.minibatch().items()})
    assert fused._fused_range(fused.minibatch()) == 1
    fused._range = 0
    assert fused._fused_range(fused.minibatch()) == 0
    mixed = dict(fused.minibatch(), y=plain.minibatch()["y"])
    with pytest.raises(population.LearnError, match="range of the population's own minibatches"):
        fused.critic_step(mixed)
    half = {k: v[:, :12] for k, v in fused.minibatch().items()}
    with pytest.raises(population.LearnError, match="range of the population's own minibatches"):
        fused.critic_step(half)
    one = _population(P=1, E=2, critic_step="fused")
    assert one._fused_range(one.minibatch()) == 1 and one._c_bytes == critic.workspace_bytes(2, 16, 32, 24)
