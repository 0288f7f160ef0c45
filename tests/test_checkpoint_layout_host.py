"""The layout of the off-policy learners' checkpoints, pinned: SAC, DroQ and DroQPopulation (P = 1 and P = 3), the DroQ
learners with the torch and with the fused critic step.  No GPU: the learners are built on the CPU, where the fused mode
only asks its library for the workspace's size.
"""

from __future__ import annotations

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import learn_reference as lr  # noqa: E402
from test_offpolicy_host import _SpecEnv  # noqa: E402
from robopianist_amd import droq, offpolicy, population  # noqa: E402

D, A, C, B, UTD, H1, H2 = 7, 3, 4, 24, 2, 16, 32
F32, F64, I32, I64 = "torch.float32", "torch.float64", "torch.int32", "torch.int64"
SIZES = dict(hidden=(H1, H2), n_critics=2, capacity=C, batch_size=B, seed=5)


def _learner(kind, P, mode):
    E = 2 if P == 1 else 6
    env = _SpecEnv(E, (4, 3), A)
    if kind == "sac":
        return offpolicy.SAC(env, **SIZES)
    if kind == "droq":
        return droq.DroQ(env, utd=UTD, critic_step=mode, **SIZES)
    return population.DroQPopulation(env, P, utd=UTD, critic_step=mode, **SIZES)


def _tree(sd):
    return {k: {n: lr.adam_tree(o) for n, o in v.items()} if k == "optimizers" else lr.state_tree(v) for k, v in sd.items()}


def _expected(kind, P, mode):
    """The tree of `state_dict(include_replay=True)`: tensors as (dtype, shape), other leaves as their type's name."""
    E = 2 if P == 1 else 6
    lead = (P,) if kind == "population" else ()          # the stacked tensors' leading dimension
    t = lambda *shape: (F32, lead + shape)
    actor = {"0.weight": t(H1, D), "0.bias": t(H1), "2.weight": t(H2, H1), "2.bias": t(H2), "4.weight": t(2 * A, H2),
             "4.bias": t(2 * A)}
    if kind == "sac":
        critic = lr.mlp_tree(D + A, 1)
    else:                                                # Linear, Dropout, LayerNorm, ReLU twice, Linear
        critic = {"0.weight": t(H1, D + A), "0.bias": t(H1), "2.weight": t(H1), "2.bias": t(H1), "4.weight": t(H2, H1),
                  "4.bias": t(H2), "6.weight": t(H2), "6.bias": t(H2), "8.weight": t(1, H2), "8.bias": t(1)}
    tree = {
        "actor": actor, "critics": [critic] * 2, "targets": [critic] * 2, "log_alpha": (F32, lead or (1,)),
        "optimizers": {"actor": {"state": {}, "params": [list(range(6))]},
                       "critic": {"state": {}, "params": [list(range(2 * len(critic)))]},
                       "alpha": {"state": {}, "params": [[0]]}},
        "normalizer": {"count": "float", "mean": (F64, lead + (D,)), "M2": (F64, lead + (D,)), "mean_f32": t(D),
                       "inv_std_f32": t(D)},
        "seed": "int", "round": "int", "n_written": "int", "generator": ("torch.uint8", (5056,)),
        "newest": {"obs": (F32, (E, D)), "reward": (F32, (E,)), "discount": (F32, (E,)), "step_type": (I32, (E,))},
        "episodes": {"ep_return": (F64, (E,)), "ep_len": (I32, (E,)), "done_return": (F64, (E,)), "done_len": (I64, (E,)),
                     "done_count": (I32, (E,))},
        "replay": {"obs": (F32, (C, E, D)), "reward": (F32, (C, E)), "discount": (F32, (C, E)), "step_type": (I32, (C, E)),
                   "action": (F32, (C, E, A))}}
    if kind != "sac":
        tree["droq"] = {"dropout": "float", "utd": "int", "ln_eps": "float"}
    if mode == "fused":
        tree["droq"]["critic_step"] = "str"
        abi_order = [t(H1, D + A), t(H1), t(H2, H1), t(H2), t(1, H2), t(1), t(H1), t(H1), t(H2), t(H2)]
        tree["critic_adam"] = {"m": [abi_order] * 2, "v": [abi_order] * 2, "t": "int"}
    if kind == "population":
        tree.update(members="int", gamma=(F32, (P,)), target_entropy=(F32, (P,)))
    return tree


CASES = [("sac", None, "torch")] + [(kind, P, mode) for kind, P in (("droq", None), ("population", 1), ("population", 3))
                                    for mode in ("torch", "fused")]


@pytest.mark.parametrize("kind,P,mode", CASES, ids=lambda v: str(v))
def test_checkpoint_trees_are_pinned(kind, P, mode):
    """Every key path of `state_dict(include_replay=True)` with its leaf's dtype and shape, against `_expected`'s
    literals.  They were written by hand and then confirmed by running this module against the package as it stood at the
    commit before the off-policy learners got their common cores, where all seven cases passed."""
    sd = _learner(kind, P, mode).state_dict(include_replay=True)
    assert _tree(sd) == _expected(kind, P, mode)
    assert "replay" not in _learner(kind, P, mode).state_dict()


@pytest.mark.parametrize("mode", ("torch", "fused"))
def test_a_population_of_one_saves_what_droq_saves_but_stacked(mode):
    """A population of one member and a DroQ of the same seed and sizes hold the same values: the checkpoints differ in
    "members", "gamma" and "target_entropy", which only the population has, and in the leading dimension of 1 of the
    networks, the normaliser and the fused step's Adam state."""
    single = _learner("droq", 1, mode).state_dict(include_replay=True)
    pop = _learner("population", 1, mode).state_dict(include_replay=True)
    assert set(pop) - set(single) == {"members", "gamma", "target_entropy"} and not set(single) - set(pop)
    assert pop["members"] == 1 and pop["gamma"].tolist() == [pytest.approx(0.99)]
    assert pop["target_entropy"].tolist() == [-float(A)]
    stacked = {"actor", "critics", "targets", "normalizer", "critic_adam"}

    def same(p, s, lead):
        if isinstance(s, torch.Tensor):
            assert tuple(p.shape) == ((1,) if lead else ()) + tuple(s.shape) and p.dtype == s.dtype
            assert torch.equal(p[0] if lead else p, s)
        elif isinstance(s, dict):
            assert list(p) == list(s)
            for k in s:
                same(p[k], s[k], lead)
        elif isinstance(s, (list, tuple)):
            assert len(p) == len(s)
            for x, y in zip(p, s):
                same(x, y, lead)
        else:
            assert p == s and type(p) is type(s)

    for key in single:
        same(pop[key], single[key], key in stacked)
