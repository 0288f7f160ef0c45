"""ctypes binding of the population kernels' C ABI (include/learn/rp_pop.h, librp_pop.so) and `DroQPopulation`, P
independent DroQ learners (droq.DroQ) that share one environment batch: member p owns the envs e with e % P == p -- the
task's own song rule, so with `midi=[P songs]` member p is the specialist of song p, and with one song the members are
P seeds or a sweep over `gamma`, `init_alpha` and `target_entropy`.

The four entry points are module functions taking raw device addresses (`sample`, `act`, `target`, `moments`); each
enqueues one kernel on the caller's HIP stream and reads nothing back.  They are the single-learner kernels' device text
(rp_sac_sample, rp_sac_act, rp_droq_target, rp_learn_moments) run on a member's rows with that member's slices of the
stacked parameters.  The ring is SAC's [C][E]..., written by the learner's unchanged `pack`.  The gradient step is plain
torch on stacked parameters [P][out][in] (`torch.baddbmm`): a loss is the sum over the members of the per-member masked
means, so member p's gradient depends on member p's rows alone, and Adam, being element-wise, keeps the members
independent.  With `DroQPopulation(critic_step="fused")` the critic step is instead the two launches of
`pop_critic.step` (include/learn/rp_pop_critic.h) for all members.  With `DroQPopulation(evolve={...})` the members meet:
population-based training's exploit and explore steps are the three kernels of `evolve` (include/learn/rp_evolve.h) on
the stacked tensors.  Like the engine, the library has no CPU fallback: a
missing library is an error.
"""

from __future__ import annotations

import ctypes
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from robopianist_amd import _abi, droq, evolve as _evolve, pop_critic
from robopianist_amd.droq import Critic, DroQCore
from robopianist_amd.learning import STEP_FIRST, LearnError, Mlp, _train_and_evaluate, mlp_table
from robopianist_amd.offpolicy import ReplayLearner, squashed_gaussian

EXPORTED_SYMBOLS = ("rp_pop_act", "rp_pop_sample", "rp_pop_target", "rp_pop_moments", "rp_pop_dim", "rp_pop_last_error")

INTERLEAVED, BLOCKED = 0, 1          # row j of member p is array row p + P j / p rows + j
TILE_MAJOR, MEMBER_MAJOR = 0, 1      # the workgroup order of act and target (speed only)

_p, _i, _u32, _f, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_float, ctypes.c_double


class ActArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("obs", _p), ("mean", _p), ("inv_std", _p), ("obs_clip", _f),
                ("log_std_min", _f), ("log_std_max", _f), ("actor", ctypes.POINTER(Mlp)), ("action", _p), ("logp", _p),
                ("pre", _p), ("env_action", _p), ("precision", _i), ("deterministic", _i), ("seed_lo", _u32),
                ("seed_hi", _u32), ("round", _u32), ("D", _i), ("H1", _i), ("H2", _i), ("A", _i), ("P", _i), ("rows", _i),
                ("layout", _i), ("grid_order", _i), ("member_first", _i), ("member_count", _i), ("row_first", _i),
                ("row_count", _i), ("hip_stream", _p)]


class SampleArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("ring_obs", _p), ("ring_action", _p), ("ring_reward", _p),
                ("ring_discount", _p), ("ring_step_type", _p), ("obs", _p), ("next_obs", _p), ("action", _p),
                ("reward", _p), ("discount", _p), ("mask", _p), ("index", _p), ("n_written", ctypes.c_longlong),
                ("seed_lo", _u32), ("seed_hi", _u32), ("round", _u32), ("C", _i), ("E", _i), ("D", _i), ("A", _i),
                ("P", _i), ("n", _i), ("member_first", _i), ("member_count", _i), ("row_first", _i), ("row_count", _i),
                ("hip_stream", _p)]


class TargetArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("next_obs", _p), ("action", _p), ("logp", _p), ("reward", _p),
                ("discount", _p), ("mean", _p), ("inv_std", _p), ("obs_clip", _f), ("gamma", _p), ("log_alpha", _p),
                ("critics", ctypes.POINTER(Critic)), ("n_critics", _i), ("y", _p), ("q_min", _p), ("q", _p),
                ("drop_threshold", _u32), ("keep_scale", _f), ("ln_eps", _f), ("seed_lo", _u32), ("seed_hi", _u32),
                ("round", _u32), ("D", _i), ("H1", _i), ("H2", _i), ("A", _i), ("P", _i), ("n", _i), ("grid_order", _i),
                ("member_first", _i), ("member_count", _i), ("row_first", _i), ("row_count", _i), ("hip_stream", _p)]


class MomentsArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("obs", _p), ("mean", _p), ("M2", _p), ("mean_f32", _p),
                ("inv_std_f32", _p), ("count", _d), ("eps", _d), ("k", _i), ("E", _i), ("D", _i), ("P", _i),
                ("member_first", _i), ("member_count", _i), ("hip_stream", _p)]


_ARGS = {"act": ActArgs, "sample": SampleArgs, "target": TargetArgs, "moments": MomentsArgs}


_entries = _abi.EntryTable("rp_pop_", _ARGS, LearnError, "RP_POP_LIB", "librp_pop.so", "population")
LIB_PATH = _entries.path
load_library, declare, make_args, call_raw, last_error, dim, _call = (
    _entries.load, _entries.declare, _entries.make_args, _entries.call_raw, _entries.last_error, _entries.dim, _entries.call)


def _order(grid_order):
    return dim("default_grid_order") if grid_order is None else int(grid_order)


def _ranges(P, rows, member_first, member_count, row_first, row_count):
    return dict(member_first=member_first, member_count=P - member_first if member_count is None else member_count,
                row_first=row_first, row_count=rows - row_first if row_count is None else row_count)


def act(obs, mean, inv_std, obs_clip, actor, D, H1, H2, A, P, rows, layout, log_std_bounds=(-5.0, 2.0), action=None,
        logp=None, pre=None, env_action=None, precision=64, deterministic=False, seed=0, round_=0, member_first=0,
        member_count=None, row_first=0, row_count=None, grid_order=None, hip_stream=None):
    """`actor`: an `Mlp` of the bases of the stacked tensors; `rows`: per member; `layout`: INTERLEAVED / BLOCKED."""
    _call("act", obs=obs, mean=mean, inv_std=inv_std, obs_clip=float(obs_clip), log_std_min=float(log_std_bounds[0]),
          log_std_max=float(log_std_bounds[1]), actor=ctypes.pointer(actor) if actor is not None else None,
          action=action, logp=logp, pre=pre, env_action=env_action, precision=precision,
          deterministic=int(bool(deterministic)), D=D, H1=H1, H2=H2, A=A, P=P, rows=rows, layout=int(layout),
          grid_order=_order(grid_order), hip_stream=hip_stream, **_abi.seed_args(seed, round_),
          **_ranges(P, rows, member_first, member_count, row_first, row_count))


def sample(ring_obs, ring_action, ring_reward, ring_discount, ring_step_type, obs, next_obs, action, reward, discount,
           mask, n_written, C, E, D, A, P, n, index=None, seed=0, round_=0, member_first=0, member_count=None,
           row_first=0, row_count=None, hip_stream=None):
    """`n`: minibatch rows per member; the outputs hold P n rows, member p's at [p n, (p + 1) n)."""
    _call("sample", ring_obs=ring_obs, ring_action=ring_action, ring_reward=ring_reward, ring_discount=ring_discount,
          ring_step_type=ring_step_type, obs=obs, next_obs=next_obs, action=action, reward=reward, discount=discount,
          mask=mask, index=index, n_written=int(n_written), C=C, E=E, D=D, A=A, P=P, n=n, hip_stream=hip_stream,
          **_abi.seed_args(seed, round_), **_ranges(P, n, member_first, member_count, row_first, row_count))


def target(next_obs, action, logp, reward, discount, mean, inv_std, obs_clip, gamma, log_alpha, critics, y, D, H1, H2, A,
           P, n, q_min=None, q=None, threshold=0, keep_scale=1.0, ln_eps=1e-5, seed=0, round_=0, member_first=0,
           member_count=None, row_first=0, row_count=None, grid_order=None, hip_stream=None):
    """`critics`: a sequence of `Critic` of the bases of the stacked target networks; `gamma`, `log_alpha`: device
    addresses of [P] float32."""
    tab = droq.critic_table(critics)
    _call("target", next_obs=next_obs, action=action, logp=logp, reward=reward, discount=discount, mean=mean,
          inv_std=inv_std, obs_clip=float(obs_clip), gamma=gamma, log_alpha=log_alpha, critics=tab, n_critics=len(tab),
          y=y, q_min=q_min, q=q, drop_threshold=int(threshold), keep_scale=float(keep_scale), ln_eps=float(ln_eps),
          D=D, H1=H1, H2=H2, A=A, P=P, n=n, grid_order=_order(grid_order), hip_stream=hip_stream,
          **_abi.seed_args(seed, round_), **_ranges(P, n, member_first, member_count, row_first, row_count))


def moments(obs, mean, M2, mean_f32, inv_std_f32, count, eps, k, E, D, P, member_first=0, member_count=None,
            hip_stream=None):
    """`obs`: the first of k consecutive ring slots [k][E][D]; the four outputs are [P][D]."""
    _call("moments", obs=obs, mean=mean, M2=M2, mean_f32=mean_f32, inv_std_f32=inv_std_f32, count=float(count),
          eps=float(eps), k=int(k), E=E, D=D, P=P, member_first=member_first,
          member_count=P - member_first if member_count is None else member_count, hip_stream=hip_stream)


# ---- the batched modules -------------------------------------------------------------------------------------------------
class BatchedLinear(nn.Module):
    """P `nn.Linear`s as one: weight [P][out][in], bias [P][out]; [P, n, in] -> [P, n, out]."""

    def __init__(self, linears):
        super().__init__()
        self.weight = nn.Parameter(torch.stack([m.weight.detach() for m in linears]).contiguous())
        self.bias = nn.Parameter(torch.stack([m.bias.detach() for m in linears]).contiguous())

    def forward(self, x):
        return torch.baddbmm(self.bias.unsqueeze(1), x, self.weight.transpose(1, 2))


class BatchedLayerNorm(nn.Module):
    """P `nn.LayerNorm`s over the last dimension as one: weight, bias [P][H]."""

    def __init__(self, norms):
        super().__init__()
        self.eps = float(norms[0].eps)
        self.weight = nn.Parameter(torch.stack([m.weight.detach() for m in norms]).contiguous())
        self.bias = nn.Parameter(torch.stack([m.bias.detach() for m in norms]).contiguous())

    def forward(self, x):
        h = F.layer_norm(x, (x.shape[-1],), None, None, self.eps)
        return h * self.weight.unsqueeze(1) + self.bias.unsqueeze(1)


def stack_networks(nets):
    """P `nn.Sequential`s of the same architecture (Linear, LayerNorm, Dropout, Tanh, ReLU) as one batched
    `nn.Sequential` with the same indices, on [P, n, .]."""
    BL, BLN = BatchedLinear, BatchedLayerNorm
    layers = []
    for group in zip(*nets):
        m = group[0]
        if isinstance(m, nn.Linear):
            layers.append(BL(group))
        elif isinstance(m, nn.LayerNorm):
            layers.append(BLN(group))
        elif isinstance(m, nn.Dropout):
            layers.append(nn.Dropout(m.p))
        else:
            layers.append(type(m)())
    return nn.Sequential(*layers)


def member_network(net, p):
    """Member p of a batched network as a plain `nn.Sequential` (a copy)."""
    BL, BLN = BatchedLinear, BatchedLayerNorm
    layers = []
    for m in net:
        if isinstance(m, BL):
            lin = nn.Linear(m.weight.shape[2], m.weight.shape[1]).to(m.weight.device, m.weight.dtype)
            with torch.no_grad():
                lin.weight.copy_(m.weight[p]); lin.bias.copy_(m.bias[p])
            layers.append(lin)
        elif isinstance(m, BLN):
            ln = nn.LayerNorm(m.weight.shape[1], m.eps).to(m.weight.device, m.weight.dtype)
            with torch.no_grad():
                ln.weight.copy_(m.weight[p]); ln.bias.copy_(m.bias[p])
            layers.append(ln)
        elif isinstance(m, nn.Dropout):
            layers.append(nn.Dropout(m.p))
        else:
            layers.append(type(m)())
    return nn.Sequential(*layers)


# ---- the losses: offpolicy's, per member, summed over the members ----------------------------------------------------------
def member_means(x, mask):
    """offpolicy._masked_mean of every member: x, mask [P, n] -> [P]."""
    return (x * mask).sum(1) / mask.sum(1).clamp(min=1.0)


def critic_losses(qs, y, mask):
    """offpolicy.critic_loss of every member on its own rows: [P].  `qs`: a list of [P, n]."""
    return sum(member_means(0.5 * (q - y) ** 2, mask) for q in qs)


def actor_losses(log_alpha, logp_new, q_new, mask):
    """offpolicy.actor_loss of every member: [P]; `log_alpha` [P]."""
    return member_means(log_alpha.detach().exp().unsqueeze(1) * logp_new - q_new, mask)


def alpha_losses(log_alpha, logp_new, target_entropy, mask):
    """offpolicy.alpha_loss of every member: [P]; `log_alpha`, `target_entropy` [P]."""
    return member_means(-log_alpha.unsqueeze(1) * (logp_new.detach() + target_entropy.unsqueeze(1)), mask)


def critic_loss(qs, y, mask):
    """What the critics' optimizer minimises: the sum over the members, so that member p's gradient is its own loss's."""
    return critic_losses(qs, y, mask).sum()


def actor_loss(log_alpha, logp_new, q_new, mask):
    return actor_losses(log_alpha, logp_new, q_new, mask).sum()


def alpha_loss(log_alpha, logp_new, target_entropy, mask):
    return alpha_losses(log_alpha, logp_new, target_entropy, mask).sum()


def _per_member(value, P, name):
    """A scalar or a length-P sequence as a list of P floats."""
    if np.ndim(value) == 0:
        return [float(value)] * P
    out = [float(v) for v in value]
    if len(out) != P:
        raise ValueError(f"{name} must be a scalar or a sequence of {P} values (one per member), got {len(out)}")
    return out


EVOLVE_DEFAULTS = {"every": 10, "percent": 25, "min_episodes": 1, "min_gap": 0.0, "factors": (0.8, 1.25),
                   "gamma_bounds": (0.0, 0.9999), "entropy_bounds": (-math.inf, math.inf),
                   "explore": ("gamma", "target_entropy")}


def _evolve_options(evolve):
    """`DroQPopulation`'s evolve option with its defaults filled in and its values checked; None stays None."""
    if evolve is None:
        return None
    if not isinstance(evolve, dict):
        raise ValueError(f"evolve must be None or a dict of options, got {evolve!r}")
    unknown = sorted(set(evolve) - set(EVOLVE_DEFAULTS))
    if unknown:
        raise ValueError(f"evolve has no option {unknown[0]!r}: its options are {', '.join(EVOLVE_DEFAULTS)}")
    o = dict(EVOLVE_DEFAULTS, **evolve)
    for k in ("every", "percent", "min_episodes"):
        if isinstance(o[k], bool) or int(o[k]) != o[k]:
            raise ValueError(f"evolve's {k} must be an integer, got {o[k]!r}")
        o[k] = int(o[k])
    if o["every"] < 1:
        raise ValueError(f"evolve's every must be >= 1, got {o['every']}")
    if not 0 <= o["percent"] <= 100:
        raise ValueError(f"evolve's percent must lie in [0, 100], got {o['percent']}")
    if o["min_episodes"] < 1:
        raise ValueError(f"evolve's min_episodes must be >= 1, got {o['min_episodes']}")
    o["min_gap"] = float(o["min_gap"])
    if not o["min_gap"] >= 0.0:
        raise ValueError(f"evolve's min_gap must be >= 0, got {o['min_gap']}")
    for k in ("factors", "gamma_bounds", "entropy_bounds"):
        if np.ndim(o[k]) != 1 or len(o[k]) != 2:
            raise ValueError(f"evolve's {k} must be a pair, got {o[k]!r}")
        o[k] = (float(o[k][0]), float(o[k][1]))
    if not (o["factors"][0] > 0.0 and o["factors"][1] > 0.0):
        raise ValueError(f"evolve's factors must be (down, up), both > 0, got {o['factors']}")
    for k in ("gamma_bounds", "entropy_bounds"):
        if not o[k][0] <= o[k][1]:
            raise ValueError(f"evolve's {k} must be (min, max) with min <= max, got {o[k]}")
    explore = (o["explore"],) if isinstance(o["explore"], str) else tuple(o["explore"])
    for name in explore:
        if name not in EVOLVE_DEFAULTS["explore"]:
            raise ValueError(f'evolve explores "gamma" and "target_entropy", got {name!r}')
    o["explore"] = tuple(k for k in EVOLVE_DEFAULTS["explore"] if k in explore)
    return o


class DroQPopulation(DroQCore, ReplayLearner):
    """`members` = P independent `droq.DroQ` learners over one env batch of E = P Em envs: member p collects with, and
    learns from, the envs p, p + P, p + 2 P, ... alone, and has its own actor, critics, targets, temperature, observation
    normaliser and minibatches of `batch_size` rows (per member).  `gamma`, `init_alpha` and `target_entropy` take a
    scalar or a sequence of P values; everything else is shared.  With `members=1` this is DroQ.

    `collect(n)` launches, per control step, one `rp_pop_act` over all envs (each env by its member's actor), the env's
    step and `pack`, then one `rp_pop_moments` per contiguous run of new slots; nothing is read back.  `update(g)` is
    DroQ's schedule with one `rp_pop_sample`, one `rp_pop_act` and, per range, one `rp_pop_target` for all members.

    `critic_step`: "torch" (the default: autograd on the stacked tensors with torch's own dropout, torch's Adam,
    `_foreach_lerp_`) or "fused" (`pop_critic.step`: the step of all members in two launches, with Philox dropout masks
    keyed by (seed, round, row); the population then owns Adam's stacked m and v and one step count for all members,
    and torch's critic optimiser stays unused) -- `droq.DroQ`'s contract.  `actor_step`: "torch" only; `droq.DroQ`'s "fused"
    (`actor.step`) is refused here: the population's actor step stays the stacked torch one.

    `evolve`: None (the default: the members never meet) or a dict of population-based training's options (Jaderberg et
    al. 2017; include/learn/rp_evolve.h), every key optional: `every` (10: the rounds of `train()` between two events),
    `percent` (25: the share of the eligible members at either end), `min_episodes` (1: the ended episodes a member's
    window needs to be ranked), `min_gap` (0: what a winner's mean return must exceed a loser's by), `factors`
    ((0.8, 1.25): the two perturbations (down, up)), `gamma_bounds` ((0, 0.9999)), `entropy_bounds` ((-inf, inf)) and
    `explore` (("gamma", "target_entropy"): the hyper-parameters a copy perturbs).  `episode_stats()` then folds the
    ended episodes' returns into every member's window before it clears them, and `evolve()` -- called by `train()` after
    every `every`-th round -- overwrites the losers' slices of every stacked tensor with a winner's and perturbs the
    copied `gamma` and `target_entropy`, all on the device: `rp_evolve_plan`, then `rp_evolve_copy`."""

    _reads, _me = "the population kernels read", "population"

    def __init__(self, env, members: int, hidden=(256, 256), n_critics: int = 2, capacity: int = 64,
                 batch_size: int = 256, gamma=0.99, tau: float = 0.005, lr: float = 3e-4, init_alpha=1.0,
                 target_entropy=None, log_std_bounds=(-5.0, 2.0), learning_starts: int = 0, obs_clip: float = 10.0,
                 seed: int = 0, norm_eps: float = 1e-8, dropout: float = 0.01, utd: int = 20, ln_eps: float = 1e-5,
                 critic_step: str = "torch", actor_step: str = "torch", evolve=None):
        super().__init__(env)
        self.evolve_options = _evolve_options(evolve)
        if actor_step == "fused":
            raise ValueError('DroQPopulation has no fused actor step yet: actor_step="fused" is droq.DroQ\'s; a population '
                             'takes actor_step="torch"')
        self._init_droq(dropout, utd, ln_eps, critic_step, actor_step)
        self.P = P = int(members)
        if P < 1:
            raise ValueError(f"members must be >= 1, got {members}")
        if self.E % P:
            raise ValueError(f"members = {P} does not divide n_envs = {self.E}: member p owns the envs e % members == p")
        self.Em = self.E // P
        if P * self.utd * int(batch_size) > 2 ** 31 - 1:
            raise ValueError("members x utd x batch_size must stay below 2^31")
        alpha0 = _per_member(init_alpha, P, "init_alpha")
        self._init_replay(self.Em, "n_envs / members", hidden, n_critics, capacity, batch_size, tau, lr,
                          [math.log(a) for a in alpha0], log_std_bounds, learning_starts, obs_clip, seed, norm_eps)
        D, z = self.D, self._zeros
        f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=self._dev)
        self.gamma = f32(_per_member(gamma, P, "gamma"))
        entropy = -float(self.A) if target_entropy is None else target_entropy
        self.target_entropy = f32(_per_member(entropy, P, "target_entropy"))
        # the normaliser, per member (DeviceLearner allocated one row)
        self._mean, self._M2 = z(P, D, dtype=torch.float64), z(P, D, dtype=torch.float64)
        self._mean_f32, self._inv_std_f32 = z(P, D), torch.ones(P, D, dtype=torch.float32, device=self._dev)
        # the minibatches: member p's utd ranges of B rows at [p n, (p + 1) n), n = utd B
        self._init_ranges(P * self.utd * self.B)
        self._range = self.utd - 1
        if self.evolve_options is not None:
            if P > _evolve.MAX_MEMBERS:
                raise ValueError(f"evolve ranks at most {_evolve.MAX_MEMBERS} members, got members = {P}")
            # the members' fitness windows, the last event's decision, the events so far and the rounds train() has run
            self._fit_sum, self._fit_count = z(P, dtype=torch.float64), z(P, dtype=torch.int64)
            self._source = torch.arange(P, dtype=torch.int32, device=self._dev)
            self.generation, self._evolve_rounds = 0, 0

    def _draw(self):
        """(actor, critics) member after member, as P single learners of this seed's stream would draw them, stacked."""
        drawn = [self._draw_member() for _ in range(self.P)]
        return (stack_networks([a for a, _ in drawn]),
                [stack_networks([cs[i] for _, cs in drawn]) for i in range(self.n_critics)])

    def _workspace_bytes(self):
        return pop_critic.workspace_bytes(self.n_critics, self.H1, self.H2, self.B, self.P)

    # -- accessors ---------------------------------------------------------------------------------------------------
    @property
    def members(self):
        return self.P

    @property
    def alpha(self):
        """[P] floats."""
        return self.log_alpha.detach().exp().cpu().numpy().astype(np.float64)

    def rows(self):
        """The utd x batch_size rows per member that the last actor step drew, [P, utd B, ...] views (live)."""
        v = lambda t: t.view(self.P, self.utd * self.B, *t.shape[1:])
        return {"obs": v(self._u_obs), "next_obs": v(self._u_next), "action": v(self._u_action),
                "reward": v(self._u_reward), "discount": v(self._u_discount), "mask": v(self._u_mask),
                "next_action": v(self._u_next_action), "next_logp": v(self._u_next_logp), "y": v(self._u_y)}

    def minibatch(self):
        """The range of `rows()` the last launches worked on: [P, B, ...] views (live)."""
        r = slice(self._range * self.B, (self._range + 1) * self.B)
        return {k: v[:, r] for k, v in self.rows().items()}

    def _actor_table(self):
        """The stacked actor as rp_learn_mlp: the bases of its tensors as they are now."""
        tensors = [t for i in (0, 2, 4) for t in (self.actor[i].weight, self.actor[i].bias)]
        for t in tensors:
            if not t.is_contiguous() or t.dtype != torch.float32:
                raise LearnError(f"{self._reads} contiguous float32 parameters")
        return mlp_table(tensors)

    def _act(self, obs, rows, layout, st, **out):
        act(obs.data_ptr(), self._mean_f32.data_ptr(), self._inv_std_f32.data_ptr(), self.obs_clip, self._actor_table(),
            self.D, self.H1, self.H2, self.A, self.P, rows, layout, log_std_bounds=self.log_std_bounds, seed=self.seed,
            round_=self._round, hip_stream=st, **out)

    def _act_envs(self, obs, st, **out):
        self._act(obs, self.Em, INTERLEAVED, st, **out)

    def _merge_run(self, obs, k, st):
        """k consecutive slots into the running moments of every member (one launch)."""
        moments(obs.data_ptr(), self._mean.data_ptr(), self._M2.data_ptr(), self._mean_f32.data_ptr(),
                self._inv_std_f32.data_ptr(), self._count, self.norm_eps, k, self.E, self.D, self.P, hip_stream=st)
        self._count += float(k * self.Em)

    def normalize(self, obs):
        """What the kernels feed the first layer (torch): obs [P, n, D] by the member's moments."""
        return torch.clamp((obs - self._mean_f32.unsqueeze(1)) * self._inv_std_f32.unsqueeze(1), -self.obs_clip,
                           self.obs_clip)

    # -- the gradient steps ----------------------------------------------------------------------------------------------
    def draw_and_act(self):
        """The two launches of an actor step that cover all members and all utd ranges: the utd x B rows of every
        member, and every member's policy at their next observations."""
        n = self.utd * self.B
        with torch.cuda.device(self._dev):
            st = self._stream()
            sample(self._obs.data_ptr(), self._action.data_ptr(), self._reward.data_ptr(), self._discount.data_ptr(),
                   self._step_type.data_ptr(), self._u_obs.data_ptr(), self._u_next.data_ptr(), self._u_action.data_ptr(),
                   self._u_reward.data_ptr(), self._u_discount.data_ptr(), self._u_mask.data_ptr(), self.n_written,
                   self.C, self.E, self.D, self.A, self.P, n, seed=self.seed, round_=self._round, hip_stream=st)
            self._act(self._u_next, n, BLOCKED, st, action=self._u_next_action.data_ptr(),
                      logp=self._u_next_logp.data_ptr())

    def target_range(self, u):
        """The TD target of range u of every member from the target critics as they are now (one launch); returns
        `minibatch()` on it."""
        with torch.cuda.device(self._dev):
            target(self._u_next.data_ptr(), self._u_next_action.data_ptr(), self._u_next_logp.data_ptr(),
                   self._u_reward.data_ptr(), self._u_discount.data_ptr(), self._mean_f32.data_ptr(),
                   self._inv_std_f32.data_ptr(), self.obs_clip, self.gamma.data_ptr(), self.log_alpha.data_ptr(),
                   [self._critic_table(t) for t in self.targets], self._u_y.data_ptr(), self.D, self.H1, self.H2, self.A,
                   self.P, self.utd * self.B, threshold=self._threshold, keep_scale=self._keep_scale, ln_eps=self.ln_eps,
                   seed=self.seed, round_=self._round, row_first=u * self.B, row_count=self.B, hip_stream=self._stream())
        self._range = u
        return self.minibatch()

    def _fused_range(self, batch):
        """The range u whose views `batch` holds (what `target_range(u)` and `minibatch()` return)."""
        D, B, n = self.D, self.B, self.utd * self.B
        obs = batch["obs"]
        off = obs.data_ptr() - self._u_obs.data_ptr()
        u = off // (4 * D * B)
        if off < 0 or off % (4 * D * B) or u >= self.utd or tuple(obs.shape) != (self.P, B, D) or \
                (self.P > 1 and obs.stride(0) != n * D) or \
                any(batch[k].data_ptr() != getattr(self, "_u_" + k)[u * B:].data_ptr() or batch[k].shape[:2] != obs.shape[:2] or
                    (self.P > 1 and batch[k].stride(0) != getattr(self, "_u_" + k)[0].numel() * n)
                    for k in ("action", "y", "mask")):
            raise LearnError('critic_step="fused" steps on a range of the population\'s own minibatches: pass what '
                             "target_range(u) or minibatch() returned")
        return u

    def _launch_critic_step(self, *block, **options):
        pop_critic.step(*block, self.P, self.utd * self.B, **options)

    def _range_loss(self, u):
        """The per-member losses of range u from the fused step's q."""
        v = lambda t: t.view(self.P, self.utd * self.B)[:, u * self.B:(u + 1) * self.B]
        return critic_losses([v(q) for q in self._u_q], v(self._u_y), v(self._u_mask))

    def critic_step(self, batch, loss: bool = True):
        """The critics' Adam step on `batch` ([P, n, ...]; torch's own dropout) and the targets' Polyak step over the
        stacked tensors.  Returns the per-member losses [P] (a tensor).  With critic_step="fused": the two launches of
        `pop_critic.step` on the range `batch` views, and the losses only if `loss`."""
        if self.critic_mode == "fused":
            return self._fused_critic_step(self._fused_range(batch), loss)
        xa = torch.cat([self.normalize(batch["obs"]), batch["action"]], dim=2)
        per = critic_losses([c(xa).squeeze(-1) for c in self.critics], batch["y"], batch["mask"])
        self.critic_optimizer.zero_grad(set_to_none=True)
        per.sum().backward()
        self.critic_optimizer.step()
        with torch.no_grad():
            torch._foreach_lerp_([p for t in self.targets for p in t.parameters()],
                                 [p for c in self.critics for p in c.parameters()], self.tau)
        return per.detach()

    def actor_step(self, batch):
        """The actors' and the temperatures' Adam steps on `batch`; the critics stay in train() mode, as in the paper.
        Returns per-member statistics, [P] tensors."""
        mask = batch["mask"]
        xn = self.normalize(batch["obs"])
        eps = torch.randn(xn.shape[0], xn.shape[1], self.A, generator=self._gen, device=xn.device, dtype=xn.dtype)
        a_new, logp_new, _ = squashed_gaussian(self.actor(xn), eps, self.log_std_bounds)
        xa_new = torch.cat([xn, a_new], dim=2)
        q_new = torch.stack([c(xa_new).squeeze(-1) for c in self.critics]).min(0).values
        la = actor_losses(self.log_alpha, logp_new, q_new, mask)
        self.actor_optimizer.zero_grad(set_to_none=True)
        la.sum().backward()   # (the critics' gradients of this pass are dropped by their next zero_grad)
        self.actor_optimizer.step()
        lt = alpha_losses(self.log_alpha, logp_new, self.target_entropy, mask)
        self.alpha_optimizer.zero_grad(set_to_none=True)
        lt.sum().backward()
        self.alpha_optimizer.step()
        return {"actor_loss": la.detach(), "alpha_loss": lt.detach(), "alpha": self.log_alpha.detach().exp(),
                "entropy": -member_means(logp_new.detach(), mask), "masked": 1.0 - mask.mean(1)}

    def _host_stats(self, stats):
        """float64 arrays [P] (one read-back)."""
        if not stats:
            return {}
        return dict(zip(stats, torch.stack([v.to(torch.float64) for v in stats.values()]).cpu().numpy()))

    def episode_stats(self):
        """{"episodes" [P] int, "mean_return" [P], "mean_length" [P]} of the episodes that ended since the last call, per
        member (one read-back); the counters start again from zero."""
        if self.evolve_options is not None:   # (the windows see the counters before they are cleared)
            with torch.cuda.device(self._dev):
                _evolve.fold(self._done_return.data_ptr(), self._done_count.data_ptr(), self._fit_sum.data_ptr(),
                             self._fit_count.data_ptr(), self.E, self.P, hip_stream=self._stream())
        by_member = lambda t: t.view(self.Em, self.P).sum(0).to(torch.float64)
        host = torch.stack([by_member(self._done_count), by_member(self._done_return), by_member(self._done_len)]).cpu().numpy()
        n = host[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            out = {"episodes": n.astype(np.int64), "mean_return": np.where(n > 0, host[1] / n, np.nan),
                   "mean_length": np.where(n > 0, host[2] / n, np.nan)}
        self._done_return.zero_(); self._done_len.zero_(); self._done_count.zero_()
        return out

    def _mean_reward(self, slots):
        """[P]: of every member's new TimeSteps that are not FIRST (one read-back)."""
        live = (self._step_type[slots] != STEP_FIRST).to(torch.float64).view(-1, self.Em, self.P)
        reward = self._reward[slots].to(torch.float64).view(-1, self.Em, self.P)
        sums = torch.stack([(reward * live).sum((0, 1)), live.sum((0, 1))]).cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(sums[1] > 0, sums[0] / sums[1], np.nan)

    # -- population-based training ---------------------------------------------------------------------------------------
    def _member_fields(self):
        """[(name, tensor)]: every tensor [P][...] a member owns a slice of, as they are now -- the actor's 6, every
        critic's and every target's 10, log_alpha, the normaliser's four, the fused critic step's m and v, and the
        moments of torch's three Adams where they exist.  `gamma` and `target_entropy` are the plan's to write; the step
        counts, the normaliser's count, the ring and the generator are shared and stay out."""
        fields = [(f"actor.{i}", t) for i, t in enumerate(self._actor_tensors())]
        for group, nets in (("critics", self.critics), ("targets", self.targets)):
            fields += [(f"{group}.{c}.{i}", t) for c, net in enumerate(nets) for i, t in enumerate(self._critic_tensors(net))]
        fields.append(("log_alpha", self.log_alpha))
        fields += [(k, getattr(self, k)) for k in ("_mean", "_M2", "_mean_f32", "_inv_std_f32")]
        if self.critic_mode == "fused":
            for k, group in (("_c_m", self._c_m), ("_c_v", self._c_v)):
                fields += [(f"{k}.{c}.{i}", t) for c, net in enumerate(group) for i, t in enumerate(net)]
        for name in ("actor", "critic", "alpha"):
            opt = getattr(self, name + "_optimizer")
            for i, param in enumerate(opt.param_groups[0]["params"]):
                fields += [(f"{name}_optimizer.{i}.{k}", opt.state[param][k]) for k in ("exp_avg", "exp_avg_sq")
                           if param in opt.state and k in opt.state[param]]
        for name, t in fields:
            if not t.is_contiguous() or t.shape[0] != self.P or t.element_size() % 4:
                raise LearnError(f"evolve copies contiguous stacked tensors [members][...] of 4- or 8-byte elements: {name}")
        return fields

    def _field_table(self):
        """`_member_fields()` as rp_evolve_field rows: (base address, 4-byte words per member)."""
        return [(t.data_ptr(), t[0].numel() * t.element_size() // 4) for _, t in self._member_fields()]

    def evolve(self):
        """One event of population-based training on the learner's stream, nothing read back: `rp_evolve_plan` on the
        members' fitness windows (which it clears), then `rp_evolve_copy` over `_member_fields()`; `generation`, the
        Philox round word of the plan, then counts one more.  Returns the launches enqueued."""
        o = self.evolve_options
        if o is None:
            raise LearnError("evolve() needs the population's evolve option: DroQPopulation(..., evolve={...})")
        ptr = lambda name, t: t.data_ptr() if name in o["explore"] else None
        with torch.cuda.device(self._dev):
            st = self._stream()
            _evolve.plan(self._fit_sum.data_ptr(), self._fit_count.data_ptr(), self._source.data_ptr(), self.P,
                         percent=o["percent"], min_episodes=o["min_episodes"], min_gap=o["min_gap"], factors=o["factors"],
                         gamma=ptr("gamma", self.gamma), gamma_bounds=o["gamma_bounds"],
                         target_entropy=ptr("target_entropy", self.target_entropy), entropy_bounds=o["entropy_bounds"],
                         seed=self.seed, generation=self.generation, hip_stream=st)
            launches = 1 + _evolve.copy(self._field_table(), self._source.data_ptr(), self.P, hip_stream=st)
        self.generation += 1
        return launches

    def last_evolution(self):
        """`source` [P] of the last event as a numpy array (the one read-back): member p took member source[p]'s slices;
        source[p] == p: it kept its own."""
        if self.evolve_options is None:
            raise LearnError("last_evolution() needs the population's evolve option")
        return self._source.cpu().numpy()

    def train(self, n: int, steps_per_round: int = 1, grad_steps: int = 1, callback=None):
        """The replay learner's rounds; with the evolve option, `evolve()` after every `every`-th round this population
        has trained (counted over all calls)."""
        if self.evolve_options is None:
            return super().train(n, steps_per_round, grad_steps, callback)
        log = []
        for i in range(int(n)):
            log += ReplayLearner.train(self, 1, steps_per_round, grad_steps)
            self._evolve_rounds += 1
            if self._evolve_rounds % self.evolve_options["every"] == 0:
                self.evolve()
            if callback is not None:   # (after the round's event, so that it sees it)
                callback(i, log[-1])
        return log

    # -- evaluation ----------------------------------------------------------------------------------------------------
    def actor_of(self, p: int):
        """Member p's actor as a plain `nn.Sequential` (a copy): what `droq.DroQ.actor` or `offpolicy.SAC.actor` of a
        single-learner env batch loads with `load_state_dict(actor_of(p).state_dict())`."""
        if not 0 <= int(p) < self.P:
            raise ValueError(f"member {p} of {self.P}")
        return member_network(self.actor, int(p))

    def normalizer_of(self, p: int):
        """(count, mean [D] f64, M2 [D] f64, mean_f32 [D], inv_std_f32 [D]) of member p -- live views."""
        return self._count, self._mean[p], self._M2[p], self._mean_f32[p], self._inv_std_f32[p]

    # -- checkpoint / resume -------------------------------------------------------------------------------------------
    def state_dict(self, include_replay: bool = False):
        """The replay learner's contract on the stacked tensors and DroQ's blocks, plus "members", "gamma" and
        "target_entropy"; with the evolve option also "evolve": the options, `generation`, the rounds trained, the
        fitness windows and the last event's `source`."""
        sd = super().state_dict(include_replay)
        sd.update(members=self.P, gamma=self.gamma.detach().clone(), target_entropy=self.target_entropy.detach().clone())
        if self.evolve_options is not None:
            sd["evolve"] = {"options": dict(self.evolve_options), "generation": self.generation,
                            "rounds": self._evolve_rounds, "fit_sum": self._fit_sum.detach().clone(),
                            "fit_count": self._fit_count.detach().clone(), "source": self._source.detach().clone()}
        return sd

    def load_state_dict(self, sd):
        """A checkpoint written with another `members`, dropout, utd, ln_eps, critic_step or evolve is refused."""
        if sd.get("members") != self.P:
            raise ValueError(f"the checkpoint was written with members = {sd.get('members', 'nothing')}, this population "
                             f"has members = {self.P}")
        got = sd["evolve"]["options"] if "evolve" in sd else None
        if got != self.evolve_options:
            raise ValueError(f"the checkpoint was written with evolve = {got}, this population has evolve = "
                             f"{self.evolve_options}")
        super().load_state_dict(sd)
        self.gamma.copy_(sd["gamma"])
        self.target_entropy.copy_(sd["target_entropy"])
        if got is not None:
            mine = sd["evolve"]
            self.generation, self._evolve_rounds = int(mine["generation"]), int(mine["rounds"])
            self._fit_sum.copy_(mine["fit_sum"])
            self._fit_count.copy_(mine["fit_count"])
            self._source.copy_(mine["source"])


def _row(values, fmt="{:9.4f}"):
    return " ".join(fmt.format(float(v)) for v in values)


def train_and_evaluate(env, rounds: int, members: int, steps_per_round: int = 16, grad_steps: int = 1,
                       time_limit: float = None, log=print, **kwargs):
    """What the examples' --train-population does: `rounds` rounds of a `DroQPopulation` of `members` on `env` (a
    batched Environment), one line per round with every member's mean return of the episodes that ended in it and the
    smallest and largest temperature, then one deterministic episode of every env through a MidiEvaluationWrapper and
    every member's precision, recall and F1 (the mean over its envs).  Stops early after `time_limit` seconds.  Returns
    (population, log of the rounds, metrics: name -> [P] array)."""
    pop = DroQPopulation(env, members, **kwargs)
    P = pop.P
    last_mean = np.full(P, np.nan)
    evolved = {"generation": 0, "replaced": 0}

    def replaced():
        """The members replaced so far: one read-back per event (`last_evolution`), none in between."""
        if pop.generation != evolved["generation"]:
            source = pop.last_evolution()
            evolved["replaced"] += int((source != np.arange(P)).sum())
            evolved["generation"] = pop.generation
            changed = np.flatnonzero(source != np.arange(P))
            if len(changed):
                log(f"\tgeneration {pop.generation}: " + ", ".join(f"member {p} <- {source[p]}" for p in changed))
        return evolved["replaced"]

    def line(i, s, seconds):
        ended = s["episodes"] > 0
        last_mean[ended] = s["mean_return"][ended]
        # (a member none of whose episodes ended in the round shows the mean of the last round in which some did)
        alpha = s.get("alpha", np.full(P, np.nan))
        swaps = f"  replaced {replaced():4d}" if pop.evolve_options is not None else ""
        return (f"update {i + 1:4d}  episodes {int(s['episodes'].sum()):6d}  mean return per member {_row(last_mean)}  "
                f"alpha {float(np.min(alpha)):8.5f} .. {float(np.max(alpha)):8.5f}{swaps}  {seconds:7.1f} s")

    def metrics(evaluated, log):
        per_env = evaluated.get_musical_metrics_per_env()
        found = {k: torch.nanmean(v.view(pop.Em, P), dim=0).cpu().numpy() for k, v in per_env.items()}
        for k, v in found.items():
            log(f"\t{k} per member: {_row(v, '{:.4f}')}")
        return found

    train_one = lambda cb: pop.train(1, steps_per_round, grad_steps, callback=cb)
    rounds_log, found = _train_and_evaluate(pop, rounds, train_one, None, time_limit, log, line=line, metrics=metrics)
    return pop, rounds_log, found
