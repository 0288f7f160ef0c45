"""ctypes binding of the DroQ target kernel's C ABI (include/learn/rp_droq.h, librp_droq.so) and `DroQ`, dropout
Q-functions (Hiroe et al. 2022) on top of `offpolicy.SAC`: the replay ring, the sampler and the policy are SAC's,
unchanged; the critics are Linear -> Dropout -> LayerNorm -> ReLU twice and `utd` critic steps are taken per actor step.

The entry point is a module function taking raw device addresses (`target`); it enqueues one kernel on the caller's HIP
stream and reads nothing back.  An actor step draws its utd x B rows with one `rp_sac_sample` launch and acts on all
their next observations with one `rp_sac_act` launch; every critic step is one `rp_droq_target` launch on its B rows
plus plain torch (the loss, autograd with torch's own dropout, Adam, the Polyak step), or, with
`DroQ(critic_step="fused")`, plus the two launches of `critic.step` (include/learn/rp_critic.h), whose dropout masks are
a function of (seed, round) too; the actor's and the temperature's step is plain torch, or, with
`DroQ(actor_step="fused")`, the two launches of `actor.step` (include/learn/rp_actor.h).  What does not depend on the
number of learners is `DroQCore`, which
`population.DroQPopulation` shares.  Like the engine, the library has no CPU fallback: a missing library is an error.
"""

from __future__ import annotations

import ctypes

from robopianist_amd import _abi, actor, critic, offpolicy
from robopianist_amd.learning import LearnError, Mlp, _train_and_evaluate
from robopianist_amd.offpolicy import SAC, _masked_mean, actor_loss, alpha_loss, critic_loss, squashed_gaussian

EXPORTED_SYMBOLS = ("rp_droq_target", "rp_droq_dim", "rp_droq_last_error")

MAX_CRITICS = offpolicy.MAX_CRITICS
COUNTER = 32   # the last Philox counter word of critic i, layer L is COUNTER + 2 i + L

_p, _i, _u32, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_float


class Critic(ctypes.Structure):
    """rp_droq_critic."""
    _fields_ = [("net", Mlp), ("g1", _p), ("be1", _p), ("g2", _p), ("be2", _p)]


class TargetArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("next_obs", _p), ("action", _p), ("logp", _p), ("reward", _p),
                ("discount", _p), ("mean", _p), ("inv_std", _p), ("obs_clip", _f), ("gamma", _f), ("log_alpha", _p),
                ("critics", ctypes.POINTER(Critic)), ("n_critics", _i), ("y", _p), ("q_min", _p), ("q", _p),
                ("drop_threshold", _u32), ("keep_scale", _f), ("ln_eps", _f), ("seed_lo", _u32), ("seed_hi", _u32),
                ("round", _u32), ("D", _i), ("H1", _i), ("H2", _i), ("A", _i), ("B", _i), ("row_first", _i),
                ("row_count", _i), ("hip_stream", _p)]


_ARGS = {"target": TargetArgs}


_entries = _abi.EntryTable("rp_droq_", _ARGS, LearnError, "RP_DROQ_LIB", "librp_droq.so", "DroQ target")
LIB_PATH = _entries.path
load_library, declare, make_args, call_raw, last_error, dim, _call = (
    _entries.load, _entries.declare, _entries.make_args, _entries.call_raw, _entries.last_error, _entries.dim, _entries.call)


def drop_threshold(p: float) -> int:
    """The word below which a unit is dropped: a Philox word is below it with probability p (to 2^-32)."""
    return min(int(p * 2 ** 32), 2 ** 32 - 1)


def critic_entry(tensors):
    """An rp_droq_critic from the ten tensors (w1, b1, w2, b2, w3, b3, g1, be1, g2, be2) of a critic."""
    c = Critic()
    for (name, _), t in zip(Mlp._fields_, tensors[:6]):
        setattr(c.net, name, t.data_ptr())
    c.g1, c.be1, c.g2, c.be2 = (t.data_ptr() for t in tensors[6:])
    return c


def critic_table(critics):
    """A ctypes array of rp_droq_critic from a sequence of `Critic`."""
    critics = list(critics)
    if not 1 <= len(critics) <= MAX_CRITICS:
        raise LearnError(f"the target takes 1 .. {MAX_CRITICS} critics per launch, got {len(critics)}")
    tab = (Critic * len(critics))()
    for i, c in enumerate(critics):
        tab[i] = c
    return tab


def target(next_obs, action, logp, reward, discount, mean, inv_std, obs_clip, gamma, log_alpha, critics, y, D, H1, H2, A,
           B, q_min=None, q=None, threshold=0, keep_scale=1.0, ln_eps=1e-5, seed=0, round_=0, row_first=0,
           row_count=None, hip_stream=None):
    """`critics`: a sequence of `Critic` (the target networks).  `threshold`: `drop_threshold(p)`."""
    tab = critic_table(critics)
    _call("target", next_obs=next_obs, action=action, logp=logp, reward=reward, discount=discount, mean=mean,
          inv_std=inv_std, obs_clip=float(obs_clip), gamma=float(gamma), log_alpha=log_alpha, critics=tab,
          n_critics=len(tab), y=y, q_min=q_min, q=q, drop_threshold=int(threshold), keep_scale=float(keep_scale),
          ln_eps=float(ln_eps), D=D, H1=H1, H2=H2, A=A, B=B, row_first=row_first,
          row_count=B - row_first if row_count is None else row_count, hip_stream=hip_stream,
          **_abi.seed_args(seed, round_))


class DroQCore:
    """What the DroQ learners (`DroQ`, population's `DroQPopulation`) share, as a mixin in front of an
    `offpolicy.ReplayLearner`: the hyper-parameters, the critic's architecture and its ten tensors, the utd ranges of the
    minibatch, the schedule of `update()`, the bookkeeping of the fused critic step and of the fused actor step and the
    "droq", "critic_adam" and "actor_adam" blocks of the checkpoint.  A subclass states `draw_and_act()`, `target_range(u)`, the torch body of `critic_step()`,
    `actor_step()`, `_fused_range()`, and of the fused step its workspace (`_workspace_bytes()`), its launch
    (`_launch_critic_step()`) and its loss (`_range_loss(u)`)."""

    _me = "learner"   # (how the checkpoint's refusals name the reader)

    def _init_droq(self, dropout, utd, ln_eps, critic_step, actor_step="torch"):
        self.dropout, self.utd, self.ln_eps = float(dropout), int(utd), float(ln_eps)
        if critic_step not in ("torch", "fused"):
            raise ValueError(f'critic_step must be "torch" or "fused", got {critic_step!r}')
        if actor_step not in ("torch", "fused"):
            raise ValueError(f'actor_step must be "torch" or "fused", got {actor_step!r}')
        self.critic_mode, self.actor_mode = critic_step, actor_step
        if not 0.0 <= self.dropout < 1.0:
            raise ValueError(f"dropout must lie in [0, 1), got {dropout}")
        if self.utd < 1:
            raise ValueError(f"utd must be >= 1, got {utd}")
        if not self.ln_eps > 0.0:
            raise ValueError(f"ln_eps must be > 0, got {ln_eps}")
        self._threshold = drop_threshold(self.dropout)
        self._keep_scale = 1.0 / (1.0 - self.dropout)

    def _init_ranges(self, n):
        """The minibatch of n rows in all: utd ranges of B rows per learner, drawn and acted on at once; with
        critic_step="fused" also Adam's m and v, its step count (one for all parameters), the workspace and the step's q."""
        import torch
        D, A, z = self.D, self.A, self._zeros
        self._u_obs, self._u_next, self._u_action = z(n, D), z(n, D), z(n, A)
        self._u_reward, self._u_discount, self._u_mask = z(n), z(n), z(n)
        self._u_next_action, self._u_next_logp, self._u_y = z(n, A), z(n), z(n)
        if self.critic_mode == "fused":
            self._c_m = [[torch.zeros_like(t) for t in self._critic_tensors(c)] for c in self.critics]
            self._c_v = [[torch.zeros_like(t) for t in self._critic_tensors(c)] for c in self.critics]
            self._c_t = 0
            self._c_bytes = self._workspace_bytes()
            self._c_ws, self._u_q = z(max(self._c_bytes // 4, 1)), z(self.n_critics, n)
        if self.actor_mode == "fused":
            self._a_m = [torch.zeros_like(t) for t in self._actor_tensors()]
            self._a_v = [torch.zeros_like(t) for t in self._actor_tensors()]
            self._la_m, self._la_v = torch.zeros_like(self.log_alpha), torch.zeros_like(self.log_alpha)
            self._a_t = self._la_t = 0
            self._a_bytes = actor.workspace_bytes(self.H1, self.H2, self.A, self.B)
            self._a_ws, self._a_stats = z(max(self._a_bytes // 4, 1)), z(len(actor.STATS))

    def _draw_member(self):
        """One learner's actor (SAC's tanh network) and critics, drawn in this order from torch's global generator."""
        from torch import nn
        p, eps = self.dropout, self.ln_eps
        critic_net = lambda n_in: nn.Sequential(
            nn.Linear(n_in, self.H1), nn.Dropout(p), nn.LayerNorm(self.H1, eps), nn.ReLU(),
            nn.Linear(self.H1, self.H2), nn.Dropout(p), nn.LayerNorm(self.H2, eps), nn.ReLU(), nn.Linear(self.H2, 1))
        return self._net(self.D, 2 * self.A), [critic_net(self.D + self.A) for _ in range(self.n_critics)]

    _draw = _draw_member   # (a learner of one member; a population stacks its members' draws)

    def _critic_tensors(self, net):
        """The ten parameters of `net` in rp_droq_critic's order, as they are now."""
        import torch
        tensors = [t for i in (0, 4, 8) for t in (net[i].weight, net[i].bias)]
        tensors += [t for i in (2, 6) for t in (net[i].weight, net[i].bias)]
        for t in tensors:
            if not t.is_contiguous() or t.dtype != torch.float32:
                raise LearnError(f"{self._reads} contiguous float32 parameters")
        return tensors

    def _critic_table(self, net):
        """`net` as rp_droq_critic: the addresses of the parameters as they are now."""
        return critic_entry(self._critic_tensors(net))

    def _actor_tensors(self):
        """The six parameters of the actor in rp_actor_set's order, as they are now."""
        import torch
        tensors = [t for i in (0, 2, 4) for t in (self.actor[i].weight, self.actor[i].bias)]
        for t in tensors:
            if not t.is_contiguous() or t.dtype != torch.float32:
                raise LearnError(f"{self._reads} contiguous float32 parameters")
        return tensors

    # -- the gradient steps ----------------------------------------------------------------------------------------------
    def _fused_actor_step(self, u):
        """The fused actor and temperature step on range u: two launches; returns the device array of its statistics
        (actor.STATS' order), which `_host_stats` reads."""
        import torch
        ga, gt = self.actor_optimizer.param_groups[0], self.alpha_optimizer.param_groups[0]
        self._a_t += 1
        self._la_t += 1
        with torch.cuda.device(self._dev):
            actor.step(self._u_obs.data_ptr(), self._u_mask.data_ptr(), self._mean_f32.data_ptr(), self._inv_std_f32.data_ptr(),
                       self.obs_clip, actor.set_entry(self._actor_tensors()), actor.set_entry(self._a_m),
                       actor.set_entry(self._a_v), [critic.set_entry(self._critic_tensors(c)) for c in self.critics],
                       self.log_alpha.data_ptr(), self._la_m.data_ptr(), self._la_v.data_ptr(), self.target_entropy,
                       self.log_std_bounds, self._a_ws.data_ptr(), self._a_bytes, self._a_stats.data_ptr(), self.D, self.H1,
                       self.H2, self.A, self.utd * self.B,
                       actor.adam_entry(ga["lr"], self._a_t, ga["betas"], ga["eps"]),
                       actor.adam_entry(gt["lr"], self._la_t, gt["betas"], gt["eps"]), threshold=self._threshold,
                       keep_scale=self._keep_scale, ln_eps=self.ln_eps, seed=self.seed, round_=self._round,
                       row_first=u * self.B, row_count=self.B, hip_stream=self._stream())
        return {"actor_stats": self._a_stats}

    def _host_stats(self, stats):
        """The replay learner's read-back; the fused actor step's five statistics come from its device array."""
        stats = dict(stats)
        fused = stats.pop("actor_stats", None)
        if fused is not None:
            stats.update(zip(actor.STATS, fused.tolist()))
        return super()._host_stats(stats)

    def _fused_critic_step(self, u, loss):
        """The fused step on range u: two launches; the loss (from the step's q, y and mask) only where asked for."""
        import torch
        group = self.critic_optimizer.param_groups[0]
        self._c_t += 1
        step_size, bc2_sqrt = critic.adam_scalars(group["lr"], self._c_t, group["betas"])
        sets = lambda nets: [critic.set_entry(self._critic_tensors(net)) for net in nets]
        with torch.cuda.device(self._dev):
            self._launch_critic_step(
                self._u_obs.data_ptr(), self._u_action.data_ptr(), self._u_y.data_ptr(), self._u_mask.data_ptr(),
                self._mean_f32.data_ptr(), self._inv_std_f32.data_ptr(), self.obs_clip, sets(self.critics),
                [critic.set_entry(m) for m in self._c_m], [critic.set_entry(v) for v in self._c_v], sets(self.targets),
                self._u_q.data_ptr(), self._c_ws.data_ptr(), self._c_bytes, self.D, self.H1, self.H2, self.A,
                step_size=step_size, bc2_sqrt=bc2_sqrt, eps=group["eps"], betas=group["betas"], tau=self.tau,
                threshold=self._threshold, keep_scale=self._keep_scale, ln_eps=self.ln_eps, seed=self.seed,
                round_=self._round, row_first=u * self.B, row_count=self.B, hip_stream=self._stream())
        return self._range_loss(u) if loss else None

    def update(self, g: int = 1):
        """g actor steps of utd critic steps each; returns the statistics of the last one (`_host_stats`)."""
        if self.n_written < 2:
            raise LearnError("update() needs at least two TimeSteps in the ring: call collect() first")
        stats = {}
        for k in range(int(g)):
            self.draw_and_act()
            for u in range(self.utd):
                batch = self.target_range(u)
                if self.critic_mode == "fused":   # (the loss costs torch launches: only where it is returned)
                    lc = self.critic_step(batch, loss=u == self.utd - 1 and k == int(g) - 1)
                else:
                    lc = self.critic_step(batch)
            stats = dict({} if lc is None else {"critic_loss": lc}, **self.actor_step(batch))
            if self.critic_mode == "fused" and self.actor_mode == "torch":
                self.critic_optimizer.zero_grad(set_to_none=True)   # (the actor pass's critic gradients: nobody reads them)
            self._round += 1
        return self._host_stats(stats)

    # -- checkpoint / resume -------------------------------------------------------------------------------------------
    def state_dict(self, include_replay: bool = False):
        """The replay learner's (Module.state_dict carries the LayerNorm parameters), plus "dropout", "utd" and "ln_eps";
        with critic_step="fused" also the mode and the critics' Adam state (m, v per tensor and the step count)."""
        sd = super().state_dict(include_replay)
        sd["droq"] = {"dropout": self.dropout, "utd": self.utd, "ln_eps": self.ln_eps}
        if self.critic_mode == "fused":
            sd["droq"]["critic_step"] = "fused"
            c = lambda group: [[t.detach().clone() for t in net] for net in group]
            sd["critic_adam"] = {"m": c(self._c_m), "v": c(self._c_v), "t": self._c_t}
        if self.actor_mode == "fused":
            sd["droq"]["actor_step"] = "fused"
            c = lambda group: [t.detach().clone() for t in group]
            sd["actor_adam"] = {"actor": {"m": c(self._a_m), "v": c(self._a_v), "t": self._a_t},
                                "log_alpha": {"m": self._la_m.detach().clone(), "v": self._la_v.detach().clone(), "t": self._la_t}}
        return sd

    def load_state_dict(self, sd):
        """A checkpoint written with another dropout, utd, ln_eps or critic_step is refused."""
        mine = {"dropout": self.dropout, "utd": self.utd, "ln_eps": self.ln_eps}
        for k, v in mine.items():
            if "droq" not in sd or sd["droq"].get(k) != v:
                got = sd.get("droq", {}).get(k, "nothing")
                raise ValueError(f"the checkpoint was written with {k} = {got}, this {self._me} has {k} = {v}")
        got = sd["droq"].get("critic_step", "torch")
        if got != self.critic_mode:
            raise ValueError(f"the checkpoint was written with critic_step = {got}, this {self._me} has critic_step = "
                             f"{self.critic_mode}")
        got = sd["droq"].get("actor_step", "torch")
        if got != self.actor_mode:
            raise ValueError(f"the checkpoint was written with actor_step = {got}, this {self._me} has actor_step = "
                             f"{self.actor_mode}")
        super().load_state_dict(sd)
        if self.actor_mode == "fused":
            mine = sd["actor_adam"]
            for group, src in ((self._a_m, mine["actor"]["m"]), (self._a_v, mine["actor"]["v"])):
                for t, s_ in zip(group, src):
                    t.copy_(s_)
            self._la_m.copy_(mine["log_alpha"]["m"])
            self._la_v.copy_(mine["log_alpha"]["v"])
            self._a_t, self._la_t = int(mine["actor"]["t"]), int(mine["log_alpha"]["t"])
        if self.critic_mode == "fused":
            for mine, theirs in ((self._c_m, sd["critic_adam"]["m"]), (self._c_v, sd["critic_adam"]["v"])):
                for net, src in zip(mine, theirs):
                    for t, s_ in zip(net, src):
                        t.copy_(s_)
            self._c_t = int(sd["critic_adam"]["t"])


class DroQ(DroQCore, SAC):
    """DroQ (Hiroe et al. 2022): `SAC` whose critics are Linear -> Dropout(`dropout`) -> LayerNorm -> ReLU twice, with
    `utd` critic steps (the update-to-data ratio) per actor step.  The actor stays SAC's tanh network.

    `update(g)` takes g actor steps.  Each draws utd x `batch_size` rows in one sampler launch and acts on all their
    next observations in one launch (the actor does not change in between); critic step u then computes its TD target
    on the rows [u B, (u + 1) B) with `rp_droq_target`, whose dropout masks come from the learner's (seed, round), and
    takes its Adam and Polyak steps in torch.  The actor and the temperature step on the last range.

    `critic_step`: "torch" (the default: autograd with torch's own dropout, torch's Adam, `_foreach_lerp_`) or "fused"
    (`critic.step`: the same step in two launches, with Philox dropout masks keyed by (seed, round, row); the learner
    then owns Adam's m and v and its step count, and torch's critic optimiser stays unused).

    `actor_step`: "torch" (the default: autograd through the actor and every critic, a draw from the learner's
    `torch.Generator`, torch's two Adams) or "fused" (`actor.step`, include/learn/rp_actor.h: the actor's and the
    temperature's step in two launches, with noise and dropout masks keyed by (seed, round, row); the learner then owns the
    two optimisers' m, v and step counts, its generator is not advanced and no parameter gets a .grad).  The two options
    are independent."""

    def __init__(self, env, *sac_args, dropout: float = 0.01, utd: int = 20, ln_eps: float = 1e-5,
                 critic_step: str = "torch", actor_step: str = "torch", **sac_kwargs):
        self._init_droq(dropout, utd, ln_eps, critic_step, actor_step)
        super().__init__(env, *sac_args, **sac_kwargs)
        self._init_ranges(self.utd * self.B)
        self._set_range(self.utd - 1)

    def _workspace_bytes(self):
        return critic.workspace_bytes(self.n_critics, self.H1, self.H2, self.B)

    # -- the minibatch ---------------------------------------------------------------------------------------------------
    def _set_range(self, u):
        """The minibatch views (`_b_*`, what `minibatch()` and `gradient_step()` read) on range u."""
        r = slice(u * self.B, (u + 1) * self.B)
        self._b_obs, self._b_next, self._b_action = self._u_obs[r], self._u_next[r], self._u_action[r]
        self._b_reward, self._b_discount, self._b_mask = self._u_reward[r], self._u_discount[r], self._u_mask[r]
        self._b_next_action, self._b_next_logp, self._b_y = self._u_next_action[r], self._u_next_logp[r], self._u_y[r]

    def draw_and_act(self):
        """The two launches of an actor step that cover all utd ranges: the utd x B rows of the minibatch, and the
        policy at their next observations."""
        import torch
        n = self.utd * self.B
        with torch.cuda.device(self._dev):
            st = self._stream()
            offpolicy.sample(self._obs.data_ptr(), self._action.data_ptr(), self._reward.data_ptr(),
                             self._discount.data_ptr(), self._step_type.data_ptr(), self._u_obs.data_ptr(),
                             self._u_next.data_ptr(), self._u_action.data_ptr(), self._u_reward.data_ptr(),
                             self._u_discount.data_ptr(), self._u_mask.data_ptr(), self.n_written, self.C, self.E, self.D,
                             self.A, n, seed=self.seed, round_=self._round, hip_stream=st)
            self._act(self._u_next, n, st, action=self._u_next_action.data_ptr(), logp=self._u_next_logp.data_ptr())

    def target_range(self, u):
        """The TD target of range u from the target critics as they are now (one launch); returns `minibatch()` on it."""
        import torch
        with torch.cuda.device(self._dev):
            target(self._u_next.data_ptr(), self._u_next_action.data_ptr(), self._u_next_logp.data_ptr(),
                   self._u_reward.data_ptr(), self._u_discount.data_ptr(), self._mean_f32.data_ptr(),
                   self._inv_std_f32.data_ptr(), self.obs_clip, self.gamma, self.log_alpha.data_ptr(),
                   [self._critic_table(t) for t in self.targets], self._u_y.data_ptr(), self.D, self.H1, self.H2, self.A,
                   self.utd * self.B, threshold=self._threshold, keep_scale=self._keep_scale, ln_eps=self.ln_eps,
                   seed=self.seed, round_=self._round, row_first=u * self.B, row_count=self.B, hip_stream=self._stream())
        self._set_range(u)
        return self.minibatch()

    def sample_and_target(self):
        """SAC's meaning at utd == 1: the minibatch, the policy at its next observations, the TD target."""
        if self.utd != 1:
            raise LearnError("sample_and_target() is one gradient step's launches: with utd > 1 use update()")
        self.draw_and_act()
        batch = self.target_range(0)
        self._round += 1
        return batch

    # -- the gradient steps ----------------------------------------------------------------------------------------------
    def _fused_range(self, batch, option="critic_step"):
        """The range u whose views `batch` holds (what `target_range(u)` and `minibatch()` return)."""
        D, B = self.D, self.B
        off = batch["obs"].data_ptr() - self._u_obs.data_ptr()
        u = off // (4 * D * B)
        if off < 0 or off % (4 * D * B) or u >= self.utd or batch["obs"].shape[0] != B or \
                any(batch[k].data_ptr() != getattr(self, "_u_" + k)[u * B:].data_ptr() for k in ("action", "y", "mask")):
            raise LearnError(f'{option}="fused" steps on a range of the learner\'s own minibatch: pass what '
                             "target_range(u) or minibatch() returned")
        return u

    def _launch_critic_step(self, *block, **options):
        critic.step(*block, self.utd * self.B, **options)

    def _range_loss(self, u):
        r = slice(u * self.B, (u + 1) * self.B)
        return critic_loss(list(self._u_q[:, r]), self._u_y[r], self._u_mask[r])

    def critic_step(self, batch, loss: bool = True):
        """The critics' Adam step on `batch` (torch's own dropout: the modules are in train() mode) and the targets'
        Polyak step over all parameters, LayerNorm's included.  Returns the loss (a tensor).  With critic_step="fused":
        the two launches of `critic.step` on the range `batch` views, and the loss only if `loss`."""
        import torch
        if self.critic_mode == "fused":
            return self._fused_critic_step(self._fused_range(batch), loss)
        xa = torch.cat([self.normalize(batch["obs"]), batch["action"]], dim=1)
        lc = critic_loss([c(xa).squeeze(-1) for c in self.critics], batch["y"], batch["mask"])
        self.critic_optimizer.zero_grad(set_to_none=True)
        lc.backward()
        self.critic_optimizer.step()
        with torch.no_grad():
            torch._foreach_lerp_([p for t in self.targets for p in t.parameters()],
                                 [p for c in self.critics for p in c.parameters()], self.tau)
        return lc.detach()

    def actor_step(self, batch):
        """The actor's and the temperature's Adam steps on `batch`; the critics stay in train() mode, as in the paper.
        With actor_step="fused": the two launches of `actor.step` on the range `batch` views; the statistics then stay on
        the device until `_host_stats` reads them."""
        import torch
        if self.actor_mode == "fused":
            return self._fused_actor_step(self._fused_range(batch, "actor_step"))
        mask = batch["mask"]
        xn = self.normalize(batch["obs"])
        eps = torch.randn(xn.shape[0], self.A, generator=self._gen, device=xn.device)
        a_new, logp_new, _ = squashed_gaussian(self.actor(xn), eps, self.log_std_bounds)
        xa_new = torch.cat([xn, a_new], dim=1)
        q_new = torch.stack([c(xa_new).squeeze(-1) for c in self.critics]).min(0).values
        la = actor_loss(self.log_alpha, logp_new, q_new, mask)
        self.actor_optimizer.zero_grad(set_to_none=True)
        la.backward()   # (the critics' gradients of this pass are dropped by their next zero_grad)
        self.actor_optimizer.step()
        lt = alpha_loss(self.log_alpha, logp_new, self.target_entropy, mask)
        self.alpha_optimizer.zero_grad(set_to_none=True)
        lt.backward()
        self.alpha_optimizer.step()
        return {"actor_loss": la.detach(), "alpha_loss": lt.detach(), "alpha": self.log_alpha.detach().exp()[0],
                "entropy": -_masked_mean(logp_new.detach(), mask), "masked": 1.0 - mask.mean()}

    def gradient_step(self, batch):
        """One critic step (with its Polyak step) and one actor and temperature step on `batch`: SAC's meaning."""
        lc = self.critic_step(batch)
        return dict({"critic_loss": lc}, **self.actor_step(batch))


def train_and_evaluate(env, rounds: int, steps_per_round: int = 16, grad_steps: int = 1, time_limit: float = None,
                       log=print, **droq_kwargs):
    """What the examples' --train-droq does: `rounds` rounds of DroQ on `env` (a batched Environment), one line per
    round with the mean return of the episodes that ended in it, then one deterministic episode of every env through a
    MidiEvaluationWrapper.  Stops early after `time_limit` seconds.  Returns (droq, log of the rounds, metrics)."""
    learner = DroQ(env, **droq_kwargs)
    train_one = lambda cb: learner.train(1, steps_per_round, grad_steps, callback=cb)
    rounds_log, metrics = _train_and_evaluate(learner, rounds, train_one, ("alpha", "alpha"), time_limit, log)
    return learner, rounds_log, metrics
