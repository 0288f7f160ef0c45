"""ctypes binding of the off-policy learner kernels' C ABI (include/learn/rp_sac.h, librp_sac.so) and `SAC`, soft
actor-critic over a batched environment with the replay ring kept on the device.

The three entry points are module functions taking raw device addresses (`sample`, `act`, `target`); each enqueues one
kernel on the caller's HIP stream and reads nothing back.  The ring is written by the learner's unchanged `pack`
(learning.py), its normaliser is the learner's `moments`.  Per control step `SAC.collect()` enqueues `act`, the
environment's step and `pack`: HIP kernels only, no torch kernel of its own.  A gradient step (`SAC.update`) draws its
minibatch and computes its TD target with the kernels; the losses (`critic_loss`, `actor_loss`, `alpha_loss`), autograd
and Adam are plain torch.  Like the engine, the library has no CPU fallback: a missing library is an error.
"""

from __future__ import annotations

import copy
import ctypes
import math

from robopianist_amd import _abi
from robopianist_amd.learning import (F32, F64, MAX_ACTIONS, MAX_FIELDS, MAX_HIDDEN, STEP_FIRST, STEP_LAST, STEP_MID,  # noqa: F401
                                      LOG_2PI, DeviceLearner, LearnError, Mlp, _train_and_evaluate, _unwrap, field_table,
                                      mlp_table, moments, pack)

EXPORTED_SYMBOLS = ("rp_sac_sample", "rp_sac_act", "rp_sac_target", "rp_sac_dim", "rp_sac_last_error")

MAX_CRITICS = 4
SAMPLE_TRIES = 4
LN_2 = math.log(2.0)

_p, _i, _u32, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_float


class SampleArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("ring_obs", _p), ("ring_action", _p), ("ring_reward", _p),
                ("ring_discount", _p), ("ring_step_type", _p), ("obs", _p), ("next_obs", _p), ("action", _p),
                ("reward", _p), ("discount", _p), ("mask", _p), ("index", _p), ("n_written", ctypes.c_longlong),
                ("seed_lo", _u32), ("seed_hi", _u32), ("round", _u32), ("C", _i), ("E", _i), ("D", _i), ("A", _i),
                ("B", _i), ("row_first", _i), ("row_count", _i), ("hip_stream", _p)]


class ActArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("obs", _p), ("mean", _p), ("inv_std", _p), ("obs_clip", _f),
                ("log_std_min", _f), ("log_std_max", _f), ("actor", ctypes.POINTER(Mlp)), ("action", _p), ("logp", _p),
                ("pre", _p), ("env_action", _p), ("precision", _i), ("deterministic", _i), ("seed_lo", _u32),
                ("seed_hi", _u32), ("round", _u32), ("D", _i), ("H1", _i), ("H2", _i), ("A", _i), ("n_rows", _i),
                ("row_first", _i), ("row_count", _i), ("hip_stream", _p)]


class TargetArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("next_obs", _p), ("action", _p), ("logp", _p), ("reward", _p),
                ("discount", _p), ("mean", _p), ("inv_std", _p), ("obs_clip", _f), ("gamma", _f), ("log_alpha", _p),
                ("critics", ctypes.POINTER(Mlp)), ("n_critics", _i), ("y", _p), ("q_min", _p), ("D", _i), ("H1", _i),
                ("H2", _i), ("A", _i), ("B", _i), ("row_first", _i), ("row_count", _i), ("hip_stream", _p)]


_ARGS = {"sample": SampleArgs, "act": ActArgs, "target": TargetArgs}


_entries = _abi.EntryTable("rp_sac_", _ARGS, LearnError, "RP_SAC_LIB", "librp_sac.so", "off-policy learner")
LIB_PATH = _entries.path
load_library, declare, make_args, call_raw, last_error, dim, _call = (
    _entries.load, _entries.declare, _entries.make_args, _entries.call_raw, _entries.last_error, _entries.dim, _entries.call)


def critic_table(critics):
    """A ctypes array of rp_learn_mlp from a sequence of `Mlp`."""
    critics = list(critics)
    if not 1 <= len(critics) <= MAX_CRITICS:
        raise LearnError(f"the target takes 1 .. {MAX_CRITICS} critics per launch, got {len(critics)}")
    tab = (Mlp * len(critics))()
    for i, m in enumerate(critics):
        tab[i] = m
    return tab


def sample(ring_obs, ring_action, ring_reward, ring_discount, ring_step_type, obs, next_obs, action, reward, discount,
           mask, n_written, C, E, D, A, B, index=None, seed=0, round_=0, row_first=0, row_count=None, hip_stream=None):
    _call("sample", ring_obs=ring_obs, ring_action=ring_action, ring_reward=ring_reward, ring_discount=ring_discount,
          ring_step_type=ring_step_type, obs=obs, next_obs=next_obs, action=action, reward=reward, discount=discount,
          mask=mask, index=index, n_written=int(n_written), C=C, E=E, D=D, A=A, B=B, row_first=row_first,
          row_count=B - row_first if row_count is None else row_count, hip_stream=hip_stream,
          **_abi.seed_args(seed, round_))


def act(obs, mean, inv_std, obs_clip, actor, D, H1, H2, A, n_rows, log_std_bounds=(-5.0, 2.0), action=None, logp=None,
        pre=None, env_action=None, precision=64, deterministic=False, seed=0, round_=0, row_first=0, row_count=None,
        hip_stream=None):
    """`actor`: an `Mlp` whose last layer has 2 A outputs."""
    _call("act", obs=obs, mean=mean, inv_std=inv_std, obs_clip=float(obs_clip), log_std_min=float(log_std_bounds[0]),
          log_std_max=float(log_std_bounds[1]), actor=ctypes.pointer(actor) if actor is not None else None,
          action=action, logp=logp, pre=pre, env_action=env_action, precision=precision,
          deterministic=int(bool(deterministic)), D=D, H1=H1, H2=H2, A=A, n_rows=n_rows, row_first=row_first,
          row_count=n_rows - row_first if row_count is None else row_count, hip_stream=hip_stream,
          **_abi.seed_args(seed, round_))


def target(next_obs, action, logp, reward, discount, mean, inv_std, obs_clip, gamma, log_alpha, critics, y, D, H1, H2, A,
           B, q_min=None, row_first=0, row_count=None, hip_stream=None):
    """`critics`: a sequence of `Mlp` (the target networks)."""
    tab = critic_table(critics)
    _call("target", next_obs=next_obs, action=action, logp=logp, reward=reward, discount=discount, mean=mean,
          inv_std=inv_std, obs_clip=float(obs_clip), gamma=float(gamma), log_alpha=log_alpha, critics=tab,
          n_critics=len(tab), y=y, q_min=q_min, D=D, H1=H1, H2=H2, A=A, B=B, row_first=row_first,
          row_count=B - row_first if row_count is None else row_count, hip_stream=hip_stream)


# ---- the losses ----------------------------------------------------------------------------------------------------------
def squashed_gaussian(out, eps, log_std_bounds):
    """The kernel's epilogue in torch, differentiable: `out` [n, 2 A] is the actor's head, `eps` [n, A] the draw.
    -> (a = tanh(p), logp, p)."""
    import torch
    A = out.shape[-1] // 2
    mu, l = out[..., :A], out[..., A:]
    ls = torch.clamp(l, float(log_std_bounds[0]), float(log_std_bounds[1]))
    p = mu + ls.exp() * eps
    w = -2.0 * p
    sp = torch.clamp(w, min=0.0) + torch.log1p(torch.exp(-w.abs()))
    lg = 2.0 * (LN_2 - p - sp)
    logp = ((-0.5 * eps * eps - ls) - lg).sum(-1) - 0.5 * A * LOG_2PI
    return torch.tanh(p), logp, p


def _masked_mean(x, mask):
    return (x * mask).sum() / mask.sum().clamp(min=1.0)


def critic_loss(qs, y, mask):
    """The mask-weighted mean over the rows of 0.5 (Q_i - y)^2, summed over the ensemble.  `qs`: a list of [n]."""
    return sum(_masked_mean(0.5 * (q - y) ** 2, mask) for q in qs)


def actor_loss(log_alpha, logp_new, q_new, mask):
    """The mask-weighted mean of alpha logp_new - min_i Q_i(x, a_new); alpha is a constant here."""
    return _masked_mean(log_alpha.detach().exp() * logp_new - q_new, mask)


def alpha_loss(log_alpha, logp_new, target_entropy, mask):
    """The temperature's loss: the mask-weighted mean of -log_alpha (logp_new + target_entropy)."""
    return _masked_mean(-log_alpha * (logp_new.detach() + float(target_entropy)), mask)


class ReplayLearner(DeviceLearner):
    """What the learners over a replay ring (`SAC`, population's `DroQPopulation`) share: the ring of `capacity` slots of E
    rows, `collect()` into it, the networks' targets, the three Adams, the round loop of `train()` and the checkpoint.  A
    slot's rows belong to one actor or to several; a subclass says which: `_draw()` (the actor and the critics, from
    torch's global generator), `_act()` and `_act_envs()` (the policy kernel on any rows, and on a slot's), `_merge_run()`
    (k slots into the normaliser), `_mean_reward()` (of a round's new slots) and `_host_stats()` (an update's read-back).
    Its constructor calls `DeviceLearner.__init__`, then `_init_replay`."""

    def _init_replay(self, rows, per, hidden, n_critics, capacity, batch_size, tau, lr, log_alpha, log_std_bounds,
                     learning_starts, obs_clip, seed, norm_eps):
        """`rows`: the rows of a slot that one actor owns, named `per` by the 2^32 bound; `log_alpha`: a list of floats."""
        import torch
        from torch import nn
        self.C, self.B = int(capacity), int(batch_size)
        if self.C < 2:
            raise ValueError("capacity must be >= 2 slots")
        if self.B < 1:
            raise ValueError("batch_size must be >= 1")
        if (self.C - 1) * rows >= 2 ** 32:
            raise ValueError(f"(capacity - 1) x {per} must stay below 2^32")
        self._init_specs(hidden, obs_clip, seed, norm_eps)
        self.n_critics = int(n_critics)
        if not 1 <= self.n_critics <= MAX_CRITICS:
            raise ValueError(f"n_critics must be 1 .. {MAX_CRITICS}, got {n_critics}")
        self.tau = float(tau)
        self.log_std_bounds = (float(log_std_bounds[0]), float(log_std_bounds[1]))
        if not self.log_std_bounds[0] <= self.log_std_bounds[1]:
            raise ValueError("log_std_bounds must be (min, max) with min <= max")
        self.learning_starts = int(learning_starts)
        self.n_written = 0
        with torch.random.fork_rng(devices=[]):   # (the global generator is left as it was)
            torch.manual_seed(self.seed)
            self.actor, self.critics = self._draw()
        self.actor.to(self._dev)
        for c in self.critics:
            c.to(self._dev)
        self.targets = [copy.deepcopy(c) for c in self.critics]
        for t in self.targets:
            t.requires_grad_(False)
        self.log_alpha = nn.Parameter(torch.tensor(log_alpha, dtype=torch.float32, device=self._dev))
        adam = lambda params: torch.optim.Adam(params, lr=float(lr))
        self.actor_optimizer = adam(list(self.actor.parameters()))
        self.critic_optimizer = adam([p for c in self.critics for p in c.parameters()])
        self.alpha_optimizer = adam([self.log_alpha])
        # the gradient step's own draws (torch's rsample); a CPU device keeps the host tests possible
        self._gen = torch.Generator(device=self._dev).manual_seed(self.seed)
        C, E, D, A, z = self.C, self.E, self.D, self.A, self._zeros
        self._obs, self._reward, self._discount = z(C, E, D), z(C, E), z(C, E)
        self._step_type, self._action = z(C, E, dtype=torch.int32), z(C, E, A)
        self._logp, self._env_action = z(E), z(E, A, dtype=self._dtype)

    def ring(self):
        """The replay ring as a dict of views (live); TimeStep m lives in slot m mod capacity."""
        return {"obs": self._obs, "reward": self._reward, "discount": self._discount, "step_type": self._step_type,
                "action": self._action}

    # -- collection ----------------------------------------------------------------------------------------------------
    def collect(self, n: int):
        """The next n control steps of every env into the ring (the first call resets the env and writes TimeStep 0
        first), then the new slots into the normaliser.  Returns `ring()`."""
        import torch
        C, n = self.C, int(n)
        with torch.cuda.device(self._dev):
            st = self._stream()
            kept = []
            first_new = self.n_written
            if self.n_written == 0:
                ts = self._env.reset()
                self._pack(ts, 0, st)
                kept.append(ts)
                self.n_written = 1
            for _ in range(n):
                newest = (self.n_written - 1) % C
                self._act_envs(self._obs[newest], st, action=self._action[newest].data_ptr(), logp=self._logp.data_ptr(),
                               env_action=self._env_action.data_ptr(), precision=self._precision)
                self._round += 1
                ts = self._env.step_canonical(self._env_action, self._bounds, False)
                self._pack(ts, self.n_written % C, st)
                self.n_written += 1
                kept.append(ts)
            self._merge(first_new, self.n_written, st)
            self._keep = kept   # alive until the kernels have run
        return self.ring()

    def _merge(self, first, end, st):
        """The TimeSteps first .. end - 1 that the ring still holds into the running moments: one launch per contiguous
        run of slots (two where the slots wrap)."""
        C = self.C
        first = max(first, end - C)
        while first < end:
            s = first % C
            k = min(end - first, C - s)
            self._merge_run(self._obs[s], k, st)
            first += k

    def _host_stats(self, stats):
        """The last gradient step's statistics as `update()` returns them."""
        return {k: float(v) for k, v in stats.items()}

    def train(self, n: int, steps_per_round: int = 1, grad_steps: int = 1, callback=None):
        """n rounds of collect(steps_per_round) and, once `learning_starts` control steps have been collected,
        update(grad_steps); returns the list of per-round statistics (the update's, plus "mean_reward": the mean reward
        of the round's new TimeSteps that are not FIRST, and `episode_stats()`)."""
        import torch
        log = []
        for i in range(int(n)):
            first = max(self.n_written, 1)
            self.collect(steps_per_round)
            s = self.update(grad_steps) if self.n_written - 1 >= max(self.learning_starts, 1) and grad_steps > 0 else {}
            slots = torch.arange(max(first, self.n_written - self.C), self.n_written, device=self._dev) % self.C
            s["mean_reward"] = self._mean_reward(slots)
            s.update(self.episode_stats())
            log.append(s)
            if callback is not None:
                callback(i, s)
        return log

    # -- evaluation ----------------------------------------------------------------------------------------------------
    def act(self, observation, deterministic: bool = True):
        """The policy's action for an observation dict of E rows: [E, A] of the engine's dtype in [-1, 1] (what a
        CanonicalSpecWrapper's step takes).  Live: the next call overwrites it."""
        import torch
        with torch.cuda.device(self._dev):
            st = self._stream()
            self._pack_observation(observation, st)
            self._act_envs(self._e_obs, st, action=self._e_action.data_ptr(), logp=self._e_logp.data_ptr(),
                           env_action=self._e_env_action.data_ptr(), precision=self._precision, deterministic=deterministic)
            if not deterministic:
                self._round += 1
        return self._e_env_action

    # -- checkpoint / resume -------------------------------------------------------------------------------------------
    def state_dict(self, include_replay: bool = False):
        """The networks, the targets, the three Adams, log_alpha, the normaliser, the seed, round and n_written
        counters, the torch generator of the gradient step, the running episode statistics and the newest slot (the
        TimeStep the next `collect()` acts on); the whole ring only with `include_replay`.  With the env's own
        `state_dict()` the next `collect()` is resumed bit for bit."""
        c = lambda t: t.detach().clone()
        nets = lambda ms: [{k: c(v) for k, v in m.state_dict().items()} for m in ms]
        newest = (self.n_written - 1) % self.C if self.n_written else 0
        sd = {"actor": nets([self.actor])[0], "critics": nets(self.critics), "targets": nets(self.targets),
              "log_alpha": c(self.log_alpha),
              "optimizers": {k: copy.deepcopy(getattr(self, k + "_optimizer").state_dict())
                             for k in ("actor", "critic", "alpha")},
              "normalizer": self._normalizer_state(),
              "seed": self.seed, "round": self._round, "n_written": self.n_written, "generator": self._gen.get_state(),
              "newest": {"obs": c(self._obs[newest]), "reward": c(self._reward[newest]),
                         "discount": c(self._discount[newest]), "step_type": c(self._step_type[newest])},
              "episodes": self._episodes_state()}
        if include_replay:
            sd["replay"] = {k: c(v) for k, v in self.ring().items()}
        return sd

    def load_state_dict(self, sd):
        """Without the ring in `sd` the ring restarts from the newest slot alone: its older slots are marked LAST, so
        nothing the snapshot did not hold can be drawn."""
        import torch
        self.actor.load_state_dict(sd["actor"])   # (in place)
        for group, key in ((self.critics, "critics"), (self.targets, "targets")):
            for m, s in zip(group, sd[key]):
                m.load_state_dict(s)
        with torch.no_grad():
            self.log_alpha.copy_(sd["log_alpha"])
        for k, s in sd["optimizers"].items():
            getattr(self, k + "_optimizer").load_state_dict(copy.deepcopy(s))   # (Adam would adopt sd's own tensors)
        self._load_shared_state(sd)
        self.seed, self._round, self.n_written = int(sd["seed"]), int(sd["round"]), int(sd["n_written"])
        self._gen.set_state(sd["generator"])
        if "replay" in sd:
            for k, v in sd["replay"].items():
                self.ring()[k].copy_(v)
        else:
            self._step_type.fill_(STEP_LAST)
        newest = (self.n_written - 1) % self.C if self.n_written else 0
        for buf, key in ((self._obs, "obs"), (self._reward, "reward"), (self._discount, "discount"),
                         (self._step_type, "step_type")):
            buf[newest].copy_(sd["newest"][key])


class SAC(ReplayLearner):
    """Soft actor-critic (Haarnoja et al. 2018) with a tanh-squashed, state-dependent Gaussian policy, an ensemble of
    `n_critics` critics with Polyak-averaged targets and a learned temperature, over every env of `env` at once.  `env`
    is a batched `Environment` or a `CanonicalSpecWrapper` around one; the squashed action in [-1, 1]^A is what is
    stored and what `step_canonical` receives.

    The replay ring holds `capacity` slots of E rows, so (capacity - 1) E transitions; TimeStep number m lives in slot
    m mod capacity and the next observation is never stored twice.  `collect(n)` launches, on torch's current stream
    and without reading anything back, n x (act on the newest slot, env step, pack into the next slot) and merges the
    new slots into the observation normaliser.  `update(g)` takes g gradient steps on minibatches of `batch_size` rows
    drawn by the sampler kernel; rows for which the sampler found no valid transition carry mask 0 and zeros."""

    def __init__(self, env, hidden=(256, 256), n_critics: int = 2, capacity: int = 64, batch_size: int = 4096,
                 gamma: float = 0.99, tau: float = 0.005, lr: float = 3e-4, init_alpha: float = 1.0,
                 target_entropy: float = None, log_std_bounds=(-5.0, 2.0), learning_starts: int = 0,
                 obs_clip: float = 10.0, seed: int = 0, norm_eps: float = 1e-8):
        super().__init__(env)
        self._init_replay(self.E, "n_envs", hidden, n_critics, capacity, batch_size, tau, lr, [math.log(float(init_alpha))],
                          log_std_bounds, learning_starts, obs_clip, seed, norm_eps)
        self.gamma = float(gamma)
        self.target_entropy = -float(self.A) if target_entropy is None else float(target_entropy)
        # the minibatch
        B, D, A, z = self.B, self.D, self.A, self._zeros
        self._b_obs, self._b_next, self._b_action = z(B, D), z(B, D), z(B, A)
        self._b_reward, self._b_discount, self._b_mask = z(B), z(B), z(B)
        self._b_next_action, self._b_next_logp, self._b_y = z(B, A), z(B), z(B)

    def _draw(self):
        return self._net(self.D, 2 * self.A), [self._net(self.D + self.A, 1) for _ in range(self.n_critics)]

    # -- accessors ---------------------------------------------------------------------------------------------------
    @property
    def alpha(self):
        return float(self.log_alpha.detach().exp())

    def minibatch(self):
        """The buffers the last gradient step's kernels filled (live)."""
        return {"obs": self._b_obs, "next_obs": self._b_next, "action": self._b_action, "reward": self._b_reward,
                "discount": self._b_discount, "mask": self._b_mask, "next_action": self._b_next_action,
                "next_logp": self._b_next_logp, "y": self._b_y}

    def _act(self, obs, n_rows, st, **out):
        act(obs.data_ptr(), self._mean_f32.data_ptr(), self._inv_std_f32.data_ptr(), self.obs_clip, self._mlp(self.actor),
            self.D, self.H1, self.H2, self.A, n_rows, log_std_bounds=self.log_std_bounds, seed=self.seed,
            round_=self._round, hip_stream=st, **out)

    def _act_envs(self, obs, st, **out):
        self._act(obs, self.E, st, **out)

    def _merge_run(self, obs, k, st):
        self._merge_moments(obs, k * self.E, st)

    def _mean_reward(self, slots):
        live = self._step_type[slots] != STEP_FIRST
        return float(self._reward[slots][live].mean()) if bool(live.any()) else float("nan")

    # -- the gradient step ---------------------------------------------------------------------------------------------
    def sample_and_target(self):
        """The three launches of a gradient step: the minibatch, the policy at its next observations, the TD target."""
        import torch
        with torch.cuda.device(self._dev):
            st = self._stream()
            sample(self._obs.data_ptr(), self._action.data_ptr(), self._reward.data_ptr(), self._discount.data_ptr(),
                   self._step_type.data_ptr(), self._b_obs.data_ptr(), self._b_next.data_ptr(), self._b_action.data_ptr(),
                   self._b_reward.data_ptr(), self._b_discount.data_ptr(), self._b_mask.data_ptr(), self.n_written,
                   self.C, self.E, self.D, self.A, self.B, seed=self.seed, round_=self._round, hip_stream=st)
            self._act(self._b_next, self.B, st, action=self._b_next_action.data_ptr(), logp=self._b_next_logp.data_ptr())
            self._round += 1
            target(self._b_next.data_ptr(), self._b_next_action.data_ptr(), self._b_next_logp.data_ptr(),
                   self._b_reward.data_ptr(), self._b_discount.data_ptr(), self._mean_f32.data_ptr(),
                   self._inv_std_f32.data_ptr(), self.obs_clip, self.gamma, self.log_alpha.data_ptr(),
                   [self._mlp(t) for t in self.targets], self._b_y.data_ptr(), self.D, self.H1, self.H2, self.A, self.B,
                   hip_stream=st)
        return self.minibatch()

    def gradient_step(self, batch):
        """Adam steps of the critics, the actor and the temperature on `batch` (`minibatch()`'s keys "obs", "action",
        "y", "mask"), then the targets' Polyak step.  Plain torch on the batch's device; returns tensors."""
        import torch
        mask, y = batch["mask"], batch["y"]
        xn = self.normalize(batch["obs"])
        xa = torch.cat([xn, batch["action"]], dim=1)
        lc = critic_loss([c(xa).squeeze(-1) for c in self.critics], y, mask)
        self.critic_optimizer.zero_grad(set_to_none=True)
        lc.backward()
        self.critic_optimizer.step()
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
        with torch.no_grad():
            torch._foreach_lerp_([p for t in self.targets for p in t.parameters()],
                                 [p for c in self.critics for p in c.parameters()], self.tau)
        return {"critic_loss": lc.detach(), "actor_loss": la.detach(), "alpha_loss": lt.detach(),
                "alpha": self.log_alpha.detach().exp()[0], "entropy": -_masked_mean(logp_new.detach(), mask),
                "masked": 1.0 - mask.mean()}

    def update(self, g: int = 1):
        """g gradient steps; returns the statistics of the last one as floats."""
        if self.n_written < 2:
            raise LearnError("update() needs at least two TimeSteps in the ring: call collect() first")
        stats = {}
        for _ in range(int(g)):
            stats = self.gradient_step(self.sample_and_target())
        return self._host_stats(stats)


def train_and_evaluate(env, rounds: int, steps_per_round: int = 16, grad_steps: int = 4, time_limit: float = None,
                       log=print, **sac_kwargs):
    """What the examples' --train-sac does: `rounds` rounds of SAC on `env` (a batched Environment), one line per round
    with the mean return of the episodes that ended in it, then one deterministic episode of every env through a
    MidiEvaluationWrapper.  Stops early after `time_limit` seconds.  Returns (sac, log of the rounds, metrics)."""
    sac = SAC(env, **sac_kwargs)
    train_one = lambda cb: sac.train(1, steps_per_round, grad_steps, callback=cb)
    rounds_log, metrics = _train_and_evaluate(sac, rounds, train_one, ("alpha", "alpha"), time_limit, log)
    return sac, rounds_log, metrics
