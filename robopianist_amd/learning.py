"""ctypes binding of the learner kernels' C ABI (include/learn/rp_learn.h, librp_learn.so) and `PPO`, proximal policy
optimisation over a batched environment with the rollout collected on the device.

The four entry points are module functions taking raw device addresses (`pack`, `act`, `gae`, `moments`); each enqueues
one kernel on the caller's HIP stream and reads nothing back.  Per control step `PPO.collect()` enqueues `act`, the
environment's step and `pack`: HIP kernels only, no torch kernel of its own.  The gradient step (`PPO.update`,
`ppo_loss`) is plain torch -- autograd and Adam -- once per rollout.  Like the engine, the library has no CPU fallback:
a missing library is an error.
"""

from __future__ import annotations

import copy
import ctypes
import math

import numpy as np

from robopianist_amd import _abi

EXPORTED_SYMBOLS = ("rp_learn_pack", "rp_learn_act", "rp_learn_gae", "rp_learn_moments", "rp_learn_dim",
                    "rp_learn_last_error")

MAX_FIELDS = 64
MAX_HIDDEN = 256
MAX_ACTIONS = 128
F32, F64 = 0, 1
STEP_FIRST, STEP_MID, STEP_LAST = 0, 1, 2


class LearnError(RuntimeError):
    pass


_p, _i, _u32, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_double


class Field(ctypes.Structure):
    """rp_learn_field."""
    _fields_ = [("src", _p), ("width", _i), ("dtype", _i)]


class Mlp(ctypes.Structure):
    """rp_learn_mlp."""
    _fields_ = [("w1", _p), ("b1", _p), ("w2", _p), ("b2", _p), ("w3", _p), ("b3", _p)]


class PackArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("fields", ctypes.POINTER(Field)), ("n_fields", _i), ("precision", _i),
                ("step_type", _p), ("reward", _p), ("discount", _p), ("obs", _p), ("slot_reward", _p),
                ("slot_discount", _p), ("slot_step_type", _p), ("ep_return", _p), ("ep_len", _p), ("done_return", _p),
                ("done_len", _p), ("done_count", _p), ("E", _i), ("D", _i), ("env_first", _i), ("env_count", _i),
                ("hip_stream", _p)]


class ActArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("obs", _p), ("mean", _p), ("inv_std", _p), ("obs_clip", ctypes.c_float),
                ("actor", ctypes.POINTER(Mlp)), ("critic", ctypes.POINTER(Mlp)), ("log_std", _p), ("action", _p),
                ("logp", _p), ("mu", _p), ("env_action", _p), ("value", _p), ("precision", _i), ("deterministic", _i),
                ("seed_lo", _u32), ("seed_hi", _u32), ("round", _u32), ("D", _i), ("H1", _i), ("H2", _i), ("A", _i),
                ("n_rows", _i), ("row_first", _i), ("row_count", _i), ("hip_stream", _p)]


class GaeArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("reward", _p), ("discount", _p), ("step_type", _p), ("value", _p),
                ("adv", _p), ("ret", _p), ("valid", _p), ("gamma", _d), ("lambda", _d), ("T", _i), ("E", _i),
                ("env_first", _i), ("env_count", _i), ("hip_stream", _p)]


class MomentsArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("obs", _p), ("mean", _p), ("M2", _p), ("mean_f32", _p),
                ("inv_std_f32", _p), ("count", _d), ("eps", _d), ("n_rows", ctypes.c_longlong), ("D", _i),
                ("hip_stream", _p)]


_ARGS = {"pack": PackArgs, "act": ActArgs, "gae": GaeArgs, "moments": MomentsArgs}


_entries = _abi.EntryTable("rp_learn_", _ARGS, LearnError, "RP_LEARN_LIB", "librp_learn.so", "learner")
LIB_PATH = _entries.path
load_library, declare, make_args, call_raw, last_error, dim, _call = (
    _entries.load, _entries.declare, _entries.make_args, _entries.call_raw, _entries.last_error, _entries.dim, _entries.call)


def field_table(fields):
    """A ctypes array of rp_learn_field from (src address, width, dtype code) triples."""
    fields = list(fields)
    if not 1 <= len(fields) <= MAX_FIELDS:
        raise LearnError(f"a pack takes 1 .. {MAX_FIELDS} fields per launch, got {len(fields)}")
    tab = (Field * len(fields))()
    for f, (src, width, dtype) in zip(tab, fields):
        f.src, f.width, f.dtype = src, int(width), int(dtype)
    return tab


def mlp_table(tensors):
    """An rp_learn_mlp from the six tensors (w1, b1, w2, b2, w3, b3) of a network."""
    m = Mlp()
    for (name, _), t in zip(Mlp._fields_, tensors):
        setattr(m, name, t.data_ptr())
    return m


def pack(table, precision, step_type, reward, discount, obs, slot_reward, slot_discount, slot_step_type, E, D, stats=None,
         env_first=0, env_count=None, hip_stream=None):
    """`stats` = the addresses (ep_return, ep_len, done_return, done_len, done_count), or None."""
    s = dict(zip(("ep_return", "ep_len", "done_return", "done_len", "done_count"), stats)) if stats is not None else {}
    _call("pack", fields=table, n_fields=len(table), precision=precision, step_type=step_type, reward=reward,
          discount=discount, obs=obs, slot_reward=slot_reward, slot_discount=slot_discount, slot_step_type=slot_step_type,
          E=E, D=D, env_first=env_first, env_count=E - env_first if env_count is None else env_count, hip_stream=hip_stream,
          **s)


def act(obs, mean, inv_std, obs_clip, actor, critic, D, H1, H2, A, n_rows, log_std=None, action=None, logp=None, mu=None,
        env_action=None, value=None, precision=64, deterministic=False, seed=0, round_=0, row_first=0, row_count=None,
        hip_stream=None):
    """`actor`, `critic`: an `Mlp` or None."""
    _call("act", obs=obs, mean=mean, inv_std=inv_std, obs_clip=float(obs_clip),
          actor=ctypes.pointer(actor) if actor is not None else None,
          critic=ctypes.pointer(critic) if critic is not None else None, log_std=log_std, action=action, logp=logp, mu=mu,
          env_action=env_action, value=value, precision=precision, deterministic=int(bool(deterministic)),
          D=D, H1=H1, H2=H2, A=A, n_rows=n_rows, row_first=row_first,
          row_count=n_rows - row_first if row_count is None else row_count, hip_stream=hip_stream,
          **_abi.seed_args(seed, round_))


def gae(reward, discount, step_type, value, adv, ret, valid, gamma, lam, T, E, env_first=0, env_count=None,
        hip_stream=None):
    _call("gae", reward=reward, discount=discount, step_type=step_type, value=value, adv=adv, ret=ret, valid=valid,
          gamma=float(gamma), T=T, E=E, env_first=env_first, env_count=E - env_first if env_count is None else env_count,
          hip_stream=hip_stream, **{"lambda": float(lam)})


def moments(obs, mean, M2, mean_f32, inv_std_f32, count, eps, n_rows, D, hip_stream=None):
    _call("moments", obs=obs, mean=mean, M2=M2, mean_f32=mean_f32, inv_std_f32=inv_std_f32, count=float(count),
          eps=float(eps), n_rows=int(n_rows), D=D, hip_stream=hip_stream)


# ---- the loss ----------------------------------------------------------------------------------------------------------
LOG_2PI = math.log(2.0 * math.pi)


def gaussian_logp(mu, log_std, action):
    """log N(action; mu, exp(log_std)^2), summed over the last dimension."""
    z = (action - mu) * (-log_std).exp()
    return (-0.5 * z * z - log_std).sum(-1) - 0.5 * mu.shape[-1] * LOG_2PI


def ppo_loss(mu, log_std, value, action, logp_old, adv, ret, clip=0.2, vf_coef=0.5, ent_coef=0.0):
    """The clipped surrogate, the value loss and the entropy term of a batch (any device).  `adv` is used as given.
    Returns (loss, {"pg", "vf", "entropy", "approx_kl", "clip_fraction"}) -- tensors, nothing is read back."""
    import torch
    logp = gaussian_logp(mu, log_std, action)
    ratio = (logp - logp_old).exp()
    pg = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv).mean()
    vf = 0.5 * ((value - ret) ** 2).mean()
    entropy = (log_std + 0.5 * (1.0 + LOG_2PI)).sum()
    loss = pg + vf_coef * vf - ent_coef * entropy
    with torch.no_grad():
        stats = {"pg": pg.detach(), "vf": vf.detach(), "entropy": entropy.detach(),
                 "approx_kl": (logp_old - logp).mean(), "clip_fraction": ((ratio - 1.0).abs() > clip).float().mean()}
    return loss, stats


def _unwrap(env):
    """The batched Environment behind `env` (itself, or the one a CanonicalSpecWrapper wraps)."""
    from robopianist_amd.wrappers.canonical import CanonicalSpecWrapper
    if isinstance(env, CanonicalSpecWrapper):
        env = env._environment
    if not hasattr(env, "step_canonical"):
        raise ValueError("PPO needs a batched Environment (or a CanonicalSpecWrapper around one): "
                         f"{type(env).__name__} has no step_canonical")
    return env


class DeviceLearner:
    """What the learners (`PPO`, offpolicy's `SAC`) share: the environment and its specs, the packing of a TimeStep into
    a slot of the learner's storage, the running episode statistics, the observation normaliser and the evaluation slot.
    A subclass allocates the storage the pack writes (`_obs`, `_reward`, `_discount`, `_step_type`, indexed by slot) and
    builds its networks: two tanh layers of `hidden` units, which the kernels read in place.  A subclass's constructor
    calls `__init__`, checks its own storage sizes, then calls `_init_specs`."""

    _reads = "the kernels read"   # (how `_mlp`'s error names the reader)

    def __init__(self, env):
        import torch
        self._env = base = _unwrap(env)
        phys = base.physics
        self._dev, self._dtype = torch.device(phys.device), phys.dtype
        self._precision = 32 if phys.dtype == torch.float32 else 64
        self.E = int(base.n_envs)

    def _init_specs(self, hidden, obs_clip, seed, norm_eps):
        """The spec validation, D, A, H1, H2 and the action bounds; the buffers every learner has."""
        import torch
        base = self._env
        ospec = base.observation_spec()
        self._keys = sorted(ospec)
        self._widths = [int(np.prod(ospec[k].shape, dtype=np.int64)) for k in self._keys]
        if not 1 <= len(self._keys) <= MAX_FIELDS or min(self._widths) < 1:
            raise ValueError(f"{type(self).__name__} packs 1 .. {MAX_FIELDS} non-empty observation tensors, the spec has "
                             f"{len(self._keys)}")
        self.D = int(sum(self._widths))
        aspec = base.action_spec()
        self.A = int(aspec.shape[0])
        self.H1, self.H2 = (int(h) for h in hidden)
        for h in (self.H1, self.H2):
            if h < 16 or h > MAX_HIDDEN or h % 16:
                raise ValueError(f"hidden sizes must be multiples of 16 in [16, {MAX_HIDDEN}], got {tuple(hidden)}")
        if not 1 <= self.A <= MAX_ACTIONS:
            raise ValueError(f"the action has {self.A} entries, the policy kernel takes 1 .. {MAX_ACTIONS}")
        lo = np.asarray(aspec.minimum, np.float64)
        rng = np.asarray(aspec.maximum, np.float64) - lo
        self._bounds = (torch.as_tensor(lo, device=self._dev, dtype=self._dtype),
                        torch.as_tensor(rng, device=self._dev, dtype=self._dtype))
        self.obs_clip, self.norm_eps = float(obs_clip), float(norm_eps)
        self.seed, self._round = int(seed), 0
        E, D, A, z = self.E, self.D, self.A, self._zeros
        self._ep_return, self._ep_len = z(E, dtype=torch.float64), z(E, dtype=torch.int32)
        self._done_return, self._done_len = z(E, dtype=torch.float64), z(E, dtype=torch.int64)
        self._done_count = z(E, dtype=torch.int32)
        # evaluation scratch (`act`): one slot of its own, no statistics
        self._e_obs, self._e_reward, self._e_discount = z(E, D), z(E), z(E)
        self._e_step_type, self._e_action, self._e_logp = z(E, dtype=torch.int32), z(E, A), z(E)
        self._e_env_action = z(E, A, dtype=self._dtype)
        # the normaliser
        self._count = 0.0
        self._mean, self._M2 = z(D, dtype=torch.float64), z(D, dtype=torch.float64)
        self._mean_f32, self._inv_std_f32 = z(D), torch.ones(D, dtype=torch.float32, device=self._dev)
        self._keep = None

    def _zeros(self, *shape, dtype=None):
        import torch
        return torch.zeros(shape, dtype=torch.float32 if dtype is None else dtype, device=self._dev)

    def _net(self, n_in, n_out):
        """A network as the kernels take it (on the CPU; drawn from torch's global generator)."""
        from torch import nn
        return nn.Sequential(nn.Linear(n_in, self.H1), nn.Tanh(), nn.Linear(self.H1, self.H2), nn.Tanh(),
                             nn.Linear(self.H2, n_out))

    # -- accessors ---------------------------------------------------------------------------------------------------
    @property
    def env(self):
        return self._env

    @property
    def observation_keys(self):
        """The packed observation tensors, in column order."""
        return list(self._keys)

    @property
    def normalizer(self):
        """(count, mean [D] f64, M2 [D] f64, mean_f32 [D], inv_std_f32 [D]) -- live."""
        return self._count, self._mean, self._M2, self._mean_f32, self._inv_std_f32

    def _stream(self):
        import torch
        if self._dev.type != "cuda":
            raise LearnError("the learner's kernels need a HIP device; there is no CPU fallback")
        return torch.cuda.current_stream(self._dev).cuda_stream

    def _mlp(self, net):
        """`net` as rp_learn_mlp: the addresses of the parameters as they are now."""
        for layer in (net[0], net[2], net[4]):
            if not (layer.weight.is_contiguous() and layer.bias.is_contiguous()):
                raise LearnError(f"{self._reads} contiguous float32 parameters")
        return mlp_table([t for i in (0, 2, 4) for t in (net[i].weight, net[i].bias)])

    def _table(self, observation):
        import torch
        fields = []
        for k, w in zip(self._keys, self._widths):
            t = observation[k]
            if t.dtype not in (torch.float32, torch.float64):
                raise LearnError(f"observation {k!r} is {t.dtype}: pack takes float32 and float64")
            if t.shape[0] != self.E or t.numel() != self.E * w or not t.is_contiguous() or t.device != self._dev:
                raise LearnError(f"observation {k!r}: expected a contiguous [{self.E}, {w}] device tensor, got "
                                 f"{tuple(t.shape)}")
            fields.append((t.data_ptr(), w, F32 if t.dtype == torch.float32 else F64))
        return field_table(fields)

    def _pack(self, ts, slot, st):
        import torch
        for name, t in (("reward", ts.reward), ("discount", ts.discount)):
            if t is not None and (t.dtype != self._dtype or not t.is_contiguous()):
                raise LearnError(f"the TimeStep's {name} must be a contiguous tensor of the engine's dtype")
        if ts.step_type.dtype != torch.int32:
            raise LearnError("the TimeStep's step_type must be int32")
        pack(self._table(ts.observation), self._precision, ts.step_type.data_ptr(),
             None if ts.reward is None else ts.reward.data_ptr(), None if ts.discount is None else ts.discount.data_ptr(),
             self._obs[slot].data_ptr(), self._reward[slot].data_ptr(), self._discount[slot].data_ptr(),
             self._step_type[slot].data_ptr(), self.E, self.D,
             stats=(self._ep_return.data_ptr(), self._ep_len.data_ptr(), self._done_return.data_ptr(),
                    self._done_len.data_ptr(), self._done_count.data_ptr()), hip_stream=st)

    def _pack_observation(self, observation, st):
        """The first half of `act()`: an observation dict of E rows into the evaluation slot (`_e_obs`)."""
        self._e_step_type.fill_(STEP_MID)
        pack(self._table(observation), self._precision, self._e_step_type.data_ptr(), None, None,
             self._e_obs.data_ptr(), self._e_reward.data_ptr(), self._e_discount.data_ptr(),
             self._e_step_type.data_ptr(), self.E, self.D, hip_stream=st)
        self._keep = observation   # alive until the pack has run (a rollout's TimeSteps have been consumed by then)

    def _merge_moments(self, obs, n_rows, st):
        """The `n_rows` rows from `obs` on into the running moments (one launch)."""
        moments(obs.data_ptr(), self._mean.data_ptr(), self._M2.data_ptr(), self._mean_f32.data_ptr(),
                self._inv_std_f32.data_ptr(), self._count, self.norm_eps, n_rows, self.D, hip_stream=st)
        self._count += float(n_rows)

    def normalize(self, obs):
        """What the kernels feed the first layer (torch, float32)."""
        import torch
        return torch.clamp((obs - self._mean_f32) * self._inv_std_f32, -self.obs_clip, self.obs_clip)

    def episode_stats(self):
        """{"episodes", "mean_return", "mean_length"} of the episodes that ended since the last call (one read-back);
        the counters start again from zero."""
        n = int(self._done_count.sum())
        out = {"episodes": n,
               "mean_return": float(self._done_return.sum()) / n if n else float("nan"),
               "mean_length": float(self._done_len.sum()) / n if n else float("nan")}
        self._done_return.zero_(); self._done_len.zero_(); self._done_count.zero_()
        return out

    # -- the blocks of a checkpoint that every learner has ---------------------------------------------------------------
    def _normalizer_state(self):
        c = lambda t: t.detach().clone()
        return {"count": self._count, "mean": c(self._mean), "M2": c(self._M2), "mean_f32": c(self._mean_f32),
                "inv_std_f32": c(self._inv_std_f32)}

    def _episodes_state(self):
        return {k: getattr(self, "_" + k).detach().clone()
                for k in ("ep_return", "ep_len", "done_return", "done_len", "done_count")}

    def _load_shared_state(self, sd):
        """The "normalizer" and "episodes" blocks of `sd`."""
        nz = sd["normalizer"]
        self._count = float(nz["count"])
        for dst, key in ((self._mean, "mean"), (self._M2, "M2"), (self._mean_f32, "mean_f32"),
                         (self._inv_std_f32, "inv_std_f32")):
            dst.copy_(nz[key])
        for key, v in sd["episodes"].items():
            getattr(self, "_" + key).copy_(v)


class PPO(DeviceLearner):
    """Proximal policy optimisation (Schulman et al. 2017) with a diagonal Gaussian policy, over every env of `env` at
    once.  `env` is a batched `Environment` or a `CanonicalSpecWrapper` around one: the policy acts in [-1, 1]^A, the
    raw action is what is stored and scored, its clamp to [-1, 1] is what `step_canonical` receives.

    The actor and the critic are `torch.nn.Sequential`s with two tanh layers of `hidden` units; the kernels read their
    weights in place, so Adam's updates need no copy.  Observations are the spec's tensors in sorted key order,
    normalised by running moments (clamped to +-`obs_clip`); the normaliser learns in `train()` after each update, so
    `collect()` alone never changes it.

    `collect()` launches, on torch's current stream and without reading anything back, T x (act, env step, pack), the
    critic at slot T and gae.  The first call resets the env; later ones continue from the last TimeStep."""

    _reads = "the policy kernel reads"

    def __init__(self, env, hidden=(256, 256), horizon: int = 16, epochs: int = 4, minibatches: int = 4,
                 gamma: float = 0.99, lam: float = 0.95, clip: float = 0.2, lr: float = 3e-4, vf_coef: float = 0.5,
                 ent_coef: float = 0.0, max_grad_norm: float = 0.5, obs_clip: float = 10.0, seed: int = 0,
                 init_log_std: float = -0.5, norm_eps: float = 1e-8):
        import torch
        from torch import nn
        super().__init__(env)
        self.T = int(horizon)
        if self.T < 1:
            raise ValueError("horizon must be >= 1")
        self._init_specs(hidden, obs_clip, seed, norm_eps)
        self.epochs, self.minibatches = int(epochs), int(minibatches)
        self.gamma, self.lam, self.clip = float(gamma), float(lam), float(clip)
        self.vf_coef, self.ent_coef, self.max_grad_norm = float(vf_coef), float(ent_coef), float(max_grad_norm)

        def mlp(n_out, last_gain):
            net = self._net(self.D, n_out)
            with torch.no_grad():
                net[4].weight.mul_(last_gain)
                net[4].bias.zero_()
            return net

        with torch.random.fork_rng(devices=[]):   # (the global generator is left as it was)
            torch.manual_seed(self.seed)
            self.actor, self.critic = mlp(self.A, 0.01), mlp(1, 1.0)
        self.actor.to(self._dev); self.critic.to(self._dev)
        self.log_std = nn.Parameter(torch.full((self.A,), float(init_log_std), device=self._dev))
        self.optimizer = torch.optim.Adam(list(self.actor.parameters()) + list(self.critic.parameters()) + [self.log_std],
                                          lr=float(lr), eps=1e-5)
        T, E, D, A, z = self.T, self.E, self.D, self.A, self._zeros
        self._obs, self._reward, self._discount = z(T + 1, E, D), z(T + 1, E), z(T + 1, E)
        self._step_type = z(T + 1, E, dtype=torch.int32)
        self._action, self._logp, self._value = z(T, E, A), z(T, E), z(T + 1, E)
        self._env_action = z(T, E, A, dtype=self._dtype)
        self._adv, self._ret, self._valid = z(T, E), z(T, E), z(T, E, dtype=torch.uint8)
        self._started = False

    # -- the rollout -------------------------------------------------------------------------------------------------
    def rollout(self):
        """The storage as a dict of views (live)."""
        return {"obs": self._obs, "reward": self._reward, "discount": self._discount, "step_type": self._step_type,
                "action": self._action, "env_action": self._env_action, "logp": self._logp, "value": self._value,
                "adv": self._adv, "ret": self._ret, "valid": self._valid}

    def collect(self):
        """Fills the storage with the next T control steps of every env; returns `rollout()`."""
        import torch
        T, E, D, A = self.T, self.E, self.D, self.A
        with torch.cuda.device(self._dev):
            st = self._stream()
            actor, critic = self._mlp(self.actor), self._mlp(self.critic)
            kept = []
            if self._started:
                for buf in (self._obs, self._reward, self._discount, self._step_type, self._value):
                    buf[0].copy_(buf[T])
            else:
                ts = self._env.reset()
                self._pack(ts, 0, st)
                kept.append(ts)
                self._started = True
            common = dict(mean=self._mean_f32.data_ptr(), inv_std=self._inv_std_f32.data_ptr(), obs_clip=self.obs_clip,
                          D=D, H1=self.H1, H2=self.H2, A=A, n_rows=E, hip_stream=st)
            for t in range(T):
                act(self._obs[t].data_ptr(), actor=actor, critic=critic, log_std=self.log_std.data_ptr(),
                    action=self._action[t].data_ptr(), logp=self._logp[t].data_ptr(),
                    env_action=self._env_action[t].data_ptr(), value=self._value[t].data_ptr(),
                    precision=self._precision, seed=self.seed, round_=self._round, **common)
                self._round += 1
                ts = self._env.step_canonical(self._env_action[t], self._bounds, False)
                self._pack(ts, t + 1, st)
                kept.append(ts)
            act(self._obs[T].data_ptr(), actor=None, critic=critic, value=self._value[T].data_ptr(), **common)
            gae(self._reward.data_ptr(), self._discount.data_ptr(), self._step_type.data_ptr(), self._value.data_ptr(),
                self._adv.data_ptr(), self._ret.data_ptr(), self._valid.data_ptr(), self.gamma, self.lam, T, E,
                hip_stream=st)
            self._keep = kept   # alive until the kernels have run
        return self.rollout()

    def update_normalizer(self):
        """Merges the observations of slots 0 .. T - 1 of the storage into the running moments (one launch)."""
        import torch
        with torch.cuda.device(self._dev):
            self._merge_moments(self._obs, self.T * self.E, self._stream())

    # -- the gradient step ---------------------------------------------------------------------------------------------
    def update(self, rollout=None):
        """`epochs` passes of `minibatches` Adam steps over the valid rows of `rollout` (default: the storage).  Plain
        torch on the rollout's device.  Returns the statistics of the last minibatch and the batch size, as floats."""
        import torch
        r = self.rollout() if rollout is None else rollout
        T = r["action"].shape[0]
        rows = r["valid"].reshape(-1).bool().nonzero().squeeze(1)
        n = int(rows.numel())
        if n == 0:
            return {"batch": 0}
        flat = lambda x: x[:T].reshape(T * x.shape[1], *x.shape[2:])[rows]
        obs = self.normalize(flat(r["obs"]))
        action, logp_old, ret = flat(r["action"]), flat(r["logp"]), flat(r["ret"])
        adv = flat(r["adv"])
        adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
        params = list(self.actor.parameters()) + list(self.critic.parameters()) + [self.log_std]
        mb = max(1, min(self.minibatches, n))
        stats = {}
        for _ in range(self.epochs):
            perm = torch.randperm(n, device=obs.device)
            for part in perm.tensor_split(mb):
                loss, stats = ppo_loss(self.actor(obs[part]), self.log_std, self.critic(obs[part]).squeeze(-1),
                                       action[part], logp_old[part], adv[part], ret[part], self.clip, self.vf_coef,
                                       self.ent_coef)
                self.optimizer.zero_grad(set_to_none=True)
                loss.backward()
                if self.max_grad_norm > 0:
                    torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm)
                self.optimizer.step()
        out = {k: float(v) for k, v in stats.items()}
        out["batch"] = n
        return out

    def train(self, n: int, callback=None):
        """n rounds of collect, update and normaliser merge; returns the list of per-round statistics (the update's,
        plus "mean_reward": the mean reward of the rollout's transitions, and `episode_stats()`)."""
        log = []
        for i in range(int(n)):
            r = self.collect()
            s = self.update(r)
            self.update_normalizer()
            valid = r["valid"].bool()
            s["mean_reward"] = float(r["reward"][1:][valid].mean()) if bool(valid.any()) else float("nan")
            s.update(self.episode_stats())
            log.append(s)
            if callback is not None:
                callback(i, s)
        return log

    # -- evaluation ----------------------------------------------------------------------------------------------------
    def act(self, observation, deterministic: bool = True):
        """The policy's action for an observation dict of E rows: [E, A] of the engine's dtype, clamped to [-1, 1] (what
        a CanonicalSpecWrapper's step takes).  Live: the next call overwrites it."""
        import torch
        with torch.cuda.device(self._dev):
            st = self._stream()
            self._pack_observation(observation, st)
            act(self._e_obs.data_ptr(), self._mean_f32.data_ptr(), self._inv_std_f32.data_ptr(), self.obs_clip,
                self._mlp(self.actor), None, self.D, self.H1, self.H2, self.A, self.E, log_std=self.log_std.data_ptr(),
                action=self._e_action.data_ptr(), logp=self._e_logp.data_ptr(), env_action=self._e_env_action.data_ptr(),
                precision=self._precision, deterministic=deterministic, seed=self.seed, round_=self._round, hip_stream=st)
            if not deterministic:
                self._round += 1
        return self._e_env_action

    # -- checkpoint / resume -------------------------------------------------------------------------------------------
    def state_dict(self):
        """The networks, Adam, the normaliser, the seed and round counters, the running episode statistics and the
        TimeStep the next `collect()` starts from.  With the env's own `state_dict()` the next rollout is resumed bit
        for bit."""
        c = lambda t: t.detach().clone()
        T = self.T
        return {"actor": {k: c(v) for k, v in self.actor.state_dict().items()},
                "critic": {k: c(v) for k, v in self.critic.state_dict().items()},
                "log_std": c(self.log_std), "optimizer": copy.deepcopy(self.optimizer.state_dict()),
                "normalizer": self._normalizer_state(),
                "seed": self.seed, "round": self._round, "started": self._started,
                "last": {"obs": c(self._obs[T]), "reward": c(self._reward[T]), "discount": c(self._discount[T]),
                         "step_type": c(self._step_type[T]), "value": c(self._value[T])},
                "episodes": self._episodes_state()}

    def load_state_dict(self, sd):
        import torch
        self.actor.load_state_dict(sd["actor"]); self.critic.load_state_dict(sd["critic"])   # (in place)
        with torch.no_grad():
            self.log_std.copy_(sd["log_std"])
        self.optimizer.load_state_dict(sd["optimizer"])
        self._load_shared_state(sd)
        self.seed, self._round, self._started = int(sd["seed"]), int(sd["round"]), bool(sd["started"])
        T = self.T
        for buf, key in ((self._obs, "obs"), (self._reward, "reward"), (self._discount, "discount"),
                         (self._step_type, "step_type"), (self._value, "value")):
            buf[T].copy_(sd["last"][key])


def _train_and_evaluate(learner, rounds, train_one, shown, time_limit, log, line=None, metrics=None):
    """What every `train_and_evaluate` does: `rounds` calls of `train_one(callback)` (one round of training each), one line
    per round with the mean return of the episodes that ended in it and the statistic `shown` = (label, key), then one
    deterministic episode of every env through a MidiEvaluationWrapper.  Returns (log of the rounds, metrics).  A learner
    whose statistics are no floats states its own `line(i, s, seconds)` and `metrics(evaluated, log)`."""
    import time
    import torch
    from robopianist_amd.wrappers import CanonicalSpecWrapper, MidiEvaluationWrapper
    t0 = time.perf_counter()
    rounds_log = []
    last_mean = [float("nan")]

    def mean_return_line(i, s, seconds):
        if s["episodes"]:
            last_mean[0] = s["mean_return"]
        # (a round in which no episode ended shows the mean of the last round in which some did)
        return (f"update {i + 1:4d}  episodes {s['episodes']:6d}  mean return {last_mean[0]:10.4f}  "
                f"mean reward {s['mean_reward']:8.4f}  {shown[0]} {s.get(shown[1], float('nan')):8.5f}  {seconds:7.1f} s")

    def report(i, s):
        rounds_log.append(s)
        log((line or mean_return_line)(i, s, time.perf_counter() - t0))

    for i in range(int(rounds)):
        train_one(lambda _, s, i=i: report(i, s))
        if time_limit is not None and time.perf_counter() - t0 > time_limit:
            log(f"stopped after {i + 1} updates: the time limit of {time_limit:.0f} s")
            break
    evaluated = CanonicalSpecWrapper(MidiEvaluationWrapper(learner.env))
    ts = evaluated.reset()
    done = torch.zeros(learner.E, dtype=torch.bool, device=ts.step_type.device)
    for _ in range(100000):
        ts = evaluated.step(learner.act(ts.observation, deterministic=True))
        done |= ts.last()
        if bool(done.all()):
            break
    if metrics is not None:
        return rounds_log, metrics(evaluated, log)
    found = evaluated.get_musical_metrics()
    for k, v in found.items():
        log(f"\t{k}: {v:.4f}")
    return rounds_log, found


def train_and_evaluate(env, updates: int, time_limit: float = None, log=print, **ppo_kwargs):
    """What the examples' --train-ppo does: `updates` rounds of PPO on `env` (a batched Environment), one line per
    round with the mean return of the episodes that ended in it, then one deterministic episode of every env through a
    MidiEvaluationWrapper.  Stops early after `time_limit` seconds.  Returns (ppo, log of the rounds, metrics)."""
    ppo = PPO(env, **ppo_kwargs)
    rounds, metrics = _train_and_evaluate(ppo, updates, lambda cb: ppo.train(1, callback=cb), ("kl", "approx_kl"),
                                          time_limit, log)
    return ppo, rounds, metrics
