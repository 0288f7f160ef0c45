"""The cases of the fused actor step's tests, shared by the host tests (which check their conditioning where no GPU is
needed) and the GPU tests (which run the kernels on them): the inputs, the float64 twin, the float32 restatement and two
more float32 restatements in other summation orders, computed once per (case, mode, number of critics).  Unlike a critic's
step, the actor's depends on how many critics the launch holds (the minimum runs over all of them), so every number of
critics has a reference of its own.

A case is (rows, D, H1, H2, A, p): critic_cases.ALL_CASES (droq_cases.ALL_CASES plus the one of 70 rows).  Every fourth
row has mask 0.  The actor is drawn as nn.Linear draws it; the log-std half of its head is then spread over the clamp's
three kinds: that half of b3 is drawn uniformly over [log_std_min - 3.5, log_std_max + 3.5] (twice the clamp's width) and that
half of w3 is multiplied by 8, so
that an entry's l moves by a few units from row to row (with A = 1 the kinds can only differ by row) and about a third of
the entries each lie below, inside and above.  The modes: "on" (dropout p) and "off" (drop_threshold 0, keep_scale 1)
start from non-trivial m and v, the actor at Adam's step 3 and the temperature at its step 5 with another learning rate;
"first" (FIRST_CASE only, dropout on) is step 1 of both from zero m and v.  Scalars reach the twin as the float32 values
the argument block carries.

The seeds.  Many outputs are single numbers (the statistics, log_alpha and its m and v), whose float32 error is a draw,
not a level, and the step has switches (the minimum's selection, the clamp, the critics' ReLU) that a rounding can flip.  A
seed is therefore taken only if, for every mode, every number of critics the GPU tests run and every output, two
restatements in two other summation orders each lie within 4 times the first one's error (which rejects a seed where a
switch sits within rounding of flipping: a flip is an error of another magnitude), if, without dropout, so does torch's own
float32 step on the CPU (the reference of the dropout-off GPU test, which has an error of its own: its masked mean
multiplies and divides in another order), and if the case shows what it is for:
clamped-low, clamped-high and inside entries all occur, masked and unmasked rows occur, and with at least 17 rows each
critic in use is the selected one on some row.  All of this is checked on the CPU by test_actor_host.py, which asserts it;
each seed is the first from 0 that passes (`first_seed`).
"""

from __future__ import annotations

import functools
import types

import numpy as np
import torch

import actor_reference as ar
import critic_cases as cc
import critic_reference as cr
import droq_cases as dc
import droq_reference as dr

CASES = list(cc.CASES)
WIDE_CASES = list(cc.WIDE_CASES)
ALL_CASES = CASES + WIDE_CASES
FIRST_CASE = CASES[1]
# chosen once, on the CPU, by first_seed (the rule above; test_actor_host asserts it); nothing a kernel computed
SEEDS = {CASES[0]: 4357, CASES[1]: 6, CASES[2]: 2, CASES[3]: 3, CASES[4]: 13,
         WIDE_CASES[0]: 54, WIDE_CASES[1]: 5, WIDE_CASES[2]: 274, WIDE_CASES[3]: 12}
N_CRITICS = (1, 2, 3, 4)
WIDE_N_CRITICS = (1, 4)
SEED, ROUND = (9 << 32) | 17, 5
LN_EPS, CLIP, EPS, BETAS = cc.LN_EPS, cc.CLIP, cc.EPS, cc.BETAS
LR, ALPHA_LR, T_ACTOR, T_ALPHA = 1e-2, 3e-3, 3, 5
LOG_STD_BOUNDS, LOG_ALPHA = (-5.0, 2.0), np.float32(-0.7)
KINDS = ("grad", "p", "m", "v")
f32, case_id = cc.f32, cc.case_id


def n_critics(case):
    return N_CRITICS if case in CASES else WIDE_N_CRITICS


def modes(case):
    return ("on", "off", "first") if case == FIRST_CASE else ("on", "off")


def adam_scalars(lr_, t):
    """Adam's scalars of step t as the argument block carries them (float32 values)."""
    return dict(step_size=f32(lr_ / (1.0 - BETAS[0] ** t)), bc2_sqrt=f32(np.sqrt(1.0 - BETAS[1] ** t)), eps=f32(EPS),
                omb1=f32(1.0 - BETAS[0]), beta2=f32(BETAS[1]), omb2=f32(1.0 - BETAS[1]))


def keys():
    return ("action", "logp", "q_min") + tuple(f"{kind}.{name}" for kind in KINDS for name in ar.PARAMS) + \
        tuple(f"log_alpha.{kind}" for kind in KINDS) + tuple(f"stats.{name}" for name in ar.STATS)


def flat(out):
    """Every output under a key of its own."""
    d = {k: out[k] for k in ("action", "logp", "q_min")}
    for kind in KINDS:
        d.update({f"{kind}.{name}": x for name, x in zip(ar.PARAMS, out[kind])})
        d[f"log_alpha.{kind}"] = out["log_alpha"][kind]
    d.update({f"stats.{name}": out["stats"][i:i + 1] for i, name in enumerate(ar.STATS)})
    return d


def errors(a, ref):
    return {k: float(np.abs(np.asarray(a[k], np.float64) - ref[k]).max()) for k in ref}


def actor_net(D, H1, H2, A, seed):
    """The actor, drawn as nn.Linear draws it, the log-std half of its head spread over the clamp's three kinds."""
    from torch import nn
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = nn.Sequential(nn.Linear(D, H1), nn.Tanh(), nn.Linear(H1, H2), nn.Tanh(), nn.Linear(H2, 2 * A))
        with torch.no_grad():
            net[4].weight[A:] *= 8.0
            net[4].bias[A:].uniform_(LOG_STD_BOUNDS[0] - 3.5, LOG_STD_BOUNDS[1] + 3.5)
    return net


def actor_params(net):
    return [t for i in (0, 2, 4) for t in (net[i].weight, net[i].bias)]


def actor_host(net):
    return [t.detach().cpu().numpy() for t in actor_params(net)]


class Problem(types.SimpleNamespace):
    """kw: the inputs all modes share (with all four critics); mode: what a mode adds.  run(mode, n, **o): the flat twin."""

    def twin_kw(self, mode, n, **override):
        kw = dict(self.kw, **self.mode[mode])
        kw.update(override)
        kw["critics"] = kw["critics"][:n]
        return kw

    def raw(self, mode, n, **o):
        return ar.step(**self.twin_kw(mode, n), **o)

    def run(self, mode, n, **o):
        return flat(self.raw(mode, n, **o))

    def _once(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def ref_raw(self, mode, n):
        return self._once(("ref", mode, n), lambda: self.raw(mode, n, dtype=np.float64))

    def ref(self, mode, n):
        return flat(self.ref_raw(mode, n))

    def err32(self, mode, n):
        return self._once(("err32", mode, n), lambda: errors(self.run(mode, n, dtype=np.float32), self.ref(mode, n)))

    def err_perm(self, mode, n, which):
        return self._once(("perm", mode, n, which),
                          lambda: errors(self.run(mode, n, dtype=np.float32, permute=self.seed + which), self.ref(mode, n)))

    __hash__ = object.__hash__


@functools.lru_cache(maxsize=None)
def problem(case, seed=None):
    rows, D, H1, H2, A, p = case
    seed = SEEDS[case] if seed is None else seed
    rng = np.random.default_rng(9000 * seed + rows + D)
    critics = [dc.critic_net(D + A, H1, H2, p, 100 * seed + 10 + i + rows) for i in range(max(N_CRITICS))]
    actor = actor_net(D, H1, H2, A, 100 * seed + 70 + rows)
    mean = rng.normal(size=D).astype(np.float32)
    inv_std = (1.0 / rng.uniform(0.5, 2.0, D)).astype(np.float32)
    obs = (mean + rng.normal(size=(rows, D)) * 2.0).astype(np.float32)
    obs.reshape(-1)[5::11] += 40.0                                    # every eleventh normalised entry clips at 5
    host = actor_host(actor)
    kw = dict(obs=obs, mask=(np.arange(rows) % 4 != 2).astype(np.float32), mean=mean, inv_std=inv_std, clip=CLIP, actor=host,
              critics=[dc.host(c) for c in critics], log_alpha=LOG_ALPHA, target_entropy=f32(-A),
              log_std_bounds=LOG_STD_BOUNDS, ln_eps=f32(LN_EPS), seed=SEED, round_=ROUND)
    m3 = [(rng.normal(size=a.shape) * 1e-2).astype(np.float32) for a in host]
    v3 = [(rng.uniform(0.5, 1.5, size=a.shape) * 1e-4).astype(np.float32) for a in host]
    zero = [np.zeros_like(a) for a in host]
    la_m, la_v = np.float32(rng.normal() * 1e-2), np.float32(rng.uniform(0.5, 1.5) * 1e-4)
    on = dict(threshold=dr.drop_threshold(p), keep_scale=f32(1.0 / (1.0 - p)))
    later = dict(m=m3, v=v3, log_alpha_m=la_m, log_alpha_v=la_v, actor_adam=adam_scalars(LR, T_ACTOR),
                 alpha_adam=adam_scalars(ALPHA_LR, T_ALPHA))
    mode = {"on": dict(on, **later), "off": dict(threshold=0, keep_scale=1.0, **later),
            "first": dict(on, m=zero, v=zero, log_alpha_m=np.float32(0), log_alpha_v=np.float32(0),
                          actor_adam=adam_scalars(LR, 1), alpha_adam=adam_scalars(ALPHA_LR, 1))}
    return Problem(case=case, seed=seed, cache={}, actor=actor, critics=critics, kw=kw, mode=mode,
                   t={"on": (T_ACTOR, T_ALPHA), "off": (T_ACTOR, T_ALPHA), "first": (1, 1)})


def shows_what_it_is_for(p):
    """The second half of the seeds' rule: "" if the case shows the clamp's three kinds, masked and unmasked rows, and
    (with at least 17 rows) every critic in use as the selected one; else what is missing."""
    rows = p.case[0]
    mk = p.kw["mask"]
    if not ((mk == 0).any() and (mk == 1).any()):
        return "masked and unmasked rows"
    for mode in modes(p.case):
        for n in n_critics(p.case):
            ref = p.ref_raw(mode, n)
            l, lo, hi = ref["head_l"], *LOG_STD_BOUNDS
            if not ((l <= lo).any() and (l >= hi).any() and ref["inside"].any()):
                return f"the clamp's three kinds ({mode}, {n} critics)"
            if rows >= 17 and set(ref["best"]) != set(range(n)):
                return f"every critic selected on some row ({mode}, {n} critics)"
    return ""


def conditioning(p, stop=True):
    """The first half of the seeds' rule: the worst ratio of a permuted restatement's error to the first one's over every
    mode, number of critics and output (stop: return inf at the first ratio over 4)."""
    worst = 0.0
    for mode in modes(p.case):
        for n in n_critics(p.case):
            e32 = p.err32(mode, n)
            for which in (1, 2):
                ep = p.err_perm(mode, n, which)
                for k, e in e32.items():
                    if ep[k] > 4 * e:
                        if stop:
                            return np.inf
                        worst = np.inf
                    elif e > 0:
                        worst = max(worst, ep[k] / e)
    return worst


def torch_n_critics(case):
    """The numbers of critics of the comparison with torch's own float32 step (without dropout)."""
    return (1, 3) if case in CASES else WIDE_N_CRITICS


def torch_conditioning(p):
    """The worst ratio of the error of torch's own float32 step on the CPU (one thread), without dropout and with the
    twin's noise injected, to the first restatement's, over torch_n_critics and every output."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        worst = 0.0
        for n in torch_n_critics(p.case):
            et = errors(torch_step(p, "off", n, "cpu", torch.float32, noise=p.ref_raw("off", n)["noise"]), p.ref("off", n))
            for k, e in p.err32("off", n).items():
                worst = max(worst, et[k] / e if e > 0 else (np.inf if et[k] > 0 else 0.0))
        return worst
    finally:
        torch.set_num_threads(threads)


def passes(case, seed):
    p = problem(case, seed)
    ok = not shows_what_it_is_for(p) and conditioning(p) <= 4 and torch_conditioning(p) <= 4
    if not ok:
        problem.cache_clear()
    return ok


def first_seed(case, limit=100000):
    """The first seed from 0 that passes the rule."""
    for seed in range(limit):
        if passes(case, seed):
            return seed
    raise RuntimeError(f"no seed below {limit} passes for {case}")


def torch_step(p, mode, n, device="cpu", dtype=torch.float64, masks=None, noise=None):
    """The step of the first n critics of problem p by torch in `dtype` on `device`: the twin's noise and dropout masks
    (`noise`, `masks` as ar.step returns them; masks None: no dropout) injected, autograd on offpolicy.squashed_gaussian,
    actor_loss and alpha_loss, torch.optim.Adam from the mode's m, v and step counts.  -> the flat dict."""
    import copy
    import torch.nn.functional as F
    from robopianist_amd import offpolicy
    md, kw = p.mode[mode], p.kw
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device).to(dtype)
    A = p.case[4]
    actor = copy.deepcopy(p.actor).to(device).to(dtype)
    critics = [copy.deepcopy(c).to(device).to(dtype) for c in p.critics[:n]]
    log_alpha = up(np.asarray(kw["log_alpha"]).reshape(1)).requires_grad_(True)
    params = actor_params(actor)
    t_actor, t_alpha = p.t[mode]
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS)
    opt_a = torch.optim.Adam([log_alpha], lr=ALPHA_LR, betas=BETAS, eps=EPS)
    if t_actor > 1:
        for t, m, v in zip(params, md["m"], md["v"]):
            opt.state[t] = {"step": torch.tensor(float(t_actor - 1)), "exp_avg": up(m.copy()), "exp_avg_sq": up(v.copy())}
        opt_a.state[log_alpha] = {"step": torch.tensor(float(t_alpha - 1)), "exp_avg": up(np.asarray(md["log_alpha_m"]).reshape(1)),
                                  "exp_avg_sq": up(np.asarray(md["log_alpha_v"]).reshape(1))}
    mask = up(kw["mask"])
    xn = torch.clamp((up(kw["obs"]) - up(kw["mean"])) * up(kw["inv_std"]), -CLIP, CLIP)
    a_new, logp, _ = offpolicy.squashed_gaussian(actor(xn), up(noise), LOG_STD_BOUNDS)
    x = torch.cat([xn, a_new], dim=1)
    qs = []
    for i, net in enumerate(critics):
        h = x
        for L, (lin, ln) in enumerate(((0, 2), (4, 6))):
            h = net[lin](h)
            if masks is not None:
                h = h * up(masks[i][L].astype(np.float64)) * float(md["keep_scale"])
            h = torch.relu(F.layer_norm(h, (h.shape[1],), net[ln].weight, net[ln].bias, float(kw["ln_eps"])))
        qs.append(net[8](h)[:, 0])
    q_new = torch.stack(qs).min(0).values
    la = offpolicy.actor_loss(log_alpha, logp, q_new, mask)
    opt.zero_grad(set_to_none=True)
    la.backward()
    grads = [t.grad.clone() for t in params]
    opt.step()
    before = log_alpha.detach().clone()
    lt = offpolicy.alpha_loss(log_alpha, logp, float(kw["target_entropy"]), mask)
    opt_a.zero_grad(set_to_none=True)
    lt.backward()
    ga = log_alpha.grad.clone()
    opt_a.step()
    del before
    h_ = lambda t: t.detach().cpu().numpy()
    out = {"action": h_(a_new), "logp": h_(logp), "q_min": h_(q_new), "log_alpha.grad": h_(ga), "log_alpha.p": h_(log_alpha),
           "log_alpha.m": h_(opt_a.state[log_alpha]["exp_avg"]), "log_alpha.v": h_(opt_a.state[log_alpha]["exp_avg_sq"])}
    for k, name in enumerate(ar.PARAMS):
        t = params[k]
        out.update({f"grad.{name}": h_(grads[k]), f"p.{name}": h_(t), f"m.{name}": h_(opt.state[t]["exp_avg"]),
                    f"v.{name}": h_(opt.state[t]["exp_avg_sq"])})
    stats = [la, lt, log_alpha.detach().exp()[0], -offpolicy._masked_mean(logp.detach(), mask), 1.0 - mask.mean()]
    out.update({f"stats.{name}": np.asarray(h_(torch.as_tensor(s))).reshape(1) for name, s in zip(ar.STATS, stats)})
    return out
