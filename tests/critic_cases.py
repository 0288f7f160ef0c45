"""The cases of the fused critic step's tests, shared by the host tests (which check their conditioning where no GPU is
needed) and the GPU tests (which run the kernels on them): the inputs, the float64 twin, the float32 restatement and a
second float32 restatement in another summation order, computed once per case for four critics.  Critic i's step does
not depend on how many critics the launch holds, so n critics' reference is the first n of the four.

A case is (rows, D, H1, H2, A, p): droq_cases.CASES, plus one whose 70 rows exceed two stages (32 rows each) of the apply
launch's reduction by 6, which is no multiple of 16, and whose last row tile holds 6 rows.  WIDE_CASES are droq_cases.WIDE_CASES: the row counts
that are multiples of the tile and the stage, D + A = 16 and 64, and H1 < H2.  Every fourth row has mask 0.
The modes: "on" (dropout p) and "off" (drop_threshold 0, keep_scale 1) start from non-trivial m and v at Adam's step 3;
"first" (FIRST_CASE only, dropout on) is step 1 from zero m and v.  The live critics and the targets are different
networks.  Scalars reach the twin as the float32 values the argument block carries.

The seeds.  Many outputs are single numbers (b3 and its m, v and target) or short vectors, whose float32 error is a draw,
not a level: the error of one restatement can be far below that of another by luck, and 8 times a lucky error is a bar
no float32 computation meets.  A seed is therefore taken only if, for every mode and every one of the 204 outputs, two
restatements in two other summation orders each lie within 4 times the first one's error, and, without dropout, so does
torch's own float32 step on the CPU (the reference of the dropout-off GPU test is torch's float32 step, which has an
error of its own: its loss gradient multiplies by 1 / M where the header divides).  All of this is checked on the CPU by
test_critic_host.py, which asserts it; each seed is the first from 0 that passes.
"""

from __future__ import annotations

import copy
import functools
import types

import numpy as np
import torch

import critic_reference as cr
import droq_cases as dc
import droq_reference as dr

CASES = list(dc.CASES) + [(70, 20, 32, 32, 6, 0.25)]
FIRST_CASE = CASES[1]
# chosen once, on the CPU, so that test_critic_host's conditioning check holds (it asserts it); nothing a kernel computed
SEEDS = {CASES[0]: 67, CASES[1]: 210, CASES[2]: 38, CASES[3]: 89, CASES[4]: 1842}
# droq_cases.WIDE_CASES (it says what each is for): full tiles and exact stages of rows, D + A a multiple of 16, H1 < H2,
# 16 <-> 256.  Their seeds by the same rule, each the first from 0 that passes on the CPU.
WIDE_CASES = list(dc.WIDE_CASES)
SEEDS.update({WIDE_CASES[0]: 148, WIDE_CASES[1]: 144, WIDE_CASES[2]: 4244, WIDE_CASES[3]: 57})
ALL_CASES = CASES + WIDE_CASES
N_CRITICS = (1, 2, 3, 4)
WIDE_N_CRITICS = (1, 4)   # of the wide cases in the GPU tests
SEED, ROUND = (5 << 32) | 13, 6
LN_EPS, CLIP, LR, TAU, EPS, BETAS = 1e-5, 5.0, 1e-2, 0.05, 1e-8, (0.9, 0.999)
KINDS = ("grad", "p", "m", "v", "target")


def f32(x):
    return float(np.float32(x))


def case_id(c):
    return "x".join(map(str, c))


def adam_scalars(t):
    """The Adam and Polyak scalars of step t as the argument block carries them (float32 values)."""
    return dict(step_size=f32(LR / (1.0 - BETAS[0] ** t)), bc2_sqrt=f32(np.sqrt(1.0 - BETAS[1] ** t)), eps=f32(EPS),
                omb1=f32(1.0 - BETAS[0]), beta2=f32(BETAS[1]), omb2=f32(1.0 - BETAS[1]), tau=f32(TAU))


def modes(case):
    return ("on", "off", "first") if case == FIRST_CASE else ("on", "off")


def keys(n):
    return tuple(f"q{i}" for i in range(n)) + tuple(f"{kind}{i}.{name}" for kind in KINDS for i in range(n) for name in cr.PARAMS)


def flat(out, n=None):
    """Every row of q and every tensor of every kind under a key of its own; the first n critics."""
    n = len(out["q"]) if n is None else n
    d = {f"q{i}": out["q"][i] for i in range(n)}
    for kind in KINDS:
        for i in range(n):
            for name, x in zip(cr.PARAMS, out[kind][i]):
                d[f"{kind}{i}.{name}"] = x
    return d


def first(d, n):
    """The keys of the first n critics of a flat dict of four."""
    return {k: d[k] for k in keys(n)}


def errors(a, ref):
    return {k: float(np.abs(np.asarray(a[k], np.float64) - ref[k]).max()) for k in ref}


@functools.lru_cache(maxsize=None)
def problem(case, seed=None):
    rows, D, H1, H2, A, p = case
    seed = SEEDS[case] if seed is None else seed
    rng = np.random.default_rng(7000 * seed + rows + D)
    n = max(N_CRITICS)
    critics = [dc.critic_net(D + A, H1, H2, p, 100 * seed + 10 + i + rows) for i in range(n)]
    targets = [dc.critic_net(D + A, H1, H2, p, 100 * seed + 50 + i + rows) for i in range(n)]
    mean = rng.normal(size=D).astype(np.float32)
    inv_std = (1.0 / rng.uniform(0.5, 2.0, D)).astype(np.float32)
    obs = (mean + rng.normal(size=(rows, D)) * 2.0).astype(np.float32)
    obs.reshape(-1)[5::11] += 40.0                                    # every eleventh normalised entry clips at 5
    host = [dc.host(c) for c in critics]
    kw = dict(obs=obs, action=np.tanh(rng.normal(size=(rows, A))).astype(np.float32),
              y=rng.normal(size=rows).astype(np.float32), mask=(np.arange(rows) % 4 != 2).astype(np.float32),
              mean=mean, inv_std=inv_std, clip=CLIP, critics=host, targets=[dc.host(c) for c in targets], ln_eps=f32(LN_EPS),
              seed=SEED, round_=ROUND)
    m3 = [[(rng.normal(size=a.shape) * 1e-2).astype(np.float32) for a in net] for net in host]
    v3 = [[(rng.uniform(0.5, 1.5, size=a.shape) * 1e-4).astype(np.float32) for a in net] for net in host]
    zero = [[np.zeros_like(a) for a in net] for net in host]
    on = dict(threshold=dr.drop_threshold(p), keep_scale=f32(1.0 / (1.0 - p)))
    mode = {"on": dict(on, m=m3, v=v3, **adam_scalars(3)), "off": dict(threshold=0, keep_scale=1.0, m=m3, v=v3, **adam_scalars(3)),
            "first": dict(on, m=zero, v=zero, **adam_scalars(1))}
    out = types.SimpleNamespace(case=case, critics=critics, targets=targets, kw=kw, mode=mode, ref={}, err32={}, err_perm={}, err_perm2={})
    for name in modes(case):
        run = lambda **o: flat(cr.step(**kw, **mode[name], **o))
        ref = run(dtype=np.float64)
        out.ref[name] = ref
        out.err32[name] = errors(run(dtype=np.float32), ref)
        out.err_perm[name] = errors(run(dtype=np.float32, permute=seed + 1), ref)
        out.err_perm2[name] = errors(run(dtype=np.float32, permute=seed + 2), ref)
    return out


def torch_step(p, n, device):
    """The "off" step of the first n critics of problem p by torch in float32 on `device`: the modules in eval() mode,
    autograd on offpolicy.critic_loss, torch.optim.Adam from the case's m and v at step 3, _foreach_lerp_.  -> the flat dict."""
    from robopianist_amd import offpolicy
    md, up = p.mode["off"], lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)
    nets = [copy.deepcopy(c).to(device).eval() for c in p.critics[:n]]
    targets = [copy.deepcopy(c).to(device) for c in p.targets[:n]]
    params = [t for net in nets for t in dc.params(net)]
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS)
    for t, m, v in zip(params, [a for net in md["m"][:n] for a in net], [a for net in md["v"][:n] for a in net]):
        opt.state[t] = {"step": torch.tensor(2.0), "exp_avg": up(m.copy()), "exp_avg_sq": up(v.copy())}
    xn = torch.clamp((up(p.kw["obs"]) - up(p.kw["mean"])) * up(p.kw["inv_std"]), -CLIP, CLIP)
    xa = torch.cat([xn, up(p.kw["action"])], dim=1)
    qs = [c(xa).squeeze(-1) for c in nets]
    loss = offpolicy.critic_loss(qs, up(p.kw["y"]), up(p.kw["mask"]))
    opt.zero_grad(set_to_none=True)
    loss.backward()
    grads = [t.grad.clone() for t in params]
    opt.step()
    with torch.no_grad():
        torch._foreach_lerp_([t for net in targets for t in dc.params(net)], params, TAU)
    h = lambda t: t.detach().cpu().numpy()
    out = {f"q{i}": h(q) for i, q in enumerate(qs)}
    for i in range(n):
        for k, name in enumerate(cr.PARAMS):
            t = params[10 * i + k]
            out.update({f"grad{i}.{name}": h(grads[10 * i + k]), f"p{i}.{name}": h(t), f"m{i}.{name}": h(opt.state[t]["exp_avg"]),
                        f"v{i}.{name}": h(opt.state[t]["exp_avg_sq"]), f"target{i}.{name}": h(dc.params(targets[i])[k])})
    return out
