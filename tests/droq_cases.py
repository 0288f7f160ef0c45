"""The cases of the DroQ target tests, shared by the host tests (which check their conditioning where no GPU is needed)
and the GPU tests (which run the kernel on them): the inputs, the float64 twin, the float32 restatement and a second
float32 restatement in another summation order, computed once per case.

A case is (rows, D, H1, H2, A, p).  The networks are drawn as torch draws them; the LayerNorm weights and biases are
moved off 1 and 0, so that a kernel that forgot them would be caught.  Every eleventh normalised observation clips, every
third row has discount 0.  `off` is the same problem with dropout switched off (drop_threshold 0, keep_scale 1).
"""

from __future__ import annotations

import functools
import types

import numpy as np
import torch

import droq_reference as dr

CASES = [(5, 1, 16, 16, 1, 0.5), (17, 63, 48, 16, 45, 0.5), (33, 255, 256, 256, 45, 0.01), (35, 300, 64, 64, 128, 0.25)]
# chosen once, on the CPU, so that test_droq_host's conditioning check holds (it asserts it); nothing a kernel computed
# (worst ratio of the permuted restatement's error to the first one's over all keys, of seeds 0 .. 3: case 0: 3.55, 4.60,
# 1.51, 6.10; case 1: 1.67, 2.35, 1.42, 1.42; case 2: 1.67, 2.14, 1.54, 1.50; case 3: 1.32, 1.62, 1.40, 2.35)
SEEDS = {CASES[0]: 2, CASES[1]: 2, CASES[2]: 3, CASES[3]: 0}
# The wide cases: what CASES (and critic_cases's fifth) never have.  Rows that are multiples of the tile of 16 and of the
# critic step's stage of 32, so that a last tile has no invalid row and a reduction over the rows ends on a full stage;
# D + A a multiple of 16, so that the last column tile of w1 has no lane past the input; H1 < H2; the narrowest layer into
# the widest and the reverse.
#   (32,  5,  16,  48,  3): H1 < H2; two full tiles, exactly one stage
#   (16, 12,  32,  16,  4): one full tile; D + A = 16 is one exact column tile; fewer rows than a stage
#   (64, 44,  16, 256, 20): narrowest into widest; D + A = 64; four full tiles, two exact stages; the critic step's
#                           3 x 16 + 4 x 256 + 1 = 1073 vector elements are five blocks of 256, the last with 49
#   (48, 30, 256,  16,  7): widest into narrowest; a full stage plus a full tile
WIDE_CASES = [(32, 5, 16, 48, 3, 0.5), (16, 12, 32, 16, 4, 0.25), (64, 44, 16, 256, 20, 0.25), (48, 30, 256, 16, 7, 0.5)]
# (seed 0 passes for all four: worst ratios 1.95, 2.41, 3.10, 1.78)
SEEDS.update({c: 0 for c in WIDE_CASES})
ALL_CASES = CASES + WIDE_CASES
N_CRITICS = (1, 2, 3, 4)
SEED, ROUND = (7 << 32) | 11, 3
LN_EPS, CLIP, GAMMA, LOG_ALPHA = 1e-5, 5.0, 0.97, np.float32(-0.7)


def case_id(c):
    return "x".join(map(str, c))


def critic_net(n_in, H1, H2, p, seed, eps=LN_EPS):
    """A DroQ critic, drawn as nn.Linear draws it; LayerNorm's weight in [0.5, 1.5], its bias in [-0.5, 0.5]."""
    from torch import nn
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = nn.Sequential(nn.Linear(n_in, H1), nn.Dropout(p), nn.LayerNorm(H1, eps), nn.ReLU(),
                            nn.Linear(H1, H2), nn.Dropout(p), nn.LayerNorm(H2, eps), nn.ReLU(), nn.Linear(H2, 1))
        with torch.no_grad():
            for i in (2, 6):
                net[i].weight.uniform_(0.5, 1.5)
                net[i].bias.uniform_(-0.5, 0.5)
    return net


def params(net):
    """(w1, b1, w2, b2, w3, b3, g1, be1, g2, be2) of a critic module."""
    return [t for i in (0, 4, 8) for t in (net[i].weight, net[i].bias)] + \
           [t for i in (2, 6) for t in (net[i].weight, net[i].bias)]


def host(net):
    return [t.detach().cpu().numpy() for t in params(net)]


def keys(n):
    return ("y", "q_min") + tuple(f"q{i}" for i in range(n))


def flat(out):
    """y, q_min and every row of q under keys of their own."""
    return dict({"y": out["y"], "q_min": out["q_min"]}, **{f"q{i}": q for i, q in enumerate(out["q"])})


def errors(a, ref):
    return {k: float(np.abs(a[k].astype(np.float64) - ref[k]).max()) for k in ref}


@functools.lru_cache(maxsize=None)
def problem(case, seed=None):
    rows, D, H1, H2, A, p = case
    seed = SEEDS[case] if seed is None else seed
    rng = np.random.default_rng(1000 * seed + rows + D)
    critics = [critic_net(D + A, H1, H2, p, 100 * seed + 10 + i + rows) for i in range(max(N_CRITICS))]
    mean = rng.normal(size=D).astype(np.float32)
    inv_std = (1.0 / rng.uniform(0.5, 2.0, D)).astype(np.float32)
    obs = (mean + rng.normal(size=(rows, D)) * 2.0).astype(np.float32)
    obs.reshape(-1)[5::11] += 40.0                                    # every eleventh normalised entry clips at 5
    kw = dict(next_obs=obs, action=np.tanh(rng.normal(size=(rows, A))).astype(np.float32),
              logp=rng.normal(size=rows).astype(np.float32), reward=rng.normal(size=rows).astype(np.float32),
              discount=np.where(np.arange(rows) % 3 == 1, 0.0, rng.uniform(0.5, 1.0, rows)).astype(np.float32),
              mean=mean, inv_std=inv_std, clip=CLIP, gamma=GAMMA, log_alpha=LOG_ALPHA, ln_eps=LN_EPS, seed=SEED, round_=ROUND)
    drop = {"on": dict(threshold=dr.drop_threshold(p), keep_scale=1.0 / (1.0 - p)), "off": dict(threshold=0, keep_scale=1.0)}
    out = types.SimpleNamespace(case=case, critics=critics, kw=kw, drop=drop, ref={}, err32={}, err_perm={})
    for mode, d in drop.items():
        for n in N_CRITICS:
            run = lambda **o: flat(dr.target(critics=[host(c) for c in critics[:n]], **kw, **d, **o))
            ref = run(dtype=np.float64)
            out.ref[mode, n] = ref
            out.err32[mode, n] = errors(run(dtype=np.float32), ref)
            out.err_perm[mode, n] = errors(run(dtype=np.float32, permute=seed + 1), ref)
    return out
