"""Host tests of the fused critic step (include/learn/rp_critic.h, robopianist_amd/critic.py): the float64 twin is torch's
own step (autograd on offpolicy.critic_loss, torch.optim.Adam, lerp_) with the twin's masks injected, the conditioning of
the cases the GPU tests run, the binding's symbols, struct sizes and argument validation (refused calls return before
anything touches a device), and the learner's option.

Conditioning.  The GPU tests hold the kernels to 8 times the error of a float32 restatement; that is only fair where a
float32 restatement in another summation order lies close to the first one.  Here a second restatement with the k order
of every product, the unit order of every LayerNorm sum and the row order of every batch sum shuffled must lie within 4
times the first one's error, for every case and mode and for q, every gradient and every updated p, m, v and target
tensor of all four critics, twice (two shuffles), and so must torch's own float32 step on the CPU without dropout.  The
seeds of critic_cases.SEEDS were chosen for that on the CPU (critic_cases.py says why).  The first restatement takes
every product as the header's fused-multiply-add chain, the shuffled ones and the float64 reference as numpy's product.
"""

from __future__ import annotations

import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critic_cases as cc  # noqa: E402
import critic_reference as cr  # noqa: E402
import droq_cases as dc  # noqa: E402
import droq_reference as dr  # noqa: E402
from test_offpolicy_host import _SpecEnv  # noqa: E402
from robopianist_amd import critic, droq, learning, offpolicy  # noqa: E402


# ---- the twin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_step", [1, 3])
def test_float64_twin_is_torchs_step_with_the_masks_injected(t_step):
    rows, D, H1, H2, A, p, n = 37, 5, 48, 16, 3, 0.5, 3
    rng = np.random.default_rng(4)
    lr_, tau, eps, ln_eps, clip = 3e-3, 0.1, 1e-8, float(np.float32(1e-5)), 2.0
    obs = (rng.normal(size=(rows, D)) * 3).astype(np.float32)
    action = np.tanh(rng.normal(size=(rows, A))).astype(np.float32)
    y, mask = rng.normal(size=rows), (rng.uniform(size=rows) < 0.8).astype(np.float64)
    mean, inv_std = rng.normal(size=D), 1 / rng.uniform(0.5, 2, D)
    nets = [dc.critic_net(D + A, H1, H2, p, s).double() for s in (1, 2, 3)]
    targets = [dc.critic_net(D + A, H1, H2, p, s).double() for s in (4, 5, 6)]
    host = [dc.host(c) for c in nets]
    if t_step == 1:
        m = [[np.zeros_like(a) for a in net] for net in host]
        v = [[np.zeros_like(a) for a in net] for net in host]
    else:
        m = [[rng.normal(size=a.shape) * 1e-2 for a in net] for net in host]
        v = [[rng.uniform(0.5, 1.5, size=a.shape) * 1e-4 for a in net] for net in host]
    scale = 1.0 / (1.0 - p)
    out = cr.step(obs, action, y, mask, mean, inv_std, clip, host, m, v, [dc.host(c) for c in targets],
                  step_size=lr_ / (1.0 - 0.9 ** t_step), bc2_sqrt=np.sqrt(1.0 - 0.999 ** t_step), eps=eps, omb1=1.0 - 0.9,
                  beta2=0.999, omb2=1.0 - 0.999, tau=tau, threshold=dr.drop_threshold(p), keep_scale=scale, ln_eps=ln_eps,
                  seed=cc.SEED, round_=4, dtype=np.float64)
    assert 0 < mask.sum() < rows
    xn = np.clip((obs - mean) * inv_std, -clip, clip)
    assert (np.abs(xn) == clip).any()
    x = torch.as_tensor(np.concatenate([xn, action], 1))
    qs = []
    for i, net in enumerate(nets):
        h = x
        for L, (lin, ln) in enumerate(((0, 2), (4, 6))):
            keep = cr.masks(np.arange(rows), net[lin].out_features, i, L, cc.SEED, 4, dr.drop_threshold(p))
            assert 0 < keep.sum() < keep.size and np.array_equal(keep, out["masks"][i][L])
            h = net[lin](h) * torch.as_tensor(keep.astype(np.float64)) * scale
            h = torch.relu(F.layer_norm(h, (h.shape[1],), net[ln].weight, net[ln].bias, ln_eps))
        qs.append(net[8](h)[:, 0])
    params = [t for net in nets for t in dc.params(net)]
    opt = torch.optim.Adam(params, lr=lr_)
    if t_step > 1:
        flat_m, flat_v = [a for net in m for a in net], [a for net in v for a in net]
        for t, a, b in zip(params, flat_m, flat_v):
            opt.state[t] = {"step": torch.tensor(float(t_step - 1)), "exp_avg": torch.as_tensor(a.copy()),
                            "exp_avg_sq": torch.as_tensor(b.copy())}
    loss = offpolicy.critic_loss(qs, torch.as_tensor(y), torch.as_tensor(mask))
    opt.zero_grad()
    loss.backward()
    grads = [t.grad.clone() for t in params]
    opt.step()
    with torch.no_grad():
        for tn, cn in zip(targets, nets):
            for tt, c in zip(dc.params(tn), dc.params(cn)):
                tt.lerp_(c, tau)

    def close(got, want, what):
        want = want.detach().numpy()
        bar = 1e-9 * max(float(np.abs(want).max()), 1e-300)
        assert got.shape == want.shape and float(np.abs(got - want).max()) <= bar, (what, float(np.abs(got - want).max()), bar)

    for i in range(n):
        close(out["q"][i], qs[i], f"q{i}")
        for k, name in enumerate(cr.PARAMS):
            t = params[10 * i + k]
            close(out["grad"][i][k], grads[10 * i + k], f"grad{i}.{name}")
            close(out["p"][i][k], t, f"p{i}.{name}")
            close(out["m"][i][k], opt.state[t]["exp_avg"], f"m{i}.{name}")
            close(out["v"][i][k], opt.state[t]["exp_avg_sq"], f"v{i}.{name}")
            close(out["target"][i][k], dc.params(targets[i])[k], f"target{i}.{name}")
            assert np.abs(out["grad"][i][k]).max() > 0


def test_the_counter_keeps_the_live_critics_masks_apart_from_the_targets():
    rows, t = np.arange(64), dr.drop_threshold(0.5)
    assert cr.COUNTER == critic.COUNTER == 48 and critic.dim("counter") == 48
    for i in range(4):
        for L in range(2):
            mine = cr.masks(rows, 64, i, L, cc.SEED, 1, t)
            assert 0.4 < (mine != dr.masks(rows, 64, i, L, cc.SEED, 1, t)).mean() < 0.6
    # every last counter word of the four users of one (seed, round) is its own
    words = list(range(3)) + list(range(16, 20)) + [dr.COUNTER + k for k in range(8)] + [cr.COUNTER + k for k in range(8)]
    assert len(set(words)) == len(words)
    # the range a row is computed in does not change its masks
    assert np.array_equal(cr.masks(np.arange(7, 19), 32, 1, 1, 3, 2, t), cr.masks(rows, 32, 1, 1, 3, 2, t)[7:19])


def test_the_batch_sums_of_the_twin_follow_the_header():
    x = np.random.default_rng(0).normal(size=(70, 3)).astype(np.float32)
    total = np.zeros(3, np.float32)
    for l0 in range(0, 70, 16):
        s = np.zeros(3, np.float32)
        for r in range(l0, min(l0 + 16, 70)):
            s = s + x[r]
        total = total + s
    assert np.array_equal(cr.tile_sum(x), total) and cr.tile_sum(x).dtype == np.float32
    mk = (np.arange(700) % 3 != 0).astype(np.float32)
    assert cr.mask_sum(mk) == mk.sum() and cr.mask_sum(mk[:5]) == mk[:5].sum()
    assert critic.dim("tile_rows") == cr.TILE == 16 and critic.dim("stage_rows") == 32
    # the added case exceeds two stages by a remainder that is no multiple of 16
    rows = cc.CASES[-1][0]
    assert rows > critic.dim("stage_rows") and (rows % critic.dim("stage_rows")) % 16 != 0


def test_the_wide_cases_are_what_the_first_five_are_not():
    tile, stage = critic.dim("tile_rows"), critic.dim("stage_rows")
    # the first five: no row count is a multiple of the tile, no D + A is, no H1 < H2
    assert all(c[0] % tile and (c[1] + c[4]) % 16 and c[2] >= c[3] for c in cc.CASES)
    assert cc.WIDE_CASES == dc.WIDE_CASES and len(cc.ALL_CASES) == 9 and len(set(cc.ALL_CASES)) == 9
    assert set(cc.SEEDS) == set(cc.ALL_CASES) and set(dc.SEEDS) == set(dc.ALL_CASES) and len(dc.ALL_CASES) == 8
    a, b, c, d = cc.WIDE_CASES
    # every wide case: only full tiles (the last tile has no invalid row)
    assert all(w[0] % tile == 0 for w in cc.WIDE_CASES)
    # a: H1 < H2 (the transposed layer has K = H2 > N = H1; w2's apply blocks are H1 / 16 of N = H2), exactly one stage
    assert a[2] < a[3] and a[0] == stage
    # b: one full tile, fewer rows than a stage, D + A one exact column tile of w1
    assert b[0] == tile < stage and b[1] + b[4] == 16
    # c: the narrowest layer into the widest, D + A four exact column tiles, two exact stages (the prefetch of the apply
    # launch's reduction is skipped after a full stage), five vector blocks of which the last holds 49 elements
    assert (c[2], c[3]) == (16, learning.MAX_HIDDEN) and (c[1] + c[4]) % 16 == 0 and c[0] == 2 * stage
    V = 3 * c[2] + 4 * c[3] + 1
    assert V == 1073 and -(-V // 256) == 5 and V - 4 * 256 == 49
    # d: the widest into the narrowest, a full stage plus a full tile
    assert (d[2], d[3]) == (learning.MAX_HIDDEN, 16) and d[0] == stage + tile


# ---- the conditioning of the GPU cases -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.ALL_CASES, ids=cc.case_id)
def test_gpu_cases_are_well_conditioned(case):
    p = cc.problem(case)
    assert case[0] >= 5 and (p.kw["mask"] == 0).any() and (p.kw["mask"] == 1).any()
    assert ("first" in p.ref) == (case == cc.FIRST_CASE)
    worst = 0.0
    for mode, err in p.err32.items():
        assert set(err) == set(cc.keys(4))
        for k, e in err.items():
            for ep in (p.err_perm[mode][k], p.err_perm2[mode][k]):
                assert ep <= 4 * e, (case, mode, k, ep, e)
                worst = max(worst, ep / e if e > 0 else 0.0)
        assert all(np.abs(p.ref[mode][k]).max() > 0 for k in err if k.startswith("grad"))
    print(f"conditioning {case}: the permuted restatements' errors are at most {worst:.2f} x the first one's")
    # torch's own float32 step, the reference of the dropout-off GPU test, is as close to the float64 twin
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        et = cc.errors(cc.torch_step(p, 4, "cpu"), p.ref["off"])
    finally:
        torch.set_num_threads(threads)
    worst = max(et[k] / e if e > 0 else 0.0 for k, e in p.err32["off"].items())
    print(f"conditioning {case}: torch's float32 step on the CPU has at most {worst:.2f} x the restatement's error")
    for k, e in p.err32["off"].items():
        assert et[k] <= 4 * e, (case, "torch", k, et[k], e)
    assert not np.array_equal(p.ref["on"]["q0"], p.ref["off"]["q0"])          # the dropout of the case drops something


# ---- the binding -------------------------------------------------------------------------------------------------------
def test_exported_symbols_dims_and_struct_sizes():
    L_ = critic.load_library()
    assert set(critic.EXPORTED_SYMBOLS) == {"rp_critic_step", "rp_critic_workspace", "rp_critic_dim", "rp_critic_last_error"}
    assert [getattr(L_, s) for s in critic.EXPORTED_SYMBOLS]
    assert critic.dim("max_critics") == critic.MAX_CRITICS == 4 and critic.dim("launches") == 2
    assert critic.dim("max_hidden") == learning.MAX_HIDDEN == 256 and critic.dim("max_actions") == learning.MAX_ACTIONS
    assert critic.dim("nothing") == -1
    assert critic.PARAMS == cr.PARAMS and len(critic.PARAMS) == 10
    # the layouts of the header on the LP64 ABI
    assert ctypes.sizeof(critic.Set) == 80 and ctypes.sizeof(critic.WorkspaceArgs) == 32
    assert ctypes.sizeof(critic.StepArgs) == 232
    a = critic.make_args("step")
    assert critic.call_raw("step", a) != 0 and "struct_size" not in critic.last_error()
    a.struct_size -= 8
    assert critic.call_raw("step", a) != 0 and "struct_size" in critic.last_error()
    w = critic.make_args("workspace", n_critics=2, H1=16, H2=16, row_count=5)
    w.struct_size += 8
    assert critic.call_raw("workspace", w) != 0 and "struct_size" in critic.last_error()
    # each library keeps its own symbols
    assert not hasattr(droq.load_library(), "rp_critic_step") and not hasattr(L_, "rp_droq_target")


def test_workspace_size():
    # per critic: ds1, out1 [R][H1], ds2 [R][H2], the tiles' partial sums [T][3 H1 + 4 H2 + 1], rounded up to 16 bytes
    for n, H1, H2, R in ((1, 16, 16, 5), (2, 256, 256, 4096), (4, 48, 16, 17), (3, 32, 32, 70)):
        T = -(-R // 16)
        per = R * (2 * H1 + H2) + T * (3 * H1 + 4 * H2 + 1)
        assert critic.workspace_bytes(n, H1, H2, R) == 4 * n * (-(-per // 4) * 4)
    assert critic.workspace_bytes(2, 16, 16, 0) == 0
    for bad in (dict(n_critics=0), dict(n_critics=5), dict(H1=8), dict(H2=272), dict(row_count=-1)):
        with pytest.raises(critic.LearnError, match="rp_critic_workspace"):
            critic.workspace_bytes(**dict(dict(n_critics=2, H1=16, H2=16, row_count=4), **bad))


_A = 0x1000   # a non-null address: a refused call never reads it


def _refused(match, **values):
    args = critic.make_args("step", **values)
    assert critic.call_raw("step", args) != 0
    assert match in critic.last_error(), critic.last_error()


class _Fake:
    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address


def _set(hole=None):
    return critic.set_entry([None if k == hole else _Fake(_A) for k in range(10)])


def test_argument_validation_refuses_before_any_launch():
    tab = critic.set_table([_set(), _set()])
    need = critic.workspace_bytes(2, 16, 32, 4)
    sa = dict(obs=_A, action=_A, y=_A, mask=_A, mean=_A, inv_std=_A, obs_clip=5.0, p=tab, m=tab, v=tab, target=tab, grad=tab,
              n_critics=2, q=_A, workspace=_A, workspace_bytes=need, drop_threshold=7, keep_scale=1.0, ln_eps=1e-5,
              one_minus_beta1=0.1, beta2=0.999, one_minus_beta2=0.001, step_size=1e-3, bc2_sqrt=0.5, eps=1e-8, tau=0.005,
              D=3, H1=16, H2=32, A=2, B=4, row_first=0, row_count=4)
    # rp_droq_target's refusals
    for name in ("obs", "action", "y", "mask", "mean", "inv_std", "q"):
        _refused("a pointer is NULL", **dict(sa, **{name: None}))
    _refused("critics is NULL", **dict(sa, p=None))
    for n in (0, 5):
        _refused("n_critics", **dict(sa, n_critics=n))
    _refused("obs_clip", **dict(sa, obs_clip=-1.0))
    for bad in (0.0, -1.0, float("nan")):
        _refused("keep_scale must be > 0", **dict(sa, keep_scale=bad))
        _refused("ln_eps must be > 0", **dict(sa, ln_eps=bad))
        # ... and the step's own
        _refused("step_size must be > 0", **dict(sa, step_size=bad))
        _refused("bc2_sqrt must be > 0", **dict(sa, bc2_sqrt=bad))
        _refused("eps must be > 0", **dict(sa, eps=bad))
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
    _refused("m and v must not be NULL", **dict(sa, m=None))
    _refused("m and v must not be NULL", **dict(sa, v=None))
    _refused("target is NULL", **dict(sa, target=None))
    _refused("workspace is NULL", **dict(sa, workspace=None))
    _refused("is smaller than", **dict(sa, workspace_bytes=need - 1))
    _refused("is smaller than", **dict(sa, workspace_bytes=0))
    _refused("16-byte aligned", **dict(sa, workspace=_A + 4))
    for bad in (-1, 3):
        _refused("launches must be", **dict(sa, launches=bad))
    _refused("B must be", **dict(sa, B=0, row_count=0))
    _refused("outside the batch", **dict(sa, row_first=1, row_count=4))
    _refused("outside the batch", **dict(sa, row_first=-1))
    assert critic.last_error().startswith("rp_critic_step: ")
    # accepted: a zero-row range (nothing is launched; its workspace is empty), with or without gradient pointers
    assert critic.call_raw("step", critic.make_args("step", **dict(sa, row_count=0, workspace_bytes=0))) == 0
    assert critic.call_raw("step", critic.make_args("step", **dict(sa, row_first=4, row_count=0, grad=None))) == 0
    assert critic.call_raw("step", critic.make_args("step", **dict(sa, row_count=0, tau=0.0))) == 0
    assert critic.call_raw("step", critic.make_args("step", **dict(sa, row_count=0, tau=1.0))) == 0
    with pytest.raises(critic.LearnError):
        critic.set_table([])
    with pytest.raises(critic.LearnError):
        critic.set_table([_set()] * 5)
    with pytest.raises(critic.LearnError):
        critic.set_table([_set()], 2)
    with pytest.raises(critic.LearnError):
        critic.set_entry([_Fake(_A)] * 9)
    with pytest.raises(TypeError):
        critic.make_args("step", nothing=1)


def test_adam_scalars_are_torchs_doubles():
    for t in (1, 3, 1000):
        step_size, bc2 = critic.adam_scalars(3e-4, t)
        assert step_size == 3e-4 / (1 - 0.9 ** t) and bc2 == (1 - 0.999 ** t) ** 0.5


# ---- the learner's option ------------------------------------------------------------------------------------------------
def _droq(**kw):
    args = dict(hidden=(16, 32), n_critics=3, capacity=4, batch_size=32, lr=1e-2, tau=0.25, seed=5, dropout=0.25, utd=3)
    args.update(kw)
    return droq.DroQ(_SpecEnv(4, (4, 3), 3), **args)


def test_the_option_its_state_and_the_cross_mode_checkpoint():
    for bad in ("other", "", None, "Fused"):
        with pytest.raises(ValueError, match="critic_step must be"):
            _droq(critic_step=bad)
    plain, fused = _droq(), _droq(critic_step="fused")
    assert plain.critic_mode == "torch" and _droq(critic_step="torch").critic_mode == "torch" and fused.critic_mode == "fused"
    assert not hasattr(plain, "_c_m") and "critic_step" not in plain.state_dict()["droq"]
    # the same seed draws the same networks in both modes
    assert all(torch.equal(x, y) for a, b in zip(plain.critics, fused.critics) for x, y in zip(a.parameters(), b.parameters()))
    # m, v per tensor in the order of the ABI, zero; the workspace and q sized for one range and all ranges
    assert len(fused._c_m) == len(fused._c_v) == 3 and fused._c_t == 0
    shapes = [tuple(t.shape) for t in fused._c_m[1]]
    assert shapes == [(16, 10), (16,), (32, 16), (32,), (1, 32), (1,), (16,), (16,), (32,), (32,)]
    assert all(not bool(t.any()) for group in (fused._c_m, fused._c_v) for net in group for t in net)
    assert fused._c_bytes == critic.workspace_bytes(3, 16, 32, 32) and fused._c_ws.numel() * 4 >= fused._c_bytes
    assert tuple(fused._u_q.shape) == (3, 96)
    sd = fused.state_dict()
    assert sd["droq"]["critic_step"] == "fused" and sd["critic_adam"]["t"] == 0 and len(sd["critic_adam"]["m"][2]) == 10
    fused._c_m[1][3].fill_(2.0)
    fused._c_t = 7
    sd = fused.state_dict()
    again = _droq(critic_step="fused", seed=9)
    again.load_state_dict(sd)
    assert again._c_t == 7 and bool((again._c_m[1][3] == 2.0).all()) and not bool(again._c_m[1][2].any())
    fused._c_m[1][3].fill_(3.0)
    assert bool((sd["critic_adam"]["m"][1][3] == 2.0).all())                 # a snapshot, not a view
    with pytest.raises(ValueError, match="written with critic_step = fused, this learner has critic_step = torch"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="written with critic_step = torch, this learner has critic_step = fused"):
        fused.load_state_dict(plain.state_dict())
    # a fused step is a step on a range of the learner's own minibatch
    with pytest.raises(droq.LearnError, match="range of the learner's own minibatch"):
        fused.critic_step({k: v.clone() for k, v in fused.minibatch().items()})
    assert fused._fused_range(fused.minibatch()) == 2
