"""GPU tests of the fused critic step (include/learn/rp_critic.h) and of droq.DroQ(critic_step="fused").

q, every gradient and every p, m, v and target tensor after the step are compared with the float64 twin
(tests/critic_reference.py) under the bar of the other learner tests: 8 times the error of a float32 numpy restatement
of the same formulae on the same inputs, computed by the test, per tensor.  The dropout masks are integers and the same
in the kernels and in both restatements, so the three differ only by float32 rounding in another order.  The cases and
their seeds are critic_cases's; test_critic_host.py checks on the CPU that they are well conditioned (a second restatement
in another order within 4 times the first one's error).  The lines of a run are kept in profiles/critic_gpu_tests.txt.

Measured on an MI355X: in every line of the run -- all cases, modes, ranges, 1 .. 4 critics and the three ranges on the
piano -- the worst ratio of the kernels' error to the restatement's among the 51 outputs per critic is 1.0 to the three
digits printed: with every product taken as the header's fused-multiply-add chain the restatement errs as the kernels do.  (With
numpy's products in the restatement, which sum in blocks and err less than a chain, the ratios reached 7.4 and one
single-number output, v3.b3 of a step-1 case, stood at 8.13.)  Against torch's own float32 step without dropout the worst
outputs of the five cases lie between 2.0 and 3.8 restatement errors.  Over the wide cases (critic_cases.WIDE_CASES: full
tiles, exact stages, D + A = 16 and 64, H1 < H2) and the tests added with them -- the deep range, the two launches, tau at
its ends, the two masks, the dead layer -- the worst ratio is again 1.000 in every line (profiles/droq_wide_gpu_tests.txt);
against torch's own step the wide cases' worst outputs lie between 2.5 and 4.9 restatement errors (the 4.9: grad1.g1 of
(64, 44, 16, 256, 20, 0.25), 2.98e-08 | 6.05e-09).  The toy task went from a mean reward of -0.3737
over the first 5 rounds to -0.0411 over the last 5 of 40 (ratio 0.110; with the torch critic step test_gpu_droq.py
records 0.111).
"""

from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critic_cases as cc  # noqa: E402
import critic_reference as cr  # noqa: E402
import droq_cases as dc  # noqa: E402
from test_gpu_droq import DEEP_B, DEEP_FIRST, TOY, deep  # noqa: E402
from test_gpu_offpolicy import POISON, _ToyEnv, _dev, _piano_env, _same_bits, _stream, _up  # noqa: E402
from robopianist_amd import critic, droq, offpolicy  # noqa: E402

pytestmark = pytest.mark.gpu


def _run_step(p, n, mode="on", first=0, count=None, round_=cc.ROUND, launches=(critic.STEP,), grad=True, tau=cc.TAU, **override):
    """The step on the first n critics of case p; -> the flat dict of critic_cases (q: the rows of the range), "q_all".
    `override`: inputs that are not p.kw's (the batch is as long as its obs).  `launches`: the `launches` of successive
    calls on the same tensors and workspace; with more than one -> the list of the dicts after each call.  `grad`: whether
    the call gets gradient pointers (without them the dict has no gradient keys)."""
    _, D, H1, H2, A, _ = p.case
    kw, md = dict(p.kw, **override), p.mode[mode]
    rows = len(kw["obs"])
    count = rows - first if count is None else count
    dev = _dev()
    d = {k: _up(kw[k]) for k in ("obs", "action", "y", "mask", "mean", "inv_std")}
    up = lambda group: [[_up(a) for a in net] for net in group[:n]]
    P, T, M, V = up(kw["critics"]), up(kw["targets"]), up(md["m"]), up(md["v"])
    G = [[torch.full_like(t, POISON) for t in net] for net in P]
    q = torch.full((n, rows), POISON, device=dev)
    nbytes = critic.workspace_bytes(n, H1, H2, count)
    ws = torch.full((max(nbytes // 4, 1),), float("nan"), device=dev)
    sets = lambda group: [critic.set_entry(net) for net in group]
    host = lambda group: [[t.cpu().numpy() for t in net] for net in group]
    outs = []
    for launch in launches:
        critic.step(d["obs"].data_ptr(), d["action"].data_ptr(), d["y"].data_ptr(), d["mask"].data_ptr(), d["mean"].data_ptr(),
                    d["inv_std"].data_ptr(), cc.CLIP, sets(P), sets(M), sets(V), sets(T), q.data_ptr(), ws.data_ptr(), nbytes,
                    D, H1, H2, A, rows, md["step_size"], md["bc2_sqrt"], eps=cc.EPS, betas=cc.BETAS, tau=tau,
                    grad=sets(G) if grad else None, threshold=md["threshold"], keep_scale=md["keep_scale"], ln_eps=cc.LN_EPS,
                    seed=cc.SEED, round_=round_, row_first=first, row_count=count, launches=launch, hip_stream=_stream())
        torch.cuda.synchronize()
        q_all = q.cpu().numpy()
        out = cc.flat({"q": q_all[:, first:first + count], "grad": host(G), "p": host(P), "m": host(M), "v": host(V), "target": host(T)})
        if not grad:
            assert all((g == POISON).all() for net in host(G) for g in net)
            out = {k: v for k, v in out.items() if not k.startswith("grad")}
        out["q_all"] = q_all
        outs.append(out)
    return outs[0] if len(outs) == 1 else outs


def _inputs(p, n, mode="on"):
    """What _run_step uploads for the p, m, v and target tensors, under the keys of its dict."""
    kw, md = p.kw, p.mode[mode]
    groups = {"p": kw["critics"], "m": md["m"], "v": md["v"], "target": kw["targets"]}
    return {f"{kind}{i}.{name}": a for kind, group in groups.items() for i in range(n) for name, a in zip(cr.PARAMS, group[i])}


def _within(got, ref, err32, label):
    pairs = {k: (float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max()), err32[k]) for k in ref}
    ratio = lambda k: pairs[k][0] / pairs[k][1] if pairs[k][1] > 0 else (np.inf if pairs[k][0] > 0 else 0.0)
    worst = max(pairs, key=ratio)
    show = [k for k in pairs if k in ("q0", "grad0.w1", "p0.w1", "m0.w1", "v0.w1", "target0.w1")] + [worst]
    print(f"{label}: kernel error | float32 restatement error: " +
          ", ".join(f"{k} {pairs[k][0]:.2e} | {pairs[k][1]:.2e}" for k in dict.fromkeys(show)) +
          f" (worst ratio: {worst} {ratio(worst):.3f})")
    for k, (e, b) in pairs.items():
        assert got[k].shape == ref[k].shape and e <= 8 * b, (label, k, e, b)


@pytest.mark.parametrize("case", cc.ALL_CASES, ids=cc.case_id)
def test_step_equals_the_float64_twin_within_8_float32_restatement_errors(case):
    p = cc.problem(case)
    for mode in cc.modes(case):
        if mode == "off":
            continue
        for n in (cc.N_CRITICS if case in cc.CASES else cc.WIDE_N_CRITICS):
            got = _run_step(p, n, mode)
            _within(cc.first(got, n), cc.first(p.ref[mode], n), p.err32[mode], f"step {case} {mode} critics {n}")
            assert all(np.isfinite(v).all() for v in got.values())


@pytest.mark.parametrize("case", [cc.CASES[1], cc.CASES[4]], ids=cc.case_id)
def test_step_is_deterministic_the_round_changes_it_and_the_masks_are_the_twins(case):
    p = cc.problem(case)
    a, b = _run_step(p, 2), _run_step(p, 2)
    assert all(_same_bits(a[k], b[k]) for k in a)
    other = _run_step(p, 2, round_=cc.ROUND + 1)
    for i in range(2):
        assert not np.array_equal(other[f"q{i}"], a[f"q{i}"])
        assert all(not np.array_equal(other[f"grad{i}.{name}"], a[f"grad{i}.{name}"]) for name in cr.PARAMS)
    if case[5] == 0.5:
        # the kernel's q meets the bar only with the twin's masks: the twin with another round's masks misses it by far
        wrong = cc.flat(cr.step(**p.kw, **p.mode["on"], dtype=np.float64), 2)
        moved = cc.flat(cr.step(**dict(p.kw, round_=cc.ROUND + 1), **p.mode["on"], dtype=np.float64), 2)
        for i in range(2):
            k = f"q{i}"
            assert np.abs(moved[k] - wrong[k]).max() > 1000 * 8 * p.err32["on"][k]
            assert np.abs(a[k] - p.ref["on"][k]).max() <= 8 * p.err32["on"][k]
            assert np.abs(other[k] - moved[k]).max() < 0.01 * np.abs(moved[k] - wrong[k]).max()


@pytest.mark.parametrize("case", cc.ALL_CASES, ids=cc.case_id)
def test_step_without_dropout_is_torchs_own_step(case):
    p = cc.problem(case)
    rows, D, H1, H2, A, _ = case
    dev, md, missed = _dev(), p.mode["off"], {}
    for n in (1, 3):
        got = _run_step(p, n, "off")
        _within(cc.first(got, n), cc.first(p.ref["off"], n), p.err32["off"], f"step {case} dropout off critics {n}")
        want = cc.torch_step(p, n, dev)
        pairs = {k: (float(np.abs(got[k].astype(np.float64) - w).max()), p.err32["off"][k]) for k, w in want.items()}
        worst = max(pairs, key=lambda k: pairs[k][0] / pairs[k][1] if pairs[k][1] > 0 else 0.0)
        print(f"step {case} dropout off critics {n}: against torch's own step on the GPU | float32 restatement error: "
              f"q0 {pairs['q0'][0]:.2e} | {pairs['q0'][1]:.2e}, worst {worst} {pairs[worst][0]:.2e} | {pairs[worst][1]:.2e}")
        over = {k: (f"{e:.2e}", f"{b:.2e}") for k, (e, b) in pairs.items() if not e <= 8 * b}
        print(f"step {case} dropout off critics {n}: {len(over)} of {len(pairs)} tensors over the bar against torch: {over}")
        missed.update(over)
    assert not missed, (case, missed)


def _row_ranges(case):
    """The wide case: a tile-aligned inner range, one exact stage, the last row alone."""
    rows = case[0]
    return ((16, 32), (0, 32), (63, 1)) if case == cc.WIDE_CASES[2] else ((3, rows - 7), (rows - 1, 1), (0, 17))


@pytest.mark.parametrize("case", [cc.CASES[2], cc.CASES[4], cc.WIDE_CASES[2]], ids=cc.case_id)
def test_step_row_ranges_read_and_write_nothing_outside(case):
    p = cc.problem(case)
    rows = case[0]
    for first, count in _row_ranges(case):
        inside = np.zeros(rows, bool); inside[first:first + count] = True
        fill = lambda value: {k: np.where(inside.reshape((-1,) + (1,) * (p.kw[k].ndim - 1)), p.kw[k], np.float32(value))
                              for k in ("obs", "action", "y", "mask")}
        nan, zero = _run_step(p, 2, first=first, count=count, **fill(np.nan)), _run_step(p, 2, first=first, count=count, **fill(0.0))
        assert all(np.isfinite(v).all() for k, v in nan.items())
        assert all(_same_bits(nan[k], zero[k]) for k in nan), (first, count)
        assert (nan["q_all"][:, ~inside] == POISON).all() and (nan["q_all"][:, inside] != POISON).all()
        # the range's step is the twin's on that range
        run = lambda **o: cc.flat(cr.step(**p.kw, **p.mode["on"], row_first=first, row_count=count, **o), 2)
        ref = run(dtype=np.float64)
        _within(cc.first(nan, 2), ref, cc.errors(run(dtype=np.float32), ref), f"step {case} rows [{first}, {first + count})")


def test_an_all_masked_range_is_adams_step_on_a_zero_gradient():
    p = cc.problem(cc.CASES[1])
    rows, n = cc.CASES[1][0], 2
    got = _run_step(p, n, mask=np.zeros(rows, np.float32))
    md = p.mode["on"]
    sc = [np.float32(md[k]) for k in ("step_size", "bc2_sqrt", "eps", "omb1", "beta2", "omb2", "tau")]
    for i in range(n):
        for k, name in enumerate(cr.PARAMS):
            g = got[f"grad{i}.{name}"]
            assert g.shape == p.kw["critics"][i][k].shape and not g.any(), name      # M clamps to 1: 0 / 1, not 0 / 0
            want = cr.adam(p.kw["critics"][i][k], md["m"][i][k], md["v"][i][k], p.kw["targets"][i][k], np.zeros_like(g), *sc)
            for kind, w in zip(("p", "m", "v", "target"), want):
                assert _same_bits(got[f"{kind}{i}.{name}"], w), (kind, i, name)
    assert np.isfinite(got["q_all"]).all()


def _twin(p, n, mode="on", first=0, count=None, scalars=None, **override):
    """The float64 twin and the float32 restatement's error on inputs that are not the case's own, computed here."""
    md = dict(p.mode[mode], **(scalars or {}))
    kw = dict(p.kw, **override)
    kw.update(critics=kw["critics"][:n], targets=kw["targets"][:n])
    run = lambda **o: cc.flat(cr.step(**kw, **md, row_first=first, row_count=count, **o), n)
    ref = run(dtype=np.float64)
    return ref, cc.errors(run(dtype=np.float32), ref)


@pytest.mark.parametrize("case", [cc.CASES[4], cc.WIDE_CASES[0]], ids=cc.case_id)
def test_the_two_launches_make_the_step(case):
    """ROWS_ONLY and APPLY_ONLY, the modes tools/gpu/critic_bench.py times, are the two launches of a step: the first
    writes q and the workspace only, the second on that workspace leaves what one STEP call leaves."""
    p, rows, n = cc.problem(case), case[0], 2
    before = _inputs(p, n)
    for first, count in ((0, rows), (5, rows - 9)):
        inside = np.zeros(rows, bool); inside[first:first + count] = True
        step = _run_step(p, n, first=first, count=count)
        rows_only, both = _run_step(p, n, first=first, count=count, launches=(critic.ROWS_ONLY, critic.APPLY_ONLY))
        assert [k for k, a in before.items() if not _same_bits(rows_only[k], a)] == []
        assert all((rows_only[k] == POISON).all() for k in rows_only if k.startswith("grad"))
        assert (rows_only["q_all"][:, ~inside] == POISON).all() and _same_bits(rows_only["q_all"], step["q_all"])
        assert set(both) == set(step) and [k for k in step if not _same_bits(both[k], step[k])] == [], (first, count)
        assert all(not np.array_equal(step[k], a) for k, a in before.items())


def test_the_step_without_gradient_pointers_is_the_step_with_them():
    p, n = cc.problem(cc.WIDE_CASES[3]), 2
    with_, without = _run_step(p, n), _run_step(p, n, grad=False)
    kept = [k for k in with_ if not k.startswith("grad")]
    assert set(without) == set(kept) and len(kept) == 1 + n * (1 + 4 * len(cr.PARAMS))
    assert [k for k in kept if not _same_bits(without[k], with_[k])] == []
    assert all((with_[k] != POISON).all() for k in with_ if k.startswith("grad"))


def test_tau_at_its_ends():
    case = cc.CASES[4]
    p, n = cc.problem(case), 2
    base, before = _run_step(p, n), _inputs(p, n)
    # tau = 0: the targets keep their bits; the critics and their moments step as ever
    still = _run_step(p, n, tau=0.0)
    for k in base:
        assert _same_bits(still[k], before[k] if k.startswith("target") else base[k]), k
    # tau = 1: the twin's t + (p - t) 1, which need not round to p
    ref, err32 = _twin(p, n, scalars=dict(tau=1.0))
    full = _run_step(p, n, tau=1.0)
    _within(cc.first(full, n), ref, err32, f"step {case} tau 1")
    assert all(_same_bits(full[k], base[k]) for k in base if not k.startswith("target"))
    assert all(not np.array_equal(full[k], base[k]) for k in base if k.startswith("target"))


def test_step_deep_in_a_batch_differs_by_addresses_and_masks_only():
    """test_gpu_droq's deep range on the step: rows [1024, 1040) of a batch of 1040 whose other rows are NaN."""
    case = cc.WIDE_CASES[1]
    p, rows, n = cc.problem(case), case[0], 2
    far = deep(p.kw, ("obs", "action", "y", "mask"), rows)
    far = {k: far[k] for k in ("obs", "action", "y", "mask")}
    inside = np.zeros(DEEP_B, bool); inside[DEEP_FIRST:] = True
    for mode in ("off", "on"):
        compact = _run_step(p, n, mode)
        got = _run_step(p, n, mode, first=DEEP_FIRST, count=rows, **far)
        assert all(np.isfinite(v).all() for v in got.values())
        assert (got["q_all"][:, ~inside] == POISON).all() and got["q_all"].shape == (n, DEEP_B)
        there = {k: v for k, v in got.items() if k != "q_all"}
        if mode == "off":
            assert [k for k in there if not _same_bits(there[k], compact[k])] == []
        else:
            assert all(not np.array_equal(there[f"q{i}"], compact[f"q{i}"]) for i in range(n))
        ref, err32 = _twin(p, n, mode, first=DEEP_FIRST, count=rows, **far)
        _within(there, ref, err32, f"step {case} rows [{DEEP_FIRST}, {DEEP_B}) dropout {mode}")


def test_a_mask_sum_between_0_and_1_clamps_to_1_and_one_row_of_a_partial_tile_carries_a_step():
    case = cc.CASES[4]
    p, rows, n = cc.problem(case), case[0], 2
    quarter, last = np.zeros(rows, np.float32), np.zeros(rows, np.float32)
    quarter[[1, 33, 69]] = 0.25                                          # MSUM = 0.75: M = 1, not 0.75
    last[rows - 1] = 1.0                                                 # row 5 of the last tile's 6
    assert rows % 16 == 6 and cr.mask_sum(quarter) == np.float32(0.75)
    for label, mask in (("three rows of mask 0.25", quarter), ("the last row alone", last)):
        ref, err32 = _twin(p, n, mask=mask)
        got = _run_step(p, n, mask=mask)
        _within(cc.first(got, n), ref, err32, f"step {case} {label}")
        assert all(got[k].any() and ref[k].any() for k in ref if k.startswith("grad")), label


def test_a_dead_first_layer_has_variance_0_and_the_other_critic_does_not_see_it():
    """w1 = 0 and b1 = 0 in critic 0: every row of its layer 1 is 0 before LayerNorm, so 1 / sigma = 1 / sqrt(ln_eps)
    carries its backward pass (and o1 = 0: g1's gradient is 0).  Critic 1, in the same launches, is not touched."""
    case = cc.WIDE_CASES[0]
    p, n = cc.problem(case), 2
    critics = [list(net) for net in p.kw["critics"]]
    critics[0][0], critics[0][1] = np.zeros_like(critics[0][0]), np.zeros_like(critics[0][1])
    base, got = _run_step(p, n), _run_step(p, n, critics=critics)
    assert all(np.isfinite(v).all() for v in got.values())
    ref, err32 = _twin(p, n, critics=critics)
    _within(cc.first(got, n), ref, err32, f"step {case} critic 0's first layer dead")
    own = lambda k, i: k.split(".")[0].endswith(str(i))
    assert [k for k in base if k != "q_all" and own(k, 1) and not _same_bits(got[k], base[k])] == []
    assert not got["grad0.g1"].any() and got["grad0.w1"].any() and got["grad0.be1"].any()
    assert not np.array_equal(got["q0"], base["q0"])


# ---- the learner ---------------------------------------------------------------------------------------------------------
def _host(groups):
    torch.cuda.synchronize()
    return [[t.detach().cpu().numpy().copy() for t in net] for net in groups]


def _state(d):
    return dict(p=_host([d._critic_tensors(c) for c in d.critics]), target=_host([d._critic_tensors(c) for c in d.targets]),
                m=_host(d._c_m), v=_host(d._c_v))


def test_fused_droq_on_the_self_actuated_piano():
    E, C, B, utd, tau = 5, 4, 16, 3, 0.25
    env_a, env_b = _piano_env(E), _piano_env(E)
    kw = dict(hidden=(32, 16), n_critics=2, capacity=C, batch_size=B, lr=1e-3, tau=tau, seed=21, utd=utd, dropout=0.5,
              critic_step="fused")
    d_a, d_b = droq.DroQ(env_a, **kw), droq.DroQ(env_b, **kw)
    d_a.collect(6)
    others = list(d_a.actor.parameters()) + [d_a.log_alpha]
    others_before = [t.detach().clone() for t in others]
    before, after, losses = [], [], []
    critic_step = d_a.critic_step

    def hooked(batch, **kwargs):
        before.append(_state(d_a))
        out = critic_step(batch, **kwargs)
        losses.append(out)
        after.append(_state(d_a))
        return out

    d_a.critic_step = hooked
    round_ = d_a._round
    stats = d_a.update(1)
    del d_a.critic_step
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in stats.values()), stats
    assert set(stats) == {"critic_loss", "actor_loss", "alpha_loss", "alpha", "entropy", "masked"}
    assert len(before) == utd and d_a._c_t == utd and d_a._round == round_ + 1
    assert [x is None for x in losses] == [True, True, False]                 # the loss only where update() returns it
    rows = {k: getattr(d_a, "_u_" + k).cpu().numpy() for k in ("obs", "action", "y", "mask")}
    q = d_a._u_q.cpu().numpy()
    mean, inv_std = d_a.normalizer[3].cpu().numpy(), d_a.normalizer[4].cpu().numpy()
    assert rows["mask"].sum() >= 1
    for u in range(utd):
        step_size, bc2_sqrt = critic.adam_scalars(1e-3, u + 1)
        skw = dict(obs=rows["obs"], action=rows["action"], y=rows["y"], mask=rows["mask"], mean=mean, inv_std=inv_std,
                   clip=d_a.obs_clip, critics=before[u]["p"], m=before[u]["m"], v=before[u]["v"], targets=before[u]["target"],
                   step_size=cc.f32(step_size), bc2_sqrt=cc.f32(bc2_sqrt), eps=cc.f32(1e-8), omb1=cc.f32(1.0 - 0.9),
                   beta2=cc.f32(0.999), omb2=cc.f32(1.0 - 0.999), tau=cc.f32(tau), threshold=droq.drop_threshold(0.5),
                   keep_scale=2.0, ln_eps=cc.f32(d_a.ln_eps), seed=d_a.seed, round_=round_, row_first=u * B, row_count=B)
        keys = [k for k in cc.keys(2) if not k.startswith("grad")]
        ref = cc.flat(cr.step(dtype=np.float64, **skw))
        f32 = cc.errors(cc.flat(cr.step(dtype=np.float32, **skw)), ref)
        got = cc.flat({"q": q[:, u * B:(u + 1) * B], "grad": after[u]["p"], **after[u]})
        _within({k: got[k] for k in keys}, {k: ref[k] for k in keys}, f32, f"fused DroQ update, range {u}")
        # the targets follow tau towards the just-updated critics
        for net_b, net_c, net_t in zip(before[u]["target"], after[u]["p"], after[u]["target"]):
            for tb, c, ta in zip(net_b, net_c, net_t):
                np.testing.assert_allclose(ta, tb + np.float32(tau) * (c - tb), rtol=1e-5, atol=1e-7)
                assert not np.array_equal(ta, tb)
        if u + 1 < utd:
            assert all(_same_bits(x, y) for k in after[u] for nx, ny in zip(after[u][k], before[u + 1][k]) for x, y in zip(nx, ny))
    want = offpolicy.critic_loss(list(d_a._u_q[:, (utd - 1) * B:]), d_a._u_y[(utd - 1) * B:], d_a._u_mask[(utd - 1) * B:])
    assert stats["critic_loss"] == float(want)
    # the actor and the temperature still step
    for b, a in zip(others_before, others):
        assert bool((a != b).any()) and bool(torch.isfinite(a).all())
    # two learners joined by load_state_dict take the same update bit for bit
    d_b.load_state_dict(d_a.state_dict(include_replay=True))
    assert d_b._c_t == utd
    torch.manual_seed(9)
    s_a = d_a.update(1)
    torch.manual_seed(9)
    s_b = d_b.update(1)
    assert s_a == s_b
    sa, sb = _state(d_a), _state(d_b)
    assert all(_same_bits(x, y) for k in sa for nx, ny in zip(sa[k], sb[k]) for x, y in zip(nx, ny))
    assert all(torch.equal(x, y) for x, y in zip(d_a.actor.parameters(), d_b.actor.parameters()))
    # a cross-mode checkpoint raises, both ways
    plain = droq.DroQ(env_b, **dict(kw, critic_step="torch"))
    with pytest.raises(ValueError, match="written with critic_step = fused"):
        plain.load_state_dict(d_a.state_dict())
    with pytest.raises(ValueError, match="written with critic_step = torch"):
        d_b.load_state_dict(plain.state_dict())


def test_fused_droq_learns_a_toy_task():
    """test_gpu_droq's toy task and hyper-parameters unchanged, plus critic_step="fused", under the same criterion."""
    torch.manual_seed(0)
    env = _ToyEnv(256, seed=1)
    learner = droq.DroQ(env, critic_step="fused", **TOY["droq"])
    log = learner.train(TOY["rounds"], TOY["steps_per_round"], TOY["grad_steps"])
    curve = [s["mean_reward"] for s in log]
    first5, last5 = float(np.mean(curve[:5])), float(np.mean(curve[-5:]))
    print(f"toy task, fused critic step: mean reward {first5:.4f} (first 5 rounds) -> {last5:.4f} (last 5); ratio "
          f"{last5 / first5:.3f}; alpha {log[-1]['alpha']:.4f}; curve {[round(c, 3) for c in curve[::5]]}")
    assert first5 < -0.1 and last5 >= 0.5 * first5
    assert all(np.isfinite(s["critic_loss"]) for s in log) and log[-1]["episodes"] > 0
