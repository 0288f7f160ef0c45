"""GPU tests of the fused actor step (include/learn/rp_actor.h) and of droq.DroQ(actor_step="fused").

The per-row outputs (action, logp, q_min), the seven gradients, every p, m and v after the step, log_alpha with its m and
v and the five statistics are compared with the float64 twin (tests/actor_reference.py, which test_actor_host.py checks
against torch's autograd) under the bar of the other learner tests: 8 times the error of a float32 numpy restatement of
the same formulae on the same inputs, computed by the test, per output.  The noise and the dropout masks are integers and
the same in the kernels and in both restatements, so the three differ only by float32 rounding in another order.  The
cases and their seeds are actor_cases's; test_actor_host.py checks on the CPU that they are well conditioned.  The lines of
a run are kept in profiles/actor_gpu_tests.txt.

Tests on inputs that are not a case's own (row ranges, the deep range, the mask edge cases, the learner's step) were not
screened by the seeds' rule; `_levels` says what their single-number outputs are held to and why.

Measured on an MI355X: over all cases, modes and numbers of critics the worst ratio of the kernels' error to the
restatement's among the 37 outputs is 5.2 (stats.entropy of (64, 44, 16, 256, 20) without dropout, 4.72e-06 | 9.01e-07);
most lines stand between 1.0 and 1.5.  Against torch's own float32 step without dropout the worst outputs of the nine
cases lie between 1.4 and 2.2 restatement errors.  The toy task went from a mean reward of -0.3589 over the first 5 rounds
to -0.0415 over the last 5 of 40 with the torch critic step (ratio 0.116) and from -0.3630 to -0.0408 with the fused one
(ratio 0.112); test_gpu_droq.py records 0.111 for the torch actor step.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import actor_cases as ac  # noqa: E402
import actor_reference as ar  # noqa: E402
import critic_reference as cr  # noqa: E402
from test_gpu_droq import DEEP_B, DEEP_FIRST, TOY, deep  # noqa: E402
from test_gpu_offpolicy import POISON, _ToyEnv, _dev, _piano_env, _same_bits, _stream, _up  # noqa: E402
from robopianist_amd import actor, critic, droq  # noqa: E402

pytestmark = pytest.mark.gpu

ROW_KEYS = ("action", "logp", "q_min")


def _run_step(p, n, mode="on", first=0, count=None, round_=ac.ROUND, launches=(actor.STEP,), grad=True, rows_out=True, **override):
    """The step on the first n critics of case p; -> the flat dict of actor_cases (the per-row outputs: the rows of the
    range), plus "<key>_all" (the whole per-row arrays) and "critics" (the critics' tensors after the call).
    `override`: inputs that are not p.kw's (the batch is as long as its obs).  `launches`: the `launches` of successive
    calls on the same tensors and workspace; with more than one -> the list of the dicts after each call.  `grad`,
    `rows_out`: whether the call gets gradient pointers and per-row output pointers."""
    _, D, H1, H2, A, _ = p.case
    kw = p.twin_kw(mode, n, **override)
    rows = len(kw["obs"])
    count = rows - first if count is None else count
    dev = _dev()
    d = {k: _up(kw[k]) for k in ("obs", "mask", "mean", "inv_std")}
    P, M, V = ([_up(a) for a in kw[k]] for k in ("actor", "m", "v"))
    G = [torch.full_like(t, POISON) for t in P]
    C = [[_up(a) for a in net] for net in kw["critics"]]
    one = lambda x: _up(np.asarray(x, np.float32).reshape(1))
    la, la_m, la_v, la_g = one(kw["log_alpha"]), one(kw["log_alpha_m"]), one(kw["log_alpha_v"]), one(POISON)
    out_rows = {"action": torch.full((rows, A), POISON, device=dev), "logp": torch.full((rows,), POISON, device=dev),
                "q_min": torch.full((rows,), POISON, device=dev)}
    stats = torch.full((5,), POISON, device=dev)
    nbytes = actor.workspace_bytes(H1, H2, A, count)
    ws = torch.full((max(nbytes // 4, 1),), float("nan"), device=dev)
    adam = lambda s: actor.Adam(s["omb1"], s["beta2"], s["omb2"], s["step_size"], s["bc2_sqrt"], s["eps"])
    host = lambda group: [t.cpu().numpy() for t in group]
    outs = []
    for launch in launches:
        actor.step(d["obs"].data_ptr(), d["mask"].data_ptr(), d["mean"].data_ptr(), d["inv_std"].data_ptr(), kw["clip"],
                   actor.set_entry(P), actor.set_entry(M), actor.set_entry(V), [critic.set_entry(net) for net in C],
                   la.data_ptr(), la_m.data_ptr(), la_v.data_ptr(), kw["target_entropy"], kw["log_std_bounds"], ws.data_ptr(),
                   nbytes, stats.data_ptr(), D, H1, H2, A, rows, adam(kw["actor_adam"]), adam(kw["alpha_adam"]),
                   grad=actor.set_entry(G) if grad else None, log_alpha_grad=la_g.data_ptr() if grad else None,
                   **({k: t.data_ptr() for k, t in out_rows.items()} if rows_out else {}), threshold=kw["threshold"],
                   keep_scale=kw["keep_scale"], ln_eps=kw["ln_eps"], seed=kw["seed"], round_=round_, row_first=first,
                   row_count=count, launches=launch, hip_stream=_stream())
        torch.cuda.synchronize()
        whole = {k: t.cpu().numpy() for k, t in out_rows.items()}
        out = ac.flat({**{k: a[first:first + count] for k, a in whole.items()}, "grad": host(G), "p": host(P), "m": host(M),
                       "v": host(V), "log_alpha": {"grad": la_g.cpu().numpy(), "p": la.cpu().numpy(), "m": la_m.cpu().numpy(),
                                                   "v": la_v.cpu().numpy()}, "stats": stats.cpu().numpy()})
        if not grad:
            assert all((out[k] == POISON).all() for k in out if "grad" in k)
            out = {k: v for k, v in out.items() if "grad" not in k}
        if not rows_out:
            assert all((whole[k] == POISON).all() for k in whole)
            out = {k: v for k, v in out.items() if k not in ROW_KEYS}
        out.update({k + "_all": a for k, a in whole.items()})
        out["critics"] = [host(net) for net in C]
        outs.append(out)
    return outs[0] if len(outs) == 1 else outs


def _compared(got):
    return {k: v for k, v in got.items() if not k.endswith("_all") and k != "critics"}


def _within(got, ref, err32, label):
    pairs = {k: (float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max()), err32[k]) for k in ref}
    ratio = lambda k: pairs[k][0] / pairs[k][1] if pairs[k][1] > 0 else (np.inf if pairs[k][0] > 0 else 0.0)
    worst = max(pairs, key=ratio)
    show = [k for k in pairs if k in ("action", "logp", "q_min", "grad.w1", "grad.w3", "p.w1", "log_alpha.p", "stats.actor_loss")] + [worst]
    print(f"{label}: kernel error | float32 restatement error: " +
          ", ".join(f"{k} {pairs[k][0]:.2e} | {pairs[k][1]:.2e}" for k in dict.fromkeys(show)) +
          f" (worst ratio: {worst} {ratio(worst):.3f})")
    for k, (e, b) in pairs.items():
        assert got[k].shape == ref[k].shape and e <= 8 * b, (label, k, e, b)


@pytest.mark.parametrize("case", ac.ALL_CASES, ids=ac.case_id)
def test_step_equals_the_float64_twin_within_8_float32_restatement_errors(case):
    """Dropout on: "on" starts from non-trivial m and v at the actor's step 3 and the temperature's step 5; "first"
    (FIRST_CASE) is step 1 of both from zero."""
    p = ac.problem(case)
    for mode in ac.modes(case):
        if mode == "off":
            continue
        for n in ac.n_critics(case):
            got = _run_step(p, n, mode)
            _within(_compared(got), p.ref(mode, n), p.err32(mode, n), f"actor step {case} {mode} critics {n}")
            assert all(np.isfinite(v).all() for v in _compared(got).values())


@pytest.mark.parametrize("case", ac.ALL_CASES, ids=ac.case_id)
def test_step_without_dropout_is_the_twin_and_torchs_own_step(case):
    p = ac.problem(case)
    missed = {}
    for n in ac.n_critics(case):
        got = _compared(_run_step(p, n, "off"))
        _within(got, p.ref("off", n), p.err32("off", n), f"actor step {case} dropout off critics {n}")
        if n not in ac.torch_n_critics(case):
            continue
        want = ac.torch_step(p, "off", n, _dev(), torch.float32, noise=p.ref_raw("off", n)["noise"])
        e32 = p.err32("off", n)
        pairs = {k: (float(np.abs(got[k].astype(np.float64) - w).max()), e32[k]) for k, w in want.items()}
        ratio = lambda k: pairs[k][0] / pairs[k][1] if pairs[k][1] > 0 else (np.inf if pairs[k][0] > 0 else 0.0)
        worst = max(pairs, key=ratio)
        print(f"actor step {case} dropout off critics {n}: against torch's own step on the GPU | float32 restatement error: "
              f"worst {worst} {pairs[worst][0]:.2e} | {pairs[worst][1]:.2e} (ratio {ratio(worst):.3f})")
        over = {k: (f"{e:.2e}", f"{b:.2e}") for k, (e, b) in pairs.items() if not e <= 8 * b}
        print(f"actor step {case} dropout off critics {n}: {len(over)} of {len(pairs)} outputs over the bar against torch: {over}")
        missed.update(over)
    assert not missed, (case, missed)


@pytest.mark.parametrize("case", [ac.CASES[1], ac.CASES[4]], ids=ac.case_id)
def test_step_is_deterministic_the_round_changes_it_and_the_noise_and_masks_are_the_twins(case):
    p = ac.problem(case)
    a, b = _compared(_run_step(p, 2)), _compared(_run_step(p, 2))
    assert all(_same_bits(a[k], b[k]) for k in a)
    other = _compared(_run_step(p, 2, round_=ac.ROUND + 1))
    assert all(not np.array_equal(other[k], a[k]) for k in a if "grad" in k or k in ROW_KEYS)
    # the kernel meets the bar only with the twin's noise and masks: the twin of another round misses it by far
    ref, e32 = p.ref("on", 2), p.err32("on", 2)
    moved = ac.flat(ar.step(**p.twin_kw("on", 2, round_=ac.ROUND + 1), dtype=np.float64))
    for k in ROW_KEYS + ("grad.w1", "grad.w3"):
        assert np.abs(moved[k] - ref[k]).max() > 1000 * 8 * e32[k], k
        assert np.abs(a[k] - ref[k]).max() <= 8 * e32[k], k
        assert np.abs(other[k] - moved[k]).max() < 0.01 * np.abs(moved[k] - ref[k]).max(), k


def _levels(kw, ref, e32):
    """The error level per output on inputs that the seeds' rule did not screen.  The single-number outputs (log_alpha's and
    the statistics) are weighted means of per-row values, w summing to at most 1.  A restatement's error of such a mean is
    a draw that can fall far below the per-row errors it averages (and the shuffled restatements share numpy's
    elementary functions with the first, so their draws are no others), while per-row errors that are correlated, as an
    elementary function's are, reach the mean at full size.  The level of such an output is therefore the larger of the
    restatement's own error and its per-row levels (logp's and q_min's restatement errors) carried through the header's
    formula in float64: g, entropy <- logp;  actor_loss <- al logp + q_min;  alpha_loss <- |log_alpha| logp;  log_alpha's
    p, m and v <- Adam's statements at g -+ logp's level;  alpha <- alpha times p's.  Every other output keeps the
    restatement's error."""
    lp, q = e32["logp"], e32["q_min"]
    la0 = np.asarray(kw["log_alpha"], np.float64).reshape(1)
    sc = [np.float64(kw["alpha_adam"][k]) for k in ar.ADAM]
    m, v = (np.asarray(kw[k], np.float64).reshape(1) for k in ("log_alpha_m", "log_alpha_v"))
    g = np.asarray(ref["log_alpha.grad"], np.float64)
    base = ar.adam(la0, m, v, g, *sc)
    moved = [ar.adam(la0, m, v, g + s * lp, *sc) for s in (-1.0, 1.0)]
    d = lambda i: max(float(np.abs(mv[i] - base[i]).max()) for mv in moved)
    carried = {"log_alpha.grad": lp, "log_alpha.p": d(0), "log_alpha.m": d(1), "log_alpha.v": d(2), "stats.entropy": lp,
               "stats.alpha_loss": float(np.abs(la0[0])) * lp, "stats.alpha": float(np.exp(base[0][0])) * d(0),
               "stats.actor_loss": float(np.exp(la0[0])) * lp + q}
    return {k: max(e, carried.get(k, 0.0)) for k, e in e32.items()}


def _twin(p, n, mode="on", first=0, count=None, **override):
    """The float64 twin and the error levels (`_levels`) on inputs that are not the case's own, computed here."""
    kw = p.twin_kw(mode, n, **override)
    run = lambda **o: ac.flat(ar.step(**kw, row_first=first, row_count=count, **o))
    ref = run(dtype=np.float64)
    return ref, _levels(kw, ref, ac.errors(run(dtype=np.float32), ref))


@pytest.mark.parametrize("case", [ac.CASES[2], ac.CASES[4], ac.WIDE_CASES[2]], ids=ac.case_id)
def test_step_row_ranges_read_and_write_nothing_outside(case):
    p = ac.problem(case)
    rows = case[0]
    ranges = ((16, 32), (0, 32), (63, 1)) if case == ac.WIDE_CASES[2] else ((3, rows - 7), (rows - 1, 1), (0, 17))
    for first, count in ranges:
        inside = np.zeros(rows, bool); inside[first:first + count] = True
        fill = lambda value: {k: np.where(inside.reshape((-1,) + (1,) * (p.kw[k].ndim - 1)), p.kw[k], np.float32(value))
                              for k in ("obs", "mask")}
        nan, zero = _run_step(p, 2, first=first, count=count, **fill(np.nan)), _run_step(p, 2, first=first, count=count, **fill(0.0))
        assert all(np.isfinite(v).all() for v in _compared(nan).values())
        assert all(_same_bits(nan[k], zero[k]) for k in _compared(nan)), (first, count)
        for k in ROW_KEYS:
            assert (nan[k + "_all"][~inside] == POISON).all() and (nan[k + "_all"][inside] != POISON).all(), k
        ref, e32 = _twin(p, 2, first=first, count=count)
        _within(_compared(nan), ref, e32, f"actor step {case} rows [{first}, {first + count})")


def test_step_deep_in_a_batch_differs_by_the_row_keyed_noise_and_masks_only():
    """Rows [1024, 1040) of a batch of 1040 whose other rows are NaN: nothing outside is read or written, and without
    dropout the only difference from the same rows at row_first = 0 is the noise, which the row keys."""
    case = ac.WIDE_CASES[1]
    p, rows, n = ac.problem(case), case[0], 2
    far = deep(p.kw, ("obs", "mask"), rows)
    far = {k: far[k] for k in ("obs", "mask")}
    inside = np.zeros(DEEP_B, bool); inside[DEEP_FIRST:] = True
    for mode in ("off", "on"):
        compact = _compared(_run_step(p, n, mode))
        got = _run_step(p, n, mode, first=DEEP_FIRST, count=rows, **far)
        there = _compared(got)
        assert all(np.isfinite(v).all() for v in there.values())
        for k in ROW_KEYS:
            assert (got[k + "_all"][~inside] == POISON).all() and len(got[k + "_all"]) == DEEP_B
        assert all(not np.array_equal(there[k], compact[k]) for k in ROW_KEYS)        # another row, another draw
        assert _same_bits(there["stats.masked"], compact["stats.masked"])
        ref, e32 = _twin(p, n, mode, first=DEEP_FIRST, count=rows, **far)
        _within(there, ref, e32, f"actor step {case} rows [{DEEP_FIRST}, {DEEP_B}) dropout {mode}")


def test_an_all_masked_range_is_adams_step_on_a_zero_gradient():
    case = ac.CASES[1]
    p, rows, n = ac.problem(case), case[0], 2
    got = _run_step(p, n, mask=np.zeros(rows, np.float32))
    kw = p.twin_kw("on", n)
    for which, sc in (("actor", kw["actor_adam"]), ("log_alpha", kw["alpha_adam"])):
        sc = [np.float32(sc[k]) for k in ar.ADAM]
        if which == "actor":
            triples = [(f"{{}}.{name}", a, m, v) for name, a, m, v in zip(ar.PARAMS, kw["actor"], kw["m"], kw["v"])]
        else:
            triples = [("log_alpha.{}", *(np.asarray(kw[k], np.float32).reshape(1) for k in ("log_alpha", "log_alpha_m", "log_alpha_v")))]
        for key, a, m, v in triples:
            g = got[key.format("grad")]
            assert g.shape == a.shape and not g.any(), key                       # M clamps to 1: 0 / 1, not 0 / 0
            want = ar.adam(a, m, v, np.zeros_like(a), *sc)
            for kind, w in zip(("p", "m", "v"), want):
                assert _same_bits(got[key.format(kind)], w), (key, kind)
    assert np.isfinite(got["action_all"]).all() and np.isfinite(got["logp_all"]).all() and np.isfinite(got["q_min_all"]).all()
    assert got["stats.masked"][0] == 1.0 and got["stats.actor_loss"][0] == 0.0 and got["stats.entropy"][0] == 0.0


def test_a_mask_sum_between_0_and_1_clamps_to_1_and_one_row_of_a_partial_tile_carries_a_step():
    case = ac.CASES[4]
    p, rows, n = ac.problem(case), case[0], 2
    quarter, last = np.zeros(rows, np.float32), np.zeros(rows, np.float32)
    quarter[[1, 33, 69]] = 0.25                                          # MSUM = 0.75: M = 1, not 0.75
    last[rows - 1] = 1.0                                                 # row 5 of the last tile's 6
    assert rows % 16 == 6 and cr.mask_sum(quarter) == np.float32(0.75)
    for label, mask in (("three rows of mask 0.25", quarter), ("the last row alone", last)):
        ref, e32 = _twin(p, n, mask=mask)
        got = _compared(_run_step(p, n, mask=mask))
        _within(got, ref, e32, f"actor step {case} {label}")
        assert all(got[k].any() and ref[k].any() for k in ref if "grad" in k), label


@pytest.mark.parametrize("case", [ac.CASES[3], ac.WIDE_CASES[3]], ids=ac.case_id)
def test_the_critics_are_not_written(case):
    p, n = ac.problem(case), 4
    got = _run_step(p, n)
    for net, before in zip(got["critics"], p.kw["critics"]):
        assert all(_same_bits(a, b) for a, b in zip(net, before))
    assert all(not np.array_equal(got[f"p.{name}"], a) for name, a in zip(ar.PARAMS, p.kw["actor"]))


@pytest.mark.parametrize("case", [ac.CASES[4], ac.WIDE_CASES[0]], ids=ac.case_id)
def test_the_two_launches_make_the_step(case):
    """ROWS_ONLY and APPLY_ONLY, the modes tools/gpu/actor_bench.py times, are the two launches of a step: the first writes
    the per-row outputs and the workspace only, the second on that workspace leaves what one STEP call leaves."""
    p, rows, n = ac.problem(case), case[0], 2
    assert actor.dim("launches") == 2
    kw = p.twin_kw("on", n)
    before = dict({f"{kind}.{name}": a for kind, key in (("p", "actor"), ("m", "m"), ("v", "v")) for name, a in zip(ar.PARAMS, kw[key])},
                  **{f"log_alpha.{kind}": np.asarray(kw[key], np.float32).reshape(1)
                     for kind, key in (("p", "log_alpha"), ("m", "log_alpha_m"), ("v", "log_alpha_v"))})
    for first, count in ((0, rows), (5, rows - 9)):
        step = _run_step(p, n, first=first, count=count)
        rows_only, both = _run_step(p, n, first=first, count=count, launches=(actor.ROWS_ONLY, actor.APPLY_ONLY))
        assert [k for k, a in before.items() if not _same_bits(rows_only[k], a)] == []
        assert all((rows_only[k] == POISON).all() for k in rows_only if "grad" in k or k.startswith("stats"))
        assert all(_same_bits(rows_only[k + "_all"], step[k + "_all"]) for k in ROW_KEYS)
        cs, cb = _compared(step), _compared(both)
        assert set(cb) == set(cs) and [k for k in cs if not _same_bits(cb[k], cs[k])] == [], (first, count)
        assert all(not np.array_equal(cs[k], a) for k, a in before.items())


def test_the_step_without_optional_pointers_is_the_step_with_them():
    p, n = ac.problem(ac.WIDE_CASES[3]), 2
    with_, without = _compared(_run_step(p, n)), _compared(_run_step(p, n, grad=False, rows_out=False))
    kept = [k for k in with_ if "grad" not in k and k not in ROW_KEYS]
    assert set(without) == set(kept) and len(kept) == 3 * 6 + 3 + 5
    assert [k for k in kept if not _same_bits(without[k], with_[k])] == []
    assert all((with_[k] != POISON).all() for k in with_ if "grad" in k)


@pytest.mark.parametrize("n", [1, 2])
def test_q_min_has_the_bits_of_the_critic_steps_q_at_the_actors_action(n):
    """The actor step and the critic step evaluate a critic through one device body, so without dropout (where the two
    launches' Philox counters do not matter) q_min of the actor step is, bit for bit, the q that the critic step's rows
    launch writes for the same observations, the same critics and the action the actor step wrote: q[0] with one critic,
    the elementwise minimum of q[0] and q[1] with two.  The case: 17 rows (a full tile and a partial one), H1 = 48, H2 = 16,
    D + A = 108, no multiple of 16."""
    case = ac.CASES[1]
    rows, D, H1, H2, A, _ = case
    assert rows % 16 and rows > 16 and H1 != H2 and (D + A) % 16
    p = ac.problem(case)
    kw = p.twin_kw("off", n)
    assert kw["threshold"] == 0 and kw["keep_scale"] == 1.0
    got = _run_step(p, n, "off")
    assert all(_same_bits(a, b) for net, before in zip(got["critics"], kw["critics"]) for a, b in zip(net, before))
    dev = _dev()
    d = {k: _up(kw[k]) for k in ("obs", "mask", "mean", "inv_std")}
    action, y = _up(got["action_all"]), torch.zeros(rows, device=dev)
    P = [[_up(a) for a in net] for net in kw["critics"]]
    M, V, T = ([[torch.zeros_like(t) for t in net] for net in P] for _ in range(3))
    q = torch.full((n, rows), POISON, device=dev)
    nbytes = critic.workspace_bytes(n, H1, H2, rows)
    ws = torch.full((max(nbytes // 4, 1),), float("nan"), device=dev)
    sets = lambda group: [critic.set_entry(net) for net in group]
    critic.step(d["obs"].data_ptr(), action.data_ptr(), y.data_ptr(), d["mask"].data_ptr(), d["mean"].data_ptr(),
                d["inv_std"].data_ptr(), kw["clip"], sets(P), sets(M), sets(V), sets(T), q.data_ptr(), ws.data_ptr(), nbytes,
                D, H1, H2, A, rows, 1e-3, 1.0, threshold=0, keep_scale=1.0, ln_eps=kw["ln_eps"], seed=kw["seed"], round_=ac.ROUND,
                launches=critic.ROWS_ONLY, hip_stream=_stream())
    torch.cuda.synchronize()
    assert all(_same_bits(t.cpu().numpy(), a) for net, before in zip(P, kw["critics"]) for t, a in zip(net, before))
    q = q.cpu().numpy()
    assert (q != POISON).all() and np.isfinite(q).all()
    want = q[0] if n == 1 else np.minimum(q[0], q[1])
    if n == 2:
        assert (q[0] < q[1]).any() and (q[1] < q[0]).any()          # each critic is the selected one on some row
    print(f"actor step {case} critics {n}: q_min against the critic step's q at the actor's action: "
          f"{int((got['q_min_all'].view(np.uint32) != want.view(np.uint32)).sum())} of {rows} rows differ in bits")
    assert _same_bits(got["q_min_all"], want)


# ---- the learner ---------------------------------------------------------------------------------------------------------
def _learner_bits(d):
    torch.cuda.synchronize()
    tensors = list(d.actor.parameters()) + [d.log_alpha] + [t for c in list(d.critics) + list(d.targets) for t in c.parameters()]
    if d.actor_mode == "fused":
        tensors += d._a_m + d._a_v + [d._la_m, d._la_v]
    return [t.detach().cpu().numpy().copy() for t in tensors]


@pytest.mark.parametrize("critic_step", ["torch", "fused"])
def test_fused_actor_droq_learns_a_toy_task(critic_step):
    """test_gpu_droq's toy task and hyper-parameters unchanged, plus actor_step="fused", under the same criterion; no
    parameter gets a .grad (with the fused critic step), the learner's generator is not advanced, and two learners with
    the same seed end with identical bits."""
    def run(rounds, at=None):
        torch.manual_seed(0)
        env = _ToyEnv(256, seed=1)
        learner = droq.DroQ(env, critic_step=critic_step, actor_step="fused", **TOY["droq"])
        gen, kept = learner._gen.get_state().clone(), []
        keep = lambda i, s: kept.append(_learner_bits(learner)) if i == at else None
        log = learner.train(rounds, TOY["steps_per_round"], TOY["grad_steps"], callback=keep)
        assert torch.equal(learner._gen.get_state(), gen)
        assert all(t.grad is None for t in list(learner.actor.parameters()) + [learner.log_alpha])
        if critic_step == "fused":
            assert all(t.grad is None for c in learner.critics for t in c.parameters())
        assert learner._a_t == learner._la_t == rounds * TOY["grad_steps"]
        return log, kept[0] if kept else _learner_bits(learner)

    # the second learner stops after 5 rounds, where the first one's bits were kept
    (log, bits), (log2, bits2) = run(TOY["rounds"], at=4), run(5)
    assert [s["actor_loss"] for s in log[:5]] == [s["actor_loss"] for s in log2]
    assert all(_same_bits(x, y) for x, y in zip(bits, bits2))
    curve = [s["mean_reward"] for s in log]
    first5, last5 = float(np.mean(curve[:5])), float(np.mean(curve[-5:]))
    print(f"toy task, fused actor step, critic step {critic_step}: mean reward {first5:.4f} (first 5 rounds) -> {last5:.4f} "
          f"(last 5); ratio {last5 / first5:.3f}; alpha {log[-1]['alpha']:.4f}; curve {[round(c, 3) for c in curve[::5]]}")
    assert first5 < -0.1 and last5 >= 0.5 * first5
    assert all(np.isfinite(s[k]) for s in log for k in ("critic_loss",) + actor.STATS) and log[-1]["episodes"] > 0


def test_fused_actor_droq_on_the_self_actuated_piano():
    """One update(1) per mode combination gives finite statistics; the fused actor step of an update is the twin's on the
    learner's own tensors; state_dict -> load_state_dict -> update reproduces the bits of the uninterrupted learner."""
    E, C, B, utd = 5, 4, 16, 3
    kw = dict(hidden=(32, 16), n_critics=2, capacity=C, batch_size=B, lr=1e-3, tau=0.25, seed=21, utd=utd, dropout=0.5)
    for critic_step in ("torch", "fused"):
        for actor_step in ("torch", "fused"):
            d = droq.DroQ(_piano_env(E), critic_step=critic_step, actor_step=actor_step, **kw)
            d.collect(6)
            torch.manual_seed(3)
            stats = d.update(1)
            assert set(stats) == {"critic_loss", "actor_loss", "alpha_loss", "alpha", "entropy", "masked"}
            assert all(np.isfinite(v) for v in stats.values()), (critic_step, actor_step, stats)
    # the last learner is fused / fused: its next actor step against the twin
    host = lambda ts: [t.detach().cpu().numpy().copy() for t in ts]
    step, seen = d._fused_actor_step, {}

    def hooked(u):
        torch.cuda.synchronize()
        seen.update(u=u, actor=host(d._actor_tensors()), m=host(d._a_m), v=host(d._a_v),
                    critics=[host(d._critic_tensors(c)) for c in d.critics], log_alpha=d.log_alpha.detach().cpu().numpy().copy(),
                    la_m=d._la_m.cpu().numpy().copy(), la_v=d._la_v.cpu().numpy().copy(), round=d._round, t=(d._a_t + 1, d._la_t + 1))
        return step(u)

    d._fused_actor_step = hooked
    stats = d.update(1)
    del d._fused_actor_step
    torch.cuda.synchronize()
    assert seen["u"] == utd - 1 and seen["t"] == (2, 2)
    scalars = lambda t: dict(zip(ar.ADAM, (ac.f32(x) for x in (*critic.adam_scalars(1e-3, t), 1e-8, 1.0 - 0.9, 0.999, 1.0 - 0.999))))
    skw = dict(obs=d._u_obs.cpu().numpy(), mask=d._u_mask.cpu().numpy(), mean=d.normalizer[3].cpu().numpy(),
               inv_std=d.normalizer[4].cpu().numpy(), clip=d.obs_clip, actor=seen["actor"], m=seen["m"], v=seen["v"],
               critics=seen["critics"], log_alpha=seen["log_alpha"], log_alpha_m=seen["la_m"], log_alpha_v=seen["la_v"],
               target_entropy=ac.f32(d.target_entropy), log_std_bounds=d.log_std_bounds, actor_adam=scalars(2), alpha_adam=scalars(2),
               threshold=droq.drop_threshold(0.5), keep_scale=2.0, ln_eps=ac.f32(d.ln_eps), seed=d.seed, round_=seen["round"],
               row_first=(utd - 1) * B, row_count=B)
    keys = [k for k in ac.keys() if "grad" not in k and k not in ROW_KEYS]
    ref = ac.flat(ar.step(dtype=np.float64, **skw))
    e32 = _levels(skw, ref, ac.errors(ac.flat(ar.step(dtype=np.float32, **skw)), ref))
    got = ac.flat({"action": None, "logp": None, "q_min": None, "grad": [None] * 6, "p": host(d._actor_tensors()), "m": host(d._a_m),
                   "v": host(d._a_v), "log_alpha": {"grad": None, "p": host([d.log_alpha])[0], "m": host([d._la_m])[0],
                                                    "v": host([d._la_v])[0]}, "stats": d._a_stats.cpu().numpy()})
    _within({k: got[k] for k in keys}, {k: ref[k] for k in keys}, e32, "fused DroQ update, the actor step")
    assert [stats[k] for k in actor.STATS] == [float(x) for x in d._a_stats.cpu().numpy()]
    # two learners joined by load_state_dict take the same update bit for bit
    other = droq.DroQ(_piano_env(E), critic_step="fused", actor_step="fused", **kw)
    other.load_state_dict(d.state_dict(include_replay=True))
    assert (other._a_t, other._la_t) == (d._a_t, d._la_t) == (2, 2)
    s_a, s_b = d.update(1), other.update(1)
    assert s_a == s_b
    assert all(_same_bits(x, y) for x, y in zip(_learner_bits(d), _learner_bits(other)))
    # a cross-mode checkpoint raises, both ways
    plain = droq.DroQ(_piano_env(E), critic_step="fused", **kw)
    with pytest.raises(ValueError, match="written with actor_step = fused"):
        plain.load_state_dict(d.state_dict())
    with pytest.raises(ValueError, match="written with actor_step = torch"):
        other.load_state_dict(plain.state_dict())
