"""GPU tests of the fused task kernels (include/rp_task.h: rp_task_prestep, rp_task_rewards, rp_task_advance,
rp_task_rasterize) on synthetic states, against the float64 twin (tests/task_reference.py).

The four classes of task_kernels.py are driven with a stub `physics` of device tensors: no scene, no engine step, every
"model constant" the case's own (tests/task_cases.py; test_task_reference_host.py pins the twin to the torch hooks and
checks on the CPU that the cases are well conditioned).  Every output buffer is pre-filled with a poison value.

Bars.  Float64 floats: 1e-12 max(1, |twin|).  Float32 floats: 8 times the error of the float32 numpy restatement of
the same formulae on the same inputs against the float64 twin, per output, computed by the test; where the restatement
is exact the kernel must be.  Everything discrete (step types, counters, flags, indices, the evaluation reduction, the
trajectory record's words), the pre-step and the rasteriser: exact.  One line per case and precision gives the kernels'
error next to the restatement's; the lines of a run are kept in profiles/task_kernels_gpu_tests.txt.

Measured on an MI355X: over the 119 float32 lines (21 reward cases, 7 chains of 12 to 16 launches, the edges) the worst
ratio of the kernels' error to the restatement's is 3.98 (the OT fingering term of the five-env case
5-89-3x3x0-70-3x1-1-2-0, 6.53e-08 | 1.64e-08: a mean of at most five tolerances, where one restatement's draw falls below
the kernel's); the median line stands at 1.00 and 104 of the 119 at or below 1.5.  In float64 the worst error is 1e-15 of
the bar's unit.  The first run found one refusal that the header does not ask for: rp_task_prestep returned "null array
pointer" for n_action == 1, whose hand_act has no entries (tests/task_cases.py PRESTEP_CASES[0]); the check now asks for
the pointer only when there are hand actions.  docs/LAB_NOTEBOOK.md has the table of planted faults.
"""

from __future__ import annotations

import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import task_cases as tc  # noqa: E402
import task_reference as tr  # noqa: E402
from robopianist_amd import task_kernels as tk  # noqa: E402
from robopianist_amd.suite.scripted import ScriptedActions  # noqa: E402

pytestmark = pytest.mark.gpu

PRECISIONS = [np.float64, np.float32]
TORCH = {np.float64: torch.float64, np.float32: torch.float32}
prec_id = lambda T: "fp64" if T == np.float64 else "fp32"


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _up(a, T=None):
    """A numpy array on the device; floating arrays in the precision T."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f" and T is not None:
        a = a.astype(T)
    return torch.as_tensor(a, device=_dev()).contiguous()


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def _stub(T, E, nu, eng=None, nv=1):
    """The handful of attributes task_kernels reads from `physics`, as device tensors."""
    dev = _dev()
    z = lambda *s: torch.zeros(s, device=dev, dtype=TORCH[T])
    ph = types.SimpleNamespace(device=dev, dtype=TORCH[T], warn=torch.zeros(E, device=dev, dtype=torch.int32),
                               ctrl=torch.full((E, nu), tc.POISON, device=dev, dtype=TORCH[T]),
                               active_mask=torch.full((E,), tc.IPOISON, device=dev, dtype=torch.int32),
                               qpos=z(E, nv), act_force=z(E, nu), act_vel=z(E, nu), site_xpos_eng=z(E, tc.N_SITES, 3),
                               contact_geoms=torch.full((E, 1, 2), -1, device=dev, dtype=torch.int32))
    if eng is not None:
        ph.qpos, ph.act_force, ph.act_vel = _up(eng["qpos"], T), _up(eng["act_force"], T), _up(eng["act_vel"], T)
        ph.site_xpos_eng, ph.contact_geoms = _up(eng["site_xpos"], T), _up(eng["contact_geoms"].astype(np.int32))
    return ph


def _fused_rewards(T, kw, eng):
    E = len(eng["qpos"])
    ph = _stub(T, E, eng["act_force"].shape[1], eng)
    fr = tk.FusedRewards(ph, n_envs=E, key_qadr=kw["key_qadr"], key_anchor=torch.as_tensor(kw["key_anchor"]),
                         key_half=torch.as_tensor(kw["key_half"]), hand_act=kw["hand_act"], tip_site=kw["tip_site"], rfa=kw["rfa"],
                         lfa=kw["lfa"], use_fingering=kw["use_fingering"], use_forearm=kw["use_forearm"], energy_coef=kw["energy_coef"],
                         key_close=kw["key_close"], finger_close=kw["finger_close"], hand_filter=kw["hand_filter"])
    fr.terms.fill_(tc.POISON)
    fr.total.fill_(tc.POISON)
    return ph, fr


def _run_rewards(T, kw):
    E = len(kw["qpos"])
    _, fr = _fused_rewards(T, kw, kw)
    total, terms = fr.compute(goal_current=_up(kw["goal_current"], T), key_norm_state=_up(kw["key_norm_state"], T),
                              key_activation=_up(kw["key_activation"].astype(bool)),
                              sustain_activation=_up(kw["sustain_activation"].astype(bool).reshape(E, 1)),
                              finger_current=_up(kw["finger_current"].astype(np.int64)))
    return {"terms": _host(terms), "total": _host(total)}


def _within(T, got, ref, err32, label, show=None):
    """Every floating output under its bar; prints the line of the case.  -> the worst ratio to the bar's unit."""
    pairs, fails = {}, []
    for k in ref:
        r = np.asarray(ref[k], np.float64)
        g = np.asarray(got[k], np.float64)
        assert g.shape == r.shape, (label, k, g.shape, r.shape)
        err = np.abs(g - r)
        if T == np.float64:
            unit = float((err / np.maximum(1.0, np.abs(r))).max()) if err.size else 0.0
            pairs[k] = (unit, 1e-12)
            if not unit <= 1e-12:
                fails.append((k, unit))
        else:
            e, b = (float(err.max()) if err.size else 0.0), err32[k]
            pairs[k] = (e, b)
            if not e <= 8 * b:
                fails.append((k, e, b))
    ratio = lambda k: pairs[k][0] / pairs[k][1] if pairs[k][1] > 0 else (np.inf if pairs[k][0] > 0 else 0.0)
    worst = max(pairs, key=ratio)
    what = "kernel error / max(1, |twin|) | bar" if T == np.float64 else "kernel error | float32 restatement error"
    print(f"{label} {prec_id(T)}: {what}: " + ", ".join(f"{k} {pairs[k][0]:.2e} | {pairs[k][1]:.2e}" for k in (show or pairs)) +
          f" (worst ratio: {worst} {ratio(worst):.3f})")
    assert not fails, (label, fails)
    return ratio(worst)


def _same_bits(a, b):
    """Bit for bit; a NaN's payload is not an operation's result and is left out."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.kind == "f":
        nan = np.isnan(a) & np.isnan(b)
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return bool(((a.view(u) == b.view(u)) | nan).all())
    return bool(np.array_equal(a, b))


# ---- rp_task_rewards ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", PRECISIONS, ids=prec_id)
@pytest.mark.parametrize("case", tc.REWARD_CASES, ids=tc.case_id)
def test_rewards_match_the_twin(case, T):
    p = tc.reward_problem(case)
    got = tc.flat_rewards(_run_rewards(T, p.kw))
    _within(T, got, tc.flat_rewards(p.ref()), p.err32(), f"rewards {tc.case_id(case)}")
    if not case[6]:
        assert (got["fingering"] == 0).all()
    if not case[7]:
        assert (got["forearm"] == 0).all()


@pytest.mark.parametrize("T", PRECISIONS, ids=prec_id)
@pytest.mark.parametrize("case", tc.OT_CASES, ids=tc.case_id)
def test_ot_term_at_every_goal_set_size(case, T):
    p = tc.reward_problem(case)
    got = tc.flat_rewards(_run_rewards(T, p.kw))
    ref = tc.flat_rewards(p.ref())
    _within(T, got, ref, p.err32(), f"OT {tc.case_id(case)}")
    sizes = np.asarray([len(k) for k in p.on_keys])
    ntip = 5 if case[5] else 10
    assert {0, 1, ntip - 1, ntip, ntip + 1, 88} <= set(sizes.tolist())
    assert (got["fingering"][sizes == 0] == 1.0).all()       # the no-key env: exactly 1
    e32 = np.abs(np.asarray(p.run(np.float32)["terms"][3], np.float64) - ref["fingering"])
    for n in sorted(set(sizes.tolist())):
        err = np.abs(np.asarray(got["fingering"], np.float64) - ref["fingering"])[sizes == n].max()
        print(f"  {n:2d} keys: kernel error {err:.2e} | restatement {e32[sizes == n].max():.2e}")


@pytest.mark.parametrize("T", PRECISIONS, ids=prec_id)
@pytest.mark.parametrize("case", [tc.REWARD_CASES[3], tc.REWARD_CASES[15], tc.OT_CASES[0]], ids=tc.case_id)
def test_rewards_envs_are_independent(case, T):
    """Permuting the envs permutes the outputs bit for bit; one env alone gives row 0 of the 70."""
    p = tc.reward_problem(case)
    assert p.E == 70
    base = _run_rewards(T, p.kw)
    perm = np.random.default_rng(3).permutation(p.E)
    moved = _run_rewards(T, tc.take(p.kw, perm))
    assert _same_bits(moved["terms"], base["terms"][:, perm]) and _same_bits(moved["total"], base["total"][perm])
    for row in (0, 11, 69):
        one = _run_rewards(T, tc.take(p.kw, [row]))
        assert _same_bits(one["terms"], base["terms"][:, [row]]) and _same_bits(one["total"], base["total"][[row]])


# ---- rp_task_advance ----------------------------------------------------------------------------------------------------
class _Advance:
    """FusedAdvance on device arrays that start from `state` (numpy, the case's initial arrays)."""

    STATE = ("needs_reset", "key_state", "key_norm_state", "key_activation", "sustain_state", "sustain_activation", "t_idx",
             "should_terminate", "failure_termination", "discount_state", "goal_state", "goal_current", "finger_next",
             "finger_current", "fingering_state")

    def __init__(self, T, state, const, options, eng, record=True):
        self.T, E = T, len(eng["qpos"])
        self.E, self.nv = E, eng["qpos"].shape[1]
        kw = options
        self.ph, self.fr = _fused_rewards(T, kw, eng)
        self.const = {"goal_bank": _up(const["goal_bank"], T), "finger_bank": _up(const["finger_bank"].astype(np.int64)),
                      "song_len": _up(const["song_len"].astype(np.int64)), "key_qrange": _up(const["key_qrange"], T)}
        self.song_id = _up(np.asarray(state["song_id"], np.int64))
        self.fa = fa = tk.FusedAdvance(self.fr, n_lookahead=kw["n_lookahead"], song_id=self.song_id,
                                       wrong_press_termination=kw["wrong_press_termination"], key_threshold=kw["key_threshold"],
                                       sustain_threshold=kw["sustain_threshold"], warn_fatal_mask=kw["warn_fatal_mask"],
                                       warn_count_mask=kw["warn_count_mask"], **self.const)
        # (the launch must work on these very tensors: the constructor takes what already has the device and the type)
        assert fa._song_id is self.song_id and all(getattr(fa, "_" + k) is v for k, v in self.const.items())
        fa.fatal_count.copy_(_up(state["fatal_count"]))
        fa.warn_count.copy_(_up(state["warn_count"]))
        fa.discount.fill_(tc.POISON)
        fa.step_type.fill_(tc.IPOISON)
        self.extra = {}
        if "eval_sums" in state:
            ev = [_up(state[k]) for k in tr.ADVANCE_EVAL]
            fa.set_evaluation_buffers(*ev)
            self.extra.update(zip(tr.ADVANCE_EVAL, ev))
        if "next_ready" in state:
            nr, co = _up(state["next_ready"].astype(np.uint8)), _up(state["consumed"].astype(np.uint8))
            fa.set_prefetch_buffers(nr, co)
            self.extra.update(next_ready=nr, consumed=co)
        if record:
            fa.enable_trajectory_record(1)
            fa._traj[0].fill_(tc.POISON)
        bools = ("needs_reset", "key_activation", "sustain_activation", "should_terminate", "failure_termination")
        self.t = {k: _up(np.asarray(state[k]).astype(bool) if k in bools else state[k], T) for k in self.STATE if k != "sustain_state"}
        self.t["sustain_state"] = torch.zeros((E, 1), device=_dev(), dtype=TORCH[T])

    def reads(self):
        ph = self.ph
        return {"qpos": ph.qpos, "act_force": ph.act_force, "act_vel": ph.act_vel, "site_xpos": ph.site_xpos_eng,
                "contact_geoms": ph.contact_geoms, "warn": ph.warn, "sustain_state": self.t["sustain_state"], **self.const,
                "key_qadr": self.fr._key_qadr, "key_anchor": self.fr._key_anchor, "key_half": self.fr._key_half,
                "hand_act": self.fr._hand_act, "tip_site": self.fr._tip_site, "rfa": self.fr._rfa, "lfa": self.fr._lfa}

    def launch(self, inp):
        T, ph = self.T, self.ph
        ph.qpos.copy_(_up(inp["qpos"], T)); ph.act_force.copy_(_up(inp["act_force"], T)); ph.act_vel.copy_(_up(inp["act_vel"], T))
        ph.site_xpos_eng.copy_(_up(inp["site_xpos"], T)); ph.contact_geoms.copy_(_up(inp["contact_geoms"].astype(np.int32)))
        ph.warn.copy_(_up(inp["warn"].astype(np.int32)))
        self.t["sustain_state"].copy_(_up(inp["sustain_state"], T))
        if "ready_set" in inp:
            self.extra["next_ready"].bitwise_or_(_up(inp["ready_set"].astype(np.uint8)))
        before = {k: v.clone() for k, v in self.reads().items()}
        self.fa.advance(**self.t)
        torch.cuda.synchronize()
        for k, v in self.reads().items():       # what the header says is only read
            assert torch.equal(v, before[k]), k
        fa = self.fa
        out = {k: _host(v) for k, v in self.t.items() if k != "sustain_state"}
        out.update(discount=_host(fa.discount), step_type=_host(fa.step_type), terms=_host(self.fr.terms), total=_host(self.fr.total),
                   fatal_count=_host(fa.fatal_count), warn_count=_host(fa.warn_count), song_id=_host(self.song_id))
        out.update({k: _host(v) for k, v in self.extra.items()})
        if fa.trajectory_record is not None:
            out["traj_record"] = _host(fa.trajectory_record)
        return out


def _compare_advance(T, got, ref, err32, written, float_keys, nv, label):
    floats = {k: got[k] for k in float_keys}
    rfl = {k: ref[k] for k in float_keys}
    e32 = None if err32 is None else dict(err32)
    if "traj_record" in written:
        floats["traj_record"], rfl["traj_record"] = got["traj_record"][:, :nv + 3], ref["traj_record"][:, :nv + 3]
        assert got["traj_record"].shape[1] == nv + 3 + (2 if T == np.float64 else 3)
        words = np.ascontiguousarray(got["traj_record"][:, nv + 3:]).view(np.uint8)
        want = np.stack([tr.traj_words(row, T).view(np.uint8) for row in ref["key_activation"]])
        assert np.array_equal(words, want), (label, "the record's words")
    ratio = _within(T, floats, rfl, e32, label, show=("key_norm_state", "terms", "total", "traj_record"))
    for k in written:
        if k in float_keys or k == "traj_record":
            continue
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        if k in tr.ADVANCE_EVAL and g.dtype.kind == "f":
            assert _same_bits(g, r.astype(np.float64)), (label, k)      # the evaluation reduction is in double: exact
        else:
            assert np.array_equal(g.reshape(r.shape).astype(np.int64), r.astype(np.int64)), (label, k, g, r)
    return ratio


@pytest.mark.parametrize("T", PRECISIONS, ids=prec_id)
@pytest.mark.parametrize("name", list(tc.ADVANCE_CASES))
def test_advance_chain_matches_the_twin(name, T):
    """Launches chained on the device arrays and on the twin side by side: after every launch every array the header
    says is written is compared (the record's words, the counters, the flags, the evaluation reduction exactly), and
    every array it says is only read is unchanged."""
    p = tc.advance_problem(name)
    err32 = p.err32() if T == np.float32 else [None] * len(p.launches)
    run = _Advance(T, p.init, p.const, p.options, p.launches[0])
    state = p.init
    worst = 0.0
    for n, (inp, ref) in enumerate(zip(p.launches, p.refs)):
        resetting = np.asarray(state["needs_reset"], bool)
        got = run.launch(inp)
        worst = max(worst, _compare_advance(T, got, ref, err32[n], p.written(), p.float_keys(), p.c["nv"], f"advance {name} launch {n:2d}"))
        # a resetting env discards its state: FIRST, reward 0, discount 1, time 0, the task's discount back at 1 unless
        # a wrong press is standing
        assert (got["step_type"][resetting] == 0).all() and (got["total"][resetting] == 0).all()
        assert (got["discount"][resetting] == 1).all() and (got["t_idx"][resetting] == 0).all()
        assert not got["needs_reset"][resetting].any()
        state = ref
    print(f"advance {name} {prec_id(T)}: worst ratio over {len(p.launches)} launches {worst:.3f}")


def test_advance_exact_edges():
    """|st - hi| == key_threshold, goal - state == key_close, sustain_state == sustain_threshold, a joint exactly at lo
    or hi: float64, dyadic constants, the contract decides (test_task_reference_host.py says what)."""
    md, key, state, options, expect = tc.edge_problem()
    const = {k: state[k] for k in ("goal_bank", "finger_bank", "song_len", "key_qrange")}
    run = _Advance(np.float64, state, const, options, state)
    got = run.launch(state)
    ref = tr.advance(np.float64, state, **options)
    assert [bool(got["key_activation"][e, key[e]]) for e in range(5)] == expect["pressed"]
    assert got["sustain_activation"].ravel().tolist() == expect["sustain_on"]
    assert [got["key_state"][e, key[e]] for e in range(5)] == expect["key_state"]
    assert got["terms"][0, 1] == 1.0 and got["key_norm_state"][2, key[2]] == 1.0 and got["key_norm_state"][3, key[3]] == -0.5
    written = tr.ADVANCE_WRITES + ("traj_record",)
    floats = ("key_state", "key_norm_state", "goal_current", "goal_state", "fingering_state", "discount_state", "discount", "terms", "total")
    _compare_advance(np.float64, got, ref, None, written, floats, 89, "advance exact edges")


def test_advance_refusals_launch_nothing():
    """next_ready without consumed, partial evaluation buffers: a negative code, a message, and no output written."""
    p = tc.advance_problem("prefetch")
    run = _Advance(np.float64, p.init, p.const, p.options, p.launches[0])
    run.launch(p.launches[0])       # (fills every pointer of the argument block)
    fa, L = run.fa, tk._lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)

    def refused(message):
        watched = [fa.discount, fa.step_type, run.fr.terms, run.fr.total, run.t["t_idx"], run.t["key_state"], fa.trajectory_record]
        for t in watched:
            t.fill_(tc.IPOISON)
        rc = L.rp_task_advance(ctypes.byref(fa._p), stream)
        torch.cuda.synchronize()
        assert rc == -1 and message in L.rp_task_last_error().decode(), (rc, L.rp_task_last_error())
        assert all(bool((t == tc.IPOISON).all()) for t in watched)

    keep = fa._p.consumed
    fa._p.consumed = None
    refused("next_ready without consumed")
    fa._p.consumed = keep
    for field in ("eval_count", "eval_hist", "eval_nfinished"):
        keep = getattr(fa._p, field)
        setattr(fa._p, field, None)
        refused("incomplete evaluation buffers")
        setattr(fa._p, field, keep)
    keep, fa._p.eval_deque = fa._p.eval_deque, 0
    refused("incomplete evaluation buffers")
    fa._p.eval_deque = keep


# ---- rp_task_prestep ----------------------------------------------------------------------------------------------------
def _prestep(T, kw):
    E = len(kw["needs_reset"])
    nu = kw["ctrl"].shape[1]
    na = (kw["action_table"] if kw["action"] is None else kw["action"]).shape[1]
    ph = _stub(T, E, nu)
    sus = torch.full((E, 1), tc.POISON, device=_dev(), dtype=TORCH[T])
    fp = tk.FusedPrestep(ph, n_envs=E, n_action=na, hand_act=kw["hand_act"], sustain_state=sus)
    fp.reset_mask.fill_(77)
    return ph, sus, fp


@pytest.mark.parametrize("T", PRECISIONS, ids=prec_id)
@pytest.mark.parametrize("case", tc.PRESTEP_CASES, ids=tc.case_id)
def test_prestep_is_exact(case, T):
    """Every output bit for bit (the kernel rounds each operation on its own, the twin does the same in the same type);
    the rows of resetting envs and the actuators outside hand_act keep their poison."""
    kw = tc.prestep_problem(case)
    ph, sus, fp = _prestep(T, kw)
    index = None
    if kw["action"] is None:
        index = _up(kw["action_index"])
        action = ScriptedActions(_up(kw["action_table"], T), index)
    else:
        action = _up(kw["action"], T)
    bounds = (_up(kw["act_lo"], T), _up(kw["act_range"], T)) if "act_lo" in kw else None
    mask = fp.run(action, _up(kw["needs_reset"]), bounds, kw["clip"])
    ref = tr.prestep(T, **kw)
    got = {"ctrl": _host(ph.ctrl), "sustain_state": _host(sus), "active": _host(ph.active_mask), "reset_mask": _host(mask)}
    if index is not None:
        got["action_index"] = _host(index)
    for k in ref:
        assert _same_bits(got[k], ref[k]), (case, k, got[k], ref[k])
    untouched = np.ones(got["ctrl"].shape, bool)
    untouched[np.ix_(~kw["needs_reset"], kw["hand_act"])] = False
    assert (got["ctrl"][untouched] == tc.POISON).all()
    print(f"prestep {tc.case_id(case)} {prec_id(T)}: {sum(v.size for v in ref.values())} numbers bit for bit, "
          f"{int(untouched.sum())} of ctrl keep their poison, {int(np.isnan(got['ctrl']).sum())} NaN passed through")


def test_prestep_refusals_launch_nothing():
    """nu < n_action - 1 and an action table without its index."""
    kw = tc.prestep_problem(tc.PRESTEP_CASES[2])
    T = np.float64
    ph, sus, fp = _prestep(T, kw)
    index = _up(kw["action_index"])
    fp.run(ScriptedActions(_up(kw["action_table"], T), index), _up(kw["needs_reset"]), None, False)
    L, a = tk._lib(), fp._args
    stream = ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)

    def refused(message):
        ph.ctrl.fill_(tc.POISON); sus.fill_(tc.POISON); ph.active_mask.fill_(tc.IPOISON); fp.reset_mask.fill_(77)
        index.copy_(_up(kw["action_index"]))
        rc = L.rp_task_prestep(ctypes.byref(a), stream)
        torch.cuda.synchronize()
        assert rc == -1 and message in L.rp_task_last_error().decode(), (rc, L.rp_task_last_error())
        assert bool((ph.ctrl == tc.POISON).all()) and bool((sus == tc.POISON).all()) and bool((ph.active_mask == tc.IPOISON).all())
        assert bool((fp.reset_mask == 77).all()) and np.array_equal(_host(index), kw["action_index"])

    keep, a.nu = a.nu, a.n_action - 2
    refused("bad sizes")
    a.nu = keep
    keep, a.action_index = a.action_index, None
    refused("null array pointer")
    a.action_index = keep
    keep, a.action_table_len = a.action_table_len, 0
    refused("null array pointer")
    a.action_table_len = keep


# ---- rp_task_rasterize --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", PRECISIONS, ids=prec_id)
@pytest.mark.parametrize("case", tc.RASTER_CASES, ids=lambda c: f"dt{c[0]}-buffer{c[1]}")
def test_rasterize_is_exact(case, T):
    """Goal and fingering tables, lengths and statuses equal the host definition's; the slot of the job that does not fit
    and the slot no job names keep their poison."""
    kw = tc.raster_kw(case)
    ras = tk.Rasterizer(_dev(), TORCH[T], kw["songs"], kw["control_timestep"], kw["initial_buffer_time"])
    assert ras._p.n_buffer == case[1] and ras.MAX_OPS == len(tc.FULL_CHAIN)
    goal, fing, slen = _up(kw["goal_bank"], T), _up(kw["finger_bank"]), _up(kw["song_len"])
    status = ras.rasterize(goal, fing, slen, kw["slots"], kw["job_songs"], kw["ops"])
    ref = tr.rasterize(T, **kw)
    got = {"goal_bank": _host(goal), "finger_bank": _host(fing), "song_len": _host(slen), "status": _host(status)}
    for k in ref:
        assert _same_bits(got[k], ref[k]), (case, k, np.argwhere(got[k] != ref[k])[:10])
    assert (got["goal_bank"][[2, 6]] == tc.POISON).all() and (got["finger_bank"][[2, 6]] == tc.IPOISON).all()
    print(f"rasterize dt {case[0]} buffer {case[1]} {prec_id(T)}: {len(kw['slots'])} jobs, statuses {got['status'].tolist()}, "
          f"lengths {got['song_len'].tolist()}, {int((got['goal_bank'][got['goal_bank'] != tc.POISON] > 0).sum())} goal entries set")
