"""Host tests of population-based training (include/learn/rp_evolve.h, robopianist_amd/evolve.py): the numpy twin
(evolve_reference.py, written from the header) against answers worked out by hand, the binding's symbols, struct layouts and
argument validation (refused calls return before anything touches a device), and `DroQPopulation(evolve=...)` on the CPU:
the option, the field table, the checkpoint."""

from __future__ import annotations

import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evolve_cases as ec  # noqa: E402
import evolve_reference as er  # noqa: E402
import plan_reference as pr  # noqa: E402
from test_offpolicy_host import _SpecEnv  # noqa: E402
from robopianist_amd import evolve, population  # noqa: E402
from robopianist_amd.learning import LearnError  # noqa: E402

f32 = np.float32


# ---- the twin against answers worked out by hand -----------------------------------------------------------------------------
def test_five_members_with_a_tie_and_an_ineligible_member():
    """min_episodes 2, percent 50.  Scores 2, 3, (100: one episode, ineligible), 3, 3: the three 3s rank 0, 1, 2 by member
    number, member 0 ranks 3; n = 4, k = min(4 x 50 / 100, 4 / 2) = 2: winners 1 and 3, losers 4 and 0.  Member 4's score
    equals every winner's: its gap 0 is not > 0 and it keeps itself.  Member 0 draws the words below (Philox is held to its
    known answers in test_plan_host.py): word 0 is even -> the winner of rank 0, member 1; word 1 has bits 0 and 1 set ->
    `up` for both.  With factors (0.5, 1.5): gamma = 1 - (1 - 0.75) x 1.5 = 0.625, target_entropy = -4 x 1.5 = -6."""
    assert [hex(w) for w in er.draw(7, 3, 0)][:2] == ["0x18d31004", "0x32d5a633"]
    assert [hex(w) for w in er.draw(7, 3, 4)][:2] == ["0x697da803", "0xe05c8531"]
    fit_sum, fit_count = np.array([8.0, 12.0, 100.0, 6.0, 24.0]), np.array([4, 4, 1, 2, 8])
    gamma, entropy = np.array([0.9, 0.75, 0.3, 0.5, 0.7], f32), np.array([-1.0, -4.0, -3.0, -8.0, -2.0], f32)
    kw = dict(percent=50, min_episodes=2, factors=(0.5, 1.5), gamma=gamma, target_entropy=entropy, seed=7, generation=3)
    out = er.plan(fit_sum, fit_count, **kw)
    assert out["rank"].tolist() == [3, 0, -1, 1, 2] and (out["n"], out["k"]) == (4, 2)
    assert out["winners"] == [1, 3] and sorted(out["losers"]) == [0, 4]
    assert out["source"].tolist() == [1, 1, 2, 3, 4] and out["source"].dtype == np.int32
    assert out["gamma"].tolist() == [0.625, 0.75, f32(0.3), 0.5, f32(0.7)] and out["gamma"].dtype == f32
    assert out["target_entropy"].tolist() == [-6.0, -4.0, -3.0, -8.0, -2.0]
    assert not out["fit_sum"].any() and not out["fit_count"].any() and out["fit_count"].dtype == np.int64
    # member 4 at score 2 ties with member 0, which ranks first of the two; its word 0 is odd -> the winner of rank 1,
    # member 3; word 1 = ...0001: `up` for gamma, `down` for the entropy: 1 - 0.5 x 1.5 = 0.25 and -8 x 0.5 = -4
    out = er.plan(np.array([8.0, 12.0, 100.0, 6.0, 16.0]), fit_count, **kw)
    assert out["rank"].tolist() == [2, 0, -1, 1, 3] and out["source"].tolist() == [1, 1, 2, 3, 3]
    assert out["gamma"].tolist() == [0.625, 0.75, f32(0.3), 0.5, 0.25]
    assert out["target_entropy"].tolist() == [-6.0, -4.0, -3.0, -8.0, -4.0]
    # a gap that is not larger than min_gap keeps the loser: both gaps are exactly 1
    assert er.plan(np.array([8.0, 12.0, 100.0, 6.0, 16.0]), fit_count, **dict(kw, min_gap=1.0))["source"].tolist() == [0, 1, 2, 3, 4]
    # a quantity that is not explored is not returned, and the other one is explored as before
    only = er.plan(fit_sum, fit_count, **dict(kw, gamma=None))
    assert only["gamma"] is None and only["target_entropy"].tolist() == [-6.0, -4.0, -3.0, -8.0, -2.0]


def test_the_summation_order_of_fold():
    """One member, 130 envs.  Lane 0 holds the envs 0, 64, 128: (1e16 + 1) + -1e16 = 0 (the 1 is below half an ulp of
    1e16); lane 1 holds env 1: 1; the lanes ascending: 0 + 1 = 1.  The envs ascending give ((1e16 + 1) + 1) - 1e16 = 0."""
    r = np.zeros(130)
    r[0], r[1], r[64], r[128] = 1e16, 1.0, 1.0, -1e16
    c = np.zeros(130, np.int32)
    c[[0, 1, 64, 128]] = 1, 2, 3, 4
    s, n = er.fold(r, c, [0.5], [10], 1)
    assert s.tolist() == [1.5] and n.tolist() == [20] and s.dtype == np.float64 and n.dtype == np.int64
    ascending = 0.0
    for v in r:
        ascending = ascending + v
    assert ascending == 0.0
    assert er.fold(r, c, [0.5], [10], 1, wave=1)[0].tolist() == [0.5]          # (one lane: the envs ascending)
    # the lanes' sum is added to the window, not the window to the first lane: 1e16 + (1 + 1) against (1e16 + 1) + 1
    r = np.zeros(2)
    r[:] = 1.0
    assert er.fold(r, np.zeros(2, np.int32), [1e16], [0], 1)[0].tolist() == [1e16 + 2.0] and 1e16 + 1.0 + 1.0 == 1e16
    # member p owns the envs p + P j; counts near 2^31 per env add up in 64 bits
    r, c = np.arange(6, dtype=np.float64), np.full(6, 2 ** 31 - 1, np.int32)
    s, n = er.fold(r, c, np.zeros(2), np.zeros(2, np.int64), 2)
    assert s.tolist() == [0.0 + 2.0 + 4.0, 1.0 + 3.0 + 5.0] and n.tolist() == [3 * (2 ** 31 - 1)] * 2
    # every case's data shows its order: the envs ascending give other bits (where a lane holds more than one env)
    for P, Em in ec.FOLD_CASES:
        p = ec.fold_problem(P, Em)
        got = er.fold(p["done_return"], p["done_count"], p["fit_sum"], p["fit_count"], P)
        other = er.fold(p["done_return"], p["done_count"], p["fit_sum"], p["fit_count"], P, wave=1)
        assert np.array_equal(got[1], other[1])
        if Em > 64:
            assert not np.array_equal(got[0], other[0]), (P, Em)
        lo, hi = np.abs(p["done_return"]).min(), np.abs(p["done_return"]).max()
        assert lo >= 1e-3 and hi <= 1e9 and (Em < 64 or hi / lo > 1e9)


def test_the_size_of_the_ends():
    want = {0: [0] * 10, 25: [0, 0, 0, 0, 1, 1, 1, 1, 2, 2], 50: [0, 0, 1, 1, 2, 2, 3, 3, 4, 4], 100: [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]}
    for percent, ks in want.items():
        assert [er.ends(n, percent) for n in range(10)] == ks, percent
    assert er.ends(256, 1) == 2 and er.ends(99, 1) == 0 and er.ends(255, 100) == 127


def test_the_explore_statements_at_the_clamp():
    # inside, at and beyond either bound; every operation rounded to float32 on its own
    assert er.explore_gamma(f32(0.75), 1.5, 0.0, 1.0) == f32(0.625) and er.explore_gamma(f32(0.75), 1.5, 0.7, 1.0) == f32(0.7)
    assert er.explore_gamma(f32(0.75), 0.5, 0.0, 0.8) == f32(0.8) and er.explore_gamma(f32(0.75), 0.5, 0.875, 0.875) == f32(0.875)
    g = er.explore_gamma(f32(0.99), 0.8, 0.0, 1.0)
    d = f32(1.0) - f32(0.99)
    assert g == f32(1.0) - d * f32(0.8) and g.dtype == f32
    assert float(d) == 1.0 - float(f32(0.99)) and d != f32(0.01)                      # (1 - 0.99f is exact, and is not 0.01f)
    assert er.explore_gamma(f32(0.9999), 0.8, 0.0, 0.9999) == f32(0.9999)
    assert er.explore_entropy(f32(-4.0), 1.5, -5.0, 0.0) == f32(-5.0) and er.explore_entropy(f32(-4.0), 0.5, -5.0, -3.0) == f32(-3.0)
    assert er.explore_entropy(f32(-4.0), 1.25, -np.inf, np.inf) == f32(-5.0)
    assert er.explore_entropy(f32(-3.3), 0.8, -np.inf, np.inf) == f32(-3.3) * f32(0.8)


def _twin_kw(case, P):
    """`er.plan`'s arguments of a case of `ec.plan_cases(P)`."""
    kind, seed = case["windows"]
    fit_sum, fit_count = ec.plan_windows(P, kind, seed)
    gamma, entropy = ec.plan_hypers(P, seed)
    kw = {k: v for k, v in case.items() if k not in ("windows", "explore")}
    kw.update(gamma=gamma if "gamma" in case["explore"] else None,
              target_entropy=entropy if "target_entropy" in case["explore"] else None)
    return fit_sum, fit_count, kw


@pytest.mark.parametrize("P", ec.PLAN_MEMBERS)
def test_the_plan_cases_show_what_they_are_for(P):
    """Structure, in every case: a source differs from its member only for a loser and is a winner; winners and losers are
    disjoint; the windows are cleared.  And the kinds hold what their names say."""
    replaced = 0
    for case in ec.plan_cases(P):
        fit_sum, fit_count, kw = _twin_kw(case, P)
        out = er.plan(fit_sum, fit_count, **kw)
        assert not set(out["winners"]) & set(out["losers"]) and len(out["winners"]) == len(out["losers"]) == out["k"]
        for p in range(P):
            if out["source"][p] != p:
                assert p in out["losers"] and out["source"][p] in out["winners"]
        assert not out["fit_sum"].any() and not out["fit_count"].any()
        kind = case["windows"][0]
        score, eligible = er.scores(fit_sum, fit_count, ec.MIN_EPISODES)
        if kind == "none":
            assert out["n"] == 0 and (out["source"] == np.arange(P)).all()
        if kind == "tie":
            assert out["n"] == P and len(set(score)) == 1 and (out["source"] == np.arange(P)).all()
            assert out["rank"].tolist() == list(range(P))
        if kind == "mixed":
            assert 0 < out["n"] < P or P == 1
            assert P < 8 or (np.isnan(fit_sum).any() and (fit_count < ec.MIN_EPISODES).any())
        if kind == "inf" and P >= 4:
            assert np.isposinf(score).sum() == 2 and np.isneginf(score).sum() == 2
        if case["percent"] == 0 or case["min_gap"] > 0:
            assert (out["source"] == np.arange(P)).all()
        for name, lo_hi in (("gamma", case["gamma_bounds"]), ("target_entropy", case["entropy_bounds"])):
            if out[name] is not None:
                changed = out["source"] != np.arange(P)
                assert (out[name][changed] >= f32(lo_hi[0])).all() and (out[name][changed] <= f32(lo_hi[1])).all()
        replaced += int((out["source"] != np.arange(P)).sum())
    assert replaced > 0 or P < 4
    # the two tight-bound cases clamp every explored value, one at each bound
    if P >= 4:
        low, high = [c for c in ec.plan_cases(P) if c["gamma_bounds"] in ((0.9995, 0.9999), (0.5, 0.75))]
        for case, side in ((low, 0), (high, 1)):
            fit_sum, fit_count, kw = _twin_kw(case, P)
            out = er.plan(fit_sum, fit_count, **kw)
            changed = out["source"] != np.arange(P)
            assert changed.any() and (out["gamma"][changed] == f32(case["gamma_bounds"][side])).all()
            assert (out["target_entropy"][changed] == f32(case["entropy_bounds"][side])).all()
        # generations and seeds draw differently
        drawn = {(c["seed"], c["generation"]): er.plan(*_twin_kw(c, P)[:2], **_twin_kw(c, P)[2])
                 for c in ec.plan_cases(P) if c["windows"] == ("spread", 6)}
        assert len(drawn) == 6 and (P < 16 or len({tuple(o["source"]) for o in drawn.values()}) > 1)


def test_the_copy_twin_and_the_layout_of_its_cases():
    a = np.arange(12, dtype=np.uint32).reshape(4, 3)
    assert er.copy(a, [0, 0, 2, 2]).tolist() == [[0, 1, 2], [0, 1, 2], [6, 7, 8], [6, 7, 8]]
    assert er.copy(a, [0, 1, 2, 3]).tolist() == a.tolist()
    # a source that does not keep itself, or lies outside the population, copies nothing
    assert er.copy(a, [1, 2, 2, 9]).tolist() == [[0, 1, 2], [6, 7, 8], [6, 7, 8], [9, 10, 11]]
    assert er.copy(a, [-1, 1, 2, 3]).tolist() == a.tolist()
    assert er.copy(a.astype(np.float64), [3, 1, 2, 3])[0].tolist() == [9.0, 10.0, 11.0]
    assert [er.launches(n) for n in (0, 1, 63, 64, 65, 128, 129, 130)] == [0, 1, 1, 1, 2, 2, 3, 3] and er.launches(7, P=1) == 0
    assert [evolve.launches_for(n) for n in (0, 1, 64, 65, 130)] == [0, 1, 1, 2, 3] and evolve.launches_for(7, 1) == 0
    total, at = ec.copy_layout(ec.small_fields(), 5)
    assert len(at) == 40 and sorted({(4 * first) % 16 for first, _ in at}) == [0, 4, 8, 12]
    ends = [(first, first + 5 * words) for first, words in at]
    assert all(b0 - a1 >= ec.GUARD for (_, a1), (b0, _) in zip(ends, ends[1:])) and ends[0][0] >= ec.GUARD
    assert total - ends[-1][1] == ec.GUARD
    # odd slices: source and destination differ in alignment
    assert any((4 * words) % 16 for _, words in at)
    for P in (2, 5, 6):
        s = ec.copy_sources(P)
        assert (s["identity"] == np.arange(P)).all() and (s["one"] != np.arange(P)).sum() == 1
        assert (s["half"] != np.arange(P)).sum() == P // 2
        assert all(src[src[p]] == src[p] for src in s.values() for p in range(P))


# ---- the binding -------------------------------------------------------------------------------------------------------
def test_exported_symbols_dims_and_struct_layouts():
    L_ = evolve.load_library()
    assert set(evolve.EXPORTED_SYMBOLS) == {"rp_evolve_fold", "rp_evolve_plan", "rp_evolve_copy", "rp_evolve_dim",
                                            "rp_evolve_last_error"}
    assert [getattr(L_, s) for s in evolve.EXPORTED_SYMBOLS]
    assert evolve.dim("max_members") == evolve.MAX_MEMBERS == er.MAX_MEMBERS == 256
    assert evolve.dim("max_fields") == evolve.MAX_FIELDS == er.MAX_FIELDS == 64
    assert evolve.dim("chunk_words") == evolve.CHUNK_WORDS == er.CHUNK_WORDS == 4096
    assert evolve.dim("counter") == evolve.COUNTER == er.COUNTER == 96 and evolve.dim("wave_size") == er.WAVE == 64
    assert evolve.dim("nothing") == -1
    # the counter word is clear of the other kernels': the policy, the sampler, the targets, the critic and the actor steps
    used = list(range(3)) + list(range(16, 20)) + list(range(32, 40)) + list(range(48, 56)) + list(range(64, 67)) + list(range(80, 88))
    assert evolve.COUNTER not in used
    # the layouts of the header on the LP64 ABI
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "learn", "rp_evolve.h")).read()
    for name, value in (("MAX_MEMBERS", 256), ("MAX_COPY_MEMBERS", 65535), ("MAX_FIELDS", 64), ("CHUNK_WORDS", 4096), ("COUNTER", 96)):
        assert f"#define RP_EVOLVE_{name} {value}" in header
    assert ctypes.sizeof(evolve.Field) == 16 and ctypes.sizeof(evolve.FoldArgs) == 56
    assert ctypes.sizeof(evolve.PlanArgs) == 120 and ctypes.sizeof(evolve.CopyArgs) == 48
    offsets = lambda cls: {name: getattr(cls, name).offset for name, _ in cls._fields_}
    assert offsets(evolve.FoldArgs) == dict(struct_size=0, done_return=8, done_count=16, fit_sum=24, fit_count=32, E=40, P=44,
                                            hip_stream=48)
    assert offsets(evolve.PlanArgs) == dict(struct_size=0, fit_sum=8, fit_count=16, source=24, gamma=32, target_entropy=40,
                                            min_gap=48, min_episodes=56, up=64, down=68, gamma_lo=72, gamma_hi=76, entropy_lo=80,
                                            entropy_hi=84, seed_lo=88, seed_hi=92, generation=96, P=100, percent=104, hip_stream=112)
    assert offsets(evolve.CopyArgs) == dict(struct_size=0, fields=8, source=16, n_fields=24, P=28, launches=32, hip_stream=40)
    # the fields of each block in the header's order
    for struct, cls in (("rp_evolve_fold_args", evolve.FoldArgs), ("rp_evolve_plan_args", evolve.PlanArgs),
                        ("rp_evolve_copy_args", evolve.CopyArgs), ("rp_evolve_field", evolve.Field)):
        body = re.sub(r"/\*.*?\*/", "", header[header.index("typedef struct " + struct):header.index("} " + struct)], flags=re.S)
        at = [re.search(r"[ *]" + name + "[;,]", body).start() for name, _ in cls._fields_]   # (the declarators)
        assert at == sorted(at), struct
    for entry in ("fold", "plan", "copy"):
        a = evolve.make_args(entry)
        assert evolve.call_raw(entry, a) != 0 and "struct_size" not in evolve.last_error()
        a.struct_size -= 8
        assert evolve.call_raw(entry, a) != 0 and "struct_size" in evolve.last_error()
    from robopianist_amd import pop_critic
    assert not hasattr(pop_critic.load_library(), "rp_evolve_plan") and not hasattr(L_, "rp_pop_critic_step")


_A = 0x1000   # a non-null, 16-byte aligned address: a refused call never reads it


def _refused(entry, match, **values):
    args = evolve.make_args(entry, **values)
    assert evolve.call_raw(entry, args) != 0
    assert match in evolve.last_error(), evolve.last_error()
    assert evolve.last_error().startswith(f"rp_evolve_{entry}: ")


def test_argument_validation_refuses_before_any_launch():
    nan, inf = float("nan"), float("inf")
    fold = dict(done_return=_A, done_count=_A, fit_sum=_A, fit_count=_A, E=8, P=4)
    for name in ("done_return", "done_count", "fit_sum", "fit_count"):
        _refused("fold", "a pointer is NULL", **dict(fold, **{name: None}))
    for P in (0, -1):
        _refused("fold", "P must be >= 1", **dict(fold, P=P))
    for E in (0, -4, 6, 9):
        _refused("fold", "E must be a positive multiple of P", **dict(fold, E=E))
    plan = dict(fit_sum=_A, fit_count=_A, source=_A, gamma=_A, target_entropy=_A, min_gap=0.0, min_episodes=1, up=1.25, down=0.8,
                gamma_lo=0.0, gamma_hi=1.0, entropy_lo=-inf, entropy_hi=inf, seed_lo=1, seed_hi=2, generation=3, P=4, percent=25)
    for name in ("fit_sum", "fit_count", "source"):
        _refused("plan", "a pointer is NULL", **dict(plan, **{name: None}))
    for P in (0, -1, 257):
        _refused("plan", "P must be 1 .. 256", **dict(plan, P=P))
    for q in (-1, 101):
        _refused("plan", "percent must lie in [0, 100]", **dict(plan, percent=q))
    for n in (0, -3):
        _refused("plan", "min_episodes must be >= 1", **dict(plan, min_episodes=n))
    for gap in (-1e-300, -1.0, nan):
        _refused("plan", "min_gap must be >= 0", **dict(plan, min_gap=gap))
    for bad in (0.0, -1.0, nan):
        _refused("plan", "up must be > 0", **dict(plan, up=bad))
        _refused("plan", "down must be > 0", **dict(plan, down=bad))
    _refused("plan", "gamma_lo must be <= gamma_hi", **dict(plan, gamma_lo=0.5, gamma_hi=0.25))
    _refused("plan", "gamma_lo must be <= gamma_hi", **dict(plan, gamma_hi=nan))
    _refused("plan", "entropy_lo must be <= entropy_hi", **dict(plan, entropy_lo=1.0, entropy_hi=-1.0))
    _refused("plan", "entropy_lo must be <= entropy_hi", **dict(plan, entropy_lo=nan))
    table = lambda *rows: evolve.field_table(rows)
    copy = dict(fields=table((_A, 3), (_A + 4, 1)), source=_A, n_fields=2, P=4)
    _refused("copy", "source is NULL", **dict(copy, source=None))
    _refused("copy", "fields is NULL", **dict(copy, fields=None))
    for P in (0, -1, 65536):
        _refused("copy", "P must be 1 .. 65535", **dict(copy, P=P))
    _refused("copy", "n_fields must be >= 0", **dict(copy, n_fields=-1))
    _refused("copy", "field 1 has slice_words < 1", **dict(copy, fields=table((_A, 3), (_A, 0))))
    _refused("copy", "field 0 has slice_words < 1", **dict(copy, fields=table((_A, -2), (_A, 1))))
    _refused("copy", "field 1 has a NULL base", **dict(copy, fields=table((_A, 3), (None, 1))))
    for off in (1, 2, 3):
        _refused("copy", "field 1 has a base that is not 4-byte aligned", **dict(copy, fields=table((_A, 3), (_A + off, 1))))
    _refused("copy", "field 0 has a slice of more than 2^35 words", **dict(copy, fields=table((_A, 2 ** 35 + 1), (_A, 1))))
    # a bad field beyond the first launch's 64 is found before anything is launched
    rows = [(_A, 2)] * 70 + [(_A + 2, 2)]
    _refused("copy", "field 70 has a base that is not 4-byte aligned", **dict(copy, fields=table(*rows), n_fields=71))
    # accepted without a launch: no field (with or without a table), one member
    for values in (dict(copy, n_fields=0), dict(copy, n_fields=0, fields=None), dict(copy, P=1)):
        a = evolve.make_args("copy", launches=7, **values)
        assert evolve.call_raw("copy", a) == 0 and a.launches == 0
    assert evolve.copy([], _A, 4) == 0 and evolve.copy([(_A, 5)], _A, 1) == 0
    with pytest.raises(LearnError, match="rp_evolve_copy: field 0 has slice_words < 1"):
        evolve.copy([(_A, 0)], _A, 2)
    with pytest.raises(LearnError, match="rp_evolve_plan: percent"):
        evolve.plan(_A, _A, _A, 4, percent=200)
    with pytest.raises(LearnError, match="rp_evolve_fold: E must be"):
        evolve.fold(_A, _A, _A, _A, 7, 2)
    with pytest.raises(TypeError):
        evolve.make_args("plan", nothing=1)


# ---- the learner's option ------------------------------------------------------------------------------------------------
P_, E_ = 4, 8
KW = dict(hidden=(16, 32), n_critics=2, capacity=4, batch_size=8, utd=2, seed=3)
TODAY = {"actor", "critics", "targets", "log_alpha", "optimizers", "normalizer", "seed", "round", "n_written", "generator",
         "newest", "episodes", "droq", "members", "gamma", "target_entropy"}


def _pop(**kw):
    return population.DroQPopulation(_SpecEnv(E_, (4, 3), 3), P_, **dict(KW, **kw))


def test_option_validation():
    d = _pop(evolve={}).evolve_options
    assert d == dict(every=10, percent=25, min_episodes=1, min_gap=0.0, factors=(0.8, 1.25), gamma_bounds=(0.0, 0.9999),
                     entropy_bounds=(-math.inf, math.inf), explore=("gamma", "target_entropy"))
    assert d == population.EVOLVE_DEFAULTS and d is not population.EVOLVE_DEFAULTS
    o = _pop(evolve=dict(every=3, percent=50, min_episodes=2, min_gap=0.5, factors=[0.5, 2], gamma_bounds=[0.9, 0.99],
                         entropy_bounds=(-10, -1), explore="target_entropy")).evolve_options
    assert o == dict(every=3, percent=50, min_episodes=2, min_gap=0.5, factors=(0.5, 2.0), gamma_bounds=(0.9, 0.99),
                     entropy_bounds=(-10.0, -1.0), explore=("target_entropy",))
    assert _pop(evolve=dict(explore=())).evolve_options["explore"] == ()
    assert _pop(evolve=dict(explore=["target_entropy", "gamma"])).evolve_options["explore"] == ("gamma", "target_entropy")
    assert _pop(evolve=dict(percent=0)).evolve_options["percent"] == 0
    for bad, match in ((7, "evolve must be None or a dict"), ("on", "evolve must be None or a dict"),
                       (dict(often=2), "evolve has no option 'often'"), (dict(every=0), "every must be >= 1"),
                       (dict(every=2.5), "every must be an integer"), (dict(every=True), "every must be an integer"),
                       (dict(percent=-1), r"percent must lie in \[0, 100\]"), (dict(percent=101), r"percent must lie in \[0, 100\]"),
                       (dict(min_episodes=0), "min_episodes must be >= 1"), (dict(min_gap=-1.0), "min_gap must be >= 0"),
                       (dict(min_gap=float("nan")), "min_gap must be >= 0"), (dict(factors=(0.0, 1.25)), "factors must be"),
                       (dict(factors=(0.8, float("nan"))), "factors must be"), (dict(factors=0.8), "factors must be a pair"),
                       (dict(factors=(1, 2, 3)), "factors must be a pair"), (dict(gamma_bounds=(0.9, 0.5)), "gamma_bounds must be"),
                       (dict(entropy_bounds=(0.0, float("nan"))), "entropy_bounds must be"),
                       (dict(explore=("lr",)), 'evolve explores "gamma" and "target_entropy"')):
        with pytest.raises(ValueError, match=match):
            _pop(evolve=bad)
    # the option is independent of the critic mode; the fused actor step stays refused
    assert _pop(evolve={}, critic_step="fused").critic_mode == "fused"
    with pytest.raises(ValueError, match="DroQPopulation has no fused actor step yet"):
        _pop(evolve={}, actor_step="fused")


def test_without_the_option_nothing_changes():
    for mode in ("torch", "fused"):
        pop = _pop(critic_step=mode)
        assert pop.evolve_options is None
        assert set(pop.state_dict()) == TODAY | ({"critic_adam"} if mode == "fused" else set())
        assert not hasattr(pop, "_fit_sum") and not hasattr(pop, "generation")
        with pytest.raises(LearnError, match="evolve\\(\\) needs the population's evolve option"):
            pop.evolve()
        with pytest.raises(LearnError, match="needs the population's evolve option"):
            pop.last_evolution()
        assert type(pop).train is not population.ReplayLearner.train      # (the override; it defers without the option)
    on = _pop(evolve={})
    assert set(on.state_dict()) == TODAY | {"evolve"}
    assert (on.generation, on._evolve_rounds) == (0, 0) and on._source.tolist() == [0, 1, 2, 3]
    assert on._fit_sum.dtype == torch.float64 and on._fit_count.dtype == torch.int64 and on._source.dtype == torch.int32
    assert tuple(on._fit_sum.shape) == tuple(on._fit_count.shape) == tuple(on._source.shape) == (P_,)
    assert on.last_evolution().tolist() == [0, 1, 2, 3]


def _reachable(pop):
    """Every tensor with a leading dimension of P that a member owns a slice of, found without `_member_fields()`: the
    parameters of the networks and the targets, log_alpha, the normaliser, the fused step's Adam state and whatever the
    three torch optimisers hold."""
    found = list(pop.actor.parameters()) + [t for net in pop.critics + pop.targets for t in net.parameters()] + [pop.log_alpha]
    found += [pop._mean, pop._M2, pop._mean_f32, pop._inv_std_f32]
    for k in ("_c_m", "_c_v"):
        found += [t for net in getattr(pop, k, []) for t in net]
    for name in ("actor", "critic", "alpha"):
        for state in getattr(pop, name + "_optimizer").state.values():
            found += [v for v in state.values() if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == pop.P]
    assert all(t.shape[0] == pop.P for t in found)
    return found


def _complete(pop):
    fields = pop._member_fields()
    names, tensors = [n for n, _ in fields], [t for _, t in fields]
    assert len(set(names)) == len(names)
    assert sorted(t.data_ptr() for t in tensors) == sorted(t.data_ptr() for t in _reachable(pop))
    assert len({t.data_ptr() for t in tensors}) == len(tensors)                          # exactly once
    table = pop._field_table()
    assert [base for base, _ in table] == [t.data_ptr() for t in tensors]
    assert [words for _, words in table] == [t.numel() // pop.P * t.element_size() // 4 for t in tensors]
    assert not {pop.gamma.data_ptr(), pop.target_entropy.data_ptr()} & {t.data_ptr() for t in tensors}
    return dict(fields)


def test_the_field_table_is_complete():
    D, A, H1, H2 = 7, 3, 16, 32
    pop = _pop(evolve={})
    f = _complete(pop)
    n0 = 6 + 2 * 10 + 2 * 10 + 1 + 4
    assert len(f) == n0
    words = lambda name: f[name][0].numel() * f[name].element_size() // 4
    assert words("actor.0") == H1 * D and words("actor.5") == 2 * A and words("critics.1.0") == H1 * (D + A)
    assert words("targets.0.4") == H2 and words("targets.1.9") == H2 and words("log_alpha") == 1
    assert words("_mean") == words("_M2") == 2 * D and words("_mean_f32") == words("_inv_std_f32") == D   # (float64: two words)
    # a torch step of each optimiser: the table grows by their moments
    rng = np.random.default_rng(0)
    t = lambda *shape: torch.as_tensor(rng.normal(size=shape).astype(np.float32))
    batch = {"obs": t(P_, 8, D), "action": torch.tanh(t(P_, 8, A)), "y": t(P_, 8), "mask": torch.ones(P_, 8)}
    pop.critic_step(batch)
    assert len(_complete(pop)) == n0 + 2 * 20
    pop.actor_step(batch)
    f = _complete(pop)
    assert len(f) == n0 + 2 * (20 + 6 + 1)
    assert tuple(f["alpha_optimizer.0.exp_avg"].shape) == (P_,) and tuple(f["actor_optimizer.0.exp_avg_sq"].shape) == (P_, H1, D)
    # the fused critic step owns m and v from the start; torch's critic optimiser stays empty
    fused = _pop(evolve={}, critic_step="fused")
    f = _complete(fused)
    assert len(f) == n0 + 2 * 20 and tuple(f["_c_m.1.0"].shape) == (P_, H1, D + A) and "_c_v.0.9" in f
    # a table of 85 or 95 fields: more than one launch of 64
    assert evolve.launches_for(len(f)) == 2


def test_the_checkpoint_round_trip_and_the_refusal_of_the_other_setting():
    a = _pop(evolve=dict(every=2, percent=50))
    a.generation, a._evolve_rounds = 3, 7
    a._fit_sum.copy_(torch.tensor([1.5, -2.0, 0.0, 8.0], dtype=torch.float64))
    a._fit_count.copy_(torch.tensor([2, 1, 0, 2 ** 40]))
    a._source.copy_(torch.tensor([0, 0, 2, 2], dtype=torch.int32))
    a.gamma.copy_(torch.tensor([0.9, 0.91, 0.92, 0.93]))
    sd = a.state_dict()
    assert set(sd["evolve"]) == {"options", "generation", "rounds", "fit_sum", "fit_count", "source"}
    assert sd["evolve"]["options"] == a.evolve_options and sd["evolve"]["options"] is not a.evolve_options
    a._fit_sum.zero_()
    assert sd["evolve"]["fit_sum"].tolist() == [1.5, -2.0, 0.0, 8.0]                     # a snapshot, not a view
    b = _pop(evolve=dict(every=2, percent=50), seed=9)
    b.load_state_dict(sd)
    assert (b.generation, b._evolve_rounds) == (3, 7) and b._fit_sum.tolist() == [1.5, -2.0, 0.0, 8.0]
    assert b._fit_count.tolist() == [2, 1, 0, 2 ** 40] and b.last_evolution().tolist() == [0, 0, 2, 2]
    assert torch.equal(b.gamma, a.gamma)
    off = _pop()
    with pytest.raises(ValueError, match="the checkpoint was written with evolve = {'every': 2.*, this population has evolve = None"):
        off.load_state_dict(sd)
    with pytest.raises(ValueError, match="the checkpoint was written with evolve = None, this population has evolve = {'every': 2"):
        b.load_state_dict(off.state_dict())
    with pytest.raises(ValueError, match="the checkpoint was written with evolve = .*'percent': 50.* has evolve = .*'percent': 25"):
        _pop(evolve=dict(every=2)).load_state_dict(sd)
    off.load_state_dict(_pop(seed=9).state_dict())                                         # today's checkpoint loads as today
