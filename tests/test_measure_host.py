"""tools/gpu/_measure.py on the CPU: the two timing loops under a fake clock and fake events, the window schedule, the
statistics against the windows stored in profiles/, the overlap criterion, the report writer and the task load."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "gpu"))
import _measure  # noqa: E402
from _measure import Times  # noqa: E402


def profile(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        return json.load(f)


# ---- host_time

@pytest.mark.parametrize("repeat", [1, 3])
def test_host_time_syncs_around_all_calls_and_returns_the_clock_difference(repeat):
    log = []
    ticks = iter([10.0, 12.5])

    def clock():
        log.append("clock")
        return next(ticks)

    seconds = _measure.host_time(lambda: log.append("fn"), repeat, sync=lambda: log.append("sync"), clock=clock)
    assert seconds == 2.5
    assert log == ["sync", "clock"] + ["fn"] * repeat + ["sync", "clock"]


def test_host_time_default_repeat_is_one_call():
    calls = []
    ticks = iter([0.0, 1.0])
    assert _measure.host_time(lambda: calls.append(1), sync=lambda: None, clock=lambda: next(ticks)) == 1.0
    assert len(calls) == 1


def test_host_per_call_divides_by_the_calls_one_fn_makes(monkeypatch):
    monkeypatch.setattr(_measure, "host_time", lambda fn: 3.0)
    assert _measure.host_per_call((None, 200)) == 3.0 / 200


# ---- event_window

class FakeEvents:
    """An event-pair factory whose k-th pair reports the k-th scripted elapsed time."""

    def __init__(self, elapsed_ms, log):
        self.elapsed_ms, self.log = iter(elapsed_ms), log

    def __call__(self):
        return _FakeEvent(self, "a"), _FakeEvent(self, "b")


class _FakeEvent:
    def __init__(self, owner, name):
        self.owner, self.name = owner, name

    def record(self):
        self.owner.log.append(self.name + ".record")

    def synchronize(self):
        self.owner.log.append(self.name + ".synchronize")

    def elapsed_time(self, other):
        assert (self.name, other.name) == ("a", "b")
        return next(self.owner.elapsed_ms)


def batches(log):
    """The numbers of fn calls between each a.record and b.record, b.synchronize."""
    out, text = [], " ".join(log)
    for part in text.split("a.record")[1:]:
        body, tail = part.split("b.record")
        assert tail.strip() == "b.synchronize"
        out.append(body.split().count("fn"))
    return out


def test_event_window_doubles_until_the_window_is_full():
    log = []
    ms = _measure.event_window(lambda: log.append("fn"), 0.1, events=FakeEvents([20.0, 30.0, 49.0, 1.0, 1e9], log))
    assert batches(log) == [8, 16, 32, 64]            # 20, 50, 99 < 100; 100 >= 100 stops
    assert ms == (20.0 + 30.0 + 49.0 + 1.0) / (8 + 16 + 32 + 64)


def test_event_window_stops_after_a_first_batch_that_fills_it():
    log = []
    ms = _measure.event_window(lambda: log.append("fn"), 0.1, events=FakeEvents([250.0, 1e9], log))
    assert batches(log) == [8]
    assert ms == 250.0 / 8


def test_event_window_first():
    log = []
    ms = _measure.event_window(lambda: log.append("fn"), 1.0, first=2, events=FakeEvents([400.0, 700.0, 1e9], log))
    assert batches(log) == [2, 4]
    assert ms == 1100.0 / 6


# ---- alternate

def test_alternate_warms_every_workload_once_then_goes_round_in_order():
    seen = []
    figures = iter(range(100))

    def measure(item):
        seen.append(item)
        return float(next(figures))

    t = _measure.alternate({"a": "A", "b": "B", "c": "C"}, 2, measure)
    assert seen == ["A", "B", "C"] + ["A", "B", "C"] * 2
    assert t.windows == {"a": [3.0, 6.0], "b": [4.0, 7.0], "c": [5.0, 8.0]}     # the warm-up's 0, 1, 2 are discarded
    assert list(t.windows) == ["a", "b", "c"]


def test_alternate_without_warm_up():
    seen = []
    t = _measure.alternate({"a": 1, "b": 2}, 3, lambda item: seen.append(item) or float(item), warm=False)
    assert seen == [1, 2] * 3
    assert t.windows == {"a": [1.0] * 3, "b": [2.0] * 3}


# ---- Times against the committed record: exact, the arithmetic is the one that wrote the files

def test_times_reproduce_pop_bench():
    p = profile("pop_bench.json")
    t = Times(p["seconds_per_call_windows"])
    assert len(p["spread"]) == 32 and set(p["spread"]) == set(t.windows)
    for k in p["spread"]:
        assert t.spread(k) == p["spread"][k]
    assert 1e6 * t.median["sac_act"] == p["single_learner"]["sac_act_us"]
    assert t.stat("sac_act", 1e6)["median"] == p["single_learner"]["sac_act_us"]


def test_times_reproduce_render_ik_plan_and_hearing():
    p = profile("render_bench.json")
    t = Times(p["windows_ms"])
    assert t.median["step"] == p["env_step_ms"] and t.median["render"] == p["render_84x84_alone_ms"]
    p = profile("ik_bench.json")
    assert Times(p["windows_ms"]).median["solve_k1"] == p["solve_k1_ms"]
    p = profile("plan_bench.json")
    t = Times({k: [w[k] for w in p["windows"]] for k in p["windows"][0]})
    assert p["median"] and t.median == p["median"]
    p = profile("hearing_timing.json")
    assert Times(p["ms_per_call_windows"]).median == p["ms_per_call"]


def test_times_figures_are_plain_floats():
    t = Times({"a": [3, 1, 2]})
    assert (t.median["a"], t.lowest["a"], t.highest["a"]) == (2.0, 1.0, 3.0)
    assert all(type(v["a"]) is float for v in (t.median, t.lowest, t.highest))
    assert t.spread("a") == [0.5, 1.5]
    assert t.stat("a", 1e3) == {"median": 2000.0, "lowest": 1000.0, "highest": 3000.0}


# ---- apart / verdict

def test_apart_and_verdict():
    t = Times({"fast": [1.0, 1.1, 1.2], "slow": [1.3, 1.4, 1.5], "touch": [1.2, 1.25, 1.3], "wide": [0.9, 1.25, 1.6]})
    assert t.apart("fast", "slow") is True and t.apart("slow", "fast") is False
    assert t.verdict("fast", "slow") == "faster" and t.verdict("slow", "fast") == "slower"
    # touching: highest[fast] == lowest[touch], highest[touch] == lowest[slow]
    assert t.apart("fast", "touch") is False and t.apart("touch", "slow") is False
    assert t.verdict("fast", "touch") == t.verdict("touch", "fast") == "windows overlap"
    # overlapping
    for k in ("fast", "slow", "touch"):
        assert not t.apart(k, "wide") and not t.apart("wide", k)
        assert t.verdict(k, "wide") == "windows overlap"


# ---- write_report

REPORT = {"a": 1, "windows": {"x": [1.0, 2.0]}}


@pytest.mark.parametrize("path", ["result.json", os.path.join("new", "deeper", "result.json")])
def test_write_report_makes_the_directory_and_ends_with_one_newline(tmp_path, monkeypatch, capsys, path):
    monkeypatch.chdir(tmp_path)
    _measure.write_report(REPORT, path)
    text = (tmp_path / path).read_text()
    assert json.loads(text) == REPORT
    assert text == json.dumps(REPORT, indent=1) + "\n"
    assert text.endswith("}\n") and not text.endswith("\n\n")
    assert capsys.readouterr().out == json.dumps(REPORT) + "\n"


def test_write_report_prints_the_trimmed_mapping_with_the_given_indent(tmp_path, capsys):
    path = tmp_path / "out" / "r.json"
    _measure.write_report(REPORT, str(path), printed={"a": 1}, indent=1)
    assert json.loads(path.read_text()) == REPORT
    assert capsys.readouterr().out == json.dumps({"a": 1}, indent=1) + "\n"


# ---- load_twinkle: the keyword sets the scripts passed before they shared it, written out

def recorded_load(monkeypatch):
    from robopianist_amd import suite
    calls = []
    monkeypatch.setattr(suite, "load", lambda *a, **kw: calls.append((a, kw)) or "env")
    return calls


def test_load_twinkle_learner_family(monkeypatch):
    calls = recorded_load(monkeypatch)
    assert _measure.load_twinkle(4096, precision=64, **_measure.HANDS) == "env"
    assert calls == [(("RoboPianist-debug-TwinkleTwinkleRousseau-v0",), dict(
        seed=12345, n_envs=4096, precision=64,
        task_kwargs=dict(trim_silence=True, control_timestep=0.05, gravity_compensation=True,
                         reduced_action_space=False, n_steps_lookahead=10)))]


def test_load_twinkle_render_bench(monkeypatch):
    calls = recorded_load(monkeypatch)
    _measure.load_twinkle(4096, **_measure.HANDS, primitive_fingertip_collisions=False, change_color_on_activation=True)
    _measure.load_twinkle(64, seed=1, primitive_fingertip_collisions=False)
    assert calls == [
        (("RoboPianist-debug-TwinkleTwinkleRousseau-v0",), dict(
            seed=12345, n_envs=4096,
            task_kwargs=dict(trim_silence=True, control_timestep=0.05, gravity_compensation=True,
                             reduced_action_space=False, n_steps_lookahead=10, primitive_fingertip_collisions=False,
                             change_color_on_activation=True))),
        (("RoboPianist-debug-TwinkleTwinkleRousseau-v0",), dict(
            seed=1, n_envs=64,
            task_kwargs=dict(trim_silence=True, gravity_compensation=True, primitive_fingertip_collisions=False)))]


def test_load_twinkle_recording_load(monkeypatch):
    calls = recorded_load(monkeypatch)
    _measure.load_twinkle(2, record_key_trace=True, control_timestep=0.05, primitive_fingertip_collisions=True)
    assert calls == [(("RoboPianist-debug-TwinkleTwinkleRousseau-v0",), dict(
        seed=12345, n_envs=2, record_key_trace=True,
        task_kwargs=dict(trim_silence=True, control_timestep=0.05, gravity_compensation=True,
                         primitive_fingertip_collisions=True)))]
