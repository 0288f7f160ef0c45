"""The one copy of what the timing scripts of this directory share: the task load, the scripted replay, the two timers
(a host clock between two synchronises; device events around a window of calls), the window schedule, the statistics of
the windows with the overlap criterion, and the report writer.

The scripts run as `python tools/gpu/x.py`, so `import _measure` finds this file next to them.  torch and the package are
imported where they are first needed: the statistics, the schedule and the loops (with their clocks injected) run on a
machine without a GPU, which is how tests/test_measure_host.py drives them.
"""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TWINKLE = "RoboPianist-debug-TwinkleTwinkleRousseau-v0"
# the task keywords of bench.py's configs 2 and 3 (on top of the two every load shares)
HANDS = dict(control_timestep=0.05, reduced_action_space=False, n_steps_lookahead=10)


def load_twinkle(n_envs, *, seed=12345, precision=None, record_key_trace=None, **task_kwargs):
    """suite.load of the TwinkleTwinkle task with n_envs envs; task_kwargs go on top of the two keywords every caller
    shares, precision and record_key_trace are passed only where given."""
    from robopianist_amd import suite
    extra = {k: v for k, v in (("precision", precision), ("record_key_trace", record_key_trace)) if v is not None}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return suite.load(TWINKLE, seed=seed, n_envs=n_envs, **extra,
                          task_kwargs=dict(trim_silence=True, gravity_compensation=True, **task_kwargs))


def scripted_replay(base):
    """(CanonicalSpecWrapper of base, the ScriptedActions of the recorded TwinkleTwinkle replay, its length T)."""
    import torch
    from robopianist_amd.suite.scripted import ScriptedActions
    from robopianist_amd.wrappers import CanonicalSpecWrapper
    phys = base.physics
    actions = np.load(os.path.join(ROOT, "tests", "golden", "twinkle_twinkle_actions.npy"))
    script = ScriptedActions(torch.as_tensor(actions, dtype=phys.dtype, device=phys.device),
                             torch.zeros(base.n_envs, dtype=torch.long, device=phys.device))
    return CanonicalSpecWrapper(base), script, actions.shape[0]


def staggered_replay(base):
    """scripted_replay(base) after a reset and T untimed steps that leave env e at e mod T steps into its episode, as
    bench.py staggers it."""
    import torch
    env, script, T = scripted_replay(base)
    env.reset()
    phase = torch.arange(base.n_envs, device=base.physics.device) % T
    for j in range(T):   # untimed prologue: spreads the envs over the episode
        base.request_reset(phase == (T - 1 - j))
        env.step(script)
    return env, script, T


def host_time(fn, repeat=1, *, sync=None, clock=None):
    """Seconds for `repeat` calls of fn, by a host clock between two device synchronises."""
    if sync is None:
        import torch
        sync = torch.cuda.synchronize
    clock = clock or time.perf_counter
    sync()
    t0 = clock()
    for _ in range(repeat):
        fn()
    sync()
    return clock() - t0


def host_per_call(item):
    """Seconds per call of item = (fn, n), where one fn() makes n calls: what the learner scripts hand to alternate()."""
    fn, n = item
    return host_time(fn) / n


def _torch_events():
    import torch
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def _elapsed_ms(fn, n, events):
    a, b = events()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def event_time(fn, calls):
    """ms per call of `calls` back-to-back calls of fn, by one pair of device events."""
    return _elapsed_ms(fn, calls, _torch_events) / calls


def event_window(fn, seconds, first=8, *, events=None):
    """ms per call over a window of at least `seconds`: batches of first, 2 first, 4 first, ... calls, each between a
    pair of device events, until the batches' times add up to the window."""
    events = events or _torch_events
    n, calls, total = first, 0, 0.0
    while total < seconds * 1e3:
        total += _elapsed_ms(fn, n, events); calls += n
        n *= 2
    return total / calls


class Times:
    """The windows of every workload with their median, lowest and highest (`windows` maps name -> list of figures;
    recorded windows do as well as measured ones)."""

    def __init__(self, windows):
        self.windows = dict(windows)
        self.median = {k: float(np.median(v)) for k, v in self.windows.items()}
        self.lowest = {k: float(min(v)) for k, v in self.windows.items()}
        self.highest = {k: float(max(v)) for k, v in self.windows.items()}

    def spread(self, k):
        return [float(self.lowest[k] / self.median[k]), float(self.highest[k] / self.median[k])]

    def stat(self, k, scale):
        return {"median": scale * self.median[k], "lowest": scale * self.lowest[k], "highest": scale * self.highest[k]}

    def apart(self, a, b):
        """a's slowest window below b's fastest: the medians differ by more than both spreads."""
        return bool(self.highest[a] < self.lowest[b])

    def verdict(self, a, b):
        return "faster" if self.apart(a, b) else "slower" if self.apart(b, a) else "windows overlap"


def alternate(work, windows, measure, warm=True):
    """Times of measure(work[name]) over `windows` rounds through the workloads in their order, after one discarded
    measure of each (the warm-up of every shape)."""
    if warm:
        for item in work.values():
            measure(item)
    times = {k: [] for k in work}
    for _ in range(windows):
        for k, item in work.items():
            times[k].append(measure(item))
    return Times(times)


def write_report(report, path, *, printed=None, indent=None):
    """Saves the report, then prints it (or `printed`, the trimmed mapping of a script that stores its windows)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report if printed is None else printed, indent=indent))
