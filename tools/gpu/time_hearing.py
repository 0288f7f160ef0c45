"""Cost of the audio observation per control step (bench.py is left as it is).

4096 envs, n_sub = 10, the default analysis (16 kHz, W = 2048, 88 bins).  The key trace and the sustain flag of every
control step of the TwinkleTwinkle scripted replay are recorded from one env (158 control steps); env e then plays that
recording from step 7 e mod 158 on, round and round, so the banks hold what a played episode leaves in them and the
envs are out of phase.  One pass over the recording warms up and fills the banks; then `observe` (rp_hear_track +
rp_hear_spectrum), and the two calls on their own, are timed with device events in windows of at least `--seconds`,
the workloads alternating in one process.

Writes profiles/hearing_timing.json: ms per call, and the arithmetic the calls need (from the shapes and the mean number
of voices that can sound in a window) over that time.

    python tools/gpu/time_hearing.py [--envs 4096] [--windows 3] [--out profiles/hearing_timing.json]
"""
import argparse
import itertools
import os

import torch

from _measure import ROOT, Times, event_time, load_twinkle, scripted_replay, write_report


def record_replay_steps():
    """(rows [n_steps][n_sub][4] int32, sustain [n_steps] int32, dt) of env 0 over the scripted replay."""
    base = load_twinkle(2, record_key_trace=True, control_timestep=0.05, primitive_fingertip_collisions=True)
    env, script, n_steps = scripted_replay(base)
    env.reset()
    rows, sustain = [], []
    for _ in range(n_steps):
        ts = env.step(script)
        rows.append(base.key_trace[0].clone())
        sustain.append(base.task.piano.sustain_activation[0, 0].to(torch.int32))
        if bool(ts.last()[0]):
            break
    return torch.stack(rows), torch.stack(sustain), float(base.task.physics_timestep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hearing_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_hearing.py needs the GPU: there is no CPU path to time")
    from robopianist_amd.music import hearing

    rows, sustain, dt = record_replay_steps()
    n_steps, n_sub = int(rows.shape[0]), int(rows.shape[1])
    E, dev = args.envs, rows.device
    h = hearing.Hearing(E, physics_timestep=dt, max_substeps_per_call=n_sub)
    start = (7 * torch.arange(E, device=dev)) % n_steps
    # every step's batch is made before the clock starts: the gather is not part of the observation
    traces = [rows[(start + t) % n_steps].contiguous() for t in range(n_steps)]
    pedals = [sustain[(start + t) % n_steps].contiguous() for t in range(n_steps)]
    for t in range(n_steps):   # warm-up: every kernel has run, the banks are what an episode leaves
        h.observe(traces[t], pedal=pedals[t])
    torch.cuda.synchronize()
    forgotten = int(h.forgotten.sum())

    def audible_voices():
        """Mean number of bank voices per env that can sound in the current window (t_off + 8 tau_rel after its start)."""
        t_end = h.substeps.to(torch.float64) * dt
        t_start = t_end - (h.window - 1) / float(h.sample_rate)
        tail = 8.0 * float(h.timbre["tau_rel"])
        live = (h.t_on >= 0) & (h.t_on <= t_end[:, None, None]) & (h.t_off + tail > t_start[:, None, None])
        return float(live.sum()) / E
    voices = audible_voices()

    spec_args = h.spectrum_args(h.outputs()[0])

    def run(which, t):
        if which == "observe":
            h.observe(traces[t % n_steps], pedal=pedals[t % n_steps])
        elif which == "track":
            h.track(traces[t % n_steps], pedal=pedals[t % n_steps])
        else:   # the bank as the last track left it
            if h.spectrum_raw(spec_args) != 0:
                raise RuntimeError(h.last_error())

    def measure(which, calls):
        """ms per call of `calls` calls of the workload, at steps 0, 1, ... of the recording."""
        t = itertools.count()
        return event_time(lambda: run(which, next(t)), calls)

    names = ("observe", "track", "spectrum")
    calls = {}
    for w in names:   # size every window to --seconds from a short probe
        ms = measure(w, 20)
        calls[w] = max(20, int(args.seconds * 1000.0 / ms))
    ms = {w: [] for w in names}
    for _ in range(args.windows):
        for w in names:
            ms[w].append(measure(w, calls[w]))
    med = Times(ms).median

    W, B, H = h.window, h.n_bins, int(h.timbre["H"])
    analysis_flop = 2.0 * E * W * 2 * B
    # per voice-partial and sample the phasor step is 4 fused multiply-adds and one add: 9 flop (the closed form at a
    # thread's first sample and the per-voice gains are not counted)
    window_flop = 9.0 * E * voices * H * W
    result = {
        "tool": "tools/gpu/time_hearing.py",
        "workload": f"{E} envs, n_sub {n_sub}, dt {dt}, default analysis ({h.sample_rate} Hz, W {W}, B {B}), banks from the "
                    f"TwinkleTwinkle scripted replay ({n_steps} control steps, env e starts at step 7 e mod {n_steps})",
        "device": torch.cuda.get_device_name(0),
        "timing": f"device events, median of {args.windows} windows of >= {args.seconds} s per workload, alternating, after "
                  f"one pass of {n_steps} calls",
        "calls_per_window": calls,
        "ms_per_call": med,
        "ms_per_call_windows": ms,
        "forgotten_voices_after_warm_up": forgotten,
        "mean_voices_per_env_that_can_sound_in_the_window": voices,
        "analysis_gflop_per_call": analysis_flop / 1e9,
        "window_gflop_per_call_phasor_steps_only": window_flop / 1e9,
        "spectrum_tflops_counted": (analysis_flop + window_flop) / (med["spectrum"] * 1e-3) / 1e12,
    }
    write_report(result, args.out)


if __name__ == "__main__":
    main()
