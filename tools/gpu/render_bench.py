"""Cost of the camera renderer next to the env step it serves (bench.py is left as it is).

Config 2 (TwinkleTwinkle scripted replay, hull fingertips) at 4096 envs, staggered as bench.py staggers it (env e is
e mod T steps into its episode).  Timed with device events after a warm-up, in windows of at least a second, the two
workloads alternating in one process:

    A  env.step
    B  env.step + render(84, 84, "piano/back")  (with task.key_rgb, as PixelWrapper calls it)

plus a 64-env 240 x 320 render on its own.  Writes profiles/render_bench.json (ms per call, images/s, pixels/s).

    python tools/gpu/render_bench.py [--envs 4096] [--windows 3] [--out profiles/render_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/gpu/render_bench.py --windows 1 --seconds 0.3
        (kernel table: profiles/render_kernel_stats.csv)
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=3, help="timed windows per workload (each at least --seconds long)")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    args = ap.parse_args()

    from robopianist_amd import suite
    from robopianist_amd.suite.scripted import ScriptedActions
    from robopianist_amd.wrappers import CanonicalSpecWrapper
    E = args.envs
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = suite.load("RoboPianist-debug-TwinkleTwinkleRousseau-v0", seed=12345, n_envs=E,
                          task_kwargs=dict(trim_silence=True, control_timestep=0.05, gravity_compensation=True,
                                           reduced_action_space=False, n_steps_lookahead=10,
                                           primitive_fingertip_collisions=False,   # hull fingertips, as bench.py's config 2
                                           change_color_on_activation=True))
    env = CanonicalSpecWrapper(base)
    phys, task = base.physics, base.task
    dev = phys.device
    actions = np.load(os.path.join(ROOT, "tests", "golden", "twinkle_twinkle_actions.npy"))
    T = actions.shape[0]
    script = ScriptedActions(torch.as_tensor(actions, dtype=phys.dtype, device=dev),
                             torch.zeros(E, dtype=torch.long, device=dev))
    env.reset()
    phase = torch.arange(E, device=dev) % T
    for j in range(T):   # untimed prologue: spreads the envs over the episode
        base.request_reset(phase == (T - 1 - j))
        env.step(script)

    def step_only():
        env.step(script)

    def step_and_render():
        env.step(script)
        phys.render(84, 84, "piano/back", key_rgb=task.key_rgb(phys), colorize_fingertips=task.colorize_fingertips)

    def render_only():
        phys.render(84, 84, "piano/back", key_rgb=task.key_rgb(phys), colorize_fingertips=task.colorize_fingertips)

    def window(fn, seconds):
        """ms per call over a window of at least `seconds` (device events around the whole window)."""
        n, calls, total = 8, 0, 0.0
        while total < seconds * 1e3:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                fn()
            b.record()
            b.synchronize()
            total += a.elapsed_time(b); calls += n
            n *= 2
        return total / calls

    for fn in (step_only, step_and_render, render_only):   # warm-up (allocations, the renderer's creation)
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    res = {"step": [], "step_render": [], "render": []}
    for _ in range(args.windows):   # alternating
        res["step"].append(window(step_only, args.seconds))
        res["step_render"].append(window(step_and_render, args.seconds))
        res["render"].append(window(render_only, args.seconds))
    med = {k: float(np.median(v)) for k, v in res.items()}

    # 64 envs, 240 x 320 (dm_control's default image size)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        small = suite.load("RoboPianist-debug-TwinkleTwinkleRousseau-v0", seed=1, n_envs=64,
                           task_kwargs=dict(trim_silence=True, gravity_compensation=True,
                                            primitive_fingertip_collisions=False))
    small.reset()
    big = lambda: small.physics.render(240, 320, "piano/back")
    for _ in range(5):
        big()
    torch.cuda.synchronize()
    big_ms = float(np.median([window(big, args.seconds) for _ in range(args.windows)]))

    out = {
        "device": torch.cuda.get_device_name(dev),
        "workload": f"config 2 (TwinkleTwinkle scripted replay, hull fingertips), {E} envs, staggered, fp64",
        "method": f"device events, {args.windows} windows of >= {args.seconds} s per workload, alternating; medians",
        "env_step_ms": med["step"],
        "env_step_plus_render_84x84_ms": med["step_render"],
        "render_84x84_alone_ms": med["render"],
        "render_84x84_added_ms": med["step_render"] - med["step"],
        "render_84x84_images_per_s": E / (med["render"] * 1e-3),
        "render_84x84_pixels_per_s": E * 84 * 84 / (med["render"] * 1e-3),
        "windows_ms": res,
        "render_240x320_64envs_ms": big_ms,
        "render_240x320_images_per_s": 64 / (big_ms * 1e-3),
        "render_240x320_pixels_per_s": 64 * 240 * 320 / (big_ms * 1e-3),
        "camera": "piano/back", "includes": "task.key_rgb (torch) + rp_render (two launches)",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "windows_ms"}))


if __name__ == "__main__":
    main()
