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
import os

import torch

from _measure import HANDS, ROOT, alternate, event_window, load_twinkle, staggered_replay, write_report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=3, help="timed windows per workload (each at least --seconds long)")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    args = ap.parse_args()

    E = args.envs
    base = load_twinkle(E, **HANDS, primitive_fingertip_collisions=False,   # hull fingertips, as bench.py's config 2
                        change_color_on_activation=True)
    phys, task = base.physics, base.task
    dev = phys.device
    env, script, _ = staggered_replay(base)

    def step_only():
        env.step(script)

    def step_and_render():
        env.step(script)
        phys.render(84, 84, "piano/back", key_rgb=task.key_rgb(phys), colorize_fingertips=task.colorize_fingertips)

    def render_only():
        phys.render(84, 84, "piano/back", key_rgb=task.key_rgb(phys), colorize_fingertips=task.colorize_fingertips)

    work = {"step": step_only, "step_render": step_and_render, "render": render_only}
    for fn in work.values():   # warm-up (allocations, the renderer's creation)
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    measure = lambda fn: event_window(fn, args.seconds)
    times = alternate(work, args.windows, measure, warm=False)
    med, res = times.median, times.windows

    # 64 envs, 240 x 320 (dm_control's default image size)
    small = load_twinkle(64, seed=1, primitive_fingertip_collisions=False)
    small.reset()
    big = lambda: small.physics.render(240, 320, "piano/back")
    for _ in range(5):
        big()
    torch.cuda.synchronize()
    big_ms = alternate({"big": big}, args.windows, measure, warm=False).median["big"]

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
    write_report(out, args.out, printed={k: v for k, v in out.items() if k != "windows_ms"})


if __name__ == "__main__":
    main()
