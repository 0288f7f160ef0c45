"""Cost of the JPEG encoder next to the render of the same images (bench.py is left as it is).

Three workloads on the TwinkleTwinkle scene after a few control steps of the scripted replay, so the images are what a
recording holds (hands over the keys): 4096 frames of 84 x 84, 64 frames of 240 x 320, 4 frames of 480 x 640, camera
piano/back, quality 90.  Per workload, timed with device events after a warm-up, in windows of at least `--seconds`,
the two alternating in one process:

    A  physics.render(H, W)               (with task.key_rgb, as the wrappers call it)
    B  Encoder.encode(rendered images)    (the four launches of rp_video_encode; no read-back)

Writes profiles/video_bench.json: ms per call, frames/s, input and output MB/s, bytes per frame.

    python tools/gpu/video_bench.py [--windows 3] [--seconds 0.5] [--out profiles/video_bench.json]
"""
import argparse
import json
import os

import numpy as np
import torch

from _measure import ROOT, alternate, event_window, load_twinkle, scripted_replay

WORKLOADS = ((4096, 84, 84), (64, 240, 320), (4, 480, 640))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3, help="timed windows per workload (each at least --seconds long)")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_bench.json"))
    args = ap.parse_args()

    results = []
    for E, H, W in WORKLOADS:
        base = load_twinkle(E, control_timestep=0.05, primitive_fingertip_collisions=True, change_color_on_activation=True)
        phys, task = base.physics, base.task
        env, script, _ = scripted_replay(base)
        env.reset()
        for _ in range(40):   # untimed: the hands are over the keys, some keys are down and coloured
            env.step(script)
        enc = phys.jpeg_encoder(H, W, E, args.quality)

        def render():
            return phys.render(H, W, "piano/back", key_rgb=task.key_rgb(phys), colorize_fingertips=task.colorize_fingertips)

        rgb = render()

        def encode():
            enc.encode(rgb)

        for fn in (render, encode):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = alternate({"render": render, "encode": encode}, args.windows,
                          lambda fn: event_window(fn, args.seconds, first=4), warm=False)
        _, length = enc.encode(rgb)
        n = length.cpu().numpy().astype(np.int64)
        assert (n > 0).all()
        r, e = times.median["render"], times.median["encode"]
        results.append({
            "frames": E, "height": H, "width": W, "quality": args.quality,
            "render_ms": r, "encode_ms": e, "encode_over_render": e / r,
            "encode_frames_per_s": E / (e * 1e-3),
            "encode_input_MB_per_s": E * H * W * 3 / (e * 1e-3) / 1e6,
            "encode_output_MB_per_s": float(n.sum()) / (e * 1e-3) / 1e6,
            "bytes_per_frame_mean": float(n.mean()), "bytes_per_frame_max": int(n.max()), "bytes_cap": enc.max_bytes,
            "compression": E * H * W * 3 / float(n.sum()),
            "windows_ms": times.windows,
        })
        del env, base, enc, rgb
        torch.cuda.empty_cache()
    out = {
        "device": torch.cuda.get_device_name(0),
        "scene": "TwinkleTwinkle scripted replay after 40 control steps, camera piano/back, task.key_rgb",
        "method": f"device events, {args.windows} windows of >= {args.seconds} s per workload, alternating; medians",
        "encode": "rp_video_encode: transform, sizing, layout and writing launches; no read-back",
        "workloads": results,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:   # (its own writer: one printed line per workload, not the report)
        json.dump(out, f, indent=1)
        f.write("\n")
    for w in results:
        print(json.dumps({k: v for k, v in w.items() if k != "windows_ms"}))


if __name__ == "__main__":
    main()
