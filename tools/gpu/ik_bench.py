"""Cost of the fingertip inverse kinematics next to the env step it feeds (bench.py is left as it is).

Config 2 (TwinkleTwinkle scripted replay, hull fingertips) at 4096 envs, staggered as bench.py staggers it (env e is
e mod T steps into its episode).  Timed with device events after a warm-up, in windows of at least a second, the
workloads alternating in one process:

    A  env.step (scripted replay, no wrapper)
    B  FingertipIK.solve alone on the batch's current state, K = 1 and K = 4 (absolute targets 1 cm above the tips)
    C  solve (K = 1) into the wrapper's action buffer, then A's env.step: the wrapper's added work on A's physics
    D  FingertipActionWrapper.step with small random delta actions (its own trajectory: the physics differs from A's),
       after everything else

and the kernel's registers, LDS and scratch from the compiler's resource report (hipcc is run once more for it; skip
with --no-resources).  Writes profiles/ik_bench.json.

    python tools/gpu/ik_bench.py [--envs 4096] [--windows 3] [--out profiles/ik_bench.json]
"""
import argparse
import os
import re
import subprocess

import torch

from _measure import HANDS, ROOT, Times, event_window, load_twinkle, staggered_replay, write_report


def kernel_resources():
    """{kernel: {VGPRs, AGPRs, SGPRs, scratch_bytes_per_lane, lds_bytes_per_block, occupancy_waves_per_simd}} from
    `hipcc -Rpass-analysis=kernel-resource-usage` on csrc/rp_ik.hip with build()'s flags."""
    src = os.path.join(ROOT, "robopianist_amd", "csrc", "rp_ik.hip")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on", "-c",
                        "-Rpass-analysis=kernel-resource-usage", src, "-o", os.devnull], capture_output=True, text=True)
    out, name = {}, None
    keys = {"VGPRs": "VGPRs", "AGPRs": "AGPRs", "TotalSGPRs": "SGPRs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "LDS Size [bytes/block]": "lds_bytes_per_block", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd",
            "SGPRs Spill": "sgpr_spills", "VGPRs Spill": "vgpr_spills"}
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = "rp_ik_kernel<float>" if "IfEE" in m.group(1) else ("rp_ik_kernel<double>" if "IdEE" in m.group(1) else m.group(1))
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and name and m.group(1).strip() in keys:
            out[name][keys[m.group(1).strip()]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=3, help="timed windows per workload (each at least --seconds long)")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--no-resources", dest="resources", action="store_false")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik_bench.json"))
    args = ap.parse_args()

    from robopianist_amd.wrappers import FingertipActionWrapper
    E = args.envs
    base = load_twinkle(E, **HANDS, primitive_fingertip_collisions=False,   # hull fingertips, as bench.py's config 2
                        change_color_on_activation=True)
    tip_env = FingertipActionWrapper(base)          # (K = 1, delta mode: the defaults)
    ik = tip_env.ik
    phys = base.physics
    dev = phys.device
    env, script, _ = staggered_replay(base)

    targets = torch.zeros((E, ik.n_tips, 3), dtype=torch.float64, device=dev)
    up = torch.zeros_like(targets); up[..., 2] = 0.01

    def retarget():
        targets.copy_(ik.tip_positions(phys.qpos, phys._tree_offset) + up)

    def step_only():
        env.step(script)

    def solve_k(k):
        return lambda: ik.solve(phys.qpos, targets, tree_offset=phys._tree_offset, iterations=k)

    def step_plus_solve():
        ik.solve(phys.qpos, targets, tree_offset=phys._tree_offset, iterations=1, out=tip_env.native_action)
        env.step(script)

    gen = torch.Generator(device=dev); gen.manual_seed(1)
    deltas = torch.rand((E, 3 * ik.n_tips + 1), generator=gen, device=dev, dtype=torch.float64) * 0.2 - 0.1
    deltas[:, -1] = 0.0

    def wrapped_step():
        tip_env.step(deltas)

    retarget()
    for fn in (step_only, solve_k(1), solve_k(4), step_plus_solve):   # warm-up (allocations)
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    res = {"step": [], "solve_k1": [], "solve_k4": [], "step_plus_solve": [], "wrapped_step": []}
    for _ in range(args.windows):   # alternating
        res["step"].append(event_window(step_only, args.seconds))
        retarget()
        res["solve_k1"].append(event_window(solve_k(1), args.seconds))
        res["solve_k4"].append(event_window(solve_k(4), args.seconds))
        res["step_plus_solve"].append(event_window(step_plus_solve, args.seconds))
    for _ in range(5):
        wrapped_step()
    for _ in range(args.windows):
        res["wrapped_step"].append(event_window(wrapped_step, args.seconds))
    med = Times(res).median

    out = {
        "device": torch.cuda.get_device_name(dev),
        "workload": f"config 2 (TwinkleTwinkle scripted replay, hull fingertips), {E} envs, staggered, fp64",
        "method": f"device events, {args.windows} windows of >= {args.seconds} s per workload, alternating; medians",
        "env_step_ms": med["step"],
        "solve_k1_ms": med["solve_k1"],
        "solve_k4_ms": med["solve_k4"],
        "solve_k1_share_of_step": med["solve_k1"] / med["step"],
        "env_step_plus_solve_k1_ms": med["step_plus_solve"],
        "solve_k1_added_ms": med["step_plus_solve"] - med["step"],
        "wrapped_step_ms": med["wrapped_step"],
        "wrapped_step_note": "random delta actions: the hands leave the replay's trajectory, so its physics is not A's",
        "solves_per_s_k1": E / (med["solve_k1"] * 1e-3),
        "windows_ms": res,
        "kernel_resources": kernel_resources() if args.resources else None,
    }
    write_report(out, args.out, printed={k: v for k, v in out.items() if k != "windows_ms"})


if __name__ == "__main__":
    main()
