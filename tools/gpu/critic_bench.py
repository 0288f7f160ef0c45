"""Cost of DroQ's fused critic step next to the torch critic step it replaces, of each of its two launches, and of
DroQ.update(1) in both modes (bench.py is left as it is).

E envs of the TwinkleTwinkle hands task with hull fingertips (bench.py's config 3), droq_bench.py's method and shape: a
host clock around work that ends in a device synchronise, after a warm-up of every shape, the workloads alternating in
one process, medians over the windows with the lowest and the highest window:

    fused_step             critic.step on the B rows of a minibatch (dropout 0.01, two critics): two launches
    torch_step             DroQ.critic_step(batch), the default path, on the same rows: the normaliser, the cat, two critics
                           forward with torch's dropout, autograd, Adam, _foreach_lerp_
    fused_rows             the rows launch alone
    fused_apply            the apply launch alone (on the workspace the last rows launch left)
    update_{torch,fused}_utd{1,4,U}   one DroQ.update(1) at that utd in that mode

The fused step counts as faster only where the medians differ by more than both spreads.

    python tools/gpu/critic_bench.py [--envs 4096] [--capacity 64] [--batch 4096] [--utd 20] [--out profiles/critic_bench.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from robopianist_amd import critic, droq, suite  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--utd", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "critic_bench.json"))
    args = ap.parse_args()
    E, C, B, U = args.envs, args.capacity, args.batch, args.utd
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = suite.load("RoboPianist-debug-TwinkleTwinkleRousseau-v0", seed=12345, n_envs=E, precision=64,
                         task_kwargs=dict(trim_silence=True, control_timestep=0.05, gravity_compensation=True,
                                          reduced_action_space=False, n_steps_lookahead=10))
    utds = sorted({1, 4, U})
    modes = ("torch", "fused")
    learners = {(m, u): droq.DroQ(env, capacity=C, batch_size=B, seed=1, utd=u, critic_step=m) for m in modes for u in utds}
    plain, fused = learners["torch", 1], learners["fused", 1]
    dev = env.physics.device
    sync = torch.cuda.synchronize
    for l in learners.values():   # every ring is full from here on
        l.collect(C)
    st = torch.cuda.current_stream(dev).cuda_stream
    plain.sample_and_target()     # a minibatch of B rows and its y, in each of the two learners
    fused.sample_and_target()
    mb = plain.minibatch()
    sets = lambda nets: [critic.set_entry(fused._critic_tensors(net)) for net in nets]
    step_args = (fused._u_obs.data_ptr(), fused._u_action.data_ptr(), fused._u_y.data_ptr(), fused._u_mask.data_ptr(),
                 fused._mean_f32.data_ptr(), fused._inv_std_f32.data_ptr(), fused.obs_clip, sets(fused.critics),
                 [critic.set_entry(m) for m in fused._c_m], [critic.set_entry(v) for v in fused._c_v], sets(fused.targets),
                 fused._u_q.data_ptr(), fused._c_ws.data_ptr(), fused._c_bytes, fused.D, fused.H1, fused.H2, fused.A, B)

    def fused_steps(launches):
        def run(n=200):
            for i in range(n):
                step_size, bc2_sqrt = critic.adam_scalars(3e-4, i + 1)
                critic.step(*step_args, step_size, bc2_sqrt, tau=fused.tau, threshold=fused._threshold,
                            keep_scale=fused._keep_scale, ln_eps=fused.ln_eps, seed=1, round_=i, launches=launches, hip_stream=st)
        return run

    def torch_steps(n=200):
        for _ in range(n):
            plain.critic_step(mb)

    def updates(key, n):
        def run():
            for _ in range(n):
                learners[key].update(1)
        return run

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return time.perf_counter() - t0

    work = {"fused_step": (fused_steps(critic.STEP), 200), "torch_step": (torch_steps, 200),
            "fused_rows": (fused_steps(critic.ROWS_ONLY), 200), "fused_apply": (fused_steps(critic.APPLY_ONLY), 200)}
    for u in utds:
        n = max(2, 120 // (3 * u))
        for m in modes:
            work[f"update_{m}_utd{u}"] = (updates((m, u), n), n)
    for fn, _ in work.values():   # warm-up of every shape
        timed(fn)
    times = {k: [] for k in work}
    for _ in range(args.windows):
        for k, (fn, n) in work.items():
            times[k].append(timed(fn) / n)
    med = {k: float(np.median(v)) for k, v in times.items()}
    lo, hi = {k: float(min(v)) for k, v in times.items()}, {k: float(max(v)) for k, v in times.items()}
    apart = lambda a, b: bool(hi[a] < lo[b])   # a's slowest window below b's fastest: more than both spreads
    out = {
        "task": "RoboPianist-debug-TwinkleTwinkleRousseau-v0, hull fingertips, precision 64",
        "n_envs": E, "capacity": C, "batch": B, "obs_dim": fused.D, "action_dim": fused.A, "hidden": [fused.H1, fused.H2],
        "n_critics": fused.n_critics, "dropout": fused.dropout, "utd": U, "windows": args.windows,
        "us": {k: {"median": 1e6 * med[k], "lowest": 1e6 * lo[k], "highest": 1e6 * hi[k]}
               for k in ("fused_step", "torch_step", "fused_rows", "fused_apply")},
        "update_ms": {m: {str(u): {"median": 1e3 * med[f"update_{m}_utd{u}"], "lowest": 1e3 * lo[f"update_{m}_utd{u}"],
                                   "highest": 1e3 * hi[f"update_{m}_utd{u}"]} for u in utds} for m in modes},
        "fused_step_is_faster": apart("fused_step", "torch_step"),
        "fused_step_is_slower": apart("torch_step", "fused_step"),
        "fused_update_is_faster": {str(u): apart(f"update_fused_utd{u}", f"update_torch_utd{u}") for u in utds},
        "fused_update_is_slower": {str(u): apart(f"update_torch_utd{u}", f"update_fused_utd{u}") for u in utds},
        "method": "host clock around work that ends in a device synchronise; every workload warmed up once, then "
                  "alternating windows in one process; medians with the lowest and highest window; faster / slower only "
                  "where the two sets of windows do not overlap",
    }
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
