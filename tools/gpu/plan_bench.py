"""Cost of one PredictiveSampler.plan() next to the plain env steps it is made of (bench.py is left as it is).

G real envs of the TwinkleTwinkle task with hull fingertips, K candidates each, horizon H: the planning environment has
G K envs.  Timed with a host clock around work that ends in a device synchronise, after a warm-up of every shape, the
workloads alternating in one process, medians over the windows:

    plan      PredictiveSampler.plan(): shift, sample, fork, active <- 1, physics.forward(), H x (action, env.step,
              accumulate), select, first action
    steps     H plain env.step calls of the planning environment (from the states the last rollout ended in, one action)
    fork      the fork alone: rp_plan_fork, active <- 1, physics.forward()
    rollout   fork + the H x (action, env.step, accumulate) of a plan
    quiet     the same rollout with the nominal in every row: the candidates of a group follow one plan
    kernels   the launches of librp_plan.so of one plan, enqueued alone (shift, sample, fork, H x (action, accumulate),
              select, action)

    python tools/gpu/plan_bench.py [--groups 64] [--candidates 64] [--horizon 8] [--out profiles/plan_bench.json]
    python tools/gpu/plan_bench.py --profile     # three plans and nothing else, for a kernel trace
"""
import argparse
import os

import numpy as np
import torch

from _measure import ROOT, Times, host_time, load_twinkle, write_report   # (puts ROOT on sys.path)
from robopianist_amd import planning


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--knots", type=int, default=2)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_bench.json"))
    args = ap.parse_args()
    G, K, H, P = args.groups, args.candidates, args.horizon, args.knots

    def load(n):
        return load_twinkle(n, seed=3, n_steps_lookahead=10)

    real = load(G)
    s = planning.PredictiveSampler(real, load, n_candidates=K, horizon=H, n_knots=P, sigma=0.2, seed=1)
    plan_env = s.plan_env
    real.reset()
    spec = real.action_spec()
    rng = np.random.default_rng(0)
    lo, hi = np.asarray(spec.minimum), np.asarray(spec.maximum)
    for _ in range(10):   # a state off the reset state, different in every env
        real.step(torch.as_tensor(lo + rng.uniform(0.3, 0.7, (G, spec.shape[0])) * (hi - lo), device=real.physics.device))
    sync = torch.cuda.synchronize

    if args.profile:
        for _ in range(3):
            s.plan()
        sync()
        print("3 plans")
        return

    def ms_per_call(fn, n):
        return 1e3 * host_time(fn, n) / n

    def steps():
        for _ in range(H):
            plan_env.step(s._act)

    st = torch.cuda.current_stream(real.physics.device).cuda_stream
    reward = torch.zeros(s.E, dtype=s._dtype, device=real.physics.device)
    step_type = torch.ones(s.E, dtype=torch.int32, device=real.physics.device)

    def kernels():
        planning.shift(s._nominal.data_ptr(), s._spline, H, P, s.nu, G, hip_stream=st)
        planning.sample(s._nominal.data_ptr(), s._sigma.data_ptr(), s._lo.data_ptr(), s._hi.data_ptr(), s._knots.data_ptr(),
                        1, 0, G, K, P, s.nu, hip_stream=st)
        for tab in s._tables:
            planning.fork(tab, G, K, hip_stream=st)
        for h in range(H):
            planning.action(s._knots.data_ptr(), s._act.data_ptr(), s._precision, s._spline, h, H, P, s.nu, s.E, hip_stream=st)
            planning.accumulate(s._ret.data_ptr(), s._alive.data_ptr(), reward.data_ptr(), step_type.data_ptr(), s._precision,
                                1.0, s.E, hip_stream=st)
        planning.select(s._ret.data_ptr(), s._knots.data_ptr(), s._nominal.data_ptr(), s._best_k.data_ptr(),
                        s._best_return.data_ptr(), G, K, P, s.nu, hip_stream=st)
        planning.action(s._nominal.data_ptr(), s._first.data_ptr(), s._precision, s._spline, 0, H, P, s.nu, G, hip_stream=st)

    def quiet():
        s.rollout(quiet_knots)

    work = (("plan_ms", s.plan, 8), ("steps_ms", steps, 8), ("fork_ms", s.fork, 20), ("rollout_ms", s.rollout, 8),
            ("quiet_ms", quiet, 8), ("kernels_ms", kernels, 200))
    s.plan()
    quiet_knots = s.nominal.repeat_interleave(K, dim=0).contiguous()
    for _, fn, _ in work:   # warm every shape
        ms_per_call(fn, 2)
    windows = []
    for _ in range(args.windows):
        windows.append({name: ms_per_call(fn, n) for name, fn, n in work})
        print(windows[-1], flush=True)
    med = Times({k: [w[k] for w in windows] for k in windows[0]}).median
    out = dict(device=torch.cuda.get_device_name(0), G=G, K=K, H=H, P=P, nu=s.nu, planning_envs=s.E, fields=len(s._fields),
               fork_bytes_per_row=sum(rb for *_, rb in s._fields), median=med, windows=windows,
               kernels_share_of_plan=med["kernels_ms"] / med["plan_ms"], plan_over_steps=med["plan_ms"] / med["steps_ms"],
               warn=int(plan_env.physics.warn.max()))
    write_report(out, args.out)


if __name__ == "__main__":
    main()
