"""Cost of DroQ's fused actor and temperature step next to the torch actor step it replaces, of each of its two launches,
and of DroQ.update(1) in the four combinations of critic_step and actor_step (bench.py is left as it is).

E envs of the TwinkleTwinkle hands task with hull fingertips (bench.py's config 3), critic_bench.py's method and shape: a
host clock around work that ends in a device synchronise, after a warm-up of every shape, the workloads alternating in
one process, medians over the windows with the lowest and the highest window:

    fused_step             actor.step on the B rows of a minibatch (dropout 0.01, two critics): two launches
    torch_step             DroQ.actor_step(batch), the default path, on the same rows: the normaliser, the actor, torch's
                           randn, the cat, two critics forward with torch's dropout, autograd through all of them, two Adams
    fused_rows             the rows launch alone
    fused_apply            the apply launch alone (on the workspace the last rows launch left)
    update_{critic}_{actor}_utd{1,4,U}   one DroQ.update(1) at that utd with critic_step / actor_step in that mode

The fused step counts as faster only where the medians differ by more than both spreads; what it is compared with is
torch's step in the same job.

    python tools/gpu/actor_bench.py [--envs 4096] [--capacity 64] [--batch 4096] [--utd 20] [--out profiles/actor_bench.json]
"""
import argparse
import os

import torch

from _measure import HANDS, ROOT, alternate, host_per_call, load_twinkle, write_report   # (puts ROOT on sys.path)
from robopianist_amd import actor, critic, droq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--utd", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actor_bench.json"))
    args = ap.parse_args()
    E, C, B, U = args.envs, args.capacity, args.batch, args.utd
    env = load_twinkle(E, precision=64, **HANDS)
    utds = sorted({1, 4, U})
    modes = [(c, a) for c in ("torch", "fused") for a in ("torch", "fused")]
    learners = {(c, a, u): droq.DroQ(env, capacity=C, batch_size=B, seed=1, utd=u, critic_step=c, actor_step=a)
                for c, a in modes for u in utds}
    plain, fused = learners["torch", "torch", 1], learners["torch", "fused", 1]
    dev = env.physics.device
    for l in learners.values():   # every ring is full from here on
        l.collect(C)
    st = torch.cuda.current_stream(dev).cuda_stream
    plain.sample_and_target()     # a minibatch of B rows, in each of the two learners
    fused.sample_and_target()
    mb = plain.minibatch()
    f = fused

    def fused_steps(launches):
        def run(n=200):
            for i in range(n):
                actor.step(f._u_obs.data_ptr(), f._u_mask.data_ptr(), f._mean_f32.data_ptr(), f._inv_std_f32.data_ptr(), f.obs_clip,
                           actor.set_entry(f._actor_tensors()), actor.set_entry(f._a_m), actor.set_entry(f._a_v),
                           [critic.set_entry(f._critic_tensors(c)) for c in f.critics], f.log_alpha.data_ptr(),
                           f._la_m.data_ptr(), f._la_v.data_ptr(), f.target_entropy, f.log_std_bounds, f._a_ws.data_ptr(),
                           f._a_bytes, f._a_stats.data_ptr(), f.D, f.H1, f.H2, f.A, B, actor.adam_entry(3e-4, i + 1),
                           actor.adam_entry(3e-4, i + 1), threshold=f._threshold, keep_scale=f._keep_scale, ln_eps=f.ln_eps,
                           seed=1, round_=i, launches=launches, hip_stream=st)
        return run

    def torch_steps(n=200):
        for _ in range(n):
            plain.actor_step(mb)

    def updates(key, n):
        def run():
            for _ in range(n):
                learners[key].update(1)
        return run

    work = {"fused_step": (fused_steps(actor.STEP), 200), "torch_step": (torch_steps, 200),
            "fused_rows": (fused_steps(actor.ROWS_ONLY), 200), "fused_apply": (fused_steps(actor.APPLY_ONLY), 200)}
    name = lambda c, a, u: f"update_{c}_{a}_utd{u}"
    for u in utds:
        n = max(2, 120 // (3 * u))
        for c, a in modes:
            work[name(c, a, u)] = (updates((c, a, u), n), n)
    t = alternate(work, args.windows, host_per_call)
    out = {
        "task": "RoboPianist-debug-TwinkleTwinkleRousseau-v0, hull fingertips, precision 64",
        "n_envs": E, "capacity": C, "batch": B, "obs_dim": f.D, "action_dim": f.A, "hidden": [f.H1, f.H2],
        "n_critics": f.n_critics, "dropout": f.dropout, "utd": U, "windows": args.windows,
        "us": {k: t.stat(k, 1e6) for k in ("fused_step", "torch_step", "fused_rows", "fused_apply")},
        "update_ms": {f"{c}_critic_{a}_actor": {str(u): t.stat(name(c, a, u), 1e3) for u in utds} for c, a in modes},
        "fused_step_is_faster": t.apart("fused_step", "torch_step"),
        "fused_step_is_slower": t.apart("torch_step", "fused_step"),
        "fused_actor_update_is_faster": {c: {str(u): t.apart(name(c, "fused", u), name(c, "torch", u)) for u in utds}
                                         for c in ("torch", "fused")},
        "fused_actor_update_is_slower": {c: {str(u): t.apart(name(c, "torch", u), name(c, "fused", u)) for u in utds}
                                         for c in ("torch", "fused")},
        "method": "host clock around work that ends in a device synchronise; every workload warmed up once, then "
                  "alternating windows in one process; medians with the lowest and highest window; faster / slower only "
                  "where the two sets of windows do not overlap",
    }
    write_report(out, args.out, indent=1)


if __name__ == "__main__":
    main()
