"""Cost of the population's fused critic step next to the single learner's, of each of its two launches, of both grid
orders, and of DroQPopulation.update(1) in both modes (bench.py is left as it is).

E envs of the TwinkleTwinkle hands task with hull fingertips (bench.py's config 3), pop_bench.py's and critic_bench.py's
method and shape: a host clock around work that ends in a device synchronise, after a warm-up of every shape, the
workloads alternating in one process, medians over the windows with the lowest and the highest window.  For every P of
--members (B = --batch / P rows per member, so the totals agree):

    pop_step_{tile,member}_major_P      pop_critic.step on one range of all members (dropout 0.01, two critics): two launches
    pop_rows_P / pop_apply_P            each of the two launches alone, in the default grid order (the apply launch on the
                                        workspace the last rows launch left)
    single_step / _rows / _apply        critic.step on --batch rows with ONE weight set, and its two launches
    update_{torch,fused}_utd{1,4,U}_P   one DroQPopulation.update(1) at that utd in that mode
    droq_update_fused_utd{1,4,U}        one DroQ.update(1), critic_step="fused", at --batch rows

A difference counts only where the two sets of windows do not overlap.

    python tools/gpu/pop_critic_bench.py [--envs 4096] [--members 1,8,16] [--batch 4096] [--utd 20]
                                         [--out profiles/pop_critic_bench.json]
"""
import argparse
import os

import torch

from _measure import HANDS, ROOT, alternate, host_per_call, load_twinkle, write_report   # (puts ROOT on sys.path)
from robopianist_amd import critic, droq, pop_critic, population


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--members", default="1,8,16")
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4096, help="rows of one range over all members")
    ap.add_argument("--utd", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pop_critic_bench.json"))
    args = ap.parse_args()
    E, C, B, U = args.envs, args.capacity, args.batch, args.utd
    members = [int(p) for p in args.members.split(",")]
    env = load_twinkle(E, precision=64, **HANDS)
    utds = sorted({1, 4, U})
    modes = ("torch", "fused")
    singles = {u: droq.DroQ(env, capacity=C, batch_size=B, seed=1, utd=u, critic_step="fused") for u in utds}
    pops = {(P, m, u): population.DroQPopulation(env, P, capacity=C, batch_size=B // P, seed=1, utd=u, critic_step=m)
            for P in members for m in modes for u in utds}
    dev = env.physics.device
    for l in list(singles.values()) + list(pops.values()):   # every ring is full from here on
        l.collect(C)
        l.update(1)                                          # ... and every minibatch buffer holds rows and y
    st = torch.cuda.current_stream(dev).cuda_stream
    single = singles[1]
    D, A, H1, H2 = single.D, single.A, single.H1, single.H2

    def single_steps(launches):
        sets = lambda nets: [critic.set_entry(single._critic_tensors(net)) for net in nets]
        a = (single._u_obs.data_ptr(), single._u_action.data_ptr(), single._u_y.data_ptr(), single._u_mask.data_ptr(),
             single._mean_f32.data_ptr(), single._inv_std_f32.data_ptr(), single.obs_clip, sets(single.critics),
             [critic.set_entry(m) for m in single._c_m], [critic.set_entry(v) for v in single._c_v], sets(single.targets),
             single._u_q.data_ptr(), single._c_ws.data_ptr(), single._c_bytes, D, H1, H2, A, B)

        def run(n=200):
            for i in range(n):
                step_size, bc2_sqrt = critic.adam_scalars(3e-4, i + 1)
                critic.step(*a, step_size, bc2_sqrt, tau=single.tau, threshold=single._threshold, keep_scale=single._keep_scale,
                            ln_eps=single.ln_eps, seed=1, round_=i, launches=launches, hip_stream=st)
        return run

    def pop_steps(pop, launches, order):
        sets = lambda nets: [critic.set_entry(pop._critic_tensors(net)) for net in nets]
        a = (pop._u_obs.data_ptr(), pop._u_action.data_ptr(), pop._u_y.data_ptr(), pop._u_mask.data_ptr(),
             pop._mean_f32.data_ptr(), pop._inv_std_f32.data_ptr(), pop.obs_clip, sets(pop.critics),
             [critic.set_entry(m) for m in pop._c_m], [critic.set_entry(v) for v in pop._c_v], sets(pop.targets),
             pop._u_q.data_ptr(), pop._c_ws.data_ptr(), pop._c_bytes, D, H1, H2, A, pop.P, pop.utd * pop.B)

        def run(n=200):
            for i in range(n):
                step_size, bc2_sqrt = critic.adam_scalars(3e-4, i + 1)
                pop_critic.step(*a, step_size, bc2_sqrt, tau=pop.tau, threshold=pop._threshold, keep_scale=pop._keep_scale,
                                ln_eps=pop.ln_eps, seed=1, round_=i, row_first=0, row_count=pop.B, grid_order=order,
                                launches=launches, hip_stream=st)
        return run

    def updates(l, n):
        def run():
            for _ in range(n):
                l.update(1)
        return run

    work = {"single_step": (single_steps(critic.STEP), 200), "single_rows": (single_steps(critic.ROWS_ONLY), 200),
            "single_apply": (single_steps(critic.APPLY_ONLY), 200)}
    for P in members:
        pop = pops[P, "fused", 1]
        work.update({f"pop_step_tile_major_P{P}": (pop_steps(pop, pop_critic.STEP, pop_critic.TILE_MAJOR), 200),
                     f"pop_step_member_major_P{P}": (pop_steps(pop, pop_critic.STEP, pop_critic.MEMBER_MAJOR), 200),
                     f"pop_rows_P{P}": (pop_steps(pop, pop_critic.ROWS_ONLY, None), 200),
                     f"pop_apply_P{P}": (pop_steps(pop, pop_critic.APPLY_ONLY, None), 200)})
    for u in utds:
        n = max(2, 120 // (3 * u))
        work[f"droq_update_fused_utd{u}"] = (updates(singles[u], n), n)
        for P in members:
            for m in modes:
                work[f"update_{m}_utd{u}_P{P}"] = (updates(pops[P, m, u], n), n)
    times = alternate(work, args.windows, host_per_call)
    stat, verdict = times.stat, times.verdict
    out = {
        "task": "RoboPianist-debug-TwinkleTwinkleRousseau-v0, hull fingertips, precision 64",
        "n_envs": E, "capacity": C, "batch_all_members": B, "obs_dim": D, "action_dim": A, "hidden": [H1, H2],
        "n_critics": single.n_critics, "dropout": single.dropout, "utd": U, "members": members, "windows": args.windows,
        "default_grid_order": "tile_major" if pop_critic.dim("default_grid_order") == pop_critic.TILE_MAJOR else "member_major",
        "single_learner_us": {k: stat(f"single_{k}", 1e6) for k in ("step", "rows", "apply")},
        "population_us": {str(P): {"step_tile_major": stat(f"pop_step_tile_major_P{P}", 1e6),
                                   "step_member_major": stat(f"pop_step_member_major_P{P}", 1e6),
                                   "rows": stat(f"pop_rows_P{P}", 1e6), "apply": stat(f"pop_apply_P{P}", 1e6),
                                   "step_against_single_learner": verdict(f"pop_step_tile_major_P{P}", "single_step"),
                                   "tile_major_against_member_major": verdict(f"pop_step_tile_major_P{P}",
                                                                              f"pop_step_member_major_P{P}")}
                          for P in members},
        "droq_update_fused_ms": {str(u): stat(f"droq_update_fused_utd{u}", 1e3) for u in utds},
        "update_ms": {str(P): {str(u): {"torch": stat(f"update_torch_utd{u}_P{P}", 1e3),
                                        "fused": stat(f"update_fused_utd{u}_P{P}", 1e3),
                                        "fused_against_torch": verdict(f"update_fused_utd{u}_P{P}", f"update_torch_utd{u}_P{P}"),
                                        "fused_against_droq_fused": verdict(f"update_fused_utd{u}_P{P}", f"droq_update_fused_utd{u}")}
                               for u in utds} for P in members},
        "method": "host clock around work that ends in a device synchronise; every workload warmed up once, then "
                  "alternating windows in one process; medians with the lowest and highest window; faster / slower only "
                  "where the two sets of windows do not overlap",
    }
    write_report(out, args.out, indent=1)


if __name__ == "__main__":
    main()
