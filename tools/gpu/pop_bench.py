"""Cost of the population kernels and of DroQPopulation next to what they replace (bench.py is left as it is).

E envs of the TwinkleTwinkle hands task (droq_bench.py's env, shape and method): a host clock around work that ends in a
device synchronise, after a warm-up of every shape, the workloads alternating in one process, medians over the windows;
the windows themselves are stored.  For every P of --members (B = --batch / P rows per member, so the totals agree):

    pop_act_tile_major / pop_act_member_major   rp_pop_act, interleaved, on the newest slot's E rows, in both grid orders
    sac_act                                     rp_sac_act on the same E rows with ONE weight set (comparable at P = 1 only:
                                                for P > 1 it is the cost of the tile when every workgroup reads the same
                                                weights)
    gather_act_scatter                          the alternative without the kernel: index_select into a blocked copy, P
                                                launches of rp_sac_act on row ranges with the member's slices, index_copy
                                                of action, logp and env_action back
    pop_sample / sac_sample                     utd x batch rows in all, one launch each
    pop_target / droq_target / torch_target     one range of `batch` rows in all: rp_pop_target, rp_droq_target (one weight
                                                set), and the batched torch restatement on the population's modules
    pop_collect / droq_collect                  collect(T), per control step
    pop_update / droq_update                    update(1) at --utd

    python tools/gpu/pop_bench.py [--envs 4096] [--members 1,8,16] [--batch 4096] [--utd 20] [--out profiles/pop_bench.json]
"""
import argparse
import os

import torch

from _measure import HANDS, ROOT, alternate, host_per_call, load_twinkle, write_report   # (puts ROOT on sys.path)
from robopianist_amd import droq, learning, offpolicy, population


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--members", default="1,8,16")
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4096, help="rows of one range over all members")
    ap.add_argument("--utd", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=16, help="control steps per collect()")
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pop_bench.json"))
    args = ap.parse_args()
    E, C, B, U, T = args.envs, args.capacity, args.batch, args.utd, args.horizon
    members = [int(p) for p in args.members.split(",")]
    env = load_twinkle(E, precision=64, **HANDS)
    single = droq.DroQ(env, capacity=C, batch_size=B, seed=1, utd=U)
    pops = {P: population.DroQPopulation(env, P, capacity=C, batch_size=B // P, seed=1, utd=U) for P in members}
    dev, D, A = env.physics.device, single.D, single.A
    for l in [single] + list(pops.values()):   # every ring is full from here on
        l.collect(C)
        l.update(1)                            # ... and every minibatch buffer holds rows, policy outputs and y
    st = torch.cuda.current_stream(dev).cuda_stream
    newest = lambda l: (l.n_written - 1) % C
    s_targets = [single._critic_table(t) for t in single.targets]

    def sac_act(n=200):
        for i in range(n):
            single._act(single._obs[newest(single)], E, st, action=single._action[newest(single)].data_ptr(),
                        logp=single._logp.data_ptr(), env_action=single._env_action.data_ptr(), precision=single._precision)

    def sac_sample(n=20):
        for i in range(n):
            offpolicy.sample(single._obs.data_ptr(), single._action.data_ptr(), single._reward.data_ptr(),
                             single._discount.data_ptr(), single._step_type.data_ptr(), single._u_obs.data_ptr(),
                             single._u_next.data_ptr(), single._u_action.data_ptr(), single._u_reward.data_ptr(),
                             single._u_discount.data_ptr(), single._u_mask.data_ptr(), single.n_written, C, E, D, A, U * B,
                             seed=1, round_=i, hip_stream=st)

    def droq_target(n=500):
        for i in range(n):
            droq.target(single._u_next.data_ptr(), single._u_next_action.data_ptr(), single._u_next_logp.data_ptr(),
                        single._u_reward.data_ptr(), single._u_discount.data_ptr(), single._mean_f32.data_ptr(),
                        single._inv_std_f32.data_ptr(), single.obs_clip, single.gamma, single.log_alpha.data_ptr(), s_targets,
                        single._u_y.data_ptr(), D, single.H1, single.H2, A, U * B, threshold=single._threshold,
                        keep_scale=single._keep_scale, ln_eps=single.ln_eps, seed=1, round_=i, row_first=0, row_count=B,
                        hip_stream=st)

    def collects(l):
        def run():
            l.collect(T)
        return run

    def updates(l, n=2):
        def run():
            for _ in range(n):
                l.update(1)
        return run

    work = {"sac_act": (sac_act, 200), "sac_sample": (sac_sample, 20), "droq_target": (droq_target, 500),
            "droq_collect": (collects(single), T), "droq_update": (updates(single), 2)}

    def add(P, pop):
        Em, n = pop.Em, U * (B // P)
        slot = lambda: newest(pop)

        def pop_act(order):
            def run(k=200):
                for _ in range(k):
                    pop._act(pop._obs[slot()], Em, population.INTERLEAVED, st, action=pop._action[slot()].data_ptr(),
                             logp=pop._logp.data_ptr(), env_action=pop._env_action.data_ptr(), precision=pop._precision,
                             grid_order=order)
            return run

        idx = torch.arange(E, device=dev).view(Em, P).t().reshape(-1).contiguous()   # blocked row p Em + j <- env p + P j
        blk_obs = torch.empty(E, D, device=dev)
        blk_action, blk_logp = torch.empty(E, A, device=dev), torch.empty(E, device=dev)
        blk_env = torch.empty(E, A, device=dev, dtype=pop._dtype)
        stacked = [t for i in (0, 2, 4) for t in (pop.actor[i].weight, pop.actor[i].bias)]
        tables = [learning.mlp_table([t[p] for t in stacked]) for p in range(P)]

        def gather_act_scatter(k=50):
            for _ in range(k):
                torch.index_select(pop._obs[slot()], 0, idx, out=blk_obs)
                for p in range(P):
                    offpolicy.act(blk_obs.data_ptr(), pop._mean_f32[p].data_ptr(), pop._inv_std_f32[p].data_ptr(), pop.obs_clip,
                                  tables[p], D, pop.H1, pop.H2, A, E, log_std_bounds=pop.log_std_bounds,
                                  action=blk_action.data_ptr(), logp=blk_logp.data_ptr(), env_action=blk_env.data_ptr(),
                                  precision=pop._precision, seed=1, round_=pop._round, row_first=p * Em, row_count=Em,
                                  hip_stream=st)
                pop._action[slot()].index_copy_(0, idx, blk_action)
                pop._logp.index_copy_(0, idx, blk_logp)
                pop._env_action.index_copy_(0, idx, blk_env)

        def pop_sample(k=20):
            for i in range(k):
                population.sample(pop._obs.data_ptr(), pop._action.data_ptr(), pop._reward.data_ptr(),
                                  pop._discount.data_ptr(), pop._step_type.data_ptr(), pop._u_obs.data_ptr(),
                                  pop._u_next.data_ptr(), pop._u_action.data_ptr(), pop._u_reward.data_ptr(),
                                  pop._u_discount.data_ptr(), pop._u_mask.data_ptr(), pop.n_written, C, E, D, A, P, n, seed=1,
                                  round_=i, hip_stream=st)

        p_targets = [pop._critic_table(t) for t in pop.targets]

        def pop_target(order):
            def run(k=500):
                for i in range(k):
                    population.target(pop._u_next.data_ptr(), pop._u_next_action.data_ptr(), pop._u_next_logp.data_ptr(),
                                      pop._u_reward.data_ptr(), pop._u_discount.data_ptr(), pop._mean_f32.data_ptr(),
                                      pop._inv_std_f32.data_ptr(), pop.obs_clip, pop.gamma.data_ptr(),
                                      pop.log_alpha.data_ptr(), p_targets, pop._u_y.data_ptr(), D, pop.H1, pop.H2, A, P, n,
                                      threshold=pop._threshold, keep_scale=pop._keep_scale, ln_eps=pop.ln_eps, seed=1,
                                      round_=i, row_first=0, row_count=B // P, grid_order=order, hip_stream=st)
            return run

        def torch_target(k=500):
            pop._range = 0
            mb = pop.minibatch()
            with torch.no_grad():
                for _ in range(k):
                    xa = torch.cat([pop.normalize(mb["next_obs"]), mb["next_action"]], dim=2)
                    q = torch.stack([t(xa).squeeze(-1) for t in pop.targets]).min(0).values
                    y = mb["reward"] + pop.gamma[:, None] * mb["discount"] * (q - pop.log_alpha.exp()[:, None] * mb["next_logp"])
            return y

        work.update({f"pop_act_tile_major_P{P}": (pop_act(population.TILE_MAJOR), 200),
                     f"pop_act_member_major_P{P}": (pop_act(population.MEMBER_MAJOR), 200),
                     f"gather_act_scatter_P{P}": (gather_act_scatter, 50), f"pop_sample_P{P}": (pop_sample, 20),
                     f"pop_target_tile_major_P{P}": (pop_target(population.TILE_MAJOR), 500),
                     f"pop_target_member_major_P{P}": (pop_target(population.MEMBER_MAJOR), 500),
                     f"torch_target_P{P}": (torch_target, 500), f"pop_collect_P{P}": (collects(pop), T),
                     f"pop_update_P{P}": (updates(pop), 2)})

    for P, pop in pops.items():
        add(P, pop)

    times = alternate(work, args.windows, host_per_call)
    med = times.median
    us = lambda k: 1e6 * med[k]
    out = {
        "task": "RoboPianist-debug-TwinkleTwinkleRousseau-v0, hull fingertips, precision 64",
        "n_envs": E, "capacity": C, "batch_all_members": B, "utd": U, "obs_dim": D, "action_dim": A,
        "hidden": [single.H1, single.H2], "n_critics": single.n_critics, "dropout": single.dropout, "members": members,
        "steps_per_collect": T, "windows": args.windows,
        "default_grid_order": "tile_major" if population.dim("default_grid_order") == population.TILE_MAJOR else "member_major",
        "single_learner": {"sac_act_us": us("sac_act"), "sac_sample_us": us("sac_sample"), "droq_target_us": us("droq_target"),
                           "collect_ms_per_control_step": 1e3 * med["droq_collect"],
                           "collect_env_steps_per_s": E / med["droq_collect"], "update_ms": 1e3 * med["droq_update"]},
        "population": {str(P): {
            "act_tile_major_us": us(f"pop_act_tile_major_P{P}"), "act_member_major_us": us(f"pop_act_member_major_P{P}"),
            "gather_act_scatter_us": us(f"gather_act_scatter_P{P}"), "sample_us": us(f"pop_sample_P{P}"),
            "target_tile_major_us": us(f"pop_target_tile_major_P{P}"),
            "target_member_major_us": us(f"pop_target_member_major_P{P}"), "torch_target_us": us(f"torch_target_P{P}"),
            "collect_ms_per_control_step": 1e3 * med[f"pop_collect_P{P}"],
            "collect_env_steps_per_s": E / med[f"pop_collect_P{P}"], "update_ms": 1e3 * med[f"pop_update_P{P}"]}
            for P in members},
        "seconds_per_call_windows": times.windows,
        "spread": {k: times.spread(k) for k in work},
        "method": "host clock around work that ends in a device synchronise; every workload warmed up once, then "
                  "alternating windows in one process; medians of the windows, which are stored",
    }
    write_report(out, args.out, printed={k: v for k, v in out.items() if k != "seconds_per_call_windows"}, indent=1)


if __name__ == "__main__":
    main()
