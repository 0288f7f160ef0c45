"""Cost of SAC's collection, sampler, target and gradient step next to the plain env steps and to PPO's collection
(bench.py is left as it is).

E envs of the TwinkleTwinkle hands task with hull fingertips (bench.py's config 3), learn_bench.py's method: a host clock
around work that ends in a device synchronise, after a warm-up of every shape, the workloads alternating in one process,
windows of about half a second, medians over the windows and their spread:

    sac_collect  SAC.collect(T): T x (rp_sac_act on the newest slot, step_canonical, rp_learn_pack into the next slot),
                 then rp_learn_moments over the new slots
    replay       plain stepping under the actions the last SAC.collect() recorded (step_canonical alone)
    ppo_collect  PPO.collect() of the same horizon on the same env: T x (rp_learn_act, step_canonical, rp_learn_pack), the
                 critic at slot T, rp_learn_gae
    sample       one rp_sac_sample of B rows out of the full ring
    torch_sample the same minibatch by torch indexing: four draws per row, the validity rule, the first valid draw, five
                 gathers
    act_target   rp_sac_act on next_obs, then rp_sac_target (two launches)
    torch_target the same by torch: the normaliser, the actor, the squashed Gaussian, the target critics on the cat, the
                 minimum and the target
    grad_step    one SAC.update(1): the three launches, then the losses, autograd, three Adams and the Polyak step (torch)
    update       one SAC.update(G)

The env is shared by the two learners (each continues from its own last TimeStep; the timing does not depend on it).

    python tools/gpu/sac_bench.py [--envs 4096] [--capacity 64] [--batch 4096] [--out profiles/sac_bench.json]
"""
import argparse
import os

import torch

from _measure import HANDS, ROOT, alternate, host_per_call, load_twinkle, write_report   # (puts ROOT on sys.path)
from robopianist_amd import learning, offpolicy

HBM_PEAK = {"spec": 8.0e12, "measured_float4_copy": 6.29e12}   # bytes/s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=16, help="control steps per round (and PPO's horizon)")
    ap.add_argument("--grad-steps", type=int, default=4, help="gradient steps per round")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=4, help="rounds' worth of control steps per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_bench.json"))
    args = ap.parse_args()
    E, C, B, T, G, R = args.envs, args.capacity, args.batch, args.horizon, args.grad_steps, args.rollouts
    env = load_twinkle(E, precision=64, **HANDS)
    sac = offpolicy.SAC(env, capacity=C, batch_size=B, seed=1)
    ppo = learning.PPO(env, horizon=T, seed=1)
    dev, D, A = env.physics.device, sac.D, sac.A
    sac.collect(C)   # the ring is full from here on
    recorded = sac.ring()["action"][:T].to(env.physics.dtype).clone()

    def sac_collects():
        for _ in range(R):
            sac.collect(T)

    def replay_steps():
        for _ in range(R):
            for t in range(T):
                env.step_canonical(recorded[t], sac._bounds, False)

    def ppo_collects():
        for _ in range(R):
            ppo.collect()

    st = torch.cuda.current_stream(dev).cuda_stream
    ring = sac.ring()
    mb = sac.minibatch()

    def samples(n=4000):
        for i in range(n):
            offpolicy.sample(ring["obs"].data_ptr(), ring["action"].data_ptr(), ring["reward"].data_ptr(),
                             ring["discount"].data_ptr(), ring["step_type"].data_ptr(), mb["obs"].data_ptr(),
                             mb["next_obs"].data_ptr(), mb["action"].data_ptr(), mb["reward"].data_ptr(),
                             mb["discount"].data_ptr(), mb["mask"].data_ptr(), sac.n_written, C, E, D, A, B, seed=1,
                             round_=i, hip_stream=st)

    flat = {k: v.view(C * E, *v.shape[2:]) for k, v in ring.items()}

    def torch_samples(n=400):
        F = min(sac.n_written, C)
        for _ in range(n):
            i = torch.randint(0, (F - 1) * E, (B, offpolicy.SAMPLE_TRIES), device=dev)
            m, e = sac.n_written - F + i // E, i % E
            r0, r1 = (m % C) * E + e, ((m + 1) % C) * E + e
            ok = (flat["step_type"][r0] != offpolicy.STEP_LAST) & (flat["step_type"][r1] != offpolicy.STEP_FIRST)
            j = ok.int().argmax(1, keepdim=True)
            mask = ok.any(1).float()
            r0, r1 = r0.gather(1, j).squeeze(1), r1.gather(1, j).squeeze(1)
            out = (flat["obs"][r0] * mask[:, None], flat["obs"][r1] * mask[:, None], flat["action"][r0] * mask[:, None],
                   flat["reward"][r1] * mask, flat["discount"][r1] * mask)
        return out

    actor = sac._mlp(sac.actor)
    targets = [sac._mlp(t) for t in sac.targets]

    def act_targets(n=1000):
        for i in range(n):
            offpolicy.act(mb["next_obs"].data_ptr(), sac._mean_f32.data_ptr(), sac._inv_std_f32.data_ptr(), sac.obs_clip,
                          actor, D, sac.H1, sac.H2, A, B, log_std_bounds=sac.log_std_bounds,
                          action=mb["next_action"].data_ptr(), logp=mb["next_logp"].data_ptr(), seed=1, round_=i,
                          hip_stream=st)
            offpolicy.target(mb["next_obs"].data_ptr(), mb["next_action"].data_ptr(), mb["next_logp"].data_ptr(),
                             mb["reward"].data_ptr(), mb["discount"].data_ptr(), sac._mean_f32.data_ptr(),
                             sac._inv_std_f32.data_ptr(), sac.obs_clip, sac.gamma, sac.log_alpha.data_ptr(), targets,
                             mb["y"].data_ptr(), D, sac.H1, sac.H2, A, B, hip_stream=st)

    eps = torch.zeros((B, A), device=dev)

    def torch_targets(n=1000):
        with torch.no_grad():
            for _ in range(n):
                xn = sac.normalize(mb["next_obs"])
                eps.normal_()
                a, logp, _ = offpolicy.squashed_gaussian(sac.actor(xn), eps, sac.log_std_bounds)
                xa = torch.cat([xn, a], dim=1)
                q = torch.stack([t(xa).squeeze(-1) for t in sac.targets]).min(0).values
                y = mb["reward"] + sac.gamma * mb["discount"] * (q - sac.log_alpha.exp() * logp)
        return y

    def grad_steps(n=40):
        for _ in range(n):
            sac.update(1)

    def updates():
        for _ in range(R):
            sac.update(G)

    work = {"sac_collect": (sac_collects, R * T), "replay": (replay_steps, R * T), "ppo_collect": (ppo_collects, R * T),
            "sample": (samples, 4000), "torch_sample": (torch_samples, 400), "act_target": (act_targets, 1000),
            "torch_target": (torch_targets, 1000), "grad_step": (grad_steps, 40), "update": (updates, R)}
    times = alternate(work, args.windows, host_per_call)
    med = times.median
    rate = lambda k: E / med[k]
    sample_bytes = 2 * 4 * B * (2 * D + A + 2) + 4 * B * (2 * offpolicy.SAMPLE_TRIES + 1)   # rows read and written; step types, mask
    round_s = med["sac_collect"] * T + med["update"]
    out = {
        "task": "RoboPianist-debug-TwinkleTwinkleRousseau-v0, hull fingertips, precision 64",
        "n_envs": E, "capacity": C, "batch": B, "obs_dim": D, "action_dim": A, "hidden": [sac.H1, sac.H2],
        "n_critics": sac.n_critics, "steps_per_round": T, "grad_steps_per_round": G, "windows": args.windows,
        "seconds_per_window": {k: med[k] * n for k, (_, n) in work.items()},
        "env_steps_per_s": {"sac_collect": rate("sac_collect"), "replay_of_recorded_actions": rate("replay"),
                            "ppo_collect": rate("ppo_collect")},
        "ms_per_control_step": {k: 1e3 * med[k] for k in ("sac_collect", "replay", "ppo_collect")},
        "sample_us": 1e6 * med["sample"], "torch_sample_us": 1e6 * med["torch_sample"], "sample_bytes": sample_bytes,
        "sample_bytes_per_s": sample_bytes / med["sample"],
        "sample_over_hbm_peak": {k: sample_bytes / med["sample"] / v for k, v in HBM_PEAK.items()},
        "act_target_us": 1e6 * med["act_target"], "torch_target_us": 1e6 * med["torch_target"],
        "grad_step_ms": 1e3 * med["grad_step"], "update_ms": 1e3 * med["update"],
        "round_ms": 1e3 * round_s, "update_share_of_round": med["update"] / round_s,
        "spread": {k: times.spread(k) for k in work},
        "method": "host clock around work that ends in a device synchronise; every workload warmed up once, then "
                  "alternating windows in one process; medians",
    }
    write_report(out, args.out, indent=1)


if __name__ == "__main__":
    main()
