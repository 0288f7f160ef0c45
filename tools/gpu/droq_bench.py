"""Cost of DroQ's fused target, of its one-launch draw over all utd ranges and of its update next to SAC's (bench.py is
left as it is).

E envs of the TwinkleTwinkle hands task with hull fingertips (bench.py's config 3), sac_bench.py's method and shape: a
host clock around work that ends in a device synchronise, after a warm-up of every shape, the workloads alternating in
one process, windows of about half a second, medians over the windows and their spread:

    droq_target            rp_droq_target on B rows (dropout 0.01, two critics)
    torch_droq_target      the same target by torch: the normaliser, the cat, the target critics in train() mode (torch's
                           own dropout), the minimum and the target
    sac_target             rp_sac_target on the same rows with SAC's tanh critics, for scale
    draw_and_act_utd       DroQ.draw_and_act() at utd = U: one rp_sac_sample and one rp_sac_act of U B rows
    draw_and_act_separate  U pairs of rp_sac_sample and rp_sac_act of B rows each
    update_utd{1,4,U}      one DroQ.update(1) at that utd
    droq_collect           DroQ.collect(T), per control step
    sac_collect            SAC.collect(T) on the same env, per control step (the same code: it must lie within the spread)

    python tools/gpu/droq_bench.py [--envs 4096] [--capacity 64] [--batch 4096] [--utd 20] [--out profiles/droq_bench.json]
"""
import argparse
import os

import torch

from _measure import HANDS, ROOT, alternate, host_per_call, load_twinkle, write_report   # (puts ROOT on sys.path)
from robopianist_amd import droq, offpolicy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--utd", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=16, help="control steps per round")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=4, help="rounds' worth of control steps per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "droq_bench.json"))
    args = ap.parse_args()
    E, C, B, U, T, R = args.envs, args.capacity, args.batch, args.utd, args.horizon, args.rollouts
    env = load_twinkle(E, precision=64, **HANDS)
    utds = sorted({1, 4, U})
    sac = offpolicy.SAC(env, capacity=C, batch_size=B, seed=1)
    learners = {u: droq.DroQ(env, capacity=C, batch_size=B, seed=1, utd=u) for u in utds}
    one, big = learners[1], learners[U]
    dev, D, A = env.physics.device, sac.D, sac.A
    for l in [sac] + list(learners.values()):   # every ring is full from here on
        l.collect(C)
    st = torch.cuda.current_stream(dev).cuda_stream
    one.sample_and_target()                      # a minibatch of B rows, its policy outputs and y
    mb = one.minibatch()
    d_targets = [one._critic_table(t) for t in one.targets]
    s_targets = [sac._mlp(t) for t in sac.targets]
    common = lambda l: (mb["next_obs"].data_ptr(), mb["next_action"].data_ptr(), mb["next_logp"].data_ptr(),
                        mb["reward"].data_ptr(), mb["discount"].data_ptr(), l._mean_f32.data_ptr(),
                        l._inv_std_f32.data_ptr(), l.obs_clip, l.gamma, l.log_alpha.data_ptr())

    def droq_targets(n=1000):
        for i in range(n):
            droq.target(*common(one), d_targets, mb["y"].data_ptr(), D, one.H1, one.H2, A, B, threshold=one._threshold,
                        keep_scale=one._keep_scale, ln_eps=one.ln_eps, seed=1, round_=i, hip_stream=st)

    def torch_droq_targets(n=1000):
        with torch.no_grad():
            for _ in range(n):
                xa = torch.cat([one.normalize(mb["next_obs"]), mb["next_action"]], dim=1)
                q = torch.stack([t(xa).squeeze(-1) for t in one.targets]).min(0).values
                y = mb["reward"] + one.gamma * mb["discount"] * (q - one.log_alpha.exp() * mb["next_logp"])
        return y

    def sac_targets(n=1000):
        for _ in range(n):
            offpolicy.target(*common(sac), s_targets, mb["y"].data_ptr(), D, sac.H1, sac.H2, A, B, hip_stream=st)

    def draws_utd(n=20):
        for _ in range(n):
            big.draw_and_act()
            big._round += 1

    ring, smb, actor = sac.ring(), sac.minibatch(), sac._mlp(sac.actor)

    def draws_separate(n=20):
        for i in range(n):
            for u in range(U):
                offpolicy.sample(ring["obs"].data_ptr(), ring["action"].data_ptr(), ring["reward"].data_ptr(),
                                 ring["discount"].data_ptr(), ring["step_type"].data_ptr(), smb["obs"].data_ptr(),
                                 smb["next_obs"].data_ptr(), smb["action"].data_ptr(), smb["reward"].data_ptr(),
                                 smb["discount"].data_ptr(), smb["mask"].data_ptr(), sac.n_written, C, E, D, A, B, seed=1,
                                 round_=i * U + u, hip_stream=st)
                offpolicy.act(smb["next_obs"].data_ptr(), sac._mean_f32.data_ptr(), sac._inv_std_f32.data_ptr(),
                              sac.obs_clip, actor, D, sac.H1, sac.H2, A, B, log_std_bounds=sac.log_std_bounds,
                              action=smb["next_action"].data_ptr(), logp=smb["next_logp"].data_ptr(), seed=1,
                              round_=i * U + u, hip_stream=st)

    def updates(u, n):
        def run():
            for _ in range(n):
                learners[u].update(1)
        return run

    def collects(l):
        def run():
            for _ in range(R):
                l.collect(T)
        return run

    work = {"droq_target": (droq_targets, 1000), "torch_droq_target": (torch_droq_targets, 1000),
            "sac_target": (sac_targets, 1000), "draw_and_act_utd": (draws_utd, 20), "draw_and_act_separate": (draws_separate, 20),
            "droq_collect": (collects(big), R * T), "sac_collect": (collects(sac), R * T)}
    for u in utds:
        n = max(2, 120 // (3 * u))
        work[f"update_utd{u}"] = (updates(u, n), n)
    times = alternate(work, args.windows, host_per_call)
    med = times.median
    out = {
        "task": "RoboPianist-debug-TwinkleTwinkleRousseau-v0, hull fingertips, precision 64",
        "n_envs": E, "capacity": C, "batch": B, "obs_dim": D, "action_dim": A, "hidden": [one.H1, one.H2],
        "n_critics": one.n_critics, "dropout": one.dropout, "utd": U, "steps_per_round": T, "windows": args.windows,
        "seconds_per_window": {k: med[k] * n for k, (_, n) in work.items()},
        "droq_target_us": 1e6 * med["droq_target"], "torch_droq_target_us": 1e6 * med["torch_droq_target"],
        "sac_target_us": 1e6 * med["sac_target"],
        "draw_and_act_utd_ms": 1e3 * med["draw_and_act_utd"], "draw_and_act_separate_ms": 1e3 * med["draw_and_act_separate"],
        "ms_per_control_step": {k: 1e3 * med[k] for k in ("droq_collect", "sac_collect")},
        "update_ms": {str(u): 1e3 * med[f"update_utd{u}"] for u in utds},
        "update_share_of_round": {str(u): med[f"update_utd{u}"] / (med["droq_collect"] * T + med[f"update_utd{u}"])
                                  for u in utds},
        "spread": {k: times.spread(k) for k in work},
        "method": "host clock around work that ends in a device synchronise; every workload warmed up once, then "
                  "alternating windows in one process; medians",
    }
    write_report(out, args.out, indent=1)


if __name__ == "__main__":
    main()
