"""Cost of PPO's rollout collection and gradient step next to the plain env steps (bench.py is left as it is).

E envs of the TwinkleTwinkle hands task with hull fingertips (bench.py's config 3).  Timed with a host clock around work
that ends in a device synchronise, after a warm-up of every shape, the workloads alternating in one process, medians
over the windows:

    random    plain stepping under a uniform random canonical action (torch's uniform_, then step_canonical): the
              baseline, the unchanged engine
    collect   PPO.collect(): T x (rp_learn_act, step_canonical, rp_learn_pack), the critic at slot T, rp_learn_gae
    replay    plain stepping under the env actions the last collect() recorded (step_canonical alone): what the engine's
              steps cost under the policy's actions rather than uniform ones
    torch     the same loop with the policy evaluated by torch: cat of the observation tensors, the normaliser, the two
              Sequentials, normal_, the log-probability, the clamp and the copies into the storage
    act       one rp_learn_act of E rows (both networks), enqueued back to back
    pack      one rp_learn_pack of E rows (a kept TimeStep)
    update    one PPO.update() of the collected rollout (epochs x minibatches Adam steps, torch)
    moments   one PPO.update_normalizer() (rp_learn_moments over the rollout's T E rows)

Every timed window does `--rollouts` rollouts' worth of control steps (default 4 x 16 = 64 steps, about half a second at
4096 envs); every loop steps the env exactly as often as it is divided by.

    python tools/gpu/learn_bench.py [--envs 4096] [--horizon 16] [--out profiles/learn_bench.json]
"""
import argparse
import os

import torch

from _measure import HANDS, ROOT, alternate, host_per_call, load_twinkle, write_report   # (puts ROOT on sys.path)
from robopianist_amd import learning


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=4, help="rollouts (of `horizon` control steps) per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learn_bench.json"))
    args = ap.parse_args()
    E, T, R = args.envs, args.horizon, args.rollouts
    env = load_twinkle(E, precision=64, **HANDS)
    ppo = learning.PPO(env, horizon=T, seed=1)
    dev, D, A = env.physics.device, ppo.D, ppo.A
    bounds = ppo._bounds
    ua = torch.zeros((E, A), dtype=env.physics.dtype, device=dev)

    def random_steps():
        for _ in range(R * T):
            ua.uniform_(-1.0, 1.0)
            env.step_canonical(ua, bounds, False)

    def collects():
        for _ in range(R):
            ppo.collect()

    def replay_steps():
        recorded = ppo.rollout()["env_action"]
        for _ in range(R):
            for t in range(T):
                env.step_canonical(recorded[t], bounds, False)

    keys = ppo.observation_keys
    noise = torch.zeros((E, A), device=dev)
    half_log_2pi = 0.5 * A * learning.LOG_2PI

    last = [env.step_canonical(ua, bounds, False)]   # the TimeStep the torch loop continues from (outside the timing)

    def torch_steps():
        r = ppo.rollout()
        ts = last[0]
        with torch.no_grad():
            for t in (t for _ in range(R) for t in range(T)):
                obs = torch.cat([ts.observation[k].reshape(E, -1).float() for k in keys], dim=1)
                r["obs"][t].copy_(obs)
                xn = ppo.normalize(obs)
                mu, v = ppo.actor(xn), ppo.critic(xn).squeeze(-1)
                noise.normal_()
                a = mu + ppo.log_std.exp() * noise
                logp = (-0.5 * noise * noise - ppo.log_std).sum(-1) - half_log_2pi
                r["action"][t].copy_(a); r["logp"][t].copy_(logp); r["value"][t].copy_(v)
                r["env_action"][t].copy_(a.clamp(-1.0, 1.0))
                ts = env.step_canonical(r["env_action"][t], bounds, False)
                r["reward"][t + 1].copy_(ts.reward); r["discount"][t + 1].copy_(ts.discount)
                r["step_type"][t + 1].copy_(ts.step_type)
        last[0] = ts

    ts_kept = env.step_canonical(ua, bounds, False)
    st = torch.cuda.current_stream(dev).cuda_stream
    actor, critic = ppo._mlp(ppo.actor), ppo._mlp(ppo.critic)

    def acts(n=2000):
        for _ in range(n):
            learning.act(ppo._obs[0].data_ptr(), ppo._mean_f32.data_ptr(), ppo._inv_std_f32.data_ptr(), ppo.obs_clip, actor,
                         critic, D, ppo.H1, ppo.H2, A, E, log_std=ppo.log_std.data_ptr(), action=ppo._action[0].data_ptr(),
                         logp=ppo._logp[0].data_ptr(), env_action=ppo._env_action[0].data_ptr(),
                         value=ppo._value[0].data_ptr(), precision=64, seed=1, round_=0, hip_stream=st)

    def packs(n=5000):
        for _ in range(n):
            ppo._pack(ts_kept, 1, st)

    def updates():
        for _ in range(R):
            ppo.update()

    def moments(n=20):
        for _ in range(n):
            ppo.update_normalizer()

    # (collect right before update: the update reads the rollout the collection left in the storage)
    work = {"random": (random_steps, R * T), "collect": (collects, R * T), "update": (updates, R), "moments": (moments, 20),
            "replay": (replay_steps, R * T), "torch": (torch_steps, R * T), "act": (acts, 2000), "pack": (packs, 5000)}
    times = alternate(work, args.windows, host_per_call)
    med = times.median
    rate = lambda k: E / med[k]
    out = {
        "task": "RoboPianist-debug-TwinkleTwinkleRousseau-v0, hull fingertips, precision 64",
        "n_envs": E, "horizon": T, "obs_dim": D, "action_dim": A, "hidden": [ppo.H1, ppo.H2],
        "epochs": ppo.epochs, "minibatches": ppo.minibatches, "windows": args.windows,
        "control_steps_per_window": R * T,
        "env_steps_per_s": {"random": rate("random"), "collect": rate("collect"), "policy_replay": rate("replay"),
                            "torch_policy": rate("torch")},
        "ms_per_control_step": {k: 1e3 * med[k] for k in ("random", "collect", "replay", "torch")},
        "act_us": 1e6 * med["act"], "pack_us": 1e6 * med["pack"], "update_ms": 1e3 * med["update"],
        "moments_ms": 1e3 * med["moments"],
        "rollout_ms": 1e3 * med["collect"] * T, "update_over_rollout": med["update"] / (med["collect"] * T),
        "update_and_moments_over_rollout": (med["update"] + med["moments"]) / (med["collect"] * T),
        "spread": {k: times.spread(k) for k in work},
        "method": "host clock around work that ends in a device synchronise; every workload warmed up once, then "
                  "alternating windows in one process; medians",
    }
    write_report(out, args.out, indent=1)


if __name__ == "__main__":
    main()
