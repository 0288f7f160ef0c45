"""Batched, headless counterpart of the reference's examples/self_actuated_piano_env.py: the
self-actuated piano played by the oracle policy of that example (ctrl = ctrlrange max on the
goal keys, min elsewhere; last action entry = goal sustain), which reaches F1 = 1."""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from robopianist_amd import music  # noqa: E402
from robopianist_amd.suite import environment  # noqa: E402
from robopianist_amd.suite.tasks import SelfActuatedPiano  # noqa: E402
from robopianist_amd.wrappers import MidiEvaluationWrapper  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--midi", default="TwinkleTwinkleLittleStar", help="library name or .mid path")
    ap.add_argument("--control_timestep", type=float, default=0.05)
    ap.add_argument("--n_envs", type=int, default=16)
    ap.add_argument("--precision", type=int, default=64, choices=(32, 64))
    ap.add_argument("--train-ppo", type=int, default=0, metavar="UPDATES",
                    help="train a policy with learning.PPO for that many updates instead of playing the oracle policy; "
                         "prints the mean episode return per update and the F1 of the trained policy at the end")
    ap.add_argument("--train-sac", type=int, default=0, metavar="ROUNDS",
                    help="train a policy with offpolicy.SAC for that many rounds (16 control steps and 4 gradient steps "
                         "each) instead; prints the same lines and the F1 of the trained policy at the end")
    ap.add_argument("--train-droq", type=int, default=0, metavar="ROUNDS",
                    help="train a policy with droq.DroQ for that many rounds (16 control steps and one actor step of 20 "
                         "critic steps each) instead; prints the same lines and the F1 of the trained policy at the end")
    ap.add_argument("--fused-critic", action="store_true",
                    help="--train-droq, --train-population: take the critic steps with the fused HIP step "
                         "(droq.DroQ / population.DroQPopulation(critic_step=\"fused\")) instead of torch's autograd, "
                         "Adam and lerp")
    ap.add_argument("--fused-actor", action="store_true",
                    help="--train-droq: take the actor and temperature steps with the fused HIP step "
                         "(droq.DroQ(actor_step=\"fused\")) instead of torch's autograd and its two Adams")
    ap.add_argument("--train-population", type=int, default=0, metavar="ROUNDS",
                    help="train --members independent DroQ learners (population.DroQPopulation; member p owns the envs "
                         "e %% members == p) for that many rounds instead; prints the same lines and the F1, per member")
    ap.add_argument("--members", type=int, default=8, help="--train-population: the number of members (divides --n_envs)")
    ap.add_argument("--evolve-every", dest="evolve_every", type=int, default=0, metavar="N",
                    help="--train-population: population-based training (population.DroQPopulation(evolve=...)): after "
                         "every N rounds the worst members take the best members' networks, with gamma and target_entropy "
                         "perturbed; 0 (the default): the members stay independent")
    ap.add_argument("--evolve-percent", dest="evolve_percent", type=int, default=25, metavar="Q",
                    help="--evolve-every: the share of the members at either end, in percent")
    ap.add_argument("--time-limit", type=float, default=None,
                    help="--train-ppo, --train-sac, --train-droq, --train-population: stop after that many seconds")
    args = ap.parse_args()
    if args.fused_critic and not (args.train_droq > 0 or args.train_population > 0):
        ap.error("--fused-critic goes with --train-droq or --train-population")
    if args.fused_actor and not args.train_droq > 0:
        ap.error("--fused-actor goes with --train-droq")
    if args.evolve_every and not args.train_population > 0:
        ap.error("--evolve-every goes with --train-population")
    evolve = dict(every=args.evolve_every, percent=args.evolve_percent) if args.evolve_every else None
    if (args.train_ppo > 0) + (args.train_sac > 0) + (args.train_droq > 0) + (args.train_population > 0) > 1:
        ap.error("--train-ppo, --train-sac, --train-droq and --train-population are four learners: choose one")
    if args.train_ppo > 0 or args.train_sac > 0 or args.train_droq > 0 or args.train_population > 0:
        from robopianist_amd import droq, learning, offpolicy, population
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            task = SelfActuatedPiano(midi=music.load(args.midi), n_steps_lookahead=1,
                                     control_timestep=args.control_timestep)
            env = environment.Environment(task, n_envs=args.n_envs, precision=args.precision)
        if args.train_sac > 0:
            offpolicy.train_and_evaluate(env, args.train_sac, time_limit=args.time_limit,
                                         batch_size=min(4096, 16 * args.n_envs))
        elif args.train_droq > 0:
            droq.train_and_evaluate(env, args.train_droq, time_limit=args.time_limit,
                                    batch_size=min(4096, 16 * args.n_envs),
                                    critic_step="fused" if args.fused_critic else "torch",
                                    actor_step="fused" if args.fused_actor else "torch")
        elif args.train_population > 0:
            population.train_and_evaluate(env, args.train_population, args.members, time_limit=args.time_limit,
                                          batch_size=max(1, min(4096, 16 * args.n_envs) // args.members),
                                          critic_step="fused" if args.fused_critic else "torch", evolve=evolve)
        else:
            learning.train_and_evaluate(env, args.train_ppo, time_limit=args.time_limit)
        return
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        task = SelfActuatedPiano(midi=music.load(args.midi), n_steps_lookahead=1,
                                 control_timestep=args.control_timestep, change_color_on_activation=True)
        env = MidiEvaluationWrapper(environment.Environment(task, n_envs=args.n_envs, precision=args.precision))
    spec = env.action_spec()
    lo = torch.as_tensor(spec.minimum, device=env.physics.device)
    hi = torch.as_tensor(spec.maximum, device=env.physics.device)
    timestep = env.reset()
    n, ret = 0, 0.0
    while True:
        goal = timestep.observation["goal"][:, :89]           # current goal: 88 keys + sustain
        action = torch.where(goal > 0, hi, lo)
        timestep = env.step(action)
        ret += float(timestep.reward.mean())
        n += 1
        if bool(timestep.last().all()):
            break
    print(f"{n} control steps x {args.n_envs} envs, mean return {ret:.3f}")
    for k, v in env.get_musical_metrics().items():
        print(f"\t{k}: {v:.4f}")


if __name__ == "__main__":
    main()
