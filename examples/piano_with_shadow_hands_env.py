"""Batched, headless counterpart of the reference's examples/piano_with_shadow_hands_env.py.

Same flags (argparse instead of absl; no viewer: the interactive viewer is out of scope; --record writes the first
env's sound as a WAV file, --record --video its picture and sound as an AVI file: wrappers/sound.py), plus --n_envs /
--precision, --record_dir, --pixels (camera images in the observation: wrappers/pixels.py), --hear (what every env hears in the
observation: wrappers/hearing.py) and --plan (predictive sampling: suite/predictive_pianist.py; plays the episode twice, once
with the nominal alone -- zeros, or FingeringPianist with --fingertip-pianist -- and once with the planner refining it, and
prints both returns and F1s).  Replays an action sequence (or holds zeros) for one
episode in every env and prints the musical metrics and the throughput, e.g. BASELINE config #2:

    python examples/piano_with_shadow_hands_env.py \\
        --env_name RoboPianist-debug-TwinkleTwinkleRousseau-v0 --canonicalize --trim_silence \\
        --gravity_compensation --primitive_fingertip_collisions --n_steps_lookahead 10 \\
        --action_sequence tests/golden/twinkle_twinkle_actions.npy --n_envs 4096
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from robopianist_amd import suite  # noqa: E402
from robopianist_amd.suite.fingertip_pianist import FingeringPianist  # noqa: E402
from robopianist_amd.suite.predictive_pianist import PredictivePianist  # noqa: E402
from robopianist_amd.wrappers import (AudioObservationWrapper, CanonicalSpecWrapper, FingertipActionWrapper,  # noqa: E402
                                      MidiEvaluationWrapper, PianoSoundVideoWrapper, PianoSoundWrapper, PixelWrapper)


def _task_kwargs(args):
    return dict(
        change_color_on_activation=True, trim_silence=args.trim_silence,
        control_timestep=args.control_timestep, gravity_compensation=args.gravity_compensation,
        primitive_fingertip_collisions=args.primitive_fingertip_collisions,
        reduced_action_space=args.reduced_action_space, n_steps_lookahead=args.n_steps_lookahead,
        disable_fingering_reward=args.disable_fingering_reward,
        disable_forearm_reward=args.disable_forearm_reward,
        disable_colorization=args.disable_colorization,
        disable_hand_collisions=args.disable_hand_collisions, attachment_yaw=args.attachment_yaw)


def _load(args, n_envs):
    return suite.load(
        environment_name=args.env_name, midi_file=args.midi_file, stretch=args.stretch, shift=args.shift,
        seed=args.seed, n_envs=n_envs, precision=args.precision, record_key_trace=args.record or args.hear,
        task_kwargs=_task_kwargs(args))


def _load_members(args, n_envs, names):
    """As `_load` with the task's `midi=[one song per name]`: env e plays song e % len(names)."""
    from robopianist_amd import music
    from robopianist_amd.suite import environment
    from robopianist_amd.suite.tasks import piano_with_shadow_hands
    songs = dict(zip(suite.ALL, list(music.PIG_MIDIS) + list(music.ETUDE_MIDIS) + list(music.DEBUG_MIDIS)))
    for name in names:
        if name not in songs:
            raise ValueError(f"Unknown environment {name}. Available environments: {suite.ALL}")
    midis = [music.load(songs[name], stretch=args.stretch, shift=args.shift) for name in names]
    task = piano_with_shadow_hands.PianoWithShadowHands(midi=midis, **_task_kwargs(args))
    return environment.Environment(task, n_envs=n_envs, random_state=args.seed, precision=args.precision)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--env_name", default="RoboPianist-debug-TwinkleTwinkleLittleStar-v0")
    ap.add_argument("--midi_file", default=None)
    ap.add_argument("--control_timestep", type=float, default=0.05)
    ap.add_argument("--stretch", type=float, default=1.0)
    ap.add_argument("--shift", type=int, default=0)
    for flag in ("gravity_compensation", "trim_silence", "primitive_fingertip_collisions",
                 "reduced_action_space", "disable_fingering_reward", "disable_forearm_reward",
                 "disable_colorization", "disable_hand_collisions", "canonicalize"):
        ap.add_argument("--" + flag, action="store_true")
    ap.add_argument("--n_steps_lookahead", type=int, default=1)
    ap.add_argument("--attachment_yaw", type=float, default=0.0)
    ap.add_argument("--action_sequence", default=None,
                    help="npy file with a sequence of actions to replay in every env")
    ap.add_argument("--n_envs", type=int, default=1024)
    ap.add_argument("--precision", type=int, default=64, choices=(32, 64))
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--pixels", action="store_true",
                    help="wrap the env in PixelWrapper (84 x 84 images of the piano/back camera) and print the pixels spec")
    ap.add_argument("--hear", action="store_true",
                    help="wrap the env in AudioObservationWrapper (88 magnitudes of the last 2048 samples at 16 kHz) and print "
                         "the observation's shape and the loudest bin's key of env 0 every step")
    ap.add_argument("--fingertip-pianist", dest="fingertip_pianist", action="store_true",
                    help="command the hands in fingertip space (FingertipActionWrapper, absolute targets) and let "
                         "FingeringPianist play: every finger the MIDI's fingering assigns to a key aims at it; prints the "
                         "episode's F1")
    ap.add_argument("--press_depth", type=float, default=0.01,
                    help="with --fingertip-pianist: metres below a key's surface target the assigned finger aims at")
    ap.add_argument("--ik_iterations", type=int, default=1, help="with --fingertip-pianist: IK steps per control step")
    ap.add_argument("--plan", action="store_true",
                    help="predictive sampling (PredictivePianist): every control step, --plan_candidates action splines per env "
                         "are rolled out --plan_horizon steps in a second environment of n_envs x candidates envs and the best "
                         "one's first action is taken; with --fingertip-pianist the plan is seeded from FingeringPianist")
    ap.add_argument("--plan_candidates", type=int, default=16)
    ap.add_argument("--plan_horizon", type=int, default=5)
    ap.add_argument("--plan_knots", type=int, default=2)
    ap.add_argument("--plan_spline", default="linear", choices=("linear", "zero"))
    ap.add_argument("--plan_sigma", type=float, default=None,
                    help="noise around the nominal, in the action's units (default: 0.005 m with --fingertip-pianist, else 0.1)")
    ap.add_argument("--record", action="store_true",
                    help="record env 0 with PianoSoundWrapper and write its episode as a WAV file")
    ap.add_argument("--video", action="store_true",
                    help="with --record: film env 0 as well (PianoSoundVideoWrapper) and write an AVI file with picture and sound")
    ap.add_argument("--record_dir", default="recordings")
    ap.add_argument("--train-ppo", type=int, default=0, metavar="UPDATES",
                    help="train a policy with learning.PPO for that many updates instead of stepping a fixed one; prints the "
                         "mean episode return per update and the F1 of the trained policy at the end")
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
    ap.add_argument("--member-envs", dest="member_envs", default=None, metavar="NAME[,NAME...]",
                    help="--train-population: environment names of suite.ALL, one (every member learns that song) or "
                         "--members of them (member p learns song p); default: --env_name")
    ap.add_argument("--evolve-every", dest="evolve_every", type=int, default=0, metavar="N",
                    help="--train-population: population-based training (population.DroQPopulation(evolve=...)): after "
                         "every N rounds the worst members take the best members' networks, with gamma and target_entropy "
                         "perturbed; 0 (the default): the members stay independent")
    ap.add_argument("--evolve-percent", dest="evolve_percent", type=int, default=25, metavar="Q",
                    help="--evolve-every: the share of the members at either end, in percent")
    ap.add_argument("--time-limit", type=float, default=None,
                    help="--train-ppo, --train-sac, --train-droq, --train-population: stop after that many seconds")
    args = ap.parse_args()
    if args.video and not args.record:
        ap.error("--video needs --record")
    if args.fingertip_pianist and (args.canonicalize or args.action_sequence):
        ap.error("--fingertip-pianist commands fingertips: it takes neither --canonicalize nor --action_sequence")

    if args.plan and (args.canonicalize or args.action_sequence or args.pixels or args.hear or args.record):
        ap.error("--plan goes with --fingertip-pianist or alone: not with --canonicalize, --action_sequence, --pixels, --hear "
                 "or --record")

    def load(n_envs):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return _load(args, n_envs)

    if args.fused_critic and not (args.train_droq > 0 or args.train_population > 0):
        ap.error("--fused-critic goes with --train-droq or --train-population")
    if args.fused_actor and not args.train_droq > 0:
        ap.error("--fused-actor goes with --train-droq")
    if args.evolve_every and not args.train_population > 0:
        ap.error("--evolve-every goes with --train-population")
    evolve = dict(every=args.evolve_every, percent=args.evolve_percent) if args.evolve_every else None
    if (args.train_ppo > 0) + (args.train_sac > 0) + (args.train_droq > 0) + (args.train_population > 0) > 1:
        ap.error("--train-ppo, --train-sac, --train-droq and --train-population are four learners: choose one")
    if args.train_population > 0:
        if (args.fingertip_pianist or args.plan or args.action_sequence or args.pixels or args.hear or args.record
                or args.canonicalize):
            ap.error("--train-population trains on the plain environment: it goes with the task flags only")
        names = [n for n in (args.member_envs or args.env_name).split(",") if n]
        if len(names) not in (1, args.members):
            ap.error(f"--member-envs takes one name or --members = {args.members} names, got {len(names)}")
        from robopianist_amd import population
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            env = _load_members(args, args.n_envs, names)
        population.train_and_evaluate(env, args.train_population, args.members, time_limit=args.time_limit, seed=args.seed,
                                      batch_size=max(1, min(4096, 16 * args.n_envs) // args.members),
                                      critic_step="fused" if args.fused_critic else "torch", evolve=evolve)
        return
    if args.train_droq > 0:
        if (args.fingertip_pianist or args.plan or args.action_sequence or args.pixels or args.hear or args.record
                or args.canonicalize):
            ap.error("--train-droq trains on the plain environment: it goes with the task flags only")
        from robopianist_amd import droq
        droq.train_and_evaluate(load(args.n_envs), args.train_droq, time_limit=args.time_limit, seed=args.seed,
                                batch_size=min(4096, 16 * args.n_envs),
                                critic_step="fused" if args.fused_critic else "torch",
                                actor_step="fused" if args.fused_actor else "torch")
        return
    if args.train_sac > 0:
        if (args.fingertip_pianist or args.plan or args.action_sequence or args.pixels or args.hear or args.record
                or args.canonicalize):
            ap.error("--train-sac trains on the plain environment: it goes with the task flags only")
        from robopianist_amd import offpolicy
        offpolicy.train_and_evaluate(load(args.n_envs), args.train_sac, time_limit=args.time_limit, seed=args.seed,
                                     batch_size=min(4096, 16 * args.n_envs))
        return
    if args.train_ppo > 0:
        if (args.fingertip_pianist or args.plan or args.action_sequence or args.pixels or args.hear or args.record
                or args.canonicalize):
            ap.error("--train-ppo trains on the plain environment: it goes with the task flags only")
        from robopianist_amd import learning
        learning.train_and_evaluate(load(args.n_envs), args.train_ppo, time_limit=args.time_limit, seed=args.seed)
        return

    env = load(args.n_envs)
    pianist = fingertips = None
    if args.fingertip_pianist:
        env = fingertips = FingertipActionWrapper(env, mode="absolute", iterations=args.ik_iterations)
        pianist = FingeringPianist(env, press_depth=args.press_depth)
    if args.canonicalize:
        env = CanonicalSpecWrapper(env)
    env = MidiEvaluationWrapper(env)
    planner = None
    if args.plan:
        def make_plan_env(n_envs):
            e = load(n_envs)
            return FingertipActionWrapper(e, mode="absolute", iterations=args.ik_iterations) if args.fingertip_pianist else e
        sigma = args.plan_sigma if args.plan_sigma is not None else (0.005 if args.fingertip_pianist else 0.1)
        planner = PredictivePianist(env, make_plan_env, n_candidates=args.plan_candidates, horizon=args.plan_horizon,
                                    n_knots=args.plan_knots, spline=args.plan_spline, sigma=sigma, seed=args.seed,
                                    seed_from=pianist)
        print(f"Planner: {args.plan_candidates} candidates x {args.plan_horizon} steps, {args.plan_knots} knots "
              f"({args.plan_spline}), sigma {sigma}; planning env: {planner.sampler.E} envs")
    if args.pixels:
        env = PixelWrapper(env, render_kwargs=dict(height=84, width=84, camera_id="piano/back"))
        spec = env.observation_spec()["pixels"]
        print(f"Pixels spec: shape {spec.shape} dtype {spec.dtype} (collision geometry, camera piano/back)")
    if args.hear:
        env = AudioObservationWrapper(env)
        spec = env.observation_spec()["audio"]
        print(f"Audio spec: shape {spec.shape} dtype {spec.dtype} (one magnitude per key fundamental)")

    if args.record and args.video:
        env = PianoSoundVideoWrapper(env, record_dir=args.record_dir, record_envs=(0,), record_every=1,
                                     camera_id="piano/back", height=480, width=640)
    elif args.record:
        env = PianoSoundWrapper(env, record_dir=args.record_dir, record_envs=(0,), record_every=1)

    action_spec = env.action_spec()
    E, dev = args.n_envs, env.physics.device
    zeros = np.zeros(action_spec.shape, dtype=np.float64)
    zeros[-1] = -1.0  # sustain pedal off
    print(f"Action dimension: {action_spec.shape}   envs: {E}")
    timestep = env.reset()
    dim = 0
    for k, v in timestep.observation.items():
        print(f"\t{k}: {tuple(v.shape[1:])} {v.dtype}")
        dim += int(np.prod(v.shape[1:]))
    print(f"Observation dimension: {dim}")
    print(f"Control frequency: {1 / args.control_timestep} Hz")

    actions = np.load(args.action_sequence) if args.action_sequence else None

    def episode(use_planner):
        nonlocal timestep
        n_steps, ret = 0, torch.zeros(E, device=dev, dtype=env.physics.dtype)
        t0 = time.perf_counter()
        while True:
            if use_planner:
                timestep = planner.step()
            elif pianist is not None:
                a, weights = pianist.action()
                fingertips.set_weights(weights, validate=False)
                timestep = env.step(a)
            else:
                a = actions[n_steps] if actions is not None and n_steps < len(actions) else zeros
                timestep = env.step(torch.as_tensor(a, device=dev, dtype=env.physics.dtype).expand(E, -1))
            ret += timestep.reward
            n_steps += 1
            if args.hear:   # (a demonstration: the read-back is this print's, not the wrapper's)
                audio = timestep.observation["audio"]
                loud = int(audio[0].argmax())
                print(f"step {n_steps}: audio {tuple(audio.shape)}, env 0 loudest bin: key {loud} at {float(audio[0, loud]):.4f}")
            if bool(timestep.last().all()):   # all envs play the same song: they finish together
                break
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"episode: {n_steps} control steps x {E} envs in {dt:.2f} s = {E * n_steps / dt:,.0f} env-steps/s")
        print(f"mean return {float(ret.mean()):.3f}")
        metrics = env.get_musical_metrics()
        for k, v in metrics.items():
            print(f"\t{k}: {v:.4f}")
        return float(ret.mean()), metrics

    nominal_return, metrics = episode(False)
    if pianist is not None:
        print(f"fingertip pianist: F1 {metrics['f1']:.4f} (press depth {args.press_depth} m, {args.ik_iterations} IK step(s) per control step)")
    if planner is not None:
        nominal_f1 = metrics["f1"]
        timestep = env.reset()
        plan_return, metrics = episode(True)
        print(f"predictive sampling: return {plan_return:.3f}, F1 {metrics['f1']:.4f}; the nominal alone "
              f"({'FingeringPianist' if pianist is not None else 'zeros'}): return {nominal_return:.3f}, F1 {nominal_f1:.4f}")
        print(f"planning env warn flags: {int(planner.sampler.plan_env.physics.warn.max())}")
    print(f"warn flags: {int(env.physics.warn.max())}")
    if args.record:
        print("recorded: " + (", ".join(str(p) for p in env.written) or "nothing (the episode has no note)"))


if __name__ == "__main__":
    main()
