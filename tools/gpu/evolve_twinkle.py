"""Eight members of TwinkleTwinkleLittleStar on the self-actuated piano with a deliberately spread `target_entropy` sweep
(-A x 0.125, 0.25, 0.5, 0.75, 1, 1.5, 2, 4), as profiles/pop_fused_twinkle.txt was made (4096 envs, the fused critic step,
--time-limit seconds), with or without population-based training.  Writes the lines of every fortieth round, every
replacement and the final per-member metrics to --out; run once with --evolve-every 0 and once with --evolve-every 50 and
join the two files into profiles/pop_evolve_twinkle.txt.

    python tools/gpu/evolve_twinkle.py --evolve-every 50 --out profiles/pop_evolve_twinkle_every50.txt
"""
import argparse
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from robopianist_amd import music, population  # noqa: E402
from robopianist_amd.suite import environment  # noqa: E402
from robopianist_amd.suite.tasks import SelfActuatedPiano  # noqa: E402

SWEEP = (0.125, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 4.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_envs", type=int, default=4096)
    ap.add_argument("--midi", default="TwinkleTwinkleLittleStar")
    ap.add_argument("--evolve-every", dest="every", type=int, default=0)
    ap.add_argument("--evolve-percent", dest="percent", type=int, default=25)
    ap.add_argument("--time-limit", type=float, default=280.0)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    P = len(SWEEP)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        task = SelfActuatedPiano(midi=music.load(args.midi), n_steps_lookahead=1, control_timestep=0.05)
        env = environment.Environment(task, n_envs=args.n_envs, precision=64)
    A = env.action_spec().shape[-1]
    lines = []

    def log(line):
        keep = not line.startswith("update") or (int(line.split()[1]) % 40 == 0)
        if keep:
            lines.append(line)
            print(line, flush=True)

    evolve = dict(every=args.every, percent=args.percent) if args.every else None
    pop, rounds, _ = population.train_and_evaluate(
        env, 10 ** 6, P, time_limit=args.time_limit, log=log, batch_size=max(1, min(4096, 16 * args.n_envs) // P),
        critic_step="fused", target_entropy=[-A * s for s in SWEEP], evolve=evolve)
    head = [f"# tools/gpu/evolve_twinkle.py --evolve-every {args.every} --evolve-percent {args.percent} --n_envs {args.n_envs} "
            f"--time-limit {args.time_limit:.0f}: {len(rounds)} rounds; target_entropy at the start = -{A} x {SWEEP}",
            f"# target_entropy at the end: {[round(float(v), 3) for v in pop.target_entropy.tolist()]}",
            f"# gamma at the end: {[round(float(v), 5) for v in pop.gamma.tolist()]}"]
    if evolve is not None:
        head.append(f"# generations: {pop.generation}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")


if __name__ == "__main__":
    main()
