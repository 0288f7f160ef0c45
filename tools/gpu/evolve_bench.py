"""Cost of population-based training's three entry points (include/learn/rp_evolve.h), of the same event done in torch, and
of DroQPopulation.train() with and without the evolve option (bench.py is left as it is).

E envs of the TwinkleTwinkle hands task with hull fingertips (bench.py's config 3), 256 x 256 units, two critics, the fused
critic step.  For every P of --members (batch --batch / P rows per member):

    fold_us / plan_us / copy_us     HIP events around --calls back-to-back calls on the learner's own arrays, per call; the
                                    windows are refilled before every plan (two device copies, timed alone as refill_us and
                                    not subtracted); copy moves the slices of a quarter of the members over the learner's
                                    whole field table (its launches: copy_launches)
    copy_largest_us                 the largest field alone, with its bytes read and written over the time as a share of
                                    the 8 TB/s HBM peak (MI355X; about 6.3 TB/s is what a plain float4 copy reaches)
    torch_event_us                  the same event in torch: the windows read back, a host sort, index_copy_ per tensor;
                                    a host clock around it, ending in a device synchronise
    event_us                        evolve() itself (plan + copy), host clock, ending in a device synchronise
    rounds_per_s_{off,every10}      train(--rounds, --steps-per-round, 1) with evolve=None (the parent commit's train():
                                    the override defers to it) and with every=10, alternating windows in one process

Every figure: a warm-up, then --windows repeats; the median with the lowest and the highest window.

    python tools/gpu/evolve_bench.py [--envs 4096] [--members 8,16] [--batch 4096] [--out profiles/evolve_bench.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from robopianist_amd import evolve, population, suite  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--members", default="8,16")
    ap.add_argument("--capacity", type=int, default=8)
    ap.add_argument("--batch", type=int, default=4096, help="rows of one range over all members")
    ap.add_argument("--utd", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10, help="rounds of train() per window")
    ap.add_argument("--steps-per-round", dest="steps", type=int, default=16)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evolve_bench.json"))
    args = ap.parse_args()
    E, C = args.envs, args.capacity
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = suite.load("RoboPianist-debug-TwinkleTwinkleRousseau-v0", seed=12345, n_envs=E, precision=64,
                         task_kwargs=dict(trim_silence=True, control_timestep=0.05, gravity_compensation=True,
                                          reduced_action_space=False, n_steps_lookahead=10))
    dev = env.physics.device
    sync = torch.cuda.synchronize
    st = torch.cuda.current_stream(dev).cuda_stream

    def stat(values, scale):
        return {"median": scale * float(np.median(values)), "lowest": scale * float(min(values)),
                "highest": scale * float(max(values))}

    def device_time(fn, n):
        """Seconds per call of n back-to-back calls, by HIP events."""
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        start.record()
        for _ in range(n):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e-3 / n

    def host_time(fn, n=1):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        sync()
        return (time.perf_counter() - t0) / n

    def repeats(measure):
        measure()   # warm-up
        return [measure() for _ in range(args.windows)]

    out = {"task": "RoboPianist-debug-TwinkleTwinkleRousseau-v0, hull fingertips, precision 64", "n_envs": E, "capacity": C,
           "batch_all_members": args.batch, "utd": args.utd, "steps_per_round": args.steps, "rounds_per_window": args.rounds,
           "calls_per_window": args.calls, "windows": args.windows, "members": {},
           "method": "HIP events around back-to-back calls for the kernels, a host clock around work that ends in a device "
                     "synchronise for the events and the rounds; a warm-up, then the median with the lowest and highest window"}
    for P in [int(p) for p in args.members.split(",")]:
        kw = dict(capacity=C, batch_size=args.batch // P, seed=1, utd=args.utd, critic_step="fused")
        on = population.DroQPopulation(env, P, evolve=dict(every=10, min_episodes=1), **kw)
        off = population.DroQPopulation(env, P, **kw)
        for pop in (on, off):
            pop.collect(C)
            pop.update(1)      # (the torch optimisers of the actor and the temperature now hold their moments)
        sync()
        table = on._field_table()
        names = [n for n, _ in on._member_fields()]
        words = sum(w for _, w in table)
        quarter = max(P // 4, 1)
        source = torch.arange(P, dtype=torch.int32, device=dev)
        source[P - quarter:] = torch.arange(quarter, dtype=torch.int32, device=dev)
        score = torch.linspace(1.0, 2.0, P, dtype=torch.float64, device=dev)
        count = torch.full((P,), 4, dtype=torch.int64, device=dev)
        o = on.evolve_options

        def refill():
            on._fit_sum.copy_(score)
            on._fit_count.copy_(count)

        def fold():
            evolve.fold(on._done_return.data_ptr(), on._done_count.data_ptr(), on._fit_sum.data_ptr(),
                        on._fit_count.data_ptr(), E, P, hip_stream=st)

        def plan():
            refill()
            evolve.plan(on._fit_sum.data_ptr(), on._fit_count.data_ptr(), on._source.data_ptr(), P, percent=o["percent"],
                        min_episodes=o["min_episodes"], min_gap=o["min_gap"], factors=o["factors"], gamma=on.gamma.data_ptr(),
                        gamma_bounds=o["gamma_bounds"], target_entropy=on.target_entropy.data_ptr(),
                        entropy_bounds=o["entropy_bounds"], seed=1, generation=3, hip_stream=st)

        def copy():
            return evolve.copy(table, source.data_ptr(), P, hip_stream=st)

        big = max(range(len(table)), key=lambda i: table[i][1])

        def copy_largest():
            evolve.copy([table[big]], source.data_ptr(), P, hip_stream=st)

        def event():
            refill()
            on.evolve()

        def torch_event():
            refill()
            mean = (on._fit_sum / on._fit_count.to(torch.float64)).cpu().numpy()      # the read-back
            order = np.argsort(-mean, kind="stable")                                   # the host sort
            k = min(P * o["percent"] // 100, P // 2)
            dst = torch.as_tensor(order[P - k:], device=dev)
            src = torch.as_tensor(order[np.arange(k) % max(k, 1)], device=dev)
            with torch.no_grad():
                for _, t in on._member_fields():
                    t.index_copy_(0, dst, t.index_select(0, src))
                on.gamma.index_copy_(0, dst, 1.0 - (1.0 - on.gamma.index_select(0, src)) * 0.8)
                on.target_entropy.index_copy_(0, dst, on.target_entropy.index_select(0, src) * 1.25)
            on._fit_sum.zero_()
            on._fit_count.zero_()

        r = {"fields": len(table), "copy_launches": copy(), "words_per_member": words, "members_replaced": quarter,
             "largest_field": {"name": names[big], "words_per_member": table[big][1]}}
        r["fold_us"] = stat(repeats(lambda: device_time(fold, args.calls)), 1e6)
        r["refill_us"] = stat(repeats(lambda: device_time(refill, args.calls)), 1e6)
        r["plan_us"] = stat(repeats(lambda: device_time(plan, args.calls)), 1e6)
        r["copy_us"] = stat(repeats(lambda: device_time(copy, args.calls)), 1e6)
        largest = repeats(lambda: device_time(copy_largest, args.calls))
        r["copy_largest_us"] = stat(largest, 1e6)
        moved = 2 * 4 * table[big][1] * quarter                                         # read and written
        r["copy_largest_bytes"] = moved
        r["copy_largest_share_of_hbm_peak"] = moved / float(np.median(largest)) / HBM_PEAK
        r["copy_bytes"] = 2 * 4 * words * quarter
        r["event_us"] = stat(repeats(lambda: host_time(event, 20)), 1e6)
        r["torch_event_us"] = stat(repeats(lambda: host_time(torch_event, 5)), 1e6)
        on._fit_sum.zero_()
        on._fit_count.zero_()
        # train(): alternating windows, the option off and on
        rate = {"off": [], "every10": []}
        for w in range(args.windows + 1):
            for key, pop in (("off", off), ("every10", on)):
                t = host_time(lambda: pop.train(args.rounds, args.steps, 1))
                if w:   # (the first window is the warm-up)
                    rate[key].append(args.rounds / t)
        r["rounds_per_s_off"], r["rounds_per_s_every10"] = stat(rate["off"], 1.0), stat(rate["every10"], 1.0)
        r["generations"] = on.generation
        round_s = 1.0 / r["rounds_per_s_off"]["median"]
        r["event_share_of_ten_rounds"] = r["event_us"]["median"] * 1e-6 / (10.0 * round_s)
        out["members"][str(P)] = r
        del on, off
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
