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
import os

import numpy as np
import torch

from _measure import HANDS, ROOT, Times, event_time, host_time, load_twinkle, write_report   # (puts ROOT on sys.path)
from robopianist_amd import evolve, population

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
    env = load_twinkle(E, precision=64, **HANDS)
    dev = env.physics.device
    st = torch.cuda.current_stream(dev).cuda_stream

    def repeats(measure):
        measure()   # warm-up
        return [measure() for _ in range(args.windows)]

    def device_s(fn):
        def measure():
            torch.cuda.synchronize()
            return event_time(fn, args.calls) * 1e-3
        return repeats(measure)

    def host_s(fn, n):
        return repeats(lambda: host_time(fn, n) / n)

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
        torch.cuda.synchronize()
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
        times = Times({"fold": device_s(fold), "refill": device_s(refill), "plan": device_s(plan), "copy": device_s(copy),
                       "copy_largest": device_s(copy_largest), "event": host_s(event, 20),
                       "torch_event": host_s(torch_event, 5)})                        # seconds per call
        on._fit_sum.zero_()
        on._fit_count.zero_()
        # train(): alternating windows, the option off and on
        rate = {"rounds_per_s_off": [], "rounds_per_s_every10": []}
        for i in range(args.windows + 1):
            for key, pop in (("rounds_per_s_off", off), ("rounds_per_s_every10", on)):
                t = host_time(lambda: pop.train(args.rounds, args.steps, 1))
                if i:   # (the first window is the warm-up)
                    rate[key].append(args.rounds / t)
        rates = Times(rate)
        for k in ("fold", "refill", "plan", "copy", "copy_largest"):
            r[f"{k}_us"] = times.stat(k, 1e6)
        moved = 2 * 4 * table[big][1] * quarter                                         # read and written
        r["copy_largest_bytes"] = moved
        r["copy_largest_share_of_hbm_peak"] = moved / times.median["copy_largest"] / HBM_PEAK
        r["copy_bytes"] = 2 * 4 * words * quarter
        for k in ("event", "torch_event"):
            r[f"{k}_us"] = times.stat(k, 1e6)
        for k in rate:
            r[k] = rates.stat(k, 1.0)
        r["generations"] = on.generation
        round_s = 1.0 / r["rounds_per_s_off"]["median"]
        r["event_share_of_ten_rounds"] = r["event_us"]["median"] * 1e-6 / (10.0 * round_s)
        out["members"][str(P)] = r
        del on, off
    write_report(out, args.out, indent=1)


if __name__ == "__main__":
    main()
