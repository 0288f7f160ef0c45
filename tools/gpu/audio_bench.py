"""Cost of the synthesiser's three kernels on a whole played episode (bench.py is left as it is).

The trace is the full TwinkleTwinkle scripted replay of one env (158 control steps = 1580 substeps, about 8.9 s of
audio with the tail), recorded with the pedal bit like wrappers.PianoSoundWrapper records it and copied to every env of
the batch.  Timed with device events after a warm-up, in windows of at least a second, the workloads alternating in one
process:

    notes      rp_audio_notes_from_trace
    synth      rp_audio_synthesize without pcm  (the synthesis kernel alone)
    synth_pcm  rp_audio_synthesize with pcm     (synthesis + peak / int16 kernel); pcm = synth_pcm - synth

Writes profiles/audio_bench.json: ms, samples/s, the multiple of real time and the mean audible voice-partials per
sample.

    python tools/gpu/audio_bench.py [--envs 256] [--windows 3] [--out profiles/audio_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/gpu/audio_bench.py --windows 1 --seconds 0.3
"""
import argparse
import os

import numpy as np
import torch

from _measure import ROOT, alternate, event_window, load_twinkle, scripted_replay, write_report


def record_replay_trace():
    """([T][4] int32 trace with the pedal in bit 88, dt) of env 0 over the scripted replay."""
    from robopianist_amd.music import synthesizer
    base = load_twinkle(2, record_key_trace=True, control_timestep=0.05, primitive_fingertip_collisions=True)
    env, script, n_steps = scripted_replay(base)
    env.reset()
    rows = []
    for _ in range(n_steps):
        ts = env.step(script)
        r = base.key_trace[0].clone()
        r[:, synthesizer.PEDAL_BIT // 32] |= base.task.piano.sustain_activation[0, 0].to(torch.int32) << (synthesizer.PEDAL_BIT % 32)
        rows.append(r)
        if bool(ts.last()[0]):
            break
    return torch.cat(rows), float(base.task.physics_timestep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--windows", type=int, default=3, help="timed windows per workload (each at least --seconds long)")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_bench.json"))
    args = ap.parse_args()

    from robopianist_amd.music import synthesizer
    one, dt = record_replay_trace()
    T, E = int(one.shape[0]), args.envs
    trace = one[None].expand(E, T, 4).contiguous()
    s = synthesizer.Synthesizer(n_envs=E, max_substeps=T, max_notes=4096, physics_timestep=dt)
    lengths = torch.full((E,), T, dtype=torch.int32, device=trace.device)
    n_cap = s.n_samples(T)
    wave, pcm = s.outputs(n_cap)
    a_notes = s.notes_args(trace, lengths, dt)
    a_synth = s.synth_args(lengths, dt, T, wave, None)
    a_both = s.synth_args(lengths, dt, T, wave, pcm)

    def call(fn, a):
        if fn(a) != 0:
            raise RuntimeError(s.last_error())

    work = {"notes": lambda: call(s.notes_raw, a_notes), "synth": lambda: call(s.synthesize_raw, a_synth),
            "synth_pcm": lambda: call(s.synthesize_raw, a_both)}

    for fn in work.values():   # warm-up (code objects)
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = alternate(work, args.windows, lambda fn: event_window(fn, args.seconds, first=2), warm=False)
    med, res = dict(times.median), times.windows
    med["pcm"] = med["synth_pcm"] - med["synth"]

    # what the synthesis kernel had to sum: audible voice-partials per sample of env 0's list
    count = int(s.notes["count"][0])
    key = s.notes["key"][0, :count].cpu().numpy()
    t_on = s.notes["t_on"][0, :count].cpu().numpy()
    t_off = s.notes["t_off"][0, :count].cpu().numpy()
    tb, sr = s.timbre, float(s.sample_rate)
    h = np.arange(1, tb["H"] + 1)
    f = h[None, :] * (440.0 * 2.0 ** ((key[:, None] + 21 - 69) / 12.0)) * np.sqrt(1 + np.asarray(tb["B"])[key][:, None] * h[None, :] ** 2)
    n_part = (f < 0.45 * sr).sum(1)
    audible = np.clip(np.minimum(t_off + 8 * tb["tau_rel"], n_cap / sr) - t_on, 0, None) * sr
    voice_partials = float((audible * n_part).sum() / n_cap)

    samples = E * n_cap
    out = {
        "device": torch.cuda.get_device_name(trace.device),
        "workload": f"TwinkleTwinkle scripted replay, {T} substeps of {dt} s = {n_cap} samples ({n_cap / sr:.2f} s) per env, "
                    f"{E} envs, {count} notes per env ({int(s.dropped[0])} dropped)",
        "method": f"device events, {args.windows} windows of >= {args.seconds} s per workload, alternating; medians; "
                  "pcm = synth_pcm - synth",
        "notes_ms": med["notes"], "synth_ms": med["synth"], "pcm_ms": med["pcm"], "synth_pcm_ms": med["synth_pcm"],
        "synth_samples_per_s": samples / (med["synth"] * 1e-3),
        "pcm_samples_per_s": samples / (med["pcm"] * 1e-3) if med["pcm"] > 0 else None,
        "notes_substeps_per_s": E * T / (med["notes"] * 1e-3),
        "times_real_time": {k: samples / sr / (med[k] * 1e-3) for k in ("notes", "synth", "pcm", "synth_pcm") if med[k] > 0},
        "mean_audible_voice_partials_per_sample": voice_partials,
        "synth_voice_partial_samples_per_s": samples * voice_partials / (med["synth"] * 1e-3),
        "windows_ms": res,
    }
    write_report(out, args.out, printed={k: v for k, v in out.items() if k != "windows_ms"})


if __name__ == "__main__":
    main()
