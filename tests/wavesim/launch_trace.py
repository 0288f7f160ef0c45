"""TEST INFRASTRUCTURE: writes the launch traces of tests/golden/launch_trace -- what one rp_step / rp_forward /
rp_step_masked ENQUEUES (kernel launches with their instantiation, grid, block and stream; event records and waits;
asynchronous copies and fills), schedule by schedule, as the emulator's HIP stand-in logs it (wavesim.hpp: launch trace).

    python tests/wavesim/launch_trace.py OUTDIR [group ...]      one file OUTDIR/<group>.txt per group

A file has one line per case: `## <case>` and, for the engine's creation and every call, the number of enqueues and the
SHA-1 of their lines (twelve digits) -- any launch dropped, doubled, reordered, resized or put on another stream changes
it.  Representative cases (full=True below) are followed by the lines themselves, `# <call>` by call, runs of a repeated
block folded into `repeat N [ ... ]` -- the first call of the case, or the calls `full` names.
The raw log of a group stays beside its file as <group>.raw for reading a difference.

Kernels are NOT executed (WAVESIM_SKIP_KERNELS=1) except in the group "executed": a trace is host behaviour only, and a
6144-env engine then costs its allocation.  With the kernels skipped the device reports empty lists of envs outside the
light class, so the estimate behind `many_heavy` decays from its start value of 8 through both thresholds (4, then 2)
within sixteen steps: the automatic cases step that often and show the rule on both sides.  For every automatic case the
script prints which `sched` each step took.  tests/test_wavesim.py compares the files with the committed ones."""
import hashlib, os, re, sys, warnings
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("RP_ENGINE_LIB", os.path.join(HERE, "_build", "librp_engine_wavesim.so"))
os.environ["RP_SKIP_SELF_CHECK"] = "1"
os.environ.setdefault("WAVESIM_SITE", "0")
import numpy as np
from robopianist_amd import engine
from robopianist_amd.model import scene

_scenes = {}
_full = {}        # the cases whose lines go into the file: tag -> indices of the calls to print
AUTO_STEPS = 18


def fold(lines, maxp=48):
    """Runs of a repeated block of lines as `repeat N [ block ]` (greedy, the longest saving first; lossless)."""
    out, i = [], 0
    while i < len(lines):
        best = (0, 0, 0)
        for p in range(1, min(maxp, (len(lines) - i) // 2) + 1):
            k = 1
            while lines[i + k * p:i + (k + 1) * p] == lines[i:i + p]:
                k += 1
            if k > 1 and (k - 1) * p > best[0]:
                best = ((k - 1) * p, p, k)
        if best[0] >= 3:
            _, p, k = best
            out += [f"repeat {k} ["] + ["  " + l for l in fold(lines[i:i + p], maxp)] + ["]"]
            i += p * k
        else:
            out.append(lines[i])
            i += 1
    return out


def compact(raw):
    """The raw log (`## <case>: <call>` sections) as the committed form described at the top."""
    cases = {}
    for sec in raw.split("## ")[1:]:
        head, *lines = sec.splitlines()
        if head == "end":
            continue
        tag, call = head.rsplit(": ", 1)
        cases.setdefault(tag, []).append((call, lines))
    out = []
    for tag, calls in cases.items():
        digest = [hashlib.sha1("\n".join(l).encode()).hexdigest()[:12] for _, l in calls]
        out.append(f"## {tag}")
        out.append(" | ".join(f"{c} {len(l)} {d}" for (c, l), d in zip(calls, digest)))
        if tag in _full:
            for j, (c, l) in enumerate(calls):
                if c != "create" and j - 1 in _full[tag] and digest[j] not in digest[:j]:
                    out += [f"# {c}"] + fold(l)
    return "\n".join(out) + "\n"


def scene_of(kind):
    if kind not in _scenes:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            kw = {"prim": dict(primitive_fingertip_collisions=True), "hull": dict(primitive_fingertip_collisions=False),
                  "graph": dict(primitive_fingertip_collisions=False, mesh_colliders=200),
                  # (no forearm dofs: a two-link trunk, the solver builds that are not specialised for four)
                  "short-prim": dict(primitive_fingertip_collisions=True, forearm_dofs=()),
                  "short-hull": dict(primitive_fingertip_collisions=False, forearm_dofs=())}[kind]
            si = scene.build_scene(gravity_compensation=True, **kw)
        _scenes[kind] = (si, engine.make_blob(si.model, si.key_joint_ids))
    return _scenes[kind]


def sched_of(lines):
    """The schedule number the rule gave the step whose trace lines are `lines`: 3 = fused launches, otherwise by the
    number of streams that carry position stages (one: 1, two: 2, three: 4)."""
    if any(l.startswith("launch rp_fused_") for l in lines):
        return 3
    pos = [l for l in lines if re.match(r"launch (rp_stage_kernel<\w+, 0[,>]|rp_pos_front_kernel)", l)]
    return {1: 1, 2: 2, 3: 4}[len({l.split()[-1] for l in pos})]


def case(tag, kind="prim", nenv=8, precision=64, env=None, slices=1, fused=0, split=0, lean=None, order=False, sensors=False,
         nsub=1, legacy=True, lazy=False, capturing=(), steps=1, call="step", key_trace=False, execute=None, full=False):
    """One engine, `steps` calls.  capturing: the indices of the calls made with WAVESIM_CAPTURING=1 (True = all)."""
    if full:   # (True: the first call; or the indices of the calls to print)
        _full[tag] = {0} if full is True else set(full)
    L = engine.load_library()
    si, blob = scene_of(kind)
    env = dict(env or {})
    for k, v in env.items():
        os.environ[k] = v
    os.environ["WAVESIM_SKIP_KERNELS"] = "0" if execute else "1"
    L.wavesim_trace_begin(f"{tag}: create".encode())
    p = engine.BatchedPhysics(si.model, si.key_joint_ids, n_envs=nenv, precision=precision, blob=blob)
    for k in env:
        del os.environ[k]
    p.set_stream_slices(slices)
    if precision == 64 and "RP_FORCE_DEEP" not in env:
        p.set_split_position_stage(split)
    p.set_fused_substeps(fused)
    if lean is not None:
        p.set_lean_solver(lean)
    p.set_cost_ordered_launch(order); p.set_acc_sensors(sensors)
    p.set_legacy_step(legacy); p.set_lazy_position_stage(lazy)
    automatic = slices == 0
    taken = []
    for i in range(steps):
        if execute:
            execute(p, i)
        cap = capturing is True or i in capturing
        os.environ["WAVESIM_CAPTURING"] = "1" if cap else "0"
        L.wavesim_trace_begin(f"{tag}: {call} {i}{' capturing' if cap else ''}".encode())   # (": " splits case and call)
        trace = np.zeros((nenv, nsub, 4), np.uint32) if key_trace else None
        if call == "forward":
            p.forward()
        elif call == "masked":
            os.environ["WAVESIM_DEVICE_PTRS"] = "1"   # (the reset mask must be device memory)
            p.step_masked(nsub, trace, (np.arange(nenv) % 3 == 0).astype(np.uint8))
            os.environ["WAVESIM_DEVICE_PTRS"] = "0"
        else:
            p.step(nsub, trace)
        if automatic:
            lines = open(os.environ["WAVESIM_TRACE"]).read().split("## ")[-1].splitlines()[1:]
            taken.append(sched_of(lines))
    os.environ["WAVESIM_CAPTURING"] = "0"
    if automatic:
        print(f"{tag}: sched {' '.join(map(str, taken))}")
    return p


def small(kind, precision=64, deep=False):
    """Every setting at 8 envs on one scene (fp32 and the deep builds: the settings those builds have)."""
    t = f"{kind}{precision}{'-deep' if deep else ''}"
    env = {"RP_FORCE_DEEP": "1"} if deep else {}
    kw = dict(kind=kind, precision=precision, env=env)
    shown = kind == "prim" and precision == 64 and not deep   # (the other scenes and builds differ in the kernels' names)
    case(f"{t} per-stage", **kw, full=shown)
    case(f"{t} per-stage nsub 10 sensors", sensors=True, nsub=10, steps=3, **kw, full=shown)
    case(f"{t} per-stage order key-trace", order=True, nsub=2, key_trace=True, **kw)
    case(f"{t} forward", call="forward", **kw, full=shown)
    case(f"{t} masked lazy", call="masked", lazy=True, nsub=2, steps=2, **kw, full=shown)
    case(f"{t} legacy-off lazy", legacy=False, lazy=True, steps=2, **kw)
    case(f"{t} lazy", lazy=True, steps=2, **kw)
    case(f"{t} capturing", capturing=True, sensors=True, nsub=2, **kw, full=True)   # (every build shows its three stage kernels)
    case(f"{t} fused-asked", fused=1, nsub=2, **kw)   # (falls back to one launch per stage where there is no fused build)
    case(f"{t} auto", slices=0, fused="auto", steps=2, **kw)
    if precision != 64 or deep:
        return
    case(f"{t} lean-off sensors", lean=False, sensors=True, nsub=2, **kw)
    case(f"{t} lean-off order", lean=False, order=True, **kw)
    case(f"{t} RP_LEAN=0", kind=kind, env={"RP_LEAN": "0"})
    case(f"{t} RP_HEAVY_GRID=16", kind=kind, env={"RP_HEAVY_GRID": "16"}, steps=2)
    case(f"{t} RP_SPLIT_POS=0 RP_FUSED=0 auto", kind=kind, env={"RP_SPLIT_POS": "0", "RP_FUSED": "0"}, slices=0, fused="auto", split="auto", steps=2)
    case(f"{t} split", split=1, nsub=2, sensors=True, **kw, full=shown)
    case(f"{t} split order lean-off", split=1, order=True, lean=False, **kw)
    # (no allocation inside a capture: the first call falls back to the one-kernel stage, the third has the buffers)
    case(f"{t} split capturing", split=1, capturing=(0, 2), steps=3, **kw)
    case(f"{t} fused nsub 10 sensors order", fused=1, nsub=10, sensors=True, order=True, steps=2, **kw, full=shown)
    case(f"{t} fused", fused=1, nsub=2, **kw)
    case(f"{t} fused capturing", fused=1, capturing=(0, 2), steps=3, nsub=2, **kw)
    case(f"{t} fused RP_FUSED_SPLIT=0", kind=kind, env={"RP_FUSED_SPLIT": "0"}, fused=1, sensors=True, nsub=2)
    case(f"{t} fused key-trace masked", fused=1, call="masked", key_trace=True, nsub=2, **kw)
    for n in (2, 3, 4):
        case(f"{t} slices {n}", slices=n, **kw)   # (batches under 1024 envs are never sliced)
    case(f"{t} auto all", slices=0, fused="auto", split="auto", nsub=2, steps=AUTO_STEPS, **kw)
    case(f"{t} auto capturing", slices=0, fused="auto", split="auto", capturing=True, steps=2, **kw)
    case(f"{t} auto fused-off capturing", slices=0, fused=0, split="auto", capturing=True, **kw)


def short():
    """The general-trunk solver and clean-up builds (hands without forearm dofs), with and without hulls."""
    for kind in ("short-prim", "short-hull"):
        case(f"{kind}64 per-stage sensors", kind=kind, nsub=2, sensors=True)
        case(f"{kind}64 lean-off", kind=kind, lean=False)
        case(f"{kind}64 fused", kind=kind, fused=1, nsub=2, full=True)
        case(f"{kind}64 fused RP_FUSED_SPLIT=0", kind=kind, env={"RP_FUSED_SPLIT": "0"}, fused=1, nsub=2)
    case("short-prim32 per-stage", kind="short-prim", precision=32)


def sizes():
    """The rule's edges (kernels skipped): automatic and forced schedules at 1024 .. 6144 envs."""
    for nenv in (1024, 2048, 3072, 4096, 6144):
        t = f"prim64 {nenv} envs"
        # (many_heavy is on at first -- the estimate starts at 8 -- and off from the step it has decayed under 2: the 16th)
        p = case(f"{t} auto all", nenv=nenv, slices=0, fused="auto", split="auto", steps=AUTO_STEPS,
                 full=(0, 15) if nenv in (2048, 4096) else ())   # (call 15: the first with many_heavy off)
        case(f"{t} auto fused-off", nenv=nenv, slices=0, fused=0, split="auto", steps=AUTO_STEPS)
        if nenv in (2048, 4096):
            case(f"{t} auto fused-off split-off", nenv=nenv, slices=0, fused=0, split=0, steps=AUTO_STEPS)
            case(f"{t} auto all capturing", nenv=nenv, slices=0, fused="auto", split="auto", capturing=(0, 9, AUTO_STEPS - 1), steps=AUTO_STEPS)
            case(f"{t} auto fused-off capturing", nenv=nenv, slices=0, fused=0, split="auto", capturing=(0, 9, AUTO_STEPS - 1), steps=AUTO_STEPS)
            case(f"{t} auto sensors order masked", nenv=nenv, slices=0, fused="auto", split="auto", sensors=True, order=True,
                 call="masked", nsub=2, steps=AUTO_STEPS)
        del p
    for n in (1, 2, 3, 4):
        t = f"prim64 2048 envs slices {n}"
        case(f"{t}", nenv=2048, slices=n, nsub=2, sensors=True, steps=9, full=(8,) if n == 2 else ())   # (nine steps: past the split_step threshold)
        case(f"{t} split order", nenv=2048, slices=n, split=1, order=True)
        case(f"{t} lean-off", nenv=2048, slices=n, lean=False)
        case(f"{t} fused", nenv=2048, slices=n, fused=1)
        case(f"{t} capturing", nenv=2048, slices=n, capturing=True)
        case(f"{t} forward", nenv=2048, slices=n, call="forward")
    case("prim64 1024 envs slices 2 split auto", nenv=1024, slices=2, split="auto")
    case("prim32 2048 envs slices 2", nenv=2048, precision=32, slices=2, nsub=2, sensors=True)
    case("prim32 2048 envs auto", nenv=2048, precision=32, slices=0, fused="auto", steps=2)
    case("prim64-deep 2048 envs slices 3", nenv=2048, env={"RP_FORCE_DEEP": "1"}, slices=3)
    case("prim64-deep 4096 envs auto", nenv=4096, env={"RP_FORCE_DEEP": "1"}, slices=0, fused="auto", steps=2)


def executed():
    """Kernels executed: 16 envs, the light class capped (rp_set_lean_solver(e, n)) so that the lists of envs outside
    it are long -- the device reports them, the estimate stays at 4 or more, and the heavy envs' position stage goes
    with their solver launch to the companion stream (rp_pos_list_kernel) long after the start value has decayed."""
    import test_gpu_parity as tgp
    si, _ = scene_of("prim")
    nenv, nsteps = 16, 14
    ctrl = np.stack([tgp.ctrl_sequence(si.model, nsteps, 7 + e, hold=5, lo_frac=0.0, hi_frac=1.0) for e in range(nenv)], 1)

    def drive(p, i):
        p.set(engine.CTRL, ctrl[i])

    p = case("prim64 executed cap 2", nenv=nenv, lean=2, nsub=2, sensors=True, steps=nsteps, execute=drive, full=(0, nsteps - 1))
    print("executed: envs outside the light class after the last step:", int((p.get(engine.DEBUG_HANDOVER_HDR)[:, 6] != 1).sum()))


GROUPS = {
    "prim64": lambda: small("prim"), "hull64": lambda: small("hull"), "graph64": lambda: small("graph"),
    "deep64": lambda: [small(k, deep=True) for k in ("prim", "hull", "graph")], "prim32": lambda: small("prim", 32),
    "short64": short, "sizes": sizes, "executed": executed,
}


def main():
    outdir = sys.argv[1]
    os.makedirs(outdir, exist_ok=True)
    for g in sys.argv[2:] or list(GROUPS):
        raw = os.path.join(outdir, g + ".raw")
        os.environ["WAVESIM_TRACE"] = raw
        GROUPS[g]()
        engine.load_library().wavesim_trace_begin(b"end")
        with open(os.path.join(outdir, g + ".txt"), "w") as fh:
            fh.write(compact(open(raw).read()))


if __name__ == "__main__":
    main()
