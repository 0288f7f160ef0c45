"""The reset snapshot (tests/test_gpu_reset_snapshot.py) without a GPU: switch on against switch off, bit for bit, on the
CPU wave emulator (tests/wavesim), which runs the engine's own kernel and host sources -- and what the engine enqueues
with the snapshot, read from the emulator's launch trace."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
WS = os.path.join(HERE, "wavesim")
CSRC = os.path.join(os.path.dirname(HERE), "robopianist_amd", "csrc")
CASES = ["one_kernel", "lazy_split_ordered", "fused_lazy", "fp32", "tree_offset", "options", "legacy_off"]


def _emulator_build():
    """tests/wavesim/_build/librp_engine_wavesim.so, rebuilt when a source is newer (tests/test_wavesim.py builds the
    same file)."""
    lib = os.path.join(WS, "_build", "librp_engine_wavesim.so")
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))] + \
           [os.path.join(WS, f) for f in ("wavesim.cpp", "wavesim.hpp", "build.sh")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call([os.path.join(WS, "build.sh")], stdout=subprocess.DEVNULL)
    return lib


def _env(**kw):
    env = dict(os.environ, RP_ENGINE_LIB=_emulator_build(), WAVESIM_SITE="0", RP_SKIP_SELF_CHECK="1", **kw)
    for k in [k for k in env if k.startswith("RP_") and k not in ("RP_ENGINE_LIB", "RP_SKIP_SELF_CHECK")]:
        del env[k]
    return env


def test_reset_snapshot_on_the_wave_emulator():
    """8 envs, hull fingertips, ten control steps with the reset patterns (one env, two, first and last, the same env twice
    running, all at once, one in contact with a warn bit) under the one-kernel, split and fused schedules, lazy mode on
    and off, fp32, and the fallbacks (tree offsets, an option setter between resets, legacy_step off)."""
    out = subprocess.run([sys.executable, os.path.join(WS, "reset_snapshot.py")] + CASES, env=_env(), capture_output=True,
                         text=True, timeout=1800)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert re.findall(r"CASE (\w+) OK", out.stdout) == CASES, out.stdout


_TRACE = r"""
import os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import test_gpu_reset_snapshot as t
from robopianist_amd import engine
L = engine.load_library()
si = t.hull_scene(True)
mask = np.zeros(8, np.uint8); mask[2] = 1
def masked(p, tag, capturing=False):
    os.environ["WAVESIM_CAPTURING"] = "1" if capturing else "0"
    os.environ["WAVESIM_DEVICE_PTRS"] = "1"
    L.wavesim_trace_begin(tag.encode())
    p.step_masked(1, None, mask)
    os.environ["WAVESIM_DEVICE_PTRS"] = "0"; os.environ["WAVESIM_CAPTURING"] = "0"
for on in (1, 0):
    for lazy in (1, 0):
        L.wavesim_trace_begin(b"create")
        p = engine.BatchedPhysics(si.model, si.key_joint_ids, n_envs=8)
        p.set_reset_snapshot(on); t.split_stage(p); p.set_lazy_position_stage(bool(lazy))
        L.wavesim_trace_begin(f"on={on} lazy={lazy} env-reset".encode())
        p.reset(None)   # (env.reset(): the whole batch -- with the switch on it builds the shadow and every hand-over is valid)
        masked(p, f"on={on} lazy={lazy} first")
        masked(p, f"on={on} lazy={lazy} steady")
        p.set_mpr_tolerance(1e-6, 1e-9)
        masked(p, f"on={on} lazy={lazy} stale-capturing", capturing=True)
        masked(p, f"on={on} lazy={lazy} rebuilt")
        p.set(engine.TREE_OFFSET, np.zeros((8, 2, 3)))
        masked(p, f"on={on} lazy={lazy} tree-offset")
L.wavesim_trace_begin(b"end")
"""


def test_what_the_engine_enqueues_with_and_without_the_snapshot(tmp_path):
    """Host behaviour only (kernels skipped).  With the switch on and the lazy mode on, a masked step in the steady
    state has no rp_lead_mask_kernel and no leading position launch; without the lazy mode the leading stage stays (it
    runs for every active env).  A stale snapshot is rebuilt by one reset + one one-wave stage launch in front of the
    reset -- except inside a capture, which takes the ordinary leading stage.  After rp_set(RP_TREE_OFFSET), and with the
    switch off, the launches are the ones the engine made before the snapshot existed."""
    raw = str(tmp_path / "trace.raw")
    script = str(tmp_path / "trace.py")
    with open(script, "w") as fh:
        fh.write(_TRACE)
    out = subprocess.run([sys.executable, script], env=_env(WAVESIM_TRACE=raw, WAVESIM_SKIP_KERNELS="1"), capture_output=True,
                         text=True, timeout=1800, cwd=os.path.dirname(HERE))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    calls = {}
    for sec in open(raw).read().split("## ")[1:]:
        head, *lines = sec.splitlines()
        calls[head] = [re.sub(r" s\d+$", "", l) for l in lines if l.startswith("launch ")]

    def shape(tag):
        ls = calls[tag]
        pos = [l for l in ls if re.match(r"launch rp_(pos_front|pos_back|narrow)_kernel", l)]
        return dict(build=sum("grid=1 " in l and ("rp_reset_kernel" in l or "rp_stage_kernel<double, 0" in l) for l in ls),
                    mask=sum("rp_lead_mask_kernel" in l for l in ls), pos=len(pos), resets=sum("rp_reset_kernel" in l for l in ls))

    lean = dict(build=0, mask=0, pos=3, resets=1)     # one substep: its own front / narrow / back and nothing in front
    full = dict(build=0, mask=1, pos=6, resets=1)     # ... with the leading stage
    assert shape("on=1 lazy=1 env-reset") == dict(build=2, mask=0, pos=0, resets=2)   # (a new engine has the switch off: built here)
    assert shape("on=0 lazy=1 env-reset") == dict(build=0, mask=0, pos=0, resets=1)
    assert shape("on=1 lazy=1 first") == lean
    assert shape("on=1 lazy=1 steady") == lean
    assert shape("on=1 lazy=1 stale-capturing") == full
    assert shape("on=1 lazy=1 rebuilt") == dict(full, build=2, resets=2)   # (a reset was recorded: the host no longer vouches for validity)
    assert shape("on=1 lazy=0 steady") == full
    for lazy in (0, 1):
        assert shape(f"on=1 lazy={lazy} tree-offset") == full
        for tag in ("first", "steady", "stale-capturing", "rebuilt", "tree-offset"):
            assert shape(f"on=0 lazy={lazy} {tag}") == full, (lazy, tag)
        # switch off: line for line what the same calls enqueue once tree offsets have turned the snapshot off
        assert calls[f"on=0 lazy={lazy} steady"] == calls[f"on=1 lazy={lazy} tree-offset"]
