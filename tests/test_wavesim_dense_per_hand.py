"""The lean solver stage's dense block per hand (tests/test_dense_block_per_hand.py) without a GPU: the same cases and
the RP_DENSE_HANDS switch test on the CPU wave emulator (tests/wavesim), which runs the engine's own kernel sources."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
WS = os.path.join(HERE, "wavesim")
CSRC = os.path.join(os.path.dirname(HERE), "robopianist_amd", "csrc")


def _emulator_build():
    """tests/wavesim/_build/librp_engine_wavesim.so, rebuilt when a source is newer (tests/test_wavesim.py builds the
    same file)."""
    lib = os.path.join(WS, "_build", "librp_engine_wavesim.so")
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))] + \
           [os.path.join(WS, f) for f in ("wavesim.cpp", "wavesim.hpp", "build.sh")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call([os.path.join(WS, "build.sh")], stdout=subprocess.DEVNULL)
    return lib


def test_dense_block_per_hand_on_the_wave_emulator():
    """Cases a .. e teacher-forced at 1e-9 with equal contact and Newton iteration counts, then RP_DENSE_HANDS = 1
    against 0 bit for bit and the default against 0 at 1e-12."""
    env = dict(os.environ, RP_ENGINE_LIB=_emulator_build(), WAVESIM_SITE="0", RP_SKIP_SELF_CHECK="1")
    env.pop("RP_DENSE_HANDS", None)
    out = subprocess.run([sys.executable, os.path.join(WS, "dense_per_hand.py"), "abcde", "switch"], env=env,
                         capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert sorted(re.findall(r"CASE (\w) OK", out.stdout)) == list("abcde"), out.stdout
    assert "SWITCH OK" in out.stdout, out.stdout
