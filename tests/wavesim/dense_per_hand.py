"""TEST INFRASTRUCTURE: the cases of tests/test_dense_block_per_hand.py (the lean solver stage's dense block per hand)
on the CPU wave emulator, teacher-forced against the oracle, and the RP_DENSE_HANDS switch test.
Usage: python tests/wavesim/dense_per_hand.py [cases, default abcde] [switch]"""
import os, sys, warnings
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.chdir(ROOT)
os.environ.setdefault("RP_ENGINE_LIB", os.path.join(HERE, "_build", "librp_engine_wavesim.so"))
os.environ["RP_SKIP_SELF_CHECK"] = "1"
import test_dense_block_per_hand as t
from robopianist_amd.model import scene

def main():
    cases = sys.argv[1] if len(sys.argv) > 1 else "abcde"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        si = scene.build_scene(gravity_compensation=True, primitive_fingertip_collisions=True)
    for name in cases:
        n, worst = t.check_case(si, name)
        print(f"CASE {name} OK: {n} states, worst rel dv {worst:.2e}")
    if "switch" in sys.argv[2:]:
        print(f"SWITCH OK: default vs joint block {t.check_switch(si):.2e} relative")

if __name__ == "__main__":
    main()
