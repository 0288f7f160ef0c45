"""TEST INFRASTRUCTURE: the reset snapshot (tests/test_gpu_reset_snapshot.py: switch on against switch off, bit for bit)
on the CPU wave emulator, which runs the engine's own kernel and host sources.
Usage: python tests/wavesim/reset_snapshot.py [case ...]     (default: every case)"""
import os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.chdir(ROOT)
os.environ.setdefault("RP_ENGINE_LIB", os.path.join(HERE, "_build", "librp_engine_wavesim.so"))
os.environ["RP_SKIP_SELF_CHECK"] = "1"
import numpy as np
import test_gpu_reset_snapshot as t
from robopianist_amd import engine

E, NSUB = 8, 3


def plan():
    def m(*envs):
        x = np.zeros(E, np.uint8)
        x[list(envs)] = 1
        return x
    # one env alone; two envs; the first and the last; the same env twice running; all at once; one in contact with a warn bit
    return {1: m(4), 2: m(1, 6), 3: m(0, 7), 4: m(3), 5: m(3), 6: np.ones(E, np.uint8), 8: "contact"}


def tree_offsets(p, step, which):
    if step == 2:
        off = np.zeros((E, 2, 3))
        off[:, :, 1] = 0.004 * (np.arange(E)[:, None] - 3)
        p.set(engine.TREE_OFFSET, off)


def options(p, step, which):
    if step == 3:
        p.set_mpr_tolerance(1e-6, 1e-10)


def legacy_off(p):
    t.one_kernel(p); p.set_legacy_step(False); p.set_lazy_position_stage(True)


CASES = {
    "one_kernel": dict(configure=t.one_kernel),
    "lazy_split_ordered": dict(configure=t.lazy_split_ordered),
    "fused_lazy": dict(configure=lambda p: (t.fused(p), p.set_lazy_position_stage(True))),
    "fp32": dict(precision=32, configure=lambda p: (p.set_stream_slices(1), p.set_fused_substeps(False), p.set_lazy_position_stage(True))),
    "tree_offset": dict(configure=t.lazy, between=tree_offsets, nsteps=5, need_contact=False),
    "options": dict(configure=t.lazy_split_ordered, between=options, nsteps=7, need_contact=False),
    "legacy_off": dict(configure=legacy_off, nsteps=7, need_contact=False),
}


def main():
    si = t.hull_scene()
    for name in sys.argv[1:] or list(CASES):
        kw = dict(nsteps=10, plan=plan(), nsub=NSUB)
        kw.update(CASES[name])
        t.run_pair(si, E, **kw)
        print(f"CASE {name} OK")


if __name__ == "__main__":
    main()
