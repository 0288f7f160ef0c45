"""The reset snapshot's bookkeeping (robopianist_amd/csrc/rp_schedule.hpp: RpSnapshotState and the rp_snapshot_* rules)
without a GPU: the header alone, compiled with g++ -- which calls make the snapshot stale, that a stale or disabled
snapshot is never used, that a capture with a stale snapshot takes the ordinary leading stage, and when an rp_step may
leave its leading stage out.  Plus the one list of what a reset copies (rp_model.hpp), against the hand-over buffers."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robopianist_amd", "csrc")

# The state travels as six ints (enabled, fresh, tree_offset_set, legacy_step, all_valid, poisoned), in and out.
_SRC = r"""
#include "rp_schedule.hpp"
static RpSnapshotState get(const int* s) {
  RpSnapshotState x;
  x.enabled = s[0]; x.fresh = s[1]; x.tree_offset_set = s[2]; x.legacy_step = s[3]; x.all_valid = s[4]; x.poisoned = s[5];
  return x;
}
static void put(const RpSnapshotState& x, int* s) {
  s[0] = x.enabled; s[1] = x.fresh; s[2] = x.tree_offset_set; s[3] = x.legacy_step; s[4] = x.all_valid; s[5] = x.poisoned;
}
extern "C" {
void ss_default(int* s) { put(RpSnapshotState(), s); }
int ss_use(const int* s, int capturing) { return rp_snapshot_use(get(s), capturing != 0); }
int ss_flag(const int* s) { return rp_snapshot_flag(get(s)); }
void ss_option(int* s) { RpSnapshotState x = get(s); rp_snapshot_on_option(x); put(x, s); }
void ss_built(int* s) { RpSnapshotState x = get(s); rp_snapshot_on_built(x); put(x, s); }
void ss_state_write(int* s, int tree, int capturing) { RpSnapshotState x = get(s); rp_snapshot_on_state_write(x, tree != 0, capturing != 0); put(x, s); }
void ss_reset(int* s, int used, int whole, int lead_follows, int capturing) {
  RpSnapshotState x = get(s); rp_snapshot_on_reset(x, used != 0, whole != 0, lead_follows != 0, capturing != 0); put(x, s);
}
void ss_step_done(int* s, int active_mask, int capturing) { RpSnapshotState x = get(s); rp_snapshot_on_step_done(x, active_mask != 0, capturing != 0); put(x, s); }
int ss_skippable(const int* s, int mode, int lazy_now, int capturing, int has_reset, int snap_used) {
  return rp_lead_skippable(get(s), mode, lazy_now != 0, capturing != 0, has_reset != 0, snap_used != 0);
}
}
"""

NONE, USE, BUILD = 0, 1, 2
F = ("enabled", "fresh", "tree_offset_set", "legacy_step", "all_valid", "poisoned")


class State:
    def __init__(self, L, **kw):
        self.L = L
        self.s = (ctypes.c_int * 6)()
        L.ss_default(self.s)
        for k, v in kw.items():
            self.s[F.index(k)] = int(v)

    def __getattr__(self, k):
        return bool(self.s[F.index(k)])

    def use(self, capturing=False):
        return self.L.ss_use(self.s, int(capturing))

    def reset(self, capturing=False, whole=False, lead_follows=False):
        """What Engine<T>::launch_reset does: ask, build if told to, report."""
        u = self.use(capturing)
        if u == BUILD:
            self.L.ss_built(self.s)
        self.L.ss_reset(self.s, int(u != NONE), int(whole), int(lead_follows), int(capturing))
        return u

    def skippable(self, mode=0, lazy=True, capturing=False, has_reset=False, used=False):
        return bool(self.L.ss_skippable(self.s, mode, int(lazy), int(capturing), int(has_reset), int(used)))


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    d = tmp_path_factory.mktemp("reset_snapshot_host")
    src, so = str(d / "snap.cpp"), str(d / "libsnap.so")
    with open(src, "w") as fh:
        fh.write(_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, src, "-o", so])
    return ctypes.CDLL(so)


def test_a_new_engine_builds_at_its_first_reset_and_uses_it_from_then_on(L):
    s = State(L)
    assert s.enabled and not s.fresh and not s.all_valid and s.legacy_step
    assert s.reset(whole=True) == BUILD and s.fresh and s.all_valid       # rp_create's rp_reset(NULL)
    assert s.reset() == USE and s.all_valid
    assert L.ss_flag(s.s) == 1


def test_every_option_call_makes_it_stale_and_a_stale_snapshot_is_never_used(L):
    s = State(L)
    s.reset(whole=True)
    L.ss_option(s.s)
    assert not s.fresh
    assert s.use(capturing=False) == BUILD          # rebuilt first: never copied as it is
    assert s.use(capturing=True) == NONE            # ... and inside a capture the ordinary leading stage runs
    assert L.ss_flag(s.s) == 1                      # (graphs recorded earlier keep the snapshot they were recorded with)
    assert s.reset(capturing=True, lead_follows=True) == NONE and s.poisoned and not s.all_valid
    assert s.reset() == BUILD and s.fresh


@pytest.mark.parametrize("off", ["enabled", "tree_offset_set", "legacy_step"])
def test_switch_tree_offsets_and_legacy_step_turn_it_off(L, off):
    s = State(L, fresh=True, all_valid=True, **{off: off == "tree_offset_set"})
    for cap in (False, True):
        assert s.use(cap) == NONE
    assert L.ss_flag(s.s) == 0
    assert s.reset() == NONE and not s.all_valid                 # its envs' hand-overs are stale now
    s2 = State(L, fresh=True, all_valid=True, **{off: off == "tree_offset_set"})
    assert s2.reset(lead_follows=True) == NONE and s2.all_valid  # rp_step_masked: the leading stage of the call repairs them


def test_state_writes(L):
    s = State(L, fresh=True, all_valid=True)
    L.ss_state_write(s.s, 0, 0)                                  # rp_set(RP_QPOS)
    assert not s.all_valid and not s.tree_offset_set and s.use() == USE
    L.ss_state_write(s.s, 1, 0)                                  # rp_set(RP_TREE_OFFSET): off for good
    assert s.tree_offset_set and s.use() == NONE
    L.ss_built(s.s); L.ss_option(s.s)
    assert s.use() == NONE
    s = State(L, fresh=True, all_valid=True)
    L.ss_state_write(s.s, 0, 1)                                  # recorded into a graph
    assert s.poisoned


def test_all_valid_is_only_ever_set_on_proof(L):
    s = State(L, fresh=True)
    assert s.reset(whole=False) == USE and not s.all_valid       # the other envs are unknown
    L.ss_step_done(s.s, 1, 0)
    assert not s.all_valid                                       # an RP_ACTIVE mask: only the active envs were marked
    L.ss_step_done(s.s, 0, 1)
    assert not s.all_valid                                       # a capture executes nothing
    L.ss_step_done(s.s, 0, 0)
    assert s.all_valid
    s = State(L, fresh=True, poisoned=True)
    L.ss_step_done(s.s, 0, 0); s.reset(whole=True)
    assert not s.skippable()                                     # replays of a recorded reset change validity unseen


def test_when_the_leading_stage_may_be_left_out(L):
    """The whole table: only rp_step (mode 0) in the lazy mode, outside a capture, with every hand-over known valid and the
    envs of this call's reset mask served by the snapshot; never with the switch off."""
    for bits in itertools.product((0, 1), repeat=6):
        for mode, lazy, cap, has_reset, used in itertools.product((0, 1), repeat=5):
            s = State(L, **dict(zip(F, bits)))
            want = (bits[0] and bits[4] and not bits[5] and mode == 0 and lazy and not cap and (not has_reset or used))
            assert s.skippable(mode, lazy, cap, has_reset, used) == bool(want), (bits, mode, lazy, cap, has_reset, used)


def test_the_rule_table_of_use(L):
    for bits in itertools.product((0, 1), repeat=6):
        for cap in (0, 1):
            s = State(L, **dict(zip(F, bits)))
            en, fresh, tree, legacy = bits[:4]
            want = NONE if (not en or tree or not legacy) else (USE if fresh else (NONE if cap else BUILD))
            assert s.use(cap) == want, (bits, cap)


def test_every_option_setter_of_the_abi_marks_the_snapshot_stale():
    """Each rp_set_* entry point of rp_engine.hip (the field write rp_set and rp_set_stream aside) reaches option_changed():
    a setter added later without it would leave resets copying what the stage no longer computes."""
    text = open(os.path.join(CSRC, "rp_engine.hip")).read()
    ext = text.split('extern "C" {')[1]
    bodies = {}
    for n in re.findall(r"^int (rp_set_[a-z_]+)\(rp_engine\* e", ext, flags=re.M):
        bodies[n] = re.split(r"^int |^const ", ext.split(f"int {n}(rp_engine* e")[1], flags=re.M)[0]
    setters = sorted(n for n in bodies if n not in ("rp_set_stream",))
    assert len(setters) >= 12, setters
    for n in setters:
        assert "option_changed()" in bodies[n] or "reset_snapshot(" in bodies[n], n
    assert "option_changed();" in text.split("int reset_snapshot(int on) override")[1].split("}")[0]


def test_the_copy_list_names_every_hand_over_buffer():
    """rp_model.hpp keeps ONE list of what a reset copies: every per-env buffer of RpStage up to the split stage's
    intermediates is on it, and the intermediates are not."""
    text = open(os.path.join(CSRC, "rp_model.hpp")).read()
    stage = text.split("struct RpStage {")[1].split("};")[0]
    handover, split = stage.split("// ---- split position stage")
    members = re.findall(r"^\s*(?:T|int)\*\s+(\w+);", handover, flags=re.M)
    listed = re.findall(r"X\((\w+),", text.split("#define RPK_SNAPSHOT_HANDOVER(X)")[1].split("//")[0])
    assert sorted(members) == sorted(listed) and len(members) == 10, (members, listed)
    for m in re.findall(r"^\s*(?:T|int)\*\s+(\w+);", split, flags=re.M):
        assert m not in listed
    outputs = re.findall(r"X\((\w+),", text.split("#define RPK_SNAPSHOT_OUTPUTS(X)")[1].split("__host__")[0])
    assert sorted(outputs) == sorted(["act_vel", "site_xpos", "contact_geoms", "contact_dist", "ncon", "cost_pos", "warn"])
