"""The schedule rule of rp_step (robopianist_amd/csrc/rp_schedule.hpp) without a GPU: the header alone, compiled with g++,
against a Python restatement of the rule written from the table in its comment; the slice bounds; the grid arithmetic; and
the same program under the address and undefined-behaviour sanitizers, as an executable of its own."""

import ctypes
import itertools
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robopianist_amd", "csrc")

# One C entry point per function of the header (flat arguments: no struct layout to keep in step), and a main() that walks
# the same grids for the sanitizer build.
_SRC = r"""
#include "rp_schedule.hpp"
#include <cstdio>
static RpStepInput input(int nenv, int mode, int n_slices, int fused, int fused_capable, int split_mode, int split_capable,
                         int split_dropped, int capturing, const double* est, int last_nsl, int many_heavy) {
  RpStepInput in;
  in.nenv = nenv; in.mode = mode; in.n_slices = n_slices; in.fused = fused; in.fused_capable = fused_capable != 0;
  in.split_mode = split_mode; in.split_capable = split_capable != 0; in.split_dropped = split_dropped != 0;
  in.capturing = capturing != 0; in.lean = in.fused_capable; in.deep = !in.split_capable; in.graph = false;
  for (int i = 0; i < kRpMaxSlices; i++) in.heavy_est[i] = est[i];
  in.last_nsl = last_nsl; in.many_heavy = many_heavy != 0;
  return in;
}
extern "C" {
// out: sched, nsl, fused_now, split_wanted, companion_now, many_heavy, fused report, split report (for auto_mode = sched, or
// the given one where the caller fixed the schedule)
void sh_plan(int nenv, int mode, int n_slices, int fused, int fused_capable, int split_mode, int split_capable, int split_dropped,
             int capturing, const double* est, int last_nsl, int many_heavy, int auto_mode, int* out) {
  const RpStepInput in = input(nenv, mode, n_slices, fused, fused_capable, split_mode, split_capable, split_dropped, capturing, est, last_nsl, many_heavy);
  const RpStepPlan p = rp_plan_step(in);
  out[0] = p.sched; out[1] = p.nsl; out[2] = p.fused_now; out[3] = p.split_wanted; out[4] = p.companion_now; out[5] = p.many_heavy;
  const int am = p.sched && !capturing ? p.sched : auto_mode;
  out[6] = rp_fused_report(in, am); out[7] = rp_split_report(in, am);
}
int sh_fused_capable(int lean, int deep, int graph, int fp64) { return rp_fused_capable(lean, deep, graph, fp64); }
int sh_slice_bound(int nenv, int nsl, int sl) { return rp_slice_bound(nenv, nsl, sl); }
int sh_order_threads(int cnt) { return rp_order_threads_for(cnt); }
int sh_heavy_grid(double est, int cnt, int max_grid) { return rp_heavy_grid(est, cnt, max_grid); }
double sh_heavy_est_update(double est, int seen) { return rp_heavy_est_update(est, seen); }
int sh_heavy_pos_alongside(int deep, int graph, int companion, int fp64, double est) {
  RpStepInput in; in.deep = deep != 0; in.graph = graph != 0;
  return rp_heavy_pos_alongside(in, companion != 0, fp64 != 0, est);
}
}
#ifdef SH_MAIN
int main() {
  long n = 0, acc = 0;
  const int envs[] = {8, 1023, 1024, 3071, 3072, 6143, 6144, 16384, 65540};
  const double ests[] = {0, 1.9, 2.0, 3.9, 4.0, 40};
  int out[8];
  for (int nenv : envs) for (int bits = 0; bits < 1024; bits++) for (double e : ests) for (int ns = 0; ns <= 4; ns++)
    for (int fused = 0; fused <= 2; fused++) for (int sm = 0; sm <= 2; sm++) for (int last = 1; last <= 4; last++) {
      double est[kRpMaxSlices] = {0, 0, 0, 0};
      est[last - 1] = e;
      sh_plan(nenv, bits & 1, ns, fused, (bits >> 1) & 1, sm, (bits >> 2) & 1, (bits >> 3) & 1, (bits >> 4) & 1, est, last, (bits >> 5) & 1, 1 + ((bits >> 6) & 3), out);
      for (int sl = 0; sl <= out[1]; sl++) acc += sh_slice_bound(nenv, out[1], sl);
      acc += out[0] + sh_order_threads(nenv) + sh_heavy_grid(e, nenv, 128) + sh_heavy_grid(e, nenv, 1);
      n++;
    }
  printf("walked %ld plans (checksum %ld)\n", n, acc);
  return 0;
}
#endif
"""

ENVS = (8, 1023, 1024, 3071, 3072, 6143, 6144, 16384)
ESTS = (0.0, 1.9, 2.0, 3.9, 4.0, 40.0)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("schedule_host")
    src, so = str(d / "schedule_host.cpp"), str(d / "libschedule_host.so")
    with open(src, "w") as fh:
        fh.write(_SRC)
    # (-Wall -Werror: the header is plain C++17 and compiles alone, without HIP)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, src, "-o", so])
    L = ctypes.CDLL(so)
    L.sh_plan.argtypes = [ctypes.c_int] * 9 + [ctypes.POINTER(ctypes.c_double)] + [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)]
    L.sh_heavy_grid.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_int]
    L.sh_heavy_est_update.argtypes = [ctypes.c_double, ctypes.c_int]
    L.sh_heavy_est_update.restype = ctypes.c_double
    L.sh_heavy_pos_alongside.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double]
    return L


def test_the_header_includes_nothing_and_reads_no_environment():
    text = open(os.path.join(CSRC, "rp_schedule.hpp")).read()
    assert "#include" not in text and "getenv" not in text


# ---- the twin: the rule as its comment table states it -------------------------------------------------------------------
def twin(nenv, mode, n_slices, fused, fused_capable, split_mode, split_capable, split_dropped, capturing, est, last_nsl,
         many_heavy, auto_mode):
    """Returns (sched, nsl, fused_now, split_wanted, companion_now, many_heavy, fused report, split report)."""
    step = mode == 0
    forced_fused = fused == 1 and fused_capable and step
    sched = 0
    if n_slices == 0 and step and not forced_fused:   # the engine chooses
        longest = max(est[:last_nsl])                 # (only the slices the last step used)
        many_heavy = longest >= (2.0 if many_heavy else 4.0)
        fused_ok = fused == 2 and fused_capable
        split_ok = split_mode == 2 and split_capable and not capturing and not split_dropped
        if capturing:                                 # a graph is being recorded: no streams, no allocation
            sched = 3 if fused_ok else 1
        elif nenv < 3072:                             # under one round and a half of the chip: fused, unless the lists are long
            sched = 3 if fused_ok and not many_heavy else (2 if nenv >= 1024 else 1)
        elif split_ok and not many_heavy:             # three slices with the split stage
            sched = 4
        else:                                         # two slices with companion streams; none from three rounds on
            sched = 1 if nenv >= 6144 else 2
        fused_now = sched == 3
        want = {1: 1, 2: 2, 3: 1, 4: 3}[sched]
    else:
        fused_now = forced_fused
        want = n_slices
    split_wanted = split_capable and step and (split_mode == 1 or sched == 4)
    nsl = min(want, 4) if (step and want > 1 and nenv >= 1024 and not capturing and not fused_now) else 1
    if sched and not capturing:
        auto_mode = sched
    fused_report = 0 if not fused_capable else (1 if fused == 1 else ((1 if auto_mode == 3 else 2) if fused == 2 and n_slices == 0 else 0))
    split_report = 1 if split_mode == 1 else (
        (1 if auto_mode == 4 else 2) if split_mode == 2 and n_slices == 0 and nenv >= 3072 and not split_dropped else 0)
    return (sched, nsl, int(fused_now), int(split_wanted), int(nsl <= 2), int(many_heavy), fused_report, split_report)


def _plan(L, *a):
    est = (ctypes.c_double * 4)(*a[9])
    out = (ctypes.c_int * 8)()
    L.sh_plan(*a[:9], est, *a[10:], out)
    return tuple(out)


def test_the_plan_equals_the_restatement_on_the_whole_grid(lib):
    """Every batch size at the rule's edges x every setting of the other inputs x list estimates on both sides of the two
    hysteresis thresholds, with both previous many_heavy states; the estimate sits in the last slice the previous step used
    (and in a slice it did not use, which the rule must ignore)."""
    n = 0
    seen = set()
    flags = list(itertools.product((0, 1), repeat=5))   # fused_capable, split_capable, split_dropped, capturing, many_heavy
    for nenv, mode, n_slices, fused, split_mode in itertools.product(ENVS, (0, 1), (0, 1, 2, 3, 4), (0, 1, 2), (0, 1, 2)):
        for (fc, sc, sd, cap, mh), e, last in itertools.product(flags, ESTS, (1, 3)):
            for stale in (0.0, 40.0):
                est = [stale] * 4
                est[last - 1] = e
                for k in range(last - 1):
                    est[k] = min(e, 1.0)
                args = (nenv, mode, n_slices, fused, fc, split_mode, sc, sd, cap, est, last, mh, 1 + (n % 4))
                got, want = _plan(lib, *args), twin(*args)
                assert got == want, (args, got, want)
                seen.add(got[0])
                n += 1
    assert seen == {0, 1, 2, 3, 4} and n > 500_000


def test_hysteresis_switches_on_at_four_and_off_under_two(lib):
    base = (4096, 0, 0, 2, 1, 2, 1, 0, 0)
    on = [bool(_plan(lib, *base, [e] * 4, 2, mh, 1)[5]) for mh in (0, 1) for e in ESTS]
    assert on == [False, False, False, False, True, True] + [False, False, True, True, True, True]
    # ... and the schedule follows: long lists take two slices with companion streams, short ones three with the split stage
    assert [_plan(lib, *base, [e] * 4, 2, 0, 1)[0] for e in (3.9, 4.0)] == [4, 2]


def test_fused_capable(lib):
    for lean, deep, graph, fp64 in itertools.product((0, 1), repeat=4):
        assert lib.sh_fused_capable(lean, deep, graph, fp64) == int(lean and not deep and not graph and fp64)


def test_heavy_position_stage_goes_alongside_from_four(lib):
    for deep, graph, comp, fp64 in itertools.product((0, 1), repeat=4):
        for e in ESTS:
            assert lib.sh_heavy_pos_alongside(deep, graph, comp, fp64, e) == int(comp and not deep and not graph and fp64 and e >= 4.0)


# ---- slice bounds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nenv", (1024, 1025, 4095, 4096, 65540))
def test_slice_bounds_are_multiples_of_eight_and_cover_every_env_once(lib, nenv):
    for nsl in (1, 2, 3, 4):
        b = [lib.sh_slice_bound(nenv, nsl, sl) for sl in range(nsl + 1)]
        assert b[0] == 0 and b[-1] == nenv and b == sorted(b), b
        assert all(x % 8 == 0 for x in b[:-1]), b
        assert all(hi > lo for lo, hi in zip(b, b[1:])), b          # no empty slice
        assert sum(hi - lo for lo, hi in zip(b, b[1:])) == nenv      # adjacent ranges: every env exactly once
        assert lib.sh_slice_bound(nenv, nsl, nsl + 1) == nenv


# ---- grid arithmetic ------------------------------------------------------------------------------------------------------
def test_order_threads_are_multiples_of_64_in_64_to_512(lib):
    got = {cnt: lib.sh_order_threads(cnt) for cnt in list(range(0, 9000)) + [16384, 65540, 2 ** 31 - 1]}
    assert all(t % 64 == 0 and 64 <= t <= 512 for t in got.values())
    assert got[8] == 64 and got[1039] == 64 and got[1040] == 128 and got[2048] == 128 and got[4096] == 256 and got[8192] == 512
    assert all(got[c] <= got[c + 1] for c in range(0, 8999))
    # two envs per thread over the eight residue classes, while the launch bound allows
    assert all(8 * t * 2 >= cnt - 15 for cnt, t in got.items() if cnt <= 8192)


def test_heavy_grid_has_floor_two_and_the_cap(lib):
    for cap in (2, 16, 128):   # (kHeavyGrid: 128, or what RP_HEAVY_GRID pins -- then the grid is not computed at all)
        for cnt in (1, 2, 3, 100, 4096):
            for e in (-1.0, 0.0, 0.4, 0.5, 1.9, 8.0, 62.9, 63.0, 1e6):
                want = min(cnt, max(2, min(cap, int(2.0 * e) + 2)))
                assert lib.sh_heavy_grid(e, cnt, cap) == want, (e, cnt, cap)
    assert lib.sh_heavy_grid(0.0, 4096, 128) == 2 and lib.sh_heavy_grid(8.0, 4096, 128) == 18
    assert lib.sh_heavy_grid(62.9, 4096, 128) == 127 and lib.sh_heavy_grid(63.0, 4096, 128) == 128 and lib.sh_heavy_grid(1e6, 4096, 128) == 128
    assert lib.sh_heavy_grid(8.0, 5, 128) == 5 and lib.sh_heavy_grid(0.0, 1, 128) == 1


def test_heavy_estimate_rises_at_once_and_decays_by_a_tenth(lib):
    assert lib.sh_heavy_est_update(8.0, 20) == 20.0
    assert lib.sh_heavy_est_update(8.0, 0) == pytest.approx(7.2, abs=1e-12)
    assert lib.sh_heavy_est_update(8.0, 8) == pytest.approx(8.0, abs=1e-12)
    e, steps = 8.0, 0
    while e >= 2.0:
        e, steps = lib.sh_heavy_est_update(e, 0), steps + 1
    assert steps == 14   # (what tests/wavesim/launch_trace.py's automatic cases wait for)


# ---- the sanitizers, in a program of its own ---------------------------------------------------------------------------
def test_the_rule_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same entry points over the same grids (and 65540 envs) in a stand-alone program.  Nothing sanitised is loaded
    into this process."""
    src, exe = str(tmp_path / "schedule_sanitize.cpp"), str(tmp_path / "schedule_sanitize")
    with open(src, "w") as fh:
        fh.write(_SRC)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DSH_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("this g++ cannot link -fsanitize=address,undefined: " + (r.stdout + r.stderr).strip().splitlines()[-1])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "walked" in r.stdout and "runtime error" not in r.stderr
