// rp_schedule.hpp -- the schedule of an rp_step as a pure function: which of the four schedules, how many slices, the
// slice bounds and the grids that follow the lists of envs outside the light class.  Plain C++17, no HIP and no
// environment: rp_engine.hip's Engine<T>::step() calls rp_plan_step() once and then applies the vetoes that need the
// runtime (buffers, streams, events); tests/test_schedule_host.py compiles this file alone and checks it against a
// restatement of the table below.
#pragma once

static const int kRpMaxSlices = 4;   // rp_set_stream_slices: 1 .. 4 (EngineBase::kMaxSlices)

// What the rule reads.
struct RpStepInput {
  int nenv = 0;
  int mode = 0;                // 0 = rp_step, 1 = rp_forward (never sliced, never fused)
  int n_slices = 1;            // rp_set_stream_slices (0 = the engine chooses)
  int fused = 2;               // rp_set_fused_substeps: 0 = off, 1 = on, 2 = a candidate of the engine's choice
  bool fused_capable = false;  // rp_fused_capable(lean, deep, graph, fp64)
  int split_mode = 0;          // rp_set_split_position_stage: 0 = never, 1 = in every per-stage schedule, 2 = a candidate
  bool split_capable = false;  // the fp64 default-depth builds
  bool split_dropped = false;  // the split stage has overflowed its candidate / record lists once
  bool capturing = false;      // the caller is recording a hipGraph of its step
  bool lean = false, deep = false, graph = false;   // the kernel builds in use (Engine<T>)
  double heavy_est[kRpMaxSlices] = {8, 8, 8, 8};    // estimated length of each slice's list of envs outside the light class
  int last_nsl = 1;            // slices of the last rp_step
  bool many_heavy = false;     // those lists have been long lately (the rule's state: hysteresis)
};

struct RpStepPlan {
  int sched = 0;               // 1 .. 4 (the table below); 0 = the caller fixed the schedule
  int nsl = 1;                 // slices (stream and event creation may still fall back to 1)
  bool fused_now = false;
  bool split_wanted = false;   // the split position stage, before buffer allocation can veto it
  bool companion_now = true;   // full-capacity launches on companion streams (where the solver stage has two classes)
  bool many_heavy = false;     // the new state
};

// (no fused builds for scenes with graph hulls, for the deep builds or in single precision)
inline bool rp_fused_capable(bool lean, bool deep, bool graph, bool fp64) { return lean && !deep && !graph && fp64; }

// Batch sizes the rule turns on.
static const int kRpSliceMinEnvs = 1024;   // smaller batches are never sliced
static const int kRpFusedBelow = 3072;     // under this the fused schedule is the candidate, from it on the split one
static const int kRpNoSlicesFrom = 6144;   // three rounds of the chip's wave slots per launch: no slices
// List lengths (envs outside the light class per slice) `many_heavy` switches at: on at 4, off under 2.  kRpHeavyOn is
// also the length from which the heavy envs' position stage goes with their solver launch (rp_heavy_pos_alongside).
static const double kRpHeavyOn = 4.0, kRpHeavyOff = 2.0;

// true when the engine chooses the schedule of this call itself
inline bool rp_engine_chooses(const RpStepInput& in) {
  const bool fused_forced = in.fused == 1 && in.fused_capable && in.mode == 0;
  return in.n_slices == 0 && in.mode == 0 && !fused_forced;
}

inline RpStepPlan rp_plan_step(const RpStepInput& in) {
  RpStepPlan p;
  p.many_heavy = in.many_heavy;
  int want = in.n_slices;
  p.fused_now = in.fused == 1 && in.fused_capable && in.mode == 0;
  bool sched4 = false;
  if (rp_engine_chooses(in)) {
    // The schedule of an rp_step, chosen by RULE (round 6; rounds 3-5 ran timing trials of up to four candidates on
    // some steps of every 128 .. 1024: 1 % of a run, and a choice that differed from run to run).  All schedules give
    // bit-identical results (tests/test_gpu_parity.py), so the rule only has to be good, not exact:
    //   1 = one launch per stage        2 = the same as two slices on two streams, full-capacity launches on companion streams
    //   3 = fused substeps (one launch takes a light env through all substeps; the rest in a clean-up launch)
    //   4 = three slices, the position stage split (front part / pooled narrow phase / back part), no companion streams
    // Measured on MI355X: batches under 3072 envs fill at most one round and a half of the chip's 2048 wave
    // slots -- every launch boundary there is a tail, and the fused schedule (no boundaries) wins by 6-16 %; from 3072
    // envs on, three slices with the split stage win on the replay (lists of envs outside the light class short or
    // empty), two slices with companion streams when those lists are long (random policies: the full-capacity
    // launches then need the chip to themselves beside the lean ones); 6144 envs and more are three rounds per launch
    // and need no slices at all.  `many_heavy` follows the list lengths the device reports one step late (with
    // hysteresis), never a timer.
    double hl = 0;
    for (int i = 0; i < in.last_nsl && i < kRpMaxSlices; i++) hl = in.heavy_est[i] > hl ? in.heavy_est[i] : hl;   // (the slices the last step used: the others' estimates are stale)
    p.many_heavy = in.many_heavy ? hl >= kRpHeavyOff : hl >= kRpHeavyOn;
    const bool fused_ok = in.fused == 2 && in.fused_capable;
    // (the split stage keeps at most 256 candidates / 384 result records per env where the one-kernel stage never
    // overflows: once it has dropped any -- RP_WARN_SPLIT_FULL, counted on the device and read back with the list
    // lengths -- the rule stops choosing it for this engine: identical inputs must not give different physics
    // depending on the schedule.  ADVICE round 5.)
    const bool split_ok = in.split_mode == 2 && in.split_capable && !in.capturing && !in.split_dropped;
    if (in.capturing) p.sched = fused_ok ? 3 : 1;
    else if (in.nenv < kRpFusedBelow) p.sched = (fused_ok && !p.many_heavy) ? 3 : (in.nenv >= kRpSliceMinEnvs ? 2 : 1);   // (config 5, 2048 envs, long lists: fused 245 k, two slices 286 k)
    else if (split_ok && !p.many_heavy) p.sched = 4;
    else p.sched = in.nenv >= kRpNoSlicesFrom ? 1 : 2;
    p.fused_now = p.sched == 3;
    want = p.sched == 2 ? 2 : (p.sched == 4 ? 3 : 1);
    sched4 = p.sched == 4;
  }
  p.split_wanted = in.split_capable && in.mode == 0 && (in.split_mode == 1 || sched4);
  p.nsl = (in.mode == 0 && want > 1 && in.nenv >= kRpSliceMinEnvs && !in.capturing && !p.fused_now) ? (want >= 4 ? 4 : want) : 1;
  // (slices 2 / 3 run ON the companion streams of slices 0 / 1 -- pooled_stream: four hardware queues -- so with more
  // than two slices there are no companion streams, whoever asked for the slices: the full-capacity launch then goes in
  // front of the lean one on the slice's own stream.  ADVICE round 5: only the engine's own three-slice schedule turned
  // them off; a forced rp_set_stream_slices(e, 3 | 4) queued slice 2's whole chain behind slice 0's heavy solves.)
  p.companion_now = p.nsl <= 2;
  return p;
}

// rp_get_fused_substeps / rp_get_split_position_stage: 0 = off, 1 = in use, 2 = the rule may pick it.  `auto_mode` is
// the `sched` of the engine's last own choice outside a stream capture.
inline int rp_fused_report(const RpStepInput& in, int auto_mode) {
  return !in.fused_capable ? 0 : (in.fused == 1 ? 1 : (in.fused == 2 && in.n_slices == 0 ? (auto_mode == 3 ? 1 : 2) : 0));
}
// (... 2: batches of >= 3072 envs that have never overflowed its lists)
inline int rp_split_report(const RpStepInput& in, int auto_mode) {
  return in.split_mode == 1 ? 1 : (in.split_mode == 2 && in.n_slices == 0 && in.nenv >= kRpFusedBelow && !in.split_dropped ? (auto_mode == 4 ? 1 : 2) : 0);
}

// The heavy envs' position / velocity stage goes with their solver launch to the companion stream
// (the split pays when the list is long: config 3 446 -> 455 k; on a batch whose lists are empty the extra
// launch and the later join cost 1-4 %: config 2 657 -> 632 ... 651 k -- so it follows the same lagged estimate)
inline bool rp_heavy_pos_alongside(const RpStepInput& in, bool on_companion_stream, bool fp64, double est) {
  return on_companion_stream && !in.deep && !in.graph && fp64 && est >= kRpHeavyOn;
}

// ---- The reset snapshot (rp_model.hpp: RpSnapshot): the host's bookkeeping, as pure functions of this record.
// Engine<T> calls the rp_snapshot_on_* functions where the events happen and asks the two questions below.
struct RpSnapshotState {
  bool enabled = true;           // RP_RESET_SNAPSHOT / rp_set_reset_snapshot
  bool fresh = false;            // built, and nothing that could change what the position stage computes has been set since
  bool tree_offset_set = false;  // rp_set(RP_TREE_OFFSET) has been called: the reset state is no longer the same for every env -- off for good
  bool legacy_step = true;       // rp_set_legacy_step(0): the leading stage publishes the incoming state's outputs for all envs -- off
  // What the host knows of the device's stage_valid flags: true only while EVERY env's hand-over is known to match its
  // state (then a lazy rp_step needs no leading stage at all).  Conservative: false whenever the host cannot tell.
  bool all_valid = false;
  bool poisoned = false;         // a reset or a state write was recorded into a hipGraph: its replays change stage_valid unseen -- all_valid stays false
};
enum RpSnapshotUse { kRpSnapNone = 0, kRpSnapUse = 1, kRpSnapBuild = 2 };   // (Build: build it now, then use it)
// May the reset of this call copy the snapshot?  A stale snapshot is rebuilt, except inside a stream capture (the build
// is not part of the caller's graph): that call resets the ordinary way and its envs go through the leading stage.
inline RpSnapshotUse rp_snapshot_use(const RpSnapshotState& s, bool capturing) {
  if (!s.enabled || s.tree_offset_set || !s.legacy_step) return kRpSnapNone;
  if (s.fresh) return kRpSnapUse;
  return capturing ? kRpSnapNone : kRpSnapBuild;
}
// Does the device flag RpSnapshot::ok stand?  (Staleness is not in it: a stale snapshot is only kept from NEW resets.)
inline bool rp_snapshot_flag(const RpSnapshotState& s) { return s.enabled && !s.tree_offset_set && s.legacy_step; }
// ... a model-table upload or any option setter (tolerances, impratio, capacity classes, sensors, ...): err on the side of stale
inline void rp_snapshot_on_option(RpSnapshotState& s) { s.fresh = false; }
inline void rp_snapshot_on_built(RpSnapshotState& s) { s.fresh = true; }
// ... rp_set(RP_QPOS | RP_QVEL | RP_TREE_OFFSET): every stage_valid flag is cleared
inline void rp_snapshot_on_state_write(RpSnapshotState& s, bool tree_offset, bool capturing) {
  s.all_valid = false;
  if (tree_offset) s.tree_offset_set = true;
  if (capturing) s.poisoned = true;
}
// ... a reset: `used` = its envs got the snapshot (stage_valid 1), else their flags are cleared; `whole_batch` = no mask;
// `lead_follows` = rp_step_masked without the snapshot: the leading stage of the same call makes the envs valid again
inline void rp_snapshot_on_reset(RpSnapshotState& s, bool used, bool whole_batch, bool lead_follows, bool capturing) {
  if (capturing) { s.poisoned = true; s.all_valid = false; return; }
  if (used) s.all_valid = s.all_valid || whole_batch;
  else if (!lead_follows) s.all_valid = false;
}
// ... the end of an rp_step / rp_forward: it marks every env it touched valid; without an RP_ACTIVE mask that is all of them
inline void rp_snapshot_on_step_done(RpSnapshotState& s, bool active_mask, bool capturing) {
  if (!capturing && !active_mask && !s.poisoned) s.all_valid = true;
}
// May an rp_step leave out its leading position / velocity stage (mask kernel and every slice's launch)?  Only the lazy
// mode may (otherwise the stage runs for every active env), outside a capture (a graph must work for any later state),
// when no env can need it: all valid, and the envs this call resets got the snapshot.
inline bool rp_lead_skippable(const RpSnapshotState& s, int mode, bool lazy_now, bool capturing, bool has_reset, bool snap_used) {
  // (s.enabled: with the switch off the engine enqueues exactly what it did before the snapshot existed)
  return s.enabled && mode == 0 && lazy_now && !capturing && !s.poisoned && s.all_valid && (!has_reset || snap_used);
}

// slice sl of nsl covers the envs [bound(sl), bound(sl + 1)); bounds are multiples of 8 (XCD classes of the order)
inline int rp_slice_bound(int nenv, int nsl, int sl) { return sl >= nsl ? nenv : (int)(((long long)nenv * sl / nsl + 7) / 8 * 8); }

// Threads per residue class of rp_order_kernel: two envs per thread.  (A 512-thread workgroup needs a whole
// idle CU -- with both stage kernels at two waves per SIMD it waited ~60 us for one on every substep of a
// 2048-env slice -- while a single wave takes too long over 512 envs.  Measured: 2048-env slices 64 / 128 /
// 256 threads: 681 / 678 / 647 k env-steps/s; 4096-env slices 64 / 128 / 256 / 512: 540 / 547 / 561 / 562 k.)
inline int rp_order_threads_for(int cnt) {
  // (the kernel's scan needs a full first wave and its launch bound is 512: multiples of 64 in 64 .. 512)
  const int t = ((cnt / 16 + 63) / 64) * 64;
  return t < 64 ? 64 : (t > 512 ? 512 : t);
}

// The estimate of a slice's list length after the device has reported `seen` envs: up at once, down slowly.
inline double rp_heavy_est_update(double est, int seen) { return seen > est ? seen : 0.9 * est + 0.1 * seen; }

// Grid of the full-capacity solver stage over a slice of `cnt` envs, from the estimate of its list length.
inline int rp_heavy_grid(double est, int cnt, int max_grid) {
  // (config 3, 4096 envs: fixed grids of 24 / 48 / 128: 409 / 436 / 445 k env-steps/s.  Round 6: the floor is 2
  // workgroups, not 8 -- each needs a whole idle SIMD, and on the replay, whose lists are empty most of the time, a
  // grid of one measured +0.7 %: 636.6 against 632.2 k, two runs each inside one call)
  int g = (int)(2.0 * est) + 2;
  g = g < 2 ? 2 : (g > max_grid ? max_grid : g);
  return cnt < g ? cnt : g;
}
