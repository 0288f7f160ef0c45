// rp_engine.hip — host side of the C ABI declared in include/rp_engine.h.
// Parses the model blob (robopianist_amd/model/compile.py:to_blob + engine
// tables), uploads the fixed-topology tables, owns the env-major state arrays and
// launches the stage kernels (rp_kernels.hpp; their bodies: rp_position_body there, rp_lean_solver_body in rp_solver2.hpp,
// rp_full_solver_body in rp_solver_full.hpp) on the engine's HIP stream.
#include "rp_kernels.hpp"
#include "rp_schedule.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rp_engine.h"

namespace {

// Bookkeeping of the lazy position stage (rp_set_lazy_position_stage): which envs' hand-over
// (RpStage) still matches their state.
// (lazy: skip the envs whose hand-over is still the one of their state; also: the envs rp_step_masked has just
// reset, stepped or not -- their position / velocity stage is the physics.forward() of the new episode;
// also_lazy: ... unless the reset gave them the snapshot's hand-over and outputs, which it tells by valid[e])
__global__ void rp_lead_mask_kernel(int* lead, const int* active, const unsigned char* valid, int lazy, const unsigned char* also, int also_lazy, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) lead[e] = (((active ? active[e] != 0 : true) && !(lazy && valid[e])) || (also && also[e] && !(also_lazy && valid[e]))) ? 1 : 0;
}
__global__ void rp_mark_valid_kernel(unsigned char* valid, const int* active, const unsigned char* also, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n && (!active || active[e] != 0 || (also && also[e]))) valid[e] = 1;
}

// Launch order of the envs for the solver stage that follows a position stage: descending predicted
// cost (counting sort on a small integer key), one workgroup per residue class.  With one wave per env
// and every SIMD running its envs one after the other, a heavy env that starts late is the tail of
// the whole launch; the hardware dispatches workgroups in index order to whichever slot frees up, so
// sorting the heaviest first is longest-processing-time-first list scheduling.
//   * predictor: the structure of the system the solver is about to solve, read from the hand-over
//     the position stage just wrote -- contacts, touched keys, rows of the dense (cross-chain) block --
//     with a typical Newton iteration count.  Measured (profiles/r02_cost_order.md): the per-env solver
//     time is 26 k + it * (30 k + 1.2 k nd + 5 nd^2 + 2 k nk) + 2.7 k ncon cycles (R^2 0.99), and the
//     iteration count of the next solve is nearly unpredictable from the last ones (correlation 0.37),
//     so a constant does better than the previous count.
//   * XCD affinity: workgroup b runs on XCD b mod 8, and an env's state / hand-over should stay in
//     that XCD's L2, so the sort is done within each residue class: order[8 r + x] = the r-th
//     heaviest env among those with index = x (mod 8).  Inactive envs go last in their class.
#define RP_ORDER_BUCKETS 256
#define RP_ORDER_CLASSES 8
__global__ __launch_bounds__(512) void rp_order_kernel(int* order_all, const int* hdr, const int* active, int base, int n,
                                                       int* heavy_list, int* heavy_cnt, unsigned char* listed) {
  // (sorts the envs base .. base + n - 1 into order_all[base .. base + n - 1]; base is a multiple of 8.
  // One workgroup per residue class: eight short kernels side by side instead of one 1024-thread block.)
  const int x = blockIdx.x;
  // the envs outside the light capacity class, compacted for the full-capacity solver stage (any order: envs
  // are independent); the counter is cleared by that stage's last workgroup
  if (heavy_list) {
    for (int e = x + RP_ORDER_CLASSES * (int)threadIdx.x; e < n; e += RP_ORDER_CLASSES * blockDim.x) {
      const bool on = hdr[(base + e) * rpk::HDR_N + rpk::HDR_CLASS] != 1 && !(active && active[base + e] == 0);
      if (on) heavy_list[base + atomicAdd(heavy_cnt, 1)] = base + e;
      if (listed) listed[base + e] = on ? 1 : 0;   // (the snapshot the split position launches test: RpState::listed)
    }
  }
  if (!order_all) return;
  int* order = order_all + base;
  __shared__ int hist[RP_ORDER_BUCKETS];
  for (int i = threadIdx.x; i < RP_ORDER_BUCKETS; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  auto key_of = [&](int e) -> int {
    if (active && active[e] == 0) return 0;
    const int nc = hdr[e * rpk::HDR_N + rpk::HDR_NCON], nk = hdr[e * rpk::HDR_N + rpk::HDR_NKT];
    const int nd = __popc((unsigned)hdr[e * rpk::HDR_N + rpk::HDR_DIRTY_LO]) + __popc((unsigned)hdr[e * rpk::HDR_N + rpk::HDR_DIRTY_HI]);
    if (nc < 0 || nk < 0) return 1;   // (hand-over not written yet)
    // k cycles / 4, five Newton iterations
    const int k = 1 + (26 + 5 * (30 + nd + (nd >> 2) + nd * nd / 200 + 2 * nk) + 3 * nc) / 4;
    return k < RP_ORDER_BUCKETS ? k : RP_ORDER_BUCKETS - 1;
  };
  // (a thread's first env keeps its key in a register between the two passes)
  const int e_first = x + RP_ORDER_CLASSES * (int)threadIdx.x;
  const int k_first = e_first < n ? key_of(base + e_first) : 0;
  for (int e = e_first; e < n; e += RP_ORDER_CLASSES * blockDim.x) atomicAdd(&hist[e == e_first ? k_first : key_of(base + e)], 1);
  __syncthreads();
  // descending exclusive prefix: lane l of the first wave owns the four buckets 255 - 4 l ... 252 - 4 l
  static_assert(RP_ORDER_BUCKETS == 256, "scan layout");
  if (threadIdx.x < 64) {
    const int l = threadIdx.x;
    int v[4], tot = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = hist[RP_ORDER_BUCKETS - 1 - 4 * l - k]; tot += v[k]; }
    int incl = tot;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d, 64); if (l >= d) incl += t; }
    int acc = incl - tot;
#pragma unroll
    for (int k = 0; k < 4; k++) { hist[RP_ORDER_BUCKETS - 1 - 4 * l - k] = acc; acc += v[k]; }
  }
  __syncthreads();
  for (int e = e_first; e < n; e += RP_ORDER_CLASSES * blockDim.x) {
    const int r = atomicAdd(&hist[e == e_first ? k_first : key_of(base + e)], 1);
    order[RP_ORDER_CLASSES * r + x] = base + e;
  }
}

thread_local std::string g_err;
int fail(const std::string& s) { g_err = s; return -1; }
#define HIP_OK(x)                                                                  \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess)                                                          \
      return fail(std::string(#x) + ": " + hipGetErrorString(e_));                 \
  } while (0)

#define RP_TRY(x)                                                                  \
  do {                                                                             \
    if (int r_ = (x)) return r_;                                                   \
  } while (0)

// true when `p` is device memory (a host pointer the runtime has never seen leaves an error behind: cleared)
bool is_device_ptr(const void* p) {
  hipPointerAttribute_t attr;
  const bool on_device = hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice;
  (void)hipGetLastError();
  return on_device;
}

// Which builds of the stage kernels an engine launches: fixed by the model (Engine<T>::build).  Every launch_* helper
// below dispatches over exactly the instantiations its kernel has -- a new build is added in ONE of them.
struct StageVariant {
  int hull = 0;         // the MESH template argument: 0 = primitives only, 1 = convex hulls (MPR), 2 = hulls with a vertex graph / cylinders
  bool deep = false;    // the RPK_MAXD_DEEP builds
  bool trunk4 = false;  // the solver builds specialised for "every tree has a 4-link trunk"
};

// rp_stage_kernel<T, MODE>: MODE 0 = position / velocity stage and MODE 2 = sensor stage (tree depth x hull support),
// MODE 1 = solver stage (deep, 4-link trunk or general)
template <typename T, int MODE>
inline void launch_stage(const StageVariant& v, int grid, hipStream_t st, const RpModel<T>& M, const RpState<T>& s, const RpStage<T>& B, int k, int nsub) {
#define RP_STAGE(...) hipLaunchKernelGGL((rp_stage_kernel<T, MODE, __VA_ARGS__>), dim3(grid), dim3(64), 0, st, M, s, B, k, nsub)
  if constexpr (MODE == 1) {
    if (v.deep) RP_STAGE(0, RPK_MAXD_DEEP);
    else if (v.trunk4) RP_STAGE(4);
    else RP_STAGE(0);
  } else {
    switch ((v.deep ? 3 : 0) + v.hull) {
      case 5: RP_STAGE(0, RPK_MAXD_DEEP, 2); break;
      case 4: RP_STAGE(0, RPK_MAXD_DEEP, 1); break;
      case 3: RP_STAGE(0, RPK_MAXD_DEEP); break;
      case 2: RP_STAGE(0, RPK_MAXD, 2); break;
      case 1: RP_STAGE(0, RPK_MAXD, 1); break;
      default: RP_STAGE(0); break;
    }
  }
#undef RP_STAGE
}
// the position / velocity stage as front part, pooled narrow phase (`ng` workgroups), back part: the fp64 default-depth builds
template <typename T, int MESH>
inline void launch_pos_split_as(int grid, int ng, hipStream_t st, const RpModel<T>& M, const RpState<T>& s, const RpStage<T>& Bs, int k, int nsub) {
  hipLaunchKernelGGL((rp_pos_front_kernel<T, MESH>), dim3(grid), dim3(64), 0, st, M, s, Bs, k, nsub);
  hipLaunchKernelGGL((rp_narrow_kernel<T, MESH>), dim3(ng), dim3(64), 0, st, M, s, Bs);
  hipLaunchKernelGGL((rp_pos_back_kernel<T, MESH>), dim3(grid), dim3(64), 0, st, M, s, Bs, k, nsub);
}
template <typename T>
inline void launch_pos_split(const StageVariant& v, int grid, int ng, hipStream_t st, const RpModel<T>& M, const RpState<T>& s, const RpStage<T>& Bs, int k, int nsub) {
  if constexpr (sizeof(T) == 8) {
    if (v.hull == 2) launch_pos_split_as<T, 2>(grid, ng, st, M, s, Bs, k, nsub);
    else if (v.hull == 1) launch_pos_split_as<T, 1>(grid, ng, st, M, s, Bs, k, nsub);
    else launch_pos_split_as<T, 0>(grid, ng, st, M, s, Bs, k, nsub);
  }
}
// the position / velocity stage of the envs on the list (of those outside the light class), in list order
template <typename T>
inline void launch_pos_listed(const StageVariant& v, int grid, hipStream_t st, const RpModel<T>& M, const RpState<T>& s, const RpStage<T>& B, int k, int nsub) {
  if constexpr (sizeof(T) == 8) {   // (the light class exists in the fp64 default builds only)
    if (v.hull) hipLaunchKernelGGL((rp_pos_list_kernel<T, 1>), dim3(grid), dim3(64), 0, st, M, s, B, k, nsub);
    else hipLaunchKernelGGL((rp_pos_list_kernel<T, 0>), dim3(grid), dim3(64), 0, st, M, s, B, k, nsub);
  }
}
// fused substeps: the light envs' launch (SPLIT: with the split stage's bodies, else the one-kernel body), then the clean-up
// launch over the list (fp64, default depth, no graph hulls)
template <typename T, int MESH, bool SPLIT>
inline void launch_fused_as(bool trunk4, int grid, int cgrid, hipStream_t st, const RpModel<T>& M, const RpState<T>& sf, const RpStage<T>& Bfused,
                            const RpStage<T>& B, int nsub) {
  if constexpr (SPLIT) hipLaunchKernelGGL((rp_fused_split_kernel<T, MESH>), dim3(grid), dim3(64), 0, st, M, sf, Bfused, nsub);
  else hipLaunchKernelGGL((rp_fused_steps_kernel<T, MESH>), dim3(grid), dim3(64), 0, st, M, sf, Bfused, nsub);
  if (trunk4) hipLaunchKernelGGL((rp_cleanup_steps_kernel<T, MESH, 4>), dim3(cgrid), dim3(64), 0, st, M, sf, B, nsub);
  else hipLaunchKernelGGL((rp_cleanup_steps_kernel<T, MESH, 0>), dim3(cgrid), dim3(64), 0, st, M, sf, B, nsub);
}
template <typename T>
inline void launch_fused(const StageVariant& v, bool fsplit, int grid, int cgrid, hipStream_t st, const RpModel<T>& M, const RpState<T>& sf,
                         const RpStage<T>& Bfused, const RpStage<T>& B, int nsub) {
  if constexpr (sizeof(T) == 8) {
    if (fsplit && v.hull) launch_fused_as<T, 1, true>(v.trunk4, grid, cgrid, st, M, sf, Bfused, B, nsub);
    else if (fsplit) launch_fused_as<T, 0, true>(v.trunk4, grid, cgrid, st, M, sf, Bfused, B, nsub);
    else if (v.hull) launch_fused_as<T, 1, false>(v.trunk4, grid, cgrid, st, M, sf, Bfused, B, nsub);
    else launch_fused_as<T, 0, false>(v.trunk4, grid, cgrid, st, M, sf, Bfused, B, nsub);
  }
}

struct BlobEntry { char name[40]; int32_t dtype, ndim; int64_t count, offset; };

struct Blob {
  std::vector<unsigned char> data;
  int n = 0;
  const BlobEntry* ent = nullptr;
  bool init(const void* p, size_t nb) {
    data.assign((const unsigned char*)p, (const unsigned char*)p + nb);
    if (nb < 12) return false;
    const uint32_t* h = (const uint32_t*)data.data();
    if (h[0] != 0x52504D42u) return false;
    n = (int)h[2];
    ent = (const BlobEntry*)(data.data() + 12);
    return true;
  }
  const BlobEntry* find(const char* name) const {
    for (int i = 0; i < n; i++) if (!strncmp(ent[i].name, name, 40)) return &ent[i];
    return nullptr;
  }
  bool has(const char* name) const { return find(name) != nullptr; }
  std::vector<double> f(const char* name) const {
    const BlobEntry* e = find(name);
    if (!e) throw std::string("blob entry missing: ") + name;
    std::vector<double> v((size_t)e->count);
    if (e->dtype == 0) memcpy(v.data(), data.data() + e->offset, sizeof(double) * e->count);
    else { const int32_t* s = (const int32_t*)(data.data() + e->offset); for (int64_t i = 0; i < e->count; i++) v[i] = s[i]; }
    return v;
  }
  std::vector<int> i(const char* name) const {
    const BlobEntry* e = find(name);
    if (!e) throw std::string("blob entry missing: ") + name;
    if (e->dtype != 1) throw std::string("blob entry not int: ") + name;
    std::vector<int> v((size_t)e->count);
    memcpy(v.data(), data.data() + e->offset, sizeof(int32_t) * e->count);
    return v;
  }
  int i1(const char* name) const { return i(name).at(0); }
  double f1(const char* name) const { return f(name).at(0); }
};

// The internal streams (slices 1.., companion streams) are PROCESS-WIDE, one set per device, shared by every engine and
// never destroyed.  HIP maps a stream to one of the device's hardware queues (four) when it is created; streams that
// share a queue serialise.  With a set of streams per ENGINE, the second engine of a process -- bench.py's auxiliary
// legs, a training script's evaluation env -- got streams that shared queues with each other: its two- and three-slice
// schedules measured 7.2-9.1 ms per step where the first engine's took 5.9-6.1 (round 5).  Engines that share streams
// only order their launches among each other, which independent engines never relied on.
struct StreamPool {
  static const int kSlots = 8;   // [0 .. 3] slice streams (slot 0 unused), [4 .. 7] companion streams
  hipStream_t s[kSlots] = {};
};
static std::mutex g_pool_mutex;
static std::map<int, StreamPool> g_pools;
static hipStream_t pooled_stream(int device, int slot, bool high_priority) {
  // Four hardware queues, one of them the caller's stream: the schedules the engine picks from use {caller, slice 1,
  // companion 0, companion 1} (two slices) or {caller, slice 1, slice 2} (three slices, no companions) -- never both
  // sets at once.  Slice 2 therefore IS companion 0's stream and slice 3 companion 1's: four streams in all, so that the
  // five a process would otherwise own after the schedule trials do not share a queue.
  if (slot == 2) slot = 4;
  if (slot == 3) slot = 5;
  std::lock_guard<std::mutex> lock(g_pool_mutex);
  StreamPool& p = g_pools[device];
  if (!p.s[slot]) {
    int least = 0, greatest = 0;
    hipError_t e;
    if (high_priority && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least)
      e = hipStreamCreateWithPriority(&p.s[slot], hipStreamNonBlocking, greatest);
    else { (void)hipGetLastError(); e = hipStreamCreateWithFlags(&p.s[slot], hipStreamNonBlocking); }
    if (e != hipSuccess) { (void)hipGetLastError(); p.s[slot] = nullptr; }
  }
  return p.s[slot];
}

struct EngineBase {
  virtual ~EngineBase() {}
  int nenv = 0, device = 0, precision = 32;
  int rm_rows = 0, rm_cols = 0;   // shape of RP_DEBUG_MASS_ROWS per env (the kernel build in use)
  int nv = 0, nu = 0, nsite = 0, ntree = 0, nkey = 0, nlink = 0, maxdepth = 0;
  hipStream_t stream = nullptr;
  // ring of HIP event pairs bracketing every step-kernel launch on `stream`
  static const int kRing = 128;
  hipEvent_t ev0[kRing] = {}, ev1[kRing] = {};
  bool ev_pending[kRing] = {};
  int ev_next = 0;
  double kernel_ms = 0; int kernel_launches = 0;
  // second ring: one solver-kernel (mj_step2) launch per rp_step call; the probed substep rotates
  // with the call count, so the running average is the mean over all substeps by construction
  hipEvent_t sv0[kRing] = {}, sv1[kRing] = {};
  unsigned step_calls = 0;
  // (kept per schedule kind -- [0] one launch per stage, [1] fused substeps -- and reported for the kind with more samples)
  double solver_ms_k[2] = {0, 0}, solver_envs_k[2] = {0, 0}; int solver_launches_k[2] = {0, 0};
  int sv_kind[kRing] = {};
  int sv_envs[kRing] = {};            // envs the probed solver launch of that slot covered (a slice or the batch)
  double last_solver_envs = 0;
  int last_solver_kind = 0;
  // schedule of the last rp_step when the engine chooses (n_slices == 0): see step().  Rule-based since round 6.
  int auto_mode = 1;
  bool many_heavy = false;   // the lists of envs outside the light class have been long lately (hysteresis)
  int last_nsl = 1;          // slices of the last rp_step
  void harvest(int i, bool wait) {
    if (!ev_pending[i]) return;
    if (wait) hipEventSynchronize(ev1[i]);
    else if (hipEventQuery(ev1[i]) != hipSuccess) return;
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev0[i], ev1[i]) == hipSuccess) {
      kernel_ms += ms; kernel_launches++;
    }
    if (sv_envs[i] > 0 && hipEventElapsedTime(&ms, sv0[i], sv1[i]) == hipSuccess) {
      const int kd = sv_kind[i] & 1;
      solver_ms_k[kd] += ms; solver_launches_k[kd]++; solver_envs_k[kd] += sv_envs[i];
    }
    sv_envs[i] = 0;   // (a step without a probe leaves 0)
    ev_pending[i] = false;
  }
  virtual int reset(const uint8_t* mask) = 0;
  virtual int set(rp_field f, const void* src) = 0;
  virtual int get(rp_field f, void* dst) = 0;
  virtual int step(int nsub, uint32_t* trace, int mode, const uint8_t* reset_mask = nullptr) = 0;
  virtual void limits(int newton, int ls) = 0;
  virtual void tolerances(double tol, double ls_tol) = 0;
  virtual void mpr_tolerances(double tol, double poly_tol) = 0;
  bool lazy_position = false;
  bool legacy_step = true;   // rp_set_legacy_step: false = dm_control's legacy_step=False output semantics
  // the reset snapshot's bookkeeping (rp_schedule.hpp); every setter that could change what the position stage computes
  // goes through option_changed()
  RpSnapshotState snap;
  void option_changed() { rp_snapshot_on_option(snap); }
  virtual int snapshot_flag_changed() = 0;   // (the device flag follows rp_snapshot_flag(snap))
  virtual int reset_snapshot(int on) = 0;    // rp_set_reset_snapshot
  bool cost_order = false;   // rp_set_cost_ordered_launch
  int n_slices = 1;          // rp_set_stream_slices (0 = automatic)
  static const int kMaxSlices = kRpMaxSlices;
  hipStream_t xstream[kMaxSlices] = {};   // [0] unused: slice 0 runs on the caller's stream
  hipEvent_t ev_fork = nullptr, ev_join[kMaxSlices] = {};
  // capacity classes: the full-capacity solver stage (few envs, one wave per SIMD, long waves) runs beside the
  // lean one on a companion stream of its slice, forked / joined with events every substep -- in one stream the
  // two launches serialise and every substep pays the slowest heavy env on an otherwise idle GPU
  hipStream_t hstream[kMaxSlices] = {};
  hipEvent_t ev_hfork[kMaxSlices] = {}, ev_hjoin[kMaxSlices] = {};
  virtual int acc_sensors(int on) = 0;
  virtual int lean_solver(int on) = 0;
  virtual int fused_substeps(int on) = 0;
  virtual int fused_substeps_on() const = 0;
  virtual int split_position(int on) = 0;
  virtual int split_position_on() const = 0;
  virtual int field_ptr(rp_field f, void** p, size_t* bytes) = 0;
  bool own_stream = true;
  virtual int profile(long long* out, int n, int enable) = 0;
};

template <typename T>
struct Engine : EngineBase {
  RpModel<T> M{};
  RpState<T> S{};
  RpStage<T> B{};
  std::vector<void*> allocs;
  std::vector<T> qpos0;
  T* d_qpos0 = nullptr;
  uint32_t* d_trace = nullptr; size_t trace_cap = 0;
  uint8_t* d_mask = nullptr;
  bool trunk4 = false;  // every tree has a 4-link trunk: launch the specialised solver build
  bool mesh = false;    // the model has convex-hull geoms: position / sensor stages with MPR
  bool graph = false;   // ... some of them with a vertex graph (more than 32 vertices): the MESH = 2 builds
  bool deep = false;    // a trunk of 5..8 links (more than two forearm dofs): the RPK_MAXD_DEEP builds
  StageVariant variant; // ... the four as the launch helpers read them
  int dense_joint = 0;  // RPK_LEAN_JOINT when RP_DENSE_HANDS=0 (goes to the kernels in S.lean)
  bool lean = false;    // light envs are stepped by rp_lean_solver_kernel (rp_solver2.hpp), the others by the full build
  // the position stage of the substeps as three launches: front part, pooled narrow phase (rp_collide.hpp), back part
  // split_mode: 0 = never, 1 = in every per-stage schedule, 2 = automatic: the schedule "three slices, split stage, no
  // companion streams" is a candidate of the engine's own choice (with rp_set_stream_slices(e, 0))
  bool split_capable = false;
  int split_mode = 0;
  bool split_now = false;   // (this rp_step)
  bool split_dropped = false;   // the split stage has overflowed its candidate / record lists once: the rule no longer picks it
  int split_position(int on) override {
    if (on && !split_capable) return fail("rp_set_split_position_stage: the split stage exists for the fp64 default-depth builds only");
    split_mode = on < 0 ? 2 : (on > 2 ? 2 : on);
    return 0;
  }
  // (0 = off, 1 = in use, 2 = the rule may pick it: rp_split_report)
  int split_position_on() const override { return rp_split_report(plan_input(0, false), auto_mode); }
  int lean_solver(int on) override {
    if (on && (deep || sizeof(T) != 8)) return fail("rp_set_lean_solver: the lean solver stage exists for the fp64 default builds only");
    lean = on != 0; S.lean = on > 0 ? ((on & RPK_LEAN_CAP) | dense_joint) : 0;   // (on > 1: the light class capped at that many Jacobian entries)
    return 0;
  }
  int md() const { return deep ? RPK_MAXD_DEEP : RPK_MAXD; }

  ~Engine() override {
    hipSetDevice(device);
    for (void* p : allocs) hipFree(p);
    if (d_trace) hipFree(d_trace);
    if (d_mask) hipFree(d_mask);
    if (h_heavy_peak) hipHostFree(h_heavy_peak);
    for (int i = 0; i < kRing; i++) {
      if (ev0[i]) hipEventDestroy(ev0[i]);
      if (ev1[i]) hipEventDestroy(ev1[i]);
      if (sv0[i]) hipEventDestroy(sv0[i]);
      if (sv1[i]) hipEventDestroy(sv1[i]);
    }
    if (stream && own_stream) hipStreamDestroy(stream);
    for (int i = 1; i < kMaxSlices; i++) {
      // (xstream / hstream: the process-wide pool's, never destroyed)
      if (ev_join[i]) hipEventDestroy(ev_join[i]);
    }
    for (int i = 0; i < kMaxSlices; i++) {
      if (ev_hfork[i]) hipEventDestroy(ev_hfork[i]);
      if (ev_hjoin[i]) hipEventDestroy(ev_hjoin[i]);
    }
    if (ev_fork) hipEventDestroy(ev_fork);
  }
  template <typename U> U* dalloc(size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, (n ? n : 1) * sizeof(U)) != hipSuccess) throw std::string("hipMalloc failed");
    hipMemset(p, 0, (n ? n : 1) * sizeof(U));
    allocs.push_back(p);
    return (U*)p;
  }
  const T* upF(const std::vector<double>& v) {
    std::vector<T> t(v.begin(), v.end());
    T* d = dalloc<T>(t.size());
    if (!t.empty()) hipMemcpy(d, t.data(), t.size() * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  const int* upI(const std::vector<int>& v) {
    int* d = dalloc<int>(v.size());
    if (!v.empty()) hipMemcpy(d, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice);
    return d;
  }

  void build(const Blob& b, int n_envs) {
    nenv = n_envs;
    read_options(b);
    upload_tables(b);
    alloc_state();
    read_switches();
    // The fills and uploads above went through the null stream, which is NOT ordered with the
    // engine's non-blocking stream: everything must have landed before the first kernel.
    if (hipDeviceSynchronize() != hipSuccess) throw std::string("hipDeviceSynchronize failed after model upload");
    variant.hull = mesh ? (graph ? 2 : 1) : 0; variant.deep = deep; variant.trunk4 = trunk4;
  }
  // sizes, limits and solver options
  void read_options(const Blob& b) {
    M.nlink = nlink = b.i1("eng_nlink"); M.ntree = ntree = b.i1("eng_ntree");
    M.maxdepth = maxdepth = b.i1("eng_maxdepth"); M.nkey = nkey = b.i1("eng_nkey");
    M.ngeom = b.i1("eng_ngeom");
    M.nu = nu = b.i1("eng_nu"); M.nsite = nsite = b.i1("eng_nsite"); M.nv = nv = b.i1("nv");
    if (M.nlink > RPK_NL_DEEP) throw std::string("too many hand dofs for the engine (max 60)");
    if (M.nkey > RPK_NKEYS) throw std::string("too many keys (max 128)");
    if (M.ngeom > RPK_WAVE) throw std::string("too many collision geoms (max 64)");
    if (M.nu > RPK_MAXACT) throw std::string("too many actuators");
    if (M.nsite > RPK_WAVE) throw std::string("too many sites (max 64)");
    if (M.maxdepth > RPK_MAXD_DEEP) throw std::string("tree too deep (max 13 levels: 8 trunk links + 5 finger links)");
    {
      std::vector<int> kind = b.i("eng_act_kind");
      for (int a = 0; a < nu; a++)
        if (kind[a] == 0 && a >= RPK_WAVE) throw std::string("hand actuator index >= 64");
    }
    M.iterations = b.i1("opt_iterations"); M.ls_iterations = b.i1("opt_ls_iterations");
    M.timestep = (T)b.f1("opt_timestep");
    auto g = b.f("opt_gravity");
    M.gx = (T)g[0]; M.gy = (T)g[1]; M.gz = (T)g[2];
    M.tolerance = (T)b.f1("opt_tolerance"); M.ls_tolerance = (T)b.f1("opt_ls_tolerance");
    // single precision cannot resolve MuJoCo's default 1e-8: iterating below 1e-6 only chases
    // rounding noise (measured: same accuracy against the fp64 engine, 5 % fewer iterations);
    // rp_set_solver_tolerance overrides this
    if (sizeof(T) == 4 && M.tolerance < (T)1e-6) M.tolerance = (T)1e-6;
    M.meaninertia = (T)b.f1("stat_meaninertia");
    // opt.impratio [MJ: mj_makeImpedance]: friction dimensions regularised by R / impratio
    {
      const double ir = b.has("opt_impratio") ? b.f1("opt_impratio") : 1.0;
      M.mu_scale = (T)std::sqrt(1.0 / (ir > 1e-15 ? ir : 1e-15));
    }
    M.mpr_tol = (T)1e-6; M.mpr_tol_poly = (T)1e-6;   // MuJoCo's uniform rule (rp_set_mpr_tolerance)
  }
  // every model table packed into the two device arrays (RpLayout offsets); the kernel builds the model needs
  void upload_tables(const Blob& b) {
    std::vector<double> ft((size_t)RpLayout::F_TOTAL, 0.0);
    std::vector<int> it((size_t)RpLayout::I_TOTAL, 0);
    auto putF = [&](int off, int cap, const std::vector<double>& v, const char* name) {
      if ((int)v.size() > cap) throw std::string("model table too large: ") + name;
      for (size_t i = 0; i < v.size(); i++) ft[(size_t)off + i] = v[i];
    };
    auto putI = [&](int off, int cap, const std::vector<int>& v, const char* name) {
      if ((int)v.size() > cap) throw std::string("model table too large: ") + name;
      for (size_t i = 0; i < v.size(); i++) it[(size_t)off + i] = v[i];
    };
#define PF(name, blobname) putF(RpLayout::F_##name, RpLayout::F_##name##_end - RpLayout::F_##name + 1, b.f(blobname), blobname)
#define PI(name, blobname) putI(RpLayout::I_##name, RpLayout::I_##name##_end - RpLayout::I_##name + 1, b.i(blobname), blobname)
    PI(lane_topo, "eng_lane_topo");
    PI(link_parent, "eng_link_parent"); PI(link_depth, "eng_link_depth"); PI(link_tree, "eng_link_tree");
    PI(link_jtype, "eng_link_jtype"); PI(link_dof, "eng_link_dof"); PI(link_sibrank, "eng_link_sibrank");
    PI(level_maxrank, "eng_level_maxrank"); PI(link_anc, "eng_link_anc"); PI(link_limited, "eng_link_limited");
    PI(link_act, "eng_link_act"); PI(link_desc, "eng_link_desc"); PI(link_ndesc, "eng_link_ndesc");
    PI(tree_base, "eng_tree_base"); PI(tree_trunk, "eng_tree_trunk"); PI(chain_first, "eng_chain_first");
    PI(chain_len, "eng_chain_len"); PI(link_ancmask, "eng_link_ancmask");
    {
      auto tt = b.i("eng_tree_trunk");
      trunk4 = M.ntree > 0;
      deep = M.maxdepth > RPK_MAXD || M.nlink > RPK_NL;
      for (int t = 0; t < M.ntree && t < (int)tt.size(); t++) {
        if (tt[t] > 8 || tt[t] < 1) throw std::string("the solver needs a trunk chain of 1..8 links per articulated tree");
        if (tt[t] != 4) trunk4 = false;
        if (tt[t] > 4) deep = true;   // (the register-blocked trunk of the default build holds 4 links)
      }
      if (getenv("RP_FORCE_DEEP")) { deep = true; trunk4 = false; }   // test hook: deep builds on any scene
    }
    for (int v : b.i("eng_chain_len")) if (v > 5) throw std::string("finger chain longer than 5 links is not supported by the solver");
    PF(link_lpos, "eng_link_lpos");
    {
      auto q = b.f("eng_link_lquat");
      std::vector<double> m(9 * (size_t)M.nlink);
      for (int i = 0; i < M.nlink; i++) {
        double w = q[4 * i], x = q[4 * i + 1], y = q[4 * i + 2], z = q[4 * i + 3];
        double* o = &m[9 * i];
        o[0] = 1 - 2 * (y * y + z * z); o[1] = 2 * (x * y - w * z); o[2] = 2 * (x * z + w * y);
        o[3] = 2 * (x * y + w * z); o[4] = 1 - 2 * (x * x + z * z); o[5] = 2 * (y * z - w * x);
        o[6] = 2 * (x * z - w * y); o[7] = 2 * (y * z + w * x); o[8] = 1 - 2 * (x * x + y * y);
      }
      putF(RpLayout::F_link_lmat, RPK_NL_DEEP * 9, m, "link_lmat");
    }
    PF(link_axis, "eng_link_axis"); PF(link_anchor, "eng_link_anchor"); PF(link_mass, "eng_link_mass");
    PF(link_ipos, "eng_link_ipos"); PF(link_inertia, "eng_link_inertia"); PF(link_invw_body, "eng_link_invw_body");
    PF(link_armature, "eng_link_armature"); PF(link_damping, "eng_link_damping");
    PF(link_stiffness, "eng_link_stiffness"); PF(link_springref, "eng_link_springref");
    PF(link_floss, "eng_link_floss"); PF(link_fl_R, "eng_link_fl_R"); PF(link_fl_B, "eng_link_fl_B");
    PF(link_range, "eng_link_range"); PF(link_lim_K, "eng_link_lim_K"); PF(link_lim_B, "eng_link_lim_B");
    PF(link_lim_solimp, "eng_link_lim_solimp"); PF(link_invw_dof, "eng_link_invw_dof");
    PF(link_act_coef, "eng_link_act_coef"); PF(link_gscale, "eng_link_gscale"); PF(tree_gscale, "eng_tree_gscale"); PF(tree_ref, "eng_tree_ref");
    PI(key_dof, "eng_key_dof"); PI(key_act, "eng_key_act"); PI(key_geomid, "eng_key_geomid");
    auto kpos = b.f("eng_key_pos"), khalf = b.f("eng_key_half");
    PF(key_pos, "eng_key_pos"); PF(key_half, "eng_key_half");
    {
      std::vector<double> rb((size_t)M.nkey);
      double zmax = -1e30;
      for (int k = 0; k < M.nkey; k++) {
        rb[k] = std::sqrt(khalf[3 * k] * khalf[3 * k] + khalf[3 * k + 1] * khalf[3 * k + 1] +
                          khalf[3 * k + 2] * khalf[3 * k + 2]);
        // the key box centre moves on a circle of radius hx about the hinge
        zmax = std::max(zmax, kpos[3 * k + 2] + khalf[3 * k] + rb[k]);
      }
      putF(RpLayout::F_key_rbound, RPK_NKEYS, rb, "key_rbound");
      M.key_zmax = (T)zmax;
    }
    PF(key_mass, "eng_key_mass"); PF(key_M, "eng_key_M"); PF(key_stiffness, "eng_key_stiffness");
    PF(key_springref, "eng_key_springref"); PF(key_damping, "eng_key_damping"); PF(key_range, "eng_key_range");
    PF(key_lim_K, "eng_key_lim_K"); PF(key_lim_B, "eng_key_lim_B"); PF(key_lim_solimp, "eng_key_lim_solimp");
    PF(key_invw_dof, "eng_key_invw_dof"); PF(key_invw_body, "eng_key_invw_body"); PF(key_cparam, "eng_key_cparam");
    PI(geom_link, "eng_geom_link"); PI(geom_type, "eng_geom_type"); PI(geom_modelid, "eng_geom_modelid");
    PI(geom_pairmask, "eng_geom_pairmask"); PI(geom_iskeycap, "eng_geom_iskeycap");
    PF(geom_size, "eng_geom_size"); PF(geom_pos, "eng_geom_pos"); PF(geom_mat, "eng_geom_mat");
    PF(geom_rbound, "eng_geom_rbound"); PF(geom_invw, "eng_geom_invw"); PF(geom_cparam, "eng_geom_cparam");
    PF(geom_bcap, "eng_geom_bcap");
    PI(act_kind, "eng_act_kind"); PI(act_lane, "eng_act_lane"); PI(act_ctrllimited, "eng_act_ctrllimited");
    PI(act_forcelimited, "eng_act_forcelimited");
    PF(act_coef, "eng_act_coef"); PF(act_gain, "eng_act_gain"); PF(act_bias, "eng_act_bias");
    PF(act_ctrlrange, "eng_act_ctrlrange"); PF(act_forcerange, "eng_act_forcerange");
    PI(site_link, "eng_site_link"); PF(site_pos, "eng_site_pos");
    if (b.has("eng_site_touch_radius")) PF(site_touch_radius, "eng_site_touch_radius");
    if (b.has("eng_link_bodylink")) PI(link_bodylink, "eng_link_bodylink");
    if (b.has("eng_mesh_vert")) {
      PF(mesh_vert, "eng_mesh_vert"); PI(geom_vertadr, "eng_geom_vertadr"); PI(geom_vertnum, "eng_geom_vertnum");
      if (b.has("eng_geom_vertflip")) PI(geom_vertflip, "eng_geom_vertflip");
      if (b.has("eng_geom_vertgraph")) PI(geom_vertgraph, "eng_geom_vertgraph");
      for (int t : b.i("eng_geom_type")) if (t == GEOM_MESH_) mesh = true;
    }
    // cylinders collide through the portal refinement like hulls; their support function is compiled into the MESH = 2
    // builds only (the builds of scenes with the real hand's colliders: graph hulls, cylinders), so that the benchmark's
    // kernels stay what they were
    for (int t : b.i("eng_geom_type")) if (t == GEOM_CYL_) { mesh = true; graph = true; }
#undef PF
#undef PI
    M.ft = upF(ft);
    M.it = upI(it);
    if (b.has("eng_hull_vert") && !b.f("eng_hull_vert").empty()) {
      if (b.i("eng_hull_graph").size() != b.f("eng_hull_vert").size() / 3 * RPK_HULL_GRAPH_ROW) throw std::string("eng_hull_graph does not match eng_hull_vert");
      M.hull_vert = upF(b.f("eng_hull_vert"));
      M.hull_graph = upI(b.i("eng_hull_graph"));
      graph = true;
    }
    {
      auto q0 = b.f("qpos0");
      qpos0.assign(q0.begin(), q0.end());
      d_qpos0 = const_cast<T*>(upF(q0));
    }
  }
  // the env-major state, hand-over and bookkeeping arrays
  void alloc_state() {
    size_t E = (size_t)nenv;
    S.nenv = nenv;
    S.qpos = dalloc<T>(E * nv); S.qvel = dalloc<T>(E * nv); S.warm = dalloc<T>(E * nv);
    S.ctrl = dalloc<T>(E * nu); S.qfrc_applied = dalloc<T>(E * nv); S.time = dalloc<T>(E);
    S.tree_offset = dalloc<T>(E * (ntree ? ntree : 1) * 3);
    S.act_force = dalloc<T>(E * nu); S.act_vel = dalloc<T>(E * nu);
    S.site_xpos = dalloc<T>(E * (nsite ? nsite : 1) * 3);
    S.contact_dist = dalloc<T>(E * RPK_NCOUT);
    S.ncon = dalloc<int>(E); S.contact_geoms = dalloc<int>(E * RPK_NCOUT * 2);
    S.warn = dalloc<int>(E); S.solver_iter = dalloc<int>(E);
    B.RM = dalloc<T>(E * RPK_NLX(md()) * (md() + 1));
    rm_rows = RPK_NLX(md()); rm_cols = md() + 1;
    B.lanef = dalloc<T>(E * RPK_NLF * 64);
    B.lanei = dalloc<int>(E * RPK_NLI * 64);
    B.hdr = dalloc<int>(E * rpk::HDR_N);
    B.entJ = dalloc<T>(E * RpCaps<T>::NE * 3);
    B.entM = dalloc<int>(E * RpCaps<T>::NE * 2);
    B.slots = dalloc<int>(E * rpk::SLOT_N);
    B.keyslot = dalloc<int>(E * (RPK_NKEYS / 4));
    B.covf = dalloc<T>(E * (RPK_NC - RPK_NCL) * 12);
    B.covi = dalloc<int>(E * (RPK_NC - RPK_NCL) * 4);
    // hand-over buffers start as NaN / -1 patterns: a read of anything the position kernel
    // did not write this substep shows up as a bad state instead of silently reusing old data
    hipMemset(B.RM, 0xFF, sizeof(T) * E * RPK_NLX(md()) * (md() + 1));
    hipMemset(B.lanef, 0xFF, sizeof(T) * E * RPK_NLF * 64);
    hipMemset(B.lanei, 0xFF, sizeof(int) * E * RPK_NLI * 64);
    hipMemset(B.hdr, 0xFF, sizeof(int) * E * rpk::HDR_N);
    hipMemset(B.entJ, 0xFF, sizeof(T) * E * RpCaps<T>::NE * 3);
    hipMemset(B.entM, 0xFF, sizeof(int) * E * RpCaps<T>::NE * 2);
    hipMemset(B.slots, 0xFF, sizeof(int) * E * rpk::SLOT_N);
    hipMemset(B.keyslot, 0xFF, sizeof(int) * E * (RPK_NKEYS / 4));
    S.key_trace = nullptr;
    S.prof = nullptr;
    d_active = dalloc<int>(E);
    S.active = nullptr;
    d_lead = dalloc<int>(E);
    d_order = dalloc<int>(E);
    {
      std::vector<int> id(E);
      for (size_t i = 0; i < E; i++) id[i] = (int)i;
      hipMemcpy(d_order, id.data(), E * sizeof(int), hipMemcpyHostToDevice);
    }
    S.cost_pos = dalloc<int>(E); S.cost_sol = dalloc<int>(E);
    d_heavy = dalloc<int>(E); d_heavy_cnt = dalloc<int>(2 * kMaxSlices);   // (zero-filled)
    d_listed = dalloc<unsigned char>(E); S.listed = d_listed;
    // ([kMaxSlices]: candidates the split position stage dropped this step, RP_WARN_SPLIT_FULL -- read back with the peaks)
    d_heavy_peak = dalloc<int>(kMaxSlices + 1);
    if (hipHostMalloc((void**)&h_heavy_peak, sizeof(int) * (kMaxSlices + 1)) != hipSuccess) { (void)hipGetLastError(); h_heavy_peak = nullptr; }
    else { for (int i = 0; i < kMaxSlices; i++) h_heavy_peak[i] = -1; h_heavy_peak[kMaxSlices] = 0; }
    S.heavy_list = nullptr; S.heavy_cnt = nullptr; S.heavy_done = nullptr;
    S.qpos_prev = nullptr; S.qvel_prev = nullptr;
    d_valid = dalloc<unsigned char>(E);  // (zero-filled: nothing is valid yet)
    S.max_newton = M.iterations; S.max_ls = M.ls_iterations;
    alloc_snapshot();
  }
  // The pristine env of the reset snapshot (rp_model.hpp: RpSnapshot): a one-env state and hand-over of its own, beside
  // the batch -- no env count, stride, slice bound or list of the batch knows of it.  Never stepped.
  RpSnapshot<T> P{};
  int* d_snap_ok = nullptr;
  void alloc_snapshot() {
    RpState<T>& s = P.S;
    s = RpState<T>{};
    s.nenv = 1;
    s.qpos = dalloc<T>(nv); s.qvel = dalloc<T>(nv); s.warm = dalloc<T>(nv);
    s.ctrl = dalloc<T>(nu); s.qfrc_applied = dalloc<T>(nv); s.time = dalloc<T>(1);
    s.tree_offset = dalloc<T>((ntree ? ntree : 1) * 3);   // (zeros, not null: the stage adds them as it does for the batch)
    s.act_force = dalloc<T>(nu); s.act_vel = dalloc<T>(nu);
    s.site_xpos = dalloc<T>((nsite ? nsite : 1) * 3);
    s.contact_dist = dalloc<T>(RPK_NCOUT);
    s.ncon = dalloc<int>(1); s.contact_geoms = dalloc<int>(RPK_NCOUT * 2);
    s.warn = dalloc<int>(1); s.solver_iter = dalloc<int>(1);
    s.cost_pos = dalloc<int>(1); s.cost_sol = dalloc<int>(1);
    RpStage<T>& b = P.B;
    b = RpStage<T>{};
    P.md = md();
#define X(buf, per_env, live) b.buf = dalloc<std::remove_pointer_t<decltype(b.buf)>>(per_env);
    { const int md = P.md; RPK_SNAPSHOT_HANDOVER(X) }
#undef X
    d_snap_valid = dalloc<unsigned char>(1);
    d_snap_ok = dalloc<int>(1);   // (zero: no snapshot yet)
    P.ok = d_snap_ok;
  }
  // Builds the snapshot on the engine's stream: physics.reset() of the pristine env, then the engine's own position /
  // velocity stage for it -- the one-kernel stage, which is bit-identical to the split stage and needs no pooled lists.
  // The options the stage reads travel with the launch (M, S.lean), so a build after a setter sees the new values.
  void build_snapshot() {
    RpState<T> s = P.S;
    s.max_newton = S.max_newton; s.max_ls = S.max_ls; s.lean = S.lean;
    RpSnapshot<T> none{};
    hipLaunchKernelGGL(rp_reset_kernel<T>, dim3(1), dim3(64), 0, stream, s, d_qpos0, (const unsigned char*)nullptr, nv, nu, nsite, d_snap_valid, P.B, none);
    launch_stage<T, 0>(variant, 1, stream, M, s, P.B, -1, 1);
    snap_built = true;
    rp_snapshot_on_built(snap);
    snapshot_flag_changed();
  }
  unsigned char* d_snap_valid = nullptr;   // (the pristine env's own stage_valid byte: written by its reset, read by nothing)
  bool snap_built = false;                 // the pristine env holds a snapshot, fresh or not
  int reset_snapshot(int on) override {
    HIP_OK(hipSetDevice(device));
    snap.enabled = on != 0;
    option_changed();
    if (!on) {
      // off means "as if the snapshot had never existed": the hand-overs earlier resets copied are recomputed too
      HIP_OK(hipMemsetAsync(d_valid, 0, (size_t)nenv, stream));
      rp_snapshot_on_state_write(snap, false, stream_capturing());
    }
    return snapshot_flag_changed();
  }
  int snapshot_flag_changed() override {
    if (!d_snap_ok || !snap_built) return 0;   // (never built: the flag is still the zero it was allocated with)
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipMemsetAsync(d_snap_ok, (rp_snapshot_flag(snap) && snap_built) ? 1 : 0, 1, stream));
    return 0;
  }
  // RP_SPLIT_POS, RP_LEAN, RP_DENSE_HANDS (RP_FORCE_DEEP: upload_tables; RP_FUSED, RP_FUSED_SPLIT, RP_HEAVY_GRID: their members)
  void read_switches() {
    // split position stage (front part -> pooled narrow phase -> back part): the fp64 default-depth builds
    {
      const char* sp = getenv("RP_SPLIT_POS");
      split_capable = sizeof(T) == 8 && !deep;
      split_mode = !split_capable ? 0 : (sp ? (sp[0] == '0' ? 0 : (sp[0] == '1' ? 1 : 2)) : 2);
      // (the buffers -- 78 KB per env: 320 MB at 4096 envs -- are allocated by the first rp_step that runs the split stage:
      // ensure_split_buffers; an engine that never does, small batches and RP_SPLIT_POS=0 among them, never pays for them)
    }
    {
      // The reset snapshot is off in a new engine, as the lazy mode is: rp_set_reset_snapshot turns it on (the env layer,
      // suite/physics.py, does).  RP_RESET_SNAPSHOT=1 / =0 sets the engine's own default.  Off: every launch as before it existed.
      const char* rs = getenv("RP_RESET_SNAPSHOT");
      snap.enabled = rs && rs[0] != '0';
    }
    {
      const char* le = getenv("RP_LEAN");
      lean = sizeof(T) == 8 && !deep && !(le && le[0] == '0');
      // RP_DENSE_HANDS=0: the lean solver stage keeps the dirty rows of both hands in ONE dense block whatever the
      // contacts (default: a block per hand, side by side, when no contact couples the hands -- same bits)
      const char* dh = getenv("RP_DENSE_HANDS");
      dense_joint = (dh && dh[0] == '0') ? RPK_LEAN_JOINT : 0;
      S.lean = lean ? (1 | dense_joint) : 0;
      if (lean && le && atoi(le) > 1) S.lean = (atoi(le) & RPK_LEAN_CAP) | dense_joint;   // (RP_LEAN=n > 1: the light class capped at n Jacobian entries, as rp_set_lean_solver(e, n))
    }
  }

  // The split position stage's buffers, on first use.  False (and the split stage off for good) when the device has no
  // room for them: the one-kernel stage computes the same bits.
  bool split_alloc_failed = false;
  bool ensure_split_buffers() {
    if (B.frames) return true;
    if (split_alloc_failed) return false;
    const size_t E = (size_t)nenv;
    const size_t mark = allocs.size();
    try {
      T* frames = dalloc<T>(E * RPK_NFRAME * 64);
      B.cand = dalloc<int>(E * RPK_NCAND * 2);
      B.ncand = dalloc<int>(E);
      B.cres = dalloc<T>(E * RPK_NRES * 12);
      B.cres_n = dalloc<int>(E * RPK_NCAND);
      B.tstride = ((E + RPK_NSTRIPE - 1) / RPK_NSTRIPE + 1) * RPK_NCAND;   // (+1: a slice's stripe may hold one env more than cnt / 8)
      B.tlist = dalloc<int>((size_t)RPK_NTYPE * RPK_NSTRIPE * B.tstride * 4);
      B.tcount = dalloc<int>(kMaxSlices * RPK_NSTRIPE * RPK_NTYPE_PAD);   // (zero-filled)
      B.tcount_off = 0;
      hipMemset(B.ncand, 0xFF, sizeof(int) * E);        // -1: no front part has run
      hipMemset(frames, 0xFF, sizeof(T) * E * RPK_NFRAME * 64);
      B.frames = frames;
      // (null-stream fills vs the engine's non-blocking streams, as at the end of build())
      if (hipDeviceSynchronize() != hipSuccess) throw std::string("hipDeviceSynchronize failed");
    } catch (const std::string&) {
      (void)hipGetLastError();
      while (allocs.size() > mark) { hipFree(allocs.back()); allocs.pop_back(); }
      B.frames = nullptr; B.cand = nullptr; B.ncand = nullptr; B.cres = nullptr; B.cres_n = nullptr; B.tlist = nullptr; B.tcount = nullptr;
      split_alloc_failed = true; split_mode = 0;
      return false;
    }
    return true;
  }
  long long* d_prof = nullptr;
  int* d_active = nullptr;
  int* d_order = nullptr;           // cost-ordered launch: workgroup -> env
  // the envs outside the light capacity class, compacted per slice (entries base .. of slice sl; d_heavy_cnt[2 sl]
  // = entries, [2 sl + 1] = finished workgroups of the stage that walks them)
  int *d_heavy = nullptr, *d_heavy_cnt = nullptr;
  unsigned char* d_listed = nullptr;   // 1 = on the list of the substep just solved (rp_order_kernel's snapshot)
  // Grid of the full-capacity solver stage.  Each of its workgroups needs a whole idle SIMD (512 registers) and 55 KB of
  // LDS even to find the list empty, and the slice's join waits for the last of them: the grid follows the longest
  // list the stage saw recently -- read back one step late, never waited for (a list longer than the grid is walked
  // in rounds: slower for a step, never wrong).  Measured with the 55 KB stage, config 2 hull: fixed 128: 618 k
  // env-steps/s, following the list: 651 k (the 40 KB stage of round 3 at 128: 650 k).
  int *d_heavy_peak = nullptr, *h_heavy_peak = nullptr;
  double heavy_est[kMaxSlices] = {8, 8, 8, 8};
  int heavy_grid_for(int sl, int cnt) {
    if (heavy_grid_fixed || !h_heavy_peak) return cnt < kHeavyGrid ? cnt : kHeavyGrid;
    const int seen = *(volatile int*)&h_heavy_peak[sl];
    if (seen >= 0) { heavy_est[sl] = rp_heavy_est_update(heavy_est[sl], seen); *(volatile int*)&h_heavy_peak[sl] = -1; }
    return rp_heavy_grid(heavy_est[sl], cnt, kHeavyGrid);
  }
  // fused substeps (rp_fused_steps_kernel): one launch takes every light env through all substeps of an rp_step
  // 0 = off, 1 = on, 2 = automatic (a candidate of the schedule choice when the slice count is automatic too)
  int fused = getenv("RP_FUSED") ? atoi(getenv("RP_FUSED")) : 2;
  const bool fused_split = !(getenv("RP_FUSED_SPLIT") && getenv("RP_FUSED_SPLIT")[0] == '0');
  int fused_substeps(int on) override { fused = on < 0 ? 2 : (on > 2 ? 2 : on); return 0; }
  int fused_substeps_on() const override { return rp_fused_report(plan_input(0, false), auto_mode); }
  // what the schedule rule (rp_schedule.hpp) reads, as the engine stands
  RpStepInput plan_input(int mode, bool capturing) const {
    RpStepInput in;
    in.nenv = nenv; in.mode = mode; in.n_slices = n_slices;
    in.fused = fused; in.fused_capable = rp_fused_capable(lean, deep, graph, sizeof(T) == 8);
    in.split_mode = split_mode; in.split_capable = split_capable; in.split_dropped = split_dropped;
    in.capturing = capturing; in.lean = lean; in.deep = deep; in.graph = graph;
    for (int i = 0; i < kMaxSlices; i++) in.heavy_est[i] = heavy_est[i];
    in.last_nsl = last_nsl; in.many_heavy = many_heavy;
    return in;
  }
  // MEASUREMENT-ONLY switches (they skip or repeat work: wrong physics / wasted time).  Compiled in only with
  // -DRP_EXPERIMENTS, and loud when set: a stray environment variable must not silently change a production step.
#ifdef RP_EXPERIMENTS
  static bool x_switch(const char* name) {
    const char* v = getenv(name);
    const bool on = v && v[0] == '1';
    if (on) fprintf(stderr, "librp_engine: MEASUREMENT-ONLY switch %s=1 is active -- results are not valid physics\n", name);
    return on;
  }
  const bool x_no_heavy = x_switch("RP_X_NO_HEAVY");
  const bool x_order_twice = x_switch("RP_X_ORDER_TWICE");
#else
  static constexpr bool x_no_heavy = false, x_order_twice = false;
#endif
  // (Measured and not kept, rounds 4-5: the lean launch in FRONT of the full-capacity one where there is no companion stream
  // (660 against 668 k env-steps/s); a high-priority companion stream (no effect on the dispatch order); the full-capacity
  // launch on the slice's own stream with two slices (-2.5 %).)
  // (each of these workgroups needs a whole idle SIMD, also just to find the list empty: 512 of them delayed the slice's join;
  // measured 64 ... 128 best on configs 2-4, 16 starves config 3)
  const int kHeavyGrid = getenv("RP_HEAVY_GRID") ? (atoi(getenv("RP_HEAVY_GRID")) > 0 ? atoi(getenv("RP_HEAVY_GRID")) : 1) : 128;   // (one wave of that stage owns a SIMD: half the chip at most)
  const bool heavy_grid_fixed = getenv("RP_HEAVY_GRID") != nullptr;   // (experiment: RP_HEAVY_GRID pins the grid)
  // acceleration-stage sensors (rp_set_acc_sensors): state before the last Euler step, outputs
  bool sensors_on = false;
  T *d_qpos_prev = nullptr, *d_qvel_prev = nullptr, *d_con_force = nullptr, *d_sens_torque = nullptr,
    *d_sens_touch = nullptr;
  int acc_sensors(int on) override {
    if (on && !d_qpos_prev) {
      HIP_OK(hipSetDevice(device));
      try {
        size_t E = (size_t)nenv;
        d_qpos_prev = dalloc<T>(E * nv); d_qvel_prev = dalloc<T>(E * nv);
        d_con_force = dalloc<T>(E * RPK_NC * 4);
        d_sens_torque = dalloc<T>(E * nv); d_sens_touch = dalloc<T>(E * (nsite ? nsite : 1));
      } catch (const std::string& s) { return fail("rp_set_acc_sensors: " + s); }
      HIP_OK(hipDeviceSynchronize());  // (null-stream fills vs the engine's stream)
    }
    sensors_on = on != 0;
    S.con_force = sensors_on ? d_con_force : nullptr;
    return 0;
  }
  int* d_lead = nullptr;            // lazy position stage: active && !valid
  unsigned char* d_valid = nullptr; // hand-over of env e matches its state
  int profile(long long* out, int n, int enable) override {
    HIP_OK(hipSetDevice(device));
    if (!d_prof) { d_prof = dalloc<long long>(RPK_NPROF_ALL); }
    HIP_OK(hipStreamSynchronize(stream));
    if (out) {
      long long h[RPK_NPROF_ALL];
      HIP_OK(hipMemcpy(h, d_prof, sizeof(h), hipMemcpyDeviceToHost));
      for (int i = 0; i < n && i < RPK_NPROF_ALL; i++) out[i] = h[i];
    }
    HIP_OK(hipStreamSynchronize(stream));  // counters of launches still in flight
    HIP_OK(hipMemset(d_prof, 0, sizeof(long long) * RPK_NPROF_ALL));
    HIP_OK(hipDeviceSynchronize());        // (null-stream fill vs the engine's non-blocking stream)
    S.prof = enable ? d_prof : nullptr;
    return 0;
  }
  void mpr_tolerances(double tol, double poly_tol) override {
    const double floor_ = sizeof(T) == 4 ? 1e-6 : 0.0;   // (single precision cannot resolve a tighter portal distance)
    if (tol > 0) M.mpr_tol = (T)(tol > floor_ ? tol : floor_);
    if (poly_tol > 0) M.mpr_tol_poly = (T)(poly_tol > floor_ ? poly_tol : floor_);
    else M.mpr_tol_poly = M.mpr_tol;   // (<= 0: back to `tolerance`, whether this call changed it or not)
  }
  void tolerances(double tol, double ls_tol) override {
    if (tol > 0) M.tolerance = (T)tol;
    if (ls_tol > 0) M.ls_tolerance = (T)ls_tol;
  }
  void limits(int newton, int ls) override {
    if (newton > 0) S.max_newton = newton;
    if (ls > 0) S.max_ls = ls;
  }

  // One builder each for the states the launches below get instead of S:
  // ... rp_reset_kernel: with the sensor outputs to clear
  RpState<T> reset_state() const {
    RpState<T> sr = S;
    sr.sens_torque = sensors_on ? d_sens_torque : nullptr; sr.sens_touch = sensors_on ? d_sens_touch : nullptr;
    return sr;
  }
  // ... the stages that walk or fill slice sl's list of envs outside the light class
  RpState<T> heavy_state(const RpState<T>& ss, int sl, bool capturing) const {
    RpState<T> sh = ss;
    sh.heavy_list = d_heavy + ss.env_base; sh.heavy_cnt = d_heavy_cnt + 2 * sl; sh.heavy_done = d_heavy_cnt + 2 * sl + 1;
    sh.heavy_peak = capturing ? nullptr : d_heavy_peak + sl;
    return sh;
  }
  // ... the sensor stage: the state before the last substep in, the sensor arrays out
  RpState<T> sensor_state(const RpState<T>& ss) const {
    RpState<T> sq = ss;
    sq.qpos = d_qpos_prev; sq.qvel = d_qvel_prev;
    sq.sens_torque = d_sens_torque; sq.sens_touch = d_sens_touch;
    sq.key_trace = nullptr; sq.prof = nullptr;
    return sq;
  }

  // physics.reset() of the envs a device mask flags (null: all) -- rp_reset and rp_step_masked
  // Returns true when the envs got the reset snapshot with it (their hand-over is valid: no leading stage for them).
  // lead_follows: rp_step_masked -- the leading stage of the same call takes the envs that did not get it.
  bool launch_reset(const unsigned char* dmask, bool capturing, bool lead_follows) {
    const RpSnapshotUse use = rp_snapshot_use(snap, capturing);
    if (use == kRpSnapBuild) build_snapshot();
    const bool used = use != kRpSnapNone;
    RpSnapshot<T> p = P;
    if (!used) p.ok = nullptr;
    // (four waves per env when there is a snapshot to copy: ~22 KB per reset env, a dependent load -> store trip per KB and wave)
    hipLaunchKernelGGL(rp_reset_kernel<T>, dim3(nenv), dim3(used ? 256 : 64), 0, stream, reset_state(), d_qpos0, dmask, nv, nu, nsite, d_valid, B, p);
    rp_snapshot_on_reset(snap, used, dmask == nullptr, lead_follows, capturing);
    return used;
  }
  bool stream_capturing() const {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream, &cap);
    return cap != hipStreamCaptureStatusNone;
  }
  int reset(const uint8_t* mask) override {
    HIP_OK(hipSetDevice(device));
    const unsigned char* dmask = nullptr;
    if (mask) {
      if (is_device_ptr(mask)) dmask = mask;
      else {
        if (!d_mask) HIP_OK(hipMalloc((void**)&d_mask, (size_t)nenv));
        HIP_OK(hipMemcpyAsync(d_mask, mask, (size_t)nenv, hipMemcpyHostToDevice, stream));
        HIP_OK(hipStreamSynchronize(stream));  // host source may go away
        dmask = d_mask;
      }
    }
    launch_reset(dmask, stream_capturing(), false);
    HIP_OK(hipGetLastError());
    return 0;
  }

  bool field(rp_field f, void** p, size_t* bytes, bool* writable) {
    size_t E = (size_t)nenv;
    *writable = false;
    switch (f) {
      case RP_QPOS: *p = S.qpos; *bytes = sizeof(T) * E * nv; *writable = true; return true;
      case RP_QVEL: *p = S.qvel; *bytes = sizeof(T) * E * nv; *writable = true; return true;
      case RP_QACC_WARMSTART: *p = S.warm; *bytes = sizeof(T) * E * nv; *writable = true; return true;
      case RP_CTRL: *p = S.ctrl; *bytes = sizeof(T) * E * nu; *writable = true; return true;
      case RP_QFRC_APPLIED: *p = S.qfrc_applied; *bytes = sizeof(T) * E * nv; *writable = true; return true;
      case RP_ACT_FORCE: *p = S.act_force; *bytes = sizeof(T) * E * nu; return true;
      case RP_ACT_VELOCITY: *p = S.act_vel; *bytes = sizeof(T) * E * nu; return true;
      case RP_SITE_XPOS: *p = S.site_xpos; *bytes = sizeof(T) * E * nsite * 3; return true;
      case RP_TIME: *p = S.time; *bytes = sizeof(T) * E; *writable = true; return true;
      case RP_NCON: *p = S.ncon; *bytes = sizeof(int) * E; return true;
      case RP_CONTACT_GEOMS: *p = S.contact_geoms; *bytes = sizeof(int) * E * RPK_NCOUT * 2; return true;
      case RP_WARN_FLAGS: *p = S.warn; *bytes = sizeof(int) * E; *writable = true; return true;
      case RP_SOLVER_ITER: *p = S.solver_iter; *bytes = sizeof(int) * E; return true;
      case RP_CONTACT_DIST: *p = S.contact_dist; *bytes = sizeof(T) * E * RPK_NCOUT; return true;
      case RP_ACTIVE: *p = d_active; *bytes = sizeof(int) * E; *writable = true; return true;
      case RP_TREE_OFFSET: *p = S.tree_offset; *bytes = sizeof(T) * E * ntree * 3; *writable = true; return true;
      case RP_ENV_COST: *p = S.cost_sol; *bytes = sizeof(int) * E; return true;
      case RP_DEBUG_MASS_ROWS: *p = B.RM; *bytes = sizeof(T) * E * RPK_NLX(md()) * (md() + 1); return true;
      case RP_DEBUG_HANDOVER_HDR: *p = B.hdr; *bytes = sizeof(int) * E * rpk::HDR_N; return true;
      case RP_SENSOR_TORQUE: if (!d_sens_torque) return false; *p = d_sens_torque; *bytes = sizeof(T) * E * nv; return true;
      case RP_SENSOR_TOUCH: if (!d_sens_touch) return false; *p = d_sens_touch; *bytes = sizeof(T) * E * nsite; return true;
    }
    return false;
  }
  int field_ptr(rp_field f, void** p, size_t* bytes) override {
    bool w;
    if (!field(f, p, bytes, &w)) return fail("rp_field_ptr: unknown field (sensor fields need rp_set_acc_sensors first)");
    if (f == RP_ACTIVE) S.active = d_active;  // a caller that maps the mask uses it
    return 0;
  }
  int set(rp_field f, const void* src) override {
    void* p; size_t nb; bool w;
    if (!field(f, &p, &nb, &w)) return fail("rp_set: unknown field");
    if (!w) return fail("rp_set: field is read-only");
    if (!src) { if (f == RP_ACTIVE) { S.active = nullptr; return 0; } return fail("rp_set: null source"); }
    HIP_OK(hipSetDevice(device));
    if (nb) {
      // Host sources: drain the stream first.  Stream order alone should put this copy after
      // the kernels already enqueued, but under rocprofv3 --pmc (dispatch interception) a
      // pending kernel was observed to run after a later host-to-device copy.
      if (!is_device_ptr(src)) HIP_OK(hipStreamSynchronize(stream));
      HIP_OK(hipMemcpyAsync(p, src, nb, hipMemcpyDefault, stream));
    }
    if (f == RP_ACTIVE) S.active = d_active;
    // state the position stage depends on changed: every env's hand-over is stale
    if (f == RP_QPOS || f == RP_QVEL || f == RP_TREE_OFFSET) {
      HIP_OK(hipMemsetAsync(d_valid, 0, (size_t)nenv, stream));
      rp_snapshot_on_state_write(snap, f == RP_TREE_OFFSET, stream_capturing());
      // (tree offsets: a reset state is no longer the same for every env -- the snapshot is off for this engine)
      if (f == RP_TREE_OFFSET) RP_TRY(snapshot_flag_changed());
    }
    return 0;
  }
  int get(rp_field f, void* dst) override {
    void* p; size_t nb; bool w;
    if (!field(f, &p, &nb, &w)) return fail("rp_get: unknown field");
    if (!dst) return fail("rp_get: null destination");
    HIP_OK(hipSetDevice(device));
    if (nb) HIP_OK(hipMemcpyAsync(dst, p, nb, hipMemcpyDefault, stream));
    if (!is_device_ptr(dst)) HIP_OK(hipStreamSynchronize(stream));  // device destinations stay stream-ordered
    return 0;
  }
  // ---- rp_step / rp_forward / rp_step_masked: the host half, part by part (step() at the end puts them in order) ----

  // What one call hands from part to part (on step()'s stack).
  struct StepCtx {
    int nsub = 0, mode = 0;
    const uint8_t* reset_mask = nullptr;
    bool capturing = false, timeit = false, lead_masked = false;
    int slot = 0;          // of the timer rings
    RpStepInput in;
    RpStepPlan plan;
    int nsl = 1;           // slices, after the runtime's vetoes
    RpState<T> s;          // S with this call's key trace, order and output flags
  };
  // One slice of the batch: the envs [base, base + cnt) on stream st
  struct Slice {
    int sl = 0, base = 0, cnt = 0;
    hipStream_t st = nullptr;
    RpState<T> ss;         // StepCtx::s with env_base = base
    int hgrid_step = 0;    // (the full-capacity stage's grid: one choice per step and slice)
  };

  // inside a stream capture (the caller is recording a hipGraph of its whole step) no
  // event may be synchronised and per-launch events are meaningless: skip the timers
  int begin_timers(StepCtx& c) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream, &cap);
    c.capturing = cap != hipStreamCaptureStatusNone;
    c.slot = ev_next;
    if (!c.capturing) {
      ev_next = (ev_next + 1) % kRing;
      harvest(c.slot, true);
    }
    c.timeit = (c.mode == 0) && !c.capturing;
    if (c.timeit) HIP_OK(hipEventRecord(ev0[c.slot], stream));
    return 0;
  }

  // The schedule of this call: the rule (rp_schedule.hpp), then the vetoes that need the runtime, in this order: the
  // split stage's buffers, the fork event, the slices' streams and join events.
  void plan(StepCtx& c) {
    c.in = plan_input(c.mode, c.capturing);
    if (rp_engine_chooses(c.in)) {
      // (the drop count of the split stage comes back with the list lengths: rp_plan_step's comment on split_ok)
      if (h_heavy_peak && *(volatile int*)&h_heavy_peak[kMaxSlices] > 0) split_dropped = true;
      c.in.split_dropped = split_dropped;
    }
    c.plan = rp_plan_step(c.in);
    many_heavy = c.plan.many_heavy;
    if (c.plan.sched && !c.capturing) auto_mode = c.plan.sched;
    split_now = c.plan.split_wanted;
    if (split_now && ((c.capturing && !B.frames) || !ensure_split_buffers())) split_now = false;   // (no allocation inside a stream capture)
    int nsl = c.plan.nsl;
    if (c.mode == 0 && !c.capturing) last_nsl = nsl;
    if (nsl > 1 && !ev_fork && hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); ev_fork = nullptr; nsl = 1; }
    for (int i = 1; i < nsl; i++) {
      if (xstream[i]) continue;
      xstream[i] = pooled_stream(device, i, false);
      if (!xstream[i] || hipEventCreateWithFlags(&ev_join[i], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); xstream[i] = nullptr; nsl = 1; break; }
    }
    c.nsl = nsl;
  }

  // Slices: the batch may be stepped as two halves on two streams.  Within a half the kernels are
  // ordered (solver -> position -> solver ...), between the halves they are not, so the tail of one
  // half's launch (a few heavy envs still running, most SIMDs idle) is filled by the other half's
  // next kernel instead of waiting for a launch boundary.
  int fork_slices(const StepCtx& c) {
    if (c.nsl > 1) {
      HIP_OK(hipEventRecord(ev_fork, stream));
      for (int i = 1; i < c.nsl; i++) HIP_OK(hipStreamWaitEvent(xstream[i], ev_fork, 0));
    }
    return 0;
  }
  Slice slice_of(const StepCtx& c, int sl) const {
    Slice x;
    x.sl = sl; x.st = sl == 0 ? stream : xstream[sl];
    x.base = rp_slice_bound(nenv, c.nsl, sl); x.cnt = rp_slice_bound(nenv, c.nsl, sl + 1) - x.base;
    x.ss = c.s;
    x.ss.env_base = x.base;
    return x;
  }

  // ... the slices join the caller's stream; the hand-overs are marked valid; the list peaks start their way back
  int join_slices(const StepCtx& c) {
    for (int i = 1; i < c.nsl; i++) { HIP_OK(hipEventRecord(ev_join[i], xstream[i])); HIP_OK(hipStreamWaitEvent(stream, ev_join[i], 0)); }
    hipLaunchKernelGGL(rp_mark_valid_kernel, dim3((nenv + 255) / 256), dim3(256), 0, stream, d_valid, c.s.active, c.reset_mask, nenv);
    if (c.mode == 0 && lean && !c.capturing && h_heavy_peak && !heavy_grid_fixed) {
      // the longest lists of this step, for the grids of a later one (the host never waits for the copy)
      HIP_OK(hipMemcpyAsync(h_heavy_peak, d_heavy_peak, sizeof(int) * (kMaxSlices + 1), hipMemcpyDeviceToHost, stream));
      HIP_OK(hipMemsetAsync(d_heavy_peak, 0, sizeof(int) * (kMaxSlices + 1), stream));
    }
    return 0;
  }

  // the position / velocity stage of substep k (-1: of the incoming state) for the envs of slice x
  void emit_pos(const StepCtx& c, const Slice& x, const RpState<T>& q, int k) {
    if (!(split_now && !deep && sizeof(T) == 8)) { launch_stage<T, 0>(variant, x.cnt, x.st, M, q, B, k, c.nsub); return; }
    // ... as front part, pooled narrow phase, back part (same results, bit for bit)
    RpStage<T> Bs = B;
    Bs.tcount_off = x.sl * RPK_NSTRIPE * RPK_NTYPE_PAD;
    Bs.split_dropped = c.capturing ? nullptr : d_heavy_peak + kMaxSlices;
    int ng = x.cnt / 2;
    ng = ng < 64 ? 64 : (ng > 2048 ? 2048 : ng);
    launch_pos_split<T>(variant, x.cnt, ng, x.st, M, q, Bs, k, c.nsub);
  }

  // order pass over slice x, from the hand-over the position stage just wrote: the cost order and / or the list of envs
  // outside the light class
  void emit_order(const StepCtx& c, const Slice& x, bool order, bool list) {
    hipLaunchKernelGGL(rp_order_kernel, dim3(RP_ORDER_CLASSES), dim3(rp_order_threads_for(x.cnt)), 0, x.st, order ? d_order : nullptr, B.hdr, c.s.active,
                       x.base, x.cnt, list ? d_heavy : nullptr, list ? d_heavy_cnt + 2 * x.sl : nullptr, list ? d_listed : nullptr);
  }

  // sensor stage: position / velocity stage of the state before the last substep + mj_rnePostConstraint
  // with the constrained qacc (S.warm) and the contact row forces of that substep's solver stage
  void emit_sensor_stage(const StepCtx& c, const Slice& x) {
    launch_stage<T, 2>(variant, x.cnt, x.st, M, sensor_state(x.ss), B, -1, c.nsub);
  }

  // Fused substeps: one launch takes every light env of the slice through all substeps, a clean-up launch the others.
  int emit_fused_slice(const StepCtx& c, const Slice& x) {
    if constexpr (sizeof(T) == 8) {
      // heaviest envs first (4096 envs are two rounds of resident waves), from the hand-over just written
      if (cost_order) emit_order(c, x, true, false);
      RpState<T> sf = heavy_state(x.ss, x.sl, c.capturing);
      if (sensors_on) { sf.qpos_prev = d_qpos_prev; sf.qvel_prev = d_qvel_prev; }
      const bool probe = c.timeit && x.sl == 0;
      if (probe) { HIP_OK(hipEventRecord(sv0[c.slot], x.st)); sv_envs[c.slot] = x.cnt * c.nsub; sv_kind[c.slot] = 1; }
      const int cgrid = c.capturing ? (x.cnt < kHeavyGrid ? x.cnt : kHeavyGrid) : heavy_grid_for(x.sl, x.cnt);
      // (round 6: with the split stage's bodies where they exist -- the one-kernel position body spills 276 registers
      // in the hull builds; RP_FUSED_SPLIT=0: the round-3 kernel)
      const bool fsplit = fused_split && split_capable && !deep && (c.capturing ? B.frames != nullptr : ensure_split_buffers());
      RpStage<T> Bf = B;
      Bf.tlist = nullptr;   // (no pooled lists: every wave runs its own env's narrow phase)
      launch_fused<T>(variant, fsplit, x.cnt, cgrid, x.st, M, sf, fsplit ? Bf : B, B, c.nsub);
      if (probe) HIP_OK(hipEventRecord(sv1[c.slot], x.st));
      if (sensors_on) emit_sensor_stage(c, x);
    }
    return 0;
  }

  // Substep k of slice x: mj_step2 (the solver stage), then mj_step1 (the position / velocity stage) of the new state --
  // dm_control's legacy order.  Two kernels per substep instead of one fused launch: each half fits in registers,
  // the hand-over (RpStage) stays in L2 / Infinity Cache.
  int emit_substep(const StepCtx& c, Slice& x, int k) {
    hipStream_t st = x.st;
    const int sl = x.sl, base = x.base, cnt = x.cnt, slot = c.slot;
    const bool probe = c.timeit && sl == 0 && k == (int)(step_calls % (unsigned)c.nsub);
    const bool sense = sensors_on && k == c.nsub - 1;
    // cost-ordered launch: heaviest envs first, from the hand-over the position stage just wrote
    // (the same pass compacts the envs outside the light class for the full-capacity solver stage)
    const bool listed = lean && d_heavy != nullptr;
    if (cost_order || listed) emit_order(c, x, cost_order, listed);
    // (RP_X_ORDER_TWICE=1: MEASUREMENT ONLY -- the order pass a second time (no list): what the pass costs the step)
    if (x_order_twice && cost_order) emit_order(c, x, true, false);
    if (sense) {  // the state this substep's forces belong to (the solver stage integrates in place)
      HIP_OK(hipMemcpyAsync(d_qpos_prev + (size_t)base * nv, S.qpos + (size_t)base * nv, sizeof(T) * (size_t)cnt * nv, hipMemcpyDeviceToDevice, st));
      HIP_OK(hipMemcpyAsync(d_qvel_prev + (size_t)base * nv, S.qvel + (size_t)base * nv, sizeof(T) * (size_t)cnt * nv, hipMemcpyDeviceToDevice, st));
    }
    if (probe) { HIP_OK(hipEventRecord(sv0[slot], st)); sv_envs[slot] = cnt; sv_kind[slot] = 0; }
    // solver stage; the build specialised for "every tree has a 4-link trunk" when it applies
    // light envs on the lean build (two waves per SIMD), the others on the full-capacity build (it skips
    // the light ones) -- side by side: the full-capacity launch goes to the slice's companion stream
    hipStream_t hs = st;
    if (lean && !c.capturing && c.plan.companion_now) {
      if (!hstream[sl]) hstream[sl] = pooled_stream(device, 4 + sl, false);
      if (hstream[sl] && !ev_hfork[sl] && (hipEventCreateWithFlags(&ev_hfork[sl], hipEventDisableTiming) != hipSuccess ||
                                           hipEventCreateWithFlags(&ev_hjoin[sl], hipEventDisableTiming) != hipSuccess)) {
        (void)hipGetLastError(); hstream[sl] = nullptr;
      }
      if (hstream[sl]) {
        hs = hstream[sl];
        HIP_OK(hipEventRecord(ev_hfork[sl], st));
        HIP_OK(hipStreamWaitEvent(hs, ev_hfork[sl], 0));
      }
    }
    RpState<T> sh = x.ss;
    int hgrid = cnt;
    bool split_step = false;
    if (listed) {
      sh = heavy_state(x.ss, sl, c.capturing);
      hgrid = c.capturing ? (cnt < kHeavyGrid ? cnt : kHeavyGrid) : (k == 0 ? (x.hgrid_step = heavy_grid_for(sl, cnt)) : x.hgrid_step);
      split_step = rp_heavy_pos_alongside(c.in, hs != st, sizeof(T) == 8, heavy_est[sl]);
      sh.heavy_keep = (split_step && !sense) ? 1 : 0;
    }
    // (RP_X_NO_HEAVY=1: MEASUREMENT ONLY -- the full-capacity launch is suppressed, envs outside the light class are
    // not stepped at all: what the launch costs a batch whose lists are empty)
    if (x_no_heavy && listed) { /* nothing */ }
    else launch_stage<T, 1>(variant, hgrid, hs, M, sh, B, k, c.nsub);
    // ... and, except at a substep the sensor stage follows, the heavy envs' position / velocity stage goes with
    // them: the slice's own position launch then skips them and no longer waits for the slowest heavy solve
    // (config 3: 0.27 ms of every 0.81 ms substep); the streams join after it, in front of the next order pass
    const bool split_pos = split_step && listed && !sense;
    if (hs != st && !split_pos) HIP_OK(hipEventRecord(ev_hjoin[sl], hs));
    if (lean) hipLaunchKernelGGL((rp_lean_solver_kernel<T>), dim3(cnt), dim3(64), 0, st, M, x.ss, B);
    if (hs != st && !split_pos) HIP_OK(hipStreamWaitEvent(st, ev_hjoin[sl], 0));
    if (probe) HIP_OK(hipEventRecord(sv1[slot], st));
    if (sense) emit_sensor_stage(c, x);   // (of the saved state, with the contact row forces the solver stage just stored)
    if (split_pos) {
      RpState<T> sp = sh;              // (the list; walked in list order)
      sp.order = nullptr; sp.heavy_keep = 0;
      launch_pos_listed<T>(variant, hgrid, hs, M, sp, B, k, c.nsub);
      HIP_OK(hipEventRecord(ev_hjoin[sl], hs));
      RpState<T> sm_ = x.ss;
      sm_.skip_heavy = 1;
      emit_pos(c, x, sm_, k);
      HIP_OK(hipStreamWaitEvent(st, ev_hjoin[sl], 0));
    } else {
      emit_pos(c, x, x.ss, k);
    }
    return 0;
  }

  // timers and trace copy-out
  int finish(const StepCtx& c, uint32_t* trace, size_t trace_words) {
    HIP_OK(hipGetLastError());
    if (c.mode == 0) step_calls++;
    if (c.timeit) { HIP_OK(hipEventRecord(ev1[c.slot], stream)); ev_pending[c.slot] = true; }
    if (trace && c.mode == 0)
      HIP_OK(hipMemcpyAsync(trace, d_trace, trace_words * sizeof(uint32_t), hipMemcpyDefault, stream));
    return 0;
  }

  int step(int nsub, uint32_t* trace, int mode, const uint8_t* reset_mask = nullptr) override {
    HIP_OK(hipSetDevice(device));
    if (mode == 0 && nsub <= 0) return fail("rp_step: n_substeps must be positive");
    bool snap_used = false;
    if (reset_mask) {
      // rp_step_masked: physics.reset() of the flagged envs first (same launch as rp_reset with a device mask); their
      // physics.forward() is the leading position / velocity stage below
      // -- unless the reset itself hands them the stage's results for the reset state (the reset snapshot)
      if (!is_device_ptr(reset_mask)) return fail("rp_step_masked: the reset mask must be device memory");
      snap_used = launch_reset(reset_mask, stream_capturing(), true);
    }
    StepCtx c;
    c.nsub = nsub; c.mode = mode; c.reset_mask = reset_mask;
    c.s = S;
    const size_t need = (size_t)nenv * (nsub > 0 ? nsub : 1) * 4;
    if (trace && mode == 0) {
      if (need > trace_cap) {
        if (d_trace) hipFree(d_trace);
        HIP_OK(hipMalloc((void**)&d_trace, need * sizeof(uint32_t)));
        trace_cap = need;
      }
      c.s.key_trace = d_trace;
    }
    RP_TRY(begin_timers(c));
    plan(c);
    if (cost_order && mode == 0) c.s.order = d_order;   // (initialised to the identity; refreshed by the order passes)
    // (legacy_step = False: the leading stage always runs -- it is what publishes the outputs of the incoming state,
    // which the previous step's last position stage computed but kept to itself)
    const bool lazy_now = lazy_position && legacy_step;
    c.s.stale_outputs = (!legacy_step && mode == 0) ? 1 : 0;
    c.lead_masked = (lazy_now || reset_mask) && mode == 0;
    // (the lazy mode with every hand-over known valid, the envs just reset included: no leading stage at all)
    const bool no_lead = rp_lead_skippable(snap, mode, lazy_now, c.capturing, reset_mask != nullptr, snap_used);
    if (c.lead_masked && !no_lead)
      hipLaunchKernelGGL(rp_lead_mask_kernel, dim3((nenv + 255) / 256), dim3(256), 0, stream, d_lead, c.s.active, d_valid, lazy_now ? 1 : 0, reset_mask, snap_used ? 1 : 0, nenv);
    RP_TRY(fork_slices(c));
    for (int sl = 0; sl < c.nsl; sl++) {
      Slice x = slice_of(c, sl);
      if (!no_lead) {
        // mj_step1 for the current state, in index order: d_order may date from a step with another slice
        // count (a permutation of other ranges), and every slice must write the hand-over of exactly ITS envs
        // before its solver stage reads it (the solver stage consumes the hand-over: it parks values in it)
        RpState<T> lead = x.ss;
        lead.order = nullptr;
        if (c.lead_masked) lead.active = d_lead;   // skipped for envs whose hand-over is still the one of their state
        emit_pos(c, x, lead, -1);
      }
      if (mode != 0) continue;
      // ... then n_sub x (mj_step2; mj_step1), in one launch per slice or stage by stage
      if (c.plan.fused_now && sizeof(T) == 8) { RP_TRY(emit_fused_slice(c, x)); continue; }
      for (int k = 0; k < nsub; k++) RP_TRY(emit_substep(c, x, k));
    }
    RP_TRY(join_slices(c));
    rp_snapshot_on_step_done(snap, c.s.active != nullptr, c.capturing);
    return finish(c, trace, need);
  }
};

EngineBase* E(rp_engine* e) { return reinterpret_cast<EngineBase*>(e); }

}  // namespace

extern "C" {

const char* rp_last_error(void) { return g_err.c_str(); }

int rp_create(const void* model_blob, size_t blob_bytes, int n_envs, int device_id, int precision,
              rp_engine** out) {
  if (!out) return fail("rp_create: out is null");
  *out = nullptr;
  if (!model_blob || n_envs <= 0) return fail("rp_create: bad arguments");
  if (precision != 32 && precision != 64) return fail("rp_create: precision must be 32 or 64");
  Blob b;
  if (!b.init(model_blob, blob_bytes)) return fail("rp_create: not a model blob (bad magic)");
  if (!b.has("eng_nlink")) return fail("rp_create: blob lacks engine tables (eng_*)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail("rp_create: no HIP device available (the engine has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail("rp_create: bad device id");
  HIP_OK(hipSetDevice(device_id));
  EngineBase* e = nullptr;
  try {
    if (precision == 32) { auto* p = new Engine<float>(); e = p; p->device = device_id; p->precision = 32;
      HIP_OK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking)); p->build(b, n_envs); }
    else { auto* p = new Engine<double>(); e = p; p->device = device_id; p->precision = 64;
      HIP_OK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking)); p->build(b, n_envs); }
  } catch (const std::string& s) {
    delete e;
    return fail("rp_create: " + s);
  }
  for (int i = 0; i < EngineBase::kRing; i++) {
    HIP_OK(hipEventCreate(&e->ev0[i]));
    HIP_OK(hipEventCreate(&e->ev1[i]));
    HIP_OK(hipEventCreate(&e->sv0[i]));
    HIP_OK(hipEventCreate(&e->sv1[i]));
  }
  int r = e->reset(nullptr);
  if (r) { delete e; return r; }
  *out = reinterpret_cast<rp_engine*>(e);
  return 0;
}

int rp_destroy(rp_engine* e) {
  if (!e) return fail("rp_destroy: null engine");
  delete E(e);
  return 0;
}
int rp_reset(rp_engine* e, const uint8_t* mask) { return e ? E(e)->reset(mask) : fail("null engine"); }
int rp_set(rp_engine* e, rp_field f, const void* src) { return e ? E(e)->set(f, src) : fail("null engine"); }
int rp_get(rp_engine* e, rp_field f, void* dst) { return e ? E(e)->get(f, dst) : fail("null engine"); }
int rp_step(rp_engine* e, int n_substeps, uint32_t* key_trace) {
  return e ? E(e)->step(n_substeps, key_trace, 0) : fail("null engine");
}
int rp_forward(rp_engine* e) { return e ? E(e)->step(0, nullptr, 1) : fail("null engine"); }
int rp_step_masked(rp_engine* e, int n_substeps, uint32_t* key_trace, const uint8_t* reset_mask) {
  return e ? E(e)->step(n_substeps, key_trace, 0, reset_mask) : fail("null engine");
}
int rp_set_solver_limits(rp_engine* e, int max_newton_iter, int max_ls_iter) {
  if (!e) return fail("null engine");
  E(e)->limits(max_newton_iter, max_ls_iter);
  E(e)->option_changed();
  return 0;
}
int rp_profile(rp_engine* e, long long* out, int n, int enable) {
  return e ? E(e)->profile(out, n, enable) : fail("null engine");
}
int rp_set_mpr_tolerance(rp_engine* e, double tolerance, double polytope_tolerance) {
  if (!e) return fail("null engine");
  E(e)->mpr_tolerances(tolerance, polytope_tolerance);
  E(e)->option_changed();
  return 0;
}
int rp_set_solver_tolerance(rp_engine* e, double tolerance, double ls_tolerance) {
  if (!e) return fail("null engine");
  E(e)->tolerances(tolerance, ls_tolerance);
  E(e)->option_changed();
  return 0;
}
int rp_set_lazy_position_stage(rp_engine* e, int on) {
  if (!e) return fail("null engine");
  E(e)->lazy_position = on != 0;
  E(e)->option_changed();
  return 0;
}
int rp_set_reset_snapshot(rp_engine* e, int on) {
  if (!e) return fail("null engine");
  return E(e)->reset_snapshot(on);
}
int rp_set_legacy_step(rp_engine* e, int on) {
  if (!e) return fail("null engine");
  E(e)->legacy_step = on != 0;
  E(e)->option_changed();
  E(e)->snap.legacy_step = on != 0;   // (off: the leading stage publishes every env's outputs -- no snapshot)
  return E(e)->snapshot_flag_changed();
}
int rp_set_acc_sensors(rp_engine* e, int on) { if (e) E(e)->option_changed(); return e ? E(e)->acc_sensors(on) : fail("null engine"); }
int rp_set_lean_solver(rp_engine* e, int on) { if (e) E(e)->option_changed(); return e ? E(e)->lean_solver(on) : fail("null engine"); }
int rp_set_fused_substeps(rp_engine* e, int on) { if (e) E(e)->option_changed(); return e ? E(e)->fused_substeps(on) : fail("null engine"); }
int rp_get_fused_substeps(rp_engine* e) { return e ? E(e)->fused_substeps_on() : fail("null engine"); }
int rp_set_split_position_stage(rp_engine* e, int on) { if (e) E(e)->option_changed(); return e ? E(e)->split_position(on) : fail("null engine"); }
int rp_get_split_position_stage(rp_engine* e) { return e ? E(e)->split_position_on() : fail("null engine"); }
int rp_set_stream_slices(rp_engine* e, int n) {
  if (!e) return fail("null engine");
  if (n != 0 && n != 1 && n != 2 && n != 3 && n != 4) return fail("rp_set_stream_slices: 0 (automatic), 1, 2, 3 or 4");
  E(e)->n_slices = n;
  E(e)->option_changed();
  return 0;
}
int rp_set_cost_ordered_launch(rp_engine* e, int on) {
  if (!e) return fail("null engine");
  E(e)->cost_order = on != 0;
  E(e)->option_changed();
  return 0;
}
int rp_sync(rp_engine* e) {
  if (!e) return fail("null engine");
  HIP_OK(hipSetDevice(E(e)->device));
  HIP_OK(hipStreamSynchronize(E(e)->stream));
  return 0;
}
int rp_set_stream(rp_engine* e, void* hip_stream) {
  if (!e) return fail("null engine");
  EngineBase* b = E(e);
  HIP_OK(hipSetDevice(b->device));
  HIP_OK(hipStreamSynchronize(b->stream));
  for (int i = 0; i < EngineBase::kRing; i++) b->harvest(i, true);
  if (b->own_stream && b->stream) HIP_OK(hipStreamDestroy(b->stream));
  b->stream = (hipStream_t)hip_stream;
  b->own_stream = false;
  return 0;
}
int rp_field_ptr(rp_engine* e, rp_field f, void** ptr, size_t* bytes) {
  if (!e || !ptr || !bytes) return fail("null argument");
  return E(e)->field_ptr(f, ptr, bytes);
}
int rp_get_stream(rp_engine* e, void** hip_stream) {
  if (!e || !hip_stream) return fail("null argument");
  *hip_stream = (void*)E(e)->stream;
  return 0;
}
int rp_n_envs(const rp_engine* e) { return e ? reinterpret_cast<const EngineBase*>(e)->nenv : -1; }
int rp_dim(const rp_engine* e, const char* name) {
  if (!e || !name) return -1;
  const EngineBase* b = reinterpret_cast<const EngineBase*>(e);
  if (!strcmp(name, "nv")) return b->nv;
  if (!strcmp(name, "nu")) return b->nu;
  if (!strcmp(name, "nsite")) return b->nsite;
  if (!strcmp(name, "ntree")) return b->ntree;
  if (!strcmp(name, "nkey")) return b->nkey;
  if (!strcmp(name, "nlink")) return b->nlink;
  if (!strcmp(name, "maxdepth")) return b->maxdepth;
  if (!strcmp(name, "precision")) return b->precision;
  if (!strcmp(name, "rm_rows")) return b->rm_rows;
  if (!strcmp(name, "rm_cols")) return b->rm_cols;
  // the capacities of this engine's build (RpCaps<T>): beyond them the position stage keeps the deepest contacts and
  // raises RP_WARN_CONTACT_FULL; max_dense_rows is the size of the solver's dense cross-chain block (RP_WARN_DENSE_FULL)
  const bool f32 = b->precision == 32;
  if (!strcmp(name, "max_contacts")) return f32 ? RpCaps<float>::NC : RpCaps<double>::NC;
  if (!strcmp(name, "max_entries")) return f32 ? RpCaps<float>::NE : RpCaps<double>::NE;
  if (!strcmp(name, "max_dense_rows")) return f32 ? RpCaps<float>::HMAX : RpCaps<double>::HMAX;
  return -1;
}
int rp_kernel_time(rp_engine* e, double* avg_ms, int* n_launches) {
  if (!e) return fail("null engine");
  EngineBase* b = E(e);
  HIP_OK(hipSetDevice(b->device));
  for (int i = 0; i < EngineBase::kRing; i++) b->harvest(i, true);
  if (avg_ms) *avg_ms = b->kernel_launches ? b->kernel_ms / b->kernel_launches : 0.0;
  if (n_launches) *n_launches = b->kernel_launches;
  b->kernel_ms = 0; b->kernel_launches = 0;
  return 0;
}
int rp_solver_kernel_time(rp_engine* e, double* avg_ms, int* n_launches) {
  if (!e) return fail("null engine");
  EngineBase* b = E(e);
  HIP_OK(hipSetDevice(b->device));
  // harvest without clearing the step-sequence statistics
  double km = b->kernel_ms; int kl = b->kernel_launches;
  for (int i = 0; i < EngineBase::kRing; i++) b->harvest(i, true);
  const int kd = b->solver_launches_k[1] > b->solver_launches_k[0] ? 1 : 0;
  if (avg_ms) *avg_ms = b->solver_launches_k[kd] ? b->solver_ms_k[kd] / b->solver_launches_k[kd] : 0.0;
  if (n_launches) *n_launches = b->solver_launches_k[kd];
  b->last_solver_envs = b->solver_launches_k[kd] ? b->solver_envs_k[kd] / b->solver_launches_k[kd] : 0.0;
  b->last_solver_kind = kd;
  for (int k = 0; k < 2; k++) { b->solver_ms_k[k] = 0; b->solver_launches_k[k] = 0; b->solver_envs_k[k] = 0; }
  (void)km; (void)kl;
  return 0;
}
int rp_solver_kernel_fused(rp_engine* e) { return e ? E(e)->last_solver_kind : fail("null engine"); }
int rp_solver_kernel_envs(rp_engine* e, double* avg_envs) {
  if (!e) return fail("null engine");
  if (avg_envs) *avg_envs = E(e)->last_solver_envs;
  return 0;
}

}  // extern "C"
