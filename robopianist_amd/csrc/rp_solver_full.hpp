// rp_solver_full.hpp -- the FULL-CAPACITY solver stage (mj_step2: actuation, Newton solve, Euler): the envs whose
// constraint system does not fit the light capacity class (rp_solver2.hpp: rpk::LeanCaps), the trunk-4 and the deep
// builds, and every env when the lean stage is off.  One env per wave; the whole system in registers and LDS
// (fp64: all 512 registers, 57 KB).  Reads the hand-over record the position stage wrote (rp_model.hpp: rpk::HDR_* ..).
#pragma once
#include "rp_model.hpp"
#include "rp_wave.hpp"
#include "rp_dense.hpp"

namespace rpk {
// ---- acceleration stage (mj_step2: constraint solver + Euler)
template <typename T, int MD>
struct Smem<T, 1, MD> : SmemShared<T> {
  T R[RPK_WAVE][MD + 1];  // tree factor rows (L), incl. key-leaf rows
  T Dg[RPK_WAVE];               // tree factor diagonal
  T xs[RPK_WAVE];               // solve staging
  T H[(RpCaps<T>::HMAX + 1) * (RpCaps<T>::HMAX + 2) / 2];  // dense block of the cross-coupled rows + rhs row
  T RM[RPK_NLX(MD)][MD + 1];   // mass-matrix rows: RM[i][e] = M[i][anc_e(i)]
  T keyvec[2][RPK_NKEYS];
  T entJ[RpCaps<T>::NE][3];            // contact Jacobian entries (see RpStage)
  int entM[RpCaps<T>::NE][2];
  T cC[RpCaps<T>::NC][6];       // per-contact 3x3 weight of the current Newton iteration
  T cv[RpCaps<T>::NC][3];       // per-contact 3-vector staging (J x, or the contact force)
  T jt[RPK_WAVE];               // J^T f staging, one value per solver row
  T actf[RPK_WAVE];
};
}  // namespace rpk

// FIXED_TL > 0 specialises the solver for trunks of exactly that many links.
template <typename T, int FIXED_TL = 0, int MD = RPK_MAXD, bool EXT = false>
__device__ __forceinline__ void rp_full_solver_body(const RpModel<T>& M, const RpState<T>& S, const RpStage<T>& B, const int env, void* ext,
                                                    const int lane) {
  using namespace rpk;
  using N = Num<T>;
  if (S.lean && B.hdr[env * HDR_N + HDR_CLASS] == 1) return;   // a light env: rp_lean_solver_kernel steps it
  const int env_active = S.active ? S.active[env] : 1;  // tested after the prologue loads are in flight
  using SM_ = Smem<T, 1, MD>;
  SM_& sm = rp_smem<SM_, EXT>(ext);
  constexpr int TC = MD > 9 ? 8 : 4;            // trunk links the chain-blocked solver holds
  constexpr int NT = TC * (TC + 1) / 2, NREC = NT + TC;  // packed trunk block / per-chain record
  // the chain records of the tree elimination live at the end of the dense block's LDS (sm.H); the
  // packed block (rows + its rhs row) may grow up to there
  constexpr int HSIZE = (RpCaps<T>::HMAX + 1) * (RpCaps<T>::HMAX + 2) / 2;
#ifdef RPK_POISON_LDS  // debug build: nothing may depend on what a previous workgroup left in LDS
  {
    unsigned* w_ = reinterpret_cast<unsigned*>(&sm);
    for (int i = threadIdx.x; i < (int)(sizeof(sm) / 4); i += 64) w_[i] = 0xFFF4DEADu;
    WSYNC();
  }
#endif
  int warn = 0;
  if (S.prof && env == 0 && lane < RPK_NPROF_STAGE) sm.prof[lane] = 0;
  long long prof_t = (long long)__builtin_readcyclecounter();
  const long long kernel_t0 = prof_t;
  const int nl = M.nlink, nk = M.nkey, nv = M.nv, nu = M.nu;
  const int HREC0 = HSIZE - M.ntree * 5 * NREC;   // first chain record in sm.H = capacity of the packed dense block
  const T h = M.timestep;

  // ------------------------------------------------------------ lane constants
  const bool isl = lane < nl;
  const int L = isl ? lane : 0;
  // one 64-byte topology record per link lane (engine_tables.py: eng_lane_topo), so that
  // the prologue is a single batch of independent loads instead of a chain of lookups
  int tp[16];
  // (the key tables are requested with the topology record: clamped indices, selected below)
  int kdof_raw[2], kact_raw[2];
  {
    const int4* rec = (const int4*)(M.lane_topo() + 16 * L);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int4 v = rec[q];
      tp[4 * q] = v.x; tp[4 * q + 1] = v.y; tp[4 * q + 2] = v.z; tp[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const int K = (lane + 64 * s) < M.nkey ? lane + 64 * s : 0;
      kdof_raw[s] = M.key_dof()[K]; kact_raw[s] = M.key_act()[K];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  RPK_LANE_CONSTANTS
  // actuator owned by this lane (hand actuators only; key actuators live with the key)
  const bool isa = lane < nu && M.act_kind()[lane < nu ? lane : 0] == 0;
  const int A = lane < nu ? lane : 0;

  // ------------------------------------------------------------------- state
  const size_t eo = (size_t)env * nv;
  T q[3], qd[3], qw[3], qapp[3];
  // (the reads stay under their predicates: the solver builds are over their register budget, and one unconditional batch
  // cost the fp32 build 22 more spilled registers)
  q[0] = isl ? S.qpos[eo + ldof] : (T)0; qd[0] = isl ? S.qvel[eo + ldof] : (T)0;
  qw[0] = isl ? S.warm[eo + ldof] : (T)0;
  qapp[0] = (isl && S.qfrc_applied) ? S.qfrc_applied[eo + ldof] : (T)0;
#pragma unroll
  for (int s = 0; s < 2; s++) {
    q[1 + s] = isk[s] ? S.qpos[eo + kdof[s]] : (T)0;
    qd[1 + s] = isk[s] ? S.qvel[eo + kdof[s]] : (T)0;
    qw[1 + s] = isk[s] ? S.warm[eo + kdof[s]] : (T)0;
    qapp[1 + s] = (isk[s] && S.qfrc_applied) ? S.qfrc_applied[eo + kdof[s]] : (T)0;
  }
  T ctrl = (lane < nu) ? S.ctrl[(size_t)env * nu + lane] : (T)0;
  if (lane < nu && M.act_ctrllimited()[A])
    ctrl = fmin(M.act_ctrlrange()[2 * A + 1], fmax(M.act_ctrlrange()[2 * A], ctrl));
  T kctrl[2] = {0, 0};
#pragma unroll
  for (int s = 0; s < 2; s++) if (isk[s] && kact[s] >= 0) {
    T c = S.ctrl[(size_t)env * nu + kact[s]];
    if (M.act_ctrllimited()[kact[s]])
      c = fmin(M.act_ctrlrange()[2 * kact[s] + 1], fmax(M.act_ctrlrange()[2 * kact[s]], c));
    kctrl[s] = c;
  }
  T time = S.time[env];
  if (env_active == 0) return;  // masked env (all loads above are speculative and harmless)

  PROF(0);
  // what the position / velocity stage left behind (read below)
  T qbias = 0, alen = 0, avel = 0;
  T Mr[MD + 1];  // this link's mass-matrix row over its ancestors (diag at [depth])
#pragma unroll
  for (int e = 0; e <= MD; e++) Mr[e] = 0;
  int sdepth = -1;  // solver-slot lanes: anchor link depth
  // Lanes are numbered in preorder (trunk chain, then the leaf chains), so the ancestor
  // of link `lk` at depth e is arithmetic: trunk base + e on the trunk, lk - (depth - e)
  // on lk's own chain.  (depth, trunk length, trunk base) of the links a lane needs:
  int sTL = 0, sTB = 0, salink = 0;          // slot lanes: anchor link of my key
  auto anc_of = [](int lk, int dl, int tl, int tb, int e) -> int { return e < tl ? tb + e : lk - (dl - e); };
  T ksin[2] = {0, 0}, kcos[2] = {1, 1};
  int ncon = 0, nkt = 0, nent = 0, maxm = 0;  // contacts, touched keys, Jacobian entries, max per contact
  // rows
  T fr_aref = 0;
  int lim_sign[3] = {0, 0, 0};
  T lim_D[3] = {0, 0, 0}, lim_aref[3] = {0, 0, 0};
  T con_aref[4] = {0, 0, 0, 0}, con_D = 0, con_mu = 0, con_n[3] = {0, 0, 0}, con_t1[3] = {0, 0, 0},
    con_t2[3] = {0, 0, 0};
  unsigned long long dirty_mask = 0;  // rows that need the dense block (uniform)
  int niter_last = 0;

  const size_t lf = (size_t)env * RPK_NLF * 64 + lane, li = (size_t)env * RPK_NLI * 64 + lane;
  // ---- what the position/velocity kernel left behind
  {
    ncon = B.hdr[env * HDR_N + HDR_NCON]; nkt = B.hdr[env * HDR_N + HDR_NKT];
    dirty_mask = ((unsigned long long)(unsigned)B.hdr[env * HDR_N + HDR_DIRTY_HI] << 32) | (unsigned)B.hdr[env * HDR_N + HDR_DIRTY_LO];
    nent = B.hdr[env * HDR_N + HDR_NENT]; maxm = B.hdr[env * HDR_N + HDR_MAXM];
    // (fields only some lanes own cross for those lanes only: fewer cache lines per env)
    qbias = LF(LF_QBIAS);
    if (lane < nu) { alen = LF(LF_ALEN); avel = LF(LF_AVEL); }
    ksin[0] = LF(LF_KSIN); kcos[0] = LF(LF_KCOS);
    if (isk[1]) { ksin[1] = LF(LF_KSIN + 1); kcos[1] = LF(LF_KCOS + 1); }
    fr_aref = LF(LF_FR_AREF);
    {
      const int ls = LI(LI_LIM_SIGN);
      lim_sign[0] = (ls & 3) - 1; lim_sign[1] = ((ls >> 2) & 3) - 1; lim_sign[2] = ((ls >> 4) & 3) - 1;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) if (lim_sign[k] != 0) { lim_D[k] = LF(LF_LIM_D + k); lim_aref[k] = LF(LF_LIM_AREF + k); }
    if (lane < ncon) {  // the contact lanes' fields: only those lanes' cache lines cross (other lanes: the defaults)
      con_D = LF(LF_CON_D); con_mu = LF(LF_CON_MU);
#pragma unroll
      for (int k = 0; k < 3; k++) { con_n[k] = LF(LF_CON_N + k); con_t1[k] = LF(LF_CON_T1 + k); con_t2[k] = LF(LF_CON_T2 + k); }
#pragma unroll
      for (int k = 0; k < 4; k++) con_aref[k] = LF(LF_CON_AREF + k);
    }
    sdepth = LI(LI_SDEPTH);
    if (isl) {
#pragma unroll
      for (int e = 0; e <= MD; e++) {
        Mr[e] = B.RM[((size_t)env * RPK_NLX(MD) + lane) * (MD + 1) + e];
        sm.RM[lane][e] = Mr[e];
      }
    }
    for (int i = lane; i < nent; i += 64) {
      const size_t e = (size_t)env * RpCaps<T>::NE + i;
      sm.entJ[i][0] = B.entJ[e * 3]; sm.entJ[i][1] = B.entJ[e * 3 + 1]; sm.entJ[i][2] = B.entJ[e * 3 + 2];
      sm.entM[i][0] = B.entM[e * 2]; sm.entM[i][1] = B.entM[e * 2 + 1];
    }
    if (lane < 16) {
      const int* sl = B.slots + (size_t)env * SLOT_N;
      sm.slotkey[lane] = (short)sl[SLOT_KEY + lane];
      sm.slotlink[lane] = (short)sl[SLOT_LINK + lane];
      sm.slotmask[lane] = ((unsigned long long)(unsigned)sl[SLOT_MASK_HI + lane] << 32) | (unsigned)sl[SLOT_MASK_LO + lane];
    }
    if (lane < RPK_NKEYS / 4) ((int*)sm.keyslot)[lane] = B.keyslot[(size_t)env * (RPK_NKEYS / 4) + lane];
    WSYNC();
    {
      const int sl_ = LI(LI_SLOT_ANCHOR);
      salink = sl_ & 255; sTL = (sl_ >> 8) & 255; sTB = (sl_ >> 16) & 255;
    }
  }
  // per-lane model constants of the dynamics (read here, where they are used, not pinned through the prologue)
  const T ldamp = isl ? fresh(M.link_damping())[L] : (T)0;
  const T lstiff = isl ? fresh(M.link_stiffness())[L] : (T)0;
  const T lsref = isl ? fresh(M.link_springref())[L] : (T)0;
  const T lfloss = isl ? fresh(M.link_floss())[L] : (T)0;
  const T lflR = isl ? fresh(M.link_fl_R())[L] : (T)1;
  const T lflD = (T)1 / lflR;
  T kM[2], kstiff[2], ksref[2], kdamp[2], kmass[2], khx[2];
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const int K = isk[s] ? kid[s] : 0;
    kM[s] = isk[s] ? fresh(M.key_M())[K] : (T)1;
    kstiff[s] = isk[s] ? fresh(M.key_stiffness())[K] : (T)0;
    ksref[s] = isk[s] ? fresh(M.key_springref())[K] : (T)0;
    kdamp[s] = isk[s] ? fresh(M.key_damping())[K] : (T)0;
    kmass[s] = isk[s] ? fresh(M.key_mass())[K] : (T)0;
    khx[s] = isk[s] ? fresh(M.key_half())[3 * K] : (T)0;
  }
  // ---- actuation [MJ: mj_fwdActuation]
  T aforce = 0;
  if (isa) {
    aforce = M.act_gain()[A] * ctrl + M.act_bias()[3 * A] + M.act_bias()[3 * A + 1] * alen +
             M.act_bias()[3 * A + 2] * avel;
    if (M.act_forcelimited()[A])
      aforce = fmin(M.act_forcerange()[2 * A + 1], fmax(M.act_forcerange()[2 * A], aforce));
    sm.actf[lane] = aforce;
    S.act_force[(size_t)env * nu + lane] = aforce;
  }
  WSYNC();
  T qfs[3], qs[3];
  {
    T qact = (isl && lact >= 0) ? lactcoef * sm.actf[lact] : (T)0;
    T qpas = -lstiff * (q[0] - lsref) - ldamp * qd[0];
    qfs[0] = isl ? (qpas - qbias + qapp[0] + qact) : (T)0;
#pragma unroll
    for (int s = 0; s < 2; s++) {
      // passive spring/damper, gravity torque m*g*(hx)*cos(q) about +y, actuator
      // (all key constants are 0 for lanes without a key: no branch needed)
      const T grav = -kmass[s] * M.gz * khx[s] * kcos[s] - kmass[s] * M.gx * khx[s] * ksin[s];
      T f = -kstiff[s] * (q[1 + s] - ksref[s]) - kdamp[s] * qd[1 + s] + grav + qapp[1 + s];
      {
        if (isk[s] && kact[s] >= 0) {
          T af = M.act_gain()[kact[s]] * kctrl[s];
          if (M.act_forcelimited()[kact[s]])
            af = fmin(M.act_forcerange()[2 * kact[s] + 1], fmax(M.act_forcerange()[2 * kact[s]], af));
          f += M.act_coef()[2 * kact[s]] * af;
          S.act_force[(size_t)env * nu + kact[s]] = af;
        }
      }
      qfs[1 + s] = f;
      qs[1 + s] = f / kM[s];
    }
  }
  PROF(1);
  // ---- hybrid tree-sparse / dense factor + solve [MJ: mj_factorM / mj_solveLD by levels].
  // Row r of the symmetric system is held by lane r as Rr[e] = A[r][anc_e(r)]
  // (diag at e = depth).  Touched keys (nslots of them, lanes nl..nl+nslots-1)
  // are extra leaves hanging under their anchor link.  Rows whose bit is clear in
  // `dm` ("clean") only couple to their ancestors and are eliminated leaf-to-root
  // with no fill-in.  The rows in `dm` ("dirty": supports of cross-chain contacts,
  // an ancestor-closed set) receive the Schur complement and are solved with a
  // small dense Cholesky.  The caller has already put the cross-contact blocks into the packed
  // block sm.H (zeroed + accumulated during the Hessian assembly); the Schur rows are added here.
  auto tree_solve = [&](T* Rr, T rhs, int nslots, unsigned long long dm) -> T {
    // trunk length of this lane's tree; a compile-time constant in the FIXED_TL build
    // (every predicate on it folds: -20 % instructions in the chain elimination)
    const int TLX = FIXED_TL > 0 ? FIXED_TL : TL;
    // Chain-blocked elimination.  Each tree is a trunk chain (<= TC links) carrying up
    // to five leaf chains (<= 5 links).  The first lane of every chain ("leader")
    // gathers its chain's rows and eliminates the clean links, deepest first, entirely
    // in registers; what that leaves on the trunk is summed per trunk row, the trunk
    // leader eliminates the clean trunk links, the dense block (if any) solves the
    // dirty rows, and the leaders back-substitute.  Same arithmetic as the level-by-
    // level L^T D L, five LDS hand-overs instead of one per tree level.
    const bool isslot = !isl && lane < nl + nslots;
    const bool dirty = (dm >> lane) & 1;
    const int mydiag = isl ? depth : sdepth + 1;
    // LDS reads below are issued unconditionally on in-bounds addresses and the value
    // is selected afterwards: a conditional read costs a branch and serialises the wait.
    T Dslot = 1;
    // ---- key leaves first (they hang under chain links): the slot lanes publish their
    // scaled rows, the link lanes fold them into their register rows
    if (nslots > 0) {
      if (isslot) {
        T Dk = (T)1;
#pragma unroll
        for (int e = 0; e <= MD; e++) if (e == mydiag) Dk = Rr[e];
        if (!dirty) {
          if (!(Dk >= RPK_MINVAL)) { Dk = RPK_MINVAL; warn |= 4; }
          Dslot = Dk;
        }
        const T inv = dirty ? (T)1 : rcp_nr(Dk);
#pragma unroll
        for (int e = 0; e <= MD; e++) if (e <= mydiag) sm.R[lane][e] = e < mydiag ? Rr[e] * inv : Rr[e];
        sm.Dg[lane] = Dk;
        sm.xs[lane] = rhs;
      }
      WSYNC();
      if (isl) {
        for (int sidx = 0; sidx < nslots; sidx++) {
          const T* Lk = sm.R[nl + sidx];
          T lrow[MD + 1];
#pragma unroll
          for (int e = 0; e <= MD; e++) lrow[e] = Lk[e];
          const T lk = Lk[depth], dk = sm.Dg[nl + sidx], xk = sm.xs[nl + sidx];
          if (((sm.slotmask[sidx] >> lane) & 1) && !((dm >> (nl + sidx)) & 1)) {
            const T t = lk * dk;
#pragma unroll
            for (int e = 0; e <= MD; e++) if (e <= depth) Rr[e] -= t * lrow[e];
            rhs -= lk * xk;
          }
        }
      }
    }
    if (isl && depth >= TLX) {
#pragma unroll
      for (int e = 0; e <= MD; e++) if (e <= depth) sm.R[lane][e] = Rr[e];
      sm.xs[lane] = rhs;
    }
    WSYNC();
    PROF(20);
    // ---- chain leaders: local variables 0..TC-1 = trunk, TC..TC+4 = my chain (depth order)
    const bool leader = isl && depth == TLX && TLX > 0;
    const int clen = chain_end - TLX;
    T Ac[5][TC + 5];   // Ac[ci][j]: chain link ci vs local variable j <= TC+ci
    T rc_[5], inv_[5];
    T dT[NT], drT[TC];  // what the eliminated links leave on the trunk block / rhs
    int mc[5];
#pragma unroll
    for (int k = 0; k < NT; k++) dT[k] = 0;
#pragma unroll
    for (int k = 0; k < TC; k++) drT[k] = 0;
    if (leader) {
#pragma unroll
      for (int ci = 0; ci < 5; ci++) {
        const bool pi = ci < clen;
        mc[ci] = pi && !((dm >> (lane + ci)) & 1);
        const T* row = sm.R[lane + ci];   // lane + ci < 64: always in bounds
        const T* rowc = row + TLX;         // chain columns start at depth TLX
        const T xr_ = sm.xs[lane + ci];
        rc_[ci] = pi ? xr_ : (T)0;
#pragma unroll
        for (int j = 0; j < TC + 5; j++) {
          if (j <= TC + ci) {
            const bool pj = j < TC ? j < TLX : (j - TC) < clen;
            const T raw = j < TC ? row[j] : rowc[j - TC];
            Ac[ci][j] = (pi && pj) ? raw : (j == TC + ci ? (T)1 : (T)0);
          }
        }
      }
#pragma unroll
      for (int ci = 4; ci >= 0; ci--) {
        const int v = TC + ci;
        T dv = Ac[ci][v];
        if (mc[ci] && !(dv >= RPK_MINVAL)) { dv = RPK_MINVAL; warn |= 4; }
        const T iv = mc[ci] ? rcp_nr(dv) : (T)0;
        inv_[ci] = iv;
        T l[TC + 4];
#pragma unroll
        for (int i = 0; i < TC + 4; i++) if (i < v) l[i] = Ac[ci][i] * iv;
        // chain rows above me
#pragma unroll
        for (int ci2 = 0; ci2 < 4; ci2++) {
          if (ci2 < ci) {
            const int i = TC + ci2;
#pragma unroll
            for (int j = 0; j < TC + 5; j++) if (j <= i) Ac[ci2][j] -= l[i] * Ac[ci][j];
            rc_[ci2] -= l[i] * rc_[ci];
          }
        }
        // trunk block
#pragma unroll
        for (int i = 0; i < TC; i++) {
#pragma unroll
          for (int j = 0; j < TC; j++) if (j <= i) dT[i * (i + 1) / 2 + j] -= l[i] * Ac[ci][j];
          drT[i] -= l[i] * rc_[ci];
        }
#pragma unroll
        for (int i = 0; i < TC + 4; i++) if (i < v && mc[ci]) Ac[ci][i] = l[i];
      }
      // rows / rhs of the links I did not eliminate go back for the dense block (the
      // LDS rows of eliminated links are dead, so every present row is stored)
#pragma unroll
      for (int ci = 0; ci < 5; ci++) {
        if (ci < clen) {
          T* row = sm.R[lane + ci];
          T* rowc = row + TLX;
#pragma unroll
          for (int j = 0; j < TC; j++) if (j < TLX) row[j] = Ac[ci][j];
#pragma unroll
          for (int j = TC; j < TC + 5; j++) if (j <= TC + ci) rowc[j - TC] = Ac[ci][j];
          sm.xs[lane + ci] = rc_[ci];
        }
      }
      // trunk deltas, one NREC-entry record per chain, at the end of the dense block's storage (the
      // block itself already holds the cross-contact terms; its capacity check leaves this room)
      T* rec = sm.H + HREC0 + (size_t)(ltree * 5 + mychain) * NREC;
#pragma unroll
      for (int k = 0; k < NT; k++) rec[k] = dT[k];
#pragma unroll
      for (int k = 0; k < TC; k++) rec[NT + k] = drT[k];
    }
    WSYNC();
    // ---- trunk rows collect the chains' contributions (fixed order: deterministic)
    if (isl && depth < TLX) {
      const int tro = depth * (depth + 1) / 2;
#pragma unroll
      for (int c = 0; c < 5; c++) {
        const T* rec = sm.H + HREC0 + (size_t)(ltree * 5 + c) * NREC;
        T dv[TC];
#pragma unroll
        for (int e = 0; e < TC; e++) dv[e] = rec[tro + e < NT ? tro + e : NT - 1];
        const T dr = rec[NT + depth];
        const bool has = (chainmask >> c) & 1;
#pragma unroll
        for (int e = 0; e < TC; e++) if (has && e <= depth) Rr[e] += dv[e];
        if (has) rhs += dr;
      }
#pragma unroll
      for (int e = 0; e < TC; e++) if (e <= depth) sm.R[lane][e] = Rr[e];
      sm.xs[lane] = rhs;
    }
    WSYNC();
    // ---- trunk leader eliminates the clean trunk links (deepest first)
    const bool tleader = isl && depth == 0;
    T At[TC][TC], rt[TC], invt[TC];
    int mt[TC];
    if (tleader) {
#pragma unroll
      for (int i = 0; i < TC; i++) {
        const bool pi = i < TLX;
        mt[i] = pi && !((dm >> (lane + i)) & 1);
        const T xin = sm.xs[lane + i];
        rt[i] = pi ? xin : (T)0;
#pragma unroll
        for (int j = 0; j < TC; j++) {
          if (j <= i) {
            const T raw = sm.R[lane + i][j];
            At[i][j] = pi ? raw : (j == i ? (T)1 : (T)0);
          }
        }
      }
#pragma unroll
      for (int v = TC - 1; v >= 0; v--) {
        T dv = At[v][v];
        if (mt[v] && !(dv >= RPK_MINVAL)) { dv = RPK_MINVAL; warn |= 4; }
        const T iv = mt[v] ? rcp_nr(dv) : (T)0;
        invt[v] = iv;
        T l[TC - 1];
#pragma unroll
        for (int i = 0; i < TC - 1; i++) if (i < v) l[i] = At[v][i] * iv;
#pragma unroll
        for (int i = 0; i < TC - 1; i++) {
          if (i < v) {
#pragma unroll
            for (int j = 0; j < TC - 1; j++) if (j <= i) At[i][j] -= l[i] * At[v][j];
            rt[i] -= l[i] * rt[v];
          }
        }
#pragma unroll
        for (int i = 0; i < TC - 1; i++) if (i < v && mt[v]) At[v][i] = l[i];
      }
#pragma unroll
      for (int i = 0; i < TC; i++) {
        if (i < TLX) {  // (rows of eliminated links are dead: store them all)
#pragma unroll
          for (int j = 0; j < TC; j++) if (j <= i) sm.R[lane + i][j] = At[i][j];
          sm.xs[lane + i] = rt[i];
        }
      }
    }
    WSYNC();
    PROF(21);
    // ---- dense block on the dirty rows (Schur complement + cross-contact terms)
    if (dm) {   // (the caller passes dm = 0 when the block would not fit: RP_WARN_DENSE_FULL)
      T x = (isl || isslot) ? sm.xs[lane] : (T)0;
      WSYNC();
      const int nD = __popcll(dm);
      auto cidx = [&](int l) -> int { return __popcll(dm & lanemask_lt(l)); };
      const int ci = cidx(lane);
      // every (row, ancestor) element has exactly one owner lane: plain read-modify-write
      if (dirty) {
        if (isl) {
          for (int e = 0; e <= depth; e++) sm.H[tri(ci, cidx(anc_at(e)))] += sm.R[lane][e];
        } else {
          sm.H[tri(ci, ci)] += sm.R[lane][mydiag];
#pragma unroll
          for (int e = 0; e < MD; e++) {
            if (e <= sdepth) {
              const int a_ = anc_of(salink, sdepth, sTL, sTB, e);
              if ((dm >> a_) & 1) sm.H[tri(ci, cidx(a_))] += sm.R[lane][e];
            }
          }
        }
      }
      WSYNC();
      PROF(22);
      PROF(23);
      // the rhs of compact row r (owned by a dirty lane) is row nD of the packed block
      if (dirty) sm.H[tri(nD, 0) + ci] = x;
      WSYNC();
      T xr = dense_factor_solve(sm.H, nD, lane, &warn);
      WSYNC();
      if (lane < nD) sm.Dg[lane] = xr;
      WSYNC();
      if (dirty) sm.xs[lane] = sm.Dg[ci];
      WSYNC();
    }
    PROF(25);
    // ---- back-substitution: trunk leader, then chain leaders, then key leaves
    if (tleader) {
      T xt[TC];
#pragma unroll
      for (int v = 0; v < TC; v++) xt[v] = sm.xs[lane + v];
#pragma unroll
      for (int v = 0; v < TC; v++) {
        T xv = rt[v] * invt[v];
#pragma unroll
        for (int i = 0; i < TC - 1; i++) if (i < v) xv -= At[v][i] * xt[i];
        xt[v] = mt[v] ? xv : (v < TLX ? xt[v] : (T)0);
        if (v < TLX) sm.xs[lane + v] = xt[v];
      }
    }
    WSYNC();
    if (leader) {
      T xl[TC + 5];
#pragma unroll
      for (int j = 0; j < TC; j++) { const T xin = sm.xs[tbase + j]; xl[j] = j < TLX ? xin : (T)0; }
#pragma unroll
      for (int ci = 0; ci < 5; ci++) xl[TC + ci] = sm.xs[lane + ci];
#pragma unroll
      for (int ci = 0; ci < 5; ci++) {
        const int v = TC + ci;
        T xv = rc_[ci] * inv_[ci];
#pragma unroll
        for (int i = 0; i < TC + 4; i++) if (i < v) xv -= Ac[ci][i] * xl[i];
        xl[v] = mc[ci] ? xv : (ci < clen ? xl[v] : (T)0);
        if (ci < clen) sm.xs[lane + ci] = xl[v];
      }
    }
    WSYNC();
    T x = isl ? sm.xs[lane] : (T)0;
    if (isslot) {
      x = sm.xs[lane];
      if (!dirty) {
        x = rhs / Dslot;
#pragma unroll
        for (int e = 0; e < MD; e++)
          if (e <= sdepth) x -= sm.R[lane][e] * sm.xs[anc_of(salink, sdepth, sTL, sTB, e)];
      }
    }
    WSYNC();
    return x;
  };
  // ---- qacc_smooth = M^-1 qfrc_smooth (M is always tree-sparse)
  {
    T Rr[MD + 1];
#pragma unroll
    for (int e = 0; e <= MD; e++) Rr[e] = Mr[e];
    qs[0] = tree_solve(Rr, qfs[0], 0, 0ull);
  }

  PROF(2);
  // ---- constraint solve [MJ: mj_solNewton]
  const int nsys = nl + nkt;
  const bool hascon = lane < ncon && con_D > 0;
  const T scale = (T)1 / (M.meaninertia * (T)(nv > 1 ? nv : 1));
  T qa[3], Ma[3], qfc[3];
  Rows<T> jar, frc;
  int fr_quad = 0, lim_act[3] = {0, 0, 0}, con_act[4] = {0, 0, 0, 0};

  // Contact terms run on "entry lanes": entry = (contact, one dof it touches) with the
  // 3-vector d(contact point velocity)/d(qvel of that dof).  Lane l of pass p owns entry
  // 64 p + l; sums over the entries of a contact / over the contacts of a dof are
  // fire-and-forget LDS adds.
  // y = J x for the rows owned by this lane (x in per-lane slot registers)
  auto mulJ = [&](const T* x, Rows<T>& out) {
    sm.vec[0][lane] = x[0];
    if (isk[0]) sm.keyvec[0][kid[0]] = x[1];
    if (isk[1]) sm.keyvec[0][kid[1]] = x[2];
    if (lane < ncon) { sm.cv[lane][0] = 0; sm.cv[lane][1] = 0; sm.cv[lane][2] = 0; }
    WSYNC();
    out.fr = x[0];
#pragma unroll
    for (int s = 0; s < 3; s++) out.lim[s] = (T)lim_sign[s] * x[s];
    for (int e0 = 0; e0 < nent; e0 += 64) {
      const int e = e0 + lane < nent ? e0 + lane : nent - 1;
      const int m0 = sm.entM[e][0];
      const int ln = RPK_EM_LANE(m0), c = RPK_EM_CON(m0);
      const T j0 = sm.entJ[e][0], j1 = sm.entJ[e][1], j2 = sm.entJ[e][2];
      const T xl = sm.vec[0][ln];
      const T xk = sm.keyvec[0][sm.slotkey[ln >= nl ? ln - nl : 0]];
      const T xv = ln < nl ? xl : xk;
      if (e0 + lane < nent) {
        lds_add(&sm.cv[c][0], j0 * xv); lds_add(&sm.cv[c][1], j1 * xv); lds_add(&sm.cv[c][2], j2 * xv);
      }
    }
    WSYNC();
    T vc[3] = {0, 0, 0};
    if (lane < ncon) { vc[0] = sm.cv[lane][0]; vc[1] = sm.cv[lane][1]; vc[2] = sm.cv[lane][2]; }
    T vn = dot3(con_n, vc), v1 = con_mu * dot3(con_t1, vc), v2 = con_mu * dot3(con_t2, vc);
    out.con[0] = vn + v1; out.con[1] = vn - v1; out.con[2] = vn + v2; out.con[3] = vn - v2;
    WSYNC();
  };
  // forces + active set from jar; returns this lane's share of the constraint cost
  auto update = [&](const Rows<T>& ja, Rows<T>& f) -> T {
    T cost = 0;
    f.fr = 0; fr_quad = 0;
    if (isl && lfloss > 0) {
      T x = ja.fr, rf = lflR * lfloss;
      if (x <= -rf) { f.fr = lfloss; cost += -(T)0.5 * rf * lfloss - lfloss * x; }
      else if (x >= rf) { f.fr = -lfloss; cost += -(T)0.5 * rf * lfloss + lfloss * x; }
      else { f.fr = -lflD * x; fr_quad = 1; cost += (T)0.5 * lflD * x * x; }
    }
#pragma unroll
    for (int s = 0; s < 3; s++) {
      f.lim[s] = 0; lim_act[s] = 0;
      if (lim_sign[s] != 0 && ja.lim[s] < 0) {
        f.lim[s] = -lim_D[s] * ja.lim[s]; lim_act[s] = 1;
        cost += (T)0.5 * lim_D[s] * ja.lim[s] * ja.lim[s];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      f.con[r] = 0; con_act[r] = 0;
      if (hascon && ja.con[r] < 0) {
        f.con[r] = -con_D * ja.con[r]; con_act[r] = 1;
        cost += (T)0.5 * con_D * ja.con[r] * ja.con[r];
      }
    }
    return cost;
  };
  // out = J^T f
  auto mulJT = [&](const Rows<T>& f, T* out) {
    out[0] = f.fr + (T)lim_sign[0] * f.lim[0];
    out[1] = (T)lim_sign[1] * f.lim[1];
    out[2] = (T)lim_sign[2] * f.lim[2];
    T fn = f.con[0] + f.con[1] + f.con[2] + f.con[3];
    T f1 = con_mu * (f.con[0] - f.con[1]), f2 = con_mu * (f.con[2] - f.con[3]);
    if (lane < ncon) {
#pragma unroll
      for (int k = 0; k < 3; k++) sm.cv[lane][k] = fn * con_n[k] + f1 * con_t1[k] + f2 * con_t2[k];
    }
    sm.jt[lane] = 0;
    WSYNC();
    for (int e0 = 0; e0 < nent; e0 += 64) {
      const int e = e0 + lane < nent ? e0 + lane : nent - 1;
      const int m0 = sm.entM[e][0];
      const int ln = RPK_EM_LANE(m0), c = RPK_EM_CON(m0);
      const T v = sm.entJ[e][0] * sm.cv[c][0] + sm.entJ[e][1] * sm.cv[c][1] + sm.entJ[e][2] * sm.cv[c][2];
      if (e0 + lane < nent) lds_add(&sm.jt[ln], v);
    }
    WSYNC();
    if (isl) out[0] += sm.jt[lane];
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const int ks = isk[s] ? sm.keyslot[kid[s]] : -1;
      const T v = sm.jt[ks >= 0 ? nl + ks : 0];
      if (ks >= 0) out[1 + s] += v;
    }
    WSYNC();
  };
  auto gauss = [&](const T* qa_, const T* Ma_) -> T {
    T g = 0;
#pragma unroll
    for (int s = 0; s < 3; s++) g += (Ma_[s] - qfs[s]) * (qa_[s] - qs[s]);
    return (T)0.5 * g;
  };
  // y = M x with the tree-sparse rows: ancestor terms from this lane's own row
  // (registers), descendant terms from the rows of the next `ndesc` lanes (preorder).
  auto mulM = [&](const T* x, T* out) {
    sm.xs[lane] = x[0];
    WSYNC();
    T y = 0;
    if (isl) {
      // (reads in flight together, terms in the old order: a predicated read per ancestor and a read pair per
      // descendant were up to 35 dependent LDS round trips for a trunk link)
      T xa_[MD + 1];
#pragma unroll
      for (int e = 0; e <= MD; e++) xa_[e] = sm.xs[e <= depth ? anc_at(e) : lane];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e <= MD; e++) { const T t_ = y + Mr[e] * xa_[e]; y = e <= depth ? t_ : y; }
      int j = 1;
      for (; j + 3 <= ndesc; j += 4) {
        T m_[4], x_[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { m_[u] = sm.RM[lane + j + u][depth]; x_[u] = sm.xs[lane + j + u]; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; u++) y += m_[u] * x_[u];
      }
      for (; j <= ndesc; j++) y += sm.RM[lane + j][depth] * sm.xs[lane + j];
    }
    out[0] = y;
    out[1] = kM[0] * x[1];
    out[2] = kM[1] * x[2];
    WSYNC();
  };
  auto sub_aref = [&](Rows<T>& r) {
    r.fr -= fr_aref;
#pragma unroll
    for (int s = 0; s < 3; s++) r.lim[s] -= lim_aref[s];
#pragma unroll
    for (int k = 0; k < 4; k++) r.con[k] -= con_aref[k];
  };

  // any constraint rows at all?  (uniform)
  int anyrow = (isl && lfloss > 0) || lim_sign[0] || lim_sign[1] || lim_sign[2] || hascon;
  anyrow = __ballot(anyrow) != 0ull;
  niter_last = 0;
  if (!anyrow) {
#pragma unroll
    for (int s = 0; s < 3; s++) { qa[s] = qs[s]; qfc[s] = 0; }
  } else {
    // warmstart [MJ: warmstart()]
    Rows<T> jtmp;
    mulJ(qs, jtmp); sub_aref(jtmp);
    T cost_smooth = wave_sum(update(jtmp, frc));
#pragma unroll
    for (int s = 0; s < 3; s++) qa[s] = qw[s];
    mulM(qa, Ma);
    mulJ(qa, jar); sub_aref(jar);
    T cost = wave_sum(update(jar, frc) + gauss(qa, Ma));
    if (cost > cost_smooth) {
#pragma unroll
      for (int s = 0; s < 3; s++) { qa[s] = qs[s]; Ma[s] = qfs[s]; }
      jar = jtmp;
      cost = wave_sum(update(jar, frc) + gauss(qa, Ma));
    }
    mulJT(frc, qfc);
    T grad[3];
#pragma unroll
    for (int s = 0; s < 3; s++) grad[s] = Ma[s] - qfs[s] - qfc[s];

    PROF(3);
    const int maxit = S.max_newton;
    for (int iter = 0; iter < maxit; iter++) {
      // ---- H = M + J^T D J on the coupled system (hand dofs + touched keys)
      // key diagonals and gradients to the solver slots
#pragma unroll
      for (int s = 0; s < 2; s++) if (isk[s]) {
        sm.keyvec[0][kid[s]] = kM[s] + (lim_act[1 + s] ? lim_D[1 + s] : (T)0);
        sm.keyvec[1][kid[s]] = grad[1 + s];
      }
      WSYNC();
      const bool isslot = !isl && lane < nsys;
      T rhs = isl ? grad[0] : (T)0, slotdiag = 0;
      if (isslot) {
        int k = sm.slotkey[lane - nl];
        slotdiag = sm.keyvec[0][k];
        rhs = sm.keyvec[1][k];
      }
      const T mydiag_add = (fr_quad ? lflD : (T)0) + (lim_act[0] ? lim_D[0] : (T)0);
      // per-contact 3x3 weight C = sum_r D_r w_r w_r^T with w = n +- mu t
      T Cm[6];  // xx yy zz xy xz yz
      {
        T Dr[4];
#pragma unroll
        for (int r = 0; r < 4; r++) Dr[r] = con_act[r] ? con_D : (T)0;
        T sn = Dr[0] + Dr[1] + Dr[2] + Dr[3];
        T a1 = con_mu * (Dr[0] - Dr[1]), a2 = con_mu * (Dr[2] - Dr[3]);
        T b1 = con_mu * con_mu * (Dr[0] + Dr[1]), b2 = con_mu * con_mu * (Dr[2] + Dr[3]);
        const int ia[6] = {0, 1, 2, 0, 0, 1}, ib[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
        for (int e = 0; e < 6; e++) {
          int a = ia[e], b = ib[e];
          Cm[e] = sn * con_n[a] * con_n[b] + a1 * (con_n[a] * con_t1[b] + con_t1[a] * con_n[b]) +
                  a2 * (con_n[a] * con_t2[b] + con_t2[a] * con_n[b]) + b1 * con_t1[a] * con_t1[b] +
                  b2 * con_t2[a] * con_t2[b];
        }
      }
      T x;
      {
        // rows: mass matrix + per-dof terms (link lanes), key diagonal (slot lanes) ...
        if (lane < ncon) {
#pragma unroll
          for (int e = 0; e < 6; e++) sm.cC[lane][e] = Cm[e];
        }
        if (isl) {
#pragma unroll
          for (int e = 0; e <= MD; e++) if (e <= depth) sm.R[lane][e] = Mr[e] + (e == depth ? mydiag_add : (T)0);
        } else if (isslot) {
#pragma unroll
          for (int e = 0; e <= MD; e++) if (e <= sdepth + 1) sm.R[lane][e] = e == sdepth + 1 ? slotdiag : (T)0;
        }
        WSYNC();
        // ... + J^T C J of every contact.  Entry lane a of contact c holds u = C_c J_a and
        // walks the entries b <= a of its contact (dofs in lane order: b is an ancestor
        // of a, or the same dof): single-chain contacts add u.J_b to row(a)[col(b)] of the
        // tree rows, cross-chain contacts to the packed dense block of the dirty rows (zeroed
        // here; tree_solve adds the Schur complement of the clean rows to it) -- one pass over
        // the entries for both destinations.
        unsigned long long dmx = dirty_mask;
        if (dmx && tri(__popcll(dmx) + 1, 0) > HREC0) { warn |= 32; dmx = 0; }  // cannot hold the block: drop cross terms
        if (dmx) {
          const int nD = __popcll(dmx);
          for (int i = lane; i < tri(nD, 0); i += 64) sm.H[i] = 0;
        }
        auto cidx = [&](int l) -> int { return __popcll(dmx & lanemask_lt(l)); };
        WSYNC();
        {
          for (int e0 = 0; e0 < nent; e0 += 64) {
            const bool valid = e0 + lane < nent;
            const int e = valid ? e0 + lane : nent - 1;
            const int m0 = sm.entM[e][0], m1 = sm.entM[e][1];
            const int ln = RPK_EM_LANE(m0), c = RPK_EM_CON(m0);
            const int base = RPK_EM_BASE(m1), rank = RPK_EM_RANK(m1);
            const T ja0 = sm.entJ[e][0], ja1 = sm.entJ[e][1], ja2 = sm.entJ[e][2];
            const T* C = sm.cC[c];
            const T C0 = C[0], C1 = C[1], C2 = C[2], C3 = C[3], C4 = C[4], C5 = C[5];
            const T u0 = C0 * ja0 + C3 * ja1 + C4 * ja2;
            const T u1 = C3 * ja0 + C1 * ja1 + C5 * ja2;
            const T u2 = C4 * ja0 + C5 * ja1 + C2 * ja2;
            const bool cross = RPK_EM_CROSS(m0) != 0;
            const bool mine = valid && (!cross || dmx != 0);
            const int cia = cross ? cidx(ln) : 0;
            for (int k0 = 0; k0 < maxm; k0 += 4) {
              // four entries per trip: the twelve LDS reads go out together
              int mb[4];
              T val[4];
#pragma unroll
              for (int u = 0; u < 4; u++) {
                const int b = base + k0 + u < nent ? base + k0 + u : nent - 1;
                mb[u] = sm.entM[b][0];
                val[u] = u0 * sm.entJ[b][0] + u1 * sm.entJ[b][1] + u2 * sm.entJ[b][2];
              }
#pragma unroll
              for (int u = 0; u < 4; u++) {
                if (mine && k0 + u <= rank) {
                  T* dst = cross ? &sm.H[tri(cia, cidx(RPK_EM_LANE(mb[u])))] : &sm.R[ln][RPK_EM_COL(mb[u])];
                  lds_add(dst, val[u]);
                }
              }
            }
          }
        }
        WSYNC();
        T Rr[MD + 1];
#pragma unroll
        for (int e = 0; e <= MD; e++) Rr[e] = sm.R[lane][e];
        WSYNC();
        PROF(4);
        x = tree_solve(Rr, rhs, nkt, dmx);
      }
      T search[3];
      search[0] = isl ? -x : (T)0;
      if (!isl && lane < nsys) sm.keyvec[0][sm.slotkey[lane - nl]] = -x;
      WSYNC();
#pragma unroll
      for (int s = 0; s < 2; s++) {
        // branch-free on purpose (selects, no divergent region around the key slots: see
        // the toolchain note in DESIGN.md); kM is 1 for lanes without a key
        const int kk = isk[s] ? kid[s] : 0;
        const int ks_ = sm.keyslot[kk];
        const T via_slot = sm.keyvec[0][kk];
        const T own = -grad[1 + s] / (kM[s] + (lim_act[1 + s] ? lim_D[1 + s] : (T)0));
        search[1 + s] = isk[s] ? (ks_ >= 0 ? via_slot : own) : (T)0;
      }
      WSYNC();
      PROF(5);
      T snorm = N::sqrt(wave_sum(search[0] * search[0] + search[1] * search[1] + search[2] * search[2]));
      if (!(snorm >= RPK_MINVAL)) break;
      T Mv[3];
      mulM(search, Mv);
      Rows<T> jv;
      mulJ(search, jv);
      T g0 = 0, g1 = 0, g2 = 0;
#pragma unroll
      for (int s = 0; s < 3; s++) {
        g0 += (Ma[s] - qfs[s]) * (qa[s] - qs[s]);
        g1 += search[s] * (Ma[s] - qfs[s]);
        g2 += search[s] * Mv[s];
      }
      g0 = (T)0.5 * wave_sum(g0); g1 = wave_sum(g1); g2 = (T)0.5 * wave_sum(g2);
      PROF(6);
      // ---- exact line search [MJ: PrimalSearch]
      // [MJ: PrimalPrepare] along the search direction every row's cost is a quadratic in alpha while
      // the row stays in one zone: q0 + alpha q1 + alpha^2 q2 with q = D (jar^2/2, jar jv, jv^2/2).
      // The coefficients are formed once per Newton iteration; an evaluation then only tests each
      // row's zone at alpha and sums the coefficients of the active rows [MJ: PrimalEval].  Rows a
      // lane does not own get zero coefficients.
      T qfr[3] = {0, 0, 0}, qfl[2] = {0, 0}, frf = -1;   // friction row: quadratic zone, linear zones (+-), zone bound R f
      if (isl && lfloss > 0) {
        frf = lflR * lfloss;
        qfr[0] = (T)0.5 * lflD * jar.fr * jar.fr; qfr[1] = lflD * jar.fr * jv.fr; qfr[2] = (T)0.5 * lflD * jv.fr * jv.fr;
        qfl[0] = -(T)0.5 * frf * lfloss; qfl[1] = lfloss * jar.fr;   // linear zones: qfl[0] -+ qfl[1], slope -+ lfloss jv
      }
      const T frs = lfloss * jv.fr;
      T qlim[3][3], qcon[4][3];
#pragma unroll
      for (int s = 0; s < 3; s++) {
        const T Dp = lim_sign[s] != 0 ? lim_D[s] : (T)0;
        qlim[s][0] = (T)0.5 * Dp * jar.lim[s] * jar.lim[s]; qlim[s][1] = Dp * jar.lim[s] * jv.lim[s];
        qlim[s][2] = (T)0.5 * Dp * jv.lim[s] * jv.lim[s];
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const T Dp = hascon ? con_D : (T)0;
        qcon[r][0] = (T)0.5 * Dp * jar.con[r] * jar.con[r]; qcon[r][1] = Dp * jar.con[r] * jv.con[r];
        qcon[r][2] = (T)0.5 * Dp * jv.con[r] * jv.con[r];
      }
      const bool any_con = ncon > 0;
      // phi(alpha) and its first two derivatives; the one-sided Newton iterations on phi' never
      // read the cost and skip that wave reduction
      auto ls_eval = [&](T alpha, T& d1, T& d2, const bool with_cost) -> T {
        T s0 = 0, s1 = 0, s2 = 0;
        {
          const T xx = jar.fr + alpha * jv.fr;
          const bool lo_ = xx <= -frf, hi_ = xx >= frf;   // (frf < 0 on lanes without the row: both true, zero coefficients)
          s0 = lo_ ? qfl[0] - qfl[1] : (hi_ ? qfl[0] + qfl[1] : qfr[0]);
          s1 = lo_ ? -frs : (hi_ ? frs : qfr[1]);
          s2 = (lo_ || hi_) ? (T)0 : qfr[2];
          if (frf < 0) { s0 = 0; s1 = 0; }
        }
#pragma unroll
        for (int s = 0; s < 3; s++) {
          const T xx = jar.lim[s] + alpha * jv.lim[s];
          if (xx < 0) { s0 += qlim[s][0]; s1 += qlim[s][1]; s2 += qlim[s][2]; }
        }
        if (any_con) {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const T xx = jar.con[r] + alpha * jv.con[r];
            if (xx < 0) { s0 += qcon[r][0]; s1 += qcon[r][1]; s2 += qcon[r][2]; }
          }
        }
        s1 = wave_sum(s1) + g1; s2 = wave_sum(s2) + g2;
        d1 = s1 + (T)2 * alpha * s2;
        d2 = (T)2 * s2;
        if (!with_cost) return (T)0;
        s0 = wave_sum(s0) + g0;
        return s0 + alpha * (s1 + alpha * s2);
      };
      T gtol = M.tolerance * M.ls_tolerance * snorm / scale;
      // phi at alpha = 0 needs no row evaluation: phi(0) is the current cost,
      // phi'(0) = grad . search, and phi''(0) = search^T H search = -phi'(0) because the
      // search direction solves H search = -grad.  The first trial point is the full
      // Newton step alpha = 1.
      // (fp64 only: in fp32 the cost carried over from the last update and the cost
      // formula of ls_eval differ by more than the improvements being compared.)
      T f0, h0, c0;
      if constexpr (sizeof(T) == 8) {
        f0 = wave_sum(grad[0] * search[0] + grad[1] * search[1] + grad[2] * search[2]);
        h0 = -f0; c0 = cost;
      } else {
        c0 = ls_eval((T)0, f0, h0, true);
      }
      // [MJ: engine_solver.c PrimalSearch, restated; the oracle's primal_search is the same
      // procedure written sequentially]  All of this is wave-uniform scalar control flow; a
      // point's cost is only reduced where the procedure reads it.  (Measured alternatives with
      // fewer inlined copies of ls_eval -- a state machine around one evaluation site, a to-do
      // list around two -- were 1 ... 4 % slower than this straight transcription.)
      struct LsPnt { T a, c, d0, d1; };
      auto ls_point = [&](T al, const bool with_cost) -> LsPnt {
        LsPnt p; p.a = al; p.c = ls_eval(al, p.d0, p.d1, with_cost); return p;
      };
      T alpha = 0;
      if (h0 > 0) {
        const int max_ls = S.max_ls;
        int evals = 2;                       // (alpha = 0 and the first Newton point)
        const LsPnt p0 = {(T)0, c0, f0, h0};
        LsPnt p1 = ls_point(-f0 / h0, true);  // always one Newton step
        if (p0.c < p1.c) p1 = p0;
        alpha = p1.a;
        if (!(N::abs(p1.d0) < gtol)) {
          const T dir = p1.d0 < 0 ? (T)1 : (T)-1;
          LsPnt p2 = p1;
          bool p2update = false, converged = false;
          while (p1.d0 * dir <= -gtol && evals < max_ls) {   // one-sided search
            p2 = p1; p2update = true;
            p1 = ls_point(p1.a - p1.d0 / p1.d1, false); evals++;
            if (N::abs(p1.d0) < gtol) { converged = true; break; }
          }
          alpha = p1.a;   // converged, or failed to bracket
          if (!converged && evals < max_ls && p2update) {     // bracketed search
            LsPnt p2next = p1;   // (its cost is never read: it is not converged, and the costs of the bracket ends are re-evaluated below)
            LsPnt p1next = ls_point(p1.a - p1.d0 / p1.d1, true); evals++;
            // [MJ: updateBracket] the candidate on p's side of the root whose slope is closest to zero
            auto update_bracket = [&](LsPnt& p, const LsPnt& ca, const LsPnt& cb, const LsPnt& cc, LsPnt& pnext) -> bool {
              bool moved = false;
              auto consider = [&](const LsPnt& c) {
                if ((p.d0 < 0 && c.d0 < 0 && p.d0 < c.d0) || (p.d0 > 0 && c.d0 > 0 && p.d0 > c.d0)) { p = c; moved = true; }
              };
              consider(ca); consider(cb); consider(cc);
              if (moved) { pnext = ls_point(p.a - p.d0 / p.d1, true); evals++; }
              return moved;
            };
            bool settled = false;
            while (evals < max_ls) {
              const LsPnt pmid = ls_point((T)0.5 * (p1.a + p2.a), true); evals++;
              const LsPnt ca = p1next, cb = p2next;   // this round's candidates: ca, cb, pmid
              T bestc = 0; bool found = false;
              if (N::abs(ca.d0) < gtol) { found = true; bestc = ca.c; alpha = ca.a; }
              if (N::abs(cb.d0) < gtol && (!found || cb.c < bestc)) { found = true; bestc = cb.c; alpha = cb.a; }
              if (N::abs(pmid.d0) < gtol && (!found || pmid.c < bestc)) { found = true; alpha = pmid.a; }
              if (found) { settled = true; break; }
              const bool b1 = update_bracket(p1, ca, cb, pmid, p1next);
              const bool b2 = update_bracket(p2, ca, cb, pmid, p2next);
              if (!b1 && !b2) { alpha = pmid.a; settled = true; break; }   // numerical accuracy reached
            }
            if (!settled) {   // evaluations exhausted: the better end of the bracket, if it beats alpha = 0
              T t1, t2;
              const T c1 = ls_eval(p1.a, t1, t2, true), c2 = ls_eval(p2.a, t1, t2, true);
              alpha = (c1 <= c2 && c1 < p0.c) ? p1.a : ((c2 <= c1 && c2 < p0.c) ? p2.a : (T)0);
            }
          }
        }
      }
      PROF(7);
      if (!(alpha > 0)) break;
#pragma unroll
      for (int s = 0; s < 3; s++) { qa[s] += alpha * search[s]; Ma[s] += alpha * Mv[s]; }
      jar.fr += alpha * jv.fr;
#pragma unroll
      for (int s = 0; s < 3; s++) jar.lim[s] += alpha * jv.lim[s];
#pragma unroll
      for (int r = 0; r < 4; r++) jar.con[r] += alpha * jv.con[r];
      T oldcost = cost;
      cost = wave_sum(update(jar, frc) + gauss(qa, Ma));
      mulJT(frc, qfc);
      niter_last = iter + 1;
      T gn = 0;
#pragma unroll
      for (int s = 0; s < 3; s++) { grad[s] = Ma[s] - qfs[s] - qfc[s]; gn += grad[s] * grad[s]; }
      gn = N::sqrt(wave_sum(gn));
      PROF(8);
      if (scale * (oldcost - cost) < M.tolerance || scale * gn < M.tolerance) break;
    }
  }
#pragma unroll
  for (int s = 0; s < 3; s++) qw[s] = qa[s];
  // forces of the pyramidal contact rows, for the acceleration-stage sensors (MODE 2)
  if (S.con_force && lane < RPK_NCOUT) {
#pragma unroll
    for (int r = 0; r < 4; r++)
      S.con_force[((size_t)env * RPK_NCOUT + lane) * 4 + r] = (anyrow && lane < ncon) ? frc.con[r] : (T)0;
  }

  PROF(8);
  // ---- Euler with implicit joint damping [MJ: mj_Euler, eulerdamp]
  T qe[3];
  {
    T Rr[MD + 1];
#pragma unroll
    for (int e = 0; e <= MD; e++) Rr[e] = Mr[e] + ((isl && e == depth) ? h * ldamp : (T)0);
    qe[0] = tree_solve(Rr, qfs[0] + qfc[0], 0, 0ull);
  }
#pragma unroll
  for (int s = 0; s < 2; s++) qe[1 + s] = (qfs[1 + s] + qfc[1 + s]) / (kM[s] + h * kdamp[s]);
#pragma unroll
  for (int s = 0; s < 3; s++) { qd[s] += h * qe[s]; q[s] += h * qd[s]; }
  time += h;
  PROF(9);
  // ---- new state
  if (isl) { S.qpos[eo + ldof] = q[0]; S.qvel[eo + ldof] = qd[0]; S.warm[eo + ldof] = qw[0]; }
#pragma unroll
  for (int s = 0; s < 2; s++) if (isk[s]) {
    S.qpos[eo + kdof[s]] = q[1 + s]; S.qvel[eo + kdof[s]] = qd[1 + s]; S.warm[eo + kdof[s]] = qw[1 + s];
  }

  PROF(17);
  // ------------------------------------------------------------------ outputs
  {
    int w = warn;
    w = wave_or(w);
    if (lane == 0) {
      S.warn[env] |= w;
      S.solver_iter[env] = (niter_last & 255) | ((__popcll(dirty_mask) & 255) << 8) | ((nkt & 255) << 16);
      S.time[env] = time;
    }
  }
  if (S.prof && env == 0 && lane < RPK_NPROF_STAGE) {
    WSYNC();
    atomicAdd((unsigned long long*)&S.prof[lane], (unsigned long long)sm.prof[lane]);
  }
  if (S.cost_sol && lane == 0) S.cost_sol[env] = (int)(((long long)__builtin_readcyclecounter() - kernel_t0) >> 8);
}
