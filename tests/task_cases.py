"""The cases of the fused task kernels' tests (include/rp_task.h), shared by test_task_reference_host.py and
test_gpu_task_kernels.py.

A case fixes the number of envs, the sizes of a synthetic "model" (nv, nu, the hand actuators, the contact slots, the
forearm geoms, the fingertip sites), the launch's options and a seed, and builds every input array: there is no scene and
no engine step, so every branch of the kernels is reached on purpose and not because a roll-out wandered into it.  The
sizes are the smallest at which the code can still go wrong: 1, 5 and 70 envs (the pre-step packs four envs per block),
hand actuators and contact slots on both sides of the 64 lanes of a wave, key addresses that are a permutation of a
longer qpos row, goal sets at and around the 5 / 10 fingertips of the assignment, and keys in both of a lane's slots.

Every floating input is a float32 number held in a float64 array, so both precisions see the same reals.  The seeds
follow the rule of the learner cases: the first from 0 for which a second float32 restatement, summing every per-env
reduction in a permuted order, stays within 4 times the first one's error in every output (`first_seed`);
test_task_reference_host.py asserts that rule and that no discrete output sits near its switch.
"""

from __future__ import annotations

import functools

import numpy as np

import task_reference as tr

KEY_CLOSE, FINGER_CLOSE, ENERGY_COEF = 0.05, 0.01, 5e-3
KEY_THRESHOLD, SUSTAIN_THRESHOLD = 0.00872665, 0.5
POISON = -777.0          # every floating output buffer is pre-filled with it
IPOISON = -7             # and the integer ones
N_SITES = 14
RFA, LFA = (7, 30, 31), (12, 40, 41)      # forearm geom ids; every other geom id used is >= 50
WARN_COUNT_MASK = 8 | 2

r32 = lambda x: np.asarray(x, np.float32).astype(np.float64)

PER_ENV = ("qpos", "act_force", "act_vel", "site_xpos", "contact_geoms", "goal_current", "key_norm_state", "key_activation",
           "sustain_activation", "finger_current")

# ---- the synthetic model ------------------------------------------------------------------------------------------------
HANDS = ((3, 3, False), (70, 70, False), (90, 70, True))     # (nu, n_hand_act, scattered)


def make_model(rng, nv, hands, n_rfa, n_lfa, hand_filter):
    nu, nha, scattered = hands
    adr = rng.permutation(nv)[:88]
    if adr[0] == 0:
        adr[[0, 1]] = adr[[1, 0]]
    hi = r32(rng.uniform(0.06, 0.08, 88))
    # a third of the keys can be pushed far below zero: normalised states at which a float32 exp underflows
    lo = r32(np.where(np.arange(88) % 3 == 1, -hi * rng.uniform(3.5, 4.5, 88), -rng.uniform(0.001, 0.01, 88)))
    k = np.arange(88)
    anchor = np.stack([rng.uniform(0.35, 0.45, 88), -0.6 + 0.0137 * k + rng.uniform(-0.002, 0.002, 88), rng.uniform(0, 0.02, 88)], -1)
    half = np.stack([rng.uniform(0.065, 0.075, 88), np.full(88, 0.011), rng.uniform(0.008, 0.012, 88)], -1)
    ntip = 5 if hand_filter else 10
    return {"key_qadr": adr.astype(np.int64), "key_qrange": np.stack([lo, hi], -1), "key_anchor": r32(anchor), "key_half": r32(half),
            "hand_act": (rng.permutation(nu)[:nha] if scattered else np.arange(nha)).astype(np.int64),
            "tip_site": rng.permutation(N_SITES)[:ntip].astype(np.int64), "rfa": np.asarray(RFA[:n_rfa], np.int64),
            "lfa": np.asarray(LFA[:n_lfa], np.int64), "hand_filter": hand_filter, "energy_coef": ENERGY_COEF,
            "key_close": KEY_CLOSE, "finger_close": FINGER_CLOSE, "nv": nv, "nu": nu}


GOAL_KINDS = ((), (0,), (63,), (64,), (87,), 4, 5, 6, 9, 10, 11, 88)     # per env: named keys, or that many drawn keys


def goal_keys(rng, kind, low=0):
    kind = GOAL_KINDS[kind % len(GOAL_KINDS)]
    if isinstance(kind, tuple):
        return np.asarray([k for k in kind if k >= low], np.int64)
    return np.sort(low + rng.choice(88 - low, min(kind, 88 - low), replace=False))


def contacts(rng, md, kind, n_contacts):
    """One env's contact slots.  kinds: 0 all empty; 1 an (r, l) pair; 2 an (l, r) pair; 3 a pair in the last slot only;
    4 a right-right pair; 5 a forearm geom against another geom; 6 other geoms and empty slots; 7 the last ids of both
    lists, in a middle slot."""
    cg = np.full((n_contacts, 2), -1, np.int32)
    other = lambda n: rng.integers(50, 90, size=(n, 2))
    if kind >= 4:
        fill = rng.random(n_contacts) < 0.5
        cg[fill] = other(int(fill.sum()))
    r, l = md["rfa"], md["lfa"]
    last = n_contacts - 1
    if kind == 1:
        cg[0] = (r[0], l[0])
    elif kind == 2:
        cg[min(1, last)] = (l[0], r[0])
    elif kind == 3:
        cg[last] = (r[-1], l[0])
    elif kind == 4:
        cg[0] = (r[0], r[-1])
    elif kind == 5:
        cg[0] = (r[0], 55)
        cg[last] = (60, l[-1])
    elif kind == 7:
        cg[n_contacts // 2] = (l[-1], r[-1])
    return cg


def hits(md, cg):
    """What the header says of one env's slots, written out slot by slot."""
    return any((a in md["rfa"] and b in md["lfa"]) or (a in md["lfa"] and b in md["rfa"]) for a, b in cg.tolist())


def key_targets64(md, q):
    return tr._key_targets(q[md["key_qadr"]], md["key_anchor"], md["key_half"], np.float64)


def place_tips(rng, md, q, on_keys):
    """Site positions of one env: every fingertip near the target of a key (one to press, where there is one), at a
    distance inside the tolerance's bounds, on its Gaussian flank, or so far out that a float32 exp underflows."""
    sites = rng.uniform(-1, 1, (N_SITES, 3))
    tgt = key_targets64(md, q)
    for f, s in enumerate(md["tip_site"]):
        k = on_keys[rng.integers(len(on_keys))] if len(on_keys) else rng.integers(88)
        region = rng.integers(4)
        dist = (rng.uniform(0.001, 0.008), rng.uniform(0.02, 0.08), rng.uniform(0.1, 0.3), rng.uniform(0.9, 1.2))[region]
        v = rng.normal(size=3)
        sites[s] = tgt[k] + dist * v / np.linalg.norm(v)
    return r32(sites)


def engine_arrays(rng, md, E, n_contacts, on_keys, contact_kinds, qkeys=None):
    """qpos (the key entries from `qkeys` [E][88] when given), actuator sensors, sites and contacts of E envs."""
    nv, nu = md["nv"], md["nu"]
    qpos = r32(rng.uniform(-0.1, 0.1, (E, nv)))
    if qkeys is not None:
        qpos[:, md["key_qadr"]] = qkeys
    return {"qpos": qpos, "act_force": r32(rng.normal(size=(E, nu))), "act_vel": r32(0.5 * rng.normal(size=(E, nu))),
            "site_xpos": np.stack([place_tips(rng, md, qpos[e], on_keys[e]) for e in range(E)]),
            "contact_geoms": np.stack([contacts(rng, md, contact_kinds[e] % 8, n_contacts) for e in range(E)])}


def model_kw(md, use_fingering, use_forearm):
    keys = ("key_qadr", "key_anchor", "key_half", "hand_act", "tip_site", "rfa", "lfa", "hand_filter", "energy_coef", "key_close",
            "finger_close")
    return {**{k: md[k] for k in keys}, "use_fingering": use_fingering, "use_forearm": use_forearm}


def errors(a, ref):
    return {k: float(np.abs(np.asarray(a[k], np.float64) - np.asarray(ref[k], np.float64)).max()) if np.size(ref[k]) else 0.0
            for k in ref}


# ---- rp_task_rewards ----------------------------------------------------------------------------------------------------
# (E, nv, hands, n_contacts, (n_rfa, n_lfa), hand_filter, use_fingering, use_forearm): every hand_filter x use_fingering x
# use_forearm, the sizes taken in turn
def _reward_cases():
    out = []
    for i, (hf, uf, ufa) in enumerate((hf, uf, ufa) for hf in (0, 1, 2) for uf in (0, 1, 2) for ufa in (0, 1)):
        out.append(((70, 5, 1)[i % 3], (89, 130)[i % 2], HANDS[(i // 3) % 3], (1, 64, 70)[(i + i // 6) % 3], ((1, 3), (3, 1))[(i // 2) % 2],
                    hf, uf, ufa))
    return tuple(out)


REWARD_CASES = _reward_cases()
# the OT term at every goal-set size: 70 envs, two hands and either single hand
OT_CASES = tuple((70, 89, HANDS[0], 1, (1, 1), hf, 2, 0) for hf in (0, 1, 2))
REWARD_SEEDS = {}     # filled below: first_seed of every case


def case_id(case):
    return "-".join("x".join(str(int(v)) for v in x) if isinstance(x, tuple) else str(x) for x in case)


class RewardProblem:
    def __init__(self, case, seed):
        E, nv, hands, nc, (nr, nl), hf, uf, ufa = case
        self.case, self.seed, self.E = case, seed, E
        shift = (REWARD_CASES + OT_CASES).index(case)
        rng = np.random.default_rng([seed, E, nv, hands[0], nc, nr, hf, uf, ufa])
        md = self.md = make_model(rng, nv, hands, nr, nl, hf)
        ntip = 5 if hf else 10
        self.on_keys = [goal_keys(rng, e + shift) for e in range(E)]
        self.contact_kinds = [(e + shift) % 8 for e in range(E)]
        eng = engine_arrays(rng, md, E, nc, self.on_keys, self.contact_kinds)
        goal = np.zeros((E, 89))
        nstate = rng.uniform(0.0, 0.9, (E, 88))
        region = rng.integers(4, size=(E, 88))
        nstate = np.where(region == 0, rng.uniform(0.96, 1.0, (E, 88)), nstate)                 # inside the bounds
        nstate = np.where(region == 3, rng.uniform(-4.5, -2.8, (E, 88)), nstate)                # float32 exp underflows
        pressed = np.zeros((E, 88), bool)
        finger = np.full((E, 88), -1, np.int64)
        stray = rng.random((E, 88)) < 0.1
        finger[stray] = rng.integers(0, ntip, int(stray.sum()))                                  # (off-goal keys: never read)
        for e, keys in enumerate(self.on_keys):
            goal[e, keys] = np.where(rng.random(len(keys)) < 0.25, 0.5, 1.0)                    # 0.5: states above the goal
            pressed[e, keys] = nstate[e, keys] > 0.95
            finger[e, keys] = np.where(rng.random(len(keys)) < 0.2, -1, rng.integers(0, ntip, len(keys)))
            if len(keys):
                finger[e, keys[0]] = -1 if e % 2 else finger[e, keys[0]]
            off = np.setdiff1d(np.arange(64, 88), keys)
            if e % 3 == 1 and len(off):
                pressed[e, off[-1]] = True              # the only false positive is a key of the second slot
            elif e % 3 == 2:
                pressed[e] |= rng.random(88) < 0.05
        goal[:, 88] = np.where(np.arange(E) % 4 == 0, np.arange(E) % 8 == 0, rng.uniform(0, 1, E))
        self.kw = {**eng, "goal_current": r32(goal), "key_norm_state": r32(nstate), "key_activation": pressed,
                   "sustain_activation": (rng.random((E, 1)) < 0.5), "finger_current": finger, **model_kw(md, uf, ufa)}

    @functools.lru_cache(maxsize=None)
    def run(self, dtype, permute=None):
        return tr.rewards(dtype, permute=permute, **self.kw)

    def ref(self):
        return self.run(np.float64)

    def err32(self):
        return errors(flat_rewards(self.run(np.float32)), flat_rewards(self.ref()))

    def err_perm(self, which):
        return errors(flat_rewards(self.run(np.float32, permute=1000 * which + self.seed)), flat_rewards(self.ref()))

    __hash__ = object.__hash__


def flat_rewards(out):
    return {**{name: out["terms"][i] for i, name in enumerate(tr.TERMS)}, "total": out["total"]}


def take(kw, rows):
    """The same launch on the envs `rows`, in that order."""
    rows = np.asarray(rows, np.int64)
    return {k: (np.ascontiguousarray(v[rows]) if k in PER_ENV else v) for k, v in kw.items()}


def conditioning(err32, err_perms):
    """The worst ratio of a permuted restatement's error to the first one's over the outputs (inf: an output on which the
    first restatement is exact and a permuted one is not)."""
    worst = 0.0
    for ep in err_perms:
        for k, e in err32.items():
            if ep[k] > 0:
                worst = max(worst, ep[k] / e if e > 0 else np.inf)
    return worst


@functools.lru_cache(maxsize=None)
def reward_problem(case, seed=None):
    return RewardProblem(case, REWARD_SEEDS[case] if seed is None else seed)


OT_MARGIN = 1e-4     # far above the float32 error of a distance, far below the spacing of the keys


def ot_margins(p):
    """Per env with keys to press: (number of keys, how far the best assignment that avoids an edge of the optimum lies
    above the optimum, the smallest over the optimum's edges)."""
    from scipy.optimize import linear_sum_assignment
    out = []
    for e, keys in enumerate(p.on_keys):
        if len(keys):
            cost = tr.ot_costs(key_targets64(p.md, p.kw["qpos"][e])[keys], p.kw["site_xpos"][e, p.kw["tip_site"]])
            r, c = linear_sum_assignment(cost)
            gaps = []
            for i, j in zip(r, c):
                alt = cost.copy()
                alt[i, j] = 1e6
                r2, c2 = linear_sum_assignment(alt)
                gaps.append(alt[r2, c2].sum() - cost[r, c].sum())
            out.append((len(keys), min(gaps)))
    return out


def first_seed(make, case, limit=50):
    """The first seed from 0 that passes the permuted-restatement rule and, where the case has the OT term, whose every
    optimum is unique by OT_MARGIN."""
    for seed in range(limit):
        p = make(case, seed)
        if conditioning(p.err32(), [p.err_perm(1), p.err_perm(2)]) <= 4 and (case[6] != 2 or all(g > OT_MARGIN for _, g in ot_margins(p))):
            return seed
    raise AssertionError(("no well conditioned seed", case))


# ---- rp_task_advance ----------------------------------------------------------------------------------------------------
# name -> the options of a chain of launches.  bank: three songs of 1, bank_len - 3 and bank_len rows ("prefetch": two
# slots per env of those lengths in turn); low: the lowest key that is ever a goal or pressed
ADVANCE_CASES = {
    "small":    dict(E=5, nv=89, hands=HANDS[0], nc=1, fa=(1, 3), hf=0, uf=1, ufa=1, L=0, wrong=0, fatal=0, deque=1, launches=12),
    "wide":     dict(E=70, nv=130, hands=HANDS[2], nc=70, fa=(3, 1), hf=0, uf=2, ufa=1, L=10, wrong=1, fatal=6, deque=3, launches=16),
    "prefetch": dict(E=5, nv=130, hands=HANDS[1], nc=64, fa=(1, 1), hf=1, uf=1, ufa=0, L=1, wrong=1, fatal=1, deque=3, launches=16,
                     prefetch=True),
    "left-ot":  dict(E=1, nv=89, hands=HANDS[1], nc=64, fa=(1, 1), hf=2, uf=2, ufa=1, L=10, wrong=0, fatal=1, deque=0, launches=14,
                     song=2),
    "left":     dict(E=5, nv=89, hands=HANDS[0], nc=70, fa=(3, 1), hf=2, uf=1, ufa=0, L=4, wrong=0, fatal=1, deque=3, launches=12),
    "high-keys": dict(E=5, nv=89, hands=HANDS[0], nc=1, fa=(1, 1), hf=0, uf=1, ufa=0, L=1, wrong=1, fatal=1, deque=3, launches=16,
                      low=64),
    "high-keys-no-termination": dict(E=5, nv=89, hands=HANDS[0], nc=1, fa=(1, 1), hf=0, uf=1, ufa=0, L=1, wrong=0, fatal=1, deque=1,
                                     launches=12, low=64),
}
BANK_LEN = 12
ADVANCE_SEEDS = {}    # filled below
BIT_KEYS = (31, 32, 63, 64, 87)     # the trajectory record's word boundaries


def key_angles(rng, md, pressed, low=0):
    """Joint angles of one env's keys: the `pressed` ones within half the threshold of their upper limit (or beyond it),
    the others released, one and a half to three thresholds short of the limit, or pushed below their lower limit."""
    lo, hi = md["key_qrange"][:, 0], md["key_qrange"][:, 1]
    region = rng.integers(4, size=88)
    q = rng.uniform(0, 0.5, 88) * hi
    q = np.where(region == 1, hi - KEY_THRESHOLD * rng.uniform(1.5, 3.0, 88), q)
    q = np.where(region == 2, lo * rng.uniform(0.2, 1.5, 88), q)
    if low:
        q[:low] = np.where(region[:low] == 1, q[:low], rng.uniform(0, 0.5, low) * hi[:low])
    down = np.where(rng.random(88) < 0.5, hi - KEY_THRESHOLD * rng.uniform(0, 0.5, 88), hi + rng.uniform(0, 0.01, 88))
    return r32(np.where(pressed, down, q))


class AdvanceProblem:
    """The inputs of a chain of launches and the float64 twin's outputs after each.  The key presses of a launch are drawn
    against the goal row the twin holds at that launch: right presses, misses, wrong presses (on key 87 alone in the
    high-key cases) and the single keys of BIT_KEYS."""

    def __init__(self, name, seed):
        c = self.c = ADVANCE_CASES[name]
        self.name, self.seed = name, seed
        E, L, hf = c["E"], c["L"], c["hf"]
        self.E, self.low = E, c.get("low", 0)
        rng = np.random.default_rng([seed, E, c["nv"], L, hf, c["deque"]])
        md = self.md = make_model(rng, c["nv"], c["hands"], *c["fa"], hf)
        nfing = 5 if hf else 10
        B = BANK_LEN
        n_songs = 2 * E if c.get("prefetch") else 3
        lens = np.asarray([(1, B - 3, B)[s % 3] for s in range(n_songs)], np.int64)
        bank = np.zeros((n_songs, B, 89))
        fbank = np.full((n_songs, B, 88), -1, np.int64)
        for s in range(n_songs):
            for t in range(B):      # (rows past the song's end hold notes too: the launch must not read them)
                keys = goal_keys(rng, s + 5 * t + seed, self.low)
                bank[s, t, keys] = 1.0
                fbank[s, t, keys] = np.where(rng.random(len(keys)) < 0.15, -1, rng.integers(0, 10, len(keys)))
                stray = rng.random(88) < 0.05
                fbank[s, t, stray & (bank[s, t, :88] == 0)] = 3
                bank[s, t, 88] = (0.0, 1.0, 0.25)[(s + t) % 3]
        song_id = np.asarray([2 * e + e % 2 for e in range(E)] if c.get("prefetch") else
                             [c.get("song", 0)] if E == 1 else [e % 3 for e in range(E)], np.int64)
        slen = lens[song_id]
        # envs at the start, one before the end, at the end and past it
        t_idx = np.asarray([(0, max(slen[e] - 2, 0), slen[e] - 1, slen[e] + 1)[e % 4] for e in range(E)], np.int64)
        gstate = np.zeros((E, L + 1, 89))
        fnext = np.full((E, 88), -1, np.int64)
        for e in range(E):
            for j in range(L + 1):
                if t_idx[e] + j < slen[e]:
                    gstate[e, j] = bank[song_id[e], t_idx[e] + j]
            if t_idx[e] >= slen[e]:
                gstate[e, 0, goal_keys(rng, e, self.low)] = 1.0      # (a stale row)
            keys = np.flatnonzero(gstate[e, 0, :88] > 0)
            fnext[e, keys] = np.where(rng.random(len(keys)) < 0.15, -1, rng.integers(0, nfing, len(keys)))
        D = c["deque"]
        width = c["nv"] + 3
        st = {
            "t_idx": t_idx, "needs_reset": np.arange(E) % 3 == 1, "discount_state": np.where(np.arange(E) % 5 == 4, 0.0, 1.0),
            "goal_state": gstate, "finger_next": fnext, "song_id": song_id,
            "fatal_count": np.arange(E, dtype=np.int64) % 3, "warn_count": np.arange(E, dtype=np.int64) % 2,
            # pure outputs: poison
            "key_state": np.full((E, 88), POISON), "key_norm_state": np.full((E, 88), POISON), "key_activation": np.ones((E, 88), bool),
            "sustain_activation": np.ones((E, 1), bool), "goal_current": np.full((E, 89), POISON),
            "finger_current": np.full((E, 88), IPOISON, np.int64), "fingering_state": np.full((E, nfing), POISON),
            "should_terminate": np.ones(E, bool), "failure_termination": np.ones(E, bool), "discount": np.full(E, POISON),
            "step_type": np.full(E, IPOISON, np.int32), "terms": np.full((5, E), POISON), "total": np.full(E, POISON),
            "traj_record": np.full((E, width), POISON),     # (the words past `width` differ per precision: added by the runner)
        }
        if D:
            # eval_count below 1 at an episode's end is what the ring's clamp is for: env 2 starts at -0.5
            st.update({"eval_sums": r32(rng.uniform(0, 2, (E, 6))), "eval_count": np.where(np.arange(E) == 2, -0.5, np.arange(E) % 3 * 1.0),
                       "eval_hist": np.full((E, D, 6), POISON), "eval_nfinished": np.arange(E, dtype=np.int64) % 4})
        if c.get("prefetch"):
            st.update({"next_ready": (np.arange(E) % 2).astype(np.uint8), "consumed": (np.arange(E) == 3).astype(np.uint8)})
        self.const = {"goal_bank": bank, "finger_bank": fbank, "song_len": lens, "key_qrange": md["key_qrange"]}
        self.options = dict(n_lookahead=L, wrong_press_termination=c["wrong"], key_threshold=KEY_THRESHOLD,
                            sustain_threshold=SUSTAIN_THRESHOLD, warn_fatal_mask=c["fatal"], warn_count_mask=WARN_COUNT_MASK,
                            eval_deque=D, **model_kw(md, c["uf"], c["ufa"]))
        self.init = st
        self.launches, self.refs = [], []
        state = self.with_words(st, np.float64)
        for n in range(c["launches"]):
            inp = self._launch_inputs(rng, n, state)
            state = self.apply_host_writes(state, inp)
            out = tr.advance(np.float64, {**state, **self.const, **inp}, **self.options)
            self.launches.append(inp)
            self.refs.append(out)
            state = {**state, **out}

    def with_words(self, st, dtype):
        """The initial state with the trajectory record of the precision's width."""
        words = 2 if dtype == np.float64 else 3
        return {**st, "traj_record": np.full((self.E, self.c["nv"] + 3 + words), POISON)}

    @staticmethod
    def apply_host_writes(state, inp):
        """What a host does between two launches in prefetch mode: raise next_ready on the envs it refilled."""
        if "next_ready" in state:
            return {**state, "next_ready": (np.asarray(state["next_ready"]) | inp["ready_set"]).astype(np.uint8)}
        return state

    def _launch_inputs(self, rng, n, state):
        E, md, c = self.E, self.md, self.c
        pressed = np.zeros((E, 88), bool)
        on_keys = []
        for e in range(E):
            keys = np.flatnonzero(np.asarray(state["goal_state"])[e, 0, :88] > 0)
            on_keys.append(keys)
            kind = (e + n) % 6
            if kind in (0, 2, 5):
                pressed[e, keys] = True
            if kind == 2 and 87 not in keys:
                pressed[e, 87 if self.low else rng.integers(self.low, 88)] = True      # a wrong press
            if kind == 3:
                pressed[e, keys[::2]] = True
            if kind == 4 and not self.low:
                pressed[e, rng.choice(88, 3, replace=False)] = True
            bit = BIT_KEYS[(e + n // 6) % 5]
            if kind == 5 and (not self.low or bit == 87 or bit in keys):
                pressed[e, bit] = True
        qkeys = np.stack([key_angles(rng, md, pressed[e], self.low) for e in range(E)])
        eng = engine_arrays(rng, md, E, c["nc"], on_keys, [(e + n) % 8 for e in range(E)], qkeys)
        sus = np.where(rng.random(E) < 0.5, rng.uniform(0.0, 0.45, E), rng.uniform(0.55, 1.0, E))
        warn = np.asarray([(0, 0, 1, 0, 2, 4, 8, 0, 6, 3, 0)[(3 * e + n) % 11] for e in range(E)], np.int32)
        inp = {**eng, "sustain_state": r32(sus).reshape(E, 1), "warn": warn}
        if c.get("prefetch"):
            inp["ready_set"] = ((np.arange(E) + n) % 3 == 0).astype(np.uint8)
        return inp

    def chain(self, dtype, permute=None):
        """The twin's chain in `dtype` on its own state; -> the outputs after every launch."""
        state = self.with_words(self.init, dtype)
        outs = []
        for n, inp in enumerate(self.launches):
            state = self.apply_host_writes(state, inp)
            out = tr.advance(dtype, {**state, **self.const, **inp}, permute=None if permute is None else permute + n, **self.options)
            outs.append(out)
            state = {**state, **out}
        return outs

    @functools.lru_cache(maxsize=None)
    def chain32(self, permute=None):
        return self.chain(np.float32, permute)

    def written(self):
        keys = tr.ADVANCE_WRITES + ("traj_record",)
        if self.c["deque"]:
            keys += tr.ADVANCE_EVAL
        if self.c.get("prefetch"):
            keys += tr.ADVANCE_PREFETCH
        return keys

    def float_keys(self):
        return ("key_state", "key_norm_state", "goal_current", "goal_state", "fingering_state", "discount_state", "discount",
                "terms", "total")

    def err32(self, permute=None):
        """Per launch: the float32 restatement's error in every floating output (the record's floats: its first nv + 3)."""
        outs = self.chain32(permute)
        w = self.c["nv"] + 3
        res = []
        for o, ref in zip(outs, self.refs):
            e = errors({k: o[k] for k in self.float_keys()}, {k: ref[k] for k in self.float_keys()})
            e["traj_record"] = float(np.abs(o["traj_record"][:, :w].astype(np.float64) - ref["traj_record"][:, :w]).max())
            res.append(e)
        return res

    def err_perm(self, which):
        return self.err32(1000 * which + self.seed)

    __hash__ = object.__hash__


@functools.lru_cache(maxsize=None)
def advance_problem(name, seed=None):
    return AdvanceProblem(name, ADVANCE_SEEDS[name] if seed is None else seed)


def first_advance_seed(name, limit=50):
    for seed in range(limit):
        p = advance_problem(name, seed)
        e32 = p.err32()
        if all(conditioning(e, [a, b]) <= 4 for e, a, b in zip(e32, p.err_perm(1), p.err_perm(2))):
            return seed
    raise AssertionError(("no well conditioned seed", name))


def edge_problem():
    """Exact edges, float64 only, every constant dyadic so that the edge is a number: |st - hi| == key_threshold counts
    as pressed (<=); goal - state == key_close is inside the tolerance's bounds (1 exactly); sustain_state ==
    sustain_threshold is on (>=); a joint exactly at lo or hi is its own clipped state.  Five envs, one key each."""
    E, nv = 5, 89
    hi, lo, thr, kclose = 0.5, -0.25, 2.0 ** -7, 2.0 ** -4
    md = make_model(np.random.default_rng(3), nv, HANDS[0], 1, 1, 0)
    md["key_qrange"] = np.tile([lo, hi], (88, 1))
    md["key_close"] = kclose
    key = (0, 63, 64, 87, 31)
    qk = np.zeros((E, 88))
    qk[0, key[0]] = hi - thr                # on the activation edge: pressed
    qk[1, key[1]] = hi * (1 - kclose)       # goal 1 - state == key_close: the term is exactly 1
    qk[2, key[2]] = hi                      # exactly at the upper limit
    qk[3, key[3]] = lo                      # exactly at the lower limit
    qk[4, key[4]] = hi - thr * (1 + 2.0 ** -40)     # the next numbers past the edge: not pressed
    gstate = np.zeros((E, 1, 89))
    for e in range(E):
        gstate[e, 0, key[e]] = 1.0
    gstate[:, 0, 88] = 1.0
    rng = np.random.default_rng(4)
    eng = engine_arrays(rng, md, E, 1, [np.asarray([k]) for k in key], [0] * E, qk)
    state = {"t_idx": np.zeros(E, np.int64), "needs_reset": np.zeros(E, bool), "discount_state": np.ones(E), "goal_state": gstate,
             "finger_next": np.full((E, 88), -1, np.int64), "song_id": np.zeros(E, np.int64), "fatal_count": np.zeros(E, np.int64),
             "warn_count": np.zeros(E, np.int64), "key_state": np.full((E, 88), POISON), "key_norm_state": np.full((E, 88), POISON),
             "key_activation": np.ones((E, 88), bool), "sustain_activation": np.zeros((E, 1), bool),
             "goal_current": np.full((E, 89), POISON), "finger_current": np.full((E, 88), IPOISON, np.int64),
             "fingering_state": np.full((E, 10), POISON), "should_terminate": np.ones(E, bool), "failure_termination": np.ones(E, bool),
             "discount": np.full(E, POISON), "step_type": np.full(E, IPOISON, np.int32), "terms": np.full((5, E), POISON),
             "total": np.full(E, POISON), "traj_record": np.full((E, nv + 5), POISON),
             "sustain_state": np.asarray([0.5, 0.5 - 2.0 ** -50, 0.5 + 2.0 ** -50, 0.5, 0.5]).reshape(E, 1), "warn": np.zeros(E, np.int32),
             "goal_bank": np.zeros((1, 4, 89)), "finger_bank": np.full((1, 4, 88), -1, np.int64), "song_len": np.asarray([4], np.int64),
             "key_qrange": md["key_qrange"], **eng}
    options = dict(n_lookahead=0, wrong_press_termination=0, key_threshold=thr, sustain_threshold=0.5, warn_fatal_mask=1,
                   warn_count_mask=0, eval_deque=0, **model_kw(md, 0, 0))
    expect = {"pressed": [True, False, True, False, False], "sustain_on": [True, False, True, True, True],
              "key_state": [hi - thr, hi * (1 - kclose), hi, lo, hi - thr * (1 + 2.0 ** -40)]}
    return md, key, state, options, expect


# ---- rp_task_prestep ----------------------------------------------------------------------------------------------------
# (E, n_action, nu, scattered hand_act, bounds, clip, action table)
PRESTEP_CASES = ((1, 1, 3, False, False, False, False), (5, 16, 15, False, True, True, False), (70, 17, 40, True, True, True, True),
                 (5, 46, 45, False, False, False, True), (70, 46, 90, True, True, False, False), (1, 17, 16, False, True, True, False))
TABLE_ROWS, TABLE_INDEX = 3, (-2, 0, 2, 7)


@functools.lru_cache(maxsize=None)
def prestep_problem(case):
    E, na, nu, scattered, bounds, clip, table = case
    rng = np.random.default_rng([11, E, na, nu])
    rows = TABLE_ROWS if table else E
    act = rng.uniform(-1.5, 1.5, (rows, na))
    special = (np.nan, np.inf, -np.inf, 1.0, -1.0, 1.0000001, -3.0)
    for i, v in enumerate(special):       # (rows 0 and 2 are stepped, row 1 is being reset)
        act[0, (3 * i + 1) % na] = v
        act[2 % rows, (5 * i + 2) % na] = v
    act[1 % rows, 0] = np.nan
    if rows > 1:
        act[2, na - 1], act[1, na - 1] = np.inf, np.nan       # (the sustain column)
    kw = {"action": r32(act), "needs_reset": np.arange(E) % 3 == 1,
          "hand_act": (rng.permutation(nu)[:na - 1] if scattered else np.arange(na - 1)).astype(np.int64),
          "ctrl": np.full((E, nu), POISON), "sustain_state": np.full((E, 1), POISON), "clip": clip}
    if bounds:
        lo = r32(rng.uniform(-1.0, 0.0, na))
        hi = r32(lo + rng.uniform(0.2, 2.0, na))
        kw.update(act_lo=lo, act_range=r32(hi - lo))
    if table:
        kw["action_table"], kw["action"] = kw["action"], None
        kw["action_index"] = np.asarray([TABLE_INDEX[e % 4] for e in range(E)], np.int64)
    return kw


# ---- rp_task_rasterize --------------------------------------------------------------------------------------------------
def _song(notes, ccs, total):
    """NoteArrays of (start, end, pitch, velocity, part) notes and (time, number, value) control changes, in file order."""
    from robopianist_amd.music.midi_file import NoteArrays
    a = NoteArrays()
    n, c = np.asarray(notes, np.float64).reshape(-1, 5), np.asarray(ccs, np.float64).reshape(-1, 3)
    a.start, a.end = n[:, 0].copy(), n[:, 1].copy()
    a.pitch, a.velocity, a.part = (n[:, i].astype(np.int64) for i in (2, 3, 4))
    a.cc_time, a.cc_num, a.cc_val = c[:, 0].copy(), c[:, 1].astype(np.int64), c[:, 2].astype(np.int64)
    a.total_time = float(total)
    return a


def raster_songs():
    notes = _song([
        (0.30, 0.30, 60, 90, 1),      # a zero-length note: it still fills one frame
        (0.00, 0.50, 64, 80, 2),      # a sounding note ...
        (0.20, 0.30, 64, 0, 7),       # ... silenced by a velocity-0 note over it
        (0.00, 0.20, 67, 70, 3),      # a key held ...
        (0.20, 0.40, 67, 70, 4),      # ... and struck again: released for the frame of the onset
        (0.10, 0.45, 21, 60, 9),      # the piano's ends: transposing drops them, transposing back does not restore them
        (0.10, 0.45, 108, 60, 0),
        (0.05, 0.25, 107, 60, -1),    # no fingering
        (0.55, 0.90, 72, 50, 5),      # runs past the end of the song
        (0.02, 0.04, 84, 1, 6),       # listed out of start order (the rasteriser's songs are sorted, stably)
        (0.00, 0.20, 67, 33, 8),      # same key and start as an earlier note: the later one in the list wins
    ], [], 0.6)
    pedal = _song([(0.0, 0.1, 50, 64, 0), (0.4, 0.5, 51, 64, 5),
                   # a key held, struck again and struck once more in the next frame: both onsets are released (the scan for
                   # repeated notes must see the frame before an onset as the notes left it, not as it rewrote it)
                   (0.0, 0.2, 70, 64, 1), (0.2, 0.25, 70, 64, 2), (0.25, 0.4, 70, 64, 3)], [
        (0.00, 64, 63),               # 63: off
        (0.10, 64, 64),               # 64: on
        (0.21, 64, 127), (0.22, 64, 0), (0.23, 64, 64), (0.235, 64, 63),       # four events in one frame: the last decides (off)
        (0.30, 7, 127),               # another controller: not the pedal
        (0.40, 64, 100),
        (0.52, 64, 0),
        (5.00, 64, 127),              # past the end of the song
    ], 0.56)
    long = _song([(0.0, 1.0, 40, 64, 2), (0.5, 1.9, 41, 64, 3)], [(0.5, 64, 127)], 2.0)
    return [notes, pedal, long]


FULL_CHAIN = (("stretch", 1.0), ("transpose", 3), ("stretch", 0.8), ("transpose", -3), ("stretch", 1.25), ("transpose", 30),
              ("transpose", -30), ("stretch", 1.1))
RASTER_SLOTS = 8
RASTER_BANK_LEN = 64
# (slot, song, ops): the slots are a permutation of the jobs' order, slot 6 is left alone, the job for slot 2 does not fit
RASTER_JOBS = ((4, 0, ()), (0, 1, ()), (7, 0, FULL_CHAIN), (2, 2, (("stretch", 4.0),)), (5, 1, (("stretch", 1.3), ("transpose", 2))),
               (1, 0, (("transpose", 2), ("transpose", -2))), (3, 2, (("stretch", 0.5),)))
RASTER_CASES = tuple((dt, nbuf) for dt in (0.05, 0.04) for nbuf in (0, 10))     # (control timestep, rows of silence in front)


def raster_kw(case):
    dt, nbuf = case
    S, B = RASTER_SLOTS, RASTER_BANK_LEN
    return dict(songs=raster_songs(), control_timestep=dt, initial_buffer_time=nbuf * dt, goal_bank=np.full((S, B, 89), POISON),
                finger_bank=np.full((S, B, 88), IPOISON, np.int64), song_len=np.full(S, IPOISON, np.int64),
                slots=[j[0] for j in RASTER_JOBS], job_songs=[j[1] for j in RASTER_JOBS], ops=[list(j[2]) for j in RASTER_JOBS])


REWARD_SEEDS.update({c: 0 for c in REWARD_CASES + OT_CASES})
REWARD_SEEDS.update({REWARD_CASES[7]: 1, REWARD_CASES[8]: 1, OT_CASES[1]: 2, OT_CASES[2]: 2})
ADVANCE_SEEDS.update({name: 0 for name in ADVANCE_CASES})
ADVANCE_SEEDS.update({"left-ot": 1, "left": 1})
