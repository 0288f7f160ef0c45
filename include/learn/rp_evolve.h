/* learn/rp_evolve.h — population-based training (Jaderberg et al. 2017, "Population Based Training of Neural Networks") for
 * a population of P learners whose tensors are stacked [P][...]: the members' fitness windows, the decision who copies whom
 * with the perturbation of the copied hyper-parameters, and the copy of the members' slices (C ABI, gfx950,
 * librp_evolve.so).
 *
 * Conventions are rp_critic.h's: argument blocks with struct_size, no handle, no allocation, every array is the caller's,
 * one stream, no host synchronisation, nothing read back.  Member p of a population over E = P Em envs owns the envs e with
 * e % P == p (rp_pop.h).
 *
 * 1. FOLD (rp_evolve_fold, one launch, one wave of 64 lanes per member p).
 *        lane l:   s_l = 0.0;  for j = l, l + 64, ... < Em, ascending:  s_l = s_l + done_return[p + P j]
 *        t = 0.0;  for l = 0 .. 63, ascending:  t = t + s_l
 *        fit_sum[p] = fit_sum[p] + t
 *    Every addition is a float64 addition rounded on its own.  The counts go the same way in 64-bit integers:
 *    fit_count[p] += the sum of done_count[p + P j].  done_return and done_count are read only.
 * 2. PLAN (rp_evolve_plan, one launch of one workgroup; P <= RP_EVOLVE_MAX_MEMBERS).
 *    ELIGIBLE.  c = fit_count[p];  score[p] = fit_sum[p] / (double)c (one float64 division);  p is eligible iff
 *        c >= min_episodes and score[p] is not NaN.  +inf and -inf are values like any other.  n = the eligible members.
 *    RANK, among the eligible:  rank[p] = #{q eligible: score[q] > score[p] || (score[q] == score[p] && q < p)}.
 *    ENDS.  k = min(n percent / 100, n / 2) in integer arithmetic.  Winners: rank < k.  Losers: rank >= n - k.  (2 k <= n:
 *        no member is both.)
 *    SELECTION, loser p.  x = philox(generation, p, 0, RP_EVOLVE_COUNTER; seed) (Philox4x32-10 of plan/rp_plan.h, key
 *        (seed_lo, seed_hi));  w = the winner of rank x.w[0] % k;  source[p] = w if score[w] - score[p] > min_gap (one
 *        float64 subtraction; inf - inf is NaN, which is not greater), else p.  Every member that is not a loser:
 *        source[p] = p.
 *        The counter words: 96, clear of the policy (0 .. 2), the sampler (16 .. 19), the targets (32 .. 39), the critic
 *        step (48 .. 55) and the actor step (64 .. 66, 80 .. 87): one seed serves all seven.
 *    EXPLORE, every p with source[p] != p, each operation a float32 operation rounded on its own:
 *        f = (x.w[1] & 1) ? up : down;   d = 1 - gamma[w];  e = d f;  g = 1 - e
 *        gamma[p] = fminf(fmaxf(g, gamma_lo), gamma_hi)
 *        f2 = (x.w[1] & 2) ? up : down;  t = target_entropy[w] f2
 *        target_entropy[p] = fminf(fmaxf(t, entropy_lo), entropy_hi)
 *        A winner is never written, so no thread reads what another writes.  A NULL gamma (target_entropy) leaves that
 *        quantity alone.
 *    WINDOWS.  After the decision fit_sum[p] = 0 and fit_count[p] = 0 for all P members: a new window starts.
 * 3. COPY (rp_evolve_copy).  For every field {base, slice_words} of a HOST table and every member p with s = source[p],
 *        0 <= s < P, s != p and source[s] == s:  the slice_words 4-byte words at base + 4 p slice_words bytes take the bits
 *        of those at base + 4 s slice_words.  Every other slice, and every byte outside the slices, keeps its bits.  (What
 *        rp_evolve_plan writes always has source[s] == s; a table that names one array twice is the caller's mistake.)
 *        The copy uses units of 16 bytes where the two slices' addresses agree modulo 16, of 8 where they agree modulo 8,
 *        single words otherwise: single words up to the first unit boundary, whole units from there, single words for the
 *        rest.  A stacked float64 tensor counts two words per element.
 *    LAUNCHES: ceil(n_fields / RP_EVOLVE_MAX_FIELDS), each of a grid (chunks of RP_EVOLVE_CHUNK_WORDS words of a slice,
 *        members, the launch's fields); nothing with n_fields == 0 or P == 1.  The count is returned in `launches`.
 *        `source` is read on the device: a workgroup whose member keeps itself returns at once.
 *
 * Array pointers are DEVICE pointers into caller-owned memory, except rp_evolve_copy_args.fields (HOST, copied into the
 * launches; the bases it holds are device memory).  Returns 0, or a negative code with the message in
 * rp_evolve_last_error(); a refused call launches nothing.  Refused: a struct_size mismatch, NULL pointers not marked
 * optional, P < 1, P > RP_EVOLVE_MAX_MEMBERS (plan; copy: RP_EVOLVE_MAX_COPY_MEMBERS), E < 1 or E % P != 0 (fold),
 * percent outside [0, 100], min_episodes < 1, min_gap negative or NaN, up or down not > 0, gamma_lo > gamma_hi or entropy_lo > entropy_hi (or a NaN among them),
 * n_fields < 0, a field with slice_words < 1, a NULL base or a base that is not 4-byte aligned, a slice of more than 2^35
 * words.  percent == 0, P == 1 and n_fields == 0 are accepted: plan then writes the identity, copy launches nothing.
 */
#ifndef RP_EVOLVE_H_
#define RP_EVOLVE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RP_EVOLVE_MAX_MEMBERS 256
#define RP_EVOLVE_MAX_COPY_MEMBERS 65535 /* rp_evolve_copy's P: the members are a grid dimension */
#define RP_EVOLVE_MAX_FIELDS 64    /* per launch of rp_evolve_copy */
#define RP_EVOLVE_CHUNK_WORDS 4096 /* the words of a slice one workgroup of rp_evolve_copy moves */
#define RP_EVOLVE_COUNTER 96       /* the last Philox counter word of the plan's draw */

typedef struct rp_evolve_fold_args {
  size_t struct_size;
  const double* done_return; /* [E]: the returns of the episodes that ended, summed per env */
  const int32_t* done_count; /* [E]: their number */
  double* fit_sum;           /* [P], updated in place */
  long long* fit_count;      /* [P], updated in place */
  int E, P;                  /* E % P == 0 */
  void* hip_stream;
} rp_evolve_fold_args;

int rp_evolve_fold(const rp_evolve_fold_args* args);

typedef struct rp_evolve_plan_args {
  size_t struct_size;
  double* fit_sum;         /* [P]: read, then cleared */
  long long* fit_count;    /* [P]: read, then cleared */
  int32_t* source;         /* [P], out */
  float* gamma;            /* [P], optional: explored in place */
  float* target_entropy;   /* [P], optional: explored in place */
  double min_gap;          /* >= 0 */
  long long min_episodes;  /* >= 1 */
  float up, down;          /* > 0: the two factors */
  float gamma_lo, gamma_hi;
  float entropy_lo, entropy_hi;
  uint32_t seed_lo, seed_hi, generation;
  int P;                   /* 1 .. RP_EVOLVE_MAX_MEMBERS */
  int percent;             /* 0 .. 100 */
  void* hip_stream;
} rp_evolve_plan_args;

int rp_evolve_plan(const rp_evolve_plan_args* args);

typedef struct rp_evolve_field {
  void* base;            /* a stacked array [P][slice_words words]; 4-byte aligned */
  long long slice_words; /* >= 1: the 4-byte words of one member's slice */
} rp_evolve_field;

typedef struct rp_evolve_copy_args {
  size_t struct_size;
  const rp_evolve_field* fields; /* HOST [n_fields], copied into the launches; may be NULL when n_fields == 0 */
  const int32_t* source;         /* [P] */
  int n_fields;                  /* >= 0 */
  int P;                         /* 1 .. RP_EVOLVE_MAX_COPY_MEMBERS */
  int launches;                  /* out: the launches this call enqueued */
  void* hip_stream;
} rp_evolve_copy_args;

int rp_evolve_copy(rp_evolve_copy_args* args);

/* "max_members", "max_fields", "chunk_words", "counter", "wave_size" (the lanes of fold's sum: 64); -1 otherwise */
int rp_evolve_dim(const char* name);

const char* rp_evolve_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RP_EVOLVE_H_ */
