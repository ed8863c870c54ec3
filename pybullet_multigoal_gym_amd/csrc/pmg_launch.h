/* pmg_launch.h -- host-callable launchers of the kernels in pmg_kernels.hip */
#ifndef PMG_LAUNCH_H
#define PMG_LAUNCH_H
#include <hip/hip_runtime.h>
#include "pmg_kernels.h"

hipError_t pmg_launch_plan(const pmg::EnvParams& P, const float* d_actions, hipStream_t s);
/* packed != 0 selects the fast paths: four envs per wavefront (reach, one-object tasks; pmg_packed.h) and the
 * small-contact-store list of the multi-block tasks, which runs on `side` concurrently with the full-store list */
hipError_t pmg_launch_step(const pmg::EnvParams& P, const float* d_actions, hipStream_t s, int packed, hipStream_t side,
                           hipEvent_t ev_fork, hipEvent_t ev_join, pmgx::WaveRec* trace = nullptr);   /* trace: PMG_WAVE_TRACE's records (reach, tip control) */
hipError_t pmg_launch_reset(const pmg::EnvParams& P, const unsigned char* d_mask, hipStream_t s, int done_only = 0);
hipError_t pmg_launch_sub_goal(const pmg::EnvParams& P, const unsigned char* d_mask, int level, hipStream_t s);
hipError_t pmg_launch_reward(const float* ag, const float* dg, long long B, int G, float thr, int binary, float* reward,
                             unsigned char* ok, hipStream_t s);

/* running normaliser + fused policy-input rows.  A normaliser of width D keeps on the device: totals
 * double[2 D + 1] = S | Q | n, partials double[PMG_NORM_MAX_PARTS][2 D + 1] and derived float[3 D] = mean | std | inv_std */
constexpr int PMG_NORM_MAX_PARTS = 1024;   /* partial rows of one update, whatever its batch */
constexpr int PMG_NORM_MAX_D = 256;        /* widest row (chest tasks with joint control: 115) */
constexpr int PMG_NORM_CHUNK_MIN = 64;     /* rows per workgroup of a small update; a multiple of it for a large one */
/* rows [B, D] with row_stride floats between rows; row0 = global index of row 0 (chunk boundaries sit at multiples of the
 * chunk in GLOBAL rows); S, Q, n of the unmasked rows are added to tot and der is re-derived, all behind s */
hipError_t pmg_launch_norm_update(const float* d_rows, long long row_stride, long long B, int D, long long row0,
                                  const unsigned char* d_mask, float clip_input, float eps, double* part, double* tot,
                                  float* der, hipStream_t s);
hipError_t pmg_launch_norm_derive(int D, float eps, double* tot, float* der, hipStream_t s);
/* the halves of pmg_launch_norm_update for a collective update: pmg_norm_chunk(B) = the chunk pmg_launch_norm_update cuts a
 * batch of B rows into; pmg_launch_norm_partial writes the nparts partial rows of B local rows cut at `chunk` (lead = row0 % chunk) to part;
 * pmg_launch_norm_merge adds nparts partial rows in index order onto tot and re-derives der */
long long pmg_norm_chunk(long long B);
hipError_t pmg_launch_norm_partial(const float* d_rows, long long row_stride, long long B, int D, long long chunk, long long lead, int nparts,
                                   const unsigned char* d_mask, float clip_input, double* part, hipStream_t s);
hipError_t pmg_launch_norm_merge(const double* part, int nparts, int D, float eps, double* tot, float* der, hipStream_t s);
/* out[B, Ds + Dg] = clip((clip(v) - mean) * inv_std) of state | goal rows; der_* = the derived arrays of their normalisers */
hipError_t pmg_launch_policy_input(const float* d_state, long long state_stride, int Ds, const float* d_goal, long long goal_stride,
                                   int Dg, long long B, const float* der_state, const float* der_goal, float clip_input,
                                   float clip_output, float* d_out, hipStream_t s);

/* HER minibatches from caller-owned episode rows (pmg_her_sample_device): everything both kernels need, validated
 * by the caller.  Row (e, t) of the table sits at rows + e * res + t * rts; so / ago / dgo = first column of the state kind,
 * the achieved and the desired goal in a packed row.  idx is never null when x or xn is given. */
struct PmgHer {
    const float* rows; long long res, rts;
    const float* act; long long aes, ats;
    int E, T, A, Ds, G, so, ago, dgo;
    int raw, binary;
    float thr, cin, cout;
    unsigned long long seed, counter, relabel_below;   /* relabelled iff r_2 < relabel_below = ceil(future_p * 2^32) */
    long long B;
    const float* der_state; const float* der_goal;     /* derived arrays of the two normalisers (unused when raw) */
    float* x; float* xn; float* action; float* reward; unsigned char* ok; int* idx;
};
hipError_t pmg_launch_her(const PmgHer& H, hipStream_t s);

/* actor forward + exploration (pmg_mlp_forward_device, pmg_act_env_device): the network and the outputs, validated by
 * the caller.  w[l] = [width[l + 1], width[l]] row-major, b[l] = [width[l + 1]] or null.  out: forward = [B, width[L]] rows of out_activation(z)
 * at out_stride; act = the pre-activations z (may be null), and actions [B, width[L]] contiguous = the action of global env env0 + row. */
struct PmgMlp {
    int L, width[5], out_act;
    const float* w[4]; const float* b[4];
    long long B;
    float* out; long long out_stride;
    float* actions; long long env0;
    int explore; float noise_eps;                       /* explore == 0: a = clip(out_activation(z)), no draw */
    unsigned long long seed, counter, random_below;     /* random iff r_3 < random_below = ceil(random_eps * 2^32) */
    unsigned long long key;                             /* mix(seed ^ mix(counter + GOLD)): set by the launcher */
};
/* the input rows of the act entry: state columns [so, so + Ds) and desired-goal columns [dgo, dgo + Dg) of packed rows, through
 * policy_norm with the derived arrays of the two normalisers */
struct PmgMlpEnv {
    const float* rows; long long stride;
    int so, dgo, Ds, Dg;
    const float* der_state; const float* der_goal;
    float cin, cout;
};
hipError_t pmg_launch_mlp_forward(const PmgMlp& M, const float* d_in, long long in_stride, hipStream_t s);
hipError_t pmg_launch_mlp_act(const PmgMlp& M, const PmgMlpEnv& E, hipStream_t s);

/* critic and TD target (pmg_q_device, pmg_td_target_device), validated by the caller.  q: M = the critic (width[L] == 1) with
 * out = d_q, on the rows x[r] | a[r] (x_dim | width[0] - x_dim floats).  TD target: actor.B rows of x' [B, actor.width[0]] at xs floats, the
 * critic takes actor.width[0] + actor.width[L] inputs; term, qn, na may be null; na is [B, actor.width[L]] contiguous. */
struct PmgTd {
    const float* xn; long long xs;
    const float* reward; const unsigned char* term;
    float gamma, lo, hi;
    float* y; float* qn; float* na;
};
hipError_t pmg_launch_mlp_q(const PmgMlp& M, const float* d_x, long long x_stride, int x_dim, const float* d_a, long long a_stride, hipStream_t s);
hipError_t pmg_launch_td_target(const PmgMlp& actor, const PmgMlp& critic, const PmgTd& T, hipStream_t s);
/* TD3's target (pmg_td3_target_device), validated by the caller.  T as for pmg_launch_td_target with qn = q_min; T.na is not
 * used: keep = where the smoothed action a~ [B, A] (contiguous) is written and, with a second critic, read back -- the caller's
 * d_next_action when given, else the workspace when twin, else null.  q1 / q2 may be null.  noise != 0: sigma > 0, draws from (seed, counter),
 * sample index (row_offset + row) * A + j; c = the clip of the noise (may be +inf).  critic2 is read only when twin != 0. */
struct PmgTd3 {
    PmgTd T;
    float* q1; float* q2; float* keep;
    int twin, noise;
    float sigma, c;
    unsigned long long seed, counter, row_offset;
    unsigned long long key;                             /* mix(seed ^ mix(counter + GOLD)): set by the launcher */
};
hipError_t pmg_launch_td3_target(const PmgMlp& actor, const PmgMlp& critic1, const PmgMlp& critic2, const PmgTd3& X, hipStream_t s);
/* SAC's Gaussian head (pmg_sac_sample_device, pmg_sac_act_env_device, pmg_sac_target_device), validated by the caller.  The
 * actor has width[L] = 2 A outputs: means | log standard deviations.  sample != 0: draws from (seed, counter), sample index
 * (row_offset + row) * A + j (the env entry passes its env_index_offset as row_offset).  action / noise [B, A] at as / ns floats, preact
 * [B, 2 A] at ps, logp [B]: any may be null. */
struct PmgSac {
    float ls_lo, ls_hi;
    int sample;
    unsigned long long seed, counter, row_offset;
    unsigned long long key;                             /* mix(seed ^ mix(counter + GOLD)): set by the launcher */
    float* action; long long as;
    float* logp;
    float* noise; long long ns;
    float* preact; long long ps;
};
hipError_t pmg_launch_sac_sample(const PmgMlp& M, const PmgSac& G, const float* d_in, long long in_stride, hipStream_t s);
hipError_t pmg_launch_sac_act(const PmgMlp& M, const PmgSac& G, const PmgMlpEnv& E, hipStream_t s);
/* SAC's soft target (pmg_sac_target_device), validated by the caller.  T as for pmg_launch_td3_target.  G: the head's arguments; G.action =
 * where a' [B, A] is written and read back for every critic (the caller's d_next_action, else the workspace; never null), G.as = A; G.noise
 * and G.preact are null.  d_alpha: a device scalar that replaces alpha when not null.  critic2 is read only when twin != 0. */
struct PmgSacTd {
    PmgTd T;
    PmgSac G;
    float* q1; float* q2;
    int twin;
    float alpha; const float* d_alpha;
};
hipError_t pmg_launch_sac_target(const PmgMlp& actor, const PmgMlp& critic1, const PmgMlp& critic2, const PmgSacTd& X, hipStream_t s);

/* back-propagation, Adam and Polyak (pmg_mlp_grad_device, pmg_mlp_adam_device, pmg_mlp_polyak_device), validated by the caller.
 * Rows x[r] | a[r] as pmg_launch_mlp_q takes them (a == null: raw rows of x_dim = width[0] floats).  dw / db: the gradient tensors, used iff
 * grads != 0 (db[l] null where the network has no bias).  wh[l], l >= 1: h_l [B, width[l]]; wd[l]: delta_l [B, width[l + 1]]: the workspace,
 * cut by pmg_grad_work_layout; both are written and read only when grads != 0. */
struct PmgGrad {
    const float* x; long long xs; int x_dim;
    const float* a; long long as; int a_dim;
    const float* gout; long long gos;
    const float* target; long long ts;
    float gscale;
    int grads;
    float* dw[4]; float* db[4];
    float* gx; long long gxs; float* ga; long long gas; float* out; long long os;
    float* wh[4]; float* wd[4];
};
/* floats of workspace for B rows of network M; with work != null also sets G.wh / G.wd */
long long pmg_grad_work_layout(const PmgMlp& M, long long B, float* work, PmgGrad* G);
hipError_t pmg_launch_mlp_grad(const PmgMlp& M, const PmgGrad& G, hipStream_t s);
/* up to eight tensors swept by one elementwise launch: tensor k owns the flat elements [end[k - 1], end[k]).  Adam: p, g, m, v;
 * Polyak: p = the target (written), g = the source */
struct PmgSegs {
    int n; long long end[8];
    float* p[8]; const float* g[8]; float* m[8]; float* v[8];
};
struct PmgAdam { float beta1, beta2, omb1, omb2, step_size, rsc2, eps; };
/* the chunked batch reduction of dW / db (pmg_mlp_grad_chunked_device), C >= 2 chunks of R rows (R even; the last chunk
 * holds the rest).  part: [C][P] floats behind the layout of pmg_grad_work_layout, P = the network's parameters, chunk c's partial of
 * every tensor in the flat order of T; pw[l] / pb[l]: where dW_l / db_l start in chunk 0's (pb[l] null without that bias); tiles =
 * pmg_grad_w_tiles(M), the 32 x 32 tiles of all dW_l; T.p: the gradient tensors the merge writes.  G.grads != 0. */
struct PmgGradChunks {
    long long R, C, P;
    int tiles;
    float* part;
    float* pw[4]; float* pb[4];
};
int pmg_grad_w_tiles(const PmgMlp& M);
hipError_t pmg_launch_mlp_grad_chunked(const PmgMlp& M, const PmgGrad& G, const PmgGradChunks& Q, const PmgSegs& T, hipStream_t s);
/* the actor's half of an update in one call (pmg_policy_grad_device), validated by the caller.  actor.B = critic.B rows of
 * G.x [B, actor.width[0]]; G carries the ACTOR's arguments as for pmg_launch_mlp_grad (out = o unclipped, grads, dw / db, wh / wd cut by
 * pmg_grad_work_layout(actor); a, gout, target, gx, ga null); X: a = clip(o) [B, A] at as, q [B], ga = dLoss / da [B, A] at gas (any may be
 * null).  Q / T: the chunked reduction of the actor's dW / db as for pmg_launch_mlp_grad_chunked, or both null: one chain. */
struct PmgPolicy {
    float gscale, l2scale;
    float* action; long long as;
    float* q;
    float* ga; long long gas;
};
/* the behaviour-cloning term of pmg_policy_grad_bc_device, validated by the caller: rows b >= begin are demonstrations with
 * the action ad[b] (ad [B, A] at ads, indexed by the batch row; null only when begin == B); qd [B] (written from begin on) and filter [B]
 * bytes (every row) may be null.  D == null launches pmg_policy_grad_device's kernel, and so does begin == B, with the filter zeroed behind it. */
struct PmgPolicyBc {
    long long begin;
    const float* ad; long long ads;
    float bcscale;
    int q_filter;
    float* qd;
    unsigned char* filter;
};
hipError_t pmg_launch_policy_grad(const PmgMlp& actor, const PmgMlp& critic, const PmgGrad& G, const PmgPolicy& X, const PmgGradChunks* Q,
                                  const PmgSegs* T, hipStream_t s, const PmgPolicyBc* D = nullptr);
/* SAC's actor half in one call (pmg_sac_policy_grad_device), validated by the caller.  actor.B = critic.B rows of G.x
 * [B, actor.width[0]]; G carries the ACTOR's arguments as for pmg_launch_policy_grad (grads, dw / db, wh / wd; everything else null).  H: the
 * head's arguments, H.action / H.as = where a [B, A] is written and read back in front of every critic (the caller's d_action at its stride,
 * else the workspace at A; never null), H.logp may be null, H.noise and H.preact are null.  stash / ss: two floats per (row, unit) between the
 * head and the hand-back -- the actor's delta_{L-1} slot (ss = 2 A) with grads, else ghead at ghs; null when neither is given.  ga1 [B, A]
 * contiguous: critic 1's ga while critic 2 owns the tile (twin and a backward only).  d_alpha: a device scalar that replaces alpha when not
 * null.  critic2 is read only when twin != 0.  Q / T: the chunked reduction as for pmg_launch_policy_grad. */
struct PmgSacPolicy {
    PmgSac H;
    float gscale, lscale, alpha; const float* d_alpha;
    int twin;
    float* q1; float* q2;
    float* ga; long long gas;
    float* ghead; long long ghs;
    float* stash; long long ss;
    float* ga1;
};
hipError_t pmg_launch_sac_policy_grad(const PmgMlp& actor, const PmgMlp& critic1, const PmgMlp& critic2, const PmgGrad& G, const PmgSacPolicy& X,
                                      const PmgGradChunks* Q, const PmgSegs* T, hipStream_t s);
/* SAC's temperature step (pmg_sac_alpha_device), validated by the caller: state = log_alpha | m | v | alpha */
struct PmgSacAlpha {
    const float* logp; long long B;
    float target_entropy;
    PmgAdam A;
    float* state;
};
hipError_t pmg_launch_sac_alpha(const PmgSacAlpha& X, hipStream_t s);
/* PPO on whole rollouts (pmg_gae_device, pmg_adv_stats_device, pmg_adv_apply_device, pmg_ppo_policy_grad_device, pmg_ppo_stats_device; DESIGN.md
 * 3.19), validated by the caller.  A table of GAE: element (t, i) at p + t * ts + i * es floats; cut, term and ret may be null. */
struct PmgGaeTable { const float* p; long long ts, es; };
struct PmgGae {
    long long T, N;
    float gamma, gl;                                    /* gl = gamma * lambda, formed by the caller */
    PmgGaeTable reward, value, value_next, cut, term;
    float* adv; long long ats, aes;
    float* ret; long long rts, res;
};
hipError_t pmg_launch_gae(const PmgGae& X, hipStream_t s);
/* the advantage normaliser over M >= 1 contiguous floats: stats = mean | 1 / (std + eps); apply: y = (x - stats[0]) * stats[1], y may be x */
struct PmgAdvStats { const float* x; long long M; int ddof; float eps; float* stats; };
hipError_t pmg_launch_adv_stats(const PmgAdvStats& X, hipStream_t s);
hipError_t pmg_launch_adv_apply(const float* x, long long M, const float* stats, float* y, hipStream_t s);
/* the clipped-surrogate head of pmg_launch_ppo_policy_grad: zo [B, 2 A] at zos, n [B, A] at ns, adv [B]; ratio, logratio, clipped and ghead
 * (at ghs) may be null.  stash / ss: two floats per (row, unit) between the head's two passes -- the actor's delta_{L-1} slot (ss = 2 A) with
 * grads, else ghead at ghs; null when neither is given (the second pass then does not run). */
struct PmgPpoPolicy {
    float pscale, escale, clip_lo, clip_hi, ls_lo, ls_hi;
    const float* zo; long long zos;
    const float* n; long long ns;
    const float* adv;
    float* ratio; float* logratio; unsigned char* clipped;
    float* ghead; long long ghs;
    float* stash; long long ss;
};
/* actor.B rows of G.x [B, actor.width[0]]; G carries the actor's arguments as for pmg_launch_sac_policy_grad; Q / T: the chunked reduction
 * as for pmg_launch_policy_grad, or both null: one chain */
hipError_t pmg_launch_ppo_policy_grad(const PmgMlp& actor, const PmgGrad& G, const PmgPpoPolicy& X, const PmgGradChunks* Q, const PmgSegs* T, hipStream_t s);
/* the four means of a minibatch: stats = approximate KL | clip fraction | clipped surrogate | mean log-ratio; B >= 1 */
struct PmgPpoStats {
    const float* ratio; const float* logratio; const unsigned char* clipped; const float* adv; long long B;
    float clip_lo, clip_hi;
    float* stats;
};
hipError_t pmg_launch_ppo_stats(const PmgPpoStats& X, hipStream_t s);
hipError_t pmg_launch_adam(const PmgSegs& T, const PmgAdam& A, hipStream_t s);
hipError_t pmg_launch_polyak(const PmgSegs& T, float tau, hipStream_t s);
/* the data-parallel merge (pmg_mlp_params_pack_device, pmg_mlp_params_merge_device, pmg_mlp_adam_merge_device), validated by
 * the caller.  flat / a slot: the tensors of T in its flat order, T.end[T.n - 1] floats.  pack: T.g -> flat.  merge: the nslots >= 1 slots at
 * slots + r * stride added in ascending r -> T.p.  adam_merge: the same sum as the gradient of pmg_launch_adam's step on T.p / T.m / T.v;
 * keep != 0: the sum is also written to the tensors T.g names. */
hipError_t pmg_launch_params_pack(const PmgSegs& T, float* flat, hipStream_t s);
hipError_t pmg_launch_params_merge_ranks(const PmgSegs& T, const float* slots, long long stride, int nslots, hipStream_t s);
hipError_t pmg_launch_adam_merge_ranks(const PmgSegs& T, const PmgAdam& A, const float* slots, long long stride, int nslots, int keep, hipStream_t s);
#endif
