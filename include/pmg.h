/*
 * pmg.h -- C ABI of the MI355X-native vectorised multigoal manipulation env.
 *
 * This is the drop-in boundary for the reference's per-step hot path.  The
 * reference (pure Python) crosses into native code through ~25 PyBullet C-API
 * entry points per env step; this library replaces
 * that whole inner boundary with ONE batched call per phase.  Each entry
 * point below cites the reference interface it replaces
 * (P/ = pybullet_multigoal_gym/ in the reference tree).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / numpy types.
 *   - Every function returns 0 on success, a negative PMG_E_* code otherwise;
 *     the message is available from pmg_last_error().  Nothing aborts or
 *     throws across this boundary.
 *   - The caller owns every host buffer passed in; the library owns the
 *     handle and all device memory.  Buffers named d_* are DEVICE pointers
 *     (HIP) supplied by the caller (e.g. a torch tensor's data_ptr()).
 *   - A handle is used from one host thread at a time.  Host-buffer calls
 *     are synchronous at return; *_device calls are stream-ordered on the
 *     handle's HIP stream (pmg_sync() waits for it).
 *   - All arrays are row-major with a leading num_envs axis, float32.
 */
#ifndef PMG_H
#define PMG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* tasks: P/__init__.py:14-44 ('reach','push','pick_and_place','slide','block_stack','block_rearrange','chest_push',
 * 'chest_pick_and_place') */
enum {
    PMG_TASK_REACH = 0,
    PMG_TASK_PUSH = 1,
    PMG_TASK_PICK_AND_PLACE = 2,
    PMG_TASK_SLIDE = 3,
    PMG_TASK_BLOCK_STACK = 4,
    PMG_TASK_BLOCK_REARRANGE = 5,
    PMG_TASK_CHEST_PUSH = 6,            /* KukaChestPushEnv: front sliding door (kuka_multi_step_envs.py:385-403) */
    PMG_TASK_CHEST_PICK_AND_PLACE = 7   /* KukaChestPickAndPlaceEnv: up sliding lid (:230-254) */
};

enum {
    PMG_OK = 0,
    PMG_E_INVALID = -1,     /* bad argument / unsupported configuration */
    PMG_E_DEVICE = -2,      /* HIP runtime error */
    PMG_E_NOMEM = -3,
    PMG_E_STATE = -4,       /* call order error (e.g. step before reset) */
    PMG_E_COMM = -5         /* RCCL error */
};

/* which device buffer pmg_device_ptr() returns */
enum {
    PMG_BUF_PACKED = 7,  /* [N, packed_dim] float32 rows: observation | policy_state | achieved_goal |
                            desired_goal | reward | goal_achieved (0/1) | done (0/1); widths in pmg_dims */
    PMG_BUF_STATE = 8,   /* [N, 32] float32 hot state rows (q9 qd9 ee3 jt7 grip elapsed enabled resets) */
    PMG_BUF_SCHED = 9,   /* [4 + 3N + 3 ceil(N / 1024)] int32 launch schedule of the last step (diagnostics): n_prone, n_free,
                            prone list [N], free list [N], n_redo, redo list [N], then the two-pass plan's per-workgroup class
                            counts and its promotion flag -- the layout is defined in pybullet_multigoal_gym_amd/csrc/pmg_sched.h
                            (pmgx::Sched); see DESIGN.md 3.2 */
    PMG_BUF_ENV_CYCLES = 10, /* [N, 2] int32: shader cycles / 64 the env's wavefront spent in its last step, and the largest contact
                            count any of that step's substeps saw (envs with free objects).  Kept when the handle was created with
                            PMG_ENV_CYCLES=1 in the environment (diagnostics) AND whenever the longest-first order of the fast-path
                            list is on (block_stack and the chest tasks from 4096 envs, PMG_LPT_CYCLES; the plan's predictor: 8 B per
                            env written every step); PMG_E_INVALID otherwise */
    PMG_BUF_WAVE_TRACE = 11 /* [2 N] records of 64 bytes, one per wavefront of the last reach step (tip control) and its redo pass: start
                            and end on the constant-rate clock and on the shader clock (4 x int64), HW_ID, XCC_ID (uint32), role (0 list-0
                            wavefront 0, 1 list-0 helper, 2 packed, 3 redo), env (the first of a packed wavefront's four), largest contact
                            count, kernel (1 pmg_k_step_reach, 2 pmg_k_step_reach2, 3 pmg_k_redo), two unused words; unused records are all
                            0xFF bytes.  Kept when the handle was created with PMG_WAVE_TRACE=1 in the environment (diagnostics,
                            tools/wave_trace.py; PMG_BUF_ENV_CYCLES exists then too); PMG_E_INVALID otherwise */
};

/* POD configuration; mirrors the kwargs of pmg.make_env (P/__init__.py:4-11)
 * that the hot path honours, plus the batch geometry.  Zero-initialise and
 * set struct_size = sizeof(pmg_config). */
typedef struct pmg_config {
    int32_t struct_size;
    int32_t task;               /* PMG_TASK_* */
    int32_t num_envs;           /* N: envs simulated by THIS handle (one GPU) */
    int32_t num_block;          /* multi-block tasks (block_stack, block_rearrange, chest_*), 1..5 (P/__init__.py:108) */
    int32_t binary_reward;      /* P/__init__.py:4 */
    int32_t joint_control;      /* P/__init__.py:6 */
    int32_t max_episode_steps;  /* gym TimeLimit, P/__init__.py:6,105 */
    int32_t device;             /* HIP device ordinal */
    float distance_threshold;   /* P/__init__.py:6 */
    int32_t random_order;       /* block_stack, kuka_multi_step_envs.py:7 */
    uint64_t seed_base;         /* env i is seeded with seed_base + i*seed_stride */
    uint64_t seed_stride;       /* 0 reproduces the reference (every env seed 0) */
    int32_t env_index_offset;   /* global index of this shard's env 0 (multi-GPU) */
    int32_t task_decomposition; /* block_stack, chest_*: sub-goals, kuka_multi_step_envs.py:89-122, 285-342, 433-475
                                   (excludes use_curriculum) */
    int32_t use_curriculum;     /* kuka_multi_step_base_env.py:121-140: num_block levels (block_stack / block_rearrange,
                                   num_block >= 2) or num_block + 1 (chest_*: how many blocks go into the chest) */
    int32_t num_goals_to_generate; /* curriculum budget, P/__init__.py:11 (default 1e6); 0 = 1e6 */
    int32_t grip_informed_goal; /* block_stack: goals carry the gripper tip target + finger width (kuka_multi_step_envs.py:75-77);
                                   goal_dim = 3*num_block + 4, sub-goals double (pick / place).  chest_*: goal_dim =
                                   1 + 3*num_block (door joint first) + 3 (chest_push: tip) / + 4 (chest_pick_and_place: tip,
                                   finger width); 2 / 3 sub-goals per block after "open the door" */
    int32_t reserved[3];
} pmg_config;

typedef struct pmg_dims {
    int32_t num_envs;
    int32_t action_dim;      /* kuka.py:103-118 */
    int32_t observation_dim; /* kuka_single_step_base_env.py:193-221; kuka_multi_step_base_env.py:255-336 */
    int32_t policy_state_dim;
    int32_t goal_dim;        /* achieved_goal and desired_goal */
    int32_t state_dim;       /* floats per env in get_state/set_state */
    int32_t packed_dim;      /* floats per env in PMG_BUF_PACKED */
    int32_t reserved;
} pmg_dims;

typedef struct pmg_env pmg_env;

/* Replaces: pmg.make_env -> gym.make -> TaskEnv.__init__ -> BaseBulletMGEnv.__init__
 * (P/__init__.py:178; base_env.py:15-110): creates N worlds with the physics
 * parameters of base_env.py:203-220 and seeds them.  Does NOT perform the
 * constructor's implicit reset (base_env.py:84); the host layer does. */
int pmg_create(const pmg_config* cfg, pmg_env** out);
void pmg_destroy(pmg_env* env);
int pmg_get_dims(const pmg_env* env, pmg_dims* out);
const char* pmg_last_error(const pmg_env* env); /* env may be NULL: last create error */
/* HIP devices this process can see (0 when there is none / no driver): lets a rank whose launcher restricted
 * visibility to one GPU fall back to device 0 instead of LOCAL_RANK (bench.py). */
int pmg_device_count(void);

/* Replaces: BaseBulletMGEnv.seed (base_env.py:120-122) == gym.utils.seeding.np_random:
 * MT19937 seeded by init_by_array(sha512(str(seed))[:8]) per env. */
int pmg_seed(pmg_env* env, uint64_t seed_base, uint64_t seed_stride);

/* Replaces: BaseBulletMGEnv.reset (base_env.py:124-128) = Kuka.robot_specific_reset
 * (kuka.py:120-165) + _task_reset/_generate_goal (kuka_single_step_base_env.py:76-148;
 * kuka_multi_step_base_env.py:183-250; kuka_multi_step_envs.py:34-87) + _get_obs.
 * mask: N bytes (nonzero = reset this env) or NULL = all.  Output pointers may
 * be NULL to skip the copy-out.  Envs outside the mask keep their state; their rows of PMG_BUF_PACKED get a fresh
 * observation / desired goal of that state and KEEP reward | goal_achieved | done of their last step (a device-resident
 * loop may step, reset(mask = done) and then still read every env's last reward). */
int pmg_reset(pmg_env* env, const uint8_t* mask, float* observation, float* policy_state,
              float* achieved_goal, float* desired_goal);

/* Replaces: TimeLimit.step -> BaseBulletMGEnv.step (base_env.py:130-138) =
 * Kuka.apply_action (kuka.py:167-225: tip-delta, clip, IK, motors,
 * 5 x stepSimulation) + _get_obs + _compute_reward.  actions: [N, action_dim]. */
int pmg_step(pmg_env* env, const float* actions, float* observation, float* policy_state,
             float* achieved_goal, float* desired_goal, float* reward, uint8_t* goal_achieved,
             uint8_t* done);

/* Device-resident variants: inputs already in HBM, outputs stay in the
 * library's device buffers (pmg_device_ptr).  Stream-ordered, no host sync. */
int pmg_reset_device(pmg_env* env, const uint8_t* d_mask);
/* The vectorised-env policy the reference leaves to its caller (one gym env is reset by whoever reads `done`): reset, on
 * the device and without a host mask, exactly the envs whose episode has ended -- TimeLimit: elapsed steps >=
 * max_episode_steps (gym TimeLimit.step; reference: P/__init__.py:148-177 `max_episode_steps`).  Same state as
 * pmg_reset_device with the mask of those envs; in the packed row the observation / goals are the new episode's first
 * ones while reward | goal_achieved | done keep the finished step's values (the usual auto-reset convention).
 * Idempotent: a freshly reset env has elapsed = 0. */
int pmg_reset_done_device(pmg_env* env);
int pmg_step_device(pmg_env* env, const float* d_actions);
int pmg_device_ptr(pmg_env* env, int which, void** d_ptr);
int pmg_stream(pmg_env* env, void** hip_stream);
int pmg_sync(pmg_env* env);
/* copy the current output buffers to host (any pointer may be NULL) */
int pmg_read_outputs(pmg_env* env, float* observation, float* policy_state, float* achieved_goal,
                     float* desired_goal, float* reward, uint8_t* goal_achieved, uint8_t* done);

/* Replaces: KukaBulletMGEnv._compute_reward (kuka_single_step_base_env.py:237-244;
 * kuka_multi_step_base_env.py:338-345) on [B, goal_dim] batches (HER relabelling). */
int pmg_compute_reward(pmg_env* env, const float* achieved_goal, const float* desired_goal,
                       int64_t batch, float* reward, uint8_t* goal_achieved);
int pmg_compute_reward_device(pmg_env* env, const float* d_achieved_goal, const float* d_desired_goal,
                              int64_t batch, float* d_reward, uint8_t* d_goal_achieved);

/* Running normaliser and policy-input rows of goal-conditioned learners (HER + DDPG / SAC; no reference equivalent: the
 * reference leaves both to its caller).  A handle owns three independent normalisers of widths observation_dim,
 * policy_state_dim and goal_dim; each keeps, in float64 on the device, the per-column sum S and sum of squares Q of the
 * input-clipped rows it was shown and their count n, and derives in float32 mean = S/n, std = sqrt(max(eps^2,
 * Q/n - (S/n)^2)) and inv_std = 1/std (n == 0: mean 0, std = inv_std = 1).  Sums are deterministic: their order is a
 * function of the batch size, the width and env_index_offset alone.  Defaults: eps 0.01, clip_input
 * 200, clip_output 5.  *_device calls are stream-ordered on the handle's stream; none of these calls reads or writes
 * anything else of the handle. */
enum { PMG_NORM_OBSERVATION = 0, PMG_NORM_POLICY_STATE = 1, PMG_NORM_GOAL = 2 };
/* settings of all three normalisers (positive, finite); re-derives mean / std / inv_std, keeps the totals */
int pmg_norm_configure(pmg_env* env, float eps, float clip_input, float clip_output);
/* add rows [batch, D] (row_stride floats from row to row, >= D; any alignment) to normaliser `which`; d_mask: batch bytes,
 * nonzero = take the row, or NULL = all */
int pmg_norm_update_device(pmg_env* env, int which, const float* d_rows, int64_t row_stride, int64_t batch, const uint8_t* d_mask);
int pmg_norm_update(pmg_env* env, int which, const float* rows, int64_t batch, const uint8_t* mask);   /* host, contiguous */
/* observation, policy_state and desired_goal of the rows of the LAST step / reset (PMG_BUF_PACKED, read in place) into
 * the three normalisers; d_mask: N bytes or NULL */
int pmg_norm_update_env_device(pmg_env* env, const uint8_t* d_mask);
/* sum [D], sumsq [D], count [1], mean / std / inv_std [D]; any pointer may be NULL; synchronous */
int pmg_norm_read(pmg_env* env, int which, double* sum, double* sumsq, double* count, float* mean, float* std, float* inv_std);
/* restore the totals (checkpoints); NULL totals with count 0 = reset; synchronous */
int pmg_norm_write(pmg_env* env, int which, const double* sum, const double* sumsq, double count);
/* d_out [batch, Ds + Dg], contiguous, state columns first: per element y = clip((clip(v, clip_input) - mean) * inv_std,
 * clip_output) in float32; state_kind = PMG_NORM_OBSERVATION or PMG_NORM_POLICY_STATE, goals use PMG_NORM_GOAL */
int pmg_policy_input_device(pmg_env* env, int state_kind, const float* d_state, int64_t state_stride,
                            const float* d_goal, int64_t goal_stride, int64_t batch, float* d_out);
int pmg_policy_input(pmg_env* env, int state_kind, const float* state, const float* goal, int64_t batch, float* out); /* host */
/* [N, Ds + Dg] from the state and desired_goal columns of the rows of the LAST step / reset */
int pmg_policy_input_env_device(pmg_env* env, int state_kind, float* d_out);

/* Hindsight-experience-replay (HER) minibatches, sampled on the device from episodes the CALLER keeps in device memory (no
 * reference equivalent: the reference leaves replay to its caller).  The library owns no store: a rollout copies
 * PMG_BUF_PACKED (and its actions) into its own table once per step (pmg_device_copy), and pmg_her_sample_device reads
 * that table in place: it draws B transitions (e, t), relabels each with probability future_p by an achieved goal of a
 * later step f of the same episode, and writes the finished minibatch: state | goal rows for t and t + 1 through the handle's
 * normalisers, the action, and reward / flag of the (possibly relabelled) goal.  Stream-ordered on the handle's stream, no host
 * sync; it reads the normalisers' derived values as they are on the stream at that point, writes nothing but the given
 * outputs and touches neither the handle's state nor the envs' RNG streams.
 *
 * Draws, a pure function of (seed, counter, sample index b) -- sample b does not depend on B, state_kind or raw:
 *   mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31   (mod 2^64)
 *   GOLD = 0x9E3779B97F4A7C15; key = mix(seed ^ mix(counter + GOLD)); r_k(b) = mix(key + (4 b + k + 1) GOLD) >> 32, k = 0..3
 *   e = (r_0 E) >> 32; t = (r_1 T) >> 32; relabelled iff (double)r_2 < (double)future_p * 2^32; f = t + 1 + ((r_3 (T - t)) >> 32)
 * so 0 <= e < E, 0 <= t < T and t < f <= T by construction.  The multiply-shift maps 2^32 values onto n cells: a cell's
 * probability is off 1 / n by at most 2^-32 (a relative bias of at most n / 2^32), which is accepted. */
typedef struct pmg_her_source {      /* episodes in caller-owned device memory, read in place */
    int32_t struct_size;
    int32_t num_episodes;            /* E >= 1: complete episodes */
    int32_t episode_steps;           /* T >= 1: every episode has rows 0..T and actions 0..T-1; (T + 1) E < 2^31 */
    int32_t reserved;
    const float* d_rows;             /* packed rows (PMG_BUF_PACKED layout, packed_dim floats): row (e, t) at
                                        d_rows + e * row_episode_stride + t * row_time_stride */
    int64_t row_episode_stride, row_time_stride;        /* in floats, >= packed_dim; 0 only where the extent is 1 (E == 1) */
    const float* d_actions;          /* action (e, t), action_dim floats; may be NULL when d_action is NULL */
    int64_t action_episode_stride, action_time_stride;  /* in floats, >= action_dim; 0 only where the extent is 1 */
} pmg_her_source;

typedef struct pmg_her_batch {
    int32_t struct_size;
    int32_t state_kind;              /* PMG_NORM_OBSERVATION or PMG_NORM_POLICY_STATE */
    int32_t raw;                     /* 0: rows through the handle's normalisers exactly as pmg_policy_input_device;
                                        1: bit copies of state | goal, no clip, no normalisation */
    float   future_p;                /* in [0, 1]; HER's k / (k + 1), usually 0.8 */
    uint64_t seed, counter;          /* the draws are a pure function of (seed, counter, sample index) */
    int64_t batch;                   /* B >= 0; 0 is a successful no-op */
    float* d_x;                      /* [B, Ds + Dg]  state(e, t)     | g'   -- every output may be NULL */
    float* d_x_next;                 /* [B, Ds + Dg]  state(e, t + 1) | g' */
    float* d_action;                 /* [B, action_dim] */
    float* d_reward;                 /* [B]  reward of (achieved_goal(e, t + 1), g'), as pmg_compute_reward */
    uint8_t* d_goal_achieved;        /* [B] */
    int32_t* d_index;                /* [B, 3]: e, t, f (f = -1 where the goal was not relabelled) */
} pmg_her_batch;
/* g' = achieved_goal(e, f) where the sample was relabelled, desired_goal(e, t) otherwise; reward and flag use the handle's
 * binary_reward and distance_threshold.  Both strides given, a table may be time-major [T + 1, E, P] (one pmg_device_copy
 * of PMG_BUF_PACKED per step) or episode-major [E, T + 1, P], padded or not; inputs and outputs may have any 4-byte
 * alignment.  PMG_E_INVALID (nothing launched): wrong struct_size, E < 1, T < 1, (T + 1) E >= 2^31, B < 0, d_rows NULL, a
 * stride too small, state_kind not a state kind, future_p outside [0, 1] or NaN, d_action without d_actions.  With d_index
 * NULL the indices go to scratch of the handle, sized at the first call (a later LARGER batch re-sizes it, which waits
 * for the stream once). */
int pmg_her_sample_device(pmg_env* env, const pmg_her_source* src, const pmg_her_batch* out);

/* The actor on the device: a multi-layer perceptron on rows of floats, and the exploration policy of DDPG / HER on its output (no
 * reference equivalent: the reference leaves the policy to its caller).  With it a rollout is two stream-ordered calls per step,
 * pmg_act_env_device and pmg_step_device, and nothing leaves the GPU.  The caller owns the weights (device memory, read in place,
 * never written by these two calls; the update side below writes only what it is handed); the library keeps no learner state.  Both calls are stream-ordered on the handle's stream, sync nothing, write
 * only their outputs and touch no state of the handle: state rows, packed rows, RNG streams and normaliser totals stay as they are.
 *
 * Layers (normative).  Layer l, row r, unit j is ONE float32 chain: acc = bias[j] (+0.0 without a bias), then
 * acc = fmaf(h[r][k], W[j][k], acc) for k = 0, 1, ..., K - 1 in ascending order; a hidden layer's output is fmaxf(acc, 0), the last
 * layer's acc is the pre-activation z.  No split-K, no other order: a row's result does not depend on the batch it is in.
 * (Products of an exact zero with an exact zero may follow the chain: they can turn -0 into +0 and change nothing else.)
 *
 * Action of global env g = env_index_offset + i, column j, A = action_dim; the draws are those of pmg_her_sample_device above
 * with b = g A + j in place of the sample index: key = mix(seed ^ mix(counter + GOLD)), r_k = mix(key + (4 b + k + 1) GOLD) >> 32,
 *   u1 = ((r_0 >> 8) + 1) 2^-24 in (0, 1];  u2 = (r_1 >> 8) 2^-24 in [0, 1);  v = (r_2 >> 8) 2^-23 - 1 in [-1, 1)   (exact in float32)
 *   env g is random iff r_3 of ITS COLUMN 0 (b = g A) < ceil(random_eps 2^32)                                       (integer compare)
 * and in float32: a0 = out_activation ? tanh(z) : z;  a1 = noise_eps > 0 ? a0 + noise_eps sqrt(-2 ln u1) cos(2 pi u2) : a0;
 * a2 = min(max(a1, -1), 1);  a = random ? v : a2.  explore == NULL: a = a2 of a1 = a0.  So the action of env g is a function of its
 * own row, the weights and (seed, counter, g): it depends neither on N nor on the shard. */
typedef struct pmg_mlp {                 /* caller-owned device memory, read in place, never written */
    int32_t struct_size;
    int32_t num_layers;                  /* L in 1..4 */
    int32_t width[5];                    /* width[0] = inputs, width[l + 1] = outputs of layer l; each in 1..256 */
    int32_t out_activation;              /* 0 identity, 1 tanh; hidden layers are ReLU */
    const float* d_weight[4];            /* layer l: [width[l + 1], width[l]] row-major, contiguous (torch nn.Linear.weight) */
    const float* d_bias[4];              /* [width[l + 1]] or NULL (= +0.0) */
} pmg_mlp;
typedef struct pmg_explore {
    int32_t struct_size, reserved;
    float noise_eps;                     /* >= 0, finite; 0 = no noise term at all */
    float random_eps;                    /* in [0, 1] */
    uint64_t seed, counter;
} pmg_explore;
/* d_out [batch, width[L]] = out_activation(z) of the rows d_in [batch, width[0]]; in_stride / out_stride floats from row to row
 * (>= the widths); any 4-byte alignment.  batch == 0 is a successful no-op. */
int pmg_mlp_forward_device(pmg_env* env, const pmg_mlp* mlp, const float* d_in, int64_t in_stride, int64_t batch,
                           float* d_out, int64_t out_stride);
/* The actions of all N envs from the rows of the LAST step / reset: the state_kind columns and desired_goal of PMG_BUF_PACKED (under
 * pmg_comm_overlap the buffer that name refers to at this point), read in place, every element through the normalisers' derived
 * values as they are on the stream -- layer 0 sees exactly the row pmg_policy_input_env_device would write.  Needs width[0] ==
 * Ds + Dg and width[L] == action_dim.  d_actions [N, action_dim] (what pmg_step_device takes); d_preact [N, action_dim] receives z, or
 * NULL.  PMG_E_STATE before the first reset.
 * Both calls return PMG_E_INVALID, with nothing launched, for: a wrong struct_size, L or a width out of range, an out_activation
 * that is neither 0 nor 1, a NULL weight or output pointer (d_in too), a pointer not aligned to 4 bytes, a stride below the width,
 * batch < 0, a state_kind that is no state kind, widths that do not match the dims, noise_eps negative or not finite, random_eps
 * outside [0, 1] or NaN. */
int pmg_act_env_device(pmg_env* env, const pmg_mlp* mlp, int state_kind, const pmg_explore* explore /* NULL = none */,
                       float* d_actions /* [N, action_dim] */, float* d_preact /* [N, action_dim] or NULL */);

/* The critic Q(x, a) and the TD target of a DDPG / HER update on the device, forward only (no reference equivalent).  Both entries
 * take networks as pmg_mlp above, are stream-ordered on the handle's stream, sync nothing, write only their outputs and touch no
 * state of the handle.  The learner loop is pmg_her_sample_device -> pmg_td_target_device on its d_x_next and d_reward -> the
 * gradients, Adam steps and Polyak updates of pmg_mlp_grad_device, pmg_mlp_adam_device and pmg_mlp_polyak_device below.
 *
 * pmg_q_device: q[b] (at d_q + b * q_stride) = out_activation(z) of the critic on the row x[b] | a[b]: column c < x_dim is
 * x[b][c], column x_dim + j is a[b][j]; both tables are read in place at their own strides.  It is the layer chain above on that
 * row: bit for bit what pmg_mlp_forward_device returns on a table that holds the concatenated rows.
 *
 * pmg_td_target_device (normative), float32 throughout, Dx = actor.width[0], A = actor.width[L], row x' of d_x_next:
 *   a'[j] = min(max(actor.out_activation ? tanhf(z[j]) : z[j], -1), 1)      z = the actor's chain on x'
 *   q'    = critic.out_activation(z_c), z_c = the critic's chain on the row x' | a' (column c < Dx is x'[c], column Dx + j is a'[j])
 *   t     = terminal ? r : fmaf(gamma, q', r)
 *   y     = fminf(fmaxf(t, clip_lo), clip_hi)
 * A sample's result does not depend on the batch it is in.  (fminf / fmaxf of -0.0 and +0.0 may return either zero: where t and a clip
 * are zeros of opposite sign, the sign of y's zero is not specified.)
 *
 * PMG_E_INVALID, with nothing launched: everything the calls above reject in a network, for either network; critic.width[0] !=
 * x_dim + a_dim (pmg_q_device) or != Dx + A (so Dx + A <= 256); critic.width[L] != 1; x_dim < 1 or a_dim < 1; a wrong
 * struct_size; a NULL required pointer; a pointer not aligned to 4 bytes (d_terminal: any address); a stride below its width;
 * batch < 0; gamma negative or not finite; clip_lo > clip_hi or either a NaN.  batch == 0 is a successful no-op. */
int pmg_q_device(pmg_env* env, const pmg_mlp* critic, const float* d_x, int64_t x_stride, int32_t x_dim,
                 const float* d_a, int64_t a_stride, int32_t a_dim, int64_t batch, float* d_q, int64_t q_stride);
typedef struct pmg_td_target {
    int32_t struct_size, reserved;
    float gamma;                         /* finite, >= 0 */
    float clip_lo, clip_hi;              /* clip_lo <= clip_hi; -inf / +inf = no clip; NaN invalid */
    int64_t batch;
    const float* d_x_next; int64_t x_stride;   /* [B, Dx] at x_stride floats from row to row, e.g. pmg_her_batch.d_x_next */
    const float* d_reward;               /* [B] */
    const uint8_t* d_terminal;           /* [B] or NULL; non-zero: no bootstrap term, t = r */
    float* d_y;                          /* [B]     required */
    float* d_q_next;                     /* [B]     or NULL: q' */
    float* d_next_action;                /* [B, A]  or NULL: a' */
} pmg_td_target;
int pmg_td_target_device(pmg_env* env, const pmg_mlp* actor_target, const pmg_mlp* critic_target, const pmg_td_target* td);

/* The update side of a DDPG / HER learner on the device (no reference equivalent): back-propagation through a pmg_mlp, an Adam step and
 * a Polyak (soft target) update.  All three are stream-ordered on the handle's stream, sync nothing, write only their outputs (and
 * d_work) and touch no state of the handle.
 *
 * pmg_mlp_grad_device (normative), float32 throughout.
 * Forward: the layer chain above, unchanged.  h_0 is the input row (with d_a: the row x[b] | a[b] as in pmg_q_device), z_l[j] the fmaf
 * chain over k ascending from bias[j], h_{l+1} = fmaxf(z_l, 0) on hidden layers, o = out_activation ? tanhf(z_{L-1}) : z_{L-1}.  d_out,
 * when given, receives o.
 * Head: g[b][j] = d_gout[b][j] when d_gout is given;  gscale * (o[b][j] - d_target[b][j]) (two roundings) when d_gout is NULL and
 * d_target is given -- the MSE of a critic with gscale = 2 / B;  the constant gscale when both are NULL -- the actor's -mean Q with
 * gscale = -1 / B.  Giving both is invalid.
 * Output delta: delta_{L-1} = out_activation ? g * fmaf(-o, o, 1.f) : g, with o the very value written to d_out.
 * Backward, l = L-1 ... 0:
 *   dW_l[j][k]: acc = +0.0; acc = fmaf(delta_l[b][j], h_l[b][k], acc) for b = 0 ... B-1 ascending: ONE chain, no split over the batch.
 *   db_l[j]:    acc = +0.0; acc = acc + delta_l[b][j] for b ascending (fmaf(delta, 1, acc) is the same value).
 *   s_l[b][k]:  acc = +0.0; acc = fmaf(delta_l[b][j], W_l[j][k], acc) for j = 0 ... width[l+1]-1 ascending.
 *     l >= 1: delta_{l-1}[b][k] = h_l[b][k] > 0 ? s_l[b][k] : +0.0 -- a real +0.0, not a product with a zero, so a masked inf does not
 *             become a NaN; a unit whose z is exactly 0 is masked.
 *     l == 0: s_0[b][c] goes to d_gx[b][c] for c < x_dim and to d_ga[b][c - x_dim] otherwise.
 * As in the forward, padding products of exact zeros may follow a chain: they affect only the sign of a zero.
 * A row's delta, d_gx, d_ga and d_out do not depend on the batch it is in; dW and db depend on the row order and on nothing else; nothing
 * depends on the grid or the number of compute units; two calls on the same inputs give the same bits.
 * Known limit: the single chain over the batch costs B / 2 dependent matrix steps per tile of a dW.  That is the right trade for the
 * minibatches HER uses (256 to 4096 rows); pmg_mlp_grad_chunked_device below is the chunked reduction, with its own normative order.
 *
 * PMG_E_INVALID, with nothing launched: everything pmg_q_device rejects in the network and the row tables; d_a without a_dim >= 1 or the
 * reverse; x_dim + a_dim != width[0]; d_ga without d_a; both d_gout and d_target; gscale not finite; grads, d_gx, d_ga and d_out all
 * NULL; a grads tensor that is NULL where the network has that tensor, or a bias gradient where it has no bias; d_work NULL or
 * work_floats too small; a float pointer off 4 bytes; a stride below its width; batch < 0; a wrong struct_size.  batch == 0 is a
 * successful no-op that leaves grads untouched. */
typedef struct pmg_mlp_params {          /* one float per parameter, pmg_mlp's layout: [width[l + 1], width[l]] and [width[l + 1]] */
    float* d_weight[4];
    float* d_bias[4];                    /* NULL where the network has no bias */
} pmg_mlp_params;
typedef struct pmg_mlp_grad {
    int32_t struct_size, reserved;
    float gscale;                        /* finite */
    int32_t x_dim, a_dim;                /* a_dim == 0 with d_a == NULL: raw rows, x_dim == width[0] */
    int32_t reserved2;
    int64_t batch;
    const float* d_x; int64_t x_stride;            /* rows; with d_a: the row x[b] | a[b] as in pmg_q_device */
    const float* d_a; int64_t a_stride;            /* or NULL */
    const float* d_gout; int64_t gout_stride;      /* [B, width[L]] dLoss / d out, or NULL (see the head) */
    const float* d_target; int64_t target_stride;  /* [B, width[L]] or NULL */
    const pmg_mlp_params* grads;         /* written (overwritten, never accumulated into); NULL = input gradients only */
    float* d_gx; int64_t gx_stride;      /* [B, x_dim] or NULL */
    float* d_ga; int64_t ga_stride;      /* [B, a_dim] or NULL */
    float* d_out; int64_t out_stride;    /* [B, width[L]] or NULL: out_activation(z), the forward's result */
    float* d_work; int64_t work_floats;  /* scratch, at least pmg_mlp_grad_work_floats(mlp, batch) */
} pmg_mlp_grad;
int64_t pmg_mlp_grad_work_floats(const pmg_mlp* mlp, int64_t batch);   /* < 0: invalid network / batch */
int pmg_mlp_grad_device(pmg_env* env, const pmg_mlp* mlp, const pmg_mlp_grad* g);

/* pmg_mlp_grad_chunked_device (normative), float32 throughout: pmg_mlp_grad_device with the batch reduction of dW / db cut
 * into chunks of R = chunk_rows rows, so that ceil(B / R) times as many wavefronts run chains of R / 2 matrix steps instead of B / 2.
 * Stream-ordered on the handle's stream, syncs nothing, writes only its outputs and d_work, touches no state of the handle.
 * Forward, head, output delta, s_l, masks, d_gx, d_ga and d_out: pmg_mlp_grad_device above, to the letter.
 * C = ceil(B / R) chunks; chunk c holds the rows c R ... min((c + 1) R, B) - 1.
 *   P_c[j][k]:  acc = +0.0; acc = fmaf(delta_l[b][j], h_l[b][k], acc) for b ascending over chunk c.
 *   Pb_c[j]:    acc = +0.0; acc = acc + delta_l[b][j] for b ascending over chunk c.
 *   dW_l[j][k] = (...((P_0 + P_1) + P_2) ... + P_{C-1}): float32 additions, c ascending, one rounding each; db_l likewise from Pb_c.
 * C == 1 (R >= B) is by definition pmg_mlp_grad_device: the same bits.  gscale is the caller's: nothing is rescaled per chunk.  dW and db
 * depend on the row order and on R and on nothing else -- not on the grid or the number of compute units --, and two calls on the same
 * inputs give the same bits.  Zeros compare by value, as above.
 * Workspace: pmg_mlp_grad_chunked_work_floats(mlp, batch, chunk_rows) = pmg_mlp_grad_work_floats(mlp, batch), laid out as for
 * pmg_mlp_grad_device, and for C > 1 behind it C x P floats of partials, P = the sum over the layers of (width[l] + 1) * width[l + 1] (a
 * bias is counted for every layer).  With grads == NULL (input gradients only) nothing is reduced: pmg_mlp_grad_work_floats(mlp, batch)
 * suffices.
 * PMG_E_INVALID, with nothing launched: everything pmg_mlp_grad_device rejects; chunk_rows < 2 or odd (an even R keeps every chunk's
 * first row even, so only the last chunk can end on a single row); more than PMG_GRAD_MAX_CHUNKS chunks (the partials of all chunks are
 * formed by one launch, a workgroup per chunk and 32 x 32 tile of a dW_l; 65 535 chunks of the at most 256 tiles of a network stay below
 * the 2^32 work-items of one grid); work_floats below the figure above.  batch == 0 is a successful no-op that leaves grads untouched. */
#define PMG_GRAD_MAX_CHUNKS 65535
int64_t pmg_mlp_grad_chunked_work_floats(const pmg_mlp* mlp, int64_t batch, int64_t chunk_rows);   /* < 0: invalid network / batch / chunk_rows */
int pmg_mlp_grad_chunked_device(pmg_env* env, const pmg_mlp* mlp, const pmg_mlp_grad* g, int64_t chunk_rows);

/* Adam and Polyak: one elementwise launch over the up to eight tensors of a network each.  `shape` supplies the widths and which layers
 * have a bias; its pointers are not dereferenced.
 * Adam (normative per element): the host computes in double c1 = 1 - beta1^t, c2 = 1 - beta2^t and passes omb1 = (float)(1 - (double)beta1),
 * omb2 likewise, step_size = (float)(lr / c1), rsc2 = (float)(1 / sqrt(c2)); on the device
 *   m = fmaf(beta1, m, omb1 * g);  v = fmaf(beta2, v, omb2 * (g * g));  p = p - step_size * (m / (sqrtf(v) * rsc2 + eps)).
 * m and v are bit-defined; the step goes through the build's sqrtf and division and is held to a float64 model.
 * Polyak: t = fmaf(tau, p - t, t), bit-defined (p: the source's parameter, t: the target's).
 * PMG_E_INVALID: a bad network shape; a NULL or misaligned tensor where the shape has one; lr, eps or a beta not finite; a beta outside
 * [0, 1); eps < 0; step < 1; tau outside [0, 1] or NaN; a wrong struct_size. */
typedef struct pmg_adam { int32_t struct_size, reserved; float lr, beta1, beta2, eps; int64_t step; /* t >= 1 */ } pmg_adam;
int pmg_mlp_adam_device(pmg_env* env, const pmg_mlp* shape, const pmg_mlp_params* param, const pmg_mlp_params* grad,
                        const pmg_mlp_params* m, const pmg_mlp_params* v, const pmg_adam* a);
int pmg_mlp_polyak_device(pmg_env* env, const pmg_mlp* source, const pmg_mlp_params* target, float tau);

/* pmg_policy_grad_device (normative), float32 throughout: the actor's half of a DDPG / HER update in one call -- the gradient of
 *   gscale * sum_b Q(x[b], clip(pi(x[b]))) + l2scale / 2 * sum_b sum_j pi(x[b])[j]^2
 * with respect to the actor's parameters, through the online critic.  HER's loss -mean Q + action_l2 * mean(pi^2) is gscale = -1 / B and
 * l2scale = 2 * action_l2 / (B * A).  Stream-ordered on the handle's stream, syncs nothing, writes only its outputs and d_work, touches no
 * state of the handle; neither network's weights are written.  Per row b, Dx = actor.width[0], A = actor.width[L]:
 *   1. z = the actor's layer chain on x[b];  o[j] = actor.out_activation ? tanhf(z[j]) : z[j];  a[j] = fminf(fmaxf(o[j], -1), 1), the a' of
 *      pmg_td_target_device.  d_out receives o, d_action receives a.
 *   2. q = critic.out_activation(z_c), z_c = the critic's chain on the row x[b] | a.  d_q receives q.
 *   3. The critic's backward is pmg_mlp_grad_device's with the constant head gscale and input gradients only:
 *      delta = critic.out_activation ? gscale * fmaf(-q, q, 1.f) : gscale, then the transposed chains s_l and the masks;
 *      ga[j] = s_0[Dx + j].  d_gaction receives ga.  No gradient of the critic's parameters is formed.
 *   4. g[j] = fmaf(l2scale, o[j], (o[j] >= -1.f && o[j] <= 1.f) ? ga[j] : +0.0f): the clip's derivative, inclusive at +-1 as torch.clamp's is; a
 *      NaN o takes the +0.0 branch; the L2 term acts on the unclipped o.
 *   5. delta_{L-1} = actor.out_activation ? g * fmaf(-o, o, 1.f) : g, and from there dW_l and db_l of the actor exactly as pmg_mlp_grad_device
 *      (chunk_rows == 0) or pmg_mlp_grad_chunked_device (chunk_rows >= 2, even) forms them from d_gout = g.
 * So the call equals, bit for bit with zeros compared by value, pmg_mlp_forward_device(actor) -> a = clip(o) on the host ->
 * pmg_mlp_grad_device(critic, x | a, constant head, d_ga, d_out) -> g on the host -> pmg_mlp_grad[_chunked]_device(actor, d_gout = g).
 * A row's a, o, q and ga do not depend on the batch it is in; dW and db depend on the row order and on chunk_rows and on nothing else;
 * nothing depends on the grid; two calls on the same inputs give the same bits.
 * grads == NULL: steps 4 and 5 do not run and d_work is not touched.  Workspace: pmg_policy_grad_work_floats(actor, critic, batch, chunk_rows)
 * = pmg_mlp_grad_work_floats(actor, batch) for chunk_rows == 0, pmg_mlp_grad_chunked_work_floats(actor, batch, chunk_rows) otherwise, laid
 * out as those calls lay it out; while the critic runs, o is kept where the actor's delta_{L-1} will be.
 * PMG_E_INVALID, with nothing launched: everything pmg_td_target_device rejects in the pair of networks (critic.width[0] != Dx + A,
 * critic.width[L] != 1, a bad network); gscale or l2scale not finite; grads, d_action, d_out, d_q and d_gaction all NULL; a grads tensor
 * that is NULL where the actor has that tensor, or a bias gradient where it has no bias; d_x NULL; d_work NULL or work_floats too small; a
 * float pointer off 4 bytes; a stride below its width; batch < 0; chunk_rows negative, 1 or odd, or more than PMG_GRAD_MAX_CHUNKS chunks; a
 * wrong struct_size.  batch == 0 is a successful no-op that leaves grads untouched. */
typedef struct pmg_policy_grad {
    int32_t struct_size, reserved;
    float gscale;                        /* finite; -1 / B for -mean Q */
    float l2scale;                       /* finite; 2 * action_l2 / (B * A) for action_l2 * mean(o^2); 0: no L2 term */
    int64_t batch;
    const float* d_x; int64_t x_stride;            /* [B, Dx] */
    const pmg_mlp_params* grads;         /* the ACTOR's dW / db, overwritten; NULL: the outputs below only */
    float* d_action; int64_t action_stride;        /* [B, A] or NULL: a = clip(o) */
    float* d_out; int64_t out_stride;              /* [B, A] or NULL: o, unclipped */
    float* d_q;                                    /* [B] or NULL: Q(x, a) of the online critic */
    float* d_gaction; int64_t gaction_stride;      /* [B, A] or NULL: ga = dLoss / da in front of the clip and the L2 term */
    float* d_work; int64_t work_floats;  /* scratch, at least pmg_policy_grad_work_floats(actor, critic, batch, chunk_rows) */
} pmg_policy_grad;
int64_t pmg_policy_grad_work_floats(const pmg_mlp* actor, const pmg_mlp* critic, int64_t batch, int64_t chunk_rows);   /* chunk_rows 0: one chain; < 0: invalid */
int pmg_policy_grad_device(pmg_env* env, const pmg_mlp* actor, const pmg_mlp* critic, const pmg_policy_grad* g, int64_t chunk_rows);

/* pmg_policy_grad_bc_device (normative), float32 throughout: pmg_policy_grad_device with a behaviour-cloning term on the
 * demonstration rows of the minibatch and its Q-filter (Nair et al., Overcoming Exploration in RL with Demonstrations; the bc_loss / q_filter
 * options of OpenAI baselines' HER) -- the gradient of
 *   gscale * sum_b Q(x[b], clip(pi(x[b]))) + l2scale / 2 * sum_b sum_j pi(x[b])[j]^2 + bcscale / 2 * sum_{b in F} sum_j (pi(x[b])[j] - ad[b][j])^2
 * with respect to the actor's parameters, F = the demonstration rows that are cloned, a constant of the gradient.  Rows b >= demo_begin are
 * demonstrations (baselines puts them last) with the demonstrated action ad[b].  baselines' prm_loss_weight * -mean Q + aux_loss_weight *
 * sum of squares is gscale = -prm_loss_weight / B, bcscale = 2 * aux_loss_weight.  With q_filter == 0 and demo_begin == 0 the head is TD3+BC's
 * actor loss.  Per row b, steps 1-3 of pmg_policy_grad_device are taken to the letter (o, a = clip(o), q, ga).  Then:
 *   2b. for b >= demo_begin: qd = critic.out_activation(z), z = the critic's chain on the row x[b] | ad[b] -- ad as given, not clipped --,
 *       the chain pmg_q_device runs on that row.  d_q_demo[b] receives qd.
 *   2c. f = b >= demo_begin && (!q_filter || qd > q), a float32 compare: a NaN on either side gives 0, qd == q gives 0.  d_filter[b] receives f.
 *   4.  g4[j] = fmaf(l2scale, o[j], inside ? ga[j] : +0.0f) as there;  g[j] = f ? fmaf(bcscale, o[j] - ad[b][j], g4[j]) : g4[j].  The
 *       difference is rounded once, then the fmaf rounds; like the L2 term, the cloning term acts on the unclipped o.
 *   5.  as there, from g; single chain or chunked.
 * So the call equals, bit for bit with zeros compared by value, pmg_mlp_forward_device(actor) -> clip on the host -> pmg_q_device on x | ad ->
 * pmg_mlp_grad_device(critic, x | a, constant head, input gradients only) -> f and g on the host with an exact fmaf ->
 * pmg_mlp_grad[_chunked]_device(actor, d_gout = g).  With demo_begin == B every output has the bits of pmg_policy_grad_device, d_filter is
 * all 0, d_q_demo is untouched and d_demo_action may be NULL.  A row's outputs depend on its own x and ad, the weights and on whether
 * b >= demo_begin -- not on the batch, the grid or the neighbouring rows: a batch cut at row s gives the same rows when each piece passes
 * clamp(demo_begin - s, 0, B_piece).  dW and db depend on the row order and chunk_rows as there.
 * Workspace: exactly pmg_policy_grad_work_floats(actor, critic, batch, chunk_rows).  grads == NULL: steps 4 and 5 do not run and d_work is
 * not touched; d_q_demo and d_filter are still written.
 * PMG_E_INVALID, with nothing launched: everything pmg_policy_grad_device rejects, d_q_demo and d_filter counting as outputs in its "all
 * outputs NULL" rule; bc NULL or a wrong struct_size; bcscale not finite; q_filter not 0 / 1; demo_begin outside [0, B]; d_demo_action NULL
 * while demo_begin < B, or off 4 bytes, or with a stride below A; d_q_demo off 4 bytes.  batch == 0 is a successful no-op. */
typedef struct pmg_policy_bc {
    int32_t struct_size;
    int32_t q_filter;                 /* 0: every demonstration row is cloned; 1: only where q_demo > q */
    float   bcscale;                  /* finite; the term is bcscale / 2 * sum over cloned rows of sum_j (o[j] - ad[j])^2 */
    int32_t reserved;
    int64_t demo_begin;               /* 0 <= demo_begin <= B: rows b >= demo_begin are demonstrations */
    const float* d_demo_action; int64_t demo_action_stride;   /* [B, A], indexed by the batch row b; rows below demo_begin are never read, so the
                                                                 sampler's d_action of the joined minibatch can be passed as it is */
    float*   d_q_demo;                /* [B] or NULL: Q(x[b], ad[b]); written for b >= demo_begin only */
    uint8_t* d_filter;                /* [B] or NULL, any address: 1 where the row was cloned, 0 elsewhere (every row is written) */
} pmg_policy_bc;
int pmg_policy_grad_bc_device(pmg_env* env, const pmg_mlp* actor, const pmg_mlp* critic, const pmg_policy_grad* g, const pmg_policy_bc* bc,
                              int64_t chunk_rows);

/* pmg_td3_target_device (normative), float32 throughout: the TD target of TD3 in one call -- target-policy smoothing and the
 * smaller of two target critics,
 *   y = clip(r + gamma * min(Q1'(x', a~), Q2'(x', a~))),   a~ = clip(clip(pi'(x')) + clip(sigma * n, -c, c), -1, 1),   n ~ N(0, 1).
 * Stream-ordered on the handle's stream, syncs nothing, writes only its outputs and d_work, touches no state of the handle.  Per row b,
 * Dx = actor.width[0], A = actor.width[L]:
 *   1. z = the actor's layer chain on x'[b];  a0[j] = min(max(actor.out_activation ? tanhf(z[j]) : z[j], -1), 1), the a' of pmg_td_target_device.
 *   2. sigma > 0: the draws are those of pmg_her_sample_device with s = (row_offset + b) * A + j as the sample index:
 *      key = mix(seed ^ mix(counter + GOLD)), r_k = mix(key + (4 s + k + 1) GOLD) >> 32, u1 = ((r_0 >> 8) + 1) 2^-24, u2 = (r_1 >> 8) 2^-24
 *      as pmg_act_env_device forms them (r_2 and r_3 are not used);
 *        e    = fminf(fmaxf(sigma * sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2), -c), c)
 *        a~[j] = fminf(fmaxf(a0[j] + e, -1.f), 1.f)
 *      sigma == 0: no draw is made and a~ = a0 bit for bit.
 *   3. q1 = critic1.out_activation(z_c1), z_c1 = critic 1's chain on the row x'[b] | a~; q2 likewise from critic 2; qmin = fminf(q1, q2): a
 *      NaN loses against a number, and of two zeros of opposite sign either may be returned.  critic2 == NULL: qmin = q1.
 *   4. t = terminal ? r : fmaf(gamma, qmin, r);  y = fminf(fmaxf(t, clip_lo), clip_hi)   (the sign of a zero y as for pmg_td_target_device).
 * With critic2 == NULL and sigma == 0 the call returns the bits of pmg_td_target_device.  A row's outputs depend on its own x', r, terminal
 * flag, the weights and (seed, counter, row_offset + b): not on the batch, the grid or the rows around it; two calls on the same inputs
 * give the same bits.  A batch cut into pieces gives the same rows when each piece passes the index of its first row as row_offset.
 * Workspace: pmg_td3_target_work_floats = batch * A floats when a second critic is given and d_next_action is NULL (a~ has to be kept for
 * critic 2 somewhere), else 0 (d_work may then be NULL); < 0 for an invalid actor or batch.
 * PMG_E_INVALID, with nothing launched: everything pmg_td_target_device rejects, for every given network; critic2 not shaped
 * Dx + A -> ... -> 1 (its depth and hidden widths may differ from critic 1's); sigma negative or not finite; noise_clip negative or NaN
 * (+inf: the noise is not clipped); row_offset < 0; a wrong struct_size; d_work NULL or work_floats too small where the figure above is
 * positive; a float pointer off 4 bytes.  batch == 0 is a successful no-op. */
typedef struct pmg_td3_target {
    int32_t struct_size, reserved;
    float gamma;                         /* finite, >= 0 */
    float clip_lo, clip_hi;              /* as pmg_td_target */
    float sigma;                         /* >= 0, finite; 0: no noise term at all, no draw is made */
    float noise_clip;                    /* c >= 0, +inf allowed (no clip of the noise); NaN invalid */
    uint64_t seed, counter;              /* the draws are a pure function of (seed, counter, row_offset + b, j) */
    int64_t row_offset;                  /* >= 0: index of row 0 in the caller's numbering of samples */
    int64_t batch;
    const float* d_x_next; int64_t x_stride;   /* [B, Dx] at x_stride floats from row to row */
    const float* d_reward;               /* [B] */
    const uint8_t* d_terminal;           /* [B] or NULL; non-zero: no bootstrap term, t = r */
    float* d_y;                          /* [B]     required */
    float* d_q_min;                      /* [B]     or NULL: min(q1, q2) */
    float* d_q1; float* d_q2;            /* [B]     or NULL each (d_q2 is not written without a second critic) */
    float* d_next_action;                /* [B, A]  or NULL: a~, the smoothed action both critics saw */
    float* d_work; int64_t work_floats;  /* scratch, at least pmg_td3_target_work_floats(actor_target, critic2 != NULL, d_next_action != NULL, batch) */
} pmg_td3_target;
int64_t pmg_td3_target_work_floats(const pmg_mlp* actor_target, int has_critic2, int has_next_action, int64_t batch);
int pmg_td3_target_device(pmg_env* env, const pmg_mlp* actor_target, const pmg_mlp* critic1_target,
                          const pmg_mlp* critic2_target /* NULL: one critic */, const pmg_td3_target* td);

/* Soft actor-critic on the device (normative), float32 throughout: the stochastic head of a tanh-squashed Gaussian actor --
 * action, log-probability and the noise used -- on minibatch rows (pmg_sac_sample_device) and on the env's current rows
 * (pmg_sac_act_env_device), and the soft TD target in one call (pmg_sac_target_device).  All three are stream-ordered on the handle's
 * stream, sync nothing, write only their outputs (and d_work) and touch no state of the handle.  The critics' updates, the critics' input
 * gradient, the actor's backward, Adam and Polyak are the calls above, unchanged (the recipe: pybullet_multigoal_gym_amd/sac.py).
 *
 * A Gaussian actor is a pmg_mlp with width[L] == 2 A and out_activation == 0: units [0, A) are the mean, units [A, 2 A) the log standard
 * deviation; A <= 128, and for the target Dx + A <= 256.
 * The head, per (row b, unit j), z = the actor's layer chain above (bit-defined, unchanged), LOG2 = 0.69314718055994530942f,
 * HALF_LOG_2PI = 0.91893853320467274178f, TWO_PI = 6.28318530717958647692f:
 *   1. m = z[j];  ls = fminf(fmaxf(z[A + j], ls_lo), ls_hi).
 *   2. sample != 0: the draws are those of pmg_her_sample_device with s = (row_offset + b) * A + j as the sample index (env rows:
 *      s = g * A + j, g the global env index): key = mix(seed ^ mix(counter + GOLD)), r_k = mix(key + (4 s + k + 1) GOLD) >> 32,
 *      u1 = ((r_0 >> 8) + 1) 2^-24, u2 = (r_1 >> 8) 2^-24 (r_2 and r_3 are not used);  n = sqrtf(-2.f * logf(u1)) * cosf(TWO_PI * u2).
 *      sample == 0: no draw is made and n = +0.0f.
 *   3. sd = expf(ls);  u = fmaf(sd, n, m);  a = tanhf(u).
 *   4. w = -2.f * u;  sp = fmaxf(w, 0.f) + log1pf(expf(-fabsf(w)));  c2 = (LOG2 - u) - sp;
 *      l = fmaf(-2.f, c2, fmaf(-0.5f * n, n, -ls) - HALF_LOG_2PI)
 *      -- log N(u; m, sd) - log(1 - tanh^2 u) with the latter as 2 (log 2 - u - softplus(-2 u)): no cancellation where |a| rounds to 1.
 *   5. logp[b]: acc = +0.0f; acc = acc + l_j for j = 0 ... A-1 ascending: ONE chain.
 * z is bit-defined; n, a and logp go through the build's logf / sqrtf / cosf / expf / tanhf / log1pf and are held to a float64 model.  All
 * three entries return the same bits for the same (row, seed, counter, sample index).  A row's outputs depend on its own input row, the
 * weights and (seed, counter, row_offset + b): not on the batch, the grid or the rows around it.
 *
 * pmg_sac_sample_device: rows d_x [B, width[0]] at x_stride.  d_action [B, A] (a), d_logp [B], d_noise [B, A] (n), d_preact [B, 2 A] (z) may
 * each be NULL; d_action or d_logp must be given.
 * pmg_sac_act_env_device: the same on the rows pmg_policy_input_env_device writes, read in place from the packed rows of the last step /
 * reset as pmg_act_env_device reads them; B = num_envs, the sample index uses the global env index (row_offset = env_index_offset), so the
 * draws do not depend on how the envs are cut into handles.  The fields batch, row_offset, d_x and x_stride of the struct are not read.
 * The network must map Ds + Dg -> 2 * action_dim.  PMG_E_STATE before the first reset.
 *
 * pmg_sac_target_device, per row b, with the actor the caller passes (SAC: the online one), Dx = actor.width[0]:
 *   1. a'[j] and logp: the head on x'[b].
 *   2. q1 = critic1.out_activation(z_c1), z_c1 = critic 1's chain on the row x'[b] | a'; q2 likewise; qmin = fminf(q1, q2) (critic2 == NULL:
 *      qmin = q1), as pmg_td3_target_device.
 *   3. t = terminal ? r : fmaf(gamma, fmaf(-alpha, logp, qmin), r);  y = fminf(fmaxf(t, clip_lo), clip_hi).
 *   alpha: the struct's, or *d_alpha when d_alpha is given -- a device scalar read on the stream, so a learned temperature needs no host sync.
 * a' is kept for the critics in d_next_action when given, else in d_work: pmg_sac_target_work_floats = batch * A floats without
 * d_next_action, else 0 (d_work may then be NULL); < 0 for an invalid actor or batch.
 *
 * PMG_E_INVALID, with nothing launched and nothing written: everything pmg_mlp_forward_device / pmg_act_env_device /
 * pmg_td3_target_device reject; an actor whose width[L] is odd or whose out_activation != 0; a critic not shaped Dx + A -> ... -> 1;
 * ls_lo > ls_hi or either not finite; alpha negative or not finite; d_alpha off 4 bytes; row_offset < 0; no output requested (sample and
 * env entries: d_action and d_logp both NULL); d_work NULL or work_floats too small where the figure above is positive; a float pointer
 * off 4 bytes; a stride below its width; a wrong struct_size.  batch == 0 is a successful no-op. */
typedef struct pmg_sac_sample {
    int32_t struct_size, reserved;
    float ls_lo, ls_hi;                  /* finite, ls_lo <= ls_hi: the clamp of the log standard deviation */
    int32_t sample, reserved2;           /* 0: n = +0.0, no draw (the mode of the policy) */
    uint64_t seed, counter;              /* the draws are a pure function of (seed, counter, row_offset + b, j) */
    int64_t row_offset;                  /* >= 0: index of row 0 in the caller's numbering of samples */
    int64_t batch;
    const float* d_x; int64_t x_stride;            /* [B, width[0]] */
    float* d_action; int64_t action_stride;        /* [B, A]   or NULL: a */
    float* d_logp;                                 /* [B]      or NULL: log pi(a | x) */
    float* d_noise; int64_t noise_stride;          /* [B, A]   or NULL: n */
    float* d_preact; int64_t preact_stride;        /* [B, 2 A] or NULL: z */
} pmg_sac_sample;
int pmg_sac_sample_device(pmg_env* env, const pmg_mlp* actor, const pmg_sac_sample* s);
int pmg_sac_act_env_device(pmg_env* env, const pmg_mlp* actor, int state_kind, const pmg_sac_sample* s);
typedef struct pmg_sac_target {
    int32_t struct_size, reserved;
    float gamma;                         /* finite, >= 0 */
    float clip_lo, clip_hi;              /* as pmg_td_target */
    float alpha;                         /* >= 0, finite: the temperature (not read when d_alpha is given) */
    float ls_lo, ls_hi;                  /* as pmg_sac_sample */
    int32_t sample, reserved2;
    uint64_t seed, counter;
    int64_t row_offset;
    int64_t batch;
    const float* d_alpha;                /* NULL, or one float in device memory that replaces alpha */
    const float* d_x_next; int64_t x_stride;   /* [B, Dx] at x_stride floats from row to row */
    const float* d_reward;               /* [B] */
    const uint8_t* d_terminal;           /* [B] or NULL; non-zero: no bootstrap term, t = r */
    float* d_y;                          /* [B]     required */
    float* d_q_min;                      /* [B]     or NULL: min(q1, q2) */
    float* d_q1; float* d_q2;            /* [B]     or NULL each (d_q2 is not written without a second critic) */
    float* d_next_action;                /* [B, A]  or NULL: a', the action both critics saw */
    float* d_logp;                       /* [B]     or NULL: log pi(a' | x') */
    float* d_work; int64_t work_floats;  /* scratch, at least pmg_sac_target_work_floats(actor, d_next_action != NULL, batch) */
} pmg_sac_target;
int64_t pmg_sac_target_work_floats(const pmg_mlp* actor, int has_next_action, int64_t batch);
int pmg_sac_target_device(pmg_env* env, const pmg_mlp* actor, const pmg_mlp* critic1_target,
                          const pmg_mlp* critic2_target /* NULL: one critic */, const pmg_sac_target* td);

/* pmg_sac_policy_grad_device (normative), float32 throughout: the actor's half of a SAC update in one call -- the gradient of
 *   lscale * alpha * sum_b log pi(a_b | x_b) + gscale * sum_b min(Q1, Q2)(x_b, a_b),   a_b = tanh(m + exp(ls) n)  (reparameterised: n is held fixed)
 * with respect to the Gaussian actor's parameters, through the online critics.  SAC's actor loss mean(alpha log pi - min Q) is lscale = 1 / B,
 * gscale = -1 / B.  alpha: the struct's, or *d_alpha when d_alpha is given (as pmg_sac_target).  Stream-ordered on the handle's stream, syncs
 * nothing, writes only its outputs and d_work, touches no state of the handle; no network's weights are written.  Per row b,
 * Dx = actor.width[0], A = actor.width[L] / 2:
 *   1. z, n, sd = expf(ls), a, l_j and logp: the head above on x[b], sample index (row_offset + b) * A + j -- the bits pmg_sac_sample_device returns
 *      for the same (seed, counter, row_offset + b).  d_action receives a, d_logp receives logp.
 *   2. q_c = critic c's chain and output activation on the row x[b] | a.  d_q1 / d_q2 receive them.
 *   3. ga_c[j]: critic c's backward as in pmg_policy_grad_device step 3, with the constant head gscale and input gradients only.
 *   4. ga = (critic2 == NULL || q1 <= q2) ? ga1 : ga2: a tie takes critic 1, a NaN on either side critic 2.  d_gaction receives ga.
 *   5. e = lscale * alpha (one multiply);  t = fmaf(-a, a, 1.f);  d = ga * t;  sdn = sd * n;
 *        g_mu[j] = fmaf(2.f * e, a, d)
 *        g_ls[j] = (z[A + j] >= ls_lo && z[A + j] <= ls_hi) ? fmaf(e, fmaf(2.f * a, sdn, -1.f), d * sdn) : +0.0f
 *      -- the clamp's derivative, inclusive at both ends as torch.clamp's is; a NaN z takes the +0.0 branch.  d_ghead receives g_mu | g_ls.
 *   6. delta_{L-1} = g_mu | g_ls, and from there dW_l and db_l of the actor exactly as pmg_mlp_grad_device (chunk_rows == 0) or
 *      pmg_mlp_grad_chunked_device (chunk_rows >= 2, even) forms them from d_gout = g.
 * grads == NULL: steps 5 and 6 run only when d_ghead is given, and the actor's part of the workspace is not touched.  Without grads, d_gaction
 * and d_ghead no critic backward runs; with d_action / d_logp alone no critic runs at all.
 * A row's outputs do not depend on the batch it is in; dW and db depend on the row order and on chunk_rows and on nothing else; nothing depends
 * on the grid; two calls on the same inputs give the same bits.  A <= 128 and Dx + A <= 256.
 * Workspace: pmg_sac_policy_grad_work_floats = the actor's pmg_mlp_grad_work_floats (chunk_rows == 0) or pmg_mlp_grad_chunked_work_floats figure,
 * laid out as those calls lay it out, + batch * A without d_action (a has to be kept for the critics somewhere) + batch * A with a second
 * critic (ga1 while critic 2 runs); < 0 for an invalid actor, batch or chunk_rows.  Between the head and step 5, sd n and the predicate of a
 * (row, unit) are kept where its delta_{L-1} will be (without grads: in d_ghead).
 * PMG_E_INVALID, with nothing launched and nothing written: everything pmg_sac_target_device rejects in the networks, alpha, d_alpha, ls_lo,
 * ls_hi and row_offset; everything pmg_policy_grad_device rejects in grads, strides, pointers, chunk_rows, d_work and work_floats; gscale or
 * lscale not finite; grads and every output NULL; a wrong struct_size.  batch == 0 is a successful no-op that leaves grads untouched. */
typedef struct pmg_sac_policy_grad {
    int32_t struct_size, reserved;
    float gscale;                        /* finite; -1 / B for -mean min(Q1, Q2) */
    float lscale;                        /* finite; 1 / B for alpha * mean log pi; 0: no entropy term */
    float alpha;                         /* >= 0, finite: the temperature (not read when d_alpha is given) */
    float ls_lo, ls_hi;                  /* as pmg_sac_sample */
    int32_t sample, reserved2;
    uint64_t seed, counter;
    int64_t row_offset;
    int64_t batch;
    const float* d_alpha;                /* NULL, or one float in device memory that replaces alpha */
    const float* d_x; int64_t x_stride;            /* [B, Dx] */
    const pmg_mlp_params* grads;         /* the ACTOR's dW / db, overwritten; NULL: the outputs below only */
    float* d_action; int64_t action_stride;        /* [B, A]   or NULL: a */
    float* d_logp;                                 /* [B]      or NULL: log pi(a | x) */
    float* d_q1; float* d_q2;                      /* [B]      or NULL each (d_q2 is not written without a second critic) */
    float* d_gaction; int64_t gaction_stride;      /* [B, A]   or NULL: ga of the critic with the smaller Q */
    float* d_ghead; int64_t ghead_stride;          /* [B, 2 A] or NULL: g_mu | g_ls, the gradient at the actor's outputs */
    float* d_work; int64_t work_floats;  /* scratch, at least pmg_sac_policy_grad_work_floats(actor, d_action != NULL, critic2 != NULL, batch, chunk_rows) */
} pmg_sac_policy_grad;
int64_t pmg_sac_policy_grad_work_floats(const pmg_mlp* actor, int has_action, int has_critic2, int64_t batch, int64_t chunk_rows);
int pmg_sac_policy_grad_device(pmg_env* env, const pmg_mlp* actor, const pmg_mlp* critic1, const pmg_mlp* critic2 /* NULL: one critic */,
                               const pmg_sac_policy_grad* g, int64_t chunk_rows);

/* pmg_sac_alpha_device (normative), float32: one Adam step on SAC's log-temperature from the log-probabilities of a batch.
 * d_state: four caller-owned floats in device memory, log_alpha | m | v | alpha; pass d_state + 3 as d_alpha to pmg_sac_target_device and
 * pmg_sac_policy_grad_device.  Stream-ordered on the handle's stream, syncs nothing, writes d_state only.
 *   1. p_t = +0.0f;  p_t = p_t + logp[b] over the rows b = t (mod 256) in ascending order, t = 0 ... 255.
 *   2. total = +0.0f;  total = total + p_t, t ascending: ONE chain.  Bit-defined; nothing depends on a grid.
 *   3. g = -(total / (float)batch + target_entropy), the quotient correctly rounded: the gradient of -log_alpha * mean(logp + target_entropy).
 *   4. pmg_mlp_adam_device's step on log_alpha with g (m and v beside it), bit for bit.
 *   5. alpha = expf(log_alpha) into d_state[3].
 * PMG_E_INVALID, with nothing launched: batch <= 0; target_entropy not finite; everything pmg_mlp_adam_device rejects in lr, the betas, eps and
 * step; d_logp or d_state NULL or off 4 bytes; a wrong struct_size. */
typedef struct pmg_sac_alpha {
    int32_t struct_size, reserved;
    float target_entropy;                /* finite; SAC: -A */
    float lr, beta1, beta2, eps;         /* as pmg_adam */
    int32_t reserved2;
    int64_t step;                        /* t >= 1 */
    int64_t batch;
    const float* d_logp;                 /* [B] */
    float* d_state;                      /* [4]: log_alpha, m, v, alpha */
} pmg_sac_alpha;
int pmg_sac_alpha_device(pmg_env* env, const pmg_sac_alpha* a);

/* ---- PPO on whole rollouts (normative), float32 unless said otherwise ----
 * Four calls beside the existing ones: generalised advantage estimation, the advantage normaliser, the clipped-surrogate gradient of a Gaussian
 * actor and the statistics of a minibatch.  Each is stream-ordered on the handle's stream, syncs nothing, writes only its outputs (and d_work)
 * and touches no state of the handle; each is bit-reproducible and independent of the grid and of the number of CUs.
 *
 * pmg_gae_device: T steps of N envs.  Every table is addressed by (t, i) at ptr + t * time_stride + i * env_stride (floats; either stride may
 * be negative, an input's may be 0), so a time-major [T, N] table (strides N, 1), an env-major [N, T] one (1, T) and a column of recorded
 * packed rows read in place (strides N * packed_dim, packed_dim) are the same call.  One chain per env, t = T-1 ... 0:
 *     gl = gamma * lambda                                  (one float multiply, on the host)
 *     nv = terminal[t, i] != 0 ? +0.0f : value_next[t, i];   delta = fmaf(gamma, nv, reward[t, i]) - value[t, i]
 *     adv[t, i] = (t == T-1 || cut[t, i] != 0) ? delta : fmaf(gl, adv[t+1, i], delta);    ret[t, i] = adv[t, i] + value[t, i]
 * d_value_next[t, i] is V of the state that step t led to BEFORE any reset: with a [T+1, N] value table of states that were never reset it is
 * d_value + time_stride; after pmg_reset_done_device the row t+1 of such a table holds the NEW episode's first state, and the caller passes
 * the values of the recorded successor rows as a table of its own.  All episodes of this library end by TimeLimit, so the packed row's `done`
 * column is a truncation: it is d_cut (the chain restarts, the bootstrap stays), never d_terminal.  d_terminal (no bootstrap) may be the
 * goal_achieved column if the learner wants that.  d_cut NULL: no boundary but the last step; d_terminal NULL: every step bootstraps.  An
 * env's results depend on its own column only.  The outputs overlap no input and not each other (not checked).
 * PMG_E_INVALID, nothing launched: gamma or lambda outside [0, 1] or NaN; steps < 0 or envs < 0; steps * envs >= 2^31; d_reward, d_value,
 * d_value_next or d_adv NULL; a pointer off 4 bytes; an output (d_adv, d_ret) whose strides could make two (t, i) alias: with a = |time_stride|,
 * b = |env_stride| the call requires a >= 1 when steps > 1, b >= 1 when envs > 1, and a >= envs * b or b >= steps * a (sufficient, not
 * necessary: a table with gaps in both directions is refused); a wrong struct_size.  steps == 0 or envs == 0 is a successful no-op. */
typedef struct pmg_gae {
    int32_t struct_size, reserved;
    float gamma, lambda;                 /* each in [0, 1] */
    int64_t steps, envs;                 /* T, N */
    const float* d_reward; int64_t reward_time_stride, reward_env_stride;
    const float* d_value; int64_t value_time_stride, value_env_stride;                      /* V(s_t) */
    const float* d_value_next; int64_t value_next_time_stride, value_next_env_stride;       /* V of the state step t led to, before any reset */
    const float* d_cut; int64_t cut_time_stride, cut_env_stride;                            /* or NULL; != 0: an episode ends behind step t */
    const float* d_terminal; int64_t terminal_time_stride, terminal_env_stride;             /* or NULL; != 0: no bootstrap */
    float* d_adv; int64_t adv_time_stride, adv_env_stride;                                  /* required */
    float* d_ret; int64_t ret_time_stride, ret_env_stride;                                  /* or NULL: adv + value */
} pmg_gae;
int pmg_gae_device(pmg_env* env, const pmg_gae* g);

/* pmg_adv_stats_device / pmg_adv_apply_device: the advantage normaliser over M = count contiguous floats, one workgroup of 256 threads for the
 * statistics.  Thread k accumulates in DOUBLE s = s + x, q = fma(x, x, q) over the elements b = k (mod 256) in ascending order from +0.0;
 * thread 0 adds the 256 partial sums in ascending order from +0.0 (S, Q), then
 *     mean = S / M;   var = max((Q - S * mean) / (M - ddof), 0);   d_stats[0] = (float)mean;   d_stats[1] = (float)(1 / (sqrt(var) + (double)eps))
 * mean is bit-defined (x * x is exact in double, so the fma is one rounding either way); d_stats[1] goes through the build's double sqrt and
 * division (and S * mean may be fused into the subtraction) and is held to a float64 model.  eps == 0 with var == 0 gives +inf.
 * apply: y[b] = (x[b] - d_stats[0]) * d_stats[1], two roundings; d_y == d_x is allowed; the statistics are read from device memory on the
 * stream, so nothing waits between the two calls.
 * PMG_E_INVALID, nothing launched: count < 0; ddof not 0 or 1; count >= 1 and count - ddof < 1; eps negative or not finite; a NULL pointer or
 * one off 4 bytes; a wrong struct_size.  count == 0 is a successful no-op that writes nothing. */
typedef struct pmg_adv_stats {
    int32_t struct_size, ddof;           /* ddof: 0 (population) or 1 (sample) */
    float eps;                           /* finite, >= 0 */
    int32_t reserved;
    int64_t count;                       /* M */
    const float* d_x;                    /* [M] */
    float* d_stats;                      /* [2]: mean, 1 / (std + eps) */
} pmg_adv_stats;
int pmg_adv_stats_device(pmg_env* env, const pmg_adv_stats* s);
int pmg_adv_apply_device(pmg_env* env, const float* d_x, int64_t count, const float* d_stats, float* d_y);

/* pmg_ppo_policy_grad_device: the gradient of PPO's clipped surrogate and entropy bonus
 *     pscale * sum_b min(rho_b adv_b, clamp(rho_b, clip_lo, clip_hi) adv_b) + escale * sum_b sum_j ls_bj
 * with respect to the parameters of a Gaussian actor (above: width[L] == 2 A, out_activation == 0, A <= 128) in one call; PPO's loss
 * -mean(min(...)) - ent_coef * mean(entropy) is pscale = -1 / B, escale = -ent_coef / B.  rho is the ratio of the new policy to the one that drew
 * the action, both evaluated at the recorded pre-squash sample u; the tanh correction and log 2 pi are the same on both sides and are left
 * out.  The entropy is that of the PRE-SQUASH Gaussian, sum_j ls_j + const: a squashed policy's entropy has no closed form, and the usual
 * estimate -log pi(a) would need a fresh sample; the bonus therefore acts on the log-stds inside the clamp and on nothing else.
 * Per row b (x[b]; zo[b] [2 A] and n[b] [A]: the d_preact and d_noise that pmg_sac_act_env_device / pmg_sac_sample_device returned when the
 * action was drawn; adv[b]), per unit j < A:
 *   1. z = the actor's layer chain on x[b] (bit-defined, unchanged);  m = z[j];  ls = fminf(fmaxf(z[A + j], ls_lo), ls_hi);
 *      inr = z[A + j] >= ls_lo && z[A + j] <= ls_hi.
 *   2. lso = fminf(fmaxf(zo[A + j], ls_lo), ls_hi);  u = fmaf(expf(lso), n[j], zo[j]) -- the very u of the head above, the env received tanhf(u);
 *      lo_j = fmaf(-0.5f * n[j], n[j], -lso).
 *   3. isd = expf(-ls);  w = (u - m) * isd;  ln_j = fmaf(-0.5f * w, w, -ls).
 *   4. lr: acc = +0.0f; acc = acc + (ln_j - lo_j) for j ascending, ONE chain;  rho = expf(lr).
 *   5. clipped = (adv > 0 && rho > clip_hi) || (adv < 0 && rho < clip_lo);  k = clipped ? +0.0f : (pscale * adv) * rho.  That is the surrogate's
 *      gradient everywhere but on ties, where both branches of the min carry the same gradient.  A NaN adv or rho is not clipped.
 *   6. g_mu[j] = k * (w * isd);  g_ls[j] = inr ? fmaf(k, fmaf(w, w, -1.f), escale) : +0.0f  (the clamp's derivative as in pmg_sac_policy_grad).
 *   7. delta_{L-1} = g_mu | g_ls, and from there dW_l and db_l of the actor exactly as pmg_mlp_grad_device (chunk_rows == 0) or
 *      pmg_mlp_grad_chunked_device (chunk_rows >= 2, even) forms them from d_gout = g.
 * d_ratio [B] (rho), d_logratio [B] (lr), d_clipped [B] bytes (0 / 1) and d_ghead [B, 2 A] (g_mu | g_ls) may each be NULL.  grads == NULL:
 * these alone are produced (steps 6 and 7 run only for d_ghead) and d_work is not touched and may be NULL.  z is bit-defined; lr, rho and g
 * go through the build's expf and are held to a float32 model.  A row's outputs do not depend on the batch it is in; dW and db depend on the
 * row order and on chunk_rows and on nothing else; two calls on the same inputs give the same bits.
 * Workspace: pmg_ppo_policy_grad_work_floats = the actor's pmg_mlp_grad_work_floats (chunk_rows == 0) or pmg_mlp_grad_chunked_work_floats
 * figure, laid out as those calls lay it out; < 0 for an invalid actor, batch or chunk_rows.  Between steps 3 and 6, w and isd of a (row, unit)
 * are kept where its delta_{L-1} will be (without grads: in d_ghead).
 * PMG_E_INVALID, nothing launched and nothing written: everything pmg_sac_sample_device rejects in the actor, ls_lo and ls_hi; pscale or escale
 * not finite; clip_lo or clip_hi NaN, clip_lo < 0 or clip_lo > clip_hi (clip_hi may be +inf); batch < 0; d_x, d_preact_old, d_noise or d_adv NULL;
 * grads and every output NULL; everything pmg_policy_grad_device rejects in grads, chunk_rows, d_work and work_floats (with grads); a float
 * pointer off 4 bytes; a stride below its width; a wrong struct_size.  batch == 0 is a successful no-op that leaves grads untouched. */
typedef struct pmg_ppo_policy_grad {
    int32_t struct_size, reserved;
    float pscale;                        /* finite; -1 / B for -mean of the clipped surrogate */
    float escale;                        /* finite; -ent_coef / B; 0: no entropy bonus */
    float clip_lo, clip_hi;              /* 1 - eps, 1 + eps as floats; 0 <= clip_lo <= clip_hi */
    float ls_lo, ls_hi;                  /* as pmg_sac_sample: the clamp the action was drawn with */
    int64_t batch;
    const float* d_x; int64_t x_stride;                      /* [B, Dx] */
    const float* d_preact_old; int64_t preact_old_stride;    /* [B, 2 A]: zo */
    const float* d_noise; int64_t noise_stride;              /* [B, A]:   n */
    const float* d_adv;                                      /* [B] */
    const pmg_mlp_params* grads;         /* the actor's dW / db, overwritten; NULL: the outputs below only */
    float* d_ratio;                      /* [B] or NULL: rho */
    float* d_logratio;                   /* [B] or NULL: lr */
    uint8_t* d_clipped;                  /* [B] or NULL: 1 where the clip cut the gradient */
    float* d_ghead; int64_t ghead_stride;                    /* [B, 2 A] or NULL: g_mu | g_ls */
    float* d_work; int64_t work_floats;  /* scratch with grads, at least pmg_ppo_policy_grad_work_floats(actor, batch, chunk_rows) */
} pmg_ppo_policy_grad;
int64_t pmg_ppo_policy_grad_work_floats(const pmg_mlp* actor, int64_t batch, int64_t chunk_rows);
int pmg_ppo_policy_grad_device(pmg_env* env, const pmg_mlp* actor, const pmg_ppo_policy_grad* g, int64_t chunk_rows);

/* pmg_ppo_stats_device: what a PPO learner logs and stops early on, from the per-row outputs above and the advantages of a minibatch; one
 * workgroup, the two-level chain of pmg_sac_alpha_device for each of four float32 sums (thread t over the rows b = t (mod 256) ascending from
 * +0.0, thread 0 over the 256 partial sums ascending from +0.0):
 *     d_stats[0] = mean of (rho - 1.f) - lr                                     the approximate KL divergence old || new
 *     d_stats[1] = mean of (clipped != 0 ? 1.f : 0.f)                           the clip fraction
 *     d_stats[2] = mean of fminf(rho * adv, fminf(fmaxf(rho, clip_lo), clip_hi) * adv)    the clipped surrogate
 *     d_stats[3] = mean of lr
 * each quotient total / (float)batch correctly rounded.  Bit-defined.
 * PMG_E_INVALID, nothing launched: batch <= 0; a NULL pointer; a float pointer off 4 bytes; clip_lo or clip_hi as refused above; a wrong
 * struct_size. */
typedef struct pmg_ppo_stats {
    int32_t struct_size, reserved;
    float clip_lo, clip_hi;
    int64_t batch;
    const float* d_ratio; const float* d_logratio; const uint8_t* d_clipped; const float* d_adv;   /* [B] each */
    float* d_stats;                      /* [4]: approximate KL, clip fraction, surrogate, mean log-ratio */
} pmg_ppo_stats;
int pmg_ppo_stats_device(pmg_env* env, const pmg_ppo_stats* s);

/* Checkpoint / test hooks (no reference equivalent).
 * state: [N, state_dim] float32, layout documented in DESIGN.md (with use_curriculum the row ends with 16
 * floats of curriculum state: prob[5] generated[5] goal_step; chest tasks prob[6] generated[6] goal_step). */
int pmg_get_state(pmg_env* env, float* state);
int pmg_set_state(pmg_env* env, const float* state);   /* also refreshes the observation part of PMG_BUF_PACKED */
/* Host-injected goal / object poses for seed-parity tests (replaces the RNG
 * draws of _generate_goal for the masked envs).  goals: [N, goal_dim].  PMG_E_INVALID for the chest tasks (their goal
 * is the chest: no static target; goal row [0..2] holds the door joint position, velocity and motor latch). */
int pmg_set_goal(pmg_env* env, const uint8_t* mask, const float* goals);

/* Multi-step task bookkeeping (block_stack / block_rearrange), per env -- the reference keeps one copy per
 * env object.  The desired goal of these tasks is re-derived from the current block poses at every observation
 * (kuka_multi_step_base_env.py:309-312): blocks beyond the active level are "already at their goal".
 *
 * Replaces: KukaBulletMultiBlockEnv.set_sub_goal (kuka_multi_step_base_env.py:154-177): sub-goal index for
 * the masked envs (mask NULL = all), -1 = the final goal, as after reset; refreshes desired_goal in the output
 * buffers.  Valid indices: [-1, num_block), or [-1, 2*num_block) with grip_informed_goal (pick, place, pick, ...);
 * chest tasks: [-1, num_steps) with num_steps = num_block + 1, or 2*num_block + 1 (chest_push) / 3*num_block + 1
 * (chest_pick_and_place) with grip_informed_goal -- index 0 is "open the door" (kuka_multi_step_envs.py:238-242,
 * 388-392).  PMG_E_STATE unless the handle was created with task_decomposition. */
int pmg_set_sub_goal(pmg_env* env, const uint8_t* mask, int32_t sub_goal_ind);
/* Replaces: activate_curriculum_update / deactivate_curriculum_update (kuka_multi_step_base_env.py:142-152). */
int pmg_curriculum_update(pmg_env* env, int32_t enabled);
/* Curriculum read-out, any pointer may be NULL: level [N] (last_curriculum_level), goal_step [N]
 * (curriculum_goal_step = level*25 + 50), prob [N, num_curriculum] (curriculum_prob), generated [N, num_curriculum]
 * (num_generated_goals_per_curriculum); num_curriculum = num_block, or num_block + 1 for the chest tasks. */
int pmg_curriculum_read(pmg_env* env, int32_t* level, int32_t* goal_step, float* prob, float* generated);

/* Multi-GPU (no reference equivalent): one handle per
 * rank; the only exchange is an RCCL all-gather of PMG_BUF_PACKED. */
int pmg_comm_unique_id(uint8_t id[128]);
int pmg_comm_init(pmg_env* env, int rank, int nranks, const uint8_t id[128]);
/* d_gathered: [nranks*N, packed_dim] device buffer (caller-owned). */
int pmg_allgather_packed(pmg_env* env, float* d_gathered);
/* The same, OVERLAPPED with the next step (the collective must not add to the step).  pmg_comm_overlap(env, 1)
 * double-buffers the packed rows: step t writes buffer t & 1 (PMG_BUF_PACKED / pmg_device_ptr then names the buffer of the
 * LAST step: query it per step, or read the gathered rows).  pmg_allgather_packed_async enqueues ncclAllGather on the handle's own
 * communication stream behind the rows of the last step (+ the masked resets enqueued since); the step stream does not wait
 * for it -- only the step that writes the same row buffer again (two steps later) does.  d_gathered must stay untouched
 * until pmg_allgather_wait: host != 0 blocks the caller until the LAST enqueued all-gather has completed, host == 0 makes the
 * handle's stream wait for it (for consumers enqueued on pmg_stream()).  A caller that consumes gather t while gather t + 1 is in
 * flight alternates two d_gathered buffers.  pmg_sync() also waits for the communication stream. */
int pmg_comm_overlap(pmg_env* env, int32_t enabled);
int pmg_allgather_packed_async(pmg_env* env, float* d_gathered);
int pmg_allgather_wait(pmg_env* env, int32_t host);

/* The data-parallel learner (normative): the rank-ordered merge of gradients and of the normalisers' totals, so that an
 * update does not depend on how many GPUs its batch was spread over.  Every entry below is stream-ordered on the handle's stream, syncs
 * nothing, writes only its outputs and its workspace and touches no env state.  The collectives (pmg_allgather_device,
 * pmg_mlp_grad_allreduce_device, pmg_mlp_adam_allreduce_device, pmg_norm_update_ranks_device, pmg_norm_update_env_ranks_device) are one
 * ncclAllGather of floats each (doubles travel as pairs of floats) and every rank must call them in the same order; they return PMG_E_STATE
 * before pmg_comm_init, and PMG_E_STATE while pmg_comm_overlap is enabled: the overlapped all-gather runs on the handle's communication
 * stream, and two streams must not issue collectives on one communicator -- switch the overlap off around a learner update.
 *
 * Gradients.  R ranks hold B_local rows each, B_local even and equal on all ranks; the global batch is the ranks' rows concatenated in rank
 * order.  Each rank runs any gradient call as it is -- pmg_mlp_grad_device, pmg_policy_grad_device or pmg_sac_policy_grad_device, the single
 * chain (chunk_rows = 0 / none) -- with the caller's gscale = ... / B_global: G_r.  After the merge
 *   dW[i] = (...((G_0[i] + G_1[i]) + G_2[i]) ... + G_{R-1}[i]):  float32 additions in ascending rank order, one rounding each, starting from
 * G_0[i] ITSELF, not from +0.0.  That is, by the definition of pmg_mlp_grad_chunked_device, bit for bit (zeros by value) what
 * pmg_mlp_grad_chunked_device(chunk_rows = B_local) returns on the concatenated batch on one GPU.  A rank that chunks locally with
 * chunk_rows = r, r dividing B_local, gets a function of the rows, their order, r and R alone; it is not claimed equal to any single-GPU
 * call.  Every rank ends with the same bits.
 *
 * P = pmg_mlp_param_floats(shape) = the sum over the layers of width[l] * width[l + 1] + (d_bias[l] ? width[l + 1] : 0); a FLAT gradient is
 * the network's tensors in that order -- weight 0, bias 0, weight 1, ... -- as P contiguous floats.  `shape` supplies the widths and which
 * layers have a bias; its pointers are not dereferenced.  A SLOT is one rank's flat gradient; slot r lies at d_slots + r * slot_stride.
 *   pmg_mlp_params_pack_device:  the tensors of src -> d_flat [P].
 *   pmg_mlp_params_merge_device: the sum above over nslots >= 1 slots -> the tensors of out (one slot: a bit copy).
 *   pmg_mlp_adam_merge_device:   the same sum handed to pmg_mlp_adam_device's step in one sweep: m and v bit for bit those of
 *     pmg_mlp_params_merge_device followed by pmg_mlp_adam_device, p held to the same float64 model.  The summed gradient goes to
 *     grad_out when given and is never stored otherwise.
 *   pmg_mlp_grad_allreduce_device: pack, all-gather, merge back into grads, in place.
 *   pmg_mlp_adam_allreduce_device: pack, all-gather, fused merge + Adam; grads keeps THIS rank's gradient.
 *   Both take a workspace of pmg_mlp_allreduce_work_floats(env, shape) = (nranks + 1) * P floats (nranks = 1 before pmg_comm_init): this
 *   rank's flat gradient in front, the gathered slots behind it.
 *   pmg_allgather_device: count floats of every rank into d_gathered [nranks * count], rank order; count == 0 is a successful no-op.  A
 *   data-parallel SAC learner gathers its logp rows with it and runs pmg_sac_alpha_device on the global [B] on every rank.
 * PMG_E_INVALID, with nothing launched: a bad network shape; a NULL or misaligned tensor where the shape has one (a bias pointer where the
 * shape has no bias is ignored); d_flat, d_slots, d_work, d_src or d_gathered NULL or off 4 bytes; nslots < 1; slot_stride < P; work_floats
 * too small; count < 0; everything pmg_mlp_adam_device rejects in pmg_adam; a wrong struct_size.
 *
 * Normaliser.  A collective update with batch_local rows on every rank (equal on all ranks) cuts the rows at the chunk of the GLOBAL batch,
 *   chunk = 64 * ceil(R * batch_local / (64 * 1022)),
 * and batch_local must be a multiple of it unless R == 1 (PMG_E_INVALID otherwise, nothing launched).  Row 0 of rank r is global row
 * r * batch_local; for the _env_ form num_envs is batch_local and env_index_offset must equal rank * num_envs (PMG_E_INVALID otherwise).
 * Each rank forms its partial rows as pmg_norm_update_device does; gathered in rank order, [R][batch_local / chunk][2 D + 1] doubles, they are
 * exactly the partial rows of the unsharded update in index order, and the same merge adds them onto the totals and re-derives mean / std /
 * inv_std.  Totals and derived values are therefore bit-equal to ONE pmg_norm_update_device on the concatenated rows, and equal on every
 * rank.  The gathered rows live in a buffer of the handle, allocated at the first collective update (a later larger one re-sizes it, which
 * waits for the stream once) and freed by pmg_destroy.  PMG_E_INVALID: what pmg_norm_update_device rejects; d_rows off 4 bytes;
 * batch_local < 0; batch_local == 0 is a successful no-op on every rank.  PMG_E_STATE (_env_ form): before the first reset. */
int pmg_comm_info(pmg_env* env, int32_t* rank, int32_t* nranks);   /* of pmg_comm_init (either may be NULL); PMG_E_STATE before it */
int pmg_allgather_device(pmg_env* env, const float* d_src, int64_t count, float* d_gathered);
int64_t pmg_mlp_param_floats(const pmg_mlp* shape);   /* < 0: invalid network */
int pmg_mlp_params_pack_device(pmg_env* env, const pmg_mlp* shape, const pmg_mlp_params* src, float* d_flat);
int pmg_mlp_params_merge_device(pmg_env* env, const pmg_mlp* shape, const float* d_slots, int64_t slot_stride, int64_t nslots,
                                const pmg_mlp_params* out);
int pmg_mlp_adam_merge_device(pmg_env* env, const pmg_mlp* shape, const pmg_mlp_params* param, const float* d_slots, int64_t slot_stride,
                              int64_t nslots, const pmg_mlp_params* grad_out /* or NULL */, const pmg_mlp_params* m, const pmg_mlp_params* v,
                              const pmg_adam* a);
int64_t pmg_mlp_allreduce_work_floats(const pmg_env* env, const pmg_mlp* shape);   /* < 0: invalid network */
int pmg_mlp_grad_allreduce_device(pmg_env* env, const pmg_mlp* shape, const pmg_mlp_params* grads, float* d_work, int64_t work_floats);
int pmg_mlp_adam_allreduce_device(pmg_env* env, const pmg_mlp* shape, const pmg_mlp_params* param, const pmg_mlp_params* grads,
                                  const pmg_mlp_params* m, const pmg_mlp_params* v, const pmg_adam* a, float* d_work, int64_t work_floats);
int pmg_norm_update_ranks_device(pmg_env* env, int which, const float* d_rows, int64_t row_stride, int64_t batch_local, const uint8_t* d_mask);
int pmg_norm_update_env_ranks_device(pmg_env* env, const uint8_t* d_mask);

/* Device-buffer helpers for callers that have no HIP runtime of their own (e.g. a numpy-only
 * host): allocate / free / copy on the handle's device and stream.  Callers that already own
 * device memory (a torch tensor's data_ptr()) pass those pointers directly instead. */
int pmg_device_alloc(pmg_env* env, uint64_t bytes, void** d_ptr);
int pmg_device_free(pmg_env* env, void* d_ptr);
int pmg_upload(pmg_env* env, void* d_dst, const void* h_src, uint64_t bytes);   /* synchronous at return */
int pmg_download(pmg_env* env, void* h_dst, const void* d_src, uint64_t bytes); /* synchronous at return */
/* device to device, stream-ordered on the handle's stream (no host sync): how such a caller records PMG_BUF_PACKED rows of
 * a step into its own episode table (pmg_her_sample_device) */
int pmg_device_copy(pmg_env* env, void* d_dst, const void* d_src, uint64_t bytes);

/* Kernel timing of the most recent *_device call sequence: HIP events on the
 * handle's stream bracket every step kernel; returns average ms per launch
 * over the launches since the last pmg_timing_reset(). */
int pmg_timing_reset(pmg_env* env);
/* bracket only every n-th batched step with events (default 1: every step).  An event is a barrier packet with a
 * completion signal: the kernel behind it starts ~6 us after the one in front has drained (measured, rocprofv3 kernel
 * trace), against ~0.1 us between kernels that follow each other directly -- two events per step were 12 us of a 1.0 ms
 * reach step.  The untimed steps run the identical launch sequence. */
int pmg_timing_every(pmg_env* env, int n);
int pmg_timing_read(pmg_env* env, double* avg_step_kernel_ms, int64_t* launches);
/* the same launches: shortest / average / longest (any pointer may be NULL).  A batched step lasts as long as its slowest
 * wavefront, so the spread shows how often envs with finger x table / object contacts were in the batch. */
int pmg_timing_stats(pmg_env* env, double* min_ms, double* avg_ms, double* max_ms, int64_t* launches);
/* HIP events around every pmg_allgather_packed since the last pmg_timing_reset(): average / longest ms on this rank's
 * stream (it includes the wait for the slowest peer to arrive) and the count (any pointer may be NULL). */
int pmg_comm_timing(pmg_env* env, double* avg_ms, double* max_ms, int64_t* launches);

/* The per-env MT19937 streams (625 words each: state + cursor), [N, 625] uint32: with pmg_get_state / pmg_set_state a
 * checkpoint that resumes with the SAME future goals, orders and curriculum draws (no reference equivalent).  The
 * curriculum-update switch is host state: restore it with pmg_curriculum_update. */
int pmg_get_rng(pmg_env* env, uint32_t* words);
int pmg_set_rng(pmg_env* env, const uint32_t* words);

#ifdef __cplusplus
}
#endif
#endif /* PMG_H */
