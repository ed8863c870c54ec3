/*
 * pmg_api.cpp -- host side of the C ABI declared in include/pmg.h.
 *
 * Owns the device arrays of N environments on one MI355X, seeds them like
 * gym.utils.seeding.np_random (sha512 -> MT19937 init_by_array), launches
 * the step / reset kernels on its own HIP stream, times the step kernel with
 * HIP events, and exchanges the packed observation shard with RCCL.
 * There is no CPU fallback: without a HIP device pmg_create fails.
 */
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pmg.h"
#include "../../include/pmg_sha512_const.h"
#include "pmg_launch.h"

namespace {

char g_create_err[512] = "";

constexpr int EVENT_POOL = 2048;

struct Seeder { /* gym 0.17.3 seeding.np_random + numpy RandomState.seed(int list) */
    static inline uint64_t rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
    static void sha512(const unsigned char* msg, size_t len, unsigned char out[64])
    {
        static const uint64_t K[80] = PMG_SHA512_K;
        uint64_t h[8] = PMG_SHA512_H0;
        size_t total = ((len + 17 + 127) / 128) * 128;
        std::vector<unsigned char> buf(total, 0);
        memcpy(buf.data(), msg, len);
        buf[len] = 0x80;
        uint64_t bits = (uint64_t)len * 8;
        for (int i = 0; i < 8; i++) buf[total - 1 - i] = (unsigned char)(bits >> (8 * i));
        for (size_t off = 0; off < total; off += 128) {
            uint64_t w[80];
            for (int i = 0; i < 16; i++) {
                uint64_t v = 0;
                for (int b = 0; b < 8; b++) v = (v << 8) | buf[off + 8 * i + b];
                w[i] = v;
            }
            for (int i = 16; i < 80; i++) {
                uint64_t s0 = rotr(w[i - 15], 1) ^ rotr(w[i - 15], 8) ^ (w[i - 15] >> 7);
                uint64_t s1 = rotr(w[i - 2], 19) ^ rotr(w[i - 2], 61) ^ (w[i - 2] >> 6);
                w[i] = w[i - 16] + s0 + w[i - 7] + s1;
            }
            uint64_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
            for (int i = 0; i < 80; i++) {
                uint64_t t1 = hh + (rotr(e, 14) ^ rotr(e, 18) ^ rotr(e, 41)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
                uint64_t t2 = (rotr(a, 28) ^ rotr(a, 34) ^ rotr(a, 39)) + ((a & b) ^ (a & c) ^ (b & c));
                hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
            }
            h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
        }
        for (int i = 0; i < 8; i++)
            for (int b = 0; b < 8; b++) out[8 * i + b] = (unsigned char)(h[i] >> (56 - 8 * b));
    }
    /* fills mt[0..623] and mt[624] = 624 (index) */
    static void seed(uint32_t* mt, uint64_t seed)
    {
        char txt[32];
        int n = snprintf(txt, sizeof(txt), "%llu", (unsigned long long)seed);
        unsigned char dig[64];
        sha512((const unsigned char*)txt, (size_t)n, dig);
        uint32_t key[2];
        for (int w = 0; w < 2; w++)
            key[w] = (uint32_t)dig[4 * w] | ((uint32_t)dig[4 * w + 1] << 8) | ((uint32_t)dig[4 * w + 2] << 16) | ((uint32_t)dig[4 * w + 3] << 24);
        int klen = key[1] ? 2 : 1;
        mt[0] = 19650218u;
        for (int i = 1; i < 624; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        int i = 1, j = 0;
        for (int k = 624; k; k--) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
            i++; j++;
            if (i >= 624) { mt[0] = mt[623]; i = 1; }
            if (j >= klen) j = 0;
        }
        for (int k = 623; k; k--) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
            i++;
            if (i >= 624) { mt[0] = mt[623]; i = 1; }
        }
        mt[0] = 0x80000000u;
        mt[624] = 624u;
    }
};

/* A grow-only block of device scratch.  reserve() keeps a block that is large enough; otherwise it waits for the handle's stream
 * (queued work may still read the old block), frees and allocates.  No destructor: pmg_destroy releases the blocks in its order. */
struct Scratch {
    void* p = nullptr;
    size_t cap = 0;                   /* bytes */
    int reserve(pmg_env* e, size_t bytes, const char* who, const char* what);
    void release() { (void)hipFree(p); p = nullptr; cap = 0; }
    float* f32() const { return (float*)p; }
};

}  // namespace

struct pmg_env {
    pmg_config cfg;
    pmg_dims dims;
    pmg::EnvParams P;
    int nb;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;       /* second queue: the full-store list of the multi-block tasks runs beside the main one */
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    float* d_actions = nullptr;       /* staging for host-buffer pmg_step */
    unsigned char* d_mask = nullptr;
    float* h_packed = nullptr;        /* pinned */
    float* h_actions = nullptr;       /* pinned */
    /* staging of the synchronous host variants (pmg_compute_reward, pmg_norm_update, pmg_policy_input; never two at a time):
     * two inputs, one output, one mask / flag block */
    Scratch st_a, st_b, st_out, st_flag;
    hipEvent_t ev_a[EVENT_POOL], ev_b[EVENT_POOL];
    hipEvent_t cv_a[EVENT_POOL], cv_b[EVENT_POOL];   /* the same around every all-gather */
    int cv_n = 0;
    double cv_ms = 0.0, cv_max = 0.0;
    long long cv_launches = 0;
    int ev_n = 0;
    int ev_every = 1;                 /* events around every ev_every-th batched step (pmg_timing_every) */
    long long step_count = 0;
    long long plans = 0;              /* batched steps planned so far (parity of the longest-first threshold words) */
    double ev_ms = 0.0, ev_min = 0.0, ev_max = 0.0;
    long long ev_launches = 0;
    bool ever_reset = false;
    int packed = 1;                   /* reach: contact-free envs four per wavefront (PMG_PACKED=0 switches it off) */
    int two_wave = 1;                 /* reach: the two-wavefront kernel for steps with contact-prone envs (PMG_REACH_TWO_WAVES=0: never) */
    pmgx::WaveRec* wave_trace = nullptr;   /* PMG_WAVE_TRACE=1 at creation: [2 N] records of the reach step's wavefronts (PMG_BUF_WAVE_TRACE) */
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    /* overlapped all-gather (pmg_comm_overlap): the packed rows are double-buffered -- step t writes out2[t & 1], its all-gather
     * reads that buffer on the communication stream while step t + 1 computes and writes the OTHER one; step t + 2, which
     * writes out2[t & 1] again, is the one that waits for gather t */
    bool overlap = false;
    float* out2[2] = {nullptr, nullptr};
    int out_phase = 0;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_rows[2] = {nullptr, nullptr}, ev_gdone[2] = {nullptr, nullptr};
    bool gpending[2] = {false, false};
    int last_gather = -1;
    /* running normalisers (pmg_norm_*): observation, policy_state, goal.  One device block each:
     * totals double[2 D + 1] | partials double[PMG_NORM_MAX_PARTS][2 D + 1] | derived float[3 D] */
    struct Norm { int D = 0; double* tot = nullptr; double* part = nullptr; float* der = nullptr; } norm[3];
    float norm_eps = 0.01f, norm_clip_in = 200.f, norm_clip_out = 5.f;
    Scratch her_idx;                  /* e, t, f of a pmg_her_sample_device batch whose caller passed no d_index: kept until a larger batch */
    Scratch norm_gather;              /* the partial rows of all ranks of a collective normaliser update, [nranks][parts][2 D + 1] doubles: first use */
    char err[512] = "";
};

#ifndef PMG_LPT_PERMILLE_DEFAULT
#define PMG_LPT_PERMILLE_DEFAULT 400   /* the slowest 40 % of the fast-path list lead it (profiles/r06_lpt_quantile_sweep.txt) */
#endif

namespace {

int fail(pmg_env* e, int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(e ? e->err : g_create_err, 512, fmt, ap);
    va_end(ap);
    return code;
}
#define HIP_TRY(e, call)                                                                             \
    do {                                                                                             \
        hipError_t rc_ = (call);                                                                     \
        if (rc_ != hipSuccess) return fail(e, PMG_E_DEVICE, "%s -> %s", #call, hipGetErrorString(rc_)); \
    } while (0)

int Scratch::reserve(pmg_env* e, size_t bytes, const char* who, const char* what)
{
    if (bytes <= cap) return PMG_OK;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    release();
    if (hipMalloc(&p, bytes) != hipSuccess) { p = nullptr; return fail(e, PMG_E_NOMEM, "%s: no memory for %zu bytes of %s", who, bytes, what); }
    cap = bytes;
    return PMG_OK;
}
/* the staging blocks of the host variant `who`, in bytes */
int stage(pmg_env* e, const char* who, size_t a, size_t b, size_t out, size_t flag)
{
    const char* what = "host staging";
    if (int rc = e->st_a.reserve(e, a, who, what)) return rc;
    if (int rc = e->st_b.reserve(e, b, who, what)) return rc;
    if (int rc = e->st_out.reserve(e, out, who, what)) return rc;
    return e->st_flag.reserve(e, flag, who, what);
}
/* the normaliser `which` of `who`'s caller, or its state normaliser (observation or policy_state); null with the error set */
pmg_env::Norm* norm_of(pmg_env* e, int which, const char* who)
{
    if (which >= 0 && which <= 2) return &e->norm[which];
    fail(e, PMG_E_INVALID, "%s: normaliser %d is none of PMG_NORM_OBSERVATION / _POLICY_STATE / _GOAL", who, which);
    return nullptr;
}
pmg_env::Norm* state_norm_of(pmg_env* e, int state_kind, const char* who)
{
    if (state_kind == PMG_NORM_OBSERVATION || state_kind == PMG_NORM_POLICY_STATE) return &e->norm[state_kind];
    fail(e, PMG_E_INVALID, "%s: state_kind %d is neither PMG_NORM_OBSERVATION nor PMG_NORM_POLICY_STATE", who, state_kind);
    return nullptr;
}

int fill_dims(const pmg_config* c, pmg_dims* d, int* nb_out)
{
    memset(d, 0, sizeof(*d));
    int jo = c->joint_control ? 7 : 0;
    d->num_envs = c->num_envs;
    switch (c->task) {
    case PMG_TASK_REACH: d->action_dim = jo ? 7 : 3; d->observation_dim = 3 + jo; d->policy_state_dim = 3 + jo; d->goal_dim = 3; break;
    case PMG_TASK_PUSH: case PMG_TASK_SLIDE: d->action_dim = jo ? 7 : 3; d->observation_dim = 20 + jo; d->policy_state_dim = 7 + jo; d->goal_dim = 3; break;
    case PMG_TASK_PICK_AND_PLACE: d->action_dim = jo ? 8 : 4; d->observation_dim = 20 + jo; d->policy_state_dim = 7 + jo; d->goal_dim = 3; break;
    case PMG_TASK_BLOCK_STACK:
    case PMG_TASK_BLOCK_REARRANGE:
        if (c->num_block < 1 || c->num_block > 5) return -1;
        if (c->use_curriculum && (c->num_block < 2 || c->task_decomposition)) return -1; /* kuka_multi_step_base_env.py:123,131 */
        if (c->task_decomposition && c->task != PMG_TASK_BLOCK_STACK) return -1;          /* kuka_multi_step_envs.py:159 */
        d->action_dim = (jo ? 7 : 3) + (c->task == PMG_TASK_BLOCK_STACK ? 1 : 0); d->observation_dim = 8 + 16 * c->num_block + jo;
        d->policy_state_dim = 4 + 3 * c->num_block + jo; d->goal_dim = 3 * c->num_block;
        if (c->grip_informed_goal) {
            if (c->task != PMG_TASK_BLOCK_STACK) return -1; /* kuka_multi_step_envs.py:158 */
            d->goal_dim += 4;                               /* tip xyz + finger width, kuka_multi_step_base_env.py:300-304 */
        }
        break;
    case PMG_TASK_CHEST_PUSH:
    case PMG_TASK_CHEST_PICK_AND_PLACE: {
        /* kuka_multi_step_base_env.py:283-304: the multi-block layout + door joint pos / vel + 3 key points x (xyz, vel);
         * goals lead with the door state; num_curriculum = num_block + 1 (kuka_multi_step_envs.py:253,402) */
        if (c->num_block < 1 || c->num_block > 5 || (c->use_curriculum && c->task_decomposition)) return -1;
        const int gr = c->task == PMG_TASK_CHEST_PICK_AND_PLACE ? 1 : 0;
        d->action_dim = (jo ? 7 : 3) + gr; d->observation_dim = 8 + 16 * c->num_block + jo + 20;
        d->policy_state_dim = 4 + 3 * c->num_block + jo + 19; d->goal_dim = 1 + 3 * c->num_block;
        if (c->grip_informed_goal) d->goal_dim += gr ? 4 : 3;
        break;
    }
    default: return -1;
    }
    bool multi = c->task == PMG_TASK_BLOCK_STACK || c->task == PMG_TASK_BLOCK_REARRANGE || c->task == PMG_TASK_CHEST_PUSH ||
                 c->task == PMG_TASK_CHEST_PICK_AND_PLACE;
    if (!multi && (c->use_curriculum || c->task_decomposition || c->grip_informed_goal)) return -1;
    int nb = c->task == PMG_TASK_REACH ? 0 : (multi ? c->num_block : 1);
    *nb_out = nb;
    d->state_dim = 64 + 13 * nb + (c->use_curriculum ? pmg::CURR_DIM : 0);
    d->packed_dim = d->observation_dim + d->policy_state_dim + 2 * d->goal_dim + 3;
    return 0;
}

/* workspace constants: kuka.py:35-51, kuka_single_step_base_env.py:48-56 */
void fill_params(pmg_env* e)
{
    pmg::EnvParams& P = e->P;
    const pmg_config& c = e->cfg;
    int t = c.task;
    P.n_envs = c.num_envs; P.task = t; P.nb = e->nb;
    P.chest = t == PMG_TASK_CHEST_PUSH ? 0 : (t == PMG_TASK_CHEST_PICK_AND_PLACE ? 1 : -1);
    P.grasping = (t == PMG_TASK_PICK_AND_PLACE || t == PMG_TASK_BLOCK_STACK || t == PMG_TASK_CHEST_PICK_AND_PLACE);
    P.has_obj = (t != PMG_TASK_REACH);
    P.in_air = (t == PMG_TASK_REACH || t == PMG_TASK_PICK_AND_PLACE || t == PMG_TASK_BLOCK_STACK || t == PMG_TASK_CHEST_PICK_AND_PLACE);
    P.joint_control = c.joint_control; P.binary_reward = c.binary_reward; P.max_steps = c.max_episode_steps;
    P.random_order = c.random_order;
    P.multi = (t == PMG_TASK_BLOCK_STACK || t == PMG_TASK_BLOCK_REARRANGE || P.chest >= 0);
    P.curriculum = c.use_curriculum; P.curriculum_update = 0;
    P.decomposition = c.task_decomposition; P.grip_goal = c.grip_informed_goal;
    {
        double total = c.num_goals_to_generate > 0 ? (double)c.num_goals_to_generate : 1e6;
        P.goals_per_curriculum = e->nb > 0 ? floor(total / (P.chest >= 0 ? e->nb + 1 : e->nb)) : total; /* kuka_multi_step_base_env.py:139 */
    }
    P.adim = e->dims.action_dim; P.odim = e->dims.observation_dim; P.pdim = e->dims.policy_state_dim;
    P.gdim = e->dims.goal_dim; P.packed = e->dims.packed_dim;
    P.thr = c.distance_threshold;
    bool on_table = (t == PMG_TASK_PUSH || t == PMG_TASK_SLIDE || t == PMG_TASK_BLOCK_REARRANGE || t == PMG_TASK_CHEST_PUSH); /* kuka_multi_step_envs.py:169,399 */
    double range = 0.15, trange = 0.15;
    if (t == PMG_TASK_SLIDE) { range = 0.1; trange = 0.2; } /* kuka_single_step_base_env.py:66-69 */
    if (P.chest >= 0) range = 0.1;                          /* kuka_multi_step_envs.py:251,400 */
    P.tip_init[0] = -0.52; P.tip_init[1] = 0.0; P.tip_init[2] = 0.25;
    if (on_table) P.tip_init[2] = 0.175 + 0.001;
    const double hi[3] = {-0.37, 0.20, 0.55}, lo[3] = {-0.67, -0.20, 0.175};
    for (int a = 0; a < 3; a++) {
        P.ee_hi[a] = (float)hi[a]; P.ee_lo[a] = (float)lo[a];
        P.obj_lo[a] = P.tip_init[a] - range; P.obj_hi[a] = P.tip_init[a] + range;
        P.tgt_lo[a] = P.tip_init[a] - trange; P.tgt_hi[a] = P.tip_init[a] + trange;
    }
    P.obj_lo[0] += 0.03; P.obj_hi[0] -= 0.03;
    P.tgt_lo[0] += 0.03; P.tgt_hi[0] -= 0.03;
    P.tgt_lo[2] = lo[2];
    if (P.chest >= 0) { /* kuka_multi_step_base_env.py:102-105 */
        P.obj_lo[0] += 0.05; P.obj_hi[0] += 0.05;
        P.obj_lo[1] -= 0.05; P.obj_hi[1] += 0.05;
    }
    P.obj_z = 0.175;
    const float th[3] = PMG_TABLE_HALF;
    P.table_c[0] = -0.52f; P.table_c[1] = 0.f; P.table_c[2] = 0.08f;
    for (int a = 0; a < 3; a++) P.table_h[a] = th[a];
    P.table_mu = (float)PMG_TABLE_FRICTION;
    if (t == PMG_TASK_SLIDE) { /* long table (table_long.urdf), kuka_single_step_base_env.py:53-56; the puck itself is pmg::ObjT<true> */
        const float lt[3] = PMG_LONG_TABLE_HALF;
        P.tgt_lo[0] -= 0.4; P.tgt_hi[0] -= 0.4;
        P.table_c[0] = -0.70f;
        for (int a = 0; a < 3; a++) P.table_h[a] = lt[a];
        P.table_mu = (float)PMG_LONG_TABLE_FRICTION;
        P.obj_z = 0.170;
    }
}

int upload_seeds(pmg_env* e)
{
    int N = e->cfg.num_envs;
    std::vector<uint32_t> mt((size_t)N * 625);
    for (int i = 0; i < N; i++)
        Seeder::seed(mt.data() + (size_t)i * 625, e->cfg.seed_base + e->cfg.seed_stride * (uint64_t)(i + e->cfg.env_index_offset));
    HIP_TRY(e, hipMemcpyAsync(e->P.rng, mt.data(), mt.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return PMG_OK;
}

void unpack(const pmg_env* e, const float* packed, float* obs, float* pol, float* ag, float* dg, float* reward,
            uint8_t* ga, uint8_t* done)
{
    const pmg_dims& d = e->dims;
    int N = d.num_envs, S = d.packed_dim;
    for (int i = 0; i < N; i++) {
        const float* r = packed + (size_t)i * S;
        if (obs) memcpy(obs + (size_t)i * d.observation_dim, r, sizeof(float) * d.observation_dim);
        r += d.observation_dim;
        if (pol) memcpy(pol + (size_t)i * d.policy_state_dim, r, sizeof(float) * d.policy_state_dim);
        r += d.policy_state_dim;
        if (ag) memcpy(ag + (size_t)i * d.goal_dim, r, sizeof(float) * d.goal_dim);
        r += d.goal_dim;
        if (dg) memcpy(dg + (size_t)i * d.goal_dim, r, sizeof(float) * d.goal_dim);
        r += d.goal_dim;
        if (reward) reward[i] = r[0];
        if (ga) ga[i] = r[1] != 0.f;
        if (done) done[i] = r[2] != 0.f;
    }
}

void drain_events(pmg_env* e)
{
    for (int i = 0; i < e->ev_n; i++) {
        float ms = 0.f;
        (void)hipEventSynchronize(e->ev_b[i]);
        if (hipEventElapsedTime(&ms, e->ev_a[i], e->ev_b[i]) == hipSuccess) {
            if (e->ev_launches == 0 || ms < e->ev_min) e->ev_min = ms;
            if (e->ev_launches == 0 || ms > e->ev_max) e->ev_max = ms;
            e->ev_ms += ms; e->ev_launches++;
        }
    }
    e->ev_n = 0;
}

void drain_comm_events(pmg_env* e)
{
    for (int i = 0; i < e->cv_n; i++) {
        float ms = 0.f;
        (void)hipEventSynchronize(e->cv_b[i]);
        if (hipEventElapsedTime(&ms, e->cv_a[i], e->cv_b[i]) == hipSuccess) {
            if (ms > e->cv_max) e->cv_max = ms;
            e->cv_ms += ms; e->cv_launches++;
        }
    }
    e->cv_n = 0;
}

}  // namespace

extern "C" {

const char* pmg_last_error(const pmg_env* e) { return e ? e->err : g_create_err; }

int pmg_create(const pmg_config* cfg, pmg_env** out)
{
    if (!cfg || !out) return fail(nullptr, PMG_E_INVALID, "pmg_create: null argument");
    if (cfg->struct_size != (int32_t)sizeof(pmg_config)) return fail(nullptr, PMG_E_INVALID, "pmg_create: struct_size %d != %zu", cfg->struct_size, sizeof(pmg_config));
    if (cfg->num_envs < 1) return fail(nullptr, PMG_E_INVALID, "pmg_create: num_envs must be >= 1");
    if (cfg->max_episode_steps < 1) return fail(nullptr, PMG_E_INVALID, "pmg_create: max_episode_steps must be >= 1");
    pmg_dims dims;
    int nb = 0;
    if (fill_dims(cfg, &dims, &nb) != 0)
        return fail(nullptr, PMG_E_INVALID, "pmg_create: unsupported task %d / num_block %d", cfg->task, cfg->num_block);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, PMG_E_DEVICE, "pmg_create: no HIP device visible (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, PMG_E_INVALID, "pmg_create: device %d out of range (%d visible)", cfg->device, ndev);
    pmg_env* e = new pmg_env();
    e->cfg = *cfg;
    e->dims = dims;
    e->nb = nb;
    auto bail = [&](int code) { snprintf(g_create_err, sizeof(g_create_err), "%s", e->err); pmg_destroy(e); return code; };
#define CREATE_TRY(call)                                                                         \
    do {                                                                                         \
        hipError_t rc_ = (call);                                                                 \
        if (rc_ != hipSuccess) { fail(e, PMG_E_DEVICE, "%s -> %s", #call, hipGetErrorString(rc_)); return bail(PMG_E_DEVICE); } \
    } while (0)
    CREATE_TRY(hipSetDevice(cfg->device));
    CREATE_TRY(hipStreamCreate(&e->stream));
    CREATE_TRY(hipStreamCreate(&e->side));
    CREATE_TRY(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    CREATE_TRY(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    size_t N = (size_t)cfg->num_envs;
    fill_params(e);
    CREATE_TRY(hipMalloc((void**)&e->P.hot, N * pmg::HOT_DIM * sizeof(float)));
    CREATE_TRY(hipMalloc((void**)&e->P.cold, N * pmg::COLD_DIM * sizeof(float)));
    CREATE_TRY(hipMalloc((void**)&e->P.goal, N * pmg::GOAL_DIM * sizeof(float)));
    if (cfg->use_curriculum) CREATE_TRY(hipMalloc((void**)&e->P.curr, N * pmg::CURR_DIM * sizeof(float)));
    CREATE_TRY(hipMalloc((void**)&e->P.blocks, N * pmg::BLOCK_DIM * (nb ? nb : 1) * sizeof(float)));
    CREATE_TRY(hipMalloc((void**)&e->P.rng, N * 625 * sizeof(uint32_t)));
    CREATE_TRY(hipMalloc((void**)&e->P.out, N * dims.packed_dim * sizeof(float)));
    CREATE_TRY(hipMalloc((void**)&e->P.sched, pmgx::Sched::words(N) * sizeof(int)));
    if (const char* pk = getenv("PMG_PACKED")) e->packed = atoi(pk) != 0;
    if (const char* tw = getenv("PMG_REACH_TWO_WAVES")) e->two_wave = atoi(tw) != 0;
    {   /* 1.5 wavefronts per SIMD of this device: how many one-env wavefronts the plan may add to a step */
        int cus = 256;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) != hipSuccess || cus <= 0) cus = 256;
        e->P.wave_budget = 6 * cus;
        /* measured on chest_push-4 / chest_pick_and_place-4 x 4096 (tools/chest_exp.sh): 6.5 cm / 6.4 cm put 40-65 % of a
         * random-policy batch on the full-layout list (0.337 M); 5 cm / 2 cm: 20 %, no redo, 0.388 / 0.416 M */
        /* block_stack-4 (tools/near_exp.sh): 6.5 cm puts up to 8 % of the batch on the full-store list, 4.5 cm 1.5 %, no redo
         * either way: 0.549 -> 0.566 M; the one-object tasks are insensitive (0.04 starts to redo) */
        e->P.near_r = e->P.chest >= 0 ? 0.05f : (e->nb > 1 ? 0.045f : 0.065f);
        e->P.chest_reach = 0.02f;
        if (const char* nr = getenv("PMG_NEAR_R")) e->P.near_r = (float)atof(nr);   /* (tuning experiments) */
        if (const char* cr = getenv("PMG_CHEST_REACH")) e->P.chest_reach = (float)atof(cr);
        e->P.list0_prio = -1;
        /* fingers-down class of the one-object tasks: to the one-env list for pick_and_place, packed for push / slide -- by task,
         * never by batch statistics (results must not depend on how a job is sharded; EnvParams::fd_div) */
        e->P.fd_div = e->cfg.task == PMG_TASK_PICK_AND_PLACE ? -1 : 0;
        if (const char* fd = getenv("PMG_FD_DIV")) e->P.fd_div = atoi(fd);
        if (const char* wb = getenv("PMG_WAVE_BUDGET")) e->P.wave_budget = atoi(wb);
        e->P.env_cycles = nullptr;
        /* Longest first on the fast-path list of the many-body tasks (4096 one-env wavefronts on 2048 slots run in two
         * rounds: a long wavefront that starts in the second one is the tail of the step).  The predictor is the env's own
         * wavefront time in the PREVIOUS step (cycles / 64, kept per env: 8 bytes); envs beyond the threshold lead the list
         * (plan_class).  Thresholds by measurement (PMG_LPT_CYCLES sweep 0 / 60 / 70 / 85 / 100 k): chest_push-4 0.42 -> 0.46 M
         * and chest_pick_and_place-4 0.57 -> 0.58 M at 85 k / 70 k, block_stack-4 0.79 -> 0.80 M at 60 k; block_rearrange
         * loses (0.70 -> 0.61 M: there the fingers-down grouping it replaces IS the better order) and keeps it off.
         * Results do not depend on the order of a launch list, only the schedule does */
        /* Round 6: the threshold is no longer a shader-clock count tuned per task on one part at one batch size (85 000 / 70 000 / 60 000):
         * the plan derives it every step as the cycle count above which the slowest lpt_permille / 1000 of the fast-path envs lay in
         * the last step (pmg_k_plan_count's histogram, pmg_k_plan_scatter).  PMG_LPT_PERMILLE overrides the share, PMG_LPT_CYCLES > 0
         * forces a constant, PMG_LPT_CYCLES=0 switches the order off */
        e->P.lpt_thresh = 0;
        /* share of the list that leads it, measured (profiles/r06_lpt_quantile_sweep.txt): chest tasks flat between 350 and 450 (0.403 /
         * 0.545 M, the tuned constants' 0.402 / 0.547 M), block_stack best at 450 (0.804 M; constant 60 000: 0.818 M), block_rearrange loses
         * with any (0.69 -> 0.60 M: its fingers-down grouping is the better order) and keeps the rule off */
        e->P.lpt_permille = dims.num_envs < 4096 ? 0 : ((e->cfg.task == PMG_TASK_CHEST_PUSH || e->cfg.task == PMG_TASK_CHEST_PICK_AND_PLACE) ? PMG_LPT_PERMILLE_DEFAULT :
                                                        (e->cfg.task == PMG_TASK_BLOCK_STACK ? PMG_LPT_PERMILLE_DEFAULT + 50 : 0));
        e->P.lpt_parity = 0;
        e->P.lpt_state = nullptr;
        if (const char* lq = getenv("PMG_LPT_PERMILLE")) e->P.lpt_permille = atoi(lq);
        if (const char* lt = getenv("PMG_LPT_CYCLES")) { e->P.lpt_thresh = atoi(lt); if (e->P.lpt_thresh <= 0) e->P.lpt_permille = 0; }
        const char* ec = getenv("PMG_ENV_CYCLES");
        if (e->nb > 1 && e->P.lpt_permille > 0 && e->P.lpt_thresh <= 0) {
            CREATE_TRY(hipMalloc((void**)&e->P.lpt_state, (2 + pmg::LPT_BINS) * sizeof(int)));
            CREATE_TRY(hipMemset(e->P.lpt_state, 0, (2 + pmg::LPT_BINS) * sizeof(int)));
        }
        /* PMG_WAVE_TRACE=1 (diagnostics): one record per wavefront of the reach step kernels and the redo pass, 2 N of them, filled with
         * 0xFF bytes in front of every step; the records take their contact counts from env_cycles, which is kept with them */
        const char* wt = getenv("PMG_WAVE_TRACE");
        const bool trace = wt && atoi(wt) != 0;
        if (trace) {
            CREATE_TRY(hipMalloc((void**)&e->wave_trace, 2 * N * sizeof(pmgx::WaveRec)));
            CREATE_TRY(hipMemset(e->wave_trace, 0xFF, 2 * N * sizeof(pmgx::WaveRec)));
        }
        if (trace || (ec && atoi(ec) != 0) || ((e->P.lpt_thresh > 0 || e->P.lpt_permille > 0) && e->nb > 1)) {
            CREATE_TRY(hipMalloc((void**)&e->P.env_cycles, 2 * N * sizeof(int)));
            CREATE_TRY(hipMemset(e->P.env_cycles, 0, 2 * N * sizeof(int)));
        }
        if (const char* pr = getenv("PMG_LIST0_PRIO")) e->P.list0_prio = atoi(pr);
    }
    CREATE_TRY(hipMalloc((void**)&e->d_actions, N * dims.action_dim * sizeof(float)));
    CREATE_TRY(hipMalloc((void**)&e->d_mask, N));
    CREATE_TRY(hipHostMalloc((void**)&e->h_packed, N * dims.packed_dim * sizeof(float)));
    CREATE_TRY(hipHostMalloc((void**)&e->h_actions, N * dims.action_dim * sizeof(float)));
    for (int i = 0; i < EVENT_POOL; i++) { CREATE_TRY(hipEventCreate(&e->ev_a[i])); CREATE_TRY(hipEventCreate(&e->ev_b[i])); }
    for (int i = 0; i < EVENT_POOL; i++) { CREATE_TRY(hipEventCreate(&e->cv_a[i])); CREATE_TRY(hipEventCreate(&e->cv_b[i])); }
    /* initial state: rest pose kuka.py:27, blocks parked below the floor */
    {
        static const float rest0[7] = {0.f, -0.5592432f, 0.f, 1.733180f, 0.f, -0.8501557f, 0.f};
        std::vector<float> cold(N * pmg::COLD_DIM, 0.f), blk(N * pmg::BLOCK_DIM * (nb ? nb : 1), 0.f);
        for (size_t i = 0; i < N; i++) {
            memcpy(&cold[i * pmg::COLD_DIM], rest0, sizeof(rest0));
            for (int b = 0; b < nb; b++) { float* o = &blk[(i * nb + b) * pmg::BLOCK_DIM]; o[2] = -3.f; o[6] = 1.f; }
        }
        CREATE_TRY(hipMemcpy(e->P.cold, cold.data(), cold.size() * sizeof(float), hipMemcpyHostToDevice));
        CREATE_TRY(hipMemcpy(e->P.blocks, blk.data(), blk.size() * sizeof(float), hipMemcpyHostToDevice));
        {   /* identity launch schedule: all envs in the contact-prone list */
            std::vector<int> sc(pmgx::Sched::words(N), 0);   /* (redo list empty, nothing promoted) */
            const pmgx::Sched S{sc.data(), (int)N};
            S.count(0) = (int)N;
            for (size_t i = 0; i < N; i++) S.list(0)[i] = (int)i;
            CREATE_TRY(hipMemcpy(e->P.sched, sc.data(), sc.size() * sizeof(int), hipMemcpyHostToDevice));
        }
        CREATE_TRY(hipMemset(e->P.hot, 0, N * pmg::HOT_DIM * sizeof(float)));
        CREATE_TRY(hipMemset(e->P.goal, 0, N * pmg::GOAL_DIM * sizeof(float)));
        if (e->P.curr) { /* start with the easiest goal as the only possible one (kuka_multi_step_base_env.py:133) */
            std::vector<float> cs(N * pmg::CURR_DIM, 0.f);
            const int NC = e->P.chest >= 0 ? 6 : 5;   /* row: prob[NC] | generated[NC] | goal_step */
            for (size_t i = 0; i < N; i++) { cs[i * pmg::CURR_DIM] = 1.f; cs[i * pmg::CURR_DIM + 2 * NC] = 50.f; }
            CREATE_TRY(hipMemcpy(e->P.curr, cs.data(), cs.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        CREATE_TRY(hipMemset(e->P.out, 0, N * dims.packed_dim * sizeof(float)));
    }
    for (int w = 0; w < 3; w++) {   /* normalisers start empty: n = 0, mean 0, std = inv_std = 1 */
        pmg_env::Norm& nm = e->norm[w];
        nm.D = w == PMG_NORM_OBSERVATION ? dims.observation_dim : (w == PMG_NORM_POLICY_STATE ? dims.policy_state_dim : dims.goal_dim);
        const size_t P = 2 * (size_t)nm.D + 1, nd = P * (1 + PMG_NORM_MAX_PARTS);
        CREATE_TRY(hipMalloc((void**)&nm.tot, nd * sizeof(double) + 3 * (size_t)nm.D * sizeof(float)));
        nm.part = nm.tot + P;
        nm.der = (float*)(nm.tot + nd);
        std::vector<float> der(3 * (size_t)nm.D, 1.f);
        for (int c = 0; c < nm.D; c++) der[c] = 0.f;
        CREATE_TRY(hipMemset(nm.tot, 0, nd * sizeof(double)));
        CREATE_TRY(hipMemcpy(nm.der, der.data(), der.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (upload_seeds(e) != PMG_OK) return bail(PMG_E_DEVICE);
    {   /* the tuning / experiment switches this library reads from the environment change its schedule (never its results' meaning):
         * a stray one in a user's shell -- PMG_PACKED=0 halves the throughput -- must not go unnoticed: ONE line on stderr per handle */
        static const char* const kSwitches[] = {"PMG_PACKED", "PMG_REACH_TWO_WAVES", "PMG_NEAR_R", "PMG_CHEST_REACH", "PMG_FD_DIV", "PMG_WAVE_BUDGET",
                                                "PMG_LPT_CYCLES", "PMG_LPT_PERMILLE", "PMG_ENV_CYCLES", "PMG_WAVE_TRACE", "PMG_LIST0_PRIO", "PMG_LIST0_FIRST", "PMG_PLAN_TWO_PASS",
                                                "PMG_REWARD_GENERIC"};
        std::string active;
        for (const char* name : kSwitches)
            if (const char* v = getenv(name)) { active += active.empty() ? "" : " "; active += name; active += "="; active += v; }
        if (!active.empty()) fprintf(stderr, "[libpmg_hip] environment overrides active for this handle: %s\n", active.c_str());
    }
    *out = e;
    return PMG_OK;
}

void pmg_destroy(pmg_env* e)
{
    if (!e) return;
    (void)hipSetDevice(e->cfg.device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->comm_stream) (void)hipStreamSynchronize(e->comm_stream);   /* an overlapped all-gather in flight reads out2[] through e->comm */
    if (e->comm) ncclCommDestroy(e->comm);
    (void)hipFree(e->P.hot); (void)hipFree(e->P.cold); (void)hipFree(e->P.goal);
    (void)hipFree(e->P.curr); (void)hipFree(e->P.blocks); (void)hipFree(e->P.rng);
    if (e->out2[1]) { (void)hipFree(e->out2[0]); (void)hipFree(e->out2[1]); }
    else (void)hipFree(e->P.out);
    (void)hipFree(e->P.sched); (void)hipFree(e->P.env_cycles); (void)hipFree(e->wave_trace); (void)hipFree(e->P.lpt_state);
    (void)hipFree(e->d_actions); (void)hipFree(e->d_mask);
    for (int w = 0; w < 3; w++) (void)hipFree(e->norm[w].tot);
    for (Scratch* b : {&e->st_a, &e->st_b, &e->st_out, &e->st_flag, &e->her_idx, &e->norm_gather}) b->release();
    if (e->h_packed) (void)hipHostFree(e->h_packed);
    if (e->h_actions) (void)hipHostFree(e->h_actions);
    for (int i = 0; i < EVENT_POOL; i++) { if (e->ev_a[i]) (void)hipEventDestroy(e->ev_a[i]); if (e->ev_b[i]) (void)hipEventDestroy(e->ev_b[i]); }
    for (int i = 0; i < EVENT_POOL; i++) { if (e->cv_a[i]) (void)hipEventDestroy(e->cv_a[i]); if (e->cv_b[i]) (void)hipEventDestroy(e->cv_b[i]); }
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    if (e->side) { (void)hipStreamSynchronize(e->side); (void)hipStreamDestroy(e->side); }
    if (e->comm_stream) { (void)hipStreamSynchronize(e->comm_stream); (void)hipStreamDestroy(e->comm_stream); }
    for (int b = 0; b < 2; b++) { if (e->ev_rows[b]) (void)hipEventDestroy(e->ev_rows[b]); if (e->ev_gdone[b]) (void)hipEventDestroy(e->ev_gdone[b]); }
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

int pmg_device_count(void)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) return 0;
    return ndev;
}

int pmg_get_dims(const pmg_env* e, pmg_dims* out)
{
    if (!e || !out) return PMG_E_INVALID;
    *out = e->dims;
    return PMG_OK;
}

int pmg_seed(pmg_env* e, uint64_t base, uint64_t stride)
{
    if (!e) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    e->cfg.seed_base = base;
    e->cfg.seed_stride = stride;
    return upload_seeds(e);
}

/* Overlapped all-gather: a gather of the CURRENT row buffer may still be reading it on the communication stream (the step that
 * wrote it was gathered, the next step has not been queued yet).  Whatever writes rows into that buffer between two steps -- a
 * reset, set_sub_goal, the reset of nobody behind pmg_set_state -- goes behind that gather; the gathered table of step t then
 * holds step t's rows and nothing of the reset that followed it (bench.py --lockstep resets right behind the gather). */
static int rows_writer_waits_for_gather(pmg_env* e)
{
    if (e->overlap && e->gpending[e->out_phase]) {
        HIP_TRY(e, hipStreamWaitEvent(e->stream, e->ev_gdone[e->out_phase], 0));
        e->gpending[e->out_phase] = false;
    }
    return PMG_OK;
}

int pmg_reset_device(pmg_env* e, const uint8_t* d_mask)
{
    if (!e) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    if (int rc = rows_writer_waits_for_gather(e)) return rc;
    HIP_TRY(e, pmg_launch_reset(e->P, d_mask, e->stream));
    if (!d_mask) e->ever_reset = true;
    return PMG_OK;
}

int pmg_reset_done_device(pmg_env* e)
{
    if (!e) return PMG_E_INVALID;
    if (!e->ever_reset) return fail(e, PMG_E_STATE, "pmg_reset_done_device: reset() must be called (for all envs) first");
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    if (int rc = rows_writer_waits_for_gather(e)) return rc;
    HIP_TRY(e, pmg_launch_reset(e->P, nullptr, e->stream, 1));
    return PMG_OK;
}

int pmg_step_device(pmg_env* e, const float* d_actions)
{
    if (!e || !d_actions) return PMG_E_INVALID;
    if (!e->ever_reset) return fail(e, PMG_E_STATE, "pmg_step: reset() must be called (for all envs) before the first step()");
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    if (e->overlap) {
        /* this step writes the other row buffer; the all-gather that last read it (two steps ago) must be through */
        const int b = e->out_phase ^ 1;
        if (e->gpending[b]) { HIP_TRY(e, hipStreamWaitEvent(e->stream, e->ev_gdone[b], 0)); e->gpending[b] = false; }
        e->out_phase = b;
        e->P.out = e->out2[b];
    }
    const bool timed = (e->step_count++ % e->ev_every) == 0;
    if (timed && e->ev_n == EVENT_POOL) drain_events(e);
    int i = timed ? e->ev_n++ : 0;
    e->P.lpt_parity = (int)(e->plans++ & 1);
    HIP_TRY(e, pmg_launch_plan(e->P, d_actions, e->stream)); /* launch-order plan (13 us), outside the step-kernel timer */
    int mode = e->packed;
    /* reach: steps that have contact-prone envs run the two-wavefront kernel while the contact-free list is at most one
     * wavefront per SIMD (pmg_kernels.hip); mode 2 launches both kernels and the DEVICE picks one by the plan's count */
    if (e->packed && e->nb == 0 && !e->cfg.joint_control && e->two_wave && e->dims.num_envs <= (e->P.wave_budget / 6) * 16) mode = 2;
    if (e->wave_trace) HIP_TRY(e, hipMemsetAsync(e->wave_trace, 0xFF, 2 * (size_t)e->dims.num_envs * sizeof(pmgx::WaveRec), e->stream));
    if (timed) HIP_TRY(e, hipEventRecord(e->ev_a[i], e->stream));
    HIP_TRY(e, pmg_launch_step(e->P, d_actions, e->stream, mode, e->side, e->ev_fork, e->ev_join, e->wave_trace));
    if (timed) HIP_TRY(e, hipEventRecord(e->ev_b[i], e->stream));
    return PMG_OK;
}

int pmg_read_outputs(pmg_env* e, float* obs, float* pol, float* ag, float* dg, float* reward, uint8_t* ga, uint8_t* done)
{
    if (!e) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    size_t bytes = (size_t)e->dims.num_envs * e->dims.packed_dim * sizeof(float);
    HIP_TRY(e, hipMemcpyAsync(e->h_packed, e->P.out, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    unpack(e, e->h_packed, obs, pol, ag, dg, reward, ga, done);
    return PMG_OK;
}

int pmg_reset(pmg_env* e, const uint8_t* mask, float* obs, float* pol, float* ag, float* dg)
{
    if (!e) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    const uint8_t* dm = nullptr;
    if (mask) {
        if (!e->ever_reset) {
            for (int i = 0; i < e->dims.num_envs; i++)
                if (!mask[i]) return fail(e, PMG_E_STATE, "pmg_reset: the first reset must cover every env");
        }
        HIP_TRY(e, hipMemcpyAsync(e->d_mask, mask, (size_t)e->dims.num_envs, hipMemcpyHostToDevice, e->stream));
        dm = e->d_mask;
    }
    int rc = pmg_reset_device(e, dm);
    if (rc != PMG_OK) return rc;
    e->ever_reset = true;
    return pmg_read_outputs(e, obs, pol, ag, dg, nullptr, nullptr, nullptr);
}

int pmg_step(pmg_env* e, const float* actions, float* obs, float* pol, float* ag, float* dg, float* reward, uint8_t* ga, uint8_t* done)
{
    if (!e || !actions) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    size_t n = (size_t)e->dims.num_envs * e->dims.action_dim;
    for (size_t i = 0; i < n; i++) {
        /* kuka.py:168 assert action_space.contains(a): Box(-1, 1) */
        if (!(actions[i] >= -1.f && actions[i] <= 1.f)) return fail(e, PMG_E_INVALID, "pmg_step: action[%zu] = %g is outside [-1, 1]", i, (double)actions[i]);
        e->h_actions[i] = actions[i];
    }
    HIP_TRY(e, hipMemcpyAsync(e->d_actions, e->h_actions, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
    int rc = pmg_step_device(e, e->d_actions);
    if (rc != PMG_OK) return rc;
    return pmg_read_outputs(e, obs, pol, ag, dg, reward, ga, done);
}

int pmg_device_ptr(pmg_env* e, int which, void** d_ptr)
{
    if (!e || !d_ptr) return PMG_E_INVALID;
    switch (which) {
    case PMG_BUF_PACKED: *d_ptr = e->P.out; return PMG_OK;
    case PMG_BUF_STATE: *d_ptr = e->P.hot; return PMG_OK;
    case PMG_BUF_SCHED: *d_ptr = e->P.sched; return PMG_OK;
    case PMG_BUF_ENV_CYCLES:
        if (!e->P.env_cycles) return fail(e, PMG_E_INVALID, "pmg_device_ptr: PMG_BUF_ENV_CYCLES is kept only with PMG_ENV_CYCLES=1 in the environment at pmg_create, or with the longest-first order on (PMG_LPT_CYCLES)");
        *d_ptr = e->P.env_cycles; return PMG_OK;
    case PMG_BUF_WAVE_TRACE:
        if (!e->wave_trace) return fail(e, PMG_E_INVALID, "pmg_device_ptr: PMG_BUF_WAVE_TRACE is kept only with PMG_WAVE_TRACE=1 in the environment at pmg_create");
        *d_ptr = e->wave_trace; return PMG_OK;
    default: return fail(e, PMG_E_INVALID, "pmg_device_ptr: buffer %d is not a device buffer (use PMG_BUF_PACKED + pmg_dims offsets)", which);
    }
}
int pmg_stream(pmg_env* e, void** s)
{
    if (!e || !s) return PMG_E_INVALID;
    *s = (void*)e->stream;
    return PMG_OK;
}
int pmg_sync(pmg_env* e)
{
    if (!e) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    if (e->comm_stream) HIP_TRY(e, hipStreamSynchronize(e->comm_stream));   /* (an overlapped all-gather in flight) */
    return PMG_OK;
}

int pmg_compute_reward_device(pmg_env* e, const float* d_ag, const float* d_dg, int64_t batch, float* d_r, uint8_t* d_ok)
{
    if (!e || !d_ag || !d_dg || batch < 0) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, pmg_launch_reward(d_ag, d_dg, batch, e->dims.goal_dim, e->cfg.distance_threshold, e->cfg.binary_reward, d_r, d_ok, e->stream));
    return PMG_OK;
}

int pmg_compute_reward(pmg_env* e, const float* ag, const float* dg, int64_t batch, float* r, uint8_t* ok)
{
    if (!e || !ag || !dg || batch < 0) return PMG_E_INVALID;
    if (batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    const size_t goals = (size_t)batch * e->dims.goal_dim * sizeof(float);
    if (int rc = stage(e, "pmg_compute_reward", goals, goals, (size_t)batch * sizeof(float), (size_t)batch)) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->st_a.p, ag, goals, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(e->st_b.p, dg, goals, hipMemcpyHostToDevice, e->stream));
    int rc = pmg_compute_reward_device(e, e->st_a.f32(), e->st_b.f32(), batch, e->st_out.f32(), (uint8_t*)e->st_flag.p);
    if (rc != PMG_OK) return rc;
    if (r) HIP_TRY(e, hipMemcpyAsync(r, e->st_out.p, (size_t)batch * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (ok) HIP_TRY(e, hipMemcpyAsync(ok, e->st_flag.p, (size_t)batch, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return PMG_OK;
}

/* ---- running normaliser + policy-input rows ---- */
static int norm_derive_all(pmg_env* e)
{
    for (int w = 0; w < 3; w++) HIP_TRY(e, pmg_launch_norm_derive(e->norm[w].D, e->norm_eps, e->norm[w].tot, e->norm[w].der, e->stream));
    return PMG_OK;
}

int pmg_norm_configure(pmg_env* e, float eps, float clip_input, float clip_output)
{
    if (!e) return PMG_E_INVALID;
    if (!(eps > 0.f && clip_input > 0.f && clip_output > 0.f) || std::isinf(eps) || std::isinf(clip_input) || std::isinf(clip_output))
        return fail(e, PMG_E_INVALID, "pmg_norm_configure: eps %g, clip_input %g and clip_output %g must be positive and finite", (double)eps, (double)clip_input, (double)clip_output);
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    e->norm_eps = eps; e->norm_clip_in = clip_input; e->norm_clip_out = clip_output;
    return norm_derive_all(e);
}

static int norm_update_rows(pmg_env* e, int which, const float* d_rows, int64_t row_stride, int64_t batch, int64_t row0, const uint8_t* d_mask)
{
    pmg_env::Norm& nm = e->norm[which];
    HIP_TRY(e, pmg_launch_norm_update(d_rows, row_stride, batch, nm.D, row0, d_mask, e->norm_clip_in, e->norm_eps, nm.part, nm.tot, nm.der, e->stream));
    return PMG_OK;
}

int pmg_norm_update_device(pmg_env* e, int which, const float* d_rows, int64_t row_stride, int64_t batch, const uint8_t* d_mask)
{
    if (!e) return PMG_E_INVALID;
    const pmg_env::Norm* nm = norm_of(e, which, "pmg_norm_update_device"); if (!nm) return PMG_E_INVALID;
    if (!d_rows) return fail(e, PMG_E_INVALID, "pmg_norm_update_device: d_rows is null");
    if (batch < 0) return fail(e, PMG_E_INVALID, "pmg_norm_update_device: batch %lld is negative", (long long)batch);
    if (row_stride < nm->D) return fail(e, PMG_E_INVALID, "pmg_norm_update_device: row_stride %lld is smaller than the width %d", (long long)row_stride, nm->D);
    if (nm->D > PMG_NORM_MAX_D) return fail(e, PMG_E_INVALID, "pmg_norm_update_device: width %d beyond %d", nm->D, PMG_NORM_MAX_D);
    if (batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    return norm_update_rows(e, which, d_rows, row_stride, batch, 0, d_mask);
}

int pmg_norm_update(pmg_env* e, int which, const float* rows, int64_t batch, const uint8_t* mask)
{
    if (!e) return PMG_E_INVALID;
    const pmg_env::Norm* nm = norm_of(e, which, "pmg_norm_update"); if (!nm) return PMG_E_INVALID;
    if (!rows) return fail(e, PMG_E_INVALID, "pmg_norm_update: rows is null");
    if (batch < 0) return fail(e, PMG_E_INVALID, "pmg_norm_update: batch %lld is negative", (long long)batch);
    if (batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    const size_t bytes = (size_t)batch * nm->D * sizeof(float);
    if (int rc = stage(e, "pmg_norm_update", bytes, 0, 0, mask ? (size_t)batch : 0)) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->st_a.p, rows, bytes, hipMemcpyHostToDevice, e->stream));
    if (mask) HIP_TRY(e, hipMemcpyAsync(e->st_flag.p, mask, (size_t)batch, hipMemcpyHostToDevice, e->stream));
    int rc = pmg_norm_update_device(e, which, e->st_a.f32(), nm->D, batch, mask ? (const uint8_t*)e->st_flag.p : nullptr);
    if (rc != PMG_OK) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return PMG_OK;
}

int pmg_norm_update_env_device(pmg_env* e, const uint8_t* d_mask)
{
    if (!e) return PMG_E_INVALID;
    if (!e->ever_reset) return fail(e, PMG_E_STATE, "pmg_norm_update_env_device: reset() must be called (for all envs) first");
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    const pmg_dims& d = e->dims;
    const float* rows = e->P.out;   /* the buffer of the LAST step (pmg_comm_overlap: out2[out_phase]) */
    const int off[3] = {0, d.observation_dim, d.observation_dim + d.policy_state_dim + d.goal_dim};   /* observation, policy_state, desired_goal */
    for (int w = 0; w < 3; w++)
        if (int rc = norm_update_rows(e, w, rows + off[w], d.packed_dim, d.num_envs, e->cfg.env_index_offset, d_mask)) return rc;
    return PMG_OK;
}

int pmg_norm_read(pmg_env* e, int which, double* sum, double* sumsq, double* count, float* mean, float* std_, float* inv_std)
{
    if (!e) return PMG_E_INVALID;
    const pmg_env::Norm* found = norm_of(e, which, "pmg_norm_read"); if (!found) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    const pmg_env::Norm& nm = *found;
    const size_t D = (size_t)nm.D;
    std::vector<double> tot(2 * D + 1);
    std::vector<float> der(3 * D);
    HIP_TRY(e, hipMemcpyAsync(tot.data(), nm.tot, tot.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipMemcpyAsync(der.data(), nm.der, der.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    if (sum) memcpy(sum, tot.data(), D * sizeof(double));
    if (sumsq) memcpy(sumsq, tot.data() + D, D * sizeof(double));
    if (count) *count = tot[2 * D];
    if (mean) memcpy(mean, der.data(), D * sizeof(float));
    if (std_) memcpy(std_, der.data() + D, D * sizeof(float));
    if (inv_std) memcpy(inv_std, der.data() + 2 * D, D * sizeof(float));
    return PMG_OK;
}

int pmg_norm_write(pmg_env* e, int which, const double* sum, const double* sumsq, double count)
{
    if (!e) return PMG_E_INVALID;
    pmg_env::Norm* found = norm_of(e, which, "pmg_norm_write"); if (!found) return PMG_E_INVALID;
    if (!(count >= 0.0) || std::isinf(count)) return fail(e, PMG_E_INVALID, "pmg_norm_write: count %g must be finite and >= 0", count);
    if ((!sum || !sumsq) && count != 0.0) return fail(e, PMG_E_INVALID, "pmg_norm_write: null totals are zeros and need count == 0");
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    pmg_env::Norm& nm = *found;
    const size_t D = (size_t)nm.D;
    std::vector<double> tot(2 * D + 1, 0.0);
    if (sum) memcpy(tot.data(), sum, D * sizeof(double));
    if (sumsq) memcpy(tot.data() + D, sumsq, D * sizeof(double));
    tot[2 * D] = count;
    HIP_TRY(e, hipMemcpyAsync(nm.tot, tot.data(), tot.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, pmg_launch_norm_derive(nm.D, e->norm_eps, nm.tot, nm.der, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return PMG_OK;
}

int pmg_policy_input_device(pmg_env* e, int state_kind, const float* d_state, int64_t state_stride, const float* d_goal,
                            int64_t goal_stride, int64_t batch, float* d_out)
{
    if (!e) return PMG_E_INVALID;
    const pmg_env::Norm* found = state_norm_of(e, state_kind, "pmg_policy_input_device"); if (!found) return PMG_E_INVALID;
    if (!d_state || !d_goal || !d_out) return fail(e, PMG_E_INVALID, "pmg_policy_input_device: null pointer");
    if (((size_t)d_out & 3) != 0) return fail(e, PMG_E_INVALID, "pmg_policy_input_device: d_out is not aligned to a float");
    if (batch < 0) return fail(e, PMG_E_INVALID, "pmg_policy_input_device: batch %lld is negative", (long long)batch);
    const pmg_env::Norm& ns = *found;
    const pmg_env::Norm& ng = e->norm[PMG_NORM_GOAL];
    if (state_stride < ns.D || goal_stride < ng.D)
        return fail(e, PMG_E_INVALID, "pmg_policy_input_device: strides %lld / %lld are smaller than the widths %d / %d", (long long)state_stride, (long long)goal_stride, ns.D, ng.D);
    if (ns.D > PMG_NORM_MAX_D || ng.D > PMG_NORM_MAX_D) return fail(e, PMG_E_INVALID, "pmg_policy_input_device: width beyond %d", PMG_NORM_MAX_D);
    if (batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, pmg_launch_policy_input(d_state, state_stride, ns.D, d_goal, goal_stride, ng.D, batch, ns.der, ng.der, e->norm_clip_in, e->norm_clip_out, d_out, e->stream));
    return PMG_OK;
}

int pmg_policy_input(pmg_env* e, int state_kind, const float* state, const float* goal, int64_t batch, float* out)
{
    if (!e) return PMG_E_INVALID;
    const pmg_env::Norm* ns = state_norm_of(e, state_kind, "pmg_policy_input"); if (!ns) return PMG_E_INVALID;
    if (!state || !goal || !out) return fail(e, PMG_E_INVALID, "pmg_policy_input: null pointer");
    if (batch < 0) return fail(e, PMG_E_INVALID, "pmg_policy_input: batch %lld is negative", (long long)batch);
    if (batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    const int Ds = ns->D, Dg = e->norm[PMG_NORM_GOAL].D;
    const size_t sb = (size_t)batch * Ds * sizeof(float), gb = (size_t)batch * Dg * sizeof(float);
    if (int rc = stage(e, "pmg_policy_input", sb, gb, sb + gb, 0)) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->st_a.p, state, sb, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(e->st_b.p, goal, gb, hipMemcpyHostToDevice, e->stream));
    int rc = pmg_policy_input_device(e, state_kind, e->st_a.f32(), Ds, e->st_b.f32(), Dg, batch, e->st_out.f32());
    if (rc != PMG_OK) return rc;
    HIP_TRY(e, hipMemcpyAsync(out, e->st_out.p, sb + gb, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return PMG_OK;
}

int pmg_policy_input_env_device(pmg_env* e, int state_kind, float* d_out)
{
    if (!e) return PMG_E_INVALID;
    if (!state_norm_of(e, state_kind, "pmg_policy_input_env_device")) return PMG_E_INVALID;
    if (!d_out) return fail(e, PMG_E_INVALID, "pmg_policy_input_env_device: d_out is null");
    if (!e->ever_reset) return fail(e, PMG_E_STATE, "pmg_policy_input_env_device: reset() must be called (for all envs) first");
    const pmg_dims& d = e->dims;
    const float* rows = e->P.out;   /* the buffer of the LAST step, as pmg_device_ptr(PMG_BUF_PACKED) */
    return pmg_policy_input_device(e, state_kind, rows + (state_kind == PMG_NORM_OBSERVATION ? 0 : d.observation_dim), d.packed_dim,
                                   rows + d.observation_dim + d.policy_state_dim + d.goal_dim, d.packed_dim, d.num_envs, d_out);
}

/* ---- HER minibatches from caller-owned episode rows ---- */
/* a stride of `extent` items of `width` floats: at least the width, or 0 where there is one item only */
static bool her_stride_ok(int64_t stride, int64_t extent, int width) { return stride >= width || (stride == 0 && extent == 1); }

int pmg_her_sample_device(pmg_env* e, const pmg_her_source* src, const pmg_her_batch* out)
{
    if (!e) return PMG_E_INVALID;
    if (!src || !out) return fail(e, PMG_E_INVALID, "pmg_her_sample_device: null argument");
    if (src->struct_size != (int32_t)sizeof(pmg_her_source) || out->struct_size != (int32_t)sizeof(pmg_her_batch))
        return fail(e, PMG_E_INVALID, "pmg_her_sample_device: struct_size %d / %d != %zu / %zu", src->struct_size, out->struct_size, sizeof(pmg_her_source), sizeof(pmg_her_batch));
    const pmg_dims& d = e->dims;
    const int64_t E = src->num_episodes, T = src->episode_steps, B = out->batch;
    if (E < 1 || T < 1) return fail(e, PMG_E_INVALID, "pmg_her_sample_device: num_episodes %lld and episode_steps %lld must be >= 1", (long long)E, (long long)T);
    if ((T + 1) * E >= (1ll << 31)) return fail(e, PMG_E_INVALID, "pmg_her_sample_device: (episode_steps + 1) * num_episodes = %lld must stay below 2^31", (long long)((T + 1) * E));
    if (B < 0) return fail(e, PMG_E_INVALID, "pmg_her_sample_device: batch %lld is negative", (long long)B);
    if (!src->d_rows) return fail(e, PMG_E_INVALID, "pmg_her_sample_device: d_rows is null");
    if (!her_stride_ok(src->row_episode_stride, E, d.packed_dim) || !her_stride_ok(src->row_time_stride, T + 1, d.packed_dim))
        return fail(e, PMG_E_INVALID, "pmg_her_sample_device: row strides %lld / %lld are smaller than packed_dim %d", (long long)src->row_episode_stride, (long long)src->row_time_stride, d.packed_dim);
    if (out->d_action && !src->d_actions) return fail(e, PMG_E_INVALID, "pmg_her_sample_device: d_action needs d_actions");
    if (src->d_actions && (!her_stride_ok(src->action_episode_stride, E, d.action_dim) || !her_stride_ok(src->action_time_stride, T, d.action_dim)))
        return fail(e, PMG_E_INVALID, "pmg_her_sample_device: action strides %lld / %lld are smaller than action_dim %d", (long long)src->action_episode_stride, (long long)src->action_time_stride, d.action_dim);
    const pmg_env::Norm* found = state_norm_of(e, out->state_kind, "pmg_her_sample_device"); if (!found) return PMG_E_INVALID;
    if (!(out->future_p >= 0.f && out->future_p <= 1.f)) return fail(e, PMG_E_INVALID, "pmg_her_sample_device: future_p %g is outside [0, 1]", (double)out->future_p);
    if ((((size_t)src->d_rows | (size_t)src->d_actions | (size_t)out->d_x | (size_t)out->d_x_next | (size_t)out->d_action | (size_t)out->d_reward | (size_t)out->d_index) & 3) != 0)
        return fail(e, PMG_E_INVALID, "pmg_her_sample_device: a float / int32 pointer is not aligned to 4 bytes");
    const pmg_env::Norm& ns = *found;
    const pmg_env::Norm& ng = e->norm[PMG_NORM_GOAL];
    if (ns.D > PMG_NORM_MAX_D || ng.D > PMG_NORM_MAX_D) return fail(e, PMG_E_INVALID, "pmg_her_sample_device: width beyond %d", PMG_NORM_MAX_D);
    if (B == 0 || !(out->d_x || out->d_x_next || out->d_action || out->d_reward || out->d_goal_achieved || out->d_index)) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    int* idx = out->d_index;
    if (!idx && (out->d_x || out->d_x_next)) {
        /* sized at the first call; a larger batch later waits for the stream once */
        if (int rc = e->her_idx.reserve(e, (size_t)B * 3 * sizeof(int), "pmg_her_sample_device", "index rows")) return rc;
        idx = (int*)e->her_idx.p;
    }
    PmgHer H;
    H.rows = src->d_rows; H.res = src->row_episode_stride; H.rts = src->row_time_stride;
    H.act = src->d_actions; H.aes = src->action_episode_stride; H.ats = src->action_time_stride;
    H.E = (int)E; H.T = (int)T; H.A = d.action_dim; H.Ds = ns.D; H.G = d.goal_dim;
    H.so = out->state_kind == PMG_NORM_OBSERVATION ? 0 : d.observation_dim;
    H.ago = d.observation_dim + d.policy_state_dim; H.dgo = H.ago + d.goal_dim;
    H.raw = out->raw != 0; H.binary = e->cfg.binary_reward;
    H.thr = e->cfg.distance_threshold; H.cin = e->norm_clip_in; H.cout = e->norm_clip_out;
    H.seed = out->seed; H.counter = out->counter;
    H.relabel_below = (unsigned long long)ceil((double)out->future_p * 4294967296.0);   /* r_2 is an integer: r_2 < p 2^32 iff r_2 < ceil(p 2^32) */
    H.B = B; H.der_state = ns.der; H.der_goal = ng.der;
    H.x = out->d_x; H.xn = out->d_x_next; H.action = out->d_action; H.reward = out->d_reward; H.ok = out->d_goal_achieved; H.idx = idx;
    HIP_TRY(e, pmg_launch_her(H, e->stream));
    return PMG_OK;
}

/* ---- actor forward + exploration ---- */
/* the network of a call, validated -> M (L, widths, activation, weights); 0 or PMG_E_INVALID */
static int mlp_of(pmg_env* e, const pmg_mlp* mlp, const char* who, PmgMlp& M)
{
    if (!mlp) return fail(e, PMG_E_INVALID, "%s: mlp is null", who);
    if (mlp->struct_size != (int32_t)sizeof(pmg_mlp)) return fail(e, PMG_E_INVALID, "%s: struct_size %d != %zu", who, mlp->struct_size, sizeof(pmg_mlp));
    if (mlp->num_layers < 1 || mlp->num_layers > 4) return fail(e, PMG_E_INVALID, "%s: num_layers %d is outside 1..4", who, mlp->num_layers);
    if (mlp->out_activation != 0 && mlp->out_activation != 1) return fail(e, PMG_E_INVALID, "%s: out_activation %d is neither 0 (identity) nor 1 (tanh)", who, mlp->out_activation);
    memset(&M, 0, sizeof(M));
    M.L = mlp->num_layers; M.out_act = mlp->out_activation;
    for (int l = 0; l <= M.L; l++) {
        if (mlp->width[l] < 1 || mlp->width[l] > 256) return fail(e, PMG_E_INVALID, "%s: width[%d] = %d is outside 1..256", who, l, mlp->width[l]);
        M.width[l] = mlp->width[l];
    }
    for (int l = 0; l < M.L; l++) {
        if (!mlp->d_weight[l]) return fail(e, PMG_E_INVALID, "%s: d_weight[%d] is null", who, l);
        if ((((size_t)mlp->d_weight[l] | (size_t)mlp->d_bias[l]) & 3) != 0) return fail(e, PMG_E_INVALID, "%s: the weights of layer %d are not aligned to 4 bytes", who, l);
        M.w[l] = mlp->d_weight[l]; M.b[l] = mlp->d_bias[l];
    }
    return PMG_OK;
}

int pmg_mlp_forward_device(pmg_env* e, const pmg_mlp* mlp, const float* d_in, int64_t in_stride, int64_t batch, float* d_out, int64_t out_stride)
{
    if (!e) return PMG_E_INVALID;
    PmgMlp M;
    if (int rc = mlp_of(e, mlp, "pmg_mlp_forward_device", M)) return rc;
    if (!d_in || !d_out) return fail(e, PMG_E_INVALID, "pmg_mlp_forward_device: null pointer");
    if ((((size_t)d_in | (size_t)d_out) & 3) != 0) return fail(e, PMG_E_INVALID, "pmg_mlp_forward_device: a row pointer is not aligned to 4 bytes");
    if (batch < 0) return fail(e, PMG_E_INVALID, "pmg_mlp_forward_device: batch %lld is negative", (long long)batch);
    if (in_stride < M.width[0] || out_stride < M.width[M.L])
        return fail(e, PMG_E_INVALID, "pmg_mlp_forward_device: strides %lld / %lld are smaller than the widths %d / %d", (long long)in_stride, (long long)out_stride, M.width[0], M.width[M.L]);
    if (batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    M.B = batch; M.out = d_out; M.out_stride = out_stride;
    HIP_TRY(e, pmg_launch_mlp_forward(M, d_in, in_stride, e->stream));
    return PMG_OK;
}

int pmg_act_env_device(pmg_env* e, const pmg_mlp* mlp, int state_kind, const pmg_explore* explore, float* d_actions, float* d_preact)
{
    if (!e) return PMG_E_INVALID;
    PmgMlp M;
    if (int rc = mlp_of(e, mlp, "pmg_act_env_device", M)) return rc;
    const pmg_env::Norm* found = state_norm_of(e, state_kind, "pmg_act_env_device"); if (!found) return PMG_E_INVALID;
    const pmg_env::Norm& ns = *found;
    const pmg_env::Norm& ng = e->norm[PMG_NORM_GOAL];
    const pmg_dims& d = e->dims;
    if (M.width[0] != ns.D + ng.D || M.width[M.L] != d.action_dim)
        return fail(e, PMG_E_INVALID, "pmg_act_env_device: the network maps %d -> %d, the env needs %d + %d -> %d", M.width[0], M.width[M.L], ns.D, ng.D, d.action_dim);
    if (!d_actions) return fail(e, PMG_E_INVALID, "pmg_act_env_device: d_actions is null");
    if ((((size_t)d_actions | (size_t)d_preact) & 3) != 0) return fail(e, PMG_E_INVALID, "pmg_act_env_device: an output is not aligned to 4 bytes");
    if (explore) {
        if (explore->struct_size != (int32_t)sizeof(pmg_explore)) return fail(e, PMG_E_INVALID, "pmg_act_env_device: explore struct_size %d != %zu", explore->struct_size, sizeof(pmg_explore));
        if (!(explore->noise_eps >= 0.f) || std::isinf(explore->noise_eps)) return fail(e, PMG_E_INVALID, "pmg_act_env_device: noise_eps %g must be finite and >= 0", (double)explore->noise_eps);
        if (!(explore->random_eps >= 0.f && explore->random_eps <= 1.f)) return fail(e, PMG_E_INVALID, "pmg_act_env_device: random_eps %g is outside [0, 1]", (double)explore->random_eps);
        M.explore = 1; M.noise_eps = explore->noise_eps;
        M.seed = explore->seed; M.counter = explore->counter;
        M.random_below = (unsigned long long)ceil((double)explore->random_eps * 4294967296.0);   /* r_3 is an integer: r_3 < p 2^32 iff r_3 < ceil(p 2^32) */
    }
    if (!e->ever_reset) return fail(e, PMG_E_STATE, "pmg_act_env_device: reset() must be called (for all envs) first");
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    M.B = d.num_envs; M.out = d_preact; M.out_stride = d.action_dim; M.actions = d_actions; M.env0 = e->cfg.env_index_offset;
    PmgMlpEnv E;
    E.rows = e->P.out;   /* the buffer of the LAST step, as pmg_device_ptr(PMG_BUF_PACKED) */
    E.stride = d.packed_dim;
    E.so = state_kind == PMG_NORM_OBSERVATION ? 0 : d.observation_dim;
    E.dgo = d.observation_dim + d.policy_state_dim + d.goal_dim;
    E.Ds = ns.D; E.Dg = ng.D; E.der_state = ns.der; E.der_goal = ng.der; E.cin = e->norm_clip_in; E.cout = e->norm_clip_out;
    HIP_TRY(e, pmg_launch_mlp_act(M, E, e->stream));
    return PMG_OK;
}

/* ---- critic and TD target ---- */
/* a critic takes in_dim inputs and has one output; 0 or PMG_E_INVALID */
static int critic_of(pmg_env* e, const PmgMlp& M, int in_dim, const char* who)
{
    if (M.width[0] != in_dim || M.width[M.L] != 1)
        return fail(e, PMG_E_INVALID, "%s: the critic maps %d -> %d, the rows need %d -> 1", who, M.width[0], M.width[M.L], in_dim);
    return PMG_OK;
}

int pmg_q_device(pmg_env* e, const pmg_mlp* critic, const float* d_x, int64_t x_stride, int32_t x_dim, const float* d_a, int64_t a_stride,
                 int32_t a_dim, int64_t batch, float* d_q, int64_t q_stride)
{
    if (!e) return PMG_E_INVALID;
    PmgMlp M;
    if (int rc = mlp_of(e, critic, "pmg_q_device", M)) return rc;
    if (x_dim < 1 || a_dim < 1 || x_dim > 256 || a_dim > 256) return fail(e, PMG_E_INVALID, "pmg_q_device: x_dim %d / a_dim %d must be >= 1 (and sum to at most 256)", x_dim, a_dim);
    if (int rc = critic_of(e, M, x_dim + a_dim, "pmg_q_device")) return rc;
    if (!d_x || !d_a || !d_q) return fail(e, PMG_E_INVALID, "pmg_q_device: null pointer");
    if ((((size_t)d_x | (size_t)d_a | (size_t)d_q) & 3) != 0) return fail(e, PMG_E_INVALID, "pmg_q_device: a row pointer is not aligned to 4 bytes");
    if (batch < 0) return fail(e, PMG_E_INVALID, "pmg_q_device: batch %lld is negative", (long long)batch);
    if (x_stride < x_dim || a_stride < a_dim || q_stride < 1)
        return fail(e, PMG_E_INVALID, "pmg_q_device: strides %lld / %lld / %lld are smaller than the widths %d / %d / 1", (long long)x_stride, (long long)a_stride, (long long)q_stride, x_dim, a_dim);
    if (batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    M.B = batch; M.out = d_q; M.out_stride = q_stride;
    HIP_TRY(e, pmg_launch_mlp_q(M, d_x, x_stride, x_dim, d_a, a_stride, e->stream));
    return PMG_OK;
}

int pmg_td_target_device(pmg_env* e, const pmg_mlp* actor_target, const pmg_mlp* critic_target, const pmg_td_target* td)
{
    if (!e) return PMG_E_INVALID;
    PmgMlp P, Q;
    if (int rc = mlp_of(e, actor_target, "pmg_td_target_device (actor)", P)) return rc;
    if (int rc = mlp_of(e, critic_target, "pmg_td_target_device (critic)", Q)) return rc;
    const int Dx = P.width[0], A = P.width[P.L];
    if (int rc = critic_of(e, Q, Dx + A, "pmg_td_target_device")) return rc;
    if (!td) return fail(e, PMG_E_INVALID, "pmg_td_target_device: td is null");
    if (td->struct_size != (int32_t)sizeof(pmg_td_target)) return fail(e, PMG_E_INVALID, "pmg_td_target_device: struct_size %d != %zu", td->struct_size, sizeof(pmg_td_target));
    if (!td->d_x_next || !td->d_reward || !td->d_y) return fail(e, PMG_E_INVALID, "pmg_td_target_device: d_x_next, d_reward or d_y is null");
    if ((((size_t)td->d_x_next | (size_t)td->d_reward | (size_t)td->d_y | (size_t)td->d_q_next | (size_t)td->d_next_action) & 3) != 0)
        return fail(e, PMG_E_INVALID, "pmg_td_target_device: a float pointer is not aligned to 4 bytes");
    if (td->batch < 0) return fail(e, PMG_E_INVALID, "pmg_td_target_device: batch %lld is negative", (long long)td->batch);
    if (td->x_stride < Dx) return fail(e, PMG_E_INVALID, "pmg_td_target_device: x_stride %lld is smaller than the width %d", (long long)td->x_stride, Dx);
    if (!(td->gamma >= 0.f) || std::isinf(td->gamma)) return fail(e, PMG_E_INVALID, "pmg_td_target_device: gamma %g must be finite and >= 0", (double)td->gamma);
    if (!(td->clip_lo <= td->clip_hi)) return fail(e, PMG_E_INVALID, "pmg_td_target_device: clips %g / %g must be ordered and not NaN", (double)td->clip_lo, (double)td->clip_hi);
    if (td->batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    P.B = Q.B = td->batch;
    PmgTd T;
    T.xn = td->d_x_next; T.xs = td->x_stride; T.reward = td->d_reward; T.term = td->d_terminal;
    T.gamma = td->gamma; T.lo = td->clip_lo; T.hi = td->clip_hi;
    T.y = td->d_y; T.qn = td->d_q_next; T.na = td->d_next_action;
    HIP_TRY(e, pmg_launch_td_target(P, Q, T, e->stream));
    return PMG_OK;
}

/* ---- TD3's target: twin critics, target-policy smoothing ---- */
int64_t pmg_td3_target_work_floats(const pmg_mlp* actor_target, int has_critic2, int has_next_action, int64_t batch)
{
    if (!actor_target || actor_target->struct_size != (int32_t)sizeof(pmg_mlp) || actor_target->num_layers < 1 || actor_target->num_layers > 4) return -1;
    if (batch < 0 || batch > ((int64_t)1 << 40)) return -1;
    const int A = actor_target->width[actor_target->num_layers];
    if (A < 1 || A > 256) return -1;
    return has_critic2 && !has_next_action ? batch * A : 0;
}

int pmg_td3_target_device(pmg_env* e, const pmg_mlp* actor_target, const pmg_mlp* critic1_target, const pmg_mlp* critic2_target, const pmg_td3_target* td)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_td3_target_device";
    PmgMlp P, Q1, Q2;
    if (int rc = mlp_of(e, actor_target, "pmg_td3_target_device (actor)", P)) return rc;
    if (int rc = mlp_of(e, critic1_target, "pmg_td3_target_device (critic 1)", Q1)) return rc;
    const int Dx = P.width[0], A = P.width[P.L];
    if (int rc = critic_of(e, Q1, Dx + A, "pmg_td3_target_device (critic 1)")) return rc;
    if (critic2_target) {
        if (int rc = mlp_of(e, critic2_target, "pmg_td3_target_device (critic 2)", Q2)) return rc;
        if (int rc = critic_of(e, Q2, Dx + A, "pmg_td3_target_device (critic 2)")) return rc;
    } else
        Q2 = Q1;
    if (!td) return fail(e, PMG_E_INVALID, "%s: td is null", who);
    if (td->struct_size != (int32_t)sizeof(pmg_td3_target)) return fail(e, PMG_E_INVALID, "%s: struct_size %d != %zu", who, td->struct_size, sizeof(pmg_td3_target));
    if (!td->d_x_next || !td->d_reward || !td->d_y) return fail(e, PMG_E_INVALID, "%s: d_x_next, d_reward or d_y is null", who);
    if ((((size_t)td->d_x_next | (size_t)td->d_reward | (size_t)td->d_y | (size_t)td->d_q_min | (size_t)td->d_q1 | (size_t)td->d_q2 | (size_t)td->d_next_action |
          (size_t)td->d_work) & 3) != 0)
        return fail(e, PMG_E_INVALID, "%s: a float pointer is not aligned to 4 bytes", who);
    if (td->batch < 0) return fail(e, PMG_E_INVALID, "%s: batch %lld is negative", who, (long long)td->batch);
    if (td->x_stride < Dx) return fail(e, PMG_E_INVALID, "%s: x_stride %lld is smaller than the width %d", who, (long long)td->x_stride, Dx);
    if (!(td->gamma >= 0.f) || std::isinf(td->gamma)) return fail(e, PMG_E_INVALID, "%s: gamma %g must be finite and >= 0", who, (double)td->gamma);
    if (!(td->clip_lo <= td->clip_hi)) return fail(e, PMG_E_INVALID, "%s: clips %g / %g must be ordered and not NaN", who, (double)td->clip_lo, (double)td->clip_hi);
    if (!(td->sigma >= 0.f) || std::isinf(td->sigma)) return fail(e, PMG_E_INVALID, "%s: sigma %g must be finite and >= 0", who, (double)td->sigma);
    if (!(td->noise_clip >= 0.f)) return fail(e, PMG_E_INVALID, "%s: noise_clip %g must be >= 0 and not NaN", who, (double)td->noise_clip);
    if (td->row_offset < 0) return fail(e, PMG_E_INVALID, "%s: row_offset %lld is negative", who, (long long)td->row_offset);
    const int64_t need = pmg_td3_target_work_floats(actor_target, critic2_target != nullptr, td->d_next_action != nullptr, td->batch);
    if (need < 0) return fail(e, PMG_E_INVALID, "%s: batch %lld is too large", who, (long long)td->batch);
    if (need > 0 && (!td->d_work || td->work_floats < need))
        return fail(e, PMG_E_INVALID, "%s: d_work is null or work_floats %lld is below the %lld floats the smoothed action of critic 2 needs", who,
                    (long long)td->work_floats, (long long)need);
    if (td->batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    P.B = Q1.B = Q2.B = td->batch;
    PmgTd3 X;
    memset(&X, 0, sizeof(X));
    X.T.xn = td->d_x_next; X.T.xs = td->x_stride; X.T.reward = td->d_reward; X.T.term = td->d_terminal;
    X.T.gamma = td->gamma; X.T.lo = td->clip_lo; X.T.hi = td->clip_hi;
    X.T.y = td->d_y; X.T.qn = td->d_q_min;
    X.q1 = td->d_q1; X.q2 = critic2_target ? td->d_q2 : nullptr;
    X.twin = critic2_target != nullptr;
    X.keep = td->d_next_action ? td->d_next_action : (X.twin ? td->d_work : nullptr);
    X.noise = td->sigma > 0.f; X.sigma = td->sigma; X.c = td->noise_clip;
    X.seed = td->seed; X.counter = td->counter; X.row_offset = (unsigned long long)td->row_offset;
    HIP_TRY(e, pmg_launch_td3_target(P, Q1, Q2, X, e->stream));
    return PMG_OK;
}

/* ---- SAC: the Gaussian head and the soft target ---- */
/* a Gaussian actor has 2 A identity outputs; 0 or PMG_E_INVALID */
static int gaussian_of(pmg_env* e, const PmgMlp& M, const char* who)
{
    if ((M.width[M.L] & 1) != 0 || M.out_act != 0)
        return fail(e, PMG_E_INVALID, "%s: a Gaussian actor has an even number of outputs (means | log-stds) and out_activation 0, not %d outputs and out_activation %d",
                    who, M.width[M.L], M.out_act);
    return PMG_OK;
}
/* the clamp of the log-std; 0 or PMG_E_INVALID */
static int sac_clamp_of(pmg_env* e, float lo, float hi, const char* who)
{
    if (!std::isfinite(lo) || !std::isfinite(hi) || lo > hi) return fail(e, PMG_E_INVALID, "%s: ls_lo %g / ls_hi %g must be finite and ordered", who, (double)lo, (double)hi);
    return PMG_OK;
}
/* what both head entries check in their struct beyond the rows, and the head's launch arguments */
static int sac_head_of(pmg_env* e, const pmg_sac_sample* s, int A, const char* who, PmgSac& G)
{
    if (!s) return fail(e, PMG_E_INVALID, "%s: the argument struct is null", who);
    if (s->struct_size != (int32_t)sizeof(pmg_sac_sample)) return fail(e, PMG_E_INVALID, "%s: struct_size %d != %zu", who, s->struct_size, sizeof(pmg_sac_sample));
    if (int rc = sac_clamp_of(e, s->ls_lo, s->ls_hi, who)) return rc;
    if (!s->d_action && !s->d_logp) return fail(e, PMG_E_INVALID, "%s: d_action and d_logp are both null: no output is requested", who);
    if ((((size_t)s->d_action | (size_t)s->d_logp | (size_t)s->d_noise | (size_t)s->d_preact) & 3) != 0)
        return fail(e, PMG_E_INVALID, "%s: an output is not aligned to 4 bytes", who);
    if ((s->d_action && s->action_stride < A) || (s->d_noise && s->noise_stride < A) || (s->d_preact && s->preact_stride < 2 * A))
        return fail(e, PMG_E_INVALID, "%s: strides %lld / %lld / %lld are smaller than the widths %d / %d / %d", who, (long long)s->action_stride,
                    (long long)s->noise_stride, (long long)s->preact_stride, A, A, 2 * A);
    memset(&G, 0, sizeof(G));
    G.ls_lo = s->ls_lo; G.ls_hi = s->ls_hi; G.sample = s->sample != 0; G.seed = s->seed; G.counter = s->counter;
    G.action = s->d_action; G.as = s->action_stride; G.logp = s->d_logp; G.noise = s->d_noise; G.ns = s->noise_stride;
    G.preact = s->d_preact; G.ps = s->preact_stride;
    return PMG_OK;
}

int pmg_sac_sample_device(pmg_env* e, const pmg_mlp* actor, const pmg_sac_sample* s)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_sac_sample_device";
    PmgMlp M;
    PmgSac G;
    if (int rc = mlp_of(e, actor, who, M)) return rc;
    if (int rc = gaussian_of(e, M, who)) return rc;
    if (int rc = sac_head_of(e, s, M.width[M.L] / 2, who, G)) return rc;
    if (!s->d_x) return fail(e, PMG_E_INVALID, "%s: d_x is null", who);
    if (((size_t)s->d_x & 3) != 0) return fail(e, PMG_E_INVALID, "%s: d_x is not aligned to 4 bytes", who);
    if (s->batch < 0) return fail(e, PMG_E_INVALID, "%s: batch %lld is negative", who, (long long)s->batch);
    if (s->x_stride < M.width[0]) return fail(e, PMG_E_INVALID, "%s: x_stride %lld is smaller than the width %d", who, (long long)s->x_stride, M.width[0]);
    if (s->row_offset < 0) return fail(e, PMG_E_INVALID, "%s: row_offset %lld is negative", who, (long long)s->row_offset);
    if (s->batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    M.B = s->batch;
    G.row_offset = (unsigned long long)s->row_offset;
    HIP_TRY(e, pmg_launch_sac_sample(M, G, s->d_x, s->x_stride, e->stream));
    return PMG_OK;
}

int pmg_sac_act_env_device(pmg_env* e, const pmg_mlp* actor, int state_kind, const pmg_sac_sample* s)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_sac_act_env_device";
    PmgMlp M;
    PmgSac G;
    if (int rc = mlp_of(e, actor, who, M)) return rc;
    if (int rc = gaussian_of(e, M, who)) return rc;
    const pmg_env::Norm* found = state_norm_of(e, state_kind, who); if (!found) return PMG_E_INVALID;
    const pmg_env::Norm& ns = *found;
    const pmg_env::Norm& ng = e->norm[PMG_NORM_GOAL];
    const pmg_dims& d = e->dims;
    if (M.width[0] != ns.D + ng.D || M.width[M.L] != 2 * d.action_dim)
        return fail(e, PMG_E_INVALID, "%s: the network maps %d -> %d, the env needs %d + %d -> 2 * %d", who, M.width[0], M.width[M.L], ns.D, ng.D, d.action_dim);
    if (int rc = sac_head_of(e, s, d.action_dim, who, G)) return rc;
    if (!e->ever_reset) return fail(e, PMG_E_STATE, "%s: reset() must be called (for all envs) first", who);
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    M.B = d.num_envs;
    G.row_offset = (unsigned long long)e->cfg.env_index_offset;
    PmgMlpEnv E;
    E.rows = e->P.out;   /* the buffer of the LAST step, as pmg_device_ptr(PMG_BUF_PACKED) */
    E.stride = d.packed_dim;
    E.so = state_kind == PMG_NORM_OBSERVATION ? 0 : d.observation_dim;
    E.dgo = d.observation_dim + d.policy_state_dim + d.goal_dim;
    E.Ds = ns.D; E.Dg = ng.D; E.der_state = ns.der; E.der_goal = ng.der; E.cin = e->norm_clip_in; E.cout = e->norm_clip_out;
    HIP_TRY(e, pmg_launch_sac_act(M, G, E, e->stream));
    return PMG_OK;
}

int64_t pmg_sac_target_work_floats(const pmg_mlp* actor, int has_next_action, int64_t batch)
{
    if (!actor || actor->struct_size != (int32_t)sizeof(pmg_mlp) || actor->num_layers < 1 || actor->num_layers > 4) return -1;
    if (batch < 0 || batch > ((int64_t)1 << 40)) return -1;
    const int A2 = actor->width[actor->num_layers];
    if (A2 < 2 || A2 > 256 || (A2 & 1) != 0) return -1;
    return has_next_action ? 0 : batch * (A2 / 2);
}

int pmg_sac_target_device(pmg_env* e, const pmg_mlp* actor, const pmg_mlp* critic1_target, const pmg_mlp* critic2_target, const pmg_sac_target* td)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_sac_target_device";
    PmgMlp P, Q1, Q2;
    if (int rc = mlp_of(e, actor, "pmg_sac_target_device (actor)", P)) return rc;
    if (int rc = gaussian_of(e, P, "pmg_sac_target_device (actor)")) return rc;
    if (int rc = mlp_of(e, critic1_target, "pmg_sac_target_device (critic 1)", Q1)) return rc;
    const int Dx = P.width[0], A = P.width[P.L] / 2;
    if (int rc = critic_of(e, Q1, Dx + A, "pmg_sac_target_device (critic 1)")) return rc;
    if (critic2_target) {
        if (int rc = mlp_of(e, critic2_target, "pmg_sac_target_device (critic 2)", Q2)) return rc;
        if (int rc = critic_of(e, Q2, Dx + A, "pmg_sac_target_device (critic 2)")) return rc;
    } else
        Q2 = Q1;
    if (!td) return fail(e, PMG_E_INVALID, "%s: td is null", who);
    if (td->struct_size != (int32_t)sizeof(pmg_sac_target)) return fail(e, PMG_E_INVALID, "%s: struct_size %d != %zu", who, td->struct_size, sizeof(pmg_sac_target));
    if (!td->d_x_next || !td->d_reward || !td->d_y) return fail(e, PMG_E_INVALID, "%s: d_x_next, d_reward or d_y is null", who);
    if ((((size_t)td->d_x_next | (size_t)td->d_reward | (size_t)td->d_y | (size_t)td->d_q_min | (size_t)td->d_q1 | (size_t)td->d_q2 | (size_t)td->d_next_action |
          (size_t)td->d_logp | (size_t)td->d_alpha | (size_t)td->d_work) & 3) != 0)
        return fail(e, PMG_E_INVALID, "%s: a float pointer is not aligned to 4 bytes", who);
    if (td->batch < 0) return fail(e, PMG_E_INVALID, "%s: batch %lld is negative", who, (long long)td->batch);
    if (td->x_stride < Dx) return fail(e, PMG_E_INVALID, "%s: x_stride %lld is smaller than the width %d", who, (long long)td->x_stride, Dx);
    if (!(td->gamma >= 0.f) || std::isinf(td->gamma)) return fail(e, PMG_E_INVALID, "%s: gamma %g must be finite and >= 0", who, (double)td->gamma);
    if (!(td->clip_lo <= td->clip_hi)) return fail(e, PMG_E_INVALID, "%s: clips %g / %g must be ordered and not NaN", who, (double)td->clip_lo, (double)td->clip_hi);
    if (!(td->alpha >= 0.f) || std::isinf(td->alpha)) return fail(e, PMG_E_INVALID, "%s: alpha %g must be finite and >= 0", who, (double)td->alpha);
    if (int rc = sac_clamp_of(e, td->ls_lo, td->ls_hi, who)) return rc;
    if (td->row_offset < 0) return fail(e, PMG_E_INVALID, "%s: row_offset %lld is negative", who, (long long)td->row_offset);
    const int64_t need = pmg_sac_target_work_floats(actor, td->d_next_action != nullptr, td->batch);
    if (need < 0) return fail(e, PMG_E_INVALID, "%s: batch %lld is too large", who, (long long)td->batch);
    if (need > 0 && (!td->d_work || td->work_floats < need))
        return fail(e, PMG_E_INVALID, "%s: d_work is null or work_floats %lld is below the %lld floats the action of the critics needs", who,
                    (long long)td->work_floats, (long long)need);
    if (td->batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    P.B = Q1.B = Q2.B = td->batch;
    PmgSacTd X;
    memset(&X, 0, sizeof(X));
    X.T.xn = td->d_x_next; X.T.xs = td->x_stride; X.T.reward = td->d_reward; X.T.term = td->d_terminal;
    X.T.gamma = td->gamma; X.T.lo = td->clip_lo; X.T.hi = td->clip_hi;
    X.T.y = td->d_y; X.T.qn = td->d_q_min;
    X.q1 = td->d_q1; X.q2 = critic2_target ? td->d_q2 : nullptr;
    X.twin = critic2_target != nullptr;
    X.alpha = td->alpha; X.d_alpha = td->d_alpha;
    X.G.ls_lo = td->ls_lo; X.G.ls_hi = td->ls_hi; X.G.sample = td->sample != 0; X.G.seed = td->seed; X.G.counter = td->counter;
    X.G.row_offset = (unsigned long long)td->row_offset;
    X.G.action = td->d_next_action ? td->d_next_action : td->d_work; X.G.as = A;
    X.G.logp = td->d_logp;
    HIP_TRY(e, pmg_launch_sac_target(P, Q1, Q2, X, e->stream));
    return PMG_OK;
}

/* ---- back-propagation, Adam, Polyak ---- */
int64_t pmg_mlp_grad_work_floats(const pmg_mlp* mlp, int64_t batch)
{
    if (!mlp || mlp->struct_size != (int32_t)sizeof(pmg_mlp) || mlp->num_layers < 1 || mlp->num_layers > 4) return -1;
    if (batch < 0 || batch > ((int64_t)1 << 40)) return -1;
    PmgMlp M;
    memset(&M, 0, sizeof(M));
    M.L = mlp->num_layers;
    for (int l = 0; l <= M.L; l++) {
        if (mlp->width[l] < 1 || mlp->width[l] > 256) return -1;
        M.width[l] = mlp->width[l];
    }
    return pmg_grad_work_layout(M, batch, nullptr, nullptr);
}
/* the tensors of `p` a network of M's shape has (has_bias[l]: layer l has a bias), all non-null and aligned; extra_bias_ok: a bias pointer
 * where the network has none is ignored instead of refused; 0 or PMG_E_INVALID */
static int params_of(pmg_env* e, const PmgMlp& M, const pmg_mlp_params* p, bool extra_bias_ok, const char* who, const char* what)
{
    if (!p) return fail(e, PMG_E_INVALID, "%s: %s is null", who, what);
    for (int l = 0; l < M.L; l++) {
        if (!p->d_weight[l]) return fail(e, PMG_E_INVALID, "%s: %s d_weight[%d] is null", who, what, l);
        if (M.b[l] && !p->d_bias[l]) return fail(e, PMG_E_INVALID, "%s: %s d_bias[%d] is null, the network has that bias", who, what, l);
        if (!M.b[l] && p->d_bias[l] && !extra_bias_ok) return fail(e, PMG_E_INVALID, "%s: %s d_bias[%d] is given, the network has no such bias", who, what, l);
        if ((((size_t)p->d_weight[l] | (size_t)p->d_bias[l]) & 3) != 0) return fail(e, PMG_E_INVALID, "%s: %s of layer %d are not aligned to 4 bytes", who, what, l);
    }
    return PMG_OK;
}

/* everything pmg_mlp_grad_device checks in its arguments but the size of the workspace -> M; 0 or PMG_E_INVALID */
static int grad_args_of(pmg_env* e, const char* who, const pmg_mlp* mlp, const pmg_mlp_grad* g, PmgMlp& M)
{
    if (int rc = mlp_of(e, mlp, who, M)) return rc;
    if (!g) return fail(e, PMG_E_INVALID, "%s: g is null", who);
    if (g->struct_size != (int32_t)sizeof(pmg_mlp_grad)) return fail(e, PMG_E_INVALID, "%s: struct_size %d != %zu", who, g->struct_size, sizeof(pmg_mlp_grad));
    if (g->batch < 0) return fail(e, PMG_E_INVALID, "%s: batch %lld is negative", who, (long long)g->batch);
    if (!g->d_x || g->x_dim < 1 || g->x_dim > 256) return fail(e, PMG_E_INVALID, "%s: d_x is null or x_dim %d is outside 1..256", who, g->x_dim);
    if ((g->d_a != nullptr) != (g->a_dim >= 1) || g->a_dim < 0 || g->a_dim > 256)
        return fail(e, PMG_E_INVALID, "%s: d_a and a_dim %d must be given together (a_dim in 1..256) or be NULL and 0", who, g->a_dim);
    if (g->x_dim + g->a_dim != M.width[0]) return fail(e, PMG_E_INVALID, "%s: x_dim %d + a_dim %d != width[0] %d", who, g->x_dim, g->a_dim, M.width[0]);
    if (g->d_ga && !g->d_a) return fail(e, PMG_E_INVALID, "%s: d_ga without d_a", who);
    if (g->d_gout && g->d_target) return fail(e, PMG_E_INVALID, "%s: both d_gout and d_target are given", who);
    if (!std::isfinite(g->gscale)) return fail(e, PMG_E_INVALID, "%s: gscale %g is not finite", who, (double)g->gscale);
    if (!g->grads && !g->d_gx && !g->d_ga && !g->d_out) return fail(e, PMG_E_INVALID, "%s: grads, d_gx, d_ga and d_out are all null: nothing to do", who);
    if (g->grads) if (int rc = params_of(e, M, g->grads, false, who, "grads")) return rc;
    const int A = M.width[M.L];
    if ((((size_t)g->d_x | (size_t)g->d_a | (size_t)g->d_gout | (size_t)g->d_target | (size_t)g->d_gx | (size_t)g->d_ga | (size_t)g->d_out | (size_t)g->d_work) & 3) != 0)
        return fail(e, PMG_E_INVALID, "%s: a float pointer is not aligned to 4 bytes", who);
    if (g->x_stride < g->x_dim || (g->d_a && g->a_stride < g->a_dim) || (g->d_gout && g->gout_stride < A) || (g->d_target && g->target_stride < A) ||
        (g->d_gx && g->gx_stride < g->x_dim) || (g->d_ga && g->ga_stride < g->a_dim) || (g->d_out && g->out_stride < A))
        return fail(e, PMG_E_INVALID, "%s: a stride is smaller than its width", who);
    return PMG_OK;
}
/* the workspace of a checked call: `need` floats (< 0: the batch is too large) */
static int grad_work_of(pmg_env* e, const char* who, const pmg_mlp_grad* g, int64_t need)
{
    if (need < 0) return fail(e, PMG_E_INVALID, "%s: batch %lld is too large", who, (long long)g->batch);
    if (!g->d_work || g->work_floats < need) return fail(e, PMG_E_INVALID, "%s: d_work is null or work_floats %lld < %lld", who, (long long)g->work_floats, (long long)need);
    return PMG_OK;
}
/* the launcher's view of a checked call on M.B = g->batch rows, the workspace cut */
static void grad_launch_args(const pmg_mlp_grad* g, PmgMlp& M, PmgGrad& G)
{
    M.B = g->batch;
    memset(&G, 0, sizeof(G));
    G.x = g->d_x; G.xs = g->x_stride; G.x_dim = g->x_dim; G.a = g->d_a; G.as = g->a_stride; G.a_dim = g->a_dim;
    G.gout = g->d_gout; G.gos = g->gout_stride; G.target = g->d_target; G.ts = g->target_stride; G.gscale = g->gscale;
    G.grads = g->grads ? 1 : 0;
    for (int l = 0; l < M.L && g->grads; l++) { G.dw[l] = g->grads->d_weight[l]; G.db[l] = M.b[l] ? g->grads->d_bias[l] : nullptr; }
    G.gx = g->d_gx; G.gxs = g->gx_stride; G.ga = g->d_ga; G.gas = g->ga_stride; G.out = g->d_out; G.os = g->out_stride;
    pmg_grad_work_layout(M, M.B, g->d_work, &G);
}

int pmg_mlp_grad_device(pmg_env* e, const pmg_mlp* mlp, const pmg_mlp_grad* g)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_mlp_grad_device";
    PmgMlp M;
    if (int rc = grad_args_of(e, who, mlp, g, M)) return rc;
    if (int rc = grad_work_of(e, who, g, pmg_mlp_grad_work_floats(mlp, g->batch))) return rc;
    if (g->batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    PmgGrad G;
    grad_launch_args(g, M, G);
    HIP_TRY(e, pmg_launch_mlp_grad(M, G, e->stream));
    return PMG_OK;
}

/* the segment table of a network's tensors: tensor k of `p` (written) beside tensor k of g / m / v (any may be null for a launcher that
 * does not use them) */
static void segs_of(const PmgMlp& M, const pmg_mlp_params* p, const float* const* gw, const float* const* gb, const pmg_mlp_params* m,
                    const pmg_mlp_params* v, PmgSegs& T)
{
    memset(&T, 0, sizeof(T));
    long long end = 0;
    for (int l = 0; l < M.L; l++)
        for (int k = 0; k < 2; k++) {
            if (k && !M.b[l]) continue;
            end += k ? M.width[l + 1] : (long long)M.width[l + 1] * M.width[l];
            const int n = T.n++;
            T.end[n] = end;
            T.p[n] = k ? p->d_bias[l] : p->d_weight[l];
            T.g[n] = k ? gb[l] : gw[l];
            if (m) T.m[n] = k ? m->d_bias[l] : m->d_weight[l];
            if (v) T.v[n] = k ? v->d_bias[l] : v->d_weight[l];
        }
}

/* Adam's settings of `who`'s caller, validated -> the device's constants (include/pmg.h); 0 or PMG_E_INVALID */
static int adam_of(pmg_env* e, const char* who, const pmg_adam* a, PmgAdam& A)
{
    if (!a) return fail(e, PMG_E_INVALID, "%s: a is null", who);
    if (a->struct_size != (int32_t)sizeof(pmg_adam)) return fail(e, PMG_E_INVALID, "%s: struct_size %d != %zu", who, a->struct_size, sizeof(pmg_adam));
    if (!std::isfinite(a->lr) || !std::isfinite(a->eps) || !(a->eps >= 0.f)) return fail(e, PMG_E_INVALID, "%s: lr %g must be finite, eps %g finite and >= 0", who, (double)a->lr, (double)a->eps);
    if (!(a->beta1 >= 0.f && a->beta1 < 1.f) || !(a->beta2 >= 0.f && a->beta2 < 1.f)) return fail(e, PMG_E_INVALID, "%s: betas %g / %g must lie in [0, 1)", who, (double)a->beta1, (double)a->beta2);
    if (a->step < 1) return fail(e, PMG_E_INVALID, "%s: step %lld must be >= 1", who, (long long)a->step);
    const double c1 = 1.0 - pow((double)a->beta1, (double)a->step), c2 = 1.0 - pow((double)a->beta2, (double)a->step);
    A.beta1 = a->beta1; A.beta2 = a->beta2;
    A.omb1 = (float)(1.0 - (double)a->beta1); A.omb2 = (float)(1.0 - (double)a->beta2);
    A.step_size = (float)((double)a->lr / c1); A.rsc2 = (float)(1.0 / sqrt(c2)); A.eps = a->eps;
    return PMG_OK;
}

int pmg_mlp_adam_device(pmg_env* e, const pmg_mlp* shape, const pmg_mlp_params* param, const pmg_mlp_params* grad, const pmg_mlp_params* m,
                        const pmg_mlp_params* v, const pmg_adam* a)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_mlp_adam_device";
    PmgMlp M;
    if (int rc = mlp_of(e, shape, who, M)) return rc;
    if (int rc = params_of(e, M, param, true, who, "param")) return rc;
    if (int rc = params_of(e, M, grad, true, who, "grad")) return rc;
    if (int rc = params_of(e, M, m, true, who, "m")) return rc;
    if (int rc = params_of(e, M, v, true, who, "v")) return rc;
    PmgAdam A;
    if (int rc = adam_of(e, who, a, A)) return rc;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    PmgSegs T;
    segs_of(M, param, grad->d_weight, grad->d_bias, m, v, T);
    HIP_TRY(e, pmg_launch_adam(T, A, e->stream));
    return PMG_OK;
}

int pmg_mlp_polyak_device(pmg_env* e, const pmg_mlp* source, const pmg_mlp_params* target, float tau)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_mlp_polyak_device";
    PmgMlp M;
    if (int rc = mlp_of(e, source, who, M)) return rc;
    if (int rc = params_of(e, M, target, true, who, "target")) return rc;
    if (!(tau >= 0.f && tau <= 1.f)) return fail(e, PMG_E_INVALID, "%s: tau %g is outside [0, 1]", who, (double)tau);
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    PmgSegs T;
    segs_of(M, target, M.w, M.b, nullptr, nullptr, T);
    HIP_TRY(e, pmg_launch_polyak(T, tau, e->stream));
    return PMG_OK;
}

/* ---- chunked batch reduction of dW / db ---- */
/* P of the partials: a bias is counted for every layer, so the figure needs the widths alone */
static int64_t grad_chunk_params(const pmg_mlp* mlp)
{
    int64_t P = 0;
    for (int l = 0; l < mlp->num_layers; l++) P += ((int64_t)mlp->width[l] + 1) * mlp->width[l + 1];
    return P;
}
int64_t pmg_mlp_grad_chunked_work_floats(const pmg_mlp* mlp, int64_t batch, int64_t chunk_rows)
{
    const int64_t base = pmg_mlp_grad_work_floats(mlp, batch);
    if (base < 0 || chunk_rows < 2 || (chunk_rows & 1)) return -1;
    const int64_t C = batch / chunk_rows + (batch % chunk_rows != 0);
    if (C > PMG_GRAD_MAX_CHUNKS) return -1;
    return C <= 1 ? base : base + C * grad_chunk_params(mlp);
}

int pmg_mlp_grad_chunked_device(pmg_env* e, const pmg_mlp* mlp, const pmg_mlp_grad* g, int64_t chunk_rows)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_mlp_grad_chunked_device";
    PmgMlp M;
    if (int rc = grad_args_of(e, who, mlp, g, M)) return rc;
    if (chunk_rows < 2 || (chunk_rows & 1)) return fail(e, PMG_E_INVALID, "%s: chunk_rows %lld must be even and >= 2", who, (long long)chunk_rows);
    const int64_t C = g->batch / chunk_rows + (g->batch % chunk_rows != 0);
    if (C > PMG_GRAD_MAX_CHUNKS)
        return fail(e, PMG_E_INVALID, "%s: batch %lld in chunks of %lld rows is %lld chunks, more than %d", who, (long long)g->batch, (long long)chunk_rows, (long long)C, PMG_GRAD_MAX_CHUNKS);
    const bool chunked = g->grads && C > 1;
    const int64_t base = pmg_mlp_grad_work_floats(mlp, g->batch);
    if (int rc = grad_work_of(e, who, g, chunked ? pmg_mlp_grad_chunked_work_floats(mlp, g->batch, chunk_rows) : base)) return rc;
    if (g->batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    PmgGrad G;
    grad_launch_args(g, M, G);
    if (!chunked) {                                                /* one chunk is the single chain; input gradients have no reduction */
        HIP_TRY(e, pmg_launch_mlp_grad(M, G, e->stream));
        return PMG_OK;
    }
    PmgSegs T;
    segs_of(M, g->grads, g->grads->d_weight, g->grads->d_bias, nullptr, nullptr, T);
    PmgGradChunks Q;
    memset(&Q, 0, sizeof(Q));
    Q.R = chunk_rows; Q.C = C; Q.P = grad_chunk_params(mlp); Q.tiles = pmg_grad_w_tiles(M); Q.part = g->d_work + base;
    for (int l = 0, n = 0; l < M.L; l++) {                          /* tensor n of T starts at T.end[n - 1] */
        Q.pw[l] = Q.part + (n ? T.end[n - 1] : 0);
        n++;
        if (M.b[l]) { Q.pb[l] = Q.part + T.end[n - 1]; n++; }
    }
    HIP_TRY(e, pmg_launch_mlp_grad_chunked(M, G, Q, T, e->stream));
    return PMG_OK;
}

/* ---- the actor's half of an update in one call ---- */
/* the workspace is the actor's: pmg_mlp_grad_work_floats, or with chunk_rows the chunked figure */
int64_t pmg_policy_grad_work_floats(const pmg_mlp* actor, const pmg_mlp* critic, int64_t batch, int64_t chunk_rows)
{
    if (pmg_mlp_grad_work_floats(actor, batch) < 0 || pmg_mlp_grad_work_floats(critic, batch) < 0) return -1;
    if (critic->width[0] != actor->width[0] + actor->width[actor->num_layers] || critic->width[critic->num_layers] != 1) return -1;
    if (chunk_rows == 0) return pmg_mlp_grad_work_floats(actor, batch);
    return pmg_mlp_grad_chunked_work_floats(actor, batch, chunk_rows);
}

/* pmg_policy_grad_device (with_bc false: bc is not looked at) and pmg_policy_grad_bc_device: one validation, one launch */
static int policy_grad_call(pmg_env* e, const char* who, const char* who_actor, const char* who_critic, const pmg_mlp* actor, const pmg_mlp* critic,
                            const pmg_policy_grad* g, bool with_bc, const pmg_policy_bc* bc, int64_t chunk_rows)
{
    if (!e) return PMG_E_INVALID;
    PmgMlp P, Q;
    if (int rc = mlp_of(e, actor, who_actor, P)) return rc;
    if (int rc = mlp_of(e, critic, who_critic, Q)) return rc;
    const int Dx = P.width[0], A = P.width[P.L];
    if (int rc = critic_of(e, Q, Dx + A, who)) return rc;
    if (!g) return fail(e, PMG_E_INVALID, "%s: g is null", who);
    if (g->struct_size != (int32_t)sizeof(pmg_policy_grad)) return fail(e, PMG_E_INVALID, "%s: struct_size %d != %zu", who, g->struct_size, sizeof(pmg_policy_grad));
    if (g->batch < 0) return fail(e, PMG_E_INVALID, "%s: batch %lld is negative", who, (long long)g->batch);
    if (!g->d_x) return fail(e, PMG_E_INVALID, "%s: d_x is null", who);
    if (!std::isfinite(g->gscale) || !std::isfinite(g->l2scale)) return fail(e, PMG_E_INVALID, "%s: gscale %g or l2scale %g is not finite", who, (double)g->gscale, (double)g->l2scale);
    if (with_bc) {
        if (!bc) return fail(e, PMG_E_INVALID, "%s: bc is null", who);
        if (bc->struct_size != (int32_t)sizeof(pmg_policy_bc)) return fail(e, PMG_E_INVALID, "%s: bc.struct_size %d != %zu", who, bc->struct_size, sizeof(pmg_policy_bc));
        if (!std::isfinite(bc->bcscale)) return fail(e, PMG_E_INVALID, "%s: bcscale %g is not finite", who, (double)bc->bcscale);
        if (bc->q_filter != 0 && bc->q_filter != 1) return fail(e, PMG_E_INVALID, "%s: q_filter %d must be 0 or 1", who, bc->q_filter);
        if (bc->demo_begin < 0 || bc->demo_begin > g->batch) return fail(e, PMG_E_INVALID, "%s: demo_begin %lld is outside [0, %lld]", who, (long long)bc->demo_begin, (long long)g->batch);
        if (!bc->d_demo_action && bc->demo_begin < g->batch) return fail(e, PMG_E_INVALID, "%s: d_demo_action is null with demonstration rows from %lld", who, (long long)bc->demo_begin);
        if ((((size_t)bc->d_demo_action | (size_t)bc->d_q_demo) & 3) != 0) return fail(e, PMG_E_INVALID, "%s: d_demo_action or d_q_demo is not aligned to 4 bytes", who);
        if (bc->d_demo_action && bc->demo_action_stride < A) return fail(e, PMG_E_INVALID, "%s: demo_action_stride %lld < %d", who, (long long)bc->demo_action_stride, A);
    }
    if (!g->grads && !g->d_action && !g->d_out && !g->d_q && !g->d_gaction && !(with_bc && (bc->d_q_demo || bc->d_filter)))
        return fail(e, PMG_E_INVALID, "%s: grads and every output are null: nothing to do", who);
    if (g->grads) if (int rc = params_of(e, P, g->grads, false, who, "grads")) return rc;
    if ((((size_t)g->d_x | (size_t)g->d_action | (size_t)g->d_out | (size_t)g->d_q | (size_t)g->d_gaction | (size_t)g->d_work) & 3) != 0)
        return fail(e, PMG_E_INVALID, "%s: a float pointer is not aligned to 4 bytes", who);
    if (g->x_stride < Dx || (g->d_action && g->action_stride < A) || (g->d_out && g->out_stride < A) || (g->d_gaction && g->gaction_stride < A))
        return fail(e, PMG_E_INVALID, "%s: a stride is smaller than its width", who);
    if (chunk_rows < 0 || chunk_rows == 1 || (chunk_rows & 1)) return fail(e, PMG_E_INVALID, "%s: chunk_rows %lld must be 0 (one chain) or even and >= 2", who, (long long)chunk_rows);
    const int64_t C = chunk_rows ? g->batch / chunk_rows + (g->batch % chunk_rows != 0) : 1;
    if (C > PMG_GRAD_MAX_CHUNKS)
        return fail(e, PMG_E_INVALID, "%s: batch %lld in chunks of %lld rows is %lld chunks, more than %d", who, (long long)g->batch, (long long)chunk_rows, (long long)C, PMG_GRAD_MAX_CHUNKS);
    const bool chunked = g->grads && C > 1;
    const int64_t base = pmg_mlp_grad_work_floats(actor, g->batch);
    const int64_t need = chunked ? pmg_mlp_grad_chunked_work_floats(actor, g->batch, chunk_rows) : base;
    if (need < 0) return fail(e, PMG_E_INVALID, "%s: batch %lld is too large", who, (long long)g->batch);
    if (!g->d_work || g->work_floats < need) return fail(e, PMG_E_INVALID, "%s: d_work is null or work_floats %lld < %lld", who, (long long)g->work_floats, (long long)need);
    if (g->batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    P.B = Q.B = g->batch;
    PmgGrad G;
    memset(&G, 0, sizeof(G));
    G.x = g->d_x; G.xs = g->x_stride; G.x_dim = Dx;
    G.grads = g->grads ? 1 : 0;
    for (int l = 0; l < P.L && g->grads; l++) { G.dw[l] = g->grads->d_weight[l]; G.db[l] = P.b[l] ? g->grads->d_bias[l] : nullptr; }
    G.out = g->d_out; G.os = g->out_stride;
    pmg_grad_work_layout(P, P.B, g->d_work, &G);
    PmgPolicy X;
    X.gscale = g->gscale; X.l2scale = g->l2scale;
    X.action = g->d_action; X.as = g->action_stride; X.q = g->d_q; X.ga = g->d_gaction; X.gas = g->gaction_stride;
    PmgPolicyBc D;
    memset(&D, 0, sizeof(D));
    if (with_bc) {
        D.begin = bc->demo_begin; D.ad = bc->d_demo_action; D.ads = bc->demo_action_stride; D.bcscale = bc->bcscale; D.q_filter = bc->q_filter;
        D.qd = bc->d_q_demo; D.filter = bc->d_filter;
    }
    if (!chunked) {
        HIP_TRY(e, pmg_launch_policy_grad(P, Q, G, X, nullptr, nullptr, e->stream, with_bc ? &D : nullptr));
        return PMG_OK;
    }
    PmgSegs T;
    segs_of(P, g->grads, g->grads->d_weight, g->grads->d_bias, nullptr, nullptr, T);
    PmgGradChunks K;
    memset(&K, 0, sizeof(K));
    K.R = chunk_rows; K.C = C; K.P = grad_chunk_params(actor); K.tiles = pmg_grad_w_tiles(P); K.part = g->d_work + base;
    for (int l = 0, n = 0; l < P.L; l++) {                          /* tensor n of T starts at T.end[n - 1] */
        K.pw[l] = K.part + (n ? T.end[n - 1] : 0);
        n++;
        if (P.b[l]) { K.pb[l] = K.part + T.end[n - 1]; n++; }
    }
    HIP_TRY(e, pmg_launch_policy_grad(P, Q, G, X, &K, &T, e->stream, with_bc ? &D : nullptr));
    return PMG_OK;
}
int pmg_policy_grad_device(pmg_env* e, const pmg_mlp* actor, const pmg_mlp* critic, const pmg_policy_grad* g, int64_t chunk_rows)
{
    return policy_grad_call(e, "pmg_policy_grad_device", "pmg_policy_grad_device (actor)", "pmg_policy_grad_device (critic)", actor, critic, g, false, nullptr,
                            chunk_rows);
}
/* ---- the same with the behaviour-cloning term and its Q-filter ---- */
int pmg_policy_grad_bc_device(pmg_env* e, const pmg_mlp* actor, const pmg_mlp* critic, const pmg_policy_grad* g, const pmg_policy_bc* bc, int64_t chunk_rows)
{
    return policy_grad_call(e, "pmg_policy_grad_bc_device", "pmg_policy_grad_bc_device (actor)", "pmg_policy_grad_bc_device (critic)", actor, critic, g, true, bc,
                            chunk_rows);
}

/* ---- SAC's actor half in one call and the temperature step ---- */
/* the actor's figure, then a [B, A] without d_action, then critic 1's ga [B, A] with a second critic */
int64_t pmg_sac_policy_grad_work_floats(const pmg_mlp* actor, int has_action, int has_critic2, int64_t batch, int64_t chunk_rows)
{
    const int64_t base = chunk_rows == 0 ? pmg_mlp_grad_work_floats(actor, batch) : pmg_mlp_grad_chunked_work_floats(actor, batch, chunk_rows);
    if (base < 0) return -1;
    const int A2 = actor->width[actor->num_layers];
    if (A2 < 2 || (A2 & 1) != 0) return -1;
    return base + (has_action ? 0 : batch * (A2 / 2)) + (has_critic2 ? batch * (A2 / 2) : 0);
}

int pmg_sac_policy_grad_device(pmg_env* e, const pmg_mlp* actor, const pmg_mlp* critic1, const pmg_mlp* critic2, const pmg_sac_policy_grad* g, int64_t chunk_rows)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_sac_policy_grad_device";
    PmgMlp P, Q1, Q2;
    if (int rc = mlp_of(e, actor, "pmg_sac_policy_grad_device (actor)", P)) return rc;
    if (int rc = gaussian_of(e, P, "pmg_sac_policy_grad_device (actor)")) return rc;
    if (int rc = mlp_of(e, critic1, "pmg_sac_policy_grad_device (critic 1)", Q1)) return rc;
    const int Dx = P.width[0], A = P.width[P.L] / 2;
    if (int rc = critic_of(e, Q1, Dx + A, "pmg_sac_policy_grad_device (critic 1)")) return rc;
    if (critic2) {
        if (int rc = mlp_of(e, critic2, "pmg_sac_policy_grad_device (critic 2)", Q2)) return rc;
        if (int rc = critic_of(e, Q2, Dx + A, "pmg_sac_policy_grad_device (critic 2)")) return rc;
    } else
        Q2 = Q1;
    if (!g) return fail(e, PMG_E_INVALID, "%s: g is null", who);
    if (g->struct_size != (int32_t)sizeof(pmg_sac_policy_grad)) return fail(e, PMG_E_INVALID, "%s: struct_size %d != %zu", who, g->struct_size, sizeof(pmg_sac_policy_grad));
    if (g->batch < 0) return fail(e, PMG_E_INVALID, "%s: batch %lld is negative", who, (long long)g->batch);
    if (!g->d_x) return fail(e, PMG_E_INVALID, "%s: d_x is null", who);
    if (!std::isfinite(g->gscale) || !std::isfinite(g->lscale)) return fail(e, PMG_E_INVALID, "%s: gscale %g or lscale %g is not finite", who, (double)g->gscale, (double)g->lscale);
    if (!(g->alpha >= 0.f) || std::isinf(g->alpha)) return fail(e, PMG_E_INVALID, "%s: alpha %g must be finite and >= 0", who, (double)g->alpha);
    if (int rc = sac_clamp_of(e, g->ls_lo, g->ls_hi, who)) return rc;
    if (g->row_offset < 0) return fail(e, PMG_E_INVALID, "%s: row_offset %lld is negative", who, (long long)g->row_offset);
    float* const d_q2 = critic2 ? g->d_q2 : nullptr;
    if (!g->grads && !g->d_action && !g->d_logp && !g->d_q1 && !d_q2 && !g->d_gaction && !g->d_ghead)
        return fail(e, PMG_E_INVALID, "%s: grads, d_action, d_logp, d_q1, d_q2, d_gaction and d_ghead are all null: nothing to do", who);
    if (g->grads) if (int rc = params_of(e, P, g->grads, false, who, "grads")) return rc;
    if ((((size_t)g->d_x | (size_t)g->d_alpha | (size_t)g->d_action | (size_t)g->d_logp | (size_t)g->d_q1 | (size_t)g->d_q2 | (size_t)g->d_gaction | (size_t)g->d_ghead |
          (size_t)g->d_work) & 3) != 0)
        return fail(e, PMG_E_INVALID, "%s: a float pointer is not aligned to 4 bytes", who);
    if (g->x_stride < Dx || (g->d_action && g->action_stride < A) || (g->d_gaction && g->gaction_stride < A) || (g->d_ghead && g->ghead_stride < 2 * A))
        return fail(e, PMG_E_INVALID, "%s: a stride is smaller than its width", who);
    if (chunk_rows < 0 || chunk_rows == 1 || (chunk_rows & 1)) return fail(e, PMG_E_INVALID, "%s: chunk_rows %lld must be 0 (one chain) or even and >= 2", who, (long long)chunk_rows);
    const int64_t C = chunk_rows ? g->batch / chunk_rows + (g->batch % chunk_rows != 0) : 1;
    if (C > PMG_GRAD_MAX_CHUNKS)
        return fail(e, PMG_E_INVALID, "%s: batch %lld in chunks of %lld rows is %lld chunks, more than %d", who, (long long)g->batch, (long long)chunk_rows, (long long)C, PMG_GRAD_MAX_CHUNKS);
    const bool chunked = g->grads && C > 1;
    const int64_t base = pmg_mlp_grad_work_floats(actor, g->batch);
    const int64_t mine = chunked ? pmg_mlp_grad_chunked_work_floats(actor, g->batch, chunk_rows) : base;   /* the actor's part of the workspace */
    if (mine < 0) return fail(e, PMG_E_INVALID, "%s: batch %lld is too large", who, (long long)g->batch);
    const int64_t need = mine + (g->d_action ? 0 : g->batch * A) + (critic2 ? g->batch * A : 0);
    if (!g->d_work || g->work_floats < need) return fail(e, PMG_E_INVALID, "%s: d_work is null or work_floats %lld < %lld", who, (long long)g->work_floats, (long long)need);
    if (g->batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    P.B = Q1.B = Q2.B = g->batch;
    PmgGrad G;
    memset(&G, 0, sizeof(G));
    G.x = g->d_x; G.xs = g->x_stride; G.x_dim = Dx;
    G.grads = g->grads ? 1 : 0;
    for (int l = 0; l < P.L && g->grads; l++) { G.dw[l] = g->grads->d_weight[l]; G.db[l] = P.b[l] ? g->grads->d_bias[l] : nullptr; }
    pmg_grad_work_layout(P, P.B, g->d_work, &G);
    PmgSacPolicy X;
    memset(&X, 0, sizeof(X));
    X.H.ls_lo = g->ls_lo; X.H.ls_hi = g->ls_hi; X.H.sample = g->sample != 0; X.H.seed = g->seed; X.H.counter = g->counter;
    X.H.row_offset = (unsigned long long)g->row_offset;
    X.H.logp = g->d_logp;
    float* extra = g->d_work + mine;
    if (g->d_action) { X.H.action = g->d_action; X.H.as = g->action_stride; }
    else { X.H.action = extra; X.H.as = A; extra += g->batch * A; }
    X.gscale = g->gscale; X.lscale = g->lscale; X.alpha = g->alpha; X.d_alpha = g->d_alpha;
    X.twin = critic2 != nullptr;
    X.q1 = g->d_q1; X.q2 = d_q2;
    X.ga = g->d_gaction; X.gas = g->gaction_stride;
    X.ghead = g->d_ghead; X.ghs = g->ghead_stride;
    if (g->grads) { X.stash = G.wd[P.L - 1]; X.ss = 2 * A; }
    else if (g->d_ghead) { X.stash = g->d_ghead; X.ss = g->ghead_stride; }
    X.ga1 = critic2 ? extra : nullptr;
    if (!chunked) {
        HIP_TRY(e, pmg_launch_sac_policy_grad(P, Q1, Q2, G, X, nullptr, nullptr, e->stream));
        return PMG_OK;
    }
    PmgSegs T;
    segs_of(P, g->grads, g->grads->d_weight, g->grads->d_bias, nullptr, nullptr, T);
    PmgGradChunks K;
    memset(&K, 0, sizeof(K));
    K.R = chunk_rows; K.C = C; K.P = grad_chunk_params(actor); K.tiles = pmg_grad_w_tiles(P); K.part = g->d_work + base;
    for (int l = 0, n = 0; l < P.L; l++) {                          /* tensor n of T starts at T.end[n - 1] */
        K.pw[l] = K.part + (n ? T.end[n - 1] : 0);
        n++;
        if (P.b[l]) { K.pb[l] = K.part + T.end[n - 1]; n++; }
    }
    HIP_TRY(e, pmg_launch_sac_policy_grad(P, Q1, Q2, G, X, &K, &T, e->stream));
    return PMG_OK;
}

int pmg_sac_alpha_device(pmg_env* e, const pmg_sac_alpha* a)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_sac_alpha_device";
    if (!a) return fail(e, PMG_E_INVALID, "%s: a is null", who);
    if (a->struct_size != (int32_t)sizeof(pmg_sac_alpha)) return fail(e, PMG_E_INVALID, "%s: struct_size %d != %zu", who, a->struct_size, sizeof(pmg_sac_alpha));
    if (a->batch <= 0) return fail(e, PMG_E_INVALID, "%s: batch %lld must be >= 1", who, (long long)a->batch);
    if (!std::isfinite(a->target_entropy)) return fail(e, PMG_E_INVALID, "%s: target_entropy %g is not finite", who, (double)a->target_entropy);
    if (!std::isfinite(a->lr) || !std::isfinite(a->eps) || !(a->eps >= 0.f)) return fail(e, PMG_E_INVALID, "%s: lr %g must be finite, eps %g finite and >= 0", who, (double)a->lr, (double)a->eps);
    if (!(a->beta1 >= 0.f && a->beta1 < 1.f) || !(a->beta2 >= 0.f && a->beta2 < 1.f)) return fail(e, PMG_E_INVALID, "%s: betas %g / %g must lie in [0, 1)", who, (double)a->beta1, (double)a->beta2);
    if (a->step < 1) return fail(e, PMG_E_INVALID, "%s: step %lld must be >= 1", who, (long long)a->step);
    if (!a->d_logp || !a->d_state) return fail(e, PMG_E_INVALID, "%s: d_logp or d_state is null", who);
    if ((((size_t)a->d_logp | (size_t)a->d_state) & 3) != 0) return fail(e, PMG_E_INVALID, "%s: a float pointer is not aligned to 4 bytes", who);
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    /* pmg_mlp_adam_device's derived constants */
    const double c1 = 1.0 - pow((double)a->beta1, (double)a->step), c2 = 1.0 - pow((double)a->beta2, (double)a->step);
    PmgSacAlpha X;
    X.logp = a->d_logp; X.B = a->batch; X.target_entropy = a->target_entropy; X.state = a->d_state;
    X.A.beta1 = a->beta1; X.A.beta2 = a->beta2;
    X.A.omb1 = (float)(1.0 - (double)a->beta1); X.A.omb2 = (float)(1.0 - (double)a->beta2);
    X.A.step_size = (float)((double)a->lr / c1); X.A.rsc2 = (float)(1.0 / sqrt(c2)); X.A.eps = a->eps;
    HIP_TRY(e, pmg_launch_sac_alpha(X, e->stream));
    return PMG_OK;
}

/* ---- PPO on whole rollouts: GAE, the advantage normaliser, the clipped-surrogate gradient, the minibatch statistics ---- */
/* an output table of pmg_gae_device holds T x N distinct elements by the rule of include/pmg.h: a = |ts| >= 1 when T > 1, b = |es| >= 1 when
 * N > 1, and a >= N b or b >= T a.  T N < 2^31, so the products overflow only when the stride they are compared with is beyond 2^31 too */
static bool gae_out_ok(int64_t T, int64_t N, int64_t ts, int64_t es)
{
    if (T <= 0 || N <= 0) return true;                             /* an empty table */
    if (ts == INT64_MIN || es == INT64_MIN) return false;
    const int64_t a = ts < 0 ? -ts : ts, b = es < 0 ? -es : es;
    if ((T > 1 && a == 0) || (N > 1 && b == 0)) return false;
    const bool time_major = b == 0 || a / b >= N, env_major = a == 0 || b / a >= T;   /* floor(a / b) >= N iff a >= N b */
    return time_major || env_major;
}
int pmg_gae_device(pmg_env* e, const pmg_gae* g)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_gae_device";
    if (!g) return fail(e, PMG_E_INVALID, "%s: g is null", who);
    if (g->struct_size != (int32_t)sizeof(pmg_gae)) return fail(e, PMG_E_INVALID, "%s: struct_size %d != %zu", who, g->struct_size, sizeof(pmg_gae));
    if (!(g->gamma >= 0.f && g->gamma <= 1.f) || !(g->lambda >= 0.f && g->lambda <= 1.f))
        return fail(e, PMG_E_INVALID, "%s: gamma %g and lambda %g must lie in [0, 1]", who, (double)g->gamma, (double)g->lambda);
    if (g->steps < 0 || g->envs < 0) return fail(e, PMG_E_INVALID, "%s: steps %lld or envs %lld is negative", who, (long long)g->steps, (long long)g->envs);
    if (g->steps > 0 && g->envs > 0 && (g->steps >= (1ll << 31) || g->envs >= (1ll << 31) || g->steps * g->envs >= (1ll << 31)))
        return fail(e, PMG_E_INVALID, "%s: steps %lld x envs %lld is 2^31 or more", who, (long long)g->steps, (long long)g->envs);
    if (!g->d_reward || !g->d_value || !g->d_value_next || !g->d_adv) return fail(e, PMG_E_INVALID, "%s: d_reward, d_value, d_value_next or d_adv is null", who);
    if ((((size_t)g->d_reward | (size_t)g->d_value | (size_t)g->d_value_next | (size_t)g->d_cut | (size_t)g->d_terminal | (size_t)g->d_adv | (size_t)g->d_ret) & 3) != 0)
        return fail(e, PMG_E_INVALID, "%s: a float pointer is not aligned to 4 bytes", who);
    if (!gae_out_ok(g->steps, g->envs, g->adv_time_stride, g->adv_env_stride) ||
        (g->d_ret && !gae_out_ok(g->steps, g->envs, g->ret_time_stride, g->ret_env_stride)))
        return fail(e, PMG_E_INVALID, "%s: the strides of d_adv (%lld, %lld) or d_ret (%lld, %lld) could put two (t, i) of %lld x %lld on one element", who,
                    (long long)g->adv_time_stride, (long long)g->adv_env_stride, (long long)g->ret_time_stride, (long long)g->ret_env_stride, (long long)g->steps,
                    (long long)g->envs);
    if (g->steps == 0 || g->envs == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    PmgGae X;
    memset(&X, 0, sizeof(X));
    X.T = g->steps; X.N = g->envs; X.gamma = g->gamma; X.gl = g->gamma * g->lambda;
    X.reward = {g->d_reward, g->reward_time_stride, g->reward_env_stride};
    X.value = {g->d_value, g->value_time_stride, g->value_env_stride};
    X.value_next = {g->d_value_next, g->value_next_time_stride, g->value_next_env_stride};
    X.cut = {g->d_cut, g->cut_time_stride, g->cut_env_stride};
    X.term = {g->d_terminal, g->terminal_time_stride, g->terminal_env_stride};
    X.adv = g->d_adv; X.ats = g->adv_time_stride; X.aes = g->adv_env_stride;
    X.ret = g->d_ret; X.rts = g->ret_time_stride; X.res = g->ret_env_stride;
    HIP_TRY(e, pmg_launch_gae(X, e->stream));
    return PMG_OK;
}

int pmg_adv_stats_device(pmg_env* e, const pmg_adv_stats* s)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_adv_stats_device";
    if (!s) return fail(e, PMG_E_INVALID, "%s: s is null", who);
    if (s->struct_size != (int32_t)sizeof(pmg_adv_stats)) return fail(e, PMG_E_INVALID, "%s: struct_size %d != %zu", who, s->struct_size, sizeof(pmg_adv_stats));
    if (s->count < 0) return fail(e, PMG_E_INVALID, "%s: count %lld is negative", who, (long long)s->count);
    if (s->ddof != 0 && s->ddof != 1) return fail(e, PMG_E_INVALID, "%s: ddof %d must be 0 or 1", who, s->ddof);
    if (s->count >= 1 && s->count - s->ddof < 1) return fail(e, PMG_E_INVALID, "%s: count %lld - ddof %d is below 1", who, (long long)s->count, s->ddof);
    if (!std::isfinite(s->eps) || !(s->eps >= 0.f)) return fail(e, PMG_E_INVALID, "%s: eps %g must be finite and >= 0", who, (double)s->eps);
    if (!s->d_x || !s->d_stats) return fail(e, PMG_E_INVALID, "%s: d_x or d_stats is null", who);
    if ((((size_t)s->d_x | (size_t)s->d_stats) & 3) != 0) return fail(e, PMG_E_INVALID, "%s: a float pointer is not aligned to 4 bytes", who);
    if (s->count == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    PmgAdvStats X;
    X.x = s->d_x; X.M = s->count; X.ddof = s->ddof; X.eps = s->eps; X.stats = s->d_stats;
    HIP_TRY(e, pmg_launch_adv_stats(X, e->stream));
    return PMG_OK;
}

int pmg_adv_apply_device(pmg_env* e, const float* d_x, int64_t count, const float* d_stats, float* d_y)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_adv_apply_device";
    if (count < 0) return fail(e, PMG_E_INVALID, "%s: count %lld is negative", who, (long long)count);
    if (!d_x || !d_stats || !d_y) return fail(e, PMG_E_INVALID, "%s: d_x, d_stats or d_y is null", who);
    if ((((size_t)d_x | (size_t)d_stats | (size_t)d_y) & 3) != 0) return fail(e, PMG_E_INVALID, "%s: a float pointer is not aligned to 4 bytes", who);
    if (count == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, pmg_launch_adv_apply(d_x, count, d_stats, d_y, e->stream));
    return PMG_OK;
}

/* the clip of the surrogate; 0 or PMG_E_INVALID */
static int ppo_clip_of(pmg_env* e, float lo, float hi, const char* who)
{
    if (std::isnan(lo) || std::isnan(hi) || lo < 0.f || lo > hi) return fail(e, PMG_E_INVALID, "%s: clip_lo %g / clip_hi %g must be ordered, clip_lo >= 0", who, (double)lo, (double)hi);
    return PMG_OK;
}
/* the workspace is the actor's: pmg_mlp_grad_work_floats, or with chunk_rows the chunked figure */
int64_t pmg_ppo_policy_grad_work_floats(const pmg_mlp* actor, int64_t batch, int64_t chunk_rows)
{
    const int64_t base = chunk_rows == 0 ? pmg_mlp_grad_work_floats(actor, batch) : pmg_mlp_grad_chunked_work_floats(actor, batch, chunk_rows);
    if (base < 0) return -1;
    const int A2 = actor->width[actor->num_layers];
    if (A2 < 2 || (A2 & 1) != 0) return -1;
    return base;
}

int pmg_ppo_policy_grad_device(pmg_env* e, const pmg_mlp* actor, const pmg_ppo_policy_grad* g, int64_t chunk_rows)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_ppo_policy_grad_device";
    PmgMlp P;
    if (int rc = mlp_of(e, actor, who, P)) return rc;
    if (int rc = gaussian_of(e, P, who)) return rc;
    const int Dx = P.width[0], A = P.width[P.L] / 2;
    if (!g) return fail(e, PMG_E_INVALID, "%s: g is null", who);
    if (g->struct_size != (int32_t)sizeof(pmg_ppo_policy_grad)) return fail(e, PMG_E_INVALID, "%s: struct_size %d != %zu", who, g->struct_size, sizeof(pmg_ppo_policy_grad));
    if (g->batch < 0) return fail(e, PMG_E_INVALID, "%s: batch %lld is negative", who, (long long)g->batch);
    if (!g->d_x || !g->d_preact_old || !g->d_noise || !g->d_adv) return fail(e, PMG_E_INVALID, "%s: d_x, d_preact_old, d_noise or d_adv is null", who);
    if (!std::isfinite(g->pscale) || !std::isfinite(g->escale)) return fail(e, PMG_E_INVALID, "%s: pscale %g or escale %g is not finite", who, (double)g->pscale, (double)g->escale);
    if (int rc = ppo_clip_of(e, g->clip_lo, g->clip_hi, who)) return rc;
    if (int rc = sac_clamp_of(e, g->ls_lo, g->ls_hi, who)) return rc;
    if (!g->grads && !g->d_ratio && !g->d_logratio && !g->d_clipped && !g->d_ghead)
        return fail(e, PMG_E_INVALID, "%s: grads, d_ratio, d_logratio, d_clipped and d_ghead are all null: nothing to do", who);
    if (g->grads) if (int rc = params_of(e, P, g->grads, false, who, "grads")) return rc;
    if ((((size_t)g->d_x | (size_t)g->d_preact_old | (size_t)g->d_noise | (size_t)g->d_adv | (size_t)g->d_ratio | (size_t)g->d_logratio | (size_t)g->d_ghead |
          (size_t)g->d_work) & 3) != 0)
        return fail(e, PMG_E_INVALID, "%s: a float pointer is not aligned to 4 bytes", who);
    if (g->x_stride < Dx || g->preact_old_stride < 2 * A || g->noise_stride < A || (g->d_ghead && g->ghead_stride < 2 * A))
        return fail(e, PMG_E_INVALID, "%s: a stride is smaller than its width", who);
    if (chunk_rows < 0 || chunk_rows == 1 || (chunk_rows & 1)) return fail(e, PMG_E_INVALID, "%s: chunk_rows %lld must be 0 (one chain) or even and >= 2", who, (long long)chunk_rows);
    const int64_t C = chunk_rows ? g->batch / chunk_rows + (g->batch % chunk_rows != 0) : 1;
    if (C > PMG_GRAD_MAX_CHUNKS)
        return fail(e, PMG_E_INVALID, "%s: batch %lld in chunks of %lld rows is %lld chunks, more than %d", who, (long long)g->batch, (long long)chunk_rows, (long long)C, PMG_GRAD_MAX_CHUNKS);
    const bool chunked = g->grads && C > 1;
    const int64_t base = pmg_mlp_grad_work_floats(actor, g->batch);
    const int64_t need = chunked ? pmg_mlp_grad_chunked_work_floats(actor, g->batch, chunk_rows) : base;
    if (need < 0) return fail(e, PMG_E_INVALID, "%s: batch %lld is too large", who, (long long)g->batch);
    if (g->grads && (!g->d_work || g->work_floats < need))
        return fail(e, PMG_E_INVALID, "%s: d_work is null or work_floats %lld < %lld", who, (long long)g->work_floats, (long long)need);
    if (g->batch == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    P.B = g->batch;
    PmgGrad G;
    memset(&G, 0, sizeof(G));
    G.x = g->d_x; G.xs = g->x_stride; G.x_dim = Dx;
    G.grads = g->grads ? 1 : 0;
    for (int l = 0; l < P.L && g->grads; l++) { G.dw[l] = g->grads->d_weight[l]; G.db[l] = P.b[l] ? g->grads->d_bias[l] : nullptr; }
    if (g->grads) pmg_grad_work_layout(P, P.B, g->d_work, &G);
    PmgPpoPolicy X;
    memset(&X, 0, sizeof(X));
    X.pscale = g->pscale; X.escale = g->escale; X.clip_lo = g->clip_lo; X.clip_hi = g->clip_hi; X.ls_lo = g->ls_lo; X.ls_hi = g->ls_hi;
    X.zo = g->d_preact_old; X.zos = g->preact_old_stride; X.n = g->d_noise; X.ns = g->noise_stride; X.adv = g->d_adv;
    X.ratio = g->d_ratio; X.logratio = g->d_logratio; X.clipped = g->d_clipped;
    X.ghead = g->d_ghead; X.ghs = g->ghead_stride;
    if (g->grads) { X.stash = G.wd[P.L - 1]; X.ss = 2 * A; }
    else if (g->d_ghead) { X.stash = g->d_ghead; X.ss = g->ghead_stride; }
    if (!chunked) {
        HIP_TRY(e, pmg_launch_ppo_policy_grad(P, G, X, nullptr, nullptr, e->stream));
        return PMG_OK;
    }
    PmgSegs T;
    segs_of(P, g->grads, g->grads->d_weight, g->grads->d_bias, nullptr, nullptr, T);
    PmgGradChunks K;
    memset(&K, 0, sizeof(K));
    K.R = chunk_rows; K.C = C; K.P = grad_chunk_params(actor); K.tiles = pmg_grad_w_tiles(P); K.part = g->d_work + base;
    for (int l = 0, n = 0; l < P.L; l++) {                          /* tensor n of T starts at T.end[n - 1] */
        K.pw[l] = K.part + (n ? T.end[n - 1] : 0);
        n++;
        if (P.b[l]) { K.pb[l] = K.part + T.end[n - 1]; n++; }
    }
    HIP_TRY(e, pmg_launch_ppo_policy_grad(P, G, X, &K, &T, e->stream));
    return PMG_OK;
}

int pmg_ppo_stats_device(pmg_env* e, const pmg_ppo_stats* s)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_ppo_stats_device";
    if (!s) return fail(e, PMG_E_INVALID, "%s: s is null", who);
    if (s->struct_size != (int32_t)sizeof(pmg_ppo_stats)) return fail(e, PMG_E_INVALID, "%s: struct_size %d != %zu", who, s->struct_size, sizeof(pmg_ppo_stats));
    if (s->batch <= 0) return fail(e, PMG_E_INVALID, "%s: batch %lld must be >= 1", who, (long long)s->batch);
    if (int rc = ppo_clip_of(e, s->clip_lo, s->clip_hi, who)) return rc;
    if (!s->d_ratio || !s->d_logratio || !s->d_clipped || !s->d_adv || !s->d_stats) return fail(e, PMG_E_INVALID, "%s: a pointer is null", who);
    if ((((size_t)s->d_ratio | (size_t)s->d_logratio | (size_t)s->d_adv | (size_t)s->d_stats) & 3) != 0)
        return fail(e, PMG_E_INVALID, "%s: a float pointer is not aligned to 4 bytes", who);
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    PmgPpoStats X;
    X.ratio = s->d_ratio; X.logratio = s->d_logratio; X.clipped = s->d_clipped; X.adv = s->d_adv; X.B = s->batch;
    X.clip_lo = s->clip_lo; X.clip_hi = s->clip_hi; X.stats = s->d_stats;
    HIP_TRY(e, pmg_launch_ppo_stats(X, e->stream));
    return PMG_OK;
}

/* state row = hot(32) | cold(16) | goal(16) | blocks(13 nb)    */
int pmg_get_state(pmg_env* e, float* state)
{
    if (!e || !state) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    size_t N = (size_t)e->dims.num_envs;
    int S = e->dims.state_dim, nbd = pmg::BLOCK_DIM * e->nb;
    std::vector<float> hot(N * pmg::HOT_DIM), cold(N * pmg::COLD_DIM), goal(N * pmg::GOAL_DIM), blk(N * (nbd ? nbd : 1));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(hot.data(), e->P.hot, hot.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(e, hipMemcpy(cold.data(), e->P.cold, cold.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(e, hipMemcpy(goal.data(), e->P.goal, goal.size() * sizeof(float), hipMemcpyDeviceToHost));
    if (nbd) HIP_TRY(e, hipMemcpy(blk.data(), e->P.blocks, N * nbd * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; i++) {
        float* s = state + i * S;
        memcpy(s, &hot[i * pmg::HOT_DIM], sizeof(float) * pmg::HOT_DIM);
        memcpy(s + 32, &cold[i * pmg::COLD_DIM], sizeof(float) * pmg::COLD_DIM);
        memcpy(s + 48, &goal[i * pmg::GOAL_DIM], sizeof(float) * pmg::GOAL_DIM);
        if (nbd) memcpy(s + 64, &blk[i * nbd], sizeof(float) * nbd);
    }
    if (e->P.curr) {
        std::vector<float> cs(N * pmg::CURR_DIM);
        HIP_TRY(e, hipMemcpy(cs.data(), e->P.curr, cs.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < N; i++) memcpy(state + i * S + 64 + nbd, &cs[i * pmg::CURR_DIM], sizeof(float) * pmg::CURR_DIM);
    }
    return PMG_OK;
}

int pmg_set_state(pmg_env* e, const float* state)
{
    if (!e || !state) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    size_t N = (size_t)e->dims.num_envs;
    int S = e->dims.state_dim, nbd = pmg::BLOCK_DIM * e->nb;
    std::vector<float> hot(N * pmg::HOT_DIM), cold(N * pmg::COLD_DIM), goal(N * pmg::GOAL_DIM), blk(N * (nbd ? nbd : 1));
    for (size_t i = 0; i < N; i++) {
        const float* s = state + i * S;
        memcpy(&hot[i * pmg::HOT_DIM], s, sizeof(float) * pmg::HOT_DIM);
        memcpy(&cold[i * pmg::COLD_DIM], s + 32, sizeof(float) * pmg::COLD_DIM);
        memcpy(&goal[i * pmg::GOAL_DIM], s + 48, sizeof(float) * pmg::GOAL_DIM);
        if (nbd) memcpy(&blk[i * nbd], s + 64, sizeof(float) * nbd);
    }
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(e->P.hot, hot.data(), hot.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(e->P.cold, cold.data(), cold.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(e->P.goal, goal.data(), goal.size() * sizeof(float), hipMemcpyHostToDevice));
    if (nbd) HIP_TRY(e, hipMemcpy(e->P.blocks, blk.data(), N * nbd * sizeof(float), hipMemcpyHostToDevice));
    if (e->P.curr) {
        std::vector<float> cs(N * pmg::CURR_DIM);
        for (size_t i = 0; i < N; i++) memcpy(&cs[i * pmg::CURR_DIM], state + i * S + 64 + nbd, sizeof(float) * pmg::CURR_DIM);
        HIP_TRY(e, hipMemcpy(e->P.curr, cs.data(), cs.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    e->ever_reset = true;
    /* the packed rows still show the previous state: a reset of NOBODY re-derives every env's observation and goal */
    HIP_TRY(e, hipMemsetAsync(e->d_mask, 0, N, e->stream));
    if (int rc = rows_writer_waits_for_gather(e)) return rc;
    HIP_TRY(e, pmg_launch_reset(e->P, e->d_mask, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return PMG_OK;
}

int pmg_get_rng(pmg_env* e, uint32_t* words)
{
    if (!e || !words) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(words, e->P.rng, (size_t)e->dims.num_envs * 625 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return PMG_OK;
}
int pmg_set_rng(pmg_env* e, const uint32_t* words)
{
    if (!e || !words) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    for (int i = 0; i < e->dims.num_envs; i++)
        if (words[(size_t)i * 625 + 624] > 624u) return fail(e, PMG_E_INVALID, "pmg_set_rng: env %d has cursor %u > 624", i, words[(size_t)i * 625 + 624]);
    HIP_TRY(e, hipMemcpy(e->P.rng, words, (size_t)e->dims.num_envs * 625 * sizeof(uint32_t), hipMemcpyHostToDevice));
    return PMG_OK;
}

int pmg_set_goal(pmg_env* e, const uint8_t* mask, const float* goals)
{
    if (!e || !goals) return PMG_E_INVALID;
    if (e->P.chest >= 0) return fail(e, PMG_E_INVALID, "pmg_set_goal: the chest tasks have no static target");
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    size_t N = (size_t)e->dims.num_envs;
    int G = e->dims.goal_dim;
    std::vector<float> goal(N * pmg::GOAL_DIM);
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(goal.data(), e->P.goal, goal.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; i++)
        if (!mask || mask[i]) memcpy(&goal[i * pmg::GOAL_DIM], goals + i * G, sizeof(float) * (G < 15 ? G : 15)); /* static targets only */
    HIP_TRY(e, hipMemcpy(e->P.goal, goal.data(), goal.size() * sizeof(float), hipMemcpyHostToDevice));
    return PMG_OK;
}

int pmg_set_sub_goal(pmg_env* e, const uint8_t* mask, int32_t sub_goal_ind)
{
    if (!e) return PMG_E_INVALID;
    if (!e->cfg.task_decomposition) return fail(e, PMG_E_STATE, "pmg_set_sub_goal: the handle was created without task_decomposition");
    int steps = e->cfg.grip_informed_goal ? 2 * e->nb : e->nb; /* kuka_multi_step_envs.py:13-17 */
    if (e->P.chest >= 0) steps = (e->cfg.grip_informed_goal ? e->nb * (e->P.grasping ? 3 : 2) : e->nb) + 1; /* :238-242, 388-392 */
    if (sub_goal_ind < -1 || sub_goal_ind >= steps) return fail(e, PMG_E_INVALID, "pmg_set_sub_goal: index %d out of range [-1, %d)", sub_goal_ind, steps);
    if (!e->ever_reset) return fail(e, PMG_E_STATE, "pmg_set_sub_goal: reset first");
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    const unsigned char* dm = nullptr;
    if (mask) {
        HIP_TRY(e, hipMemcpyAsync(e->d_mask, mask, (size_t)e->dims.num_envs, hipMemcpyHostToDevice, e->stream));
        dm = e->d_mask;
    }
    if (int rc = rows_writer_waits_for_gather(e)) return rc;
    HIP_TRY(e, pmg_launch_sub_goal(e->P, dm, sub_goal_ind < 0 ? steps - 1 : sub_goal_ind, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return PMG_OK;
}

int pmg_curriculum_update(pmg_env* e, int32_t enabled)
{
    if (!e) return PMG_E_INVALID;
    if (!e->cfg.use_curriculum) return fail(e, PMG_E_STATE, "pmg_curriculum_update: the handle was created without use_curriculum");
    e->P.curriculum_update = enabled != 0;
    return PMG_OK;
}

int pmg_curriculum_read(pmg_env* e, int32_t* level, int32_t* goal_step, float* prob, float* generated)
{
    if (!e) return PMG_E_INVALID;
    if (!e->cfg.use_curriculum) return fail(e, PMG_E_STATE, "pmg_curriculum_read: the handle was created without use_curriculum");
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    size_t N = (size_t)e->dims.num_envs;
    std::vector<float> cs(N * pmg::CURR_DIM), cold(N * pmg::COLD_DIM);
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(cs.data(), e->P.curr, cs.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(e, hipMemcpy(cold.data(), e->P.cold, cold.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; i++) {
        if (level) level[i] = (int32_t)cold[i * pmg::COLD_DIM + 7];
        const int ncur = e->P.chest >= 0 ? e->nb + 1 : e->nb, NC = e->P.chest >= 0 ? 6 : 5;
        if (goal_step) goal_step[i] = (int32_t)cs[i * pmg::CURR_DIM + 2 * NC];
        for (int b = 0; b < ncur; b++) {
            if (prob) prob[i * ncur + b] = cs[i * pmg::CURR_DIM + b];
            if (generated) generated[i * ncur + b] = cs[i * pmg::CURR_DIM + NC + b];
        }
    }
    return PMG_OK;
}

int pmg_comm_unique_id(uint8_t id[128])
{
    ncclUniqueId u;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    if (ncclGetUniqueId(&u) != ncclSuccess) return PMG_E_COMM;
    memcpy(id, &u, 128);
    return PMG_OK;
}
int pmg_comm_init(pmg_env* e, int rank, int nranks, const uint8_t id[128])
{
    if (!e || !id || nranks < 1 || rank < 0 || rank >= nranks) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    ncclUniqueId u;
    memcpy(&u, id, 128);
    ncclResult_t rc = ncclCommInitRank(&e->comm, nranks, u, rank);
    if (rc != ncclSuccess) return fail(e, PMG_E_COMM, "ncclCommInitRank -> %s", ncclGetErrorString(rc));
    e->rank = rank;
    e->nranks = nranks;
    return PMG_OK;
}
int pmg_allgather_packed(pmg_env* e, float* d_gathered)
{
    if (!e || !d_gathered) return PMG_E_INVALID;
    if (!e->comm) return fail(e, PMG_E_STATE, "pmg_allgather_packed: pmg_comm_init was not called");
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    size_t count = (size_t)e->dims.num_envs * e->dims.packed_dim;
    if (e->cv_n == EVENT_POOL) drain_comm_events(e);
    /* the event pair counts only once both are recorded: a failed all-gather must not leave a new cv_a paired with a stale cv_b */
    const int i = e->cv_n;
    HIP_TRY(e, hipEventRecord(e->cv_a[i], e->stream));
    ncclResult_t rc = ncclAllGather(e->P.out, d_gathered, count, ncclFloat, e->comm, e->stream);
    if (rc != ncclSuccess) return fail(e, PMG_E_COMM, "ncclAllGather -> %s", ncclGetErrorString(rc));
    HIP_TRY(e, hipEventRecord(e->cv_b[i], e->stream));
    e->cv_n = i + 1;
    return PMG_OK;
}

/* ---- data-parallel learner: rank-ordered gradient and normaliser merge ---- */
/* a collective on the handle's stream needs the communicator and must be the only stream that uses it */
static int collective_of(pmg_env* e, const char* who)
{
    if (!e->comm) return fail(e, PMG_E_STATE, "%s: pmg_comm_init was not called", who);
    if (e->overlap) return fail(e, PMG_E_STATE, "%s: pmg_comm_overlap is enabled -- its all-gathers run on the communication stream, and two streams must not "
                                                "issue collectives on one communicator; switch it off first", who);
    return PMG_OK;
}
static int allgather_floats(pmg_env* e, const char* who, const float* src, size_t count, float* dst)
{
    ncclResult_t rc = ncclAllGather(src, dst, count, ncclFloat, e->comm, e->stream);
    if (rc != ncclSuccess) return fail(e, PMG_E_COMM, "%s: ncclAllGather of %zu floats per rank -> %s", who, count, ncclGetErrorString(rc));
    return PMG_OK;
}

int pmg_comm_info(pmg_env* e, int32_t* rank, int32_t* nranks)
{
    if (!e) return PMG_E_INVALID;
    if (!e->comm) return fail(e, PMG_E_STATE, "pmg_comm_info: pmg_comm_init was not called");
    if (rank) *rank = e->rank;
    if (nranks) *nranks = e->nranks;
    return PMG_OK;
}

int pmg_allgather_device(pmg_env* e, const float* d_src, int64_t count, float* d_gathered)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_allgather_device";
    if (int rc = collective_of(e, who)) return rc;
    if (count < 0 || count > (int64_t)1 << 40) return fail(e, PMG_E_INVALID, "%s: count %lld is negative or too large", who, (long long)count);
    if (!d_src || !d_gathered || ((((size_t)d_src | (size_t)d_gathered) & 3) != 0)) return fail(e, PMG_E_INVALID, "%s: a pointer is null or not aligned to 4 bytes", who);
    if (count == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    return allgather_floats(e, who, d_src, (size_t)count, d_gathered);
}

/* P of a validated network: the tensors the shape has, in the flat order of PmgSegs */
static long long param_floats_of(const PmgMlp& M)
{
    long long P = 0;
    for (int l = 0; l < M.L; l++) P += (long long)M.width[l + 1] * M.width[l] + (M.b[l] ? M.width[l + 1] : 0);
    return P;
}
int64_t pmg_mlp_param_floats(const pmg_mlp* shape)
{
    PmgMlp M;
    if (mlp_of(nullptr, shape, "pmg_mlp_param_floats", M) != PMG_OK) return -1;
    return param_floats_of(M);
}
/* nslots slots of P floats, slot_stride apart */
static int slots_of(pmg_env* e, const char* who, const float* d_slots, int64_t slot_stride, int64_t nslots, long long P)
{
    if (!d_slots || ((size_t)d_slots & 3) != 0) return fail(e, PMG_E_INVALID, "%s: d_slots is null or not aligned to 4 bytes", who);
    if (nslots < 1 || nslots > INT32_MAX) return fail(e, PMG_E_INVALID, "%s: nslots %lld must be >= 1", who, (long long)nslots);
    if (slot_stride < P) return fail(e, PMG_E_INVALID, "%s: slot_stride %lld is smaller than the %lld parameters of the network", who, (long long)slot_stride, P);
    return PMG_OK;
}

int pmg_mlp_params_pack_device(pmg_env* e, const pmg_mlp* shape, const pmg_mlp_params* src, float* d_flat)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_mlp_params_pack_device";
    PmgMlp M;
    if (int rc = mlp_of(e, shape, who, M)) return rc;
    if (int rc = params_of(e, M, src, true, who, "src")) return rc;
    if (!d_flat || ((size_t)d_flat & 3) != 0) return fail(e, PMG_E_INVALID, "%s: d_flat is null or not aligned to 4 bytes", who);
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    PmgSegs T;
    segs_of(M, src, src->d_weight, src->d_bias, nullptr, nullptr, T);
    HIP_TRY(e, pmg_launch_params_pack(T, d_flat, e->stream));
    return PMG_OK;
}

int pmg_mlp_params_merge_device(pmg_env* e, const pmg_mlp* shape, const float* d_slots, int64_t slot_stride, int64_t nslots, const pmg_mlp_params* out)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_mlp_params_merge_device";
    PmgMlp M;
    if (int rc = mlp_of(e, shape, who, M)) return rc;
    if (int rc = params_of(e, M, out, true, who, "out")) return rc;
    if (int rc = slots_of(e, who, d_slots, slot_stride, nslots, param_floats_of(M))) return rc;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    PmgSegs T;
    segs_of(M, out, out->d_weight, out->d_bias, nullptr, nullptr, T);
    HIP_TRY(e, pmg_launch_params_merge_ranks(T, d_slots, slot_stride, (int)nslots, e->stream));
    return PMG_OK;
}

/* everything pmg_mlp_adam_merge_device checks but the slots -> M, A and the table (T.g: grad_out's tensors, or param's when there is none) */
static int adam_merge_of(pmg_env* e, const char* who, const pmg_mlp* shape, const pmg_mlp_params* param, const pmg_mlp_params* grad_out,
                         const pmg_mlp_params* m, const pmg_mlp_params* v, const pmg_adam* a, PmgMlp& M, PmgAdam& A, PmgSegs& T)
{
    if (int rc = mlp_of(e, shape, who, M)) return rc;
    if (int rc = params_of(e, M, param, true, who, "param")) return rc;
    if (grad_out) if (int rc = params_of(e, M, grad_out, true, who, "grad_out")) return rc;
    if (int rc = params_of(e, M, m, true, who, "m")) return rc;
    if (int rc = params_of(e, M, v, true, who, "v")) return rc;
    if (int rc = adam_of(e, who, a, A)) return rc;
    const pmg_mlp_params* g = grad_out ? grad_out : param;
    segs_of(M, param, g->d_weight, g->d_bias, m, v, T);
    return PMG_OK;
}

int pmg_mlp_adam_merge_device(pmg_env* e, const pmg_mlp* shape, const pmg_mlp_params* param, const float* d_slots, int64_t slot_stride, int64_t nslots,
                              const pmg_mlp_params* grad_out, const pmg_mlp_params* m, const pmg_mlp_params* v, const pmg_adam* a)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_mlp_adam_merge_device";
    PmgMlp M; PmgAdam A; PmgSegs T;
    if (int rc = adam_merge_of(e, who, shape, param, grad_out, m, v, a, M, A, T)) return rc;
    if (int rc = slots_of(e, who, d_slots, slot_stride, nslots, param_floats_of(M))) return rc;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, pmg_launch_adam_merge_ranks(T, A, d_slots, slot_stride, (int)nslots, grad_out ? 1 : 0, e->stream));
    return PMG_OK;
}

int64_t pmg_mlp_allreduce_work_floats(const pmg_env* e, const pmg_mlp* shape)
{
    const int64_t P = pmg_mlp_param_floats(shape);
    if (!e || P < 0) return -1;
    return ((int64_t)e->nranks + 1) * P;
}
/* the workspace of an all-reduce: this rank's flat gradient in front, the nranks gathered slots behind it */
static int allreduce_work_of(pmg_env* e, const char* who, long long P, const float* d_work, int64_t work_floats)
{
    const long long need = ((long long)e->nranks + 1) * P;
    if (!d_work || ((size_t)d_work & 3) != 0 || work_floats < need)
        return fail(e, PMG_E_INVALID, "%s: d_work is null or not aligned to 4 bytes, or work_floats %lld < %lld", who, (long long)work_floats, need);
    return PMG_OK;
}

int pmg_mlp_grad_allreduce_device(pmg_env* e, const pmg_mlp* shape, const pmg_mlp_params* grads, float* d_work, int64_t work_floats)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_mlp_grad_allreduce_device";
    if (int rc = collective_of(e, who)) return rc;
    PmgMlp M;
    if (int rc = mlp_of(e, shape, who, M)) return rc;
    if (int rc = params_of(e, M, grads, true, who, "grads")) return rc;
    const long long P = param_floats_of(M);
    if (int rc = allreduce_work_of(e, who, P, d_work, work_floats)) return rc;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    PmgSegs T;
    segs_of(M, grads, grads->d_weight, grads->d_bias, nullptr, nullptr, T);
    HIP_TRY(e, pmg_launch_params_pack(T, d_work, e->stream));
    if (int rc = allgather_floats(e, who, d_work, (size_t)P, d_work + P)) return rc;
    HIP_TRY(e, pmg_launch_params_merge_ranks(T, d_work + P, P, e->nranks, e->stream));
    return PMG_OK;
}

int pmg_mlp_adam_allreduce_device(pmg_env* e, const pmg_mlp* shape, const pmg_mlp_params* param, const pmg_mlp_params* grads, const pmg_mlp_params* m,
                                  const pmg_mlp_params* v, const pmg_adam* a, float* d_work, int64_t work_floats)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_mlp_adam_allreduce_device";
    if (int rc = collective_of(e, who)) return rc;
    if (!grads) return fail(e, PMG_E_INVALID, "%s: grads is null", who);
    PmgMlp M; PmgAdam A; PmgSegs T;
    if (int rc = adam_merge_of(e, who, shape, param, grads, m, v, a, M, A, T)) return rc;
    const long long P = param_floats_of(M);
    if (int rc = allreduce_work_of(e, who, P, d_work, work_floats)) return rc;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, pmg_launch_params_pack(T, d_work, e->stream));          /* (T.g: this rank's gradient) */
    if (int rc = allgather_floats(e, who, d_work, (size_t)P, d_work + P)) return rc;
    HIP_TRY(e, pmg_launch_adam_merge_ranks(T, A, d_work + P, P, e->nranks, 0, e->stream));   /* grads keep this rank's own gradient */
    return PMG_OK;
}

/* one normaliser's collective update: this rank's partial rows, cut at the chunk of the GLOBAL batch, all ranks' rows gathered in rank order --
 * the partial rows of the unsharded update in index order --, then the unchanged merge */
static int norm_update_ranks_rows(pmg_env* e, const char* who, int which, const float* d_rows, int64_t row_stride, int64_t batch, long long chunk,
                                  const uint8_t* d_mask)
{
    pmg_env::Norm& nm = e->norm[which];
    const size_t P = 2 * (size_t)nm.D + 1;
    const int parts = (int)((batch + chunk - 1) / chunk);
    HIP_TRY(e, pmg_launch_norm_partial(d_rows, row_stride, batch, nm.D, chunk, 0, parts, d_mask, e->norm_clip_in, nm.part, e->stream));
    if (int rc = allgather_floats(e, who, (const float*)nm.part, 2 * P * (size_t)parts, e->norm_gather.f32())) return rc;
    HIP_TRY(e, pmg_launch_norm_merge((const double*)e->norm_gather.p, e->nranks * parts, nm.D, e->norm_eps, nm.tot, nm.der, e->stream));
    return PMG_OK;
}
/* the chunk of a collective update of batch_local rows per rank, checked; the gathered-partials buffer sized for rows of width D */
static int norm_ranks_of(pmg_env* e, const char* who, int64_t batch_local, int D, long long& chunk)
{
    if (batch_local > (int64_t)1 << 40) return fail(e, PMG_E_INVALID, "%s: batch_local %lld is too large", who, (long long)batch_local);
    chunk = pmg_norm_chunk((long long)e->nranks * batch_local);
    if (e->nranks > 1 && batch_local % chunk != 0)
        return fail(e, PMG_E_INVALID, "%s: batch_local %lld is no multiple of %lld, the chunk of the global batch of %d x %lld rows: a rank's rows must "
                                      "start and end on chunk boundaries", who, (long long)batch_local, chunk, e->nranks, (long long)batch_local);
    const size_t parts = (size_t)((batch_local + chunk - 1) / chunk);
    return e->norm_gather.reserve(e, (size_t)e->nranks * parts * (2 * (size_t)D + 1) * sizeof(double), who, "the gathered partial rows");
}

int pmg_norm_update_ranks_device(pmg_env* e, int which, const float* d_rows, int64_t row_stride, int64_t batch_local, const uint8_t* d_mask)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_norm_update_ranks_device";
    if (int rc = collective_of(e, who)) return rc;
    const pmg_env::Norm* nm = norm_of(e, which, who); if (!nm) return PMG_E_INVALID;
    if (!d_rows || ((size_t)d_rows & 3) != 0) return fail(e, PMG_E_INVALID, "%s: d_rows is null or not aligned to 4 bytes", who);
    if (batch_local < 0) return fail(e, PMG_E_INVALID, "%s: batch_local %lld is negative", who, (long long)batch_local);
    if (row_stride < nm->D) return fail(e, PMG_E_INVALID, "%s: row_stride %lld is smaller than the width %d", who, (long long)row_stride, nm->D);
    if (nm->D > PMG_NORM_MAX_D) return fail(e, PMG_E_INVALID, "%s: width %d beyond %d", who, nm->D, PMG_NORM_MAX_D);
    if (batch_local == 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    long long chunk;
    if (int rc = norm_ranks_of(e, who, batch_local, nm->D, chunk)) return rc;
    return norm_update_ranks_rows(e, who, which, d_rows, row_stride, batch_local, chunk, d_mask);
}

int pmg_norm_update_env_ranks_device(pmg_env* e, const uint8_t* d_mask)
{
    if (!e) return PMG_E_INVALID;
    const char* who = "pmg_norm_update_env_ranks_device";
    if (int rc = collective_of(e, who)) return rc;
    if (!e->ever_reset) return fail(e, PMG_E_STATE, "%s: reset() must be called (for all envs) first", who);
    const pmg_dims& d = e->dims;
    if ((long long)e->cfg.env_index_offset != (long long)e->rank * d.num_envs)
        return fail(e, PMG_E_INVALID, "%s: env_index_offset %d is not rank %d x num_envs %d: the ranks' envs must be the global envs in rank order", who,
                    e->cfg.env_index_offset, e->rank, d.num_envs);
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    long long chunk;
    const int widest = std::max(d.observation_dim, std::max(d.policy_state_dim, d.goal_dim));
    if (widest > PMG_NORM_MAX_D) return fail(e, PMG_E_INVALID, "%s: width %d beyond %d", who, widest, PMG_NORM_MAX_D);
    if (int rc = norm_ranks_of(e, who, d.num_envs, widest, chunk)) return rc;
    const float* rows = e->P.out;
    const int off[3] = {0, d.observation_dim, d.observation_dim + d.policy_state_dim + d.goal_dim};   /* observation, policy_state, desired_goal */
    for (int w = 0; w < 3; w++)
        if (int rc = norm_update_ranks_rows(e, who, w, rows + off[w], d.packed_dim, d.num_envs, chunk, d_mask)) return rc;
    return PMG_OK;
}

int pmg_comm_overlap(pmg_env* e, int32_t enabled)
{
    if (!e) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    if (!enabled) {
        if (e->overlap) {
            if (e->comm_stream) HIP_TRY(e, hipStreamSynchronize(e->comm_stream));
            e->gpending[0] = e->gpending[1] = false;
            e->last_gather = -1;
        }
        e->overlap = false;       /* (the rows stay where the last step wrote them: P.out keeps pointing at that buffer) */
        return PMG_OK;
    }
    if (!(e->out2[1] && e->comm_stream)) {
        /* everything into locals first: a failure half-way must not leave a handle that looks initialised (out2[0] set, the second
         * buffer / the stream / the events null) to the next call */
        const size_t bytes = (size_t)e->dims.num_envs * e->dims.packed_dim * sizeof(float);
        float* second = nullptr;
        hipStream_t cs = nullptr;
        hipEvent_t rows[2] = {nullptr, nullptr}, gdone[2] = {nullptr, nullptr};
        hipError_t rc = hipMalloc((void**)&second, bytes);
        if (rc == hipSuccess) rc = hipMemcpyAsync(second, e->P.out, bytes, hipMemcpyDeviceToDevice, e->stream);
        if (rc == hipSuccess) rc = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
        for (int b = 0; b < 2 && rc == hipSuccess; b++) {
            rc = hipEventCreateWithFlags(&rows[b], hipEventDisableTiming);
            if (rc == hipSuccess) rc = hipEventCreateWithFlags(&gdone[b], hipEventDisableTiming);
        }
        if (rc != hipSuccess) {
            (void)hipStreamSynchronize(e->stream);
            for (int b = 0; b < 2; b++) { if (rows[b]) (void)hipEventDestroy(rows[b]); if (gdone[b]) (void)hipEventDestroy(gdone[b]); }
            if (cs) (void)hipStreamDestroy(cs);
            if (second) (void)hipFree(second);
            return fail(e, second ? PMG_E_DEVICE : PMG_E_NOMEM, "pmg_comm_overlap: %s", hipGetErrorString(rc));
        }
        e->out2[0] = e->P.out; e->out2[1] = second;
        e->comm_stream = cs;
        for (int b = 0; b < 2; b++) { e->ev_rows[b] = rows[b]; e->ev_gdone[b] = gdone[b]; }
        e->out_phase = 0;
    }
    e->overlap = true;
    return PMG_OK;
}
int pmg_allgather_packed_async(pmg_env* e, float* d_gathered)
{
    if (!e || !d_gathered) return PMG_E_INVALID;
    if (!e->comm) return fail(e, PMG_E_STATE, "pmg_allgather_packed_async: pmg_comm_init was not called");
    if (!e->overlap) return fail(e, PMG_E_STATE, "pmg_allgather_packed_async: pmg_comm_overlap(env, 1) first");
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    const size_t count = (size_t)e->dims.num_envs * e->dims.packed_dim;
    const int b = e->out_phase;
    if (e->cv_n == EVENT_POOL) drain_comm_events(e);
    const int i = e->cv_n;
    /* rows of this step (and of the masked resets behind it) are complete on the step's stream -> the communication stream
     * may read them; nothing else of the step's stream waits for the transfer */
    HIP_TRY(e, hipEventRecord(e->ev_rows[b], e->stream));
    HIP_TRY(e, hipStreamWaitEvent(e->comm_stream, e->ev_rows[b], 0));
    HIP_TRY(e, hipEventRecord(e->cv_a[i], e->comm_stream));
    ncclResult_t rc = ncclAllGather(e->out2[b], d_gathered, count, ncclFloat, e->comm, e->comm_stream);
    if (rc != ncclSuccess) return fail(e, PMG_E_COMM, "ncclAllGather -> %s", ncclGetErrorString(rc));
    HIP_TRY(e, hipEventRecord(e->cv_b[i], e->comm_stream));
    HIP_TRY(e, hipEventRecord(e->ev_gdone[b], e->comm_stream));
    e->cv_n = i + 1;
    e->gpending[b] = true;
    e->last_gather = b;
    return PMG_OK;
}
int pmg_allgather_wait(pmg_env* e, int32_t host)
{
    if (!e) return PMG_E_INVALID;
    if (e->last_gather < 0) return PMG_OK;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    if (host) HIP_TRY(e, hipEventSynchronize(e->ev_gdone[e->last_gather]));
    else HIP_TRY(e, hipStreamWaitEvent(e->stream, e->ev_gdone[e->last_gather], 0));
    return PMG_OK;
}

int pmg_device_alloc(pmg_env* e, uint64_t bytes, void** d_ptr)
{
    if (!e || !d_ptr) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    if (hipMalloc(d_ptr, bytes ? bytes : 1) != hipSuccess) return fail(e, PMG_E_NOMEM, "pmg_device_alloc: hipMalloc(%llu) failed", (unsigned long long)bytes);
    return PMG_OK;
}
int pmg_device_free(pmg_env* e, void* d_ptr)
{
    if (!e) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipFree(d_ptr));
    return PMG_OK;
}
int pmg_upload(pmg_env* e, void* d_dst, const void* h_src, uint64_t bytes)
{
    if (!e || !d_dst || !h_src) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return PMG_OK;
}
int pmg_device_copy(pmg_env* e, void* d_dst, const void* d_src, uint64_t bytes)
{
    if (!e || !d_dst || !d_src) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, e->stream));
    return PMG_OK;
}
int pmg_download(pmg_env* e, void* h_dst, const void* d_src, uint64_t bytes)
{
    if (!e || !h_dst || !d_src) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return PMG_OK;
}

int pmg_timing_reset(pmg_env* e)
{
    if (!e) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    e->ev_n = 0;
    e->step_count = 0;
    e->ev_ms = e->ev_min = e->ev_max = 0.0;
    e->ev_launches = 0;
    e->cv_n = 0;
    e->cv_ms = e->cv_max = 0.0;
    e->cv_launches = 0;
    return PMG_OK;
}
int pmg_timing_every(pmg_env* e, int n)
{
    if (!e || n < 1) return PMG_E_INVALID;
    e->ev_every = n;
    e->step_count = 0;
    return PMG_OK;
}
int pmg_timing_stats(pmg_env* e, double* min_ms, double* avg_ms, double* max_ms, int64_t* launches)
{
    if (!e) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    drain_events(e);
    if (min_ms) *min_ms = e->ev_min;
    if (max_ms) *max_ms = e->ev_max;
    if (avg_ms) *avg_ms = e->ev_launches ? e->ev_ms / (double)e->ev_launches : 0.0;
    if (launches) *launches = e->ev_launches;
    return PMG_OK;
}
int pmg_comm_timing(pmg_env* e, double* avg_ms, double* max_ms, int64_t* launches)
{
    if (!e) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    drain_comm_events(e);
    if (avg_ms) *avg_ms = e->cv_launches ? e->cv_ms / (double)e->cv_launches : 0.0;
    if (max_ms) *max_ms = e->cv_max;
    if (launches) *launches = e->cv_launches;
    return PMG_OK;
}
int pmg_timing_read(pmg_env* e, double* avg_ms, int64_t* launches)
{
    if (!e) return PMG_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->cfg.device));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    drain_events(e);
    if (avg_ms) *avg_ms = e->ev_launches ? e->ev_ms / (double)e->ev_launches : 0.0;
    if (launches) *launches = e->ev_launches;
    return PMG_OK;
}

}  /* extern "C" */
