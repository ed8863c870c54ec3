/* her_memcheck.cpp -- memory safety of pmg_her_sample_device and pmg_policy_input_device (the two entries of the flat sweep of
 * csrc/pmg_learner_body.inc) off the GPU: a stand-alone program over the g++ emulator build of the product sources
 * (tests/emu), meant to be compiled with -fsanitize=address,undefined.  "Device" memory is malloc'd
 * there, so every buffer below is sized EXACTLY and a read or write one float outside any of them stops the run.
 * Covered: time- and episode-major tables, padded strides, inputs and outputs off their 16-byte boundary, x and x_next on
 * different boundaries, NULL outputs, E = T = 1, batches on both sides of a workgroup and of the striding grid; policy-input
 * rows of push (7 | 3) and block_stack-5 (88 | 15) at B = 1, 255, 256, 257, every out-shift 0..3 and input shifts 0..3.
 *
 * From the repository root (leak detection off: the emulator keeps its fiber stacks for the life of the process):
 *
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Ipybullet_multigoal_gym_amd/csrc \
 *       -Wno-unknown-pragmas -o her_memcheck tools/her_memcheck.cpp tests/emu/hip_emu.cpp tests/emu/pmg_probe.cpp \
 *       pybullet_multigoal_gym_amd/csrc/pmg_api.cpp -x c++ pybullet_multigoal_gym_amd/csrc/pmg_kernels.hip -lrt
 *   ASAN_OPTIONS=detect_leaks=0 ./her_memcheck
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/pmg.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, pmg_last_error(env)); exit(1); } } while (0)

static pmg_env* env;

/* an exactly sized "device" buffer of n floats that starts `shift` floats behind a 16-byte boundary (malloc aligns to 16) and
 * ends with the allocation; the `shift` floats in front are a canary, checked when the buffer goes */
struct Buf {
    unsigned char* base = nullptr;
    float* p = nullptr;
    size_t lead;
    Buf(size_t n, int shift) : lead(4 * (size_t)shift)
    {
        base = (unsigned char*)malloc(lead + 4 * n);
        memset(base, 0xA5, lead);
        p = (float*)(base + lead);
    }
    ~Buf()
    {
        for (size_t i = 0; i < lead; i++)
            if (base[i] != 0xA5) { fprintf(stderr, "her_memcheck: bytes in front of a buffer were written\n"); abort(); }
        free(base);
    }
};

static void run(int task, int num_block, int E, int T, bool time_major, bool pad, int in_shift, int sx, int sxn, long long B, int kind, int raw, unsigned null_mask)
{
    pmg_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg); cfg.task = task; cfg.num_envs = 2; cfg.num_block = num_block; cfg.binary_reward = 1;
    cfg.max_episode_steps = 50; cfg.distance_threshold = 0.05f; cfg.seed_stride = 1;
    env = nullptr;
    CHECK(pmg_create(&cfg, &env));
    pmg_dims d;
    CHECK(pmg_get_dims(env, &d));
    const int P = d.packed_dim, A = d.action_dim, Pp = pad ? P + 5 : P, Ap = pad ? A + 3 : A;
    const int Ds = kind == PMG_NORM_OBSERVATION ? d.observation_dim : d.policy_state_dim, W = Ds + d.goal_dim;
    /* the last row of a padded table ends with its last float: no padding behind it */
    const size_t nrows = (size_t)E * (T + 1), nact = (size_t)E * T;
    Buf rows((nrows - 1) * Pp + P, in_shift), acts((nact - 1) * Ap + A, in_shift);
    for (size_t i = 0; i < (nrows - 1) * Pp + P; i++) rows.p[i] = (float)(i % 1000) * 0.001f;
    for (size_t i = 0; i < (nact - 1) * Ap + A; i++) acts.p[i] = (float)(i % 7);
    Buf x((size_t)B * W, sx), xn((size_t)B * W, sxn), act((size_t)B * A, sx), rew((size_t)B, sxn), idx((size_t)B * 3, sx);
    std::vector<uint8_t> ok((size_t)B);
    pmg_her_source src;
    memset(&src, 0, sizeof(src));
    src.struct_size = sizeof(src); src.num_episodes = E; src.episode_steps = T;
    src.d_rows = rows.p; src.d_actions = acts.p;
    src.row_episode_stride = time_major ? Pp : (long long)(T + 1) * Pp; src.row_time_stride = time_major ? (long long)E * Pp : Pp;
    src.action_episode_stride = time_major ? Ap : (long long)T * Ap; src.action_time_stride = time_major ? (long long)E * Ap : Ap;
    pmg_her_batch out;
    memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(out); out.state_kind = kind; out.raw = raw; out.future_p = 0.8f; out.seed = 0x8000000000000005ull; out.counter = 3; out.batch = B;
    out.d_x = (null_mask & 1) ? nullptr : x.p; out.d_x_next = (null_mask & 2) ? nullptr : xn.p; out.d_action = (null_mask & 4) ? nullptr : act.p;
    out.d_reward = (null_mask & 8) ? nullptr : rew.p; out.d_goal_achieved = (null_mask & 16) ? nullptr : ok.data();
    out.d_index = (null_mask & 32) ? nullptr : (int32_t*)idx.p;
    CHECK(pmg_her_sample_device(env, &src, &out));
    CHECK(pmg_sync(env));
    pmg_destroy(env);
}

/* pmg_policy_input_device on contiguous state [B, Ds] and goal [B, Dg] rows, inputs `in_shift` and the output `out_shift` floats
 * behind a 16-byte boundary */
static void run_policy_input(int task, int num_block, int kind, long long B, int in_shift, int out_shift)
{
    pmg_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg); cfg.task = task; cfg.num_envs = 2; cfg.num_block = num_block; cfg.binary_reward = 1;
    cfg.max_episode_steps = 50; cfg.distance_threshold = 0.05f; cfg.seed_stride = 1;
    env = nullptr;
    CHECK(pmg_create(&cfg, &env));
    pmg_dims d;
    CHECK(pmg_get_dims(env, &d));
    const int Ds = kind == PMG_NORM_OBSERVATION ? d.observation_dim : d.policy_state_dim, Dg = d.goal_dim;
    Buf state((size_t)B * Ds, in_shift), goal((size_t)B * Dg, in_shift), out((size_t)B * (Ds + Dg), out_shift);
    for (size_t i = 0; i < (size_t)B * Ds; i++) state.p[i] = (float)(i % 1000) * 0.001f;
    for (size_t i = 0; i < (size_t)B * Dg; i++) goal.p[i] = (float)(i % 7);
    CHECK(pmg_policy_input_device(env, kind, state.p, Ds, goal.p, Dg, B, out.p));
    CHECK(pmg_sync(env));
    pmg_destroy(env);
}

int main()
{
    int n = 0, np = 0;
    const int tasks[3][2] = {{PMG_TASK_REACH, 0}, {PMG_TASK_PUSH, 0}, {PMG_TASK_BLOCK_STACK, 5}};
    for (const auto& tk : tasks)
        for (int layout = 0; layout < 4; layout++)
            for (int kind = 0; kind < 2; kind++) {
                const bool tm = layout & 1, pad = layout & 2;
                run(tk[0], tk[1], 5, 7, tm, pad, 1, 1, 1, 257, kind, kind, 0); n++;
                run(tk[0], tk[1], 5, 7, tm, pad, 0, 2, 3, 255, kind, !kind, 0); n++;         /* x and x_next on different boundaries */
                run(tk[0], tk[1], 1, 1, tm, pad, 3, 3, 3, 65, kind, 0, 0); n++;               /* E = T = 1 */
                run(tk[0], tk[1], 3, 2, tm, pad, 1, 0, 0, 1, kind, 0, 32); n++;               /* one sample, indices in scratch */
                for (unsigned m = 1; m < 64; m <<= 1) { run(tk[0], tk[1], 2, 3, tm, pad, 0, 1, 1, 64, kind, 1, m); n++; }
            }
    /* from 4 * 2048 * 256 / W rows the grid strides: W = 103 */
    run(PMG_TASK_BLOCK_STACK, 5, 7, 5, true, true, 1, 1, 1, 4 * 2048 * 256 / 103 + 1, PMG_NORM_OBSERVATION, 0, 0); n++;
    run(PMG_TASK_BLOCK_STACK, 5, 7, 5, false, false, 1, 3, 2, 4 * 2048 * 256 / 103 + 1, PMG_NORM_OBSERVATION, 1, 0); n++;
    const int ptasks[2][3] = {{PMG_TASK_PUSH, 0, PMG_NORM_POLICY_STATE}, {PMG_TASK_BLOCK_STACK, 5, PMG_NORM_OBSERVATION}};   /* 7 | 3 and 88 | 15 */
    for (const auto& tk : ptasks)
        for (long long B : {1, 255, 256, 257})
            for (int out_shift = 0; out_shift < 4; out_shift++)
                for (int in_shift = 0; in_shift < 4; in_shift++) { run_policy_input(tk[0], tk[1], tk[2], B, in_shift, out_shift); np++; }
    printf("her_memcheck: %d calls of pmg_her_sample_device, %d calls of pmg_policy_input_device, no finding\n", n, np);
    return 0;
}
