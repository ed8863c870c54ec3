/* actor_memcheck.cpp -- memory safety of pmg_mlp_forward_device and pmg_act_env_device (pmg_k_mlp of csrc/pmg_learner_body.inc) off
 * the GPU: a stand-alone program over the g++ emulator build of the product sources (tests/emu), meant to be compiled with
 * -fsanitize=address,undefined.  "Device" memory is malloc'd there, so every buffer below is sized EXACTLY -- weights, biases, the
 * last input row without its padding, the last output row without its padding -- and a read or write one float outside any of
 * them stops the run.  Covered: K and widths 1, 2, 3, 31, 32, 33, 255, 256 (odd K: the padding step; widths that end inside a strip
 * and inside a wavefront's second strip), one to four layers with and without biases, batches 1, 31, 32, 33, 101, padded strides,
 * inputs and outputs off their 16-byte boundary; the act entry on reach, push and block_stack-5, both state kinds, 37 envs, with
 * and without the pre-activation output and the exploration.
 *
 * From the repository root (leak detection off: the emulator keeps its fiber stacks for the life of the process):
 *
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Ipybullet_multigoal_gym_amd/csrc \
 *       -Wno-unknown-pragmas -o actor_memcheck tools/actor_memcheck.cpp tests/emu/hip_emu.cpp tests/emu/pmg_probe.cpp \
 *       pybullet_multigoal_gym_amd/csrc/pmg_api.cpp -x c++ pybullet_multigoal_gym_amd/csrc/pmg_kernels.hip -lrt
 *   ASAN_OPTIONS=detect_leaks=0 ./actor_memcheck
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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
        for (size_t i = 0; i < n; i++) p[i] = (float)((i * 7) % 13) * 0.125f - 0.75f;
    }
    ~Buf()
    {
        for (size_t i = 0; i < lead; i++)
            if (base[i] != 0xA5) { fprintf(stderr, "actor_memcheck: bytes in front of a buffer were written\n"); abort(); }
        free(base);
    }
};

static pmg_env* make(int task, int num_block, int n)
{
    pmg_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg); cfg.task = task; cfg.num_envs = n; cfg.num_block = num_block; cfg.binary_reward = 1;
    cfg.max_episode_steps = 50; cfg.distance_threshold = 0.05f; cfg.seed_stride = 1; cfg.env_index_offset = 32;
    env = nullptr;
    CHECK(pmg_create(&cfg, &env));
    return env;
}

/* the network widths[0..L] in exactly sized buffers, the weights `shift` floats off a 16-byte boundary */
struct Net {
    pmg_mlp m;
    std::vector<std::unique_ptr<Buf>> bufs;
    Net(const std::vector<int>& widths, bool bias, int shift)
    {
        memset(&m, 0, sizeof(m));
        m.struct_size = sizeof(m); m.num_layers = (int)widths.size() - 1; m.out_activation = 1;
        for (size_t l = 0; l < widths.size(); l++) m.width[l] = widths[l];
        for (int l = 0; l < m.num_layers; l++) {
            bufs.emplace_back(new Buf((size_t)widths[l] * widths[l + 1], shift));
            m.d_weight[l] = bufs.back()->p;
            if (bias) { bufs.emplace_back(new Buf((size_t)widths[l + 1], shift)); m.d_bias[l] = bufs.back()->p; }
        }
    }
};

static void run_forward(const std::vector<int>& widths, bool bias, long long B, int pad, int shift)
{
    const int K = widths.front(), A = widths.back();
    Net net(widths, bias, shift);
    /* the last row of a padded table ends with its last float: no padding behind it */
    Buf in((size_t)(B - 1) * (K + pad) + K, shift), out((size_t)(B - 1) * (A + pad) + A, (shift + 1) & 3);
    CHECK(pmg_mlp_forward_device(env, &net.m, in.p, K + pad, B, out.p, A + pad));
    CHECK(pmg_sync(env));
}

static void run_act(int kind, bool bias, bool preact, bool explore, int shift)
{
    pmg_dims d;
    CHECK(pmg_get_dims(env, &d));
    const int Ds = kind == PMG_NORM_OBSERVATION ? d.observation_dim : d.policy_state_dim;
    Net net({Ds + d.goal_dim, 33, 65, d.action_dim}, bias, shift);
    Buf actions((size_t)d.num_envs * d.action_dim, shift), z((size_t)d.num_envs * d.action_dim, (shift + 2) & 3);
    pmg_explore ex;
    memset(&ex, 0, sizeof(ex));
    ex.struct_size = sizeof(ex); ex.noise_eps = 0.2f; ex.random_eps = 0.3f; ex.seed = 0x8000000000000005ull; ex.counter = 3;
    CHECK(pmg_act_env_device(env, &net.m, kind, explore ? &ex : nullptr, actions.p, preact ? z.p : nullptr));
    CHECK(pmg_sync(env));
}

int main()
{
    int nf = 0, na = 0;
    const int edge[8] = {1, 2, 3, 31, 32, 33, 255, 256};
    const long long batches[5] = {1, 31, 32, 33, 101};
    make(PMG_TASK_REACH, 0, 2);
    for (int ki = 0; ki < 8; ki++)
        for (int ni = 0; ni < 8; ni++) { run_forward({edge[ki], edge[ni]}, (ki + ni) & 1, batches[(ki + ni) % 5], ni % 3, ki & 3); nf++; }
    for (long long B : batches)
        for (int shift = 0; shift < 4; shift++) {
            run_forward({33, 65, 4}, shift & 1, B, shift, shift); nf++;
            run_forward({3, 256, 255, 129, 1}, !(shift & 1), B, 0, shift); nf++;
        }
    run_forward({255, 1, 2, 33}, true, 101, 5, 1); nf++;
    run_forward({256, 256, 256, 256, 256}, true, 33, 0, 0); nf++;
    pmg_destroy(env);
    const int tasks[3][2] = {{PMG_TASK_REACH, 0}, {PMG_TASK_PUSH, 0}, {PMG_TASK_BLOCK_STACK, 5}};
    for (const auto& tk : tasks) {
        make(tk[0], tk[1], 37);
        CHECK(pmg_reset(env, nullptr, nullptr, nullptr, nullptr, nullptr));
        for (int kind = 0; kind < 2; kind++)
            for (int v = 0; v < 4; v++) { run_act(kind, v & 1, v & 2, v != 1, v); na++; }
        pmg_destroy(env);
    }
    printf("actor_memcheck: %d calls of pmg_mlp_forward_device, %d calls of pmg_act_env_device, no finding\n", nf, na);
    return 0;
}
