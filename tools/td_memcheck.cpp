/* td_memcheck.cpp -- memory safety of pmg_q_device and pmg_td_target_device (pmg_k_mlp over MlpCatRows and pmg_k_td_target of
 * csrc/pmg_learner_body.inc) off the GPU: a stand-alone program over the g++ emulator build of the product sources (tests/emu), meant
 * to be compiled with -fsanitize=address,undefined, in the manner of tools/actor_memcheck.cpp.  "Device" memory is malloc'd there, so
 * every buffer below is sized EXACTLY -- weights, biases, the last row of a padded table without its padding, d_terminal as B bytes at
 * an odd address -- with guard bytes in front that are checked when the buffer goes; a read or write one float outside any of them
 * stops the run.  Covered: pmg_q_device for x_dim 1, 2, 31, 32, 252 x a_dim 1, 3, 4 with critics (D, 33, 1) and (D, 256, 256, 1);
 * pmg_td_target_device for Dx 1, 6, 29, 31, 33 x A 1, 3, 4 and Dx + A = 256 (A = 255: every pass of the action hand-over) with actor
 * hidden widths (33) and (256, 256, 256); batches 1, 31, 32, 33, 101, padded strides, every 4-byte phase of every float pointer, every
 * optional output given and NULL, with and without d_terminal.
 *
 * From the repository root (leak detection off: the emulator keeps its fiber stacks for the life of the process):
 *
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Ipybullet_multigoal_gym_amd/csrc \
 *       -Wno-unknown-pragmas -o td_memcheck tools/td_memcheck.cpp tests/emu/hip_emu.cpp tests/emu/pmg_probe.cpp \
 *       pybullet_multigoal_gym_amd/csrc/pmg_api.cpp -x c++ pybullet_multigoal_gym_amd/csrc/pmg_kernels.hip -lrt
 *   ASAN_OPTIONS=detect_leaks=0 ./td_memcheck
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../include/pmg.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, pmg_last_error(env)); exit(1); } } while (0)

static pmg_env* env;

/* an exactly sized "device" buffer of n bytes that starts `lead` bytes behind a 16-byte boundary (malloc aligns to 16) and ends with
 * the allocation; the `lead` bytes in front are a canary, checked when the buffer goes */
struct Buf {
    unsigned char* base = nullptr;
    unsigned char* bytes = nullptr;
    float* p = nullptr;
    size_t lead;
    Buf(size_t nbytes, size_t lead_bytes) : lead(lead_bytes)
    {
        base = (unsigned char*)malloc(lead + nbytes);
        memset(base, 0xA5, lead);
        bytes = base + lead;
        p = (float*)bytes;
        if (lead % 4 == 0) for (size_t i = 0; i < nbytes / 4; i++) p[i] = (float)((i * 7) % 13) * 0.125f - 0.75f;
        else for (size_t i = 0; i < nbytes; i++) bytes[i] = (unsigned char)(i % 3 == 0);
    }
    ~Buf()
    {
        for (size_t i = 0; i < lead; i++)
            if (base[i] != 0xA5) { fprintf(stderr, "td_memcheck: bytes in front of a buffer were written\n"); abort(); }
        free(base);
    }
};
static std::unique_ptr<Buf> floats(size_t n, int shift) { return std::unique_ptr<Buf>(new Buf(4 * n, 4 * (size_t)shift)); }

/* the network widths[0..L] in exactly sized buffers, the weights `shift` floats off a 16-byte boundary */
struct Net {
    pmg_mlp m;
    std::vector<std::unique_ptr<Buf>> bufs;
    Net(const std::vector<int>& widths, bool bias, int shift, int out_activation)
    {
        memset(&m, 0, sizeof(m));
        m.struct_size = sizeof(m); m.num_layers = (int)widths.size() - 1; m.out_activation = out_activation;
        for (size_t l = 0; l < widths.size(); l++) m.width[l] = widths[l];
        for (int l = 0; l < m.num_layers; l++) {
            bufs.push_back(floats((size_t)widths[l] * widths[l + 1], shift));
            m.d_weight[l] = bufs.back()->p;
            if (bias) { bufs.push_back(floats((size_t)widths[l + 1], shift)); m.d_bias[l] = bufs.back()->p; }
        }
    }
};

static void run_q(int x_dim, int a_dim, const std::vector<int>& hidden, long long B, int pad, int shift)
{
    std::vector<int> widths = {x_dim + a_dim};
    widths.insert(widths.end(), hidden.begin(), hidden.end());
    widths.push_back(1);
    Net net(widths, shift & 1, shift, 0);
    /* the last row of a padded table ends with its last float: no padding behind it */
    auto x = floats((size_t)(B - 1) * (x_dim + pad) + x_dim, shift), a = floats((size_t)(B - 1) * (a_dim + pad) + a_dim, (shift + 1) & 3);
    auto q = floats((size_t)(B - 1) * (1 + pad) + 1, (shift + 2) & 3);
    CHECK(pmg_q_device(env, &net.m, x->p, x_dim + pad, x_dim, a->p, a_dim + pad, a_dim, B, q->p, 1 + pad));
    CHECK(pmg_sync(env));
}

static void run_td(int Dx, int A, const std::vector<int>& hidden, long long B, int pad, int shift, int variant)
{
    std::vector<int> aw = {Dx};
    aw.insert(aw.end(), hidden.begin(), hidden.end());
    aw.push_back(A);
    Net actor(aw, shift & 1, shift, variant & 1), critic({Dx + A, 33, 1}, !(shift & 1), (shift + 1) & 3, 0);
    auto x = floats((size_t)(B - 1) * (Dx + pad) + Dx, shift), r = floats((size_t)B, (shift + 1) & 3);
    auto y = floats((size_t)B, (shift + 2) & 3), qn = floats((size_t)B, (shift + 3) & 3), na = floats((size_t)B * A, shift);
    Buf term((size_t)B, 1);                                   /* B bytes at an odd address */
    pmg_td_target td;
    memset(&td, 0, sizeof(td));
    td.struct_size = sizeof(td); td.gamma = 0.98f; td.clip_lo = variant & 2 ? -50.f : -INFINITY; td.clip_hi = variant & 2 ? 0.f : INFINITY;
    td.batch = B; td.d_x_next = x->p; td.x_stride = Dx + pad; td.d_reward = r->p; td.d_y = y->p;
    td.d_terminal = variant & 4 ? term.bytes : nullptr;
    td.d_q_next = variant & 8 ? qn->p : nullptr;
    td.d_next_action = variant & 16 ? na->p : nullptr;
    CHECK(pmg_td_target_device(env, &actor.m, &critic.m, &td));
    CHECK(pmg_sync(env));
}

int main()
{
    int nq = 0, nt = 0;
    const long long batches[5] = {1, 31, 32, 33, 101};
    const int xd[5] = {1, 2, 31, 32, 252}, ad[3] = {1, 3, 4}, dx[5] = {1, 6, 29, 31, 33};
    pmg_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg); cfg.task = PMG_TASK_REACH; cfg.num_envs = 2; cfg.binary_reward = 1;
    cfg.max_episode_steps = 50; cfg.distance_threshold = 0.05f; cfg.seed_stride = 1;
    CHECK(pmg_create(&cfg, &env));
    for (int i = 0; i < 5; i++)
        for (int j = 0; j < 3; j++) {
            run_q(xd[i], ad[j], {33}, batches[(i + j) % 5], j, (i + j) & 3); nq++;
            run_q(xd[i], ad[j], {256, 256}, batches[(i + j + 2) % 5], (j + 1) % 3, (i + 2 * j + 1) & 3); nq++;
        }
    for (int shift = 0; shift < 4; shift++)
        for (long long B : batches) { run_q(6, 3, {33}, B, shift, shift); nq++; }
    for (int i = 0; i < 5; i++)
        for (int j = 0; j < 3; j++) {
            run_td(dx[i], ad[j], {33}, batches[(i + j) % 5], j, (i + j) & 3, (i * 3 + j) * 2 + 1); nt++;
            run_td(dx[i], ad[j], {256, 256, 256}, batches[(i + j + 3) % 5], (j + 2) % 3, (i + 2 * j + 1) & 3, 31 - (i * 3 + j)); nt++;
        }
    for (int shift = 0; shift < 4; shift++)
        for (long long B : batches) { run_td(29, 4, {256}, B, shift, shift, 8 * shift + (int)(B & 7)); nt++; }
    for (int variant = 0; variant < 32; variant++) { run_td(6, 3, {33}, 33, variant % 3, variant & 3, variant); nt++; }
    run_td(1, 255, {33}, 33, 1, 1, 31); nt++;                 /* Dx + A = 256: 32 passes of the action hand-over, source and target overlap */
    run_td(255, 1, {256, 256, 256}, 101, 0, 3, 31); nt++;
    run_td(128, 128, {33}, 32, 2, 2, 30); nt++;
    pmg_destroy(env);
    printf("td_memcheck: %d calls of pmg_q_device, %d calls of pmg_td_target_device, no finding\n", nq, nt);
    return 0;
}
