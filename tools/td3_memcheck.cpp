/* td3_memcheck.cpp -- memory safety of pmg_td3_target_device (pmg_k_td3_target of csrc/pmg_learner_body.inc) off the GPU: a stand-alone
 * program over the g++ emulator build of the product sources (tests/emu), meant to be compiled with -fsanitize=address,undefined, in the
 * manner of tools/td_memcheck.cpp.  "Device" memory is malloc'd there, so every buffer below is sized EXACTLY -- weights, biases, the last
 * row of a padded table without its padding, d_terminal as B bytes at an odd address, the workspace as pmg_td3_target_work_floats floats
 * (and absent where that is 0) -- with guard bytes in front that are checked when the buffer goes; a read or write one float outside any of
 * them stops the run.  Covered: the widths 1, 2, 31, 32, 33, 255, 256 as Dx, as A and as hidden widths of the actor and of either critic;
 * Dx + A = 256 with A = 255 (every pass of the hand-over and of the restore) and with A = 1; batches 1, 31, 32, 33, 101; padded strides;
 * every 4-byte phase of every float pointer; every optional output given and NULL (d_next_action NULL: the workspace path); with and
 * without critic 2, d_terminal and noise.
 *
 * From the repository root (leak detection off: the emulator keeps its fiber stacks for the life of the process):
 *
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Ipybullet_multigoal_gym_amd/csrc \
 *       -Wno-unknown-pragmas -o td3_memcheck tools/td3_memcheck.cpp tests/emu/hip_emu.cpp tests/emu/pmg_probe.cpp \
 *       pybullet_multigoal_gym_amd/csrc/pmg_api.cpp -x c++ pybullet_multigoal_gym_amd/csrc/pmg_kernels.hip -lrt
 *   ASAN_OPTIONS=detect_leaks=0 ./td3_memcheck
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
            if (base[i] != 0xA5) { fprintf(stderr, "td3_memcheck: bytes in front of a buffer were written\n"); abort(); }
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
static std::vector<int> shape(int in, const std::vector<int>& hidden, int out)
{
    std::vector<int> w = {in};
    w.insert(w.end(), hidden.begin(), hidden.end());
    w.push_back(out);
    return w;
}

/* variant bits: 1 tanh actor, 2 clips, 4 d_terminal, 8 d_q_min, 16 d_next_action, 32 d_q1, 64 d_q2, 128 critic 2, 256 noise */
static int calls = 0;
static void run(int Dx, int A, const std::vector<int>& ah, const std::vector<int>& h1, const std::vector<int>& h2, long long B, int pad, int shift, int variant)
{
    const bool twin = variant & 128;
    Net actor(shape(Dx, ah, A), shift & 1, shift, variant & 1), c1(shape(Dx + A, h1, 1), !(shift & 1), (shift + 1) & 3, 0),
        c2(shape(Dx + A, h2, 1), shift & 2, (shift + 2) & 3, (variant >> 1) & 1);
    auto x = floats((size_t)(B - 1) * (Dx + pad) + Dx, shift), r = floats((size_t)B, (shift + 1) & 3);
    auto y = floats((size_t)B, (shift + 2) & 3), qm = floats((size_t)B, (shift + 3) & 3), q1 = floats((size_t)B, shift), q2 = floats((size_t)B, (shift + 1) & 3);
    auto na = floats((size_t)B * A, (shift + 2) & 3);
    Buf term((size_t)B, 1);                                   /* B bytes at an odd address */
    pmg_td3_target td;
    memset(&td, 0, sizeof(td));
    td.struct_size = sizeof(td); td.gamma = 0.98f; td.clip_lo = variant & 2 ? -50.f : -INFINITY; td.clip_hi = variant & 2 ? 0.f : INFINITY;
    td.sigma = variant & 256 ? 0.2f : 0.f; td.noise_clip = variant & 2 ? 0.5f : INFINITY; td.seed = 3; td.counter = (uint64_t)variant;
    td.row_offset = variant & 4 ? ((int64_t)1 << 40) + 5 : 0;
    td.batch = B; td.d_x_next = x->p; td.x_stride = Dx + pad; td.d_reward = r->p; td.d_y = y->p;
    td.d_terminal = variant & 4 ? term.bytes : nullptr;
    td.d_q_min = variant & 8 ? qm->p : nullptr;
    td.d_next_action = variant & 16 ? na->p : nullptr;
    td.d_q1 = variant & 32 ? q1->p : nullptr;
    td.d_q2 = variant & 64 ? q2->p : nullptr;
    const int64_t need = pmg_td3_target_work_floats(&actor.m, twin, td.d_next_action != nullptr, B);
    if (need != (twin && !td.d_next_action ? B * A : 0)) { fprintf(stderr, "td3_memcheck: workspace figure %lld\n", (long long)need); exit(1); }
    std::unique_ptr<Buf> work;
    if (need > 0) { work = floats((size_t)need, (shift + 3) & 3); td.d_work = work->p; td.work_floats = need; }
    CHECK(pmg_td3_target_device(env, &actor.m, &c1.m, twin ? &c2.m : nullptr, &td));
    CHECK(pmg_sync(env));
    calls++;
}

int main()
{
    const long long batches[5] = {1, 31, 32, 33, 101};
    const int widths[7] = {1, 2, 31, 32, 33, 255, 256};
    pmg_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg); cfg.task = PMG_TASK_REACH; cfg.num_envs = 2; cfg.binary_reward = 1;
    cfg.max_episode_steps = 50; cfg.distance_threshold = 0.05f; cfg.seed_stride = 1;
    CHECK(pmg_create(&cfg, &env));
    /* every width as Dx (A = 3, or 1 where Dx + 3 > 256), as A (Dx = 1, or 6 where it fits) and as a hidden width of each network */
    int n = 0;
    for (int w : widths) {
        for (int v = 0; v < 2; v++, n++) {
            const int full = 128 + 256 + (v ? 8 + 32 + 64 + 4 + 2 : 16 + 1);      /* twin + noise; v: workspace path / d_next_action */
            if (w < 256) {                                    /* Dx + A <= 256: 256 is a hidden width only */
                run(w, w + 3 <= 256 ? 3 : 1, {33}, {33}, {33}, batches[n % 5], n % 3, n & 3, full);
                run(w + 6 <= 256 ? 6 : 1, w, {33}, {33}, {33}, batches[(n + 1) % 5], (n + 1) % 3, (n + 1) & 3, full);
            }
            run(6, 3, {w}, {w, 33}, {33, w}, batches[(n + 2) % 5], (n + 2) % 3, (n + 2) & 3, full);
            run(6, 3, {w, w, w}, {w, w, w}, {w}, batches[(n + 3) % 5], n % 3, (n + 3) & 3, full ^ 256);
        }
    }
    /* Dx + A = 256: A = 255 (32 passes of the hand-over and of the restore, source and target overlap) and A = 1 */
    for (int v = 0; v < 4; v++) {
        run(1, 255, {33}, {256}, {33, 256}, 33, 1, v, 128 + (v & 1 ? 256 : 0) + (v & 2 ? 16 : 0) + 8 + 32 + 64);
        run(255, 1, {256, 256, 256}, {256, 256, 256}, {256, 256, 256}, 101, 0, 3 - v, 128 + (v & 1 ? 0 : 256) + (v & 2 ? 16 : 0) + 4 + 2);
        run(128, 128, {33}, {33}, {33}, 32, 2, v, (v & 1 ? 128 : 0) + 256 + (v & 2 ? 0 : 16) + 8);
    }
    /* every 4-byte phase x every batch, the odd Dx + A = 33 */
    for (int shift = 0; shift < 4; shift++)
        for (long long B : batches) run(29, 4, {256}, {256, 33}, {33}, B, shift, shift, 128 + 256 + 8 * shift + (int)(B & 7) + (B & 1 ? 0 : 16) + 64);
    /* every optional output given and NULL, with and without critic 2, d_terminal, clips and noise: all 512 variants */
    for (int variant = 0; variant < 512; variant++) run(6, 3, {33}, {33}, {17, 9}, variant % 5 == 0 ? 33 : 5, variant % 3, variant & 3, variant);
    pmg_destroy(env);
    printf("td3_memcheck: %d calls of pmg_td3_target_device, no finding\n", calls);
    return 0;
}
