/* policy_grad_memcheck.cpp -- memory safety of pmg_policy_grad_device (pmg_k_policy_grad_rows of csrc/pmg_learner_body.inc and the weights
 * kernel / the partials and merge kernels it launches behind it) off the GPU: a stand-alone program over the g++ emulator build of the
 * product sources (tests/emu), meant to be compiled with -fsanitize=address,undefined, in the manner of tools/grad_memcheck.cpp.  "Device"
 * memory is malloc'd there, so every buffer below is sized EXACTLY -- weights, biases, gradients, the last row of a padded table without its
 * padding, the workspace at pmg_policy_grad_work_floats -- with guard bytes in front that are checked when the buffer goes; a read or write
 * one float outside any of them stops the run.  Covered: the pairs (Dx, A) of the tests and Dx + A = 256 with A = 255 and with A = 1 (32
 * passes of the hand-over each way), the widths 1, 2, 31, 32, 33, 255, 256 as Dx, as A and as hidden width of either network, one to four
 * layers on both sides, batches 1, 31, 32, 33, 101, padded strides, every 4-byte phase of every float pointer, grads given and NULL, every
 * optional output given and NULL, both output activations of both networks, with and without biases, chunk_rows 0 and 2.
 *
 * From the repository root (leak detection off: the emulator keeps its fiber stacks for the life of the process):
 *
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Ipybullet_multigoal_gym_amd/csrc \
 *       -Wno-unknown-pragmas -o policy_grad_memcheck tools/policy_grad_memcheck.cpp tests/emu/hip_emu.cpp tests/emu/pmg_probe.cpp \
 *       pybullet_multigoal_gym_amd/csrc/pmg_api.cpp -x c++ pybullet_multigoal_gym_amd/csrc/pmg_kernels.hip -lrt
 *   ASAN_OPTIONS=detect_leaks=0 ./policy_grad_memcheck
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

/* an exactly sized "device" buffer of n floats that starts `shift` floats behind a 16-byte boundary (malloc aligns to 16) and ends with the
 * allocation; the bytes in front are a canary, checked when the buffer goes */
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
            if (base[i] != 0xA5) { fprintf(stderr, "policy_grad_memcheck: bytes in front of a buffer were written\n"); abort(); }
        free(base);
    }
};
typedef std::unique_ptr<Buf> BufP;
static BufP floats(size_t n, int shift) { return BufP(new Buf(n, shift & 3)); }

/* tensors shaped like the network widths[0..L] in exactly sized buffers, tensor k at phase shift + k */
struct Tensors {
    pmg_mlp_params p;
    std::vector<BufP> bufs;
    Tensors(const std::vector<int>& widths, bool bias, int shift)
    {
        memset(&p, 0, sizeof(p));
        for (size_t l = 0; l + 1 < widths.size(); l++) {
            bufs.push_back(floats((size_t)widths[l] * widths[l + 1], shift++));
            p.d_weight[l] = bufs.back()->p;
            if (bias) { bufs.push_back(floats((size_t)widths[l + 1], shift++)); p.d_bias[l] = bufs.back()->p; }
        }
    }
};
static pmg_mlp mlp_of(const std::vector<int>& widths, const Tensors& t, int out_activation)
{
    pmg_mlp m;
    memset(&m, 0, sizeof(m));
    m.struct_size = sizeof(m); m.num_layers = (int)widths.size() - 1; m.out_activation = out_activation;
    for (size_t l = 0; l < widths.size(); l++) m.width[l] = widths[l];
    for (int l = 0; l < m.num_layers; l++) { m.d_weight[l] = t.p.d_weight[l]; m.d_bias[l] = t.p.d_bias[l]; }
    return m;
}

static int ncalls = 0;

/* an actor Dx -> ah -> A and a critic Dx + A -> ch -> 1.  variant: bit 0 tanh actor, bit 1 tanh critic, bit 2 grads, bit 3 d_action, bit 4 d_out,
 * bit 5 d_q, bit 6 d_gaction, bit 7 biases; nothing asked for: d_q */
static void run(int Dx, int A, const std::vector<int>& ah, const std::vector<int>& ch, long long B, int pad, int shift, int variant, long long chunk_rows)
{
    std::vector<int> aw = {Dx}, cw = {Dx + A};
    aw.insert(aw.end(), ah.begin(), ah.end()); aw.push_back(A);
    cw.insert(cw.end(), ch.begin(), ch.end()); cw.push_back(1);
    const bool bias = variant & 128;
    Tensors actor(aw, bias, shift), critic(cw, bias, shift + 2), grads(aw, bias, shift + 1);
    pmg_mlp pa = mlp_of(aw, actor, variant & 1), pc = mlp_of(cw, critic, (variant >> 1) & 1);
    /* the last row of a padded table ends with its last float: no padding behind it */
    auto rows = [&](int w, int sh) { return floats((size_t)(B - 1) * (w + pad) + w, sh); };
    BufP x = rows(Dx, shift), action = rows(A, shift + 1), out = rows(A, shift + 2), q = floats((size_t)B, shift + 3), ga = rows(A, shift);
    const int64_t work = pmg_policy_grad_work_floats(&pa, &pc, B, chunk_rows);
    if (work < 0) { fprintf(stderr, "policy_grad_memcheck: pmg_policy_grad_work_floats refused a valid pair of networks\n"); exit(1); }
    BufP w = floats((size_t)work, shift + 3);
    pmg_policy_grad g;
    memset(&g, 0, sizeof(g));
    g.struct_size = sizeof(g); g.batch = B; g.gscale = -0.25f; g.l2scale = 0.0625f;
    g.d_x = x->p; g.x_stride = Dx + pad;
    bool any = false;
    if (variant & 4) { g.grads = &grads.p; any = true; }
    if (variant & 8) { g.d_action = action->p; g.action_stride = A + pad; any = true; }
    if (variant & 16) { g.d_out = out->p; g.out_stride = A + pad; any = true; }
    if (variant & 64) { g.d_gaction = ga->p; g.gaction_stride = A + pad; any = true; }
    if ((variant & 32) || !any) g.d_q = q->p;
    g.d_work = w->p; g.work_floats = work;
    CHECK(pmg_policy_grad_device(env, &pa, &pc, &g, chunk_rows));
    CHECK(pmg_sync(env));
    ncalls++;
}

int main()
{
    const long long batches[5] = {1, 31, 32, 33, 101};
    const int pairs[5][2] = {{6, 3}, {1, 1}, {2, 5}, {3, 12}, {29, 4}}, ws[7] = {1, 2, 31, 32, 33, 255, 256};
    const std::vector<int> none, small = {33}, full = {256, 256, 256};
    pmg_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg); cfg.task = PMG_TASK_REACH; cfg.num_envs = 2; cfg.binary_reward = 1;
    cfg.max_episode_steps = 50; cfg.distance_threshold = 0.05f; cfg.seed_stride = 1;
    CHECK(pmg_create(&cfg, &env));
    int n = 0;
    /* the pairs of the tests on L = 1 and L = 4 of either side, everything asked for, then the outputs alone */
    for (int i = 0; i < 5; i++)
        for (int k = 0; k < 5; k++, n++) {
            const std::vector<int>& ah = k == 0 ? none : (k == 2 || k == 4 ? full : small);
            const std::vector<int>& ch = k == 1 ? none : (k >= 3 ? full : small);
            run(pairs[i][0], pairs[i][1], ah, ch, batches[n % (k >= 2 ? 4 : 5)], n % 3, n & 3, 0x7C | (n & 3) | (n & 4 ? 128 : 0), n & 1 ? 2 : 0);
            run(pairs[i][0], pairs[i][1], ah, ch, batches[(n + 1) % (k >= 2 ? 4 : 5)], (n + 1) % 3, (n + 1) & 3, 0x78 | (n & 3) | 128, 0);
        }
    /* the widths 1, 2, 31, 32, 33, 255, 256 as Dx and as A (where Dx + A <= 256), and as hidden width of the actor and of the critic */
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++) {
            if (ws[i] + ws[j] > 256) continue;
            n++;
            run(ws[i], ws[j], small, small, batches[n % 5], n % 3, n & 3, 0xFC | (n & 3), n & 2 ? 2 : 0);
            run(ws[i], ws[j], none, none, batches[(n + 2) % 5], (n + 1) % 3, (n + 1) & 3, 0x7C | (n & 3), n & 2 ? 0 : 2);
        }
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++, n++) {
            run(6, 3, {ws[i], ws[j]}, {ws[j], ws[i]}, batches[n % 4], n % 3, n & 3, 0xFC | (n & 3), n & 1 ? 2 : 0);
            run(33, 4, {ws[j]}, {ws[(i + j) % 7], ws[i], ws[j]}, batches[(n + 1) % 4], (n + 2) % 3, (n + 2) & 3, 0x7C | (n & 3), 0);
        }
    for (int i = 0; i < 7; i++, n++) run(ws[i] < 256 ? ws[i] : 255, 1, {ws[(i + 3) % 7], ws[(i + 5) % 7], ws[(i + 1) % 7]}, {ws[(i + 2) % 7], ws[(i + 4) % 7], ws[(i + 6) % 7]}, batches[n % 4], n % 3, n & 3, 0xFC | (n & 3), n & 1 ? 2 : 0);
    /* Dx + A = 256: A = 255 (32 passes each way, source and target of both hand-overs overlap), A = 1, A = 128 */
    for (int shift = 0; shift < 4; shift++) {
        run(1, 255, small, small, batches[shift + 1], shift % 3, shift, 0xFC | shift, shift & 1 ? 2 : 0);
        run(1, 255, none, none, 33, 1, shift, 0x7C, 0);
        run(255, 1, small, full, 33, 2, shift, 0xFC, 2);
        run(128, 128, full, small, 32, 0, shift, 0xFC, 0);
    }
    /* every phase, every batch, padded strides; every set of outputs, grads given and NULL */
    for (int shift = 0; shift < 4; shift++)
        for (long long B : batches) { run(6, 3, small, small, B, shift, shift, 0xFC | shift, 0); run(29, 4, small, small, B, shift, shift, 0x78, 2); run(3, 12, small, small, B, shift, shift, 0xFC, 2); }
    for (int variant = 0; variant < 256; variant++) run(variant & 1 ? 2 : 6, variant & 1 ? 5 : 3, small, small, 33, variant % 3, variant & 3, variant, variant & 2 ? 2 : 0);
    pmg_destroy(env);
    printf("policy_grad_memcheck: %d calls of pmg_policy_grad_device, no finding\n", ncalls);
    return 0;
}
