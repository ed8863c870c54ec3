/* policy_grad_bc_memcheck.cpp -- memory safety of pmg_policy_grad_bc_device (pmg_k_policy_grad_bc_rows of csrc/pmg_learner_body.inc and the
 * weights kernel / the partials and merge kernels it launches behind it) off the GPU: a stand-alone program over the g++ emulator build of the
 * product sources (tests/emu), meant to be compiled with -fsanitize=address,undefined, in the manner of tools/policy_grad_memcheck.cpp.
 * "Device" memory is malloc'd there, so every buffer below is sized EXACTLY -- weights, biases, gradients, the last row of a padded table
 * without its padding, the workspace at pmg_policy_grad_work_floats, d_q_demo at B floats, d_filter at B bytes at an odd address -- with
 * guard bytes in front that are checked when the buffer goes; a read or write one element outside any of them stops the run.  The
 * demonstration table is allocated from row demo_begin on only: d_demo_action points demo_begin rows in front of the allocation, so a read
 * of a row below demo_begin is a read outside it.  Covered: demo_begin at 0, inside a tile, on a tile edge and at B (there with a NULL
 * table); the pairs (Dx, A) of the tests and Dx + A = 256 with A = 255 and with A = 1; the widths 1, 2, 31, 32, 33, 255, 256 as hidden width of
 * either network; batches 1, 31, 32, 33, 101; padded strides; every 4-byte phase of every float pointer; grads given and NULL; every optional
 * output given and NULL; q_filter 0 and 1; both output activations; with and without biases; chunk_rows 0 and 2.
 *
 * From the repository root (leak detection off: the emulator keeps its fiber stacks for the life of the process):
 *
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Ipybullet_multigoal_gym_amd/csrc \
 *       -Wno-unknown-pragmas -o policy_grad_bc_memcheck tools/policy_grad_bc_memcheck.cpp tests/emu/hip_emu.cpp tests/emu/pmg_probe.cpp \
 *       pybullet_multigoal_gym_amd/csrc/pmg_api.cpp -x c++ pybullet_multigoal_gym_amd/csrc/pmg_kernels.hip -lrt
 *   ASAN_OPTIONS=detect_leaks=0 ./policy_grad_bc_memcheck
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../include/pmg.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, pmg_last_error(env)); exit(1); } } while (0)

static pmg_env* env;

/* an exactly sized "device" buffer of n bytes that starts `lead` bytes behind a 16-byte boundary (malloc aligns to 16) and ends with the
 * allocation; the bytes in front are a canary, checked when the buffer goes */
struct Buf {
    unsigned char* base = nullptr;
    float* p = nullptr;
    unsigned char* bytes = nullptr;
    size_t lead;
    Buf(size_t nbytes, size_t lead_) : lead(lead_)
    {
        base = (unsigned char*)malloc(lead + nbytes);
        memset(base, 0xA5, lead);
        bytes = base + lead;
        p = (float*)bytes;
        if ((lead & 3) == 0)
            for (size_t i = 0; i < nbytes / 4; i++) p[i] = (float)((i * 7) % 13) * 0.125f - 0.75f;
    }
    ~Buf()
    {
        for (size_t i = 0; i < lead; i++)
            if (base[i] != 0xA5) { fprintf(stderr, "policy_grad_bc_memcheck: bytes in front of a buffer were written\n"); abort(); }
        free(base);
    }
};
typedef std::unique_ptr<Buf> BufP;
static BufP floats(size_t n, int shift) { return BufP(new Buf(4 * n, 4 * (size_t)(shift & 3))); }

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

/* an actor Dx -> ah -> A and a critic Dx + A -> ch -> 1, rows from `begin` on demonstrations.  variant: bit 0 tanh actor, bit 1 tanh critic,
 * bit 2 grads, bit 3 d_action, bit 4 d_out, bit 5 d_q, bit 6 d_gaction, bit 7 biases, bit 8 d_q_demo, bit 9 d_filter, bit 10 q_filter; nothing
 * asked for: d_filter */
static void run(int Dx, int A, const std::vector<int>& ah, const std::vector<int>& ch, long long B, long long begin, int pad, int shift, int variant,
                long long chunk_rows)
{
    std::vector<int> aw = {Dx}, cw = {Dx + A};
    aw.insert(aw.end(), ah.begin(), ah.end()); aw.push_back(A);
    cw.insert(cw.end(), ch.begin(), ch.end()); cw.push_back(1);
    const bool bias = variant & 128;
    Tensors actor(aw, bias, shift), critic(cw, bias, shift + 2), grads(aw, bias, shift + 1);
    pmg_mlp pa = mlp_of(aw, actor, variant & 1), pc = mlp_of(cw, critic, (variant >> 1) & 1);
    /* the last row of a padded table ends with its last float: no padding behind it */
    auto rows = [&](long long n, int w, int sh) { return floats((size_t)(n - 1) * (w + pad) + w, sh); };
    BufP x = rows(B, Dx, shift), action = rows(B, A, shift + 1), out = rows(B, A, shift + 2), q = floats((size_t)B, shift + 3), ga = rows(B, A, shift);
    BufP qd = floats((size_t)B, shift + 1);
    BufP filter(new Buf((size_t)B, 1 + 2 * (size_t)(shift & 1)));        /* an odd address */
    BufP demo = begin < B ? rows(B - begin, A, shift + 3) : BufP();       /* rows [begin, B) only */
    const int64_t work = pmg_policy_grad_work_floats(&pa, &pc, B, chunk_rows);
    if (work < 0) { fprintf(stderr, "policy_grad_bc_memcheck: pmg_policy_grad_work_floats refused a valid pair of networks\n"); exit(1); }
    BufP w = floats((size_t)work, shift + 3);
    pmg_policy_grad g;
    memset(&g, 0, sizeof(g));
    g.struct_size = sizeof(g); g.batch = B; g.gscale = -0.25f; g.l2scale = 0.0625f;
    g.d_x = x->p; g.x_stride = Dx + pad;
    pmg_policy_bc bc;
    memset(&bc, 0, sizeof(bc));
    bc.struct_size = sizeof(bc); bc.q_filter = (variant >> 10) & 1; bc.bcscale = 0.015625f; bc.demo_begin = begin;
    if (demo) {          /* formed as an integer: the table's first `begin` rows do not exist */
        bc.d_demo_action = (const float*)((uintptr_t)demo->p - (uintptr_t)(4 * begin * (A + pad)));
        bc.demo_action_stride = A + pad;
    }
    bool any = false;
    if (variant & 4) { g.grads = &grads.p; any = true; }
    if (variant & 8) { g.d_action = action->p; g.action_stride = A + pad; any = true; }
    if (variant & 16) { g.d_out = out->p; g.out_stride = A + pad; any = true; }
    if (variant & 32) { g.d_q = q->p; any = true; }
    if (variant & 64) { g.d_gaction = ga->p; g.gaction_stride = A + pad; any = true; }
    if (variant & 256) { bc.d_q_demo = qd->p; any = true; }
    if ((variant & 512) || !any) bc.d_filter = filter->bytes;
    g.d_work = w->p; g.work_floats = work;
    CHECK(pmg_policy_grad_bc_device(env, &pa, &pc, &g, &bc, chunk_rows));
    CHECK(pmg_sync(env));
    if (bc.d_filter)
        for (long long b = 0; b < B; b++)
            if (filter->bytes[b] > 1 || (b < begin && filter->bytes[b])) { fprintf(stderr, "policy_grad_bc_memcheck: d_filter[%lld] = %d\n", b, filter->bytes[b]); exit(1); }
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
    /* demo_begin at 0, inside a tile, on a tile edge, at B - 1 and at B (as far as the batch has them) */
    auto begins = [](long long B) {
        std::vector<long long> v = {0, B};
        for (long long b : {1LL, 13LL, 32LL, 33LL, 64LL, B - 1}) if (b > 0 && b < B) v.push_back(b);
        return v;
    };
    int n = 0;
    /* the pairs of the tests on L = 1 and L = 4 of either side, everything asked for, every batch and every demo_begin */
    for (int i = 0; i < 5; i++)
        for (int k = 0; k < 5; k++) {
            const std::vector<int>& ah = k == 0 ? none : (k == 2 || k == 4 ? full : small);
            const std::vector<int>& ch = k == 1 ? none : (k >= 3 ? full : small);
            const long long B = batches[(i + k) % (k >= 2 ? 4 : 5)];
            for (long long b0 : begins(B)) {
                run(pairs[i][0], pairs[i][1], ah, ch, B, b0, n % 3, n & 3, 0x37C | (n & 3) | (n & 4 ? 128 : 0) | (n & 8 ? 1024 : 0), n & 1 ? 2 : 0);
                n++;
            }
        }
    /* the widths 1, 2, 31, 32, 33, 255, 256 as hidden width of the actor and of the critic */
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++, n++) {
            const long long B = batches[n % 4];
            run(6, 3, {ws[i], ws[j]}, {ws[j], ws[i]}, B, B / 2, n % 3, n & 3, 0x3FC | (n & 3) | (n & 4 ? 1024 : 0), n & 1 ? 2 : 0);
        }
    /* Dx + A = 256: A = 255 (the demonstration pass gathers 255 action columns per row), A = 1, A = 128 */
    for (int shift = 0; shift < 4; shift++)
        for (long long b0 : begins(33)) {
            run(1, 255, small, small, 33, b0, shift % 3, shift, 0x7FC | shift, shift & 1 ? 2 : 0);
            run(1, 255, none, none, 33, b0, 1, shift, 0x37C, 0);
            run(255, 1, small, full, 33, b0, 2, shift, 0x7FC, 2);
            run(255, 1, none, none, 33, b0, 0, shift, 0x3FC, 0);
        }
    for (int shift = 0; shift < 4; shift++) run(128, 128, full, small, 32, 16, 0, shift, 0x7FC, 0);
    /* every phase, every batch, every demo_begin, padded strides */
    for (int shift = 0; shift < 4; shift++)
        for (long long B : batches)
            for (long long b0 : begins(B)) {
                run(6, 3, small, small, B, b0, shift, shift, 0x7FC | shift, 0);
                run(29, 4, small, small, B, b0, shift, shift, 0x378, 2);
                run(3, 12, small, small, B, b0, shift, shift, 0x3FC, 2);
            }
    /* every set of outputs, grads given and NULL, both filters */
    for (int variant = 0; variant < 2048; variant++)
        run(variant & 1 ? 2 : 6, variant & 1 ? 5 : 3, small, small, 33, variant % 5 == 0 ? 33 : (variant % 7) * 5, variant % 3, variant & 3, variant, variant & 2 ? 2 : 0);
    pmg_destroy(env);
    printf("policy_grad_bc_memcheck: %d calls of pmg_policy_grad_bc_device, no finding\n", ncalls);
    return 0;
}
