/* sac_pg_memcheck.cpp -- memory safety of pmg_sac_policy_grad_device and pmg_sac_alpha_device (pmg_k_sac_policy_grad_rows and pmg_k_sac_alpha of
 * csrc/pmg_learner_body.inc, and the weights / partials / merge kernels they launch) off the GPU: a stand-alone program over the g++ emulator
 * build of the product sources (tests/emu), meant to be compiled with -fsanitize=address,undefined, in the manner of tools/sac_memcheck.cpp.
 * "Device" memory is malloc'd there, so every buffer below is sized EXACTLY -- weights, biases, gradient tensors, the last row of a padded
 * table without its padding, d_alpha as one float, d_state as four, the workspace as pmg_sac_policy_grad_work_floats floats -- with guard bytes
 * in front that are checked when the buffer goes; a read or write one float outside any of them stops the run.  Covered: A = 1, 2, 31, 32, 33,
 * 127, 128 (the actor's last layer 2 A wide) with a small Dx and with Dx + A = 256, and Dx < A; batches 1, 31, 32, 33, 101; padded strides; every
 * 4-byte phase of every float pointer; every combination of the optional outputs and grads; with and without critic 2 and d_alpha; chunk_rows 0
 * and 2; the temperature entry at batches 1, 255, 256, 257 and 1000.
 *
 * From the repository root (leak detection off: the emulator keeps its fiber stacks for the life of the process):
 *
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Ipybullet_multigoal_gym_amd/csrc \
 *       -Wno-unknown-pragmas -o sac_pg_memcheck tools/sac_pg_memcheck.cpp tests/emu/hip_emu.cpp tests/emu/pmg_probe.cpp \
 *       pybullet_multigoal_gym_amd/csrc/pmg_api.cpp -x c++ pybullet_multigoal_gym_amd/csrc/pmg_kernels.hip -lrt
 *   ASAN_OPTIONS=detect_leaks=0 ./sac_pg_memcheck
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
    float* p = nullptr;
    size_t lead;
    Buf(size_t nbytes, size_t lead_bytes) : lead(lead_bytes)
    {
        base = (unsigned char*)malloc(lead + nbytes);
        memset(base, 0xA5, lead);
        p = (float*)(base + lead);
        for (size_t i = 0; i < nbytes / 4; i++) p[i] = (float)((i * 7) % 13) * 0.125f - 0.75f;
    }
    ~Buf()
    {
        for (size_t i = 0; i < lead; i++)
            if (base[i] != 0xA5) { fprintf(stderr, "sac_pg_memcheck: bytes in front of a buffer were written\n"); abort(); }
        free(base);
    }
};
static std::unique_ptr<Buf> floats(size_t n, int shift) { return std::unique_ptr<Buf>(new Buf(4 * n, 4 * (size_t)shift)); }

/* the network widths[0..L] in exactly sized buffers, the weights `shift` floats off a 16-byte boundary; `grads`: tensors of the same shapes */
struct Net {
    pmg_mlp m;
    pmg_mlp_params grads;
    std::vector<std::unique_ptr<Buf>> bufs;
    Net(const std::vector<int>& widths, bool bias, int shift, int out_activation, bool with_grads = false)
    {
        memset(&m, 0, sizeof(m));
        memset(&grads, 0, sizeof(grads));
        m.struct_size = sizeof(m); m.num_layers = (int)widths.size() - 1; m.out_activation = out_activation;
        for (size_t l = 0; l < widths.size(); l++) m.width[l] = widths[l];
        for (int l = 0; l < m.num_layers; l++) {
            bufs.push_back(floats((size_t)widths[l] * widths[l + 1], shift));
            m.d_weight[l] = bufs.back()->p;
            if (bias) { bufs.push_back(floats((size_t)widths[l + 1], shift)); m.d_bias[l] = bufs.back()->p; }
            if (with_grads) {
                bufs.push_back(floats((size_t)widths[l] * widths[l + 1], (shift + 1) & 3));
                grads.d_weight[l] = bufs.back()->p;
                if (bias) { bufs.push_back(floats((size_t)widths[l + 1], (shift + 2) & 3)); grads.d_bias[l] = bufs.back()->p; }
            }
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
/* rows of `width` floats at `stride`: the last row ends with its last element */
static size_t rows(long long B, int width, int stride) { return (size_t)(B - 1) * stride + width; }

static int pg_calls = 0, alpha_calls = 0;
/* variant bits: 1 sample, 2 grads, 4 d_action, 8 d_logp, 16 d_q1, 32 d_q2, 64 d_gaction, 128 d_ghead, 256 critic 2, 512 d_alpha, 1024 chunk_rows 2,
 * 2048 a tanh critic 2 and a narrow clamp */
static void run_pg(int Dx, int A, const std::vector<int>& ah, const std::vector<int>& h1, const std::vector<int>& h2, long long B, int pad, int shift, int variant)
{
    if (!(variant & (2 + 4 + 8 + 16 + 64 + 128)) && !((variant & 32) && (variant & 256))) variant |= 8;   /* something has to be asked for */
    const bool twin = variant & 256;
    const int64_t R = variant & 1024 ? 2 : 0;
    Net actor(shape(Dx, ah, 2 * A), shift & 1, shift, 0, true), c1(shape(Dx + A, h1, 1), !(shift & 1), (shift + 1) & 3, 0),
        c2(shape(Dx + A, h2, 1), shift & 2, (shift + 2) & 3, (variant >> 11) & 1);
    const int as = A + pad, gs = A + (pad + 1) % 3, hs = 2 * A + (pad + 2) % 3;
    auto x = floats(rows(B, Dx, Dx + pad), shift), a = floats(rows(B, A, as), (shift + 1) & 3), lp = floats((size_t)B, (shift + 2) & 3);
    auto q1 = floats((size_t)B, (shift + 3) & 3), q2 = floats((size_t)B, shift), ga = floats(rows(B, A, gs), (shift + 1) & 3),
         gh = floats(rows(B, 2 * A, hs), (shift + 2) & 3), al = floats(1, (shift + 3) & 3);
    al->p[0] = 0.2f;
    pmg_sac_policy_grad g;
    memset(&g, 0, sizeof(g));
    g.struct_size = sizeof(g); g.gscale = -1.f / (float)B; g.lscale = 1.f / (float)B; g.alpha = 0.1f;
    g.ls_lo = variant & 2048 ? -1.f : -20.f; g.ls_hi = variant & 2048 ? -0.5f : 2.f;
    g.sample = variant & 1; g.seed = 3; g.counter = (uint64_t)variant; g.row_offset = variant & 8 ? ((int64_t)1 << 40) + 5 : 0;
    g.batch = B; g.d_x = x->p; g.x_stride = Dx + pad;
    g.d_alpha = variant & 512 ? al->p : nullptr;
    g.grads = variant & 2 ? &actor.grads : nullptr;
    if (variant & 4) { g.d_action = a->p; g.action_stride = as; }
    if (variant & 8) g.d_logp = lp->p;
    if (variant & 16) g.d_q1 = q1->p;
    if (variant & 32) g.d_q2 = q2->p;
    if (variant & 64) { g.d_gaction = ga->p; g.gaction_stride = gs; }
    if (variant & 128) { g.d_ghead = gh->p; g.ghead_stride = hs; }
    const int64_t need = pmg_sac_policy_grad_work_floats(&actor.m, g.d_action != nullptr, twin, B, g.grads ? R : 0);
    const int64_t base = g.grads && R ? pmg_mlp_grad_chunked_work_floats(&actor.m, B, R) : pmg_mlp_grad_work_floats(&actor.m, B);
    if (need != base + (g.d_action ? 0 : B * A) + (twin ? B * A : 0)) { fprintf(stderr, "sac_pg_memcheck: workspace figure %lld\n", (long long)need); exit(1); }
    auto work = floats((size_t)need, (shift + 3) & 3);
    g.d_work = work->p; g.work_floats = need;
    CHECK(pmg_sac_policy_grad_device(env, &actor.m, &c1.m, twin ? &c2.m : nullptr, &g, R));
    CHECK(pmg_sync(env));
    pg_calls++;
}
static void run_alpha(long long B, int shift, int steps)
{
    auto lp = floats((size_t)B, shift), st = floats(4, (shift + 1) & 3);
    st->p[0] = logf(0.2f); st->p[1] = 0.f; st->p[2] = 0.f; st->p[3] = 0.2f;
    for (int k = 0; k < steps; k++) {
        pmg_sac_alpha a;
        memset(&a, 0, sizeof(a));
        a.struct_size = sizeof(a); a.target_entropy = -3.f; a.lr = 3e-4f; a.beta1 = 0.9f; a.beta2 = 0.999f; a.eps = 1e-8f; a.step = 1 + k;
        a.batch = B; a.d_logp = lp->p; a.d_state = st->p;
        CHECK(pmg_sac_alpha_device(env, &a));
        CHECK(pmg_sync(env));
        alpha_calls++;
    }
    if (!(st->p[3] > 0.f) || !std::isfinite(st->p[0])) { fprintf(stderr, "sac_pg_memcheck: alpha %g\n", (double)st->p[3]); exit(1); }
}

int main()
{
    const long long batches[5] = {1, 31, 32, 33, 101};
    const int as[7] = {1, 2, 31, 32, 33, 127, 128};
    const int hidden[7] = {1, 2, 31, 33, 255, 256, 32};
    pmg_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg); cfg.task = PMG_TASK_REACH; cfg.num_envs = 8; cfg.binary_reward = 1;
    cfg.max_episode_steps = 50; cfg.distance_threshold = 0.05f; cfg.seed_stride = 1;
    CHECK(pmg_create(&cfg, &env));
    const int all = 1 + 2 + 4 + 8 + 16 + 32 + 64 + 128;
    /* every A with a small Dx, with Dx + A = 256 and with Dx < A, every hidden width in turn; a in d_action and in the workspace; chunk_rows 0 and 2 */
    int n = 0;
    for (int k = 0; k < 7; k++) {
        const int A = as[k], w = hidden[k];
        for (int v = 0; v < 2; v++, n++) {
            const int full = (all ^ (v ? 4 : 0)) + 256 + (v ? 512 : 0);
            run_pg(3, A, {w}, {w, 33}, {33, w}, batches[n % 5], n % 3, n & 3, full + (v ? 1024 : 0));
            run_pg(256 - A, A, {33}, {w}, {w, w, w}, batches[(n + 3) % 5], (n + 1) % 3, (n + 1) & 3, (full ^ 1) + (v ? 0 : 1024));
            run_pg(1, A, {w, w, w}, {}, {w}, batches[(n + 4) % 5], (n + 2) % 3, (n + 2) & 3, (full ^ 256) + 2048);
        }
    }
    /* Dx + A = 256 with the hazard shape A = 20 beside it, and the widest head behind three wide layers */
    for (int v = 0; v < 4; v++) {
        run_pg(236, 20, {256}, {256}, {33, 256}, 33, 1, v, (all ^ (v & 1 ? 4 : 0)) + 256 + (v & 2 ? 512 : 0));
        run_pg(128, 128, {256, 256, 256}, {256, 256, 256}, {256, 256, 256}, 101, 0, 3 - v, (all ^ (v & 2 ? 4 : 0)) + (v & 1 ? 256 : 0) + (v & 2 ? 1024 : 0));
        run_pg(1, 20, {33}, {33}, {33}, 32, 2, v, (all ^ (v & 2 ? 4 : 0)) + (v & 1 ? 256 : 0) + 1024);
        run_pg(255, 1, {33}, {33}, {33}, 33, v % 3, v, all + 256 - 4 * (v & 1));
    }
    /* every 4-byte phase x every batch, the odd Dx + A = 33 */
    for (int shift = 0; shift < 4; shift++)
        for (long long B : batches) run_pg(29, 4, {256}, {256, 33}, {33}, B, shift, shift, (all ^ (B & 1 ? 4 : 0)) + 256 + (shift & 1 ? 1024 : 0) + (shift & 2 ? 512 : 0));
    /* every combination of grads, the optional outputs, critic 2, d_alpha, chunk_rows and sampling: all 4096 variants */
    for (int variant = 0; variant < 4096; variant++) run_pg(variant & 1 ? 6 : 2, variant & 1 ? 3 : 5, {33}, {33}, {17, 9}, variant % 5 == 0 ? 33 : 5, variant % 3, variant & 3, variant);
    /* the temperature */
    const long long ab[5] = {1, 255, 256, 257, 1000};
    for (int k = 0; k < 5; k++)
        for (int shift = 0; shift < 4; shift++) run_alpha(ab[k], shift, 3);
    pmg_destroy(env);
    printf("sac_pg_memcheck: %d calls of pmg_sac_policy_grad_device, %d of pmg_sac_alpha_device, no finding\n", pg_calls, alpha_calls);
    return 0;
}
