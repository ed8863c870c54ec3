/* sac_memcheck.cpp -- memory safety of pmg_sac_sample_device, pmg_sac_act_env_device and pmg_sac_target_device (pmg_k_sac and pmg_k_sac_target of
 * csrc/pmg_learner_body.inc) off the GPU: a stand-alone program over the g++ emulator build of the product sources (tests/emu), meant to be
 * compiled with -fsanitize=address,undefined, in the manner of tools/td3_memcheck.cpp.  "Device" memory is malloc'd there, so every buffer
 * below is sized EXACTLY -- weights, biases, the last row of a padded table without its padding, d_terminal as B bytes at an odd address,
 * d_alpha as one float, the workspace as pmg_sac_target_work_floats floats (and absent where that is 0) -- with guard bytes in front that are
 * checked when the buffer goes; a read or write one float outside any of them stops the run.  Covered: A = 1, 2, 31, 32, 33, 127, 128 (the
 * actor's last layer 2 A wide) with small and large Dx and every hidden width; Dx + A = 256 with A = 128, A = 1 and A = 20; Dx < A; batches 1,
 * 31, 32, 33, 101; padded strides; every 4-byte phase of every float pointer; every combination of the optional outputs of either entry;
 * with and without critic 2, d_terminal, d_alpha and sampling; the env entry on the handle's own rows.
 *
 * From the repository root (leak detection off: the emulator keeps its fiber stacks for the life of the process):
 *
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Ipybullet_multigoal_gym_amd/csrc \
 *       -Wno-unknown-pragmas -o sac_memcheck tools/sac_memcheck.cpp tests/emu/hip_emu.cpp tests/emu/pmg_probe.cpp \
 *       pybullet_multigoal_gym_amd/csrc/pmg_api.cpp -x c++ pybullet_multigoal_gym_amd/csrc/pmg_kernels.hip -lrt
 *   ASAN_OPTIONS=detect_leaks=0 ./sac_memcheck
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
            if (base[i] != 0xA5) { fprintf(stderr, "sac_memcheck: bytes in front of a buffer were written\n"); abort(); }
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
/* rows of `width` floats at `stride`: the last row ends with its last element */
static size_t rows(long long B, int width, int stride) { return (size_t)(B - 1) * stride + width; }

static int sample_calls = 0, target_calls = 0, env_calls = 0;
/* outs bits: 1 d_action, 2 d_logp, 4 d_noise, 8 d_preact; variant bits: 1 sample, 2 a narrow clamp, 4 a large row_offset */
static void run_sample(int Dx, int A, const std::vector<int>& ah, long long B, int pad, int shift, int outs, int variant)
{
    Net actor(shape(Dx, ah, 2 * A), shift & 1, shift, 0);
    auto x = floats(rows(B, Dx, Dx + pad), shift);
    const int as = A + pad, ns = A + (pad + 1) % 3, ps = 2 * A + (pad + 2) % 3;
    auto a = floats(rows(B, A, as), (shift + 1) & 3), lp = floats((size_t)B, (shift + 2) & 3), n = floats(rows(B, A, ns), (shift + 3) & 3),
         z = floats(rows(B, 2 * A, ps), shift);
    pmg_sac_sample s;
    memset(&s, 0, sizeof(s));
    s.struct_size = sizeof(s); s.ls_lo = variant & 2 ? -1.f : -20.f; s.ls_hi = variant & 2 ? -0.5f : 2.f; s.sample = variant & 1;
    s.seed = 3; s.counter = (uint64_t)variant; s.row_offset = variant & 4 ? ((int64_t)1 << 40) + 5 : 0;
    s.batch = B; s.d_x = x->p; s.x_stride = Dx + pad;
    if (outs & 1) { s.d_action = a->p; s.action_stride = as; }
    if (outs & 2) s.d_logp = lp->p;
    if (outs & 4) { s.d_noise = n->p; s.noise_stride = ns; }
    if (outs & 8) { s.d_preact = z->p; s.preact_stride = ps; }
    CHECK(pmg_sac_sample_device(env, &actor.m, &s));
    CHECK(pmg_sync(env));
    sample_calls++;
}
/* variant bits: 1 sample, 2 clips, 4 d_terminal, 8 d_q_min, 16 d_next_action, 32 d_q1, 64 d_q2, 128 critic 2, 256 d_logp, 512 d_alpha */
static void run_target(int Dx, int A, const std::vector<int>& ah, const std::vector<int>& h1, const std::vector<int>& h2, long long B, int pad, int shift, int variant)
{
    const bool twin = variant & 128;
    Net actor(shape(Dx, ah, 2 * A), shift & 1, shift, 0), c1(shape(Dx + A, h1, 1), !(shift & 1), (shift + 1) & 3, 0),
        c2(shape(Dx + A, h2, 1), shift & 2, (shift + 2) & 3, (variant >> 1) & 1);
    auto x = floats(rows(B, Dx, Dx + pad), shift), r = floats((size_t)B, (shift + 1) & 3);
    auto y = floats((size_t)B, (shift + 2) & 3), qm = floats((size_t)B, (shift + 3) & 3), q1 = floats((size_t)B, shift), q2 = floats((size_t)B, (shift + 1) & 3);
    auto na = floats((size_t)B * A, (shift + 2) & 3), lp = floats((size_t)B, (shift + 3) & 3), al = floats(1, shift);
    Buf term((size_t)B, 1);                                   /* B bytes at an odd address */
    al->p[0] = 0.2f;
    pmg_sac_target td;
    memset(&td, 0, sizeof(td));
    td.struct_size = sizeof(td); td.gamma = 0.98f; td.clip_lo = variant & 2 ? -50.f : -INFINITY; td.clip_hi = variant & 2 ? 0.f : INFINITY;
    td.alpha = 0.1f; td.ls_lo = -20.f; td.ls_hi = 2.f; td.sample = variant & 1; td.seed = 3; td.counter = (uint64_t)variant;
    td.row_offset = variant & 4 ? ((int64_t)1 << 40) + 5 : 0;
    td.batch = B; td.d_x_next = x->p; td.x_stride = Dx + pad; td.d_reward = r->p; td.d_y = y->p;
    td.d_terminal = variant & 4 ? term.bytes : nullptr;
    td.d_q_min = variant & 8 ? qm->p : nullptr;
    td.d_next_action = variant & 16 ? na->p : nullptr;
    td.d_q1 = variant & 32 ? q1->p : nullptr;
    td.d_q2 = variant & 64 ? q2->p : nullptr;
    td.d_logp = variant & 256 ? lp->p : nullptr;
    td.d_alpha = variant & 512 ? al->p : nullptr;
    const int64_t need = pmg_sac_target_work_floats(&actor.m, td.d_next_action != nullptr, B);
    if (need != (td.d_next_action ? 0 : B * A)) { fprintf(stderr, "sac_memcheck: workspace figure %lld\n", (long long)need); exit(1); }
    std::unique_ptr<Buf> work;
    if (need > 0) { work = floats((size_t)need, (shift + 3) & 3); td.d_work = work->p; td.work_floats = need; }
    CHECK(pmg_sac_target_device(env, &actor.m, &c1.m, twin ? &c2.m : nullptr, &td));
    CHECK(pmg_sync(env));
    target_calls++;
}

int main()
{
    const long long batches[5] = {1, 31, 32, 33, 101};
    const int as[7] = {1, 2, 31, 32, 33, 127, 128};
    const int hidden[7] = {1, 2, 31, 33, 255, 256, 32};
    pmg_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg); cfg.task = PMG_TASK_REACH; cfg.num_envs = 37; cfg.binary_reward = 1;
    cfg.max_episode_steps = 50; cfg.distance_threshold = 0.05f; cfg.seed_stride = 1; cfg.env_index_offset = 32;
    CHECK(pmg_create(&cfg, &env));
    /* every A with a small and a large Dx (Dx + A = 256 where it fits the critic), every hidden width in turn, every output combination in turn */
    int n = 0;
    for (int k = 0; k < 7; k++) {
        const int A = as[k], w = hidden[k];
        for (int v = 0; v < 2; v++, n++) {
            const int full = 1 + 128 + (v ? 8 + 32 + 64 + 4 + 2 + 256 : 16 + 512);       /* sampling, twin; v: workspace path / d_next_action */
            run_sample(3, A, {w}, batches[n % 5], n % 3, n & 3, 1 + (n * 5) % 15, 1 + 2 * v);
            run_sample(256 - A, A, {w, 33}, batches[(n + 1) % 5], (n + 1) % 3, (n + 1) & 3, (1 + (n * 7 + 3) % 15) | (n & 1 ? 1 : 2), 1 + 4 * v);
            run_sample(A < 6 ? 1 : 5, A, {}, batches[(n + 2) % 5], (n + 2) % 3, (n + 2) & 3, 15, v);
            run_target(3, A, {w}, {w, 33}, {33, w}, batches[n % 5], n % 3, n & 3, full);
            run_target(256 - A, A, {33}, {w}, {w, w, w}, batches[(n + 3) % 5], (n + 1) % 3, (n + 1) & 3, full ^ 1);
            run_target(1, A, {w, w, w}, {}, {w}, batches[(n + 4) % 5], (n + 2) % 3, (n + 2) & 3, full ^ 128);
        }
    }
    /* Dx + A = 256 with the hazard shape A = 20 beside it, and the widest head behind three wide layers */
    for (int v = 0; v < 4; v++) {
        run_target(236, 20, {256}, {256}, {33, 256}, 33, 1, v, 1 + 128 + (v & 1 ? 16 : 0) + (v & 2 ? 512 : 0) + 8 + 32 + 64 + 256);
        run_target(128, 128, {256, 256, 256}, {256, 256, 256}, {256, 256, 256}, 101, 0, 3 - v, 1 + (v & 1 ? 128 : 0) + (v & 2 ? 16 : 0) + 4 + 2);
        run_target(1, 20, {33}, {33}, {33}, 32, 2, v, (v & 1 ? 128 : 0) + (v & 2 ? 0 : 16) + 8 + 256);
        run_target(255, 1, {33}, {33}, {33}, 33, v % 3, v, 1 + 128 + 16 * (v & 1));
    }
    /* every 4-byte phase x every batch, the odd Dx + A = 33 */
    for (int shift = 0; shift < 4; shift++)
        for (long long B : batches) {
            run_target(29, 4, {256}, {256, 33}, {33}, B, shift, shift, 1 + 128 + 8 * shift + (int)(B & 6) + (B & 1 ? 0 : 16) + 64 + 256);
            run_sample(29, 4, {256}, B, shift % 3, shift, 15, 1);
        }
    /* every combination of the optional outputs: the 12 of the sample entry that request d_action or d_logp x sampling, all 1024 variants of the target */
    for (int outs = 1; outs < 16; outs++)
        if (outs & 3)
            for (int v = 0; v < 8; v++) run_sample(6, 3, {33}, v % 5 == 0 ? 33 : 5, v % 3, v & 3, outs, v);
    for (int variant = 0; variant < 1024; variant++) run_target(6, 3, {33}, {33}, {17, 9}, variant % 5 == 0 ? 33 : 5, variant % 3, variant & 3, variant);
    /* the env entry: 37 envs (two tiles), every output combination, on the rows of the reset */
    {
        pmg_dims d;
        CHECK(pmg_get_dims(env, &d));
        CHECK(pmg_reset(env, nullptr, nullptr, nullptr, nullptr, nullptr));
        const int A = d.action_dim, W0 = d.policy_state_dim + d.goal_dim;
        for (int outs = 1; outs < 16; outs++) {
            if (!(outs & 3)) continue;
            const int shift = outs & 3;
            Net actor(shape(W0, {33}, 2 * A), outs & 1, shift, 0);
            auto a = floats(rows(d.num_envs, A, A + 1), (shift + 1) & 3), lp = floats((size_t)d.num_envs, (shift + 2) & 3), nn = floats((size_t)d.num_envs * A, (shift + 3) & 3),
                 z = floats(rows(d.num_envs, 2 * A, 2 * A + 2), shift);
            pmg_sac_sample s;
            memset(&s, 0, sizeof(s));
            s.struct_size = sizeof(s); s.ls_lo = -20.f; s.ls_hi = 2.f; s.sample = outs & 4 ? 1 : 0; s.seed = 5; s.counter = (uint64_t)outs;
            if (outs & 1) { s.d_action = a->p; s.action_stride = A + 1; }
            if (outs & 2) s.d_logp = lp->p;
            if (outs & 4) { s.d_noise = nn->p; s.noise_stride = A; }
            if (outs & 8) { s.d_preact = z->p; s.preact_stride = 2 * A + 2; }
            CHECK(pmg_sac_act_env_device(env, &actor.m, PMG_NORM_POLICY_STATE, &s));
            CHECK(pmg_sync(env));
            env_calls++;
        }
    }
    pmg_destroy(env);
    printf("sac_memcheck: %d calls of pmg_sac_sample_device, %d of pmg_sac_act_env_device, %d of pmg_sac_target_device, no finding\n", sample_calls, env_calls,
           target_calls);
    return 0;
}
