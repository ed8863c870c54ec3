/* ppo_memcheck.cpp -- memory safety of pmg_gae_device, pmg_adv_stats_device, pmg_adv_apply_device, pmg_ppo_policy_grad_device and
 * pmg_ppo_stats_device (pmg_k_gae, pmg_k_adv_stats, pmg_k_adv_apply, pmg_k_ppo_policy_grad_rows and pmg_k_ppo_stats of csrc/pmg_learner_body.inc,
 * and the weights / partials / merge kernels the gradient call launches) off the GPU: a stand-alone program over the g++ emulator build of the
 * product sources (tests/emu), meant to be compiled with -fsanitize=address,undefined, in the manner of tools/sac_pg_memcheck.cpp.  "Device"
 * memory is malloc'd there, so every buffer below is sized EXACTLY -- weights, biases, gradient tensors, the last row of a padded table without
 * its padding, a GAE table from its first to its last addressed element, the statistics as two and four floats, the workspace as
 * pmg_ppo_policy_grad_work_floats floats (none at all without grads) -- with guard bytes in front that are checked when the buffer goes; a read
 * or write one float outside any of them stops the run.  Covered: GAE at T = 1, 2, 7, 50 and N = 1, 63, 64, 65, 257, 300 in time-major, env-major,
 * padded and packed-row layouts, a negative time stride, the shifted and the own successor table, every combination of the optional tables;
 * the normaliser and the statistics at 1, 2, 255, 256, 257, 1025 elements, in place and out of place; the gradient at A = 1, 2, 31, 32, 33, 127,
 * 128 behind every hidden width in turn, batches 1, 31, 32, 33, 101, padded strides, every 4-byte phase of every float pointer (every byte phase
 * of d_clipped), every combination of grads and the optional outputs, chunk_rows 0, 2 and 32.
 *
 * From the repository root (leak detection off: the emulator keeps its fiber stacks for the life of the process):
 *
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Ipybullet_multigoal_gym_amd/csrc \
 *       -Wno-unknown-pragmas -o ppo_memcheck tools/ppo_memcheck.cpp tests/emu/hip_emu.cpp tests/emu/pmg_probe.cpp \
 *       pybullet_multigoal_gym_amd/csrc/pmg_api.cpp -x c++ pybullet_multigoal_gym_amd/csrc/pmg_kernels.hip -lrt
 *   ASAN_OPTIONS=detect_leaks=0 ./ppo_memcheck
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
    Buf(size_t nbytes, size_t lead_bytes, bool as_bytes = false) : lead(lead_bytes)
    {
        base = (unsigned char*)malloc(lead + nbytes);
        memset(base, 0xA5, lead);
        p = (float*)(base + lead);
        if (as_bytes) for (size_t i = 0; i < nbytes; i++) base[lead + i] = (unsigned char)(i % 3 == 0);      /* d_clipped: at any address */
        else for (size_t i = 0; i < nbytes / 4; i++) p[i] = (float)((i * 7) % 13) * 0.125f - 0.75f;
    }
    ~Buf()
    {
        for (size_t i = 0; i < lead; i++)
            if (base[i] != 0xA5) { fprintf(stderr, "ppo_memcheck: bytes in front of a buffer were written\n"); abort(); }
        free(base);
    }
};
static std::unique_ptr<Buf> floats(size_t n, int shift) { return std::unique_ptr<Buf>(new Buf(4 * n, 4 * (size_t)shift)); }

/* the network widths[0..L] in exactly sized buffers, the weights `shift` floats off a 16-byte boundary; `grads`: tensors of the same shapes */
struct Net {
    pmg_mlp m;
    pmg_mlp_params grads;
    std::vector<std::unique_ptr<Buf>> bufs;
    Net(const std::vector<int>& widths, bool bias, int shift)
    {
        memset(&m, 0, sizeof(m));
        memset(&grads, 0, sizeof(grads));
        m.struct_size = sizeof(m); m.num_layers = (int)widths.size() - 1; m.out_activation = 0;
        for (size_t l = 0; l < widths.size(); l++) m.width[l] = widths[l];
        for (int l = 0; l < m.num_layers; l++) {
            bufs.push_back(floats((size_t)widths[l] * widths[l + 1], shift));
            m.d_weight[l] = bufs.back()->p;
            for (size_t i = 0; i < (size_t)widths[l] * widths[l + 1]; i++) bufs.back()->p[i] *= 0.05f;      /* keep exp(lr) finite */
            if (bias) { bufs.push_back(floats((size_t)widths[l + 1], shift)); m.d_bias[l] = bufs.back()->p; }
            bufs.push_back(floats((size_t)widths[l] * widths[l + 1], (shift + 1) & 3));
            grads.d_weight[l] = bufs.back()->p;
            if (bias) { bufs.push_back(floats((size_t)widths[l + 1], (shift + 2) & 3)); grads.d_bias[l] = bufs.back()->p; }
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

static int gae_calls = 0, adv_calls = 0, pg_calls = 0, stats_calls = 0;

/* a GAE table from its first to its last addressed element; reverse: time runs backwards from the last block */
struct Table {
    std::unique_ptr<Buf> buf;
    float* p;
    int64_t ts, es;
    Table(long long T, long long N, int64_t ts_, int64_t es_, int shift, bool reverse = false) : ts(ts_), es(es_)
    {
        buf = floats((size_t)((T - 1) * ts + (N - 1) * es + 1), shift);
        p = buf->p;
        if (reverse) { p += (T - 1) * ts; ts = -ts; }
    }
};
/* layout 0: time-major tight, 1: time-major rows of N + 3, 2: env-major columns of T + 2, 3: env-major tight */
static void strides_of(int layout, long long T, long long N, int64_t& ts, int64_t& es)
{
    if (layout == 0) { ts = N; es = 1; } else if (layout == 1) { ts = N + 3; es = 1; } else if (layout == 2) { ts = 1; es = T + 2; } else { ts = 1; es = T; }
}
/* variant bits: 1 d_cut, 2 d_terminal, 4 d_ret, 8 the shifted value table, 16 reward and cut as columns of packed rows, 32 a negative time stride of d_adv */
static void run_gae(long long T, long long N, int layout, int shift, int variant)
{
    int64_t ts, es;
    strides_of(layout, T, N, ts, es);
    const int P = 7;
    Table packed(T, N * P, N * P, 1, shift);                     /* [T, N, P] rows: reward in column 2, cut in column 5 */
    Table reward(T, N, ts, es, (shift + 1) & 3), cut(T, N, ts, es, (shift + 2) & 3), term(T, N, ts, es, (shift + 3) & 3);
    Table vtab(T + 1, N, layout >= 2 ? 1 : ts, layout >= 2 ? T + 1 + (layout == 2 ? 2 : 0) : es, shift), value(T, N, ts, es, (shift + 1) & 3), succ(T, N, ts, es, (shift + 2) & 3);
    Table adv(T, N, ts, es, (shift + 3) & 3, variant & 32), ret(T, N, layout >= 2 ? N : 1, layout >= 2 ? 1 : T, shift);   /* the other orientation */
    pmg_gae g;
    memset(&g, 0, sizeof(g));
    g.struct_size = sizeof(g); g.gamma = 0.98f; g.lambda = 0.95f; g.steps = T; g.envs = N;
    if (variant & 16) {
        g.d_reward = packed.p + 2; g.reward_time_stride = N * P; g.reward_env_stride = P;
        if (variant & 1) { g.d_cut = packed.p + 5; g.cut_time_stride = N * P; g.cut_env_stride = P; }
    } else {
        g.d_reward = reward.p; g.reward_time_stride = reward.ts; g.reward_env_stride = reward.es;
        if (variant & 1) { g.d_cut = cut.p; g.cut_time_stride = cut.ts; g.cut_env_stride = cut.es; }
    }
    if (variant & 8) {
        g.d_value = vtab.p; g.d_value_next = vtab.p + vtab.ts;
        g.value_time_stride = g.value_next_time_stride = vtab.ts; g.value_env_stride = g.value_next_env_stride = vtab.es;
    } else {
        g.d_value = value.p; g.value_time_stride = value.ts; g.value_env_stride = value.es;
        g.d_value_next = succ.p; g.value_next_time_stride = succ.ts; g.value_next_env_stride = succ.es;
    }
    if (variant & 2) { g.d_terminal = term.p; g.terminal_time_stride = term.ts; g.terminal_env_stride = term.es; }
    g.d_adv = adv.p; g.adv_time_stride = adv.ts; g.adv_env_stride = adv.es;
    if (variant & 4) { g.d_ret = ret.p; g.ret_time_stride = ret.ts; g.ret_env_stride = ret.es; }
    CHECK(pmg_gae_device(env, &g));
    CHECK(pmg_sync(env));
    gae_calls++;
}
static void run_adv(long long M, int shift, int ddof, bool inplace)
{
    auto x = floats((size_t)M, shift), y = floats((size_t)M, (shift + 1) & 3), st = floats(2, (shift + 2) & 3);
    pmg_adv_stats s;
    memset(&s, 0, sizeof(s));
    s.struct_size = sizeof(s); s.ddof = ddof; s.eps = 1e-8f; s.count = M; s.d_x = x->p; s.d_stats = st->p;
    CHECK(pmg_adv_stats_device(env, &s));
    CHECK(pmg_adv_apply_device(env, x->p, M, st->p, inplace ? x->p : y->p));
    CHECK(pmg_sync(env));
    if (!std::isfinite(st->p[0]) || !(st->p[1] > 0.f)) { fprintf(stderr, "ppo_memcheck: statistics %g %g\n", (double)st->p[0], (double)st->p[1]); exit(1); }
    adv_calls++;
}
static void run_stats(long long B, int shift)
{
    auto rho = floats((size_t)B, shift), lr = floats((size_t)B, (shift + 1) & 3), adv = floats((size_t)B, (shift + 2) & 3), st = floats(4, (shift + 3) & 3);
    std::unique_ptr<Buf> cl(new Buf((size_t)B, (size_t)shift + 1, true)); /* bytes, at any address */
    pmg_ppo_stats s;
    memset(&s, 0, sizeof(s));
    s.struct_size = sizeof(s); s.clip_lo = 0.8f; s.clip_hi = 1.2f; s.batch = B;
    s.d_ratio = rho->p; s.d_logratio = lr->p; s.d_clipped = (const uint8_t*)cl->p; s.d_adv = adv->p; s.d_stats = st->p;
    CHECK(pmg_ppo_stats_device(env, &s));
    CHECK(pmg_sync(env));
    stats_calls++;
}
/* variant bits: 1 grads, 2 d_ratio, 4 d_logratio, 8 d_clipped, 16 d_ghead, 32 chunk_rows 2, 64 chunk_rows 32, 128 a narrow clamp and an open clip */
static void run_pg(int Dx, int A, const std::vector<int>& hidden, bool bias, long long B, int pad, int shift, int variant)
{
    if (!(variant & 31)) variant |= 2;                             /* something has to be asked for */
    const int64_t R = variant & 32 ? 2 : (variant & 64 ? 32 : 0);
    Net actor(shape(Dx, hidden, 2 * A), bias, shift);
    const int zs = 2 * A + (pad + 1) % 3, ns = A + (pad + 2) % 3, hs = 2 * A + pad;
    auto x = floats(rows(B, Dx, Dx + pad), shift), zo = floats(rows(B, 2 * A, zs), (shift + 1) & 3), n = floats(rows(B, A, ns), (shift + 2) & 3);
    auto adv = floats((size_t)B, (shift + 3) & 3), rho = floats((size_t)B, shift), lr = floats((size_t)B, (shift + 1) & 3), gh = floats(rows(B, 2 * A, hs), (shift + 2) & 3);
    std::unique_ptr<Buf> cl(new Buf((size_t)B, (size_t)(variant & 3) + 1, true));
    pmg_ppo_policy_grad g;
    memset(&g, 0, sizeof(g));
    g.struct_size = sizeof(g); g.pscale = -1.f / (float)B; g.escale = -0.01f / (float)B;
    g.clip_lo = variant & 128 ? 0.f : 0.8f; g.clip_hi = variant & 128 ? INFINITY : 1.2f;
    g.ls_lo = variant & 128 ? -1.f : -20.f; g.ls_hi = variant & 128 ? -0.5f : 2.f;
    g.batch = B; g.d_x = x->p; g.x_stride = Dx + pad; g.d_preact_old = zo->p; g.preact_old_stride = zs; g.d_noise = n->p; g.noise_stride = ns; g.d_adv = adv->p;
    g.grads = variant & 1 ? &actor.grads : nullptr;
    if (variant & 2) g.d_ratio = rho->p;
    if (variant & 4) g.d_logratio = lr->p;
    if (variant & 8) g.d_clipped = (uint8_t*)cl->p;
    if (variant & 16) { g.d_ghead = gh->p; g.ghead_stride = hs; }
    const int64_t need = pmg_ppo_policy_grad_work_floats(&actor.m, B, g.grads ? R : 0);
    const int64_t base = g.grads && R ? pmg_mlp_grad_chunked_work_floats(&actor.m, B, R) : pmg_mlp_grad_work_floats(&actor.m, B);
    if (need != base || need < 0) { fprintf(stderr, "ppo_memcheck: workspace figure %lld\n", (long long)need); exit(1); }
    std::unique_ptr<Buf> work;
    if (g.grads) { work = floats((size_t)need, (shift + 3) & 3); g.d_work = work->p; g.work_floats = need; }      /* without grads: no workspace at all */
    CHECK(pmg_ppo_policy_grad_device(env, &actor.m, &g, R));
    CHECK(pmg_sync(env));
    pg_calls++;
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
    /* GAE: every T x N x layout, every combination of the optional tables and of the ways to pass the tables */
    const long long Ts[4] = {1, 2, 7, 50}, Ns[6] = {1, 63, 64, 65, 257, 300};
    int n = 0;
    for (long long T : Ts)
        for (long long N : Ns)
            for (int layout = 0; layout < 4; layout++, n++) {
                run_gae(T, N, layout, n & 3, n % 64);
                run_gae(T, N, layout, (n + 1) & 3, 63 - n % 64);
            }
    for (int variant = 0; variant < 64; variant++) run_gae(7, 65, variant & 3, variant & 3, variant);
    /* the normaliser and the statistics */
    const long long Ms[6] = {1, 2, 255, 256, 257, 1025};
    for (long long M : Ms)
        for (int shift = 0; shift < 4; shift++) {
            run_adv(M, shift, 0, shift & 1);
            if (M > 1) run_adv(M, shift, 1, !(shift & 1));
            run_stats(M, shift);
        }
    /* the gradient: every A with a small and a large Dx and with Dx < A, every hidden width in turn; chunk_rows 0, 2 and 32 */
    const int all = 31;
    n = 0;
    for (int k = 0; k < 7; k++) {
        const int A = as[k], w = hidden[k];
        for (int v = 0; v < 2; v++, n++) {
            run_pg(3, A, {w}, v, batches[n % 5], n % 3, n & 3, all + (v ? 32 : 0));
            run_pg(256, A, {33, w}, !v, batches[(n + 3) % 5], (n + 1) % 3, (n + 1) & 3, all + (v ? 0 : 64) + 128);
            run_pg(1, A, {w, w, w}, v, batches[(n + 4) % 5], (n + 2) % 3, (n + 2) & 3, (all ^ (v ? 16 : 0)) + (v ? 64 : 32));
            run_pg(2, A, {}, !v, batches[(n + 2) % 5], n % 3, (n + 3) & 3, all ^ (v ? 1 : 0));
        }
    }
    /* the widest head behind three wide layers; every 4-byte phase x every batch */
    for (int v = 0; v < 4; v++) run_pg(128, 128, {256, 256, 256}, v & 1, 101, v % 3, v, all + (v & 2 ? 32 : 0));
    for (int shift = 0; shift < 4; shift++)
        for (long long B : batches) run_pg(29, 4, {256}, shift & 1, B, shift % 3, shift, all + (shift & 1 ? 32 : 0) + (shift & 2 ? 128 : 0));
    /* every combination of grads, the optional outputs, the chunk regimes and the clamp / clip regime: all 256 variants at two shapes */
    for (int variant = 0; variant < 256; variant++) {
        if ((variant & 96) == 96) continue;                        /* one chunk regime at a time */
        run_pg(6, 3, {33}, variant & 1, variant % 5 == 0 ? 33 : 5, variant % 3, variant & 3, variant);
        run_pg(2, 20, {17, 9}, !(variant & 1), variant % 7 == 0 ? 65 : 33, (variant + 1) % 3, (variant >> 1) & 3, variant);
    }
    pmg_destroy(env);
    printf("ppo_memcheck: %d calls of pmg_gae_device, %d of pmg_adv_stats_device + pmg_adv_apply_device, %d of pmg_ppo_policy_grad_device, %d of pmg_ppo_stats_device, no finding\n",
           gae_calls, adv_calls, pg_calls, stats_calls);
    return 0;
}
