/* dp_memcheck.cpp -- memory safety of the data-parallel merge (pmg_mlp_params_pack_device, pmg_mlp_params_merge_device,
 * pmg_mlp_adam_merge_device and, over a one-rank communicator, pmg_mlp_grad_allreduce_device, pmg_mlp_adam_allreduce_device,
 * pmg_norm_update_ranks_device and pmg_allgather_device; pmg_k_params_pack, pmg_k_params_merge_ranks and pmg_k_adam_merge_ranks of
 * csrc/pmg_learner_body.inc) off the GPU: a stand-alone program over the g++ emulator build of the product sources (tests/emu), meant to be
 * compiled with -fsanitize=address,undefined, in the manner of tools/grad_chunk_memcheck.cpp.  "Device" memory is malloc'd there, so every buffer
 * below is sized EXACTLY -- every tensor, the flat run of P floats, the slots up to the last float of the last slot, the workspace at
 * pmg_mlp_allreduce_work_floats, the rows of the normaliser without the padding of the last row -- with guard bytes in front that are checked when
 * the buffer goes; a read or write one float outside any of them stops the run.  Covered: R = 3 slots (and 1, 2, 8) with slot strides P and
 * beyond, layer widths 1, 2, 31, 32, 33, 255, 256 in every position, one to four layers, every 4-byte phase of every pointer, networks with
 * biases, without, and with a bias on some layers only, grad_out given and NULL.
 *
 * From the repository root (leak detection off: the emulator keeps its fiber stacks for the life of the process):
 *
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Ipybullet_multigoal_gym_amd/csrc \
 *       -Wno-unknown-pragmas -o dp_memcheck tools/dp_memcheck.cpp tests/emu/hip_emu.cpp tests/emu/pmg_probe.cpp \
 *       pybullet_multigoal_gym_amd/csrc/pmg_api.cpp -x c++ pybullet_multigoal_gym_amd/csrc/pmg_kernels.hip -lrt
 *   ASAN_OPTIONS=detect_leaks=0 ./dp_memcheck
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
        for (size_t i = 0; i < n; i++) p[i] = (float)((i * 7) % 13) * 0.125f + 0.0625f;
    }
    ~Buf()
    {
        for (size_t i = 0; i < lead; i++)
            if (base[i] != 0xA5) { fprintf(stderr, "dp_memcheck: bytes in front of a buffer were written\n"); abort(); }
        free(base);
    }
};
typedef std::unique_ptr<Buf> BufP;
static BufP floats(size_t n, int shift) { return BufP(new Buf(n, shift & 3)); }

/* tensors shaped like the network widths[0..L] in exactly sized buffers, tensor k at phase shift + k; bias: bit l = layer l has one */
struct Tensors {
    pmg_mlp_params p;
    std::vector<BufP> bufs;
    Tensors(const std::vector<int>& widths, int bias, int shift)
    {
        memset(&p, 0, sizeof(p));
        for (size_t l = 0; l + 1 < widths.size(); l++) {
            bufs.push_back(floats((size_t)widths[l] * widths[l + 1], shift++));
            p.d_weight[l] = bufs.back()->p;
            if (bias >> l & 1) { bufs.push_back(floats((size_t)widths[l + 1], shift++)); p.d_bias[l] = bufs.back()->p; }
        }
    }
};
static pmg_mlp mlp_of(const std::vector<int>& widths, const Tensors& t)
{
    pmg_mlp m;
    memset(&m, 0, sizeof(m));
    m.struct_size = sizeof(m); m.num_layers = (int)widths.size() - 1;
    for (size_t l = 0; l < widths.size(); l++) m.width[l] = widths[l];
    for (int l = 0; l < m.num_layers; l++) { m.d_weight[l] = t.p.d_weight[l]; m.d_bias[l] = t.p.d_bias[l]; }
    return m;
}

static int ncalls = 0;

/* pack R gradients into R slots `extra` floats apart, merge them, then the fused merge + Adam with and without grad_out; then the same
 * network through the one-rank all-reduce pair */
static void run_net(const std::vector<int>& widths, int bias, int R, int extra, int shift)
{
    Tensors net(widths, bias, shift), out(widths, bias, shift + 1), m(widths, bias, shift + 2), v(widths, bias, shift + 3), gout(widths, bias, shift);
    pmg_mlp shape = mlp_of(widths, net);
    const int64_t P = pmg_mlp_param_floats(&shape);
    if (P < 1) { fprintf(stderr, "dp_memcheck: the parameter count of a valid network was refused\n"); exit(1); }
    const int64_t stride = P + extra;
    BufP slots = floats((size_t)((R - 1) * stride + P), shift + 1);
    for (int r = 0; r < R; r++) {
        Tensors g(widths, bias, shift + r);
        CHECK(pmg_mlp_params_pack_device(env, &shape, &g.p, slots->p + r * stride));
        CHECK(pmg_sync(env));
        ncalls++;
    }
    CHECK(pmg_mlp_params_merge_device(env, &shape, slots->p, stride, R, &out.p));
    pmg_adam a;
    memset(&a, 0, sizeof(a));
    a.struct_size = sizeof(a); a.lr = 1e-3f; a.beta1 = 0.9f; a.beta2 = 0.999f; a.eps = 1e-8f; a.step = 3;
    CHECK(pmg_mlp_adam_merge_device(env, &shape, &net.p, slots->p, stride, R, &gout.p, &m.p, &v.p, &a));
    CHECK(pmg_mlp_adam_merge_device(env, &shape, &net.p, slots->p, stride, R, nullptr, &m.p, &v.p, &a));
    CHECK(pmg_mlp_params_merge_device(env, &shape, slots->p, stride, 1, &out.p));
    CHECK(pmg_sync(env));
    ncalls += 4;
    const int64_t work = pmg_mlp_allreduce_work_floats(env, &shape);
    if (work != 2 * P) { fprintf(stderr, "dp_memcheck: the all-reduce workspace of one rank is not 2 P\n"); exit(1); }
    BufP w = floats((size_t)work, shift + 2);
    CHECK(pmg_mlp_grad_allreduce_device(env, &shape, &gout.p, w->p, work));
    CHECK(pmg_mlp_adam_allreduce_device(env, &shape, &net.p, &gout.p, &m.p, &v.p, &a, w->p, work));
    CHECK(pmg_sync(env));
    ncalls += 2;
}

/* the collective normaliser update of one rank on B rows of normaliser `which` (width D) with `pad` floats between rows, masked or not */
static void run_norm(int which, int D, long long B, int pad, int shift, bool masked)
{
    BufP rows = floats((size_t)((B - 1) * (D + pad) + D), shift);
    std::vector<uint8_t> mask((size_t)B);
    for (long long i = 0; i < B; i++) mask[(size_t)i] = (uint8_t)(i % 3 != 0);
    CHECK(pmg_norm_update_ranks_device(env, which, rows->p, D + pad, B, masked ? mask.data() : nullptr));
    CHECK(pmg_sync(env));
    ncalls++;
}

int main()
{
    const int ws[7] = {1, 2, 31, 32, 33, 255, 256};
    pmg_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg); cfg.task = PMG_TASK_PUSH; cfg.num_envs = 64; cfg.binary_reward = 1;
    cfg.max_episode_steps = 50; cfg.distance_threshold = 0.05f; cfg.seed_stride = 1;
    CHECK(pmg_create(&cfg, &env));
    uint8_t id[128];
    CHECK(pmg_comm_unique_id(id));
    CHECK(pmg_comm_init(env, 0, 1, id));
    int n = 0;
    /* R = 3 with odd widths: every width as input, hidden and output width, one to four layers, every phase, strides P, P + 1, P + 2 */
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++, n++) {
            run_net({ws[i], ws[j]}, n & 1, 3, n % 3, n & 3);
            run_net({ws[j], ws[i], ws[(i + j) % 7]}, n & 3, 3, (n + 1) % 3, (n + 1) & 3);
        }
    for (int i = 0; i < 7; i++, n++) {
        run_net({ws[i], ws[(i + 3) % 7], ws[(i + 5) % 7], ws[(i + 1) % 7]}, n & 7, 3, n % 3, n & 3);
        run_net({ws[i], ws[(i + 3) % 7], ws[(i + 5) % 7], ws[(i + 1) % 7], ws[(i + 2) % 7]}, (n * 5) & 15, 3, (n + 2) % 3, (n + 1) & 3);
    }
    /* other rank counts on the learner's networks and on odd ones */
    const int ranks[4] = {1, 2, 3, 8};
    for (int r = 0; r < 4; r++) {
        run_net({13, 256, 256, 256, 1}, 15, ranks[r], r, r);
        run_net({6, 256, 256, 256, 3}, 15, ranks[r], 3 - r, r + 1);
        run_net({33, 255, 31}, 1, ranks[r], 1, r + 2);
    }
    /* the normaliser over the one-rank communicator: the widths of push (20, 7, 3), batches around the chunk, padded rows, every phase */
    const int D[3] = {20, 7, 3};
    const long long batches[6] = {1, 63, 64, 65, 257, 4097};
    for (int which = 0; which < 3; which++)
        for (int b = 0; b < 6; b++) run_norm(which, D[which], batches[b], b % 3, (which + b) & 3, b & 1);
    {   /* the env's own rows, and a plain all-gather */
        CHECK(pmg_reset(env, nullptr, nullptr, nullptr, nullptr, nullptr));
        CHECK(pmg_norm_update_env_ranks_device(env, nullptr));
        BufP src = floats(1001, 1), dst = floats(1001, 3);
        CHECK(pmg_allgather_device(env, src->p, 1001, dst->p));
        CHECK(pmg_sync(env));
        if (memcmp(src->p, dst->p, 4 * 1001) != 0) { fprintf(stderr, "dp_memcheck: the all-gather of one rank is no copy\n"); exit(1); }
        ncalls += 2;
    }
    pmg_destroy(env);
    printf("dp_memcheck: %d calls of the data-parallel entries, no finding\n", ncalls);
    return 0;
}
