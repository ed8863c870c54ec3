/* grad_chunk_memcheck.cpp -- memory safety of pmg_mlp_grad_chunked_device (pmg_k_mlp_grad_rows, pmg_k_mlp_grad_partials and pmg_k_mlp_grad_merge
 * of csrc/pmg_learner_body.inc) off the GPU: a stand-alone program over the g++ emulator build of the product sources (tests/emu), meant to be
 * compiled with -fsanitize=address,undefined, in the manner of tools/grad_memcheck.cpp.  "Device" memory is malloc'd there, so every buffer
 * below is sized EXACTLY -- weights, biases, gradients, the last row of a padded table without its padding, the workspace at
 * pmg_mlp_grad_chunked_work_floats (with grads NULL: at pmg_mlp_grad_work_floats) -- with guard bytes in front that are checked when the buffer
 * goes; a read or write one float outside any of them stops the run.  Covered: layer widths 1, 2, 31, 32, 33, 255, 256 in every position, one
 * to four layers, cat and raw rows, chunk_rows 2, 16, 34, batches 1, 33, 101, padded strides, every 4-byte phase of every float pointer, grads
 * NULL and given, every optional output given and NULL, the three heads, both output activations, networks with and without biases.
 *
 * From the repository root (leak detection off: the emulator keeps its fiber stacks for the life of the process):
 *
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Ipybullet_multigoal_gym_amd/csrc \
 *       -Wno-unknown-pragmas -o grad_chunk_memcheck tools/grad_chunk_memcheck.cpp tests/emu/hip_emu.cpp tests/emu/pmg_probe.cpp \
 *       pybullet_multigoal_gym_amd/csrc/pmg_api.cpp -x c++ pybullet_multigoal_gym_amd/csrc/pmg_kernels.hip -lrt
 *   ASAN_OPTIONS=detect_leaks=0 ./grad_chunk_memcheck
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
    unsigned char* end = nullptr;
    float* p = nullptr;
    size_t lead;
    Buf(size_t n, int shift) : lead(4 * (size_t)shift)
    {
        base = (unsigned char*)malloc(lead + 4 * n);
        end = base + lead + 4 * n;
        memset(base, 0xA5, lead);
        p = (float*)(base + lead);
        for (size_t i = 0; i < n; i++) p[i] = (float)((i * 7) % 13) * 0.125f - 0.75f;
    }
    ~Buf()
    {
        for (size_t i = 0; i < lead; i++)
            if (base[i] != 0xA5) { fprintf(stderr, "grad_chunk_memcheck: bytes in front of a buffer were written\n"); abort(); }
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

static int ncalls = 0, nchunked = 0;

/* variant: bit 0 tanh output, bits 1-2 head (0 target, 1 gout, 2 / 3 constant), bit 3 grads, bit 4 d_gx, bit 5 d_ga, bit 6 d_out, bit 7 bias */
static void run_grad(const std::vector<int>& widths, int x_dim, long long B, long long R, int pad, int shift, int variant)
{
    const int a_dim = widths[0] - x_dim, A = widths.back(), head = (variant >> 1) & 3;
    const bool bias = variant & 128;
    Tensors net(widths, bias, shift), grads(widths, bias, shift + 1);
    pmg_mlp m = mlp_of(widths, net, variant & 1);
    /* the last row of a padded table ends with its last float: no padding behind it */
    auto rows = [&](int w, int sh) { return floats((size_t)(B - 1) * (w + pad) + w, sh); };
    BufP x = rows(x_dim, shift), a = a_dim ? rows(a_dim, shift + 1) : nullptr, head_rows = head < 2 ? rows(A, shift + 2) : nullptr;
    BufP gx = rows(x_dim, shift + 3), ga = a_dim ? rows(a_dim, shift) : nullptr, out = rows(A, shift + 1);
    const int64_t work = (variant & 8) ? pmg_mlp_grad_chunked_work_floats(&m, B, R) : pmg_mlp_grad_work_floats(&m, B);
    if (work < 0) { fprintf(stderr, "grad_chunk_memcheck: the workspace size of a valid call was refused\n"); exit(1); }
    BufP w = floats((size_t)work, shift + 2);
    pmg_mlp_grad g;
    memset(&g, 0, sizeof(g));
    g.struct_size = sizeof(g); g.batch = B; g.gscale = 0.25f;
    g.d_x = x->p; g.x_stride = x_dim + pad; g.x_dim = x_dim;
    if (a_dim) { g.d_a = a->p; g.a_stride = a_dim + pad; g.a_dim = a_dim; }
    if (head == 0) { g.d_target = head_rows->p; g.target_stride = A + pad; }
    if (head == 1) { g.d_gout = head_rows->p; g.gout_stride = A + pad; }
    bool any = false;
    if (variant & 8) { g.grads = &grads.p; any = true; }
    if (variant & 16) { g.d_gx = gx->p; g.gx_stride = x_dim + pad; any = true; }
    if ((variant & 32) && a_dim) { g.d_ga = ga->p; g.ga_stride = a_dim + pad; any = true; }
    if ((variant & 64) || !any) { g.d_out = out->p; g.out_stride = A + pad; }
    g.d_work = w->p; g.work_floats = work;
    CHECK(pmg_mlp_grad_chunked_device(env, &m, &g, R));
    CHECK(pmg_sync(env));
    ncalls++;
    if ((variant & 8) && R < B) nchunked++;
}

int main()
{
    const long long batches[3] = {1, 33, 101}, chunks[3] = {2, 16, 34};
    const int ws[7] = {1, 2, 31, 32, 33, 255, 256};
    pmg_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg); cfg.task = PMG_TASK_REACH; cfg.num_envs = 2; cfg.binary_reward = 1;
    cfg.max_episode_steps = 50; cfg.distance_threshold = 0.05f; cfg.seed_stride = 1;
    CHECK(pmg_create(&cfg, &env));
    int n = 0;
    /* the widths 1, 2, 31, 32, 33, 255, 256 as input, hidden and output width; every phase; one to four layers; B and R in turn */
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++, n++) {
            run_grad({ws[i], ws[j]}, ws[i], batches[n % 3], chunks[(n / 3) % 3], n % 3, n & 3, 0xF8 | (n & 7));
            run_grad({ws[j], ws[i], ws[(i + j) % 7]}, ws[j] > 1 ? ws[j] - 1 : 1, batches[(n + 1) % 3], chunks[n % 3], (n + 1) % 3, (n + 2) & 3, (n & 1 ? 0x78 : 0xF8) | (n & 7));
        }
    for (int i = 0; i < 7; i++, n++)
        for (int r = 0; r < 3; r++)
            run_grad({ws[i], ws[(i + 3) % 7], ws[(i + 5) % 7], ws[(i + 1) % 7], ws[(i + 2) % 7]}, ws[i], batches[(n + r) % 3], chunks[r], n % 3, n & 3, 0xF8 | (n & 7));
    /* every R x every B x every phase on a critic and an actor, grads given and NULL */
    for (int shift = 0; shift < 4; shift++)
        for (long long B : batches)
            for (long long R : chunks) {
                run_grad({9, 33, 1}, 6, B, R, shift, shift, 0xF8 | (shift << 1));
                run_grad({9, 33, 1}, 6, B, R, shift, shift, 0x70);
                run_grad({6, 33, 3}, 6, B, R, shift, shift + 1, 0xD9 | (shift << 1));
            }
    /* every optional output given and NULL, the heads, both activations, with and without biases */
    for (int variant = 0; variant < 256; variant += 3) run_grad({9, 33, 33, 3}, variant & 4 ? 6 : 9, 101, chunks[variant % 3], variant % 3, variant & 3, variant);
    /* the learner's networks */
    for (int r = 0; r < 3; r++) {
        run_grad({13, 256, 256, 256, 1}, 9, batches[r], chunks[2 - r], r, r, 0xF8);
        run_grad({6, 256, 256, 256, 3}, 6, batches[(r + 1) % 3], chunks[r], r, r + 1, 0xD9);
    }
    run_grad({256, 33, 1}, 252, 33, 2, 1, 1, 0xF8);             /* Dx + A = 256 */
    run_grad({256, 256, 1}, 1, 101, 34, 0, 3, 0xFA);
    pmg_destroy(env);
    printf("grad_chunk_memcheck: %d calls of pmg_mlp_grad_chunked_device, %d of them reduced over two chunks or more, no finding\n", ncalls, nchunked);
    return 0;
}
