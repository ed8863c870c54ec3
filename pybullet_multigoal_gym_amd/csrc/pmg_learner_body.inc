/* pmg_learner_body.inc -- the learner-side kernels and their launchers (included by pmg_kernels.hip): rewards of [B, G] batches,
 * the running normaliser, policy-input rows, HER minibatches, the actor forward, the critic / TD target, back-propagation, Adam and
 * Polyak, and the actor's gradient through the critic in one call (DESIGN.md 3.6-3.13).  None of them touches EnvParams.  What two kernels share has ONE definition, so that they agree bit for bit
 * by construction: reward_of, sq_dist, policy_norm, flat_sweep, mlp_gather, mlp_layers, mlp_mma / mlp_chain. */
/* distance, threshold, binary -> reward value and flag: the one definition (all three reward kernels and pmg_k_her_draw) */
__device__ __forceinline__ float reward_of(float d, float thr, int binary, unsigned char& ok)
{
    const bool na = d > thr;
    ok = na ? 0 : 1;
    return binary ? (na ? -1.f : -0.f) : -d;
}
/* the dword sum of squares of item i of two [*, G] arrays, columns in ascending order (pmg_k_reward and pmg_k_her_draw) */
__device__ __forceinline__ float sq_dist(const float* __restrict__ a, const float* __restrict__ b, long long i, int G)
{
    float s = 0.f;
    for (int g = 0; g < G; g++) {
        const float e = a[i * G + g] - b[i * G + g];
        s += e * e;
    }
    return s;
}

/* _compute_reward on [B, G] batches (HER relabelling): kuka_single_step_base_env.py:237-244.
 * HBM-bound: 2*G*4 bytes in, 5 bytes out per item, each touched once -- so every access is non-temporal (streams past
 * the caches).  G == 3 (every single-object task): a workgroup owns 256 quads of 4 items = 3 x 256 float4 per array,
 * read as three fully coalesced float4 sweeps (lane = consecutive 16 bytes) into LDS; thread t then takes the three
 * float4 of ITS quad from LDS (stride 3: conflict-free), computes four rewards and stores one float4 of rewards and one
 * dword of flags, contiguously.  Measured (tools/reward_variants.hip, 64 Mi pairs): 6.1-6.3 TB/s = the float4-copy
 * ceiling of the part (MI355X_MICROARCH.md: 6.29), against 5.0-5.6 for the thread-owns-three-strided-float4 version
 * of rounds 1-2 (with or without non-temporal stores, one or two quads in flight). */
__global__ void __launch_bounds__(256) pmg_k_reward3(const float4* __restrict__ ag, const float4* __restrict__ dg, long long quads,
                                                    float thr, int binary, float4* __restrict__ reward,
                                                    unsigned int* __restrict__ ok)
{
    __shared__ float4 sa[3 * 256], sd[3 * 256];
    const int t = (int)threadIdx.x;
    for (long long base = (long long)blockIdx.x * 256; base < quads; base += (long long)gridDim.x * 256) {
        const long long n = quads - base < 256 ? quads - base : 256;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const long long w = k * 256 + t;
            if (w < 3 * n) { sa[w] = nt::load4(&ag[3 * base + w]); sd[w] = nt::load4(&dg[3 * base + w]); }
        }
        __syncthreads();
        if (t < n) {
            const float4 a0 = sa[3 * t], a1 = sa[3 * t + 1], a2 = sa[3 * t + 2], d0 = sd[3 * t], d1 = sd[3 * t + 1], d2 = sd[3 * t + 2];
            float e[12] = {a0.x - d0.x, a0.y - d0.y, a0.z - d0.z, a0.w - d0.w, a1.x - d1.x, a1.y - d1.y,
                           a1.z - d1.z, a1.w - d1.w, a2.x - d2.x, a2.y - d2.y, a2.z - d2.z, a2.w - d2.w};
            float r[4];
            unsigned int flags = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                unsigned char good;
                r[i] = reward_of(sqrtf(e[3 * i] * e[3 * i] + e[3 * i + 1] * e[3 * i + 1] + e[3 * i + 2] * e[3 * i + 2]), thr, binary, good);
                flags |= (unsigned int)good << (8 * i);
            }
            if (reward) nt::store4(make_float4(r[0], r[1], r[2], r[3]), &reward[base + t]);
            if (ok) nt::store(flags, &ok[base + t]);
        }
        __syncthreads();
    }
}
/* multi-block goals (G = 3 * num_block, up to 19 with the gripper tail): a workgroup owns 256 consecutive items = one
 * contiguous span of 256 * G floats = 64 * G float4 per array WHATEVER G is.  Its threads read that span flat as float4
 * (lane = consecutive 16 bytes: fully coalesced, non-temporal), every load of a thread in flight before the first use,
 * and leave the four squared differences of each float4 in LDS; thread t then adds the G squares of item t (stride G) and
 * stores one reward and one flag, contiguously.  One workgroup per 256 items, no grid-stride below 2^20 workgroups.
 * Measured (tools/reward_flat_variants.hip, 16 Mi pairs, G = 7 / 9 / 12 / 13 / 16 / 19): 6.0-6.1 TB/s at every G against
 * 5.2-5.6 for round 3's kernel (dword loads when G % 4 != 0, loads issued one per loop trip, 8192 workgroups striding);
 * partial sums per float4 when G % 4 == 0 (less LDS traffic) measured 5.9, flags packed into dwords the same as bytes. */
__global__ void __launch_bounds__(256) pmg_k_reward_flat(const float* __restrict__ ag, const float* __restrict__ dg, long long B, int G,
                                                        float thr, int binary, float* __restrict__ reward,
                                                        unsigned char* __restrict__ ok)
{
    constexpr int MAXQ = 5;                                    /* float4 per thread per array: G <= 20 */
    __shared__ float4 sq[MAXQ * 256];
    const int t = (int)threadIdx.x;
    const int q4 = G * 64;                                     /* float4 per array of a full workgroup */
    for (long long base = (long long)blockIdx.x * 256; base + 256 <= B; base += (long long)gridDim.x * 256) {
        const float4* a = (const float4*)(ag + base * G);
        const float4* d = (const float4*)(dg + base * G);
        float4 x[MAXQ], y[MAXQ];
#pragma unroll
        for (int k = 0; k < MAXQ; k++) {
            const int w = t + 256 * k;
            if (w < q4) { x[k] = nt::load4(a + w); y[k] = nt::load4(d + w); }
        }
#pragma unroll
        for (int k = 0; k < MAXQ; k++) {
            const int w = t + 256 * k;
            if (w < q4) {
                const float e0 = x[k].x - y[k].x, e1 = x[k].y - y[k].y, e2 = x[k].z - y[k].z, e3 = x[k].w - y[k].w;
                sq[w] = make_float4(e0 * e0, e1 * e1, e2 * e2, e3 * e3);
            }
        }
        __syncthreads();
        const float* part = (const float*)sq + t * G;
        float s = 0.f;
        for (int k = 0; k < G; k++) s += part[k];
        unsigned char good;
        const float r = reward_of(sqrtf(s), thr, binary, good);
        if (reward) reward[base + t] = r;
        if (ok) ok[base + t] = good;
        __syncthreads();
    }
}
/* any G, and the < 4 tail items of the G == 3 path */
__global__ void __launch_bounds__(256) pmg_k_reward(const float* __restrict__ ag, const float* __restrict__ dg, long long first,
                                                   long long B, int G, float thr, int binary, float* __restrict__ reward,
                                                   unsigned char* __restrict__ ok)
{
    long long i = first + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    unsigned char good;
    const float r = reward_of(sqrtf(sq_dist(ag, dg, i, G)), thr, binary, good);
    if (reward) reward[i] = r;
    if (ok) ok[i] = good;
}
hipError_t pmg_launch_reward(const float* ag, const float* dg, long long B, int G, float thr, int binary, float* reward,
                             unsigned char* ok, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    long long first = 0;
    bool aligned = ((((size_t)ag | (size_t)dg | (size_t)reward) & 15) == 0) && (((size_t)ok & 3) == 0);
    if (G == 3 && aligned && B >= 4) {
        long long quads = B / 4;
        long long want = (quads + 255) / 256;
        unsigned grid = (unsigned)(want < 65536 ? want : 65536); /* a workgroup per 256 quads (measured best), grid-stride beyond 64 Mi items */
        hipLaunchKernelGGL(pmg_k_reward3, dim3(grid), dim3(256), 0, s, (const float4*)ag, (const float4*)dg, quads, thr, binary,
                           (float4*)reward, (unsigned int*)ok);
        first = quads * 4;
    }
    static const int generic_only = getenv("PMG_REWARD_GENERIC") ? atoi(getenv("PMG_REWARD_GENERIC")) : 0;   /* (counter calibration: the dword kernel) */
    if (G > 3 && G <= 20 && B >= 256 && ((((size_t)ag | (size_t)dg) & 15) == 0) && !generic_only) {
        long long want = B / 256;                                /* full workgroups; the < 256 tail items go to pmg_k_reward */
        unsigned grid = (unsigned)(want < (1 << 20) ? want : (1 << 20));
        hipLaunchKernelGGL(pmg_k_reward_flat, dim3(grid), dim3(256), 0, s, ag, dg, B, G, thr, binary, reward, ok);
        first = want * 256;
    }
    if (first < B) {
        unsigned grid = (unsigned)((B - first + 255) / 256);
        hipLaunchKernelGGL(pmg_k_reward, dim3(grid), dim3(256), 0, s, ag, dg, first, B, G, thr, binary, reward, ok);
    }
    return hipGetLastError();
}

/* Running normaliser of HER learners (DESIGN.md 3.7): per column S = sum x', Q = sum x'^2 of the input-clipped rows and the row
 * count n, in double.  The order of every addition is a function of (B, D, row0) alone -- no atomics: workgroup w owns the
 * rows of chunk w (chunks are cut at multiples of `chunk` in GLOBAL row indices, `lead` = row0 % chunk), thread (j, c) adds
 * rows j, j + J, ... of column c in ascending order (W = the power of two >= D columns side by side, J = 256 / W rows),
 * an LDS tree folds the J row slots, and pmg_k_norm_merge adds the partial rows in index order.  Rows are read in place:
 * any row stride, any alignment (dword loads; the goal columns of a reach packed row start at float 9). */
__global__ void __launch_bounds__(256) pmg_k_norm_partial(const float* __restrict__ rows, long long stride, long long B, int D, int W,
                                                         long long chunk, long long lead, const unsigned char* __restrict__ mask,
                                                         float clip, double* __restrict__ part)
{
    __shared__ double ss[256], sq[256], sc[256];
    const int t = (int)threadIdx.x, c = t & (W - 1), j = t / W, J = 256 / W;
    long long r0 = (long long)blockIdx.x * chunk - lead, r1 = r0 + chunk;
    if (r0 < 0) r0 = 0;
    if (r1 > B) r1 = B;
    double s = 0.0, q = 0.0, n = 0.0;
    if (c < D)
        for (long long r = r0 + j; r < r1; r += J) {
            if (mask != nullptr && mask[r] == 0) continue;
            const float x = fminf(fmaxf(nt::load(rows + r * stride + c), -clip), clip);
            const double d = (double)x;
            s += d; q += d * d; n += 1.0;
        }
    ss[t] = s; sq[t] = q; sc[t] = n;
    __syncthreads();
    for (int h = J >> 1; h >= 1; h >>= 1) {
        if (j < h) { ss[t] += ss[t + h * W]; sq[t] += sq[t + h * W]; sc[t] += sc[t + h * W]; }
        __syncthreads();
    }
    if (j == 0 && c < D) {
        double* p = part + (size_t)blockIdx.x * (2 * D + 1);
        p[c] = ss[t]; p[D + c] = sq[t];
        if (c == 0) p[2 * D] = sc[t];
    }
}
/* one workgroup: partial rows added in index order, then to the totals; mean | std | inv_std re-derived from the totals
 * (nparts == 0: only that -- pmg_norm_configure, pmg_norm_write) */
__global__ void __launch_bounds__(256) pmg_k_norm_merge(const double* __restrict__ part, int nparts, int D, double* __restrict__ tot,
                                                       float* __restrict__ der, float eps)
{
    __shared__ double sn;
    const int t = (int)threadIdx.x, P = 2 * D + 1;
    if (t == 0) {
        double a = 0.0;
        for (int p = 0; p < nparts; p++) a += part[(size_t)p * P + 2 * D];
        sn = tot[2 * D] + a;
        tot[2 * D] = sn;
    }
    __syncthreads();
    const double n = sn, e2 = (double)eps * (double)eps;
    for (int c = t; c < D; c += 256) {
        double s = 0.0, q = 0.0;
        for (int p = 0; p < nparts; p++) { s += part[(size_t)p * P + c]; q += part[(size_t)p * P + D + c]; }
        s = tot[c] + s; q = tot[D + c] + q;
        tot[c] = s; tot[D + c] = q;
        float mean = 0.f, sd = 1.f, inv = 1.f;
        if (n > 0.0) {
            const double m = s / n;
            double var = q / n - m * m;
            if (!(var > e2)) var = e2;
            const double r = sqrt(var);
            mean = (float)m; sd = (float)r; inv = (float)(1.0 / r);
        }
        der[c] = mean; der[D + c] = sd; der[2 * D + c] = inv;
    }
}
static long long norm_chunk(long long B)
{
    /* at most PMG_NORM_MAX_PARTS - 2 chunks of a multiple of PMG_NORM_CHUNK_MIN rows (+ 1 for a leading partial chunk) */
    const long long per = (long long)PMG_NORM_CHUNK_MIN * (PMG_NORM_MAX_PARTS - 2);
    return PMG_NORM_CHUNK_MIN * ((B + per - 1) / per);
}
hipError_t pmg_launch_norm_derive(int D, float eps, double* tot, float* der, hipStream_t s)
{
    hipLaunchKernelGGL(pmg_k_norm_merge, dim3(1), dim3(256), 0, s, (const double*)nullptr, 0, D, tot, der, eps);
    return hipGetLastError();
}
hipError_t pmg_launch_norm_update(const float* d_rows, long long row_stride, long long B, int D, long long row0,
                                  const unsigned char* d_mask, float clip_input, float eps, double* part, double* tot,
                                  float* der, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    int W = 1;
    while (W < D) W <<= 1;
    const long long chunk = norm_chunk(B), lead = row0 % chunk;
    const int nparts = (int)((lead + B + chunk - 1) / chunk);   /* <= PMG_NORM_MAX_PARTS */
    hipLaunchKernelGGL(pmg_k_norm_partial, dim3(nparts), dim3(256), 0, s, d_rows, row_stride, B, D, W, chunk, lead, d_mask, clip_input, part);
    hipLaunchKernelGGL(pmg_k_norm_merge, dim3(1), dim3(256), 0, s, (const double*)part, nparts, D, tot, der, eps);
    return hipGetLastError();
}
/* the two halves on their own, for an update whose partial rows cross ranks between them (pmg_norm_update_ranks_device, DESIGN.md 3.17): the
 * caller supplies the chunk -- that of the GLOBAL batch -- and merges the gathered rows of all ranks */
long long pmg_norm_chunk(long long B) { return norm_chunk(B); }
hipError_t pmg_launch_norm_partial(const float* d_rows, long long row_stride, long long B, int D, long long chunk, long long lead, int nparts,
                                   const unsigned char* d_mask, float clip_input, double* part, hipStream_t s)
{
    int W = 1;
    while (W < D) W <<= 1;
    hipLaunchKernelGGL(pmg_k_norm_partial, dim3(nparts), dim3(256), 0, s, d_rows, row_stride, B, D, W, chunk, lead, d_mask, clip_input, part);
    return hipGetLastError();
}
hipError_t pmg_launch_norm_merge(const double* part, int nparts, int D, float eps, double* tot, float* der, hipStream_t s)
{
    hipLaunchKernelGGL(pmg_k_norm_merge, dim3(1), dim3(256), 0, s, part, nparts, D, tot, der, eps);
    return hipGetLastError();
}

/* Policy-input rows out[B, Ds + Dg] = clip((clip(v, clip_in) - mean) * inv_std, clip_out) of state | goal rows.  HBM-bound like the
 * reward kernels above: 4 bytes in and 4 bytes out per element, each touched once.  flat_sweep: an output is ONE flat stream of
 * B (Ds + Dg) floats: thread i of the sweep writes its float4 i (lane = consecutive 16 bytes, whatever the row width; non-temporal)
 * and gathers the four inputs by (row, column), which it keeps as counters: one 64-bit division per thread, none per element.
 * Inputs are read as dwords: rows come with any stride and alignment (in place from the packed rows).  mean / inv_std of the
 * Ds + Dg columns sit in LDS.  The < 4 floats in front of the first 16-byte boundary of the output and behind the last full
 * float4 are written as dwords by workgroup 0.  The sweep is written once, over a ROW SOURCE Src of N = 1 or 2 output streams that
 * share their distance to a 16-byte boundary: row(r) = the source pointers of output row r; fetch(row, col, f, v): v[n] =
 * f(element col of that row, col) for every live stream n; live(n), out(n) = whether and where stream n is written. */
__device__ __forceinline__ unsigned int norm_bits(float f) { unsigned int u; __builtin_memcpy(&u, &f, 4); return u; }
/* the one definition of a policy-input element (pmg_k_policy_input and pmg_k_her_rows: bit-equal by construction) */
__device__ __forceinline__ float policy_norm(float v, float mean, float inv_std, float cin, float cout)
{
    v = fminf(fmaxf(v, -cin), cin);
    v = (v - mean) * inv_std;
    return fminf(fmaxf(v, -cout), cout);
}
/* what a row source applies to every element it fetches: the policy-input element of column col, or (raw) the value itself */
struct PolicyCols {
    const float* mean; const float* inv_std; float cin, cout; bool raw;
    __device__ __forceinline__ float operator()(float v, int col) const { return raw ? v : policy_norm(v, mean[col], inv_std[col], cin, cout); }
};
/* the flat stream of B rows of W floats at `out`: head floats (< 4) up to the first 16-byte boundary, n4 float4, total floats; its grid */
struct FlatSpan { long long head, n4, total; unsigned grid; };
static FlatSpan flat_span(const float* out, long long B, int W)
{
    const long long total = B * W, lead = (long long)(((16 - ((size_t)out & 15)) & 15) / 4), head = lead < total ? lead : total;
    const long long n4 = (total - head) / 4, want = (n4 + 255) / 256;
    /* 2048 workgroups of four wavefronts fill the 256 compute units (8 wavefronts per SIMD); larger batches stride */
    return {head, n4, total, (unsigned)(want < 1 ? 1 : (want < 2048 ? want : 2048))};
}
template <class Src>
__device__ __forceinline__ void flat_sweep(const Src& S, const float* __restrict__ ders, int Ds, const float* __restrict__ derg, int Dg,
                                           bool raw, float cin, float cout, const FlatSpan& F)
{
    constexpr int N = Src::N;
    __shared__ float sm[2 * PMG_NORM_MAX_D], si[2 * PMG_NORM_MAX_D];
    const int W = Ds + Dg, t = (int)threadIdx.x;
    if (!raw) {
        for (int c = t; c < W; c += 256) {
            sm[c] = c < Ds ? ders[c] : derg[c - Ds];
            si[c] = c < Ds ? ders[2 * Ds + c] : derg[2 * Dg + (c - Ds)];
        }
        __syncthreads();
    }
    const PolicyCols f = {sm, si, cin, cout, raw};
    const long long head = F.head, n4 = F.n4;
    const long long sweep = (long long)gridDim.x * 256;        /* float4 per sweep of the grid */
    long long i = (long long)blockIdx.x * 256 + t;
    if (i < n4) {
        const long long e = head + 4 * i;
        long long row = e / W;
        int col = (int)(e - row * W);
        const long long drow = (4 * sweep) / W;
        const int dcol = (int)(4 * sweep - drow * W);
        for (; i < n4; i += sweep) {
            float v[4][N];
            long long rr = row;
            int cc = col;
            typename Src::Row src = S.row(rr);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                S.fetch(src, cc, f, v[k]);
                if (++cc == W) { cc = 0; rr++; if (k < 3) src = S.row(rr); }   /* k < 3: element e + k + 1 < total, so rr < B */
            }
            if (S.live(0)) nt::store4(make_float4(v[0][0], v[1][0], v[2][0], v[3][0]), (float4*)(S.out(0) + head) + i);
            if (N == 2 && S.live(1)) nt::store4(make_float4(v[0][N - 1], v[1][N - 1], v[2][N - 1], v[3][N - 1]), (float4*)(S.out(1) + head) + i);
            row += drow; col += dcol;
            if (col >= W) { col -= W; row++; }
        }
    }
    if (blockIdx.x == 0) {
        const long long body_end = head + 4 * n4;
        const int extra = (int)(head + (F.total - body_end));   /* < 8 */
        if (t < extra) {
            const long long e = t < head ? (long long)t : body_end + (t - head);
            const long long row = e / W;
            float v[N] = {};
            S.fetch(S.row(row), (int)(e - row * W), f, v);
            if (S.live(0)) nt::store(norm_bits(v[0]), (unsigned int*)(S.out(0) + e));
            if (N == 2 && S.live(1)) nt::store(norm_bits(v[N - 1]), (unsigned int*)(S.out(1) + e));
        }
    }
}
/* row r of state | goal at the given strides; every input is touched once: non-temporal loads.  A row is its index: the address
 * is formed per element, so the row hand-over of the sweep is a select, not a branch (W = 10: four float4 in ten hand over) */
struct StridedRows {
    static constexpr int N = 1;
    typedef long long Row;
    const float* __restrict__ s; long long ss; const float* __restrict__ g; long long gs; int Ds; float* __restrict__ o;
    __device__ __forceinline__ Row row(long long r) const { return r; }
    __device__ __forceinline__ void fetch(Row r, int col, const PolicyCols& f, float* v) const
    {
        v[0] = f(nt::load(col < Ds ? s + r * ss + col : g + r * gs + (col - Ds)), col);
    }
    __device__ __forceinline__ bool live(int) const { return true; }
    __device__ __forceinline__ float* out(int) const { return o; }
};
__global__ void __launch_bounds__(256) pmg_k_policy_input(StridedRows S, int Dg, const float* __restrict__ ders, const float* __restrict__ derg,
                                                         float cin, float cout, FlatSpan F)
{
    flat_sweep(S, ders, S.Ds, derg, Dg, false, cin, cout, F);
}
hipError_t pmg_launch_policy_input(const float* d_state, long long state_stride, int Ds, const float* d_goal, long long goal_stride,
                                   int Dg, long long B, const float* der_state, const float* der_goal, float clip_input,
                                   float clip_output, float* d_out, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    const FlatSpan F = flat_span(d_out, B, Ds + Dg);
    const StridedRows S = {d_state, state_stride, d_goal, goal_stride, Ds, d_out};
    hipLaunchKernelGGL(pmg_k_policy_input, dim3(F.grid), dim3(256), 0, s, S, Dg, der_state, der_goal, clip_input, clip_output, F);
    return hipGetLastError();
}

/* HER minibatches from episode rows the caller keeps in device memory (pmg_her_sample_device, DESIGN.md 3.8).
 * The draws (include/pmg.h): SplitMix64's finaliser over a counter, four 32-bit values per sample; multiply-shift
 * maps them onto [0, E), [0, T) and (t, T], so no address depends on device data. */
constexpr unsigned long long HER_GOLD = 0x9E3779B97F4A7C15ull;
__host__ __device__ __forceinline__ unsigned long long her_mix(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
/* One thread per sample: the four draws -> e, t, f (idx; -1 = not relabelled), reward and flag of (achieved_goal(e, t + 1), g')
 * from the 2 G goal floats, and the action row.  A lane per sample touches 64 different rows per wave-instruction -- the
 * slow shape -- but only for these 2 G + A floats of a sample; the row sweep below carries the bulk.  Distance and reward
 * are pmg_k_reward's: sq_dist and reward_of. */
__global__ void __launch_bounds__(256) pmg_k_her_draw(PmgHer H, unsigned long long key)
{
    for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < H.B; b += (long long)gridDim.x * 256) {
        const unsigned long long z = key + (4ull * (unsigned long long)b + 1ull) * HER_GOLD;
        const unsigned long long r0 = her_mix(z) >> 32, r1 = her_mix(z + HER_GOLD) >> 32, r2 = her_mix(z + 2ull * HER_GOLD) >> 32,
                                 r3 = her_mix(z + 3ull * HER_GOLD) >> 32;
        const int e = (int)((r0 * (unsigned long long)H.E) >> 32);
        const int t = (int)((r1 * (unsigned long long)H.T) >> 32);
        const int f = r2 < H.relabel_below ? t + 1 + (int)((r3 * (unsigned long long)(H.T - t)) >> 32) : -1;
        if (H.idx) { int* ix = H.idx + 3 * b; ix[0] = e; ix[1] = t; ix[2] = f; }   /* re-read by the sweep: plain stores */
        if (H.reward || H.ok) {
            const float* row = H.rows + (long long)e * H.res + (long long)t * H.rts;
            const float* g = f >= 0 ? H.rows + (long long)e * H.res + (long long)f * H.rts + H.ago : row + H.dgo;
            unsigned char good;
            const float r = reward_of(sqrtf(sq_dist(row + H.rts + H.ago, g, 0, H.G)), H.thr, H.binary, good);
            if (H.reward) nt::store(norm_bits(r), (unsigned int*)(H.reward + b));
            if (H.ok) H.ok[b] = good;
        }
        if (H.action) {
            const float* a = H.act + (long long)e * H.aes + (long long)t * H.ats;
            for (int k = 0; k < H.A; k++) nt::store(norm_bits(a[k]), (unsigned int*)(H.action + b * H.A + k));
        }
    }
}
/* sample b of a HER batch: (e, t, f) from idx -> state(e, t), state(e, t + 1), g'.  Two streams, x[B, Ds + G] = state(e, t) | g'
 * and xn = state(e, t + 1) | g': mode 2 fills both in one sweep and fetches g' once per sample, mode 0 / 1 fill x / xn alone.
 * Plain loads: a replay table is read again. */
struct HerRows {
    static constexpr int N = 2;
    struct Row { const float* s; const float* sn; const float* g; };
    PmgHer H; int mode;
    __device__ __forceinline__ Row row(long long b) const
    {
        const int* ix = H.idx + 3 * b;
        const int e = ix[0], t = ix[1], f = ix[2];
        const float* r = H.rows + (long long)e * H.res + (long long)t * H.rts;
        const float* s = r + H.so;
        const long long go = f >= 0 ? (long long)(f - t) * H.rts + H.ago : (long long)H.dgo;   /* g' from row (e, t) */
        return {s, s + H.rts, r + go};
    }
    __device__ __forceinline__ void fetch(const Row& r, int col, const PolicyCols& f, float* v) const
    {
        if (col >= H.Ds) { v[0] = v[1] = f(r.g[col - H.Ds], col); return; }
        if (mode != 1) v[0] = f(r.s[col], col);
        if (mode != 0) v[1] = f(r.sn[col], col);
    }
    __device__ __forceinline__ bool live(int n) const { return mode != 1 - n; }
    __device__ __forceinline__ float* out(int n) const { return n ? H.xn : H.x; }
};
__global__ void __launch_bounds__(256) pmg_k_her_rows(HerRows S, FlatSpan F)
{
    flat_sweep(S, S.H.der_state, S.H.Ds, S.H.der_goal, S.H.G, S.H.raw != 0, S.H.cin, S.H.cout, F);
}
static void launch_her_rows(const PmgHer& H, int mode, hipStream_t s)
{
    const FlatSpan F = flat_span(mode == 1 ? H.xn : H.x, H.B, H.Ds + H.G);
    const HerRows S = {H, mode};
    hipLaunchKernelGGL(pmg_k_her_rows, dim3(F.grid), dim3(256), 0, s, S, F);
}
hipError_t pmg_launch_her(const PmgHer& H, hipStream_t s)
{
    if (H.B <= 0) return hipSuccess;
    const unsigned long long key = her_mix(H.seed ^ her_mix(H.counter + HER_GOLD));
    const long long want = (H.B + 255) / 256;
    hipLaunchKernelGGL(pmg_k_her_draw, dim3((unsigned)(want < (1 << 20) ? want : (1 << 20))), dim3(256), 0, s, H, key);
    /* x and x_next share a launch iff they share their distance to a 16-byte boundary */
    if (H.x && H.xn && (((size_t)H.x ^ (size_t)H.xn) & 15) == 0) launch_her_rows(H, 2, s);
    else {
        if (H.x) launch_her_rows(H, 0, s);
        if (H.xn) launch_her_rows(H, 1, s);
    }
    return hipGetLastError();
}

/* Actor forward on the device (pmg_mlp_forward_device, pmg_act_env_device; DESIGN.md 3.9): a multi-layer perceptron of up to four
 * layers of up to 256 units on rows of floats, and for the act entry the exploration epilogue.  A workgroup owns MLP_ROWS = 32
 * rows and runs ALL layers on them: the activations stay in LDS, wavefront w owns the 32-unit strips w and w + 4 of a layer and
 * keeps their 32 x 32 results in registers (2 x 16) across the barrier behind which the tile is overwritten -- one buffer.  The last
 * layer leaves z there too, and a thread per (row, unit) writes the outputs.
 * Arithmetic (normative): unit j of a row is ONE float32 chain acc = bias[j]; acc = fmaf(h[k], W[j][k], acc), k ascending; the
 * f32-input MFMA is bit for bit that chain (two k per instruction, lower k first).  K odd: the last step multiplies a zero the
 * tile holds in column K by a zero that stands in for W[j][K]; the lanes of units beyond the layer's width run on row 0 of W and
 * their results are dropped.
 * B operand: read as dwords straight from the caller's [out, in] row-major weights, lane (unit, k parity) walking ITS row.  With 32
 * rows per workgroup = M of the instruction every weight is used by exactly one lane of one wavefront once, so staging through
 * LDS would add a write and a read per element and save none; a lane's 128-byte line serves its next 15 steps from L1. */
constexpr int MLP_ROWS = 32;             /* rows of a workgroup's tile = M of the matrix step */
constexpr int MLP_MAXW = 256;            /* widest layer */
constexpr int MLP_LD = MLP_MAXW + 2;     /* floats from row to row of the tile: = 2 (mod 64), the 32 rows x 2 k of an A read hit 64 banks */
#ifdef PMG_EMULATE
struct MlpAcc { float v[16]; float& operator[](int i) { return v[i]; } float operator[](int i) const { return v[i]; } };
#else
typedef float MlpAcc __attribute__((ext_vector_type(16)));
#endif
/* C/D map of the 32 x 32 tile: lane l holds column l & 31, register reg of it is this row */
__device__ __forceinline__ int mlp_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }
/* v, or +0.0 where keep is false, without a select: a select fed by a load becomes a branch around the load, and the loop then
 * waits for every load on its own */
__device__ __forceinline__ float mlp_keep(float v, bool keep)
{
    unsigned int u;
    __builtin_memcpy(&u, &v, 4);
    u &= keep ? 0xffffffffu : 0u;
    __builtin_memcpy(&v, &u, 4);
    return v;
}
/* THE matrix step, k0 even: acc[row][unit] = fmaf(tile[row][k0 + 1], W[unit][k0 + 1], fmaf(tile[row][k0], W[unit][k0], acc[row][unit]))
 * for the 32 rows of the tile and the 32 units of a strip; wrow = row of W of THIS lane's unit (lane & 31).  TAIL: the last step
 * of an odd K, k0 = K - 1: column K of the tile holds zeros and +0.0 stands in for W[unit][K].  Device: v_mfma_f32_32x32x2_f32,
 * A = tile[l & 31][k0 + (l >> 5)], B = W[unit l & 31][k0 + (l >> 5)].  Emulator: the same tile as fmaf over the lane's own 16
 * results, A and B read where the device body reads them (no lane exchange). */
template <bool TAIL>
__device__ __forceinline__ void mlp_mma(const float* tile, const float* __restrict__ wrow, int k0, int lane, MlpAcc& acc)
{
#ifndef PMG_EMULATE
    const int h = lane >> 5;
    const float a = tile[(lane & 31) * MLP_LD + k0 + h];
    const float b = TAIL ? mlp_keep(wrow[k0], h == 0) : wrow[k0 + h];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
#else
    for (int reg = 0; reg < 16; reg++) {
        const float* a = tile + mlp_row(reg, lane) * MLP_LD + k0;
        acc[reg] = fmaf(a[1], TAIL ? 0.f : wrow[k0 + 1], fmaf(a[0], wrow[k0], acc[reg]));
    }
#endif
}
/* all K steps of a layer for the NS = 1 or 2 strips of a wavefront, which share the A operand.  Eight steps are written out: their
 * 8 NS weight loads are in flight together (the optimizer does not unroll this loop at a run-time trip count on request) */
template <int NS>
__device__ __forceinline__ void mlp_chain(const float* tile, const float* __restrict__ w0, const float* __restrict__ w1, int K, int lane,
                                          MlpAcc& acc0, MlpAcc& acc1)
{
    const int K16 = K & ~15, Ke = K & ~1;
    for (int k0 = 0; k0 < K16; k0 += 16) {
#pragma unroll
        for (int u = 0; u < 16; u += 2) {
            mlp_mma<false>(tile, w0, k0 + u, lane, acc0);
            if (NS == 2) mlp_mma<false>(tile, w1, k0 + u, lane, acc1);
        }
    }
    for (int k0 = K16; k0 < Ke; k0 += 2) {
        mlp_mma<false>(tile, w0, k0, lane, acc0);
        if (NS == 2) mlp_mma<false>(tile, w1, k0, lane, acc1);
    }
    if (K & 1) {
        mlp_mma<true>(tile, w0, Ke, lane, acc0);
        if (NS == 2) mlp_mma<true>(tile, w1, Ke, lane, acc1);
    }
}
/* the row sources: at(r, col) = element col of input row r */
struct MlpRawRows {
    const float* __restrict__ in; long long stride;
    __device__ __forceinline__ float at(long long r, int col) const { return in[r * stride + col]; }
};
/* state | desired_goal columns of packed rows through policy_norm: the row pmg_k_policy_input writes, element by element */
struct MlpEnvRows {
    PmgMlpEnv E;
    __device__ __forceinline__ float at(long long r, int col) const
    {
        const bool st = col < E.Ds;
        const int c = st ? col : col - E.Ds, D = st ? E.Ds : E.Dg;
        const float* __restrict__ der = st ? E.der_state : E.der_goal;
        return policy_norm(E.rows[r * E.stride + (st ? E.so : E.dgo) + c], der[c], der[2 * D + c], E.cin, E.cout);
    }
};
/* the row x[r] | a[r] of two tables read in place (pmg_q_device): columns below Dx from x, the others from a */
struct MlpCatRows {
    const float* __restrict__ x; long long xs; const float* __restrict__ a; long long as; int Dx;
    __device__ __forceinline__ float at(long long r, int col) const { return col < Dx ? x[r * xs + col] : a[r * as + (col - Dx)]; }
};
/* pre-activation z -> the action without exploration: clip(out_activation(z)) (mlp_action, and a' of pmg_k_td_target) */
__device__ __forceinline__ float mlp_plain_action(int out_act, float z) { return fminf(fmaxf(out_act ? tanhf(z) : z, -1.f), 1.f); }
/* pre-activation z of column j of global env g -> action (include/pmg.h): HER's generator with b = g A + j as the sample index */
__device__ __forceinline__ float mlp_action(const PmgMlp& M, float z, unsigned long long g, int j, int A)
{
    if (!M.explore) return mlp_plain_action(M.out_act, z);
    float a = M.out_act ? tanhf(z) : z;
    const unsigned long long z0 = M.key + (4ull * (g * (unsigned long long)A) + 1ull) * HER_GOLD;   /* column 0 of the env */
    const unsigned long long zb = z0 + 4ull * (unsigned long long)j * HER_GOLD;
    if (M.noise_eps > 0.f) {
        const unsigned int r0 = (unsigned int)(her_mix(zb) >> 32), r1 = (unsigned int)(her_mix(zb + HER_GOLD) >> 32);
        const float u1 = (float)((r0 >> 8) + 1u) * 0x1p-24f, u2 = (float)(r1 >> 8) * 0x1p-24f;
        a = a + M.noise_eps * sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
    }
    a = fminf(fmaxf(a, -1.f), 1.f);
    if ((her_mix(z0 + 3ull * HER_GOLD) >> 32) < M.random_below) {
        const unsigned int r2 = (unsigned int)(her_mix(zb + 2ull * HER_GOLD) >> 32);
        a = (float)(r2 >> 8) * 0x1p-23f - 1.f;
    }
    return a;
}
/* columns [0, K) of the 32 rows from row0 of a row source into the tile, lanes along the columns; rows past the batch and the columns
 * [K, Kp) (Kp = K rounded up to even: the padding column of an odd K; Kp = K: none) are written as zeros.  Every address is valid
 * (clamped), so the loads of a thread are in flight together */
template <class Src>
__device__ __forceinline__ void mlp_gather(float* tile, const Src& S, long long row0, long long B, int K, int Kp, int t)
{
#pragma unroll 4
    for (int i = t; i < MLP_ROWS * Kp; i += 256) {
        const int r = i / Kp, c = i - r * Kp;
        const bool in = row0 + r < B && c < K;
        tile[r * MLP_LD + c] = mlp_keep(S.at(row0 + r < B ? row0 + r : B - 1, c < K ? c : K - 1), in);
    }
}
/* THE layer loop (every instantiation of pmg_k_mlp and both networks of pmg_k_td_target): all layers of M on the tile, whose columns
 * [0, width[0] rounded up to even) hold the input and real zeros as padding; behind the closing barrier columns [0, width[L]) hold z */
__device__ __forceinline__ void mlp_layers(float* tile, const PmgMlp& M, int lane, int wave, int col)
{
#pragma unroll 1
    for (int l = 0; l < M.L; l++) {
        const int K = M.width[l], Nn = M.width[l + 1];
        const float* __restrict__ W = M.w[l];
        const float* __restrict__ bias = M.b[l];
        const int u0 = 32 * wave + col, u1 = u0 + 128;            /* this lane's unit in the strips wave and wave + 4 */
        const bool live0 = u0 < Nn, live1 = u1 < Nn, strip0 = 32 * wave < Nn, strip1 = 32 * wave + 128 < Nn;
        /* a unit past the width runs on row 0 of W: valid addresses, results never used */
        const float* w0 = W + (long long)(live0 ? u0 : 0) * K;
        const float* w1 = W + (long long)(live1 ? u1 : 0) * K;
        const float b0 = bias ? bias[live0 ? u0 : 0] : 0.f, b1 = bias ? bias[live1 ? u1 : 0] : 0.f;
        MlpAcc acc0, acc1;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) { acc0[reg] = b0; acc1[reg] = b1; }
        if (strip1) mlp_chain<2>(tile, w0, w1, K, lane, acc0, acc1);
        else if (strip0) mlp_chain<1>(tile, w0, w1, K, lane, acc0, acc1);
        const bool hidden = l + 1 < M.L;
        __syncthreads();                                         /* every wavefront has read the layer's input */
        /* whole strips: a unit past the width becomes +0.0, the next layer's padding */
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            if (strip0) tile[mlp_row(reg, lane) * MLP_LD + u0] = live0 ? (hidden ? fmaxf(acc0[reg], 0.f) : acc0[reg]) : 0.f;
            if (strip1) tile[mlp_row(reg, lane) * MLP_LD + u1] = live1 ? (hidden ? fmaxf(acc1[reg], 0.f) : acc1[reg]) : 0.f;
        }
        __syncthreads();
    }
}
template <class Src, bool ACT>
__global__ void __launch_bounds__(256) pmg_k_mlp(Src S, PmgMlp M)
{
    __shared__ float tile[MLP_ROWS * MLP_LD];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31;
    const long long ntiles = (M.B + MLP_ROWS - 1) / MLP_ROWS;
    for (long long tb = blockIdx.x; tb < ntiles; tb += gridDim.x) {
        const long long row0 = tb * MLP_ROWS;
        mlp_gather(tile, S, row0, M.B, M.width[0], (M.width[0] + 1) & ~1, t);
        __syncthreads();
        mlp_layers(tile, M, lane, wave, col);
        {   /* the tile holds z: thread per (row, unit), units along the lanes */
            const int A = M.width[M.L];
            for (int i = t; i < MLP_ROWS * A; i += 256) {
                const int r = i / A, j = i - r * A;
                const long long row = row0 + r;
                if (row >= M.B) break;
                const float z = tile[r * MLP_LD + j];
                if (ACT) {
                    if (M.out) M.out[row * M.out_stride + j] = z;
                    M.actions[row * A + j] = mlp_action(M, z, (unsigned long long)(M.env0 + row), j, A);
                } else
                    M.out[row * M.out_stride + j] = M.out_act ? tanhf(z) : z;
            }
        }
        __syncthreads();                                             /* the next tile's rows overwrite this one's */
    }
}
/* TD target of DDPG / HER (pmg_td_target_device, DESIGN.md 3.10): y = clip(r + gamma Q'(x', pi'(x'))), both networks on ONE tile.  After the
 * actor's layers z sits in columns [0, A); a' = mlp_plain_action(z) moves to columns [Dx, Dx + A), the critic's action columns.  Source and
 * target overlap when A > Dx, so a thread per (row, unit) carries its value in a register across a barrier, eight units of all 32 rows per
 * pass, the units in DESCENDING order: a pass writes only columns above every column a later pass reads.  Then columns [0, Dx) are
 * gathered again from x' (layer 0 of the actor overwrote them; L2-resident) and column Dx + A of an odd Dx + A becomes +0.0.  Every
 * column the critic's layer 0 reads is thereby written for all 32 rows behind the actor -- rows past the batch as zeros --, so no stale
 * hidden activation (which may be inf) meets a padding zero.  A thread per row forms y from the critic's single output column. */
__global__ void __launch_bounds__(256) pmg_k_td_target(PmgMlp P, PmgMlp Q, PmgTd T)
{
    __shared__ float tile[MLP_ROWS * MLP_LD];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31;
    const int Dx = P.width[0], A = P.width[P.L];
    const MlpRawRows S = {T.xn, T.xs};
    const long long ntiles = (P.B + MLP_ROWS - 1) / MLP_ROWS;
    for (long long tb = blockIdx.x; tb < ntiles; tb += gridDim.x) {
        const long long row0 = tb * MLP_ROWS;
        mlp_gather(tile, S, row0, P.B, Dx, (Dx + 1) & ~1, t);
        __syncthreads();
        mlp_layers(tile, P, lane, wave, col);
        {
            const int r = t >> 3;
            const long long row = row0 + r;
            for (int hi = A; hi > 0; hi -= 8) {
                const int j = hi - 8 + (t & 7);                      /* units [hi - 8, hi) of the 32 rows */
                const float z = j >= 0 ? tile[r * MLP_LD + j] : 0.f;
                __syncthreads();                                     /* the pass has read its z: columns [Dx + hi - 8, Dx + hi) are free */
                if (j >= 0) {
                    const float a = mlp_plain_action(P.out_act, z);
                    tile[r * MLP_LD + Dx + j] = row < P.B ? a : 0.f;
                    if (T.na && row < P.B) T.na[row * A + j] = a;
                }
            }
        }
        mlp_gather(tile, S, row0, P.B, Dx, Dx, t);                   /* columns below Dx: no pass wrote them, every pass is done reading */
        if ((Dx + A) & 1) { if (t < MLP_ROWS) tile[t * MLP_LD + Dx + A] = 0.f; }
        __syncthreads();
        mlp_layers(tile, Q, lane, wave, col);
        if (t < MLP_ROWS && row0 + t < P.B) {
            const long long row = row0 + t;
            const float z = tile[t * MLP_LD], q = Q.out_act ? tanhf(z) : z, r = T.reward[row];
            const float v = T.term && T.term[row] ? r : fmaf(T.gamma, q, r);
            T.y[row] = fminf(fmaxf(v, T.lo), T.hi);
            if (T.qn) T.qn[row] = q;
        }
        __syncthreads();                                             /* the next tile's rows overwrite this one's */
    }
}
/* TD3's target (pmg_td3_target_device, DESIGN.md 3.14), pmg_k_td_target's sibling on the same tile: y = clip(r + gamma min(Q1', Q2')(x', a~)),
 * a~ = clip(a' + clip(sigma n, -c, c), -1, 1).  The actor, the descending hand-over, the regather of x' and critic 1 run as there; the noise is
 * added inside the hand-over pass by the thread that owns (row, unit), which also writes a~ to X.keep (the caller's d_next_action, or the
 * workspace).  Critic 1's layers overwrite the whole tile, so for critic 2 the row x' | a~ is built again: x' from memory, a~ from X.keep by
 * the SAME (row, unit) -> thread map as the hand-over -- a thread reads only its own earlier store, so no ordering between threads is
 * involved (the argument of pmg_k_policy_grad_rows for its stash of o).  q1 waits in a register of the row's thread (t < 32) meanwhile.
 * Stale tile between the critics: when the restore starts, the tile holds critic 1's activations (which may be inf) in columns up to its
 * widest layer.  The regather writes columns [0, Dx) of all 32 rows, the restore passes columns [Dx, Dx + A) of all 32 rows, thread t < 32
 * column Dx + A of an odd Dx + A; rows past the batch receive +0.0 in each.  These are all the columns critic 2's layer 0 reads (K = Dx + A,
 * and the padding column of an odd K), so no stale activation meets a weight or a stand-in zero.  Nothing in the restore READS the tile,
 * so its passes need no barrier between them; the barrier in front of it orders the read of q1 (column 0) before the regather's writes. */
/* the smoothing term e of sample index s = (row_offset + row) * A + j: mlp_action's expression with sigma for noise_eps, clipped to [-c, c] */
__device__ __forceinline__ float td3_noise(const PmgTd3& X, unsigned long long s)
{
    const unsigned long long zb = X.key + (4ull * s + 1ull) * HER_GOLD;
    const unsigned int r0 = (unsigned int)(her_mix(zb) >> 32), r1 = (unsigned int)(her_mix(zb + HER_GOLD) >> 32);
    const float u1 = (float)((r0 >> 8) + 1u) * 0x1p-24f, u2 = (float)(r1 >> 8) * 0x1p-24f;
    return fminf(fmaxf(X.sigma * sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2), -X.c), X.c);
}
__global__ void __launch_bounds__(256) pmg_k_td3_target(PmgMlp P, PmgMlp Q1, PmgMlp Q2, PmgTd3 X)
{
    __shared__ float tile[MLP_ROWS * MLP_LD];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31;
    const int Dx = P.width[0], A = P.width[P.L];
    const MlpRawRows S = {X.T.xn, X.T.xs};
    const int r = t >> 3;                                            /* the row of this thread in the hand-over and in the restore */
    const long long ntiles = (P.B + MLP_ROWS - 1) / MLP_ROWS;
    for (long long tb = blockIdx.x; tb < ntiles; tb += gridDim.x) {
        const long long row0 = tb * MLP_ROWS, row = row0 + r;
        mlp_gather(tile, S, row0, P.B, Dx, (Dx + 1) & ~1, t);
        __syncthreads();
        mlp_layers(tile, P, lane, wave, col);
        for (int hi = A; hi > 0; hi -= 8) {
            const int j = hi - 8 + (t & 7);                          /* units [hi - 8, hi) of the 32 rows */
            const float z = j >= 0 ? tile[r * MLP_LD + j] : 0.f;
            __syncthreads();                                         /* the pass has read its z: columns [Dx + hi - 8, Dx + hi) are free */
            if (j >= 0) {
                float a = 0.f;
                if (row < P.B) {
                    a = mlp_plain_action(P.out_act, z);
                    if (X.noise) a = fminf(fmaxf(a + td3_noise(X, (X.row_offset + (unsigned long long)row) * (unsigned long long)A + (unsigned long long)j), -1.f), 1.f);
                    if (X.keep) X.keep[row * A + j] = a;
                }
                tile[r * MLP_LD + Dx + j] = a;
            }
        }
        mlp_gather(tile, S, row0, P.B, Dx, Dx, t);                   /* columns below Dx: no pass wrote them, every pass is done reading */
        if ((Dx + A) & 1) { if (t < MLP_ROWS) tile[t * MLP_LD + Dx + A] = 0.f; }
        __syncthreads();
        mlp_layers(tile, Q1, lane, wave, col);
        const bool own = t < MLP_ROWS && row0 + t < P.B;             /* this thread forms the outputs of row row0 + t */
        float q = 0.f;
        if (own) {
            const float z = tile[t * MLP_LD];
            q = Q1.out_act ? tanhf(z) : z;
            if (X.q1) X.q1[row0 + t] = q;
        }
        if (X.twin) {
            __syncthreads();                                         /* q1 is read: column 0 is free */
            mlp_gather(tile, S, row0, P.B, Dx, Dx, t);
            for (int hi = A; hi > 0; hi -= 8) {                      /* the hand-over's map: a thread reads what it stored itself */
                const int j = hi - 8 + (t & 7);
                if (j >= 0) tile[r * MLP_LD + Dx + j] = row < P.B ? X.keep[row * A + j] : 0.f;
            }
            if ((Dx + A) & 1) { if (t < MLP_ROWS) tile[t * MLP_LD + Dx + A] = 0.f; }
            __syncthreads();
            mlp_layers(tile, Q2, lane, wave, col);
            if (own) {
                const float z = tile[t * MLP_LD], q2 = Q2.out_act ? tanhf(z) : z;
                if (X.q2) X.q2[row0 + t] = q2;
                q = fminf(q, q2);
            }
        }
        if (own) {
            const float rw = X.T.reward[row0 + t];
            const float v = X.T.term && X.T.term[row0 + t] ? rw : fmaf(X.T.gamma, q, rw);
            X.T.y[row0 + t] = fminf(fmaxf(v, X.T.lo), X.T.hi);
            if (X.T.qn) X.T.qn[row0 + t] = q;
        }
        __syncthreads();                                             /* the next tile's rows overwrite this one's */
    }
}
/* SAC's Gaussian head (include/pmg.h, DESIGN.md 3.15): the ONE definition of (mean, raw log-std, sample index) -> action a = tanh(u), the
 * noise n used and the summand l of log pi, for pmg_k_sac and pmg_k_sac_target, which thereby agree bit for bit.  The draws are
 * td3_noise's; every multiply-add is an fmaf, so the build contracts nothing.  log(1 - tanh^2 u) is taken as 2 (log 2 - u - softplus(-2 u)):
 * no cancellation where |a| rounds to 1. */
struct SacHead { float a, n, l; };
__device__ __forceinline__ SacHead sac_head(const PmgSac& G, float m, float ls_raw, unsigned long long s)
{
    const float ls = fminf(fmaxf(ls_raw, G.ls_lo), G.ls_hi);
    float n = 0.f;
    if (G.sample) {
        const unsigned long long zb = G.key + (4ull * s + 1ull) * HER_GOLD;
        const unsigned int r0 = (unsigned int)(her_mix(zb) >> 32), r1 = (unsigned int)(her_mix(zb + HER_GOLD) >> 32);
        const float u1 = (float)((r0 >> 8) + 1u) * 0x1p-24f, u2 = (float)(r1 >> 8) * 0x1p-24f;
        n = sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
    }
    const float sd = expf(ls), u = fmaf(sd, n, m);
    const float w = -2.f * u, sp = fmaxf(w, 0.f) + log1pf(expf(-fabsf(w)));
    const float c2 = (0.69314718055994530942f - u) - sp;
    SacHead h;
    h.a = tanhf(u);
    h.n = n;
    h.l = fmaf(-2.f, c2, fmaf(-0.5f * n, n, -ls) - 0.91893853320467274178f);
    return h;
}
/* log pi of row r of the tile, whose columns [0, A) hold the summands: ONE chain from +0.0, j ascending, by the row's thread */
__device__ __forceinline__ float sac_logp(const float* tile, int r, int A)
{
    float acc = 0.f;
    for (int j = 0; j < A; j++) acc = acc + tile[r * MLP_LD + j];
    return acc;
}
/* Action, log-probability and noise of a Gaussian actor (pmg_sac_sample_device, pmg_sac_act_env_device), pmg_k_mlp's sibling: gather, the
 * layers, then the head.  The tile holds z: means in columns [0, A), raw log-stds in [A, 2 A).  The thread of (row, unit j < A) in
 * pmg_k_mlp's map reads columns j and A + j of its row, writes the outputs and puts l_j back into column j.  No other thread reads or
 * writes these two columns in the pass (another unit j' of the row touches j' and A + j', and j' != j, A + j' != j as j < A), so the pass
 * needs no barrier inside; the one behind it orders the l_j before the sum of the row's thread, and the closing one that sum before the
 * next tile's gather.  Rows past the batch are left alone: nothing reads them. */
template <class Src>
__global__ void __launch_bounds__(256) pmg_k_sac(Src S, PmgMlp M, PmgSac G)
{
    __shared__ float tile[MLP_ROWS * MLP_LD];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31;
    const int A = M.width[M.L] >> 1;
    const long long ntiles = (M.B + MLP_ROWS - 1) / MLP_ROWS;
    for (long long tb = blockIdx.x; tb < ntiles; tb += gridDim.x) {
        const long long row0 = tb * MLP_ROWS;
        mlp_gather(tile, S, row0, M.B, M.width[0], (M.width[0] + 1) & ~1, t);
        __syncthreads();
        mlp_layers(tile, M, lane, wave, col);
        for (int i = t; i < MLP_ROWS * A; i += 256) {
            const int r = i / A, j = i - r * A;
            const long long row = row0 + r;
            if (row >= M.B) break;
            const float m = tile[r * MLP_LD + j], ls = tile[r * MLP_LD + A + j];
            const SacHead h = sac_head(G, m, ls, (G.row_offset + (unsigned long long)row) * (unsigned long long)A + (unsigned long long)j);
            if (G.preact) { G.preact[row * G.ps + j] = m; G.preact[row * G.ps + A + j] = ls; }
            if (G.action) G.action[row * G.as + j] = h.a;
            if (G.noise) G.noise[row * G.ns + j] = h.n;
            tile[r * MLP_LD + j] = h.l;
        }
        __syncthreads();                                             /* every l_j of the tile is written */
        if (G.logp && t < MLP_ROWS && row0 + t < M.B) G.logp[row0 + t] = sac_logp(tile, t, A);
        __syncthreads();                                             /* the next tile's rows overwrite this one's */
    }
}
/* SAC's soft target (pmg_sac_target_device, DESIGN.md 3.15), pmg_k_td3_target's sibling on the same tile:
 * y = clip(r + gamma (min(Q1, Q2)(x', a') - alpha log pi(a' | x'))), a' and log pi from the head above.
 * Hand-over.  The actor leaves 2 A columns, so the descending eight-unit schedule of the siblings does not carry over: with Dx < A a pass
 * would store an action into a column a later pass still reads as a log-std.  Instead NOTHING is handed over through the tile: the thread
 * of (row, unit) in pmg_k_sac's map writes a' to G.action (the caller's d_next_action, or the workspace) and l_j into its own column j --
 * the only thread that touches columns j and A + j of that row in the pass.  Barrier; the row's thread (t < 32) sums log pi into a
 * register; barrier (the sums are read: the tile is free).  Then the row x' | a' is built for critic 1 exactly as pmg_k_td3_target builds
 * it for critic 2: x' from memory, a' from G.action by the SAME (row, unit) -> thread map, so a thread reads only its own earlier store
 * and no ordering between threads is involved.  The same rebuild runs again in front of critic 2.
 * Stale tile: when a rebuild starts, the tile holds the actor's or critic 1's activations (which may be inf) in columns up to the widest
 * layer.  The regather writes columns [0, Dx) of all 32 rows, the rebuild's pass columns [Dx, Dx + A) of all 32 rows, thread t < 32 column
 * Dx + A of an odd Dx + A; rows past the batch receive +0.0 in each.  These are all the columns a critic's layer 0 reads, so no stale
 * activation meets a weight or a stand-in zero.  Nothing in a rebuild READS the tile, so it needs no barrier inside. */
__device__ __forceinline__ void sac_rebuild(float* tile, const MlpRawRows& S, const float* keep, long long row0, long long B, int Dx, int A, int t)
{
    mlp_gather(tile, S, row0, B, Dx, Dx, t);
    for (int i = t; i < MLP_ROWS * A; i += 256) {                    /* the head's map: a thread reads what it stored itself */
        const int r = i / A, j = i - r * A;
        tile[r * MLP_LD + Dx + j] = row0 + r < B ? keep[(row0 + r) * A + j] : 0.f;
    }
    if ((Dx + A) & 1) { if (t < MLP_ROWS) tile[t * MLP_LD + Dx + A] = 0.f; }
}
__global__ void __launch_bounds__(256) pmg_k_sac_target(PmgMlp P, PmgMlp Q1, PmgMlp Q2, PmgSacTd X)
{
    __shared__ float tile[MLP_ROWS * MLP_LD];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31;
    const int Dx = P.width[0], A = P.width[P.L] >> 1;
    const MlpRawRows S = {X.T.xn, X.T.xs};
    float* keep = X.G.action;
    const long long ntiles = (P.B + MLP_ROWS - 1) / MLP_ROWS;
    for (long long tb = blockIdx.x; tb < ntiles; tb += gridDim.x) {
        const long long row0 = tb * MLP_ROWS;
        mlp_gather(tile, S, row0, P.B, Dx, (Dx + 1) & ~1, t);
        __syncthreads();
        mlp_layers(tile, P, lane, wave, col);
        for (int i = t; i < MLP_ROWS * A; i += 256) {
            const int r = i / A, j = i - r * A;
            const long long row = row0 + r;
            if (row >= P.B) break;
            const SacHead h = sac_head(X.G, tile[r * MLP_LD + j], tile[r * MLP_LD + A + j],
                                       (X.G.row_offset + (unsigned long long)row) * (unsigned long long)A + (unsigned long long)j);
            keep[row * A + j] = h.a;
            tile[r * MLP_LD + j] = h.l;
        }
        __syncthreads();                                             /* every l_j of the tile is written */
        const bool own = t < MLP_ROWS && row0 + t < P.B;             /* this thread forms the outputs of row row0 + t */
        float logp = 0.f;
        if (own) {
            logp = sac_logp(tile, t, A);
            if (X.G.logp) X.G.logp[row0 + t] = logp;
        }
        __syncthreads();                                             /* the sums are read: the tile is free */
        sac_rebuild(tile, S, keep, row0, P.B, Dx, A, t);
        __syncthreads();
        mlp_layers(tile, Q1, lane, wave, col);
        float q = 0.f;
        if (own) {
            const float z = tile[t * MLP_LD];
            q = Q1.out_act ? tanhf(z) : z;
            if (X.q1) X.q1[row0 + t] = q;
        }
        if (X.twin) {
            __syncthreads();                                         /* q1 is read: column 0 is free */
            sac_rebuild(tile, S, keep, row0, P.B, Dx, A, t);
            __syncthreads();
            mlp_layers(tile, Q2, lane, wave, col);
            if (own) {
                const float z = tile[t * MLP_LD], q2 = Q2.out_act ? tanhf(z) : z;
                if (X.q2) X.q2[row0 + t] = q2;
                q = fminf(q, q2);
            }
        }
        if (own) {
            const float alpha = X.d_alpha ? *X.d_alpha : X.alpha;
            const float rw = X.T.reward[row0 + t];
            const float v = X.T.term && X.T.term[row0 + t] ? rw : fmaf(X.T.gamma, fmaf(-alpha, logp, q), rw);
            X.T.y[row0 + t] = fminf(fmaxf(v, X.T.lo), X.T.hi);
            if (X.T.qn) X.T.qn[row0 + t] = q;
        }
        __syncthreads();                                             /* the next tile's rows overwrite this one's */
    }
}
static unsigned mlp_grid(long long B)
{
    const long long want = (B + MLP_ROWS - 1) / MLP_ROWS;
    return (unsigned)(want < (1 << 20) ? want : (1 << 20));
}
hipError_t pmg_launch_mlp_forward(const PmgMlp& M, const float* d_in, long long in_stride, hipStream_t s)
{
    if (M.B <= 0) return hipSuccess;
    const MlpRawRows S = {d_in, in_stride};
    hipLaunchKernelGGL((pmg_k_mlp<MlpRawRows, false>), dim3(mlp_grid(M.B)), dim3(256), 0, s, S, M);
    return hipGetLastError();
}
hipError_t pmg_launch_mlp_act(const PmgMlp& net, const PmgMlpEnv& E, hipStream_t s)
{
    if (net.B <= 0) return hipSuccess;
    PmgMlp M = net;
    M.key = her_mix(M.seed ^ her_mix(M.counter + HER_GOLD));
    const MlpEnvRows S = {E};
    hipLaunchKernelGGL((pmg_k_mlp<MlpEnvRows, true>), dim3(mlp_grid(M.B)), dim3(256), 0, s, S, M);
    return hipGetLastError();
}
hipError_t pmg_launch_mlp_q(const PmgMlp& M, const float* d_x, long long x_stride, int x_dim, const float* d_a, long long a_stride, hipStream_t s)
{
    if (M.B <= 0) return hipSuccess;
    const MlpCatRows S = {d_x, x_stride, d_a, a_stride, x_dim};
    hipLaunchKernelGGL((pmg_k_mlp<MlpCatRows, false>), dim3(mlp_grid(M.B)), dim3(256), 0, s, S, M);
    return hipGetLastError();
}
hipError_t pmg_launch_td_target(const PmgMlp& actor, const PmgMlp& critic, const PmgTd& T, hipStream_t s)
{
    if (actor.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(pmg_k_td_target, dim3(mlp_grid(actor.B)), dim3(256), 0, s, actor, critic, T);
    return hipGetLastError();
}
hipError_t pmg_launch_td3_target(const PmgMlp& actor, const PmgMlp& critic1, const PmgMlp& critic2, const PmgTd3& T, hipStream_t s)
{
    if (actor.B <= 0) return hipSuccess;
    PmgTd3 X = T;
    X.key = her_mix(X.seed ^ her_mix(X.counter + HER_GOLD));
    hipLaunchKernelGGL(pmg_k_td3_target, dim3(mlp_grid(actor.B)), dim3(256), 0, s, actor, critic1, critic2, X);
    return hipGetLastError();
}
hipError_t pmg_launch_sac_sample(const PmgMlp& M, const PmgSac& head, const float* d_in, long long in_stride, hipStream_t s)
{
    if (M.B <= 0) return hipSuccess;
    PmgSac G = head;
    G.key = her_mix(G.seed ^ her_mix(G.counter + HER_GOLD));
    const MlpRawRows S = {d_in, in_stride};
    hipLaunchKernelGGL((pmg_k_sac<MlpRawRows>), dim3(mlp_grid(M.B)), dim3(256), 0, s, S, M, G);
    return hipGetLastError();
}
hipError_t pmg_launch_sac_act(const PmgMlp& M, const PmgSac& head, const PmgMlpEnv& E, hipStream_t s)
{
    if (M.B <= 0) return hipSuccess;
    PmgSac G = head;
    G.key = her_mix(G.seed ^ her_mix(G.counter + HER_GOLD));
    const MlpEnvRows S = {E};
    hipLaunchKernelGGL((pmg_k_sac<MlpEnvRows>), dim3(mlp_grid(M.B)), dim3(256), 0, s, S, M, G);
    return hipGetLastError();
}
hipError_t pmg_launch_sac_target(const PmgMlp& actor, const PmgMlp& critic1, const PmgMlp& critic2, const PmgSacTd& T, hipStream_t s)
{
    if (actor.B <= 0) return hipSuccess;
    PmgSacTd X = T;
    X.G.key = her_mix(X.G.seed ^ her_mix(X.G.counter + HER_GOLD));
    hipLaunchKernelGGL(pmg_k_sac_target, dim3(mlp_grid(actor.B)), dim3(256), 0, s, actor, critic1, critic2, X);
    return hipGetLastError();
}

/* Back-propagation through a network (pmg_mlp_grad_device, DESIGN.md 3.11): two kernels.  pmg_k_mlp_grad_rows owns 32 rows per workgroup as
 * pmg_k_mlp does, on the same tile: gather, the forward layers (mlp_layers_saved: mlp_layers that also keeps every hidden h_l in the
 * workspace and the sign of every hidden result in registers), the head and delta_{L-1} in place, a thread per (row, unit), then per layer
 * the TRANSPOSED chain s_l[b][k] = sum over j ascending of delta_l[b][j] W_l[j][k], whose masked result is delta_{l-1}, written to the tile
 * and to the workspace; s_0 goes to d_gx / d_ga.  pmg_k_mlp_grad_weights then forms dW_l = delta_l^T h_l and db_l from the workspace, one
 * wavefront per 32 x 32 tile of a dW_l, ONE chain over the batch in ascending row order.
 * ReLU mask: the backward strip (wave, reg, lane) of layer l is row mlp_row(reg, lane), unit 32 wave (+ 128) + (lane & 31) of h_l -- the very
 * element the same lane held when the forward wrote h_l.  So the lane keeps `result > 0` of its 2 x 16 results as one 32-bit word per hidden
 * layer (three words at most) and no h_l is read back: the mask costs no LDS or memory traffic and no barrier.
 * Stale padding: every write-back covers WHOLE 32-unit strips and puts +0.0 at units past the width, so column `width` of an odd width -- the
 * A operand of a chain's last step -- holds a real zero under whatever an earlier, wider layer left there; rows past the batch carry
 * delta = +0.0 from the head on. */
/* THE transposed matrix step, j0 even: acc[row][unit] = fmaf(tile[row][j0 + 1], W[j0 + 1][unit], fmaf(tile[row][j0], W[j0][unit], acc[row][unit]));
 * wcol = W + this lane's unit (lane & 31 of the strip), K = floats from row to row of W.  TAIL: the last step of an odd J, j0 = J - 1:
 * column J of the tile holds zeros and +0.0 stands in for W[J][unit].  Device: A = tile[l & 31][j0 + (l >> 5)] as in mlp_mma,
 * B = W[j0 + (l >> 5)][unit l & 31]: the lanes run along a row of W (coalesced).  Emulator: fmaf over the lane's own 16 results. */
template <bool TAIL>
__device__ __forceinline__ void mlp_mma_t(const float* tile, const float* __restrict__ wcol, int K, int j0, int lane, MlpAcc& acc)
{
#ifndef PMG_EMULATE
    const int h = lane >> 5;
    const float a = tile[(lane & 31) * MLP_LD + j0 + h];
    const float b = TAIL ? mlp_keep(wcol[(long long)j0 * K], h == 0) : wcol[(long long)(j0 + h) * K];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
#else
    for (int reg = 0; reg < 16; reg++) {
        const float* a = tile + mlp_row(reg, lane) * MLP_LD + j0;
        acc[reg] = fmaf(a[1], TAIL ? 0.f : wcol[(long long)(j0 + 1) * K], fmaf(a[0], wcol[(long long)j0 * K], acc[reg]));
    }
#endif
}
/* all J steps of a transposed layer for the NS = 1 or 2 strips of a wavefront (mlp_chain's shape: eight steps written out) */
template <int NS>
__device__ __forceinline__ void mlp_chain_t(const float* tile, const float* __restrict__ w0, const float* __restrict__ w1, int J, int K, int lane,
                                            MlpAcc& acc0, MlpAcc& acc1)
{
    const int J16 = J & ~15, Je = J & ~1;
    for (int j0 = 0; j0 < J16; j0 += 16) {
#pragma unroll
        for (int u = 0; u < 16; u += 2) {
            mlp_mma_t<false>(tile, w0, K, j0 + u, lane, acc0);
            if (NS == 2) mlp_mma_t<false>(tile, w1, K, j0 + u, lane, acc1);
        }
    }
    for (int j0 = J16; j0 < Je; j0 += 2) {
        mlp_mma_t<false>(tile, w0, K, j0, lane, acc0);
        if (NS == 2) mlp_mma_t<false>(tile, w1, K, j0, lane, acc1);
    }
    if (J & 1) {
        mlp_mma_t<true>(tile, w0, K, Je, lane, acc0);
        if (NS == 2) mlp_mma_t<true>(tile, w1, K, Je, lane, acc1);
    }
}
/* mlp_layers for the gradient: the same chains on the same tile, and per hidden layer l -> h_{l + 1}: the lane's 2 x 16 signs into
 * m1 / m2 / m3 (bit reg: strip `wave`, bit 16 + reg: strip `wave + 4`; a result that is exactly 0 or a NaN has mask 0) and, when the
 * weights kernel will run, h_{l + 1} of the rows of the batch into the workspace (lanes along the units: coalesced) */
__device__ __forceinline__ void mlp_layers_saved(float* tile, const PmgMlp& M, const PmgGrad& G, long long row0, int lane, int wave, int col,
                                                 unsigned int& m1, unsigned int& m2, unsigned int& m3)
{
#pragma unroll 1
    for (int l = 0; l < M.L; l++) {
        const int K = M.width[l], Nn = M.width[l + 1];
        const float* __restrict__ W = M.w[l];
        const float* __restrict__ bias = M.b[l];
        const int u0 = 32 * wave + col, u1 = u0 + 128;
        const bool live0 = u0 < Nn, live1 = u1 < Nn, strip0 = 32 * wave < Nn, strip1 = 32 * wave + 128 < Nn;
        const float* w0 = W + (long long)(live0 ? u0 : 0) * K;
        const float* w1 = W + (long long)(live1 ? u1 : 0) * K;
        const float b0 = bias ? bias[live0 ? u0 : 0] : 0.f, b1 = bias ? bias[live1 ? u1 : 0] : 0.f;
        MlpAcc acc0, acc1;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) { acc0[reg] = b0; acc1[reg] = b1; }
        if (strip1) mlp_chain<2>(tile, w0, w1, K, lane, acc0, acc1);
        else if (strip0) mlp_chain<1>(tile, w0, w1, K, lane, acc0, acc1);
        const bool hidden = l + 1 < M.L;
        float* __restrict__ H = hidden && G.grads ? G.wh[l + 1] : nullptr;
        unsigned int mask = 0;
        __syncthreads();                                         /* every wavefront has read the layer's input */
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int r = mlp_row(reg, lane);
            const bool inb = row0 + r < M.B;
            if (strip0) {
                const float v = live0 ? (hidden ? fmaxf(acc0[reg], 0.f) : acc0[reg]) : 0.f;
                tile[r * MLP_LD + u0] = v;
                mask |= (unsigned int)(live0 && acc0[reg] > 0.f) << reg;
                if (H && live0 && inb) H[(row0 + r) * Nn + u0] = v;
            }
            if (strip1) {
                const float v = live1 ? (hidden ? fmaxf(acc1[reg], 0.f) : acc1[reg]) : 0.f;
                tile[r * MLP_LD + u1] = v;
                mask |= (unsigned int)(live1 && acc1[reg] > 0.f) << (16 + reg);
                if (H && live1 && inb) H[(row0 + r) * Nn + u1] = v;
            }
        }
        if (l == 0) m1 = mask; else if (l == 1) m2 = mask; else if (l == 2) m3 = mask;
        __syncthreads();
    }
}
/* s_0[row][c] to where it belongs: column c < x_dim of d_gx, the others of d_ga (either may be null) */
__device__ __forceinline__ void grad_input_store(const PmgGrad& G, long long row, int c, float v)
{
    if (c < G.x_dim) { if (G.gx) G.gx[row * G.gxs + c] = v; }
    else if (G.ga) G.ga[row * G.gas + (c - G.x_dim)] = v;
}
/* the transposed layers on a tile whose columns [0, width[L] rounded up to even) hold delta_{L-1} (rows past the batch and the padding
 * column: +0.0); layer 0 runs only when an input gradient is wanted */
__device__ __forceinline__ void mlp_backward(float* tile, const PmgMlp& M, const PmgGrad& G, long long row0, int lane, int wave, int col,
                                             unsigned int m1, unsigned int m2, unsigned int m3)
{
#pragma unroll 1
    for (int l = M.L - 1; l >= 0; l--) {
        if (l == 0 && !G.gx && !G.ga) break;
        const int J = M.width[l + 1], K = M.width[l];
        const float* __restrict__ W = M.w[l];
        const int k0 = 32 * wave + col, k1 = k0 + 128;            /* this lane's input unit in the strips wave and wave + 4 */
        const bool live0 = k0 < K, live1 = k1 < K, strip0 = 32 * wave < K, strip1 = 32 * wave + 128 < K;
        /* a unit past the width runs on column 0 of W: valid addresses, results never used */
        const float* w0 = W + (live0 ? k0 : 0);
        const float* w1 = W + (live1 ? k1 : 0);
        MlpAcc acc0, acc1;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) { acc0[reg] = 0.f; acc1[reg] = 0.f; }
        if (strip1) mlp_chain_t<2>(tile, w0, w1, J, K, lane, acc0, acc1);
        else if (strip0) mlp_chain_t<1>(tile, w0, w1, J, K, lane, acc0, acc1);
        __syncthreads();                                         /* every wavefront has read delta_l */
        if (l > 0) {
            const unsigned int mask = l == 1 ? m1 : (l == 2 ? m2 : m3);
            float* __restrict__ D = G.grads ? G.wd[l - 1] : nullptr;
            /* whole strips: a masked unit and a unit past the width become a real +0.0 */
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                const int r = mlp_row(reg, lane);
                const bool inb = row0 + r < M.B;
                if (strip0) {
                    const float v = live0 && ((mask >> reg) & 1u) ? acc0[reg] : 0.f;
                    tile[r * MLP_LD + k0] = v;
                    if (D && live0 && inb) D[(row0 + r) * K + k0] = v;
                }
                if (strip1) {
                    const float v = live1 && ((mask >> (16 + reg)) & 1u) ? acc1[reg] : 0.f;
                    tile[r * MLP_LD + k1] = v;
                    if (D && live1 && inb) D[(row0 + r) * K + k1] = v;
                }
            }
            __syncthreads();
        } else {
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                const long long row = row0 + mlp_row(reg, lane);
                if (row >= M.B) continue;
                if (live0) grad_input_store(G, row, k0, acc0[reg]);
                if (live1) grad_input_store(G, row, k1, acc1[reg]);
            }
        }
    }
}
template <class Src>
__global__ void __launch_bounds__(256, 2) pmg_k_mlp_grad_rows(Src S, PmgMlp M, PmgGrad G)
{
    __shared__ float tile[MLP_ROWS * MLP_LD];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31;
    const int A = M.width[M.L];
    const long long ntiles = (M.B + MLP_ROWS - 1) / MLP_ROWS;
    for (long long tb = blockIdx.x; tb < ntiles; tb += gridDim.x) {
        const long long row0 = tb * MLP_ROWS;
        mlp_gather(tile, S, row0, M.B, M.width[0], (M.width[0] + 1) & ~1, t);
        __syncthreads();
        unsigned int m1 = 0, m2 = 0, m3 = 0;
        mlp_layers_saved(tile, M, G, row0, lane, wave, col, m1, m2, m3);
        /* the tile holds z (and +0.0 up to the end of z's last strip): head and delta_{L-1} in place, thread per (row, unit) */
        for (int i = t; i < MLP_ROWS * A; i += 256) {
            const int r = i / A, j = i - r * A;
            const long long row = row0 + r;
            float d = 0.f;
            if (row < M.B) {
                const float z = tile[r * MLP_LD + j], o = M.out_act ? tanhf(z) : z;
                if (G.out) G.out[row * G.os + j] = o;
                float g = G.gscale;
                if (G.gout) g = G.gout[row * G.gos + j];
                else if (G.target) { const float e = o - G.target[row * G.ts + j]; g = G.gscale * e; }
                d = M.out_act ? g * fmaf(-o, o, 1.f) : g;
                if (G.grads) G.wd[M.L - 1][row * A + j] = d;
            }
            tile[r * MLP_LD + j] = d;
        }
        __syncthreads();
        mlp_backward(tile, M, G, row0, lane, wave, col, m1, m2, m3);   /* ends behind a barrier: the next tile's rows may overwrite this one's */
    }
}
/* column col of the rows of a source as a pointer and the floats from row to row.  A lane of the weights kernel keeps ITS column for the
 * whole chain, so which table the column lives in is decided once, outside the loop, and the loop holds plain loads (MlpCatRows::at inside
 * it would be a select fed by two loads) */
__device__ __forceinline__ const float* mlp_column(const MlpRawRows& S, int col, long long& stride) { stride = S.stride; return S.in + col; }
__device__ __forceinline__ const float* mlp_column(const MlpCatRows& S, int col, long long& stride)
{
    const bool in_x = col < S.Dx;
    stride = in_x ? S.xs : S.as;
    return in_x ? S.x + col : S.a + (col - S.Dx);
}
/* h_l[b][this lane's unit]: the workspace (l >= 1) or the row source (l == 0) */
struct GradHCol { const float* __restrict__ p; long long stride; __device__ __forceinline__ float operator()(long long b) const { return p[b * stride]; } };
/* one step of a dW tile, b0 even: acc[j][k] = fmaf(delta[b0 + 1][j], h[b0 + 1][k], fmaf(delta[b0][j], h[b0][k], acc[j][k])) for the 32 units
 * j from jb and the lane's input unit kl (clamped, as jb's units are); BIAS: accb[j][*] likewise with 1 in place of h -- fmaf(delta, 1, acc)
 * is acc + delta exactly.  TAIL: the last step of an odd batch, b0 = B - 1: row B is +0.0 on both sides, from the valid row B - 1 through
 * mlp_keep.  Device: A = delta[b0 + (l >> 5)][jb + (l & 31)], B = h[b0 + (l >> 5)][the lane's unit]: both run along a row (coalesced).  hf(b) = h_l[b][that unit]. */
template <bool TAIL, bool BIAS>
__device__ __forceinline__ void grad_w_mma(const float* __restrict__ delta, int J, int jb, const GradHCol& hf, long long b0, int lane,
                                           MlpAcc& acc, MlpAcc& accb)
{
#ifndef PMG_EMULATE
    const int h = lane >> 5, j = jb + (lane & 31);
    const bool in = !TAIL || h == 0;
    const long long b = in ? b0 + h : b0;
    float a = delta[b * J + (j < J ? j : 0)], v = hf(b);
    if (TAIL) { a = mlp_keep(a, in); v = mlp_keep(v, in); }
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v, acc, 0, 0, 0);
    if (BIAS) accb = __builtin_amdgcn_mfma_f32_32x32x2f32(a, 1.f, accb, 0, 0, 0);
#else
    const float h0 = hf(b0), h1 = TAIL ? 0.f : hf(b0 + 1);
    for (int reg = 0; reg < 16; reg++) {
        const int j = jb + mlp_row(reg, lane), jl = j < J ? j : 0;
        const float a0 = delta[b0 * J + jl], a1 = TAIL ? 0.f : delta[(b0 + 1) * J + jl];
        acc[reg] = fmaf(a1, h1, fmaf(a0, h0, acc[reg]));
        if (BIAS) accb[reg] = fmaf(a1, 1.f, fmaf(a0, 1.f, accb[reg]));
    }
#endif
}
/* the chain over the rows [lo, hi) of one dW tile, lo even, rows ascending, and its stores (the whole batch: lo = 0, hi = B).  Eight steps are
 * written out, as in mlp_chain */
template <bool BIAS>
__device__ __forceinline__ void grad_w_tile(const float* __restrict__ delta, int J, int K, int jb, int k, const GradHCol& hf, long long lo, long long hi, int lane,
                                            float* __restrict__ dw, float* __restrict__ db)
{
    MlpAcc acc, accb;
#pragma unroll
    for (int reg = 0; reg < 16; reg++) { acc[reg] = 0.f; accb[reg] = 0.f; }
    const long long n = hi - lo, B16 = lo + (n & ~15ll), Be = lo + (n & ~1ll);
    for (long long b0 = lo; b0 < B16; b0 += 16) {
#pragma unroll
        for (int u = 0; u < 16; u += 2) grad_w_mma<false, BIAS>(delta, J, jb, hf, b0 + u, lane, acc, accb);
    }
    for (long long b0 = B16; b0 < Be; b0 += 2) grad_w_mma<false, BIAS>(delta, J, jb, hf, b0, lane, acc, accb);
    if (n & 1) grad_w_mma<true, BIAS>(delta, J, jb, hf, Be, lane, acc, accb);
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
        const int j = jb + mlp_row(reg, lane);
        if (j >= J) continue;
        if (k < K) dw[(long long)j * K + k] = acc[reg];
        if (BIAS && (lane & 31) == 0) db[j] = accb[reg];
    }
}
/* tile `tile` of the network's dW tiles (the tiles of layer 0 first) over the rows [lo, hi) into dw[l] / db[l]; the tiles of input strip 0
 * carry the bias sums of their units */
template <class Src>
__device__ __forceinline__ void grad_w_run(const Src& S, const PmgMlp& M, const PmgGrad& G, int tile, long long lo, long long hi,
                                           float* const* dw, float* const* db, long long shift)
{
    int l = 0, tk = 0;
    for (;; l++) {
        tk = (M.width[l] + 31) / 32;
        const int n = ((M.width[l + 1] + 31) / 32) * tk;
        if (tile < n || l + 1 == M.L) break;
        tile -= n;
    }
    const int J = M.width[l + 1], K = M.width[l], jb = 32 * (tile / tk), kb = 32 * (tile % tk), lane = (int)threadIdx.x;
    const int k = kb + (lane & 31), kl = k < K ? k : 0;           /* a unit past the width runs on column 0: valid addresses, never stored */
    GradHCol hf;
    if (l == 0) hf.p = mlp_column(S, kl, hf.stride);
    else { hf.p = G.wh[l] + kl; hf.stride = K; }
    if (kb == 0 && db[l] != nullptr) grad_w_tile<true>(G.wd[l], J, K, jb, k, hf, lo, hi, lane, dw[l] + shift, db[l] + shift);
    else grad_w_tile<false>(G.wd[l], J, K, jb, k, hf, lo, hi, lane, dw[l] + shift, db[l]);
}
/* one wavefront per 32 x 32 tile of a dW_l, ONE chain over the whole batch */
template <class Src>
__global__ void __launch_bounds__(64) pmg_k_mlp_grad_weights(Src S, PmgMlp M, PmgGrad G)
{
    grad_w_run(S, M, G, (int)blockIdx.x, 0, M.B, G.dw, G.db, 0);
}
long long pmg_grad_work_layout(const PmgMlp& M, long long B, float* work, PmgGrad* G)
{
    long long per_row = 0;
    for (int l = 1; l < M.L; l++) {
        if (work) G->wh[l] = work + per_row * B;
        per_row += M.width[l];
    }
    for (int l = 0; l < M.L; l++) {
        if (work) G->wd[l] = work + per_row * B;
        per_row += M.width[l + 1];
    }
    return per_row * B;
}
int pmg_grad_w_tiles(const PmgMlp& M)
{
    int tiles = 0;
    for (int l = 0; l < M.L; l++) tiles += ((M.width[l + 1] + 31) / 32) * ((M.width[l] + 31) / 32);
    return tiles;
}
template <class Src>
static void launch_mlp_grad(const Src& S, const PmgMlp& M, const PmgGrad& G, hipStream_t s)
{
    hipLaunchKernelGGL((pmg_k_mlp_grad_rows<Src>), dim3(mlp_grid(M.B)), dim3(256), 0, s, S, M, G);
    if (!G.grads) return;
    hipLaunchKernelGGL((pmg_k_mlp_grad_weights<Src>), dim3(pmg_grad_w_tiles(M)), dim3(64), 0, s, S, M, G);
}
hipError_t pmg_launch_mlp_grad(const PmgMlp& M, const PmgGrad& G, hipStream_t s)
{
    if (M.B <= 0) return hipSuccess;
    if (G.a) launch_mlp_grad(MlpCatRows{G.x, G.xs, G.a, G.as, G.x_dim}, M, G, s);
    else launch_mlp_grad(MlpRawRows{G.x, G.xs}, M, G, s);
    return hipGetLastError();
}

/* Adam and Polyak (pmg_mlp_adam_device, pmg_mlp_polyak_device, DESIGN.md 3.11): one elementwise sweep over the up to eight tensors of a
 * network.  HBM-bound; a thread finds the tensor of its flat element by comparing against the table's prefix ends (statically indexed:
 * the table stays in scalar registers).  Dword accesses: the tensors come with any 4-byte alignment. */
struct SegAt { float* p; const float* g; float* m; float* v; long long i; };
__device__ __forceinline__ SegAt seg_at(const PmgSegs& T, long long i)
{
    SegAt a = {T.p[0], T.g[0], T.m[0], T.v[0], i};
#pragma unroll
    for (int k = 1; k < 8; k++)
        if (k < T.n && i >= T.end[k - 1]) { a.p = T.p[k]; a.g = T.g[k]; a.m = T.m[k]; a.v = T.v[k]; a.i = i - T.end[k - 1]; }
    return a;
}
__global__ void __launch_bounds__(256) pmg_k_adam(PmgSegs T, PmgAdam A)
{
    const long long total = T.end[T.n - 1];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const SegAt s = seg_at(T, i);
        const float g = s.g[s.i];
        const float m = fmaf(A.beta1, s.m[s.i], A.omb1 * g);
        const float v = fmaf(A.beta2, s.v[s.i], A.omb2 * (g * g));
        s.m[s.i] = m; s.v[s.i] = v;
        s.p[s.i] = s.p[s.i] - A.step_size * (m / (sqrtf(v) * A.rsc2 + A.eps));
    }
}
__global__ void __launch_bounds__(256) pmg_k_polyak(PmgSegs T, float tau)
{
    const long long total = T.end[T.n - 1];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const SegAt s = seg_at(T, i);
        const float t = s.p[s.i];
        s.p[s.i] = fmaf(tau, s.g[s.i] - t, t);
    }
}
static unsigned seg_grid(const PmgSegs& T)
{
    const long long want = (T.end[T.n - 1] + 255) / 256;
    return (unsigned)(want < 2048 ? want : 2048);
}
hipError_t pmg_launch_adam(const PmgSegs& T, const PmgAdam& A, hipStream_t s)
{
    hipLaunchKernelGGL(pmg_k_adam, dim3(seg_grid(T)), dim3(256), 0, s, T, A);
    return hipGetLastError();
}
hipError_t pmg_launch_polyak(const PmgSegs& T, float tau, hipStream_t s)
{
    hipLaunchKernelGGL(pmg_k_polyak, dim3(seg_grid(T)), dim3(256), 0, s, T, tau);
    return hipGetLastError();
}

/* The data-parallel merge (pmg_mlp_params_pack_device, pmg_mlp_params_merge_device, pmg_mlp_adam_merge_device, DESIGN.md 3.17): three
 * elementwise sweeps of the shape of pmg_k_adam -- a thread per parameter, consecutive addresses across the lanes on the flat side, the
 * tensor of a flat element found by seg_at, dword accesses (the tensors come with any 4-byte alignment).  A slot is one rank's gradient in
 * the flat order of PmgSegs; slot r starts at slots + r * stride.  The sum is G_0 + G_1 + ... in ascending r from G_0 ITSELF, one float32
 * rounding per addition: no atomics, nothing depends on the grid. */
__global__ void __launch_bounds__(256) pmg_k_params_pack(PmgSegs T, float* __restrict__ flat)
{
    const long long total = T.end[T.n - 1];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const SegAt s = seg_at(T, i);
        flat[i] = s.g[s.i];
    }
}
__device__ __forceinline__ float rank_sum(const float* __restrict__ slots, long long stride, int n, long long i)
{
    const float* __restrict__ p = slots + i;
    float acc = p[0];
#pragma unroll 8
    for (int r = 1; r < n; r++) acc = acc + p[(long long)r * stride];
    return acc;
}
__global__ void __launch_bounds__(256) pmg_k_params_merge_ranks(PmgSegs T, const float* __restrict__ slots, long long stride, int n)
{
    const long long total = T.end[T.n - 1];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const float acc = rank_sum(slots, stride, n, i);
        const SegAt s = seg_at(T, i);
        s.p[s.i] = acc;
    }
}
/* the same sum handed straight to pmg_k_adam's step: the summed gradient stays in a register; keep != 0: it is also stored to the tensors of
 * T.g (the caller's grad_out, writable: the table merely types them as the gradient pmg_k_adam reads) */
__global__ void __launch_bounds__(256) pmg_k_adam_merge_ranks(PmgSegs T, PmgAdam A, const float* __restrict__ slots, long long stride, int n, int keep)
{
    const long long total = T.end[T.n - 1];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const float g = rank_sum(slots, stride, n, i);
        const SegAt s = seg_at(T, i);
        if (keep) const_cast<float*>(s.g)[s.i] = g;
        const float m = fmaf(A.beta1, s.m[s.i], A.omb1 * g);
        const float v = fmaf(A.beta2, s.v[s.i], A.omb2 * (g * g));
        s.m[s.i] = m; s.v[s.i] = v;
        s.p[s.i] = s.p[s.i] - A.step_size * (m / (sqrtf(v) * A.rsc2 + A.eps));
    }
}
hipError_t pmg_launch_params_pack(const PmgSegs& T, float* flat, hipStream_t s)
{
    hipLaunchKernelGGL(pmg_k_params_pack, dim3(seg_grid(T)), dim3(256), 0, s, T, flat);
    return hipGetLastError();
}
hipError_t pmg_launch_params_merge_ranks(const PmgSegs& T, const float* slots, long long stride, int nslots, hipStream_t s)
{
    hipLaunchKernelGGL(pmg_k_params_merge_ranks, dim3(seg_grid(T)), dim3(256), 0, s, T, slots, stride, nslots);
    return hipGetLastError();
}
hipError_t pmg_launch_adam_merge_ranks(const PmgSegs& T, const PmgAdam& A, const float* slots, long long stride, int nslots, int keep, hipStream_t s)
{
    hipLaunchKernelGGL(pmg_k_adam_merge_ranks, dim3(seg_grid(T)), dim3(256), 0, s, T, A, slots, stride, nslots, keep);
    return hipGetLastError();
}

/* The chunked batch reduction (pmg_mlp_grad_chunked_device, DESIGN.md 3.12): pmg_k_mlp_grad_rows as above, then pmg_k_mlp_grad_partials, one
 * wavefront per (chunk, 32 x 32 tile of a dW_l) -- grad_w_run over the chunk's rows alone, chunk c's partial of every tensor at part + c P in
 * the flat order of PmgSegs --, then pmg_k_mlp_grad_merge, a thread per parameter that adds its C partials in ascending c (consecutive
 * addresses across the lanes) and stores the sum.  Stream order is the only synchronisation: no atomics, no counter.  The chains run
 * R / 2 steps on tiles x C wavefronts where the single chain runs B / 2 on tiles. */
template <class Src>
__global__ void __launch_bounds__(64) pmg_k_mlp_grad_partials(Src S, PmgMlp M, PmgGrad G, PmgGradChunks Q)
{
    const long long c = (long long)(blockIdx.x / (unsigned)Q.tiles), lo = c * Q.R, hi = lo + Q.R < M.B ? lo + Q.R : M.B;
    grad_w_run(S, M, G, (int)(blockIdx.x % (unsigned)Q.tiles), lo, hi, Q.pw, Q.pb, c * Q.P);
}
__global__ void __launch_bounds__(256) pmg_k_mlp_grad_merge(PmgSegs T, const float* __restrict__ part, long long C, long long P)
{
    const long long total = T.end[T.n - 1];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const float* __restrict__ p = part + i;
        float acc = p[0];
#pragma unroll 8
        for (long long c = 1; c < C; c++) acc = acc + p[c * P];
        const SegAt s = seg_at(T, i);
        s.p[s.i] = acc;
    }
}
template <class Src>
static void launch_mlp_grad_chunked(const Src& S, const PmgMlp& M, const PmgGrad& G, const PmgGradChunks& Q, const PmgSegs& T, hipStream_t s)
{
    hipLaunchKernelGGL((pmg_k_mlp_grad_rows<Src>), dim3(mlp_grid(M.B)), dim3(256), 0, s, S, M, G);
    hipLaunchKernelGGL((pmg_k_mlp_grad_partials<Src>), dim3((unsigned)(Q.C * Q.tiles)), dim3(64), 0, s, S, M, G, Q);
    hipLaunchKernelGGL(pmg_k_mlp_grad_merge, dim3(seg_grid(T)), dim3(256), 0, s, T, (const float*)Q.part, Q.C, Q.P);
}
hipError_t pmg_launch_mlp_grad_chunked(const PmgMlp& M, const PmgGrad& G, const PmgGradChunks& Q, const PmgSegs& T, hipStream_t s)
{
    if (M.B <= 0) return hipSuccess;
    if (G.a) launch_mlp_grad_chunked(MlpCatRows{G.x, G.xs, G.a, G.as, G.x_dim}, M, G, Q, T, s);
    else launch_mlp_grad_chunked(MlpRawRows{G.x, G.xs}, M, G, Q, T, s);
    return hipGetLastError();
}

/* The actor's half of an update in one call (pmg_policy_grad_device, DESIGN.md 3.13): the actor's forward, the critic's forward on x | clip(o),
 * the critic's input gradient, the L2 / clip head and the actor's transposed layers on ONE tile -- pmg_k_td_target's hand-over on the way
 * forward, its mirror on the way back --, then the weights kernel of 3.11 (or the partials / merge pair of 3.12), unchanged, on the actor's
 * workspace.  While the critic owns the tile, o lives in the workspace slot of the actor's delta_{L-1}: thread (row, unit) of the hand-over
 * writes it, the same thread of the hand-back reads it and overwrites it with delta_{L-1}, so no ordering between threads is involved.
 * Without grads the actor's backward does not run, o is not needed behind the hand-over and the workspace is not touched. */
/* mlp_layers_saved for a network of which nothing is saved (the critic of pmg_k_policy_grad_rows): the same chains on the same tile and the
 * lane's 2 x 16 signs per hidden layer in m1 / m2 / m3, bit for bit as there */
__device__ __forceinline__ void mlp_layers_masked(float* tile, const PmgMlp& M, int lane, int wave, int col, unsigned int& m1, unsigned int& m2,
                                                  unsigned int& m3)
{
#pragma unroll 1
    for (int l = 0; l < M.L; l++) {
        const int K = M.width[l], Nn = M.width[l + 1];
        const float* __restrict__ W = M.w[l];
        const float* __restrict__ bias = M.b[l];
        const int u0 = 32 * wave + col, u1 = u0 + 128;
        const bool live0 = u0 < Nn, live1 = u1 < Nn, strip0 = 32 * wave < Nn, strip1 = 32 * wave + 128 < Nn;
        const float* w0 = W + (long long)(live0 ? u0 : 0) * K;
        const float* w1 = W + (long long)(live1 ? u1 : 0) * K;
        const float b0 = bias ? bias[live0 ? u0 : 0] : 0.f, b1 = bias ? bias[live1 ? u1 : 0] : 0.f;
        MlpAcc acc0, acc1;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) { acc0[reg] = b0; acc1[reg] = b1; }
        if (strip1) mlp_chain<2>(tile, w0, w1, K, lane, acc0, acc1);
        else if (strip0) mlp_chain<1>(tile, w0, w1, K, lane, acc0, acc1);
        const bool hidden = l + 1 < M.L;
        unsigned int mask = 0;
        __syncthreads();                                         /* every wavefront has read the layer's input */
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int r = mlp_row(reg, lane);
            if (strip0) {
                tile[r * MLP_LD + u0] = live0 ? (hidden ? fmaxf(acc0[reg], 0.f) : acc0[reg]) : 0.f;
                mask |= (unsigned int)(live0 && acc0[reg] > 0.f) << reg;
            }
            if (strip1) {
                tile[r * MLP_LD + u1] = live1 ? (hidden ? fmaxf(acc1[reg], 0.f) : acc1[reg]) : 0.f;
                mask |= (unsigned int)(live1 && acc1[reg] > 0.f) << (16 + reg);
            }
        }
        if (l == 0) m1 = mask; else if (l == 1) m2 = mask; else if (l == 2) m3 = mask;
        __syncthreads();
    }
}
/* mlp_backward for that network: the transposed layers L-1 ... 1 on the tile, nothing saved; then layer 0, of which only the action columns
 * [Dx, Dx + A) are wanted: s_0 of the 32-unit strips that hold any of them goes to the tile at its own columns (units past the width: +0.0)
 * and, when asked, to ga; the strips that hold none run no chain.  Ends behind a barrier */
__device__ __forceinline__ void mlp_backward_action(float* tile, const PmgMlp& M, int Dx, float* __restrict__ ga, long long gas, long long row0,
                                                    int lane, int wave, int col, unsigned int m1, unsigned int m2, unsigned int m3)
{
#pragma unroll 1
    for (int l = M.L - 1; l >= 0; l--) {
        const int J = M.width[l + 1], K = M.width[l];
        const float* __restrict__ W = M.w[l];
        const int k0 = 32 * wave + col, k1 = k0 + 128;
        const bool live0 = k0 < K, live1 = k1 < K;
        const bool strip0 = 32 * wave < K && (l > 0 || 32 * wave + 32 > Dx), strip1 = 32 * wave + 128 < K && (l > 0 || 32 * wave + 160 > Dx);
        const float* w0 = W + (live0 ? k0 : 0);
        const float* w1 = W + (live1 ? k1 : 0);
        MlpAcc acc0, acc1;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) { acc0[reg] = 0.f; acc1[reg] = 0.f; }
        if (strip0 && strip1) mlp_chain_t<2>(tile, w0, w1, J, K, lane, acc0, acc1);
        else if (strip0) mlp_chain_t<1>(tile, w0, w1, J, K, lane, acc0, acc1);
        else if (strip1) mlp_chain_t<1>(tile, w1, w0, J, K, lane, acc1, acc0);   /* layer 0 alone: strip `wave + 4` without strip `wave` */
        __syncthreads();                                         /* every wavefront has read delta_l */
        const unsigned int mask = l == 0 ? 0xffffffffu : (l == 1 ? m1 : (l == 2 ? m2 : m3));
        float* __restrict__ out = l == 0 ? ga : nullptr;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int r = mlp_row(reg, lane);
            const bool inb = row0 + r < M.B;
            if (strip0) {
                const float v = live0 && ((mask >> reg) & 1u) ? acc0[reg] : 0.f;
                tile[r * MLP_LD + k0] = v;
                if (out && live0 && k0 >= Dx && inb) out[(row0 + r) * gas + (k0 - Dx)] = v;
            }
            if (strip1) {
                const float v = live1 && ((mask >> (16 + reg)) & 1u) ? acc1[reg] : 0.f;
                tile[r * MLP_LD + k1] = v;
                if (out && live1 && k1 >= Dx && inb) out[(row0 + r) * gas + (k1 - Dx)] = v;
            }
        }
        __syncthreads();
    }
}
/* P: the actor, Q: the critic, G: the actor's gradient arguments (x, out, grads, dw / db, the workspace; gx = ga = null, so mlp_backward
 * stops in front of the actor's layer 0), X: what belongs to neither network */
__global__ void __launch_bounds__(256, 2) pmg_k_policy_grad_rows(PmgMlp P, PmgMlp Q, PmgGrad G, PmgPolicy X)
{
    __shared__ float tile[MLP_ROWS * MLP_LD];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31;
    const int Dx = P.width[0], A = P.width[P.L];
    const MlpRawRows S = {G.x, G.xs};
    float* __restrict__ stash = G.grads ? G.wd[P.L - 1] : nullptr;
    const bool back = G.grads || X.ga, critic = back || X.q;
    const int r = t >> 3;                                        /* the row of this thread in both hand-overs: 8 units of all 32 rows per pass */
    const long long ntiles = (P.B + MLP_ROWS - 1) / MLP_ROWS;
    for (long long tb = blockIdx.x; tb < ntiles; tb += gridDim.x) {
        const long long row0 = tb * MLP_ROWS, row = row0 + r;
        mlp_gather(tile, S, row0, P.B, Dx, (Dx + 1) & ~1, t);
        __syncthreads();
        unsigned int am1 = 0, am2 = 0, am3 = 0, cm1 = 0, cm2 = 0, cm3 = 0;
        mlp_layers_saved(tile, P, G, row0, lane, wave, col, am1, am2, am3);
        /* pmg_k_td_target's hand-over: z in columns [0, A) -> a = clip(o) in columns [Dx, Dx + A), the units in DESCENDING order.  The passes
         * are cut at multiples of 8 from unit 0, as the hand-back's are: unit j of a row is the same thread's both times */
        for (int lo = (A - 1) & ~7; lo >= 0; lo -= 8) {
            const int j = lo + (t & 7);
            const float z = j < A ? tile[r * MLP_LD + j] : 0.f;
            __syncthreads();                                     /* the pass has read its z: columns [Dx + lo, Dx + lo + 8) are free */
            if (j < A) {
                const float o = P.out_act ? tanhf(z) : z, a = fminf(fmaxf(o, -1.f), 1.f);
                tile[r * MLP_LD + Dx + j] = row < P.B ? a : 0.f;
                if (row < P.B) {
                    if (X.action) X.action[row * X.as + j] = a;
                    if (G.out) G.out[row * G.os + j] = o;
                    if (stash) stash[row * A + j] = o;
                }
            }
        }
        if (critic) {
            mlp_gather(tile, S, row0, P.B, Dx, Dx, t);           /* columns below Dx: no pass wrote them, every pass is done reading */
            if ((Dx + A) & 1) { if (t < MLP_ROWS) tile[t * MLP_LD + Dx + A] = 0.f; }
            __syncthreads();
            mlp_layers_masked(tile, Q, lane, wave, col, cm1, cm2, cm3);
            /* the critic's head in column 0; column 1, the padding of its single output, is +0.0 from the last layer's whole strip */
            if (t < MLP_ROWS) {
                float d = 0.f;
                if (row0 + t < P.B) {
                    const float z = tile[t * MLP_LD], q = Q.out_act ? tanhf(z) : z;
                    if (X.q) X.q[row0 + t] = q;
                    d = Q.out_act ? X.gscale * fmaf(-q, q, 1.f) : X.gscale;
                }
                tile[t * MLP_LD] = d;
            }
            __syncthreads();
        }
        if (back) mlp_backward_action(tile, Q, Dx, X.ga, X.gas, row0, lane, wave, col, cm1, cm2, cm3);
        if (G.grads) {
            /* the hand-back, the hand-over's mirror: ga in columns [Dx, Dx + A) -> the actor's delta_{L-1} in columns [0, A).  The values move DOWN,
             * so the passes run in ASCENDING order: a pass writes only columns below every column a later pass reads.  Every column the actor's
             * first transposed chain reads is written here for all 32 rows: rows past the batch and column A of an odd A as +0.0 */
            for (int lo = 0; lo < A; lo += 8) {
                const int j = lo + (t & 7);
                const float ga = j < A ? tile[r * MLP_LD + Dx + j] : 0.f;
                __syncthreads();                                 /* the pass has read its ga: columns [lo, lo + 8) are free */
                if (j < A) {
                    float d = 0.f;
                    if (row < P.B) {
                        const float o = stash[row * A + j];
                        const float g = fmaf(X.l2scale, o, (o >= -1.f && o <= 1.f) ? ga : 0.f);
                        d = P.out_act ? g * fmaf(-o, o, 1.f) : g;
                        stash[row * A + j] = d;
                    }
                    tile[r * MLP_LD + j] = d;
                }
            }
            if (A & 1) { if (t < MLP_ROWS) tile[t * MLP_LD + A] = 0.f; }
            __syncthreads();
            mlp_backward(tile, P, G, row0, lane, wave, col, am1, am2, am3);
        }
        __syncthreads();                                         /* the next tile's rows overwrite this one's */
    }
}
/* The same with a behaviour-cloning term on the demonstration rows and its Q-filter (pmg_policy_grad_bc_device, DESIGN.md 3.18):
 * pmg_k_policy_grad_rows, pass for pass, plus what is marked `bc` below.  A tile that holds a demonstration row (a workgroup-uniform
 * branch) FIRST runs the critic on x | ad -- pmg_k_mlp<MlpCatRows>'s gather and layers, the chain of pmg_q_device --; qd then waits in a
 * register of the row's thread (t < 32), as q1 does in pmg_k_td3_target, while the tile goes through the passes of the sibling unchanged.
 * Stale tile: the pass leaves the critic's activations (which may be inf) on the tile exactly as the previous tile of the grid loop leaves
 * its own, and the actor's gather behind it writes every column the actor's layer 0 reads -- [0, Dx) and the padding column of an odd Dx,
 * all 32 rows, rows past the batch as zeros -- as it does there; the pass's own gather writes columns [0, Dx + A) and the padding column of
 * an odd Dx + A the same way.  Once q exists the row's thread forms the filter flag into flt[]; the barrier behind the critic's head
 * fences it from the hand-back, whose thread (row, j) reads its row's flag and ad[row][j] from the caller's table.  The next tile's flags
 * are written behind the barriers of its own forward passes, so no reader of this tile's is still under way. */
/* the rows x[r] | ad[r] of the demonstration pass: MlpCatRows, except that a row below `begin` takes the action of row `begin` -- no
 * demonstration action below demo_begin is read; what the chain makes of such a row is used by nobody */
struct MlpDemoRows {
    const float* __restrict__ x; long long xs; const float* __restrict__ a; long long as; int Dx; long long begin;
    __device__ __forceinline__ float at(long long r, int col) const { return col < Dx ? x[r * xs + col] : a[(r < begin ? begin : r) * as + (col - Dx)]; }
};
/* P, Q, G, X: as for pmg_k_policy_grad_rows; D: the demonstrations and the filter */
__global__ void __launch_bounds__(256, 2) pmg_k_policy_grad_bc_rows(PmgMlp P, PmgMlp Q, PmgGrad G, PmgPolicy X, PmgPolicyBc D)
{
    __shared__ float tile[MLP_ROWS * MLP_LD];
    __shared__ unsigned char flt[MLP_ROWS];                      /* bc: f of the tile's rows */
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31;
    const int Dx = P.width[0], A = P.width[P.L];
    const MlpRawRows S = {G.x, G.xs};
    float* __restrict__ stash = G.grads ? G.wd[P.L - 1] : nullptr;
    const bool back = G.grads || X.ga, critic = back || X.q || D.filter;
    const int r = t >> 3;                                        /* the row of this thread in both hand-overs: 8 units of all 32 rows per pass */
    const long long ntiles = (P.B + MLP_ROWS - 1) / MLP_ROWS;
    for (long long tb = blockIdx.x; tb < ntiles; tb += gridDim.x) {
        const long long row0 = tb * MLP_ROWS, row = row0 + r;
        float qd = 0.f;
        if (row0 + MLP_ROWS > D.begin) {                         /* bc: the demonstration pass, step 2b (the launcher sees to begin < B) */
            const MlpDemoRows SD = {G.x, G.xs, D.ad, D.ads, Dx, D.begin};
            mlp_gather(tile, SD, row0, P.B, Dx + A, (Dx + A + 1) & ~1, t);
            __syncthreads();
            mlp_layers(tile, Q, lane, wave, col);
            if (t < MLP_ROWS && row0 + t < P.B && row0 + t >= D.begin) {
                const float z = tile[t * MLP_LD];
                qd = Q.out_act ? tanhf(z) : z;
                if (D.qd) D.qd[row0 + t] = qd;
            }
            __syncthreads();                                     /* qd is read: column 0 is free */
        }
        mlp_gather(tile, S, row0, P.B, Dx, (Dx + 1) & ~1, t);
        __syncthreads();
        unsigned int am1 = 0, am2 = 0, am3 = 0, cm1 = 0, cm2 = 0, cm3 = 0;
        mlp_layers_saved(tile, P, G, row0, lane, wave, col, am1, am2, am3);
        for (int lo = (A - 1) & ~7; lo >= 0; lo -= 8) {          /* the hand-over */
            const int j = lo + (t & 7);
            const float z = j < A ? tile[r * MLP_LD + j] : 0.f;
            __syncthreads();                                     /* the pass has read its z: columns [Dx + lo, Dx + lo + 8) are free */
            if (j < A) {
                const float o = P.out_act ? tanhf(z) : z, a = fminf(fmaxf(o, -1.f), 1.f);
                tile[r * MLP_LD + Dx + j] = row < P.B ? a : 0.f;
                if (row < P.B) {
                    if (X.action) X.action[row * X.as + j] = a;
                    if (G.out) G.out[row * G.os + j] = o;
                    if (stash) stash[row * A + j] = o;
                }
            }
        }
        if (critic) {
            mlp_gather(tile, S, row0, P.B, Dx, Dx, t);           /* columns below Dx: no pass wrote them, every pass is done reading */
            if ((Dx + A) & 1) { if (t < MLP_ROWS) tile[t * MLP_LD + Dx + A] = 0.f; }
            __syncthreads();
            mlp_layers_masked(tile, Q, lane, wave, col, cm1, cm2, cm3);
            if (t < MLP_ROWS) {
                float d = 0.f;
                if (row0 + t < P.B) {
                    const float z = tile[t * MLP_LD], q = Q.out_act ? tanhf(z) : z;
                    if (X.q) X.q[row0 + t] = q;
                    d = Q.out_act ? X.gscale * fmaf(-q, q, 1.f) : X.gscale;
                    const unsigned char f = row0 + t >= D.begin && (!D.q_filter || qd > q);   /* bc: step 2c */
                    flt[t] = f;
                    if (D.filter) D.filter[row0 + t] = f;
                }
                tile[t * MLP_LD] = d;
            }
            __syncthreads();
        }
        if (back) mlp_backward_action(tile, Q, Dx, X.ga, X.gas, row0, lane, wave, col, cm1, cm2, cm3);
        if (G.grads) {
            for (int lo = 0; lo < A; lo += 8) {                  /* the hand-back */
                const int j = lo + (t & 7);
                const float ga = j < A ? tile[r * MLP_LD + Dx + j] : 0.f;
                __syncthreads();                                 /* the pass has read its ga: columns [lo, lo + 8) are free */
                if (j < A) {
                    float d = 0.f;
                    if (row < P.B) {
                        const float o = stash[row * A + j];
                        float g = fmaf(X.l2scale, o, (o >= -1.f && o <= 1.f) ? ga : 0.f);
                        if (flt[r]) {                            /* bc: step 4, the difference rounded once */
                            const float e = o - D.ad[row * D.ads + j];
                            g = fmaf(D.bcscale, e, g);
                        }
                        d = P.out_act ? g * fmaf(-o, o, 1.f) : g;
                        stash[row * A + j] = d;
                    }
                    tile[r * MLP_LD + j] = d;
                }
            }
            if (A & 1) { if (t < MLP_ROWS) tile[t * MLP_LD + A] = 0.f; }
            __syncthreads();
            mlp_backward(tile, P, G, row0, lane, wave, col, am1, am2, am3);
        }
        __syncthreads();                                         /* the next tile's rows overwrite this one's */
    }
}
hipError_t pmg_launch_policy_grad(const PmgMlp& P, const PmgMlp& Q, const PmgGrad& G, const PmgPolicy& X, const PmgGradChunks* C, const PmgSegs* T,
                                  hipStream_t s, const PmgPolicyBc* D)
{
    if (P.B <= 0) return hipSuccess;
    /* a batch without a demonstration row (begin == B) is the sibling's: its kernel, which holds 45 fewer spilled SGPRs (DESIGN.md 3.18), and
     * a filter of zeros */
    if (D && D->begin < P.B) hipLaunchKernelGGL(pmg_k_policy_grad_bc_rows, dim3(mlp_grid(P.B)), dim3(256), 0, s, P, Q, G, X, *D);
    else {
        hipLaunchKernelGGL(pmg_k_policy_grad_rows, dim3(mlp_grid(P.B)), dim3(256), 0, s, P, Q, G, X);
        if (D && D->filter) if (hipError_t err = hipMemsetAsync(D->filter, 0, (size_t)P.B, s)) return err;
    }
    if (G.grads) {
        const MlpRawRows S = {G.x, G.xs};
        if (!C) hipLaunchKernelGGL((pmg_k_mlp_grad_weights<MlpRawRows>), dim3(pmg_grad_w_tiles(P)), dim3(64), 0, s, S, P, G);
        else {
            hipLaunchKernelGGL((pmg_k_mlp_grad_partials<MlpRawRows>), dim3((unsigned)(C->C * C->tiles)), dim3(64), 0, s, S, P, G, *C);
            hipLaunchKernelGGL(pmg_k_mlp_grad_merge, dim3(seg_grid(*T)), dim3(256), 0, s, *T, (const float*)C->part, C->C, C->P);
        }
    }
    return hipGetLastError();
}

/* SAC's actor half in one call (pmg_sac_policy_grad_device, DESIGN.md 3.16), pmg_k_policy_grad_rows' sibling for the Gaussian actor: the actor's
 * forward, pmg_k_sac_target's head, either critic's forward on x | a and its input-only backward, the selection of ga by q1 <= q2, the head
 * gradient and the actor's transposed layers on ONE tile, then the weights kernel of 3.11 (or the partials / merge pair of 3.12), unchanged,
 * on the actor's workspace.
 * Forward: nothing is handed to the critics through the tile (the hazard of 3.15: the actor leaves 2 A columns).  Thread (row, unit j) of
 * pmg_k_sac's map writes a to X.H.action (the caller's d_action, or the workspace), l_j into its own column j and, when the head gradient
 * will run, sd n and the in-range predicate (1.0 / 0.0) into X.stash -- two floats per (row, unit): the actor's delta_{L-1} slot, or d_ghead
 * without grads.  The SAME thread reads them back in the hand-back and overwrites them with g_mu | g_ls, and the same thread writes critic
 * 1's ga to X.ga1 and reads it back behind critic 2: a thread reads only its own earlier stores, so no ordering between threads is involved.
 * x | a is rebuilt in front of each critic by sac_rebuild's map (sac_rebuild_at: the kept action may sit at a stride).
 * Hand-back: ga sits in columns [Dx, Dx + A), g_mu | g_ls go to columns [0, 2 A), which overlap them when Dx < 2 A.  The passes (256
 * (row, unit) pairs of the head's map each) read their ga one pass AHEAD of their writes: behind the barrier of pass k the ga of the passes up to
 * k + 1 are in registers (two per thread), and passes k and k + 2 share no row (A <= 128 < 256), so no write reaches a ga still to be read.
 * Columns [0, 2 A) are written for all 32 rows, +0.0 past the batch; 2 A is even, so the actor's first transposed chain reads no padding
 * column and nothing stale.
 * Which critic supplies ga is a per-row flag in LDS beside the tile, written by the row's thread (t < 32) in front of the barrier that
 * precedes critic 2's backward; the same word holds q1 for that thread while critic 2 runs. */
__device__ __forceinline__ void sac_rebuild_at(float* tile, const MlpRawRows& S, const float* keep, long long ks, long long row0, long long B, int Dx, int A,
                                               int t)
{
    mlp_gather(tile, S, row0, B, Dx, Dx, t);
    for (int i = t; i < MLP_ROWS * A; i += 256) {                    /* the head's map: a thread reads what it stored itself */
        const int r = i / A, j = i - r * A;
        tile[r * MLP_LD + Dx + j] = row0 + r < B ? keep[(row0 + r) * ks + j] : 0.f;
    }
    if ((Dx + A) & 1) { if (t < MLP_ROWS) tile[t * MLP_LD + Dx + A] = 0.f; }
}
/* a critic's output of the row's thread (t < 32; +0.0 elsewhere) and, when its backward will run, the constant head into column 0 of all 32
 * rows (rows past the batch: +0.0); column 1, the padding of the single output, is +0.0 from the last layer's whole strip */
__device__ __forceinline__ float sac_pg_qhead(float* tile, const PmgMlp& Q, float gscale, bool back, bool own, int t)
{
    float q = 0.f;
    if (t < MLP_ROWS) {
        float d = 0.f;
        if (own) {
            const float z = tile[t * MLP_LD];
            q = Q.out_act ? tanhf(z) : z;
            d = Q.out_act ? gscale * fmaf(-q, q, 1.f) : gscale;
        }
        if (back) tile[t * MLP_LD] = d;
    }
    return q;
}
/* both critics as ONE kernel argument: the pass over the critics picks its network by a run-time index into the argument itself, which stays
 * in the kernel-argument segment (two arguments picked by a select are copied to scratch: 384 bytes per lane) */
struct PmgMlpPair { PmgMlp q[2]; };
/* P: the actor, QQ: the critics (q[1] is read only when X.twin), G: the actor's gradient arguments as for pmg_k_policy_grad_rows */
__global__ void __launch_bounds__(256, 2) pmg_k_sac_policy_grad_rows(PmgMlp P, PmgMlpPair QQ, PmgGrad G, PmgSacPolicy X)
{
    __shared__ float tile[MLP_ROWS * MLP_LD];
    __shared__ float sel[MLP_ROWS];                              /* row r of the tile: q1 while critic 2 runs (its own thread's), then 1.0 where critic 1 supplies ga */
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31;
    const int Dx = P.width[0], A = P.width[P.L] >> 1;
    const MlpRawRows S = {G.x, G.xs};
    float* keep = X.H.action;
    const long long ks = X.H.as;
    const bool headgrad = X.stash != nullptr, back = headgrad || X.ga, critic = back || X.q1 || X.q2;
    const long long ntiles = (P.B + MLP_ROWS - 1) / MLP_ROWS;
    for (long long tb = blockIdx.x; tb < ntiles; tb += gridDim.x) {
        const long long row0 = tb * MLP_ROWS;
        mlp_gather(tile, S, row0, P.B, Dx, (Dx + 1) & ~1, t);
        __syncthreads();
        unsigned int am1 = 0, am2 = 0, am3 = 0, cm1 = 0, cm2 = 0, cm3 = 0;
        mlp_layers_saved(tile, P, G, row0, lane, wave, col, am1, am2, am3);
        for (int i = t; i < MLP_ROWS * A; i += 256) {            /* the head, pmg_k_sac_target's pass */
            const int r = i / A, j = i - r * A;
            const long long row = row0 + r;
            if (row >= P.B) break;
            const float ls = tile[r * MLP_LD + A + j];
            const SacHead h = sac_head(X.H, tile[r * MLP_LD + j], ls, (X.H.row_offset + (unsigned long long)row) * (unsigned long long)A + (unsigned long long)j);
            keep[row * ks + j] = h.a;
            tile[r * MLP_LD + j] = h.l;
            if (headgrad) {
                const float sd = expf(fminf(fmaxf(ls, X.H.ls_lo), X.H.ls_hi));   /* sac_head's sd */
                X.stash[row * X.ss + j] = sd * h.n;
                X.stash[row * X.ss + A + j] = (ls >= X.H.ls_lo && ls <= X.H.ls_hi) ? 1.f : 0.f;
            }
        }
        __syncthreads();                                         /* every l_j of the tile is written */
        const bool own = t < MLP_ROWS && row0 + t < P.B;         /* this thread forms the outputs of row row0 + t */
        if (own && X.H.logp) X.H.logp[row0 + t] = sac_logp(tile, t, A);
        if (critic) {
            /* ONE call site for both critics: Q is a reference into the kernel's own arguments, picked per pass */
#pragma unroll 1
            for (int c = 0; c <= X.twin; c++) {
                const PmgMlp& Q = QQ.q[c];
                if (c && back)
                    for (int i = t; i < MLP_ROWS * A; i += 256) {    /* critic 1's ga out of critic 2's way, by the head's map */
                        const int r = i / A, j = i - r * A;
                        if (row0 + r >= P.B) break;
                        X.ga1[(row0 + r) * A + j] = tile[r * MLP_LD + Dx + j];
                    }
                __syncthreads();                                 /* the sums (c == 1: q1 and ga) are read: the tile is free */
                sac_rebuild_at(tile, S, keep, ks, row0, P.B, Dx, A, t);
                __syncthreads();
                mlp_layers_masked(tile, Q, lane, wave, col, cm1, cm2, cm3);
                const float q = sac_pg_qhead(tile, Q, X.gscale, back, own, t);
                float* __restrict__ qo = c ? X.q2 : X.q1;
                if (own && qo) qo[row0 + t] = q;
                /* q1 waits in LDS for its own thread; then the word becomes the flag: a tie takes critic 1, a NaN on either side critic 2 */
                if (t < MLP_ROWS && X.twin) sel[t] = c ? (sel[t] <= q ? 1.f : 0.f) : q;
                if (back) {
                    __syncthreads();
                    mlp_backward_action(tile, Q, Dx, nullptr, 0, row0, lane, wave, col, cm1, cm2, cm3);
                }
            }
        }
        if (back) {
            /* the hand-back: ga in columns [Dx, Dx + A) -> g_mu | g_ls in columns [0, 2 A), in passes of 256 (row, unit) pairs of the head's map.  A
             * pass reads its ga one pass AHEAD of its writes: behind the barrier of pass k the ga of the passes up to k + 1 are in registers, so
             * the writes of pass k cannot reach a ga still to be read -- passes k and k + 2 share no row (A <= 128 < 256) */
            const float e = X.lscale * (X.d_alpha ? *X.d_alpha : X.alpha);
            const int n = MLP_ROWS * A;
            float cur = t < n ? tile[(t / A) * MLP_LD + Dx + t % A] : 0.f;
#pragma unroll 1
            for (int i = t; i - t < n; i += 256) {
                const int in = i + 256, rn = in / A;
                const float nxt = in < n ? tile[rn * MLP_LD + Dx + (in - rn * A)] : 0.f;
                if (headgrad) __syncthreads();                   /* the ga of this pass and of the next are read */
                if (i < n) {
                    const int r = i / A, j = i - r * A;
                    const long long row = row0 + r;
                    float gm = 0.f, gl = 0.f;
                    if (row < P.B) {
                        const float ga = X.twin && sel[r] != 0.f ? X.ga1[row * A + j] : cur;
                        if (X.ga) X.ga[row * X.gas + j] = ga;
                        if (headgrad) {
                            const float a = keep[row * ks + j], sdn = X.stash[row * X.ss + j];
                            const bool inr = X.stash[row * X.ss + A + j] != 0.f;
                            const float d = ga * fmaf(-a, a, 1.f);
                            gm = fmaf(2.f * e, a, d);
                            gl = inr ? fmaf(e, fmaf(2.f * a, sdn, -1.f), d * sdn) : 0.f;
                            if (X.ghead) { X.ghead[row * X.ghs + j] = gm; X.ghead[row * X.ghs + A + j] = gl; }
                            /* with grads the stash IS the actor's delta_{L-1} slot: the same pointer, so the stores stay behind the loads above */
                            if (G.grads) { X.stash[row * X.ss + j] = gm; X.stash[row * X.ss + A + j] = gl; }
                        }
                    }
                    if (headgrad) { tile[r * MLP_LD + j] = gm; tile[r * MLP_LD + A + j] = gl; }
                }
                cur = nxt;
            }
            if (G.grads) {
                __syncthreads();
                mlp_backward(tile, P, G, row0, lane, wave, col, am1, am2, am3);
            }
        }
        __syncthreads();                                         /* the next tile's rows overwrite this one's */
    }
}
hipError_t pmg_launch_sac_policy_grad(const PmgMlp& P, const PmgMlp& Q1, const PmgMlp& Q2, const PmgGrad& G, const PmgSacPolicy& head, const PmgGradChunks* C,
                                      const PmgSegs* T, hipStream_t s)
{
    if (P.B <= 0) return hipSuccess;
    PmgSacPolicy X = head;
    X.H.key = her_mix(X.H.seed ^ her_mix(X.H.counter + HER_GOLD));
    PmgMlpPair QQ;
    QQ.q[0] = Q1; QQ.q[1] = Q2;
    hipLaunchKernelGGL(pmg_k_sac_policy_grad_rows, dim3(mlp_grid(P.B)), dim3(256), 0, s, P, QQ, G, X);
    if (G.grads) {
        const MlpRawRows S = {G.x, G.xs};
        if (!C) hipLaunchKernelGGL((pmg_k_mlp_grad_weights<MlpRawRows>), dim3(pmg_grad_w_tiles(P)), dim3(64), 0, s, S, P, G);
        else {
            hipLaunchKernelGGL((pmg_k_mlp_grad_partials<MlpRawRows>), dim3((unsigned)(C->C * C->tiles)), dim3(64), 0, s, S, P, G, *C);
            hipLaunchKernelGGL(pmg_k_mlp_grad_merge, dim3(seg_grid(*T)), dim3(256), 0, s, *T, (const float*)C->part, C->C, C->P);
        }
    }
    return hipGetLastError();
}

/* SAC's temperature step (pmg_sac_alpha_device, DESIGN.md 3.16): one workgroup.  Thread t sums logp over the rows b = t (mod 256) in ascending
 * order from +0.0; thread 0 adds the 256 partial sums in ascending order from +0.0, forms g = -(total / B + target_entropy), takes pmg_k_adam's
 * step on log_alpha (adam_element restates that kernel's three expressions; the tests hold the two bit for bit) and stores alpha =
 * expf(log_alpha).  The quotient is formed in double and rounded to float: with 53 >= 2 * 24 + 2 bits that IS the correctly rounded float32
 * quotient, whatever the build does with float32 division. */
__device__ __forceinline__ void adam_element(const PmgAdam& A, float g, float& p, float& m, float& v)
{
    m = fmaf(A.beta1, m, A.omb1 * g);
    v = fmaf(A.beta2, v, A.omb2 * (g * g));
    p = p - A.step_size * (m / (sqrtf(v) * A.rsc2 + A.eps));
}
__global__ void __launch_bounds__(256) pmg_k_sac_alpha(PmgSacAlpha X)
{
    __shared__ float part[256];
    const int t = (int)threadIdx.x;
    float p = 0.f;
    for (long long b = t; b < X.B; b += 256) p = p + X.logp[b];
    part[t] = p;
    __syncthreads();
    if (t == 0) {
        float total = 0.f;
        for (int i = 0; i < 256; i++) total = total + part[i];
        const float g = -((float)((double)total / (double)(float)X.B) + X.target_entropy);
        float la = X.state[0], m = X.state[1], v = X.state[2];
        adam_element(X.A, g, la, m, v);
        X.state[0] = la; X.state[1] = m; X.state[2] = v; X.state[3] = expf(la);
    }
}
hipError_t pmg_launch_sac_alpha(const PmgSacAlpha& X, hipStream_t s)
{
    hipLaunchKernelGGL(pmg_k_sac_alpha, dim3(1), dim3(256), 0, s, X);
    return hipGetLastError();
}

/* PPO on whole rollouts (pmg_gae_device, pmg_adv_stats_device, pmg_adv_apply_device, pmg_ppo_policy_grad_device, pmg_ppo_stats_device;
 * DESIGN.md 3.19).
 * Generalised advantage estimation: a thread per env runs t = T-1 ... 0 as ONE chain; the loads of a step do not depend on the chain, so the
 * unrolled loop keeps four steps' loads in flight.  Time-major tables put consecutive envs on consecutive lanes (coalesced); any other layout
 * is the same code at its strides. */
__device__ __forceinline__ float gae_at(const PmgGaeTable& a, long long t, long long i) { return a.p[t * a.ts + i * a.es]; }
__global__ void __launch_bounds__(256) pmg_k_gae(PmgGae X)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= X.N) return;
    float adv = 0.f;
#pragma unroll 4
    for (long long t = X.T - 1; t >= 0; t--) {
        const float r = gae_at(X.reward, t, i), v = gae_at(X.value, t, i);
        float nv = gae_at(X.value_next, t, i);
        if (X.term.p && gae_at(X.term, t, i) != 0.f) nv = 0.f;
        const bool cut = t == X.T - 1 || (X.cut.p && gae_at(X.cut, t, i) != 0.f);
        const float delta = fmaf(X.gamma, nv, r) - v;
        adv = cut ? delta : fmaf(X.gl, adv, delta);
        X.adv[t * X.ats + i * X.aes] = adv;
        if (X.ret) X.ret[t * X.rts + i * X.res] = adv + v;
    }
}
hipError_t pmg_launch_gae(const PmgGae& X, hipStream_t s)
{
    if (X.T <= 0 || X.N <= 0) return hipSuccess;
    hipLaunchKernelGGL(pmg_k_gae, dim3((unsigned)((X.N + 255) / 256)), dim3(256), 0, s, X);
    return hipGetLastError();
}
/* THE two-level chain of the one-workgroup statistics (pmg_k_adv_stats in double, pmg_k_ppo_stats in float; pmg_k_sac_alpha's shape, K sums
 * at once): thread t brings the K partial sums p of the elements b = t (mod 256); thread 0 adds the 256 partial sums of each in ascending
 * order from +0.0 into total (other threads' total is not written).  One barrier; part is free again behind the caller's next one. */
template <class T, int K>
__device__ __forceinline__ void chain256(T (*part)[256], int t, const T (&p)[K], T (&total)[K])
{
#pragma unroll
    for (int k = 0; k < K; k++) part[k][t] = p[k];
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            T acc = (T)0;
            for (int i = 0; i < 256; i++) acc = acc + part[k][i];
            total[k] = acc;
        }
    }
}
/* mean and 1 / (std + eps) of M floats, accumulated in double: x * x is exact in double, so q's fma is one rounding however it is built */
__global__ void __launch_bounds__(256) pmg_k_adv_stats(PmgAdvStats X)
{
    __shared__ double part[2][256];
    const int t = (int)threadIdx.x;
    double p[2] = {0.0, 0.0}, tot[2] = {0.0, 0.0};
    for (long long b = t; b < X.M; b += 256) {
        const double x = (double)X.x[b];
        p[0] = p[0] + x;
        p[1] = fma(x, x, p[1]);
    }
    chain256<double, 2>(part, t, p, tot);
    if (t == 0) {
        const double M = (double)X.M, mean = tot[0] / M;
        const double var = fmax((tot[1] - tot[0] * mean) / (M - (double)X.ddof), 0.0);
        X.stats[0] = (float)mean;
        X.stats[1] = (float)(1.0 / (sqrt(var) + (double)X.eps));
    }
}
hipError_t pmg_launch_adv_stats(const PmgAdvStats& X, hipStream_t s)
{
    hipLaunchKernelGGL(pmg_k_adv_stats, dim3(1), dim3(256), 0, s, X);
    return hipGetLastError();
}
/* y = (x - mean) * inv, the statistics read from device memory; y may be x: an element is read and written by one thread */
__global__ void __launch_bounds__(256) pmg_k_adv_apply(const float* x, long long M, const float* __restrict__ stats, float* y)
{
    const float mean = stats[0], inv = stats[1];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long long)gridDim.x * 256) y[i] = (x[i] - mean) * inv;
}
hipError_t pmg_launch_adv_apply(const float* x, long long M, const float* stats, float* y, hipStream_t s)
{
    if (M <= 0) return hipSuccess;
    const long long want = (M + 255) / 256;
    hipLaunchKernelGGL(pmg_k_adv_apply, dim3((unsigned)(want < (1 << 20) ? want : (1 << 20))), dim3(256), 0, s, x, M, stats, y);
    return hipGetLastError();
}
/* PPO's actor update in one call (pmg_ppo_policy_grad_device), pmg_k_sac_policy_grad_rows' sibling without critics: gather, the actor's
 * layers (mlp_layers_saved), the clipped-surrogate head in two passes of pmg_k_sac's (row, unit j < A) map with the row's sum between them,
 * the actor's transposed layers, then the weights kernel of 3.11 (or the partials / merge pair of 3.12), unchanged, on the actor's workspace.
 * Ownership.  The tile holds z: means in columns [0, A), raw log-stds in [A, 2 A).  In BOTH passes the thread of (row, unit j) touches columns
 * j and A + j of its row and no other (another unit j' of the row touches j' and A + j', and j' != j, A + j' != j as j < A), so neither pass
 * needs a barrier inside.  Pass 1 reads m and the raw log-std, puts the summand ln_j - lo_j of the log-ratio into column j and LEAVES the raw
 * log-std in column A + j (pass 2 takes the clamp's predicate from it); w and isd go to X.stash, two floats per (row, unit) -- the actor's
 * delta_{L-1} slot, or d_ghead without grads -- where the SAME thread reads them back in pass 2 and overwrites them with g_mu | g_ls: a thread
 * reads only its own earlier stores, so no ordering between threads is involved.
 * Barriers.  The one behind pass 1 orders every summand before the sum of the row's thread (t < 32), which writes the row's k into rowk[t],
 * LDS beside the tile.  The one behind the sum orders (a) the sum's reads of columns [0, A) before the hand-back of g_mu into them and (b) rowk
 * before its readers.  The one behind pass 2 orders g_mu | g_ls in columns [0, 2 A) before the actor's first transposed chain, and the closing
 * one everything before the next tile's gather (and rowk's readers before its next writers).
 * Stale tile.  Pass 2 writes columns [0, 2 A) of ALL 32 rows, +0.0 in the rows past the batch (pass 1 leaves those rows alone: nothing reads
 * them); 2 A is even, so the first transposed chain reads no padding column, and whatever a wider hidden layer left beyond 2 A is not read:
 * mlp_backward's own write-backs cover whole strips from there on. */
__global__ void __launch_bounds__(256, 2) pmg_k_ppo_policy_grad_rows(PmgMlp P, PmgGrad G, PmgPpoPolicy X)
{
    __shared__ float tile[MLP_ROWS * MLP_LD];
    __shared__ float rowk[MLP_ROWS];                             /* k of row r of the tile, written by its thread between the passes */
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31;
    const int Dx = P.width[0], A = P.width[P.L] >> 1;
    const MlpRawRows S = {G.x, G.xs};
    const bool second = X.stash != nullptr;                      /* g_mu | g_ls are wanted: d_ghead or grads */
    const long long ntiles = (P.B + MLP_ROWS - 1) / MLP_ROWS;
    for (long long tb = blockIdx.x; tb < ntiles; tb += gridDim.x) {
        const long long row0 = tb * MLP_ROWS;
        mlp_gather(tile, S, row0, P.B, Dx, (Dx + 1) & ~1, t);
        __syncthreads();
        unsigned int m1 = 0, m2 = 0, m3 = 0;
        mlp_layers_saved(tile, P, G, row0, lane, wave, col, m1, m2, m3);
        for (int i = t; i < MLP_ROWS * A; i += 256) {            /* pass 1: both policies at the recorded u */
            const int r = i / A, j = i - r * A;
            const long long row = row0 + r;
            if (row >= P.B) break;
            const float m = tile[r * MLP_LD + j], ls = fminf(fmaxf(tile[r * MLP_LD + A + j], X.ls_lo), X.ls_hi);
            const float n = X.n[row * X.ns + j], lso = fminf(fmaxf(X.zo[row * X.zos + A + j], X.ls_lo), X.ls_hi);
            const float u = fmaf(expf(lso), n, X.zo[row * X.zos + j]);   /* sac_head's u */
            const float lo = fmaf(-0.5f * n, n, -lso);
            const float isd = expf(-ls), w = (u - m) * isd;
            const float ln = fmaf(-0.5f * w, w, -ls);
            tile[r * MLP_LD + j] = ln - lo;
            if (second) { X.stash[row * X.ss + j] = w; X.stash[row * X.ss + A + j] = isd; }
        }
        __syncthreads();                                         /* every summand of the tile is written */
        if (t < MLP_ROWS && row0 + t < P.B) {
            const long long row = row0 + t;
            const float lr = sac_logp(tile, t, A), rho = expf(lr), adv = X.adv[row];
            const bool clipped = (adv > 0.f && rho > X.clip_hi) || (adv < 0.f && rho < X.clip_lo);
            rowk[t] = clipped ? 0.f : (X.pscale * adv) * rho;
            if (X.ratio) X.ratio[row] = rho;
            if (X.logratio) X.logratio[row] = lr;
            if (X.clipped) X.clipped[row] = clipped ? 1 : 0;
        }
        if (second) {
            __syncthreads();                                     /* the sums are read: columns [0, A) are free; rowk is written */
            for (int i = t; i < MLP_ROWS * A; i += 256) {        /* pass 2: the hand-back, all 32 rows */
                const int r = i / A, j = i - r * A;
                const long long row = row0 + r;
                float gm = 0.f, gl = 0.f;
                if (row < P.B) {
                    const float k = rowk[r], w = X.stash[row * X.ss + j], isd = X.stash[row * X.ss + A + j], raw = tile[r * MLP_LD + A + j];
                    gm = k * (w * isd);
                    gl = (raw >= X.ls_lo && raw <= X.ls_hi) ? fmaf(k, fmaf(w, w, -1.f), X.escale) : 0.f;
                    if (X.ghead) { X.ghead[row * X.ghs + j] = gm; X.ghead[row * X.ghs + A + j] = gl; }
                    /* with grads the stash IS the actor's delta_{L-1} slot: the stores stay behind the loads above */
                    if (G.grads) { X.stash[row * X.ss + j] = gm; X.stash[row * X.ss + A + j] = gl; }
                }
                tile[r * MLP_LD + j] = gm;
                tile[r * MLP_LD + A + j] = gl;
            }
            if (G.grads) {
                __syncthreads();
                mlp_backward(tile, P, G, row0, lane, wave, col, m1, m2, m3);
            }
        }
        __syncthreads();                                         /* the next tile's rows overwrite this one's */
    }
}
hipError_t pmg_launch_ppo_policy_grad(const PmgMlp& P, const PmgGrad& G, const PmgPpoPolicy& X, const PmgGradChunks* C, const PmgSegs* T, hipStream_t s)
{
    if (P.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(pmg_k_ppo_policy_grad_rows, dim3(mlp_grid(P.B)), dim3(256), 0, s, P, G, X);
    if (G.grads) {
        const MlpRawRows S = {G.x, G.xs};
        if (!C) hipLaunchKernelGGL((pmg_k_mlp_grad_weights<MlpRawRows>), dim3(pmg_grad_w_tiles(P)), dim3(64), 0, s, S, P, G);
        else {
            hipLaunchKernelGGL((pmg_k_mlp_grad_partials<MlpRawRows>), dim3((unsigned)(C->C * C->tiles)), dim3(64), 0, s, S, P, G, *C);
            hipLaunchKernelGGL(pmg_k_mlp_grad_merge, dim3(seg_grid(*T)), dim3(256), 0, s, *T, (const float*)C->part, C->C, C->P);
        }
    }
    return hipGetLastError();
}
/* the four means a PPO learner logs (pmg_ppo_stats_device): chain256 in float, the quotients in double as pmg_k_sac_alpha forms its own */
__global__ void __launch_bounds__(256) pmg_k_ppo_stats(PmgPpoStats X)
{
    __shared__ float part[4][256];
    const int t = (int)threadIdx.x;
    float p[4] = {0.f, 0.f, 0.f, 0.f}, tot[4] = {0.f, 0.f, 0.f, 0.f};
    for (long long b = t; b < X.B; b += 256) {
        const float rho = X.ratio[b], lr = X.logratio[b], adv = X.adv[b];
        const float cr = fminf(fmaxf(rho, X.clip_lo), X.clip_hi);
        p[0] = p[0] + ((rho - 1.f) - lr);
        p[1] = p[1] + (X.clipped[b] ? 1.f : 0.f);
        p[2] = p[2] + fminf(rho * adv, cr * adv);
        p[3] = p[3] + lr;
    }
    chain256<float, 4>(part, t, p, tot);
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) X.stats[k] = (float)((double)tot[k] / (double)(float)X.B);
    }
}
hipError_t pmg_launch_ppo_stats(const PmgPpoStats& X, hipStream_t s)
{
    hipLaunchKernelGGL(pmg_k_ppo_stats, dim3(1), dim3(256), 0, s, X);
    return hipGetLastError();
}
