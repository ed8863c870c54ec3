/* pmg_gpu_probe.hip -- TEST INFRASTRUCTURE: small probe kernels that run single primitives of the SHIPPED pmg_wave.h and
 * single device functions of pmg_device.h / pmg_contact.h on a real gfx950, compiled with the product's own flags
 * (Makefile), so that tests/test_gpu_wave_primitives.py and tests/test_gpu_device_functions.py can compare each of them
 * with its model / the float64 oracle directly instead of through a whole rollout.  Never part of the product.
 *
 * Every probe is finite and masks every index it derives from its arguments, and every probe but one is ONE workgroup: the plan
 * probe (pmgd_plan) runs the grids of pmg_launch_plan, up to ceil(131 072 / 1024) = 128 workgroups of 1024 threads at its largest
 * batch (65 for the 65 792 envs the tests go to).  Every exported function allocates, launches on the null stream, synchronises,
 * copies back and returns the HIP status (< 0: bad arguments, nothing launched).
 * Built twice: as is (the inline-asm DPP paths that ship) and with -DPMG_NO_R0_DPP -DPMG_NO_DPP_FMAC -DPMG_NO_NEWBCAST
 * (the plain C++ branches of the same header), same symbols, two libraries. */
#include <hip/hip_runtime.h>
#include <cstring>
#include "pmg_kernels.h"   /* (pmg_contact.h, and the step bodies for the reach row set-up) */
#include "pmg_plan_probe.inc"

#define WV wv
#define PRIM_FN prim_probe_wv
#define PRIM_WR 0
#include "pmg_prim_probe.inc"
#undef WV
#undef PRIM_FN
#undef PRIM_WR
#define WV wr
#define PRIM_FN prim_probe_wr
#define PRIM_WR 1
#include "pmg_prim_probe.inc"
#undef WV
#undef PRIM_FN
#undef PRIM_WR

#define WV wv
#define NSP pmg
#define LEAN_FN lean_probe_wv
#define FK_FN fk_probe_wv
#define IK_FN ik_probe_wv
#include "pmg_lean_probe.inc"
#undef WV
#undef NSP
#undef LEAN_FN
#undef FK_FN
#undef IK_FN
#define WV wr
#define NSP pmgp
#define LEAN_FN lean_probe_wr
#define FK_FN fk_probe_wr
#define IK_FN ik_probe_wr
#include "pmg_lean_probe.inc"
#undef WV
#undef NSP
#undef LEAN_FN
#undef FK_FN
#undef IK_FN

namespace {

/* device buffers of one call: freed on every path */
struct Dev {
    void* p[12];
    int n = 0;
    hipError_t err = hipSuccess;
    template <class T>
    T* up(const T* h, size_t count)          /* allocate and fill from the host (h == nullptr: zeros) */
    {
        void* d = nullptr;
        if (err != hipSuccess || n >= 12) { if (err == hipSuccess) err = hipErrorOutOfMemory; return nullptr; }
        err = hipMalloc(&d, count * sizeof(T) ? count * sizeof(T) : 4);
        if (err != hipSuccess) return nullptr;
        p[n++] = d;
        err = h ? hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice) : hipMemset(d, 0, count * sizeof(T));
        return (T*)d;
    }
    template <class T>
    void down(T* h, const T* d, size_t count)
    {
        if (err == hipSuccess) err = hipMemcpy(h, d, count * sizeof(T), hipMemcpyDeviceToHost);
    }
    void sync()
    {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    ~Dev() { for (int i = 0; i < n; i++) (void)hipFree(p[i]); }
};

/* ---- primitives ------------------------------------------------------------------------------------------------ */
/* wave: the wavefront of the workgroup that runs the probe (the others leave at once: the helper wavefronts of the list-0
 * kernels).  rowsel < 0: all 64 lanes together; 0..3: that 16-lane row alone; 4: the four rows one after the other, each
 * in its own divergent branch (the packed layout's "control flow diverges by row") */
template <bool WR>
__global__ void __launch_bounds__(192) k_prim(int fam, int wave, int rowsel, int src, const float* in, float* out)
{
    const int t = (int)threadIdx.x;
    if ((t >> 6) != wave) return;
    const int row = (t >> 4) & 3;
    const int k0 = rowsel == 4 ? 0 : rowsel, k1 = rowsel == 4 ? 3 : rowsel;
    for (int k = k0; k <= k1; k++)
        if (k < 0 || row == k) {
            if (WR) prim_probe_wr(fam, src, in, out);
            else prim_probe_wv(fam, src, in, out);
        }
}

/* ---- the matrix-pipe primitive: one wavefront, every lane alive (prim::mfma_chain) ------------------------------------- */
__global__ void __launch_bounds__(64) k_mfma(int n, int steps, const float* a, const float* b, const float* c, float* out)
{
    prim::mfma_chain(n, steps, a, b, c, out);
}

/* ---- the reach row set-up: one wavefront, the product's contact store (prim::rowsetup_cases) ----------------------------- */
__global__ void __launch_bounds__(64) k_rowsetup(int n, const float* q, const float* qd, const float* con, const float* mu, const int* ncs, float* coef, float* resp,
                                                 float* misc, float* S_out, float* minv_out)
{
    __shared__ pmg::ContactLds<0, 8> L;
    __shared__ pmg::LaneTabStore lcs;
    prim::rowsetup_cases(L, lcs, n, q, qd, con, mu, ncs, coef, resp, misc, S_out, minv_out);
}

/* ---- dynamics / IK: the bodies of pmge_probe_dynamics / pmge_probe_ik (tests/emu/pmg_probe.cpp), case after case ---- */
#define DYN_BODY(NSP, WVN, CASE, VALID)                                                                                    \
    {                                                                                                                     \
        using namespace NSP;                                                                                              \
        const int l = WVN::lane();                                                                                        \
        const float ql = l < NJ ? q[9 * (CASE) + l] : 0.f, qdl = l < NJ ? qd[9 * (CASE) + l] : 0.f, tl = l < NJ ? tau[9 * (CASE) + l] : 0.f; \
        Kin k;                                                                                                            \
        fk(c, ql, k);                                                                                                     \
        float tip[3], Rt[9];                                                                                              \
        tip_frame(k, tip, Rt);                                                                                            \
        float I10[10], minv[NJ];                                                                                          \
        body_inertia(c, k, I10);                                                                                          \
        if (l >= NJ)                                                                                                      \
            for (int a = 0; a < 10; a++) I10[a] = 0.f;                                                                    \
        mass_inverse(k, I10, minv);                                                                                       \
        const float h = bias_torque(c, k, I10, qdl);                                                                      \
        const float rq = l < NJ ? tl - h : 0.f;                                                                           \
        float acc = 0.f;                                                                                                  \
        for (int j = 0; j < NJ; j++) acc += minv[j] * WVN::bcast(rq, j);                                                  \
        if ((VALID) && l < NJ) {                                                                                          \
            qdd[9 * (CASE) + l] = acc;                                                                                    \
            for (int j = 0; j < NJ; j++) minv_out[81 * (CASE) + 9 * l + j] = minv[j];                                     \
        }                                                                                                                 \
        if ((VALID) && l == 0) {                                                                                          \
            for (int a = 0; a < 3; a++) tip_out[12 * (CASE) + a] = tip[a];                                                \
            for (int a = 0; a < 9; a++) tip_out[12 * (CASE) + 3 + a] = Rt[a];                                             \
        }                                                                                                                 \
    }

__global__ void __launch_bounds__(64) k_dynamics(int n, const float* q, const float* qd, const float* tau, float* qdd, float* minv_out, float* tip_out)
{
    __shared__ pmg::LaneTabStore lcs;
    pmg::LaneConst c;
    pmg::load_lane_const(lcs, c);
    for (int i = 0; i < n; i++) DYN_BODY(pmg, wv, i, true)
}
/* the packed reach layout: four cases at once, one per 16-lane row */
__global__ void __launch_bounds__(64) k_dynamics_packed(int n, const float* q, const float* qd, const float* tau, float* qdd, float* minv_out, float* tip_out)
{
    __shared__ pmgp::LaneTabStore lcs;
    pmgp::LaneConst c;
    pmgp::load_lane_const(lcs, c);
    for (int i = 0; i < n; i += 4) {
        const int mine = i + wr::row();
        const bool valid = mine < n;
        const int cs = valid ? mine : n - 1;           /* (a row without a case repeats the last one and stores nothing) */
        DYN_BODY(pmgp, wr, cs, valid)
    }
}
__global__ void __launch_bounds__(64) k_ik(int n, const float* q, const float* target, float* q_out)
{
    using namespace pmg;
    __shared__ LaneTabStore lcs;
    LaneConst c;
    load_lane_const(lcs, c);
    const int l = wv::lane();
    for (int i = 0; i < n; i++) {
        const float r = ik_solve(c, l < NJ ? q[9 * i + l] : 0.f, target + 3 * i);
        if (l < NJ) q_out[9 * i + l] = r;
    }
}
__global__ void __launch_bounds__(64) k_ik_packed(int n, const float* q, const float* target, float* q_out)
{
    using namespace pmgp;
    __shared__ LaneTabStore lcs;
    LaneConst c;
    load_lane_const(lcs, c);
    const int l = wr::lane();
    for (int i = 0; i < n; i += 4) {
        const int mine = i + wr::row();
        const bool valid = mine < n;
        const int cs = valid ? mine : n - 1;
        const float r = ik_solve(c, l < NJ ? q[9 * cs + l] : 0.f, target + 3 * cs);
        if (valid && l < NJ) q_out[9 * cs + l] = r;
    }
}

/* ---- PMG_IK_LEAN: the lean primitives, fk() in float32 and ik_solve() in either layout (pmg_lean_probe.inc) ---------------- */
template <bool WR>
__global__ void __launch_bounds__(64) k_lean_prim(int fam, const float* in, float* out)
{
    if (WR) lean_probe_wr(fam, in, out);
    else lean_probe_wv(fam, in, out);
}
__global__ void __launch_bounds__(64) k_fk32(int n, const float* q, float* out)
{
    __shared__ pmg::LaneTabStore lcs;
    fk_probe_wv(lcs, n, q, out);
}
__global__ void __launch_bounds__(64) k_fk32_packed(int n, const float* q, float* out)
{
    __shared__ pmgp::LaneTabStore lcs;
    fk_probe_wr(lcs, n, q, out);
}

/* ---- narrowphase: one pair per lane, every operand in LDS as in the product (tools/prof_narrow.hip's layout) ---------- */
constexpr int PAIR_FLOATS = 30;   /* ca3 Ra9 ha3 cb3 Rb9 hb3 */
__global__ void __launch_bounds__(64) k_narrow(int kind, int np, const float* pairs, float margin, float* outp, int* nout, float* ambp)
{
    __shared__ __attribute__((aligned(16))) float A[64][12], B[64][12], hA[64][4], hB[64][4], out[64][4 * pmg::CP], W[64][pmg::BOX_WORK];
    const int l = (int)threadIdx.x & 63;
    np = np < 64 ? np : 64;
    if (l < np) {
        const float* p = pairs + PAIR_FLOATS * l;
        for (int a = 0; a < 12; a++) { A[l][a] = p[a]; B[l][a] = p[15 + a]; }
        for (int a = 0; a < 3; a++) { hA[l][a] = p[12 + a]; hB[l][a] = p[27 + a]; }
        for (int a = 0; a < 4 * pmg::CP; a++) out[l][a] = 0.f;
    }
    __syncthreads();
    int n = 0;
    float amb = 1e30f;
    if (l < np) {
        if (kind == 0) n = pmg::box_box_fast(A[l], A[l] + 3, hA[l], B[l], B[l] + 3, hB[l], margin, out[l], W[l]);
        else if (kind == 2) n = pmg::box_box(A[l], A[l] + 3, hA[l], B[l], B[l] + 3, hB[l], margin, out[l], W[l]);
        else if (kind == 3) n = pmg::box_box_fast<true, true>(A[l], A[l] + 3, hA[l], B[l], B[l] + 3, hB[l], margin, out[l], W[l]);
        else n = pmg::cyl_box(A[l], A[l] + 3, hA[l][0], hA[l][2], B[l], B[l] + 3, hB[l][0], hB[l][1], hB[l][2], margin, out[l], W[l], &amb);
    }
    wv::lds_sync();
    if (l < np) {
        n = n < 0 ? 0 : (n > 4 ? 4 : n);
        for (int a = 0; a < 4 * pmg::CP; a++) outp[4 * pmg::CP * l + a] = out[l][a];
        nout[l] = n;
        ambp[l] = amb;
    }
}

/* ---- the double-precision helpers of the cylinder repeat: one case per lane ----------------------------------------- */
__global__ void __launch_bounds__(64) k_fk64(int n, const float* q9, const int* body, double* p, double* R)
{
    const int l = (int)threadIdx.x & 63;
    for (int i = l; i < n; i += 64) {
        const int b = body[i];
        const int bb = (b == pmg::BODY_FINGER1 || b == pmg::BODY_FINGER2) ? b : pmg::BODY_GBASE;
        pmg::fk64_link(q9 + 9 * i, bb, p + 3 * i, R + 9 * i);
    }
}
__global__ void __launch_bounds__(64) k_cyl_redo64(int n, int ck, const float* q9, const float* blk, const float* doorq, const float* kc, float prad, float phl,
                                                   float* outp, int* nout)
{
    __shared__ __attribute__((aligned(16))) float out[64][4 * pmg::CP], W[64][pmg::BOX_WORK];
    const int l = (int)threadIdx.x & 63;
    n = n < 64 ? n : 64;
    if (l < n) {
        for (int a = 0; a < 4 * pmg::CP; a++) out[l][a] = 0.f;
        int m;
        /* the slide puck (free body 0) against the table alone; every other pair: k_cyl_redo64_pairs */
        if (ck == 0) m = pmg::cyl_redo64<0>(0, pmg::BODY_STATIC, -1, q9 + 9 * l, blk + pmg::BLOCK_DIM * l, doorq + l, kc, prad, phl, out[l], W[l]);
        else if (ck == 1) m = pmg::cyl_redo64<1>(0, pmg::BODY_STATIC, -1, q9 + 9 * l, blk + pmg::BLOCK_DIM * l, doorq + l, kc, prad, phl, out[l], W[l]);
        else m = pmg::cyl_redo64<-1>(0, pmg::BODY_STATIC, -1, q9 + 9 * l, blk + pmg::BLOCK_DIM * l, doorq + l, kc, prad, phl, out[l], W[l]);
        m = m < 0 ? 0 : (m > 4 ? 4 : m);
        for (int a = 0; a < 4 * pmg::CP; a++) outp[4 * pmg::CP * l + a] = out[l][a];
        nout[l] = m;
    }
}

/* cyl_redo64 on ANY of the pairs collide() hands it: one case per lane, the lanes of a launch carrying different kinds of pair,
 * so that the out-of-line callee is entered divergently as in collide().  ids: cyl_body, box_body, wall, handed per case (checked
 * by the host entry); blk: TWO free-body rows per case.  handed: the lane first derives its robot body's double pose the way
 * spec_fk does -- sincos64 per arm joint into a table in LDS, fk64_chain with that table -- and hands it in (spec_pairs) */
constexpr int REDO_IDS = 4, REDO_ROWS = 2;
__device__ __forceinline__ int redo_robot_body(int cyl_body, int box_body)
{
    if (cyl_body == pmg::BODY_GBASE) return pmg::BODY_GBASE;
    return (box_body == pmg::BODY_FINGER1 || box_body == pmg::BODY_FINGER2) ? box_body : -1;
}
template <int CK>
__device__ __forceinline__ int redo_pair(const int* id, const float* q9, const float* blk, const float* doorq, const float* kc, float prad, float phl, float* out, float* W,
                                         double (*sc)[2])
{
    const int rb = redo_robot_body(id[0], id[1]);
    if (id[3] && rb >= 0) {
        double p[3], R[9];
        for (int j = 0; j < 7; j++) pmg::sincos64((double)q9[j], sc[j][0], sc[j][1]);
        pmg::fk64_chain(q9, sc, rb, p, R);
        return pmg::cyl_redo64<CK>(id[0], id[1], id[2], q9, blk, doorq, kc, prad, phl, out, W, p, R);
    }
    return pmg::cyl_redo64<CK>(id[0], id[1], id[2], q9, blk, doorq, kc, prad, phl, out, W);
}
__global__ void __launch_bounds__(64) k_cyl_redo64_pairs(int n, int ck, const int* ids, const float* q9, const float* blk, const float* doorq, const float* kc, float prad,
                                                         float phl, float* outp, int* nout)
{
    __shared__ __attribute__((aligned(16))) float out[64][4 * pmg::CP], W[64][pmg::BOX_WORK];
    __shared__ double sc[64][7][2];
    const int l = (int)threadIdx.x & 63;
    n = n < 64 ? n : 64;
    if (l < n) {
        for (int a = 0; a < 4 * pmg::CP; a++) out[l][a] = 0.f;
        const int* id = ids + REDO_IDS * l;
        const float *q = q9 + 9 * l, *b = blk + REDO_ROWS * pmg::BLOCK_DIM * l;
        int m;
        if (ck == 0) m = redo_pair<0>(id, q, b, doorq + l, kc, prad, phl, out[l], W[l], sc[l]);
        else if (ck == 1) m = redo_pair<1>(id, q, b, doorq + l, kc, prad, phl, out[l], W[l], sc[l]);
        else m = redo_pair<-1>(id, q, b, doorq + l, kc, prad, phl, out[l], W[l], sc[l]);
        m = m < 0 ? 0 : (m > 4 ? 4 : m);
        for (int a = 0; a < 4 * pmg::CP; a++) outp[4 * pmg::CP * l + a] = out[l][a];
        nout[l] = m;
    }
}
/* the double arithmetic of the repeat, one element per lane.  op 0: t_sqrt(x) -> o0; 1: t_div(x, y) -> o0; 2: sincos64(x) -> o0, o1 */
__global__ void __launch_bounds__(64) k_double_maths(int op, int n, const double* x, const double* y, double* o0, double* o1)
{
    const int l = (int)threadIdx.x & 63;
    for (int i = l; i < n; i += 64) {
        if (op == 0) o0[i] = pmg::t_sqrt(x[i]);
        else if (op == 1) o0[i] = pmg::t_div(x[i], y[i]);
        else pmg::sincos64(x[i], o0[i], o1[i]);
    }
}


/* ---- the launch plan: the product's four plan kernels under other names, same bounds, same bodies (pmg_kernels.hip) -------- */
__global__ void __launch_bounds__(1024) k_plan(pmg::EnvParams P, const float* __restrict__ actions) { pmg::plan_all(P, actions); }
__global__ void __launch_bounds__(1024) k_plan_reach(pmg::EnvParams P, const float* __restrict__ actions) { pmg::plan_all<true>(P, actions); }
__global__ void __launch_bounds__(1024) k_plan_count(pmg::EnvParams P, const float* __restrict__ actions) { pmg::plan_count(P, actions); }
__global__ void __launch_bounds__(1024) k_plan_scatter(pmg::EnvParams P, const float* __restrict__ actions) { pmg::plan_scatter(P, actions); }

}  // namespace

extern "C" {

/* which build this is: 0 = the shipped paths, 1 = the plain C++ branches */
int pmgd_variant()
{
#if defined(PMG_NO_R0_DPP) && defined(PMG_NO_DPP_FMAC) && defined(PMG_NO_NEWBCAST)
    return 1;
#else
    return 0;
#endif
}
int pmgd_prim_nin() { return prim::NIN; }
int pmgd_prim_nout() { return prim::NOUT; }
int pmgd_prim_families() { return prim::F_COUNT; }

/* in [NIN][64], out [NOUT][64] (in and out: the caller's sentinel stays where the probe writes nothing) */
int pmgd_prim(int wr_ns, int fam, int threads, int wave, int rowsel, int src, const float* in, float* out)
{
    if ((threads != 64 && threads != 128 && threads != 192) || wave < 0 || wave >= threads / 64 || fam < 0 || fam >= prim::F_COUNT || rowsel < -1 || rowsel > 4)
        return -1;
    Dev d;
    const float* din = d.up(in, (size_t)prim::NIN * 64);
    float* dout = d.up(out, (size_t)prim::NOUT * 64);
    if (d.err == hipSuccess) {
        if (wr_ns) hipLaunchKernelGGL(k_prim<true>, dim3(1), dim3(threads), 0, 0, fam, wave, rowsel, src & 63, din, dout);
        else hipLaunchKernelGGL(k_prim<false>, dim3(1), dim3(threads), 0, 0, fam, wave, rowsel, src & 63, din, dout);
    }
    d.sync();
    d.down(out, dout, (size_t)prim::NOUT * 64);
    return (int)d.err;
}

/* wv::mfma_32x32x2, `steps` (1..8) chained calls per case: a, b [n][steps][64], c [n][16][64] -> out [n][16][64] */
int pmgd_mfma(int n, int steps, const float* a, const float* b, const float* c, float* out)
{
    if (n < 1 || n > prim::MFMA_MAX_CASES || steps < 1 || steps > prim::MFMA_MAX_STEPS) return -1;
    Dev d;
    const float *da = d.up(a, (size_t)n * steps * 64), *db = d.up(b, (size_t)n * steps * 64), *dc = d.up(c, (size_t)n * 16 * 64);
    float* dout = d.up<float>(nullptr, (size_t)n * 16 * 64);
    if (d.err == hipSuccess) hipLaunchKernelGGL(k_mfma, dim3(1), dim3(64), 0, 0, n, steps, da, db, dc, dout);
    d.sync();
    d.down(out, dout, (size_t)n * 16 * 64);
    return (int)d.err;
}

/* pmg::reach_rowspace_setup<0, 8> on n (1..64) cases: prim::rowsetup_cases for the arguments */
int pmgd_rowsetup(int n, const float* q, const float* qd, const float* con, const float* mu, const int* ncs, float* coef, float* resp, float* misc, float* S_out,
                  float* minv_out)
{
    if (n < 1 || n > prim::ROWSETUP_MAX_CASES) return -1;
    Dev d;
    const float *dq = d.up(q, 9 * (size_t)n), *dqd = d.up(qd, 9 * (size_t)n), *dcon = d.up(con, 96 * (size_t)n), *dmu = d.up(mu, 8 * (size_t)n);
    const int* dn = d.up(ncs, (size_t)n);
    float *dc = d.up<float>(nullptr, 64 * 24 * (size_t)n), *dr = d.up<float>(nullptr, 64 * 9 * (size_t)n), *dm = d.up<float>(nullptr, 64 * 4 * (size_t)n);
    float *dS = d.up<float>(nullptr, 54 * (size_t)n), *dmi = d.up<float>(nullptr, 81 * (size_t)n);
    if (d.err == hipSuccess) hipLaunchKernelGGL(k_rowsetup, dim3(1), dim3(64), 0, 0, n, dq, dqd, dcon, dmu, dn, dc, dr, dm, dS, dmi);
    d.sync();
    d.down(coef, dc, 64 * 24 * (size_t)n); d.down(resp, dr, 64 * 9 * (size_t)n); d.down(misc, dm, 64 * 4 * (size_t)n);
    d.down(S_out, dS, 54 * (size_t)n); d.down(minv_out, dmi, 81 * (size_t)n);
    return (int)d.err;
}
int pmgd_rowspace_mfma() { return PMG_ROWSPACE_MFMA; }
int pmgd_rowsetup_pipeline() { return PMG_ROWSETUP_PIPELINE; }

/* n cases: q, qd, tau [n][9] -> qdd [n][9], minv [n][81], tip [n][12] (position, rotation of the tip frame) */
int pmgd_dynamics(int packed, int n, const float* q, const float* qd, const float* tau, float* qdd, float* minv_out, float* tip_out)
{
    if (n < 1 || n > 4096) return -1;
    Dev d;
    const float *dq = d.up(q, 9 * (size_t)n), *dqd = d.up(qd, 9 * (size_t)n), *dt = d.up(tau, 9 * (size_t)n);
    float *da = d.up<float>(nullptr, 9 * (size_t)n), *dm = d.up<float>(nullptr, 81 * (size_t)n), *dp = d.up<float>(nullptr, 12 * (size_t)n);
    if (d.err == hipSuccess) {
        if (packed) hipLaunchKernelGGL(k_dynamics_packed, dim3(1), dim3(64), 0, 0, n, dq, dqd, dt, da, dm, dp);
        else hipLaunchKernelGGL(k_dynamics, dim3(1), dim3(64), 0, 0, n, dq, dqd, dt, da, dm, dp);
    }
    d.sync();
    d.down(qdd, da, 9 * (size_t)n); d.down(minv_out, dm, 81 * (size_t)n); d.down(tip_out, dp, 12 * (size_t)n);
    return (int)d.err;
}
int pmgd_ik(int packed, int n, const float* q, const float* target, float* q_out)
{
    if (n < 1 || n > 4096) return -1;
    Dev d;
    const float *dq = d.up(q, 9 * (size_t)n), *dt = d.up(target, 3 * (size_t)n);
    float* dout = d.up<float>(nullptr, 9 * (size_t)n);
    if (d.err == hipSuccess) {
        if (packed) hipLaunchKernelGGL(k_ik_packed, dim3(1), dim3(64), 0, 0, n, dq, dt, dout);
        else hipLaunchKernelGGL(k_ik, dim3(1), dim3(64), 0, 0, n, dq, dt, dout);
    }
    d.sync();
    d.down(q_out, dout, 9 * (size_t)n);
    return (int)d.err;
}
/* PMG_IK_LEAN of this build, and the probes of pmg_lean_probe.inc: in [NIN][64] -> out [NOUT][64] (in and out, as pmgd_prim) */
int pmgd_ik_lean() { return PMG_IK_LEAN; }
int pmgd_lean_prim(int wr_ns, int fam, const float* in, float* out)
{
    if (fam < 0 || fam >= prim::LEAN_FAMILIES) return -1;
    Dev d;
    const float* din = d.up(in, (size_t)prim::NIN * 64);
    float* dout = d.up(out, (size_t)prim::NOUT * 64);
    if (d.err == hipSuccess) {
        if (wr_ns) hipLaunchKernelGGL(k_lean_prim<true>, dim3(1), dim3(64), 0, 0, fam, din, dout);
        else hipLaunchKernelGGL(k_lean_prim<false>, dim3(1), dim3(64), 0, 0, fam, din, dout);
    }
    d.sync();
    d.down(out, dout, (size_t)prim::NOUT * 64);
    return (int)d.err;
}
/* fk() in float32: q [n][9] -> out [n][16][18] (R, p, S of the sixteen lanes of the env's row) */
int pmgd_fk(int packed, int n, const float* q, float* out)
{
    if (n < 1 || n > 4096) return -1;
    Dev d;
    const float* dq = d.up(q, 9 * (size_t)n);
    float* dout = d.up<float>(nullptr, 16 * prim::FK_ROW_FLOATS * (size_t)n);
    if (d.err == hipSuccess) {
        if (packed) hipLaunchKernelGGL(k_fk32_packed, dim3(1), dim3(64), 0, 0, n, dq, dout);
        else hipLaunchKernelGGL(k_fk32, dim3(1), dim3(64), 0, 0, n, dq, dout);
    }
    d.sync();
    d.down(out, dout, 16 * prim::FK_ROW_FLOATS * (size_t)n);
    return (int)d.err;
}

/* n pairs [n][30] (ca3 Ra9 ha3 cb3 Rb9 hb3; a cylinder A: ha = r, r, half length), `lanes` (1..64) of them per launch, one
 * per lane.  kind 0: box_box_fast, 1: cyl_box, 2: box_box, 3: box_box_fast<true, true>.  -> out [n][40], nout [n], amb [n] */
int pmgd_narrowphase(int kind, int n, int lanes, const float* pairs, float margin, float* out, int* nout, float* amb)
{
    if (kind < 0 || kind > 3 || n < 1 || n > 65536 || lanes < 1 || lanes > 64) return -1;
    Dev d;
    const float* dp = d.up(pairs, (size_t)PAIR_FLOATS * n);
    float *dout = d.up<float>(nullptr, 40 * (size_t)n), *damb = d.up<float>(nullptr, (size_t)n);
    int* dn = d.up<int>(nullptr, (size_t)n);
    for (int i = 0; i < n && d.err == hipSuccess; i += lanes) {
        const int np = n - i < lanes ? n - i : lanes;
        hipLaunchKernelGGL(k_narrow, dim3(1), dim3(64), 0, 0, kind, np, dp + (size_t)PAIR_FLOATS * i, margin, dout + 40 * (size_t)i, dn + i, damb + i);
        d.err = hipGetLastError();
    }
    d.sync();
    d.down(out, dout, 40 * (size_t)n); d.down(nout, dn, (size_t)n); d.down(amb, damb, (size_t)n);
    return (int)d.err;
}

/* fk64_link: q9 [n][9], body [n] (BODY_FINGER1 / 2, anything else: the gripper base) -> p [n][3], R [n][9] (double) */
int pmgd_fk64(int n, const float* q9, const int* body, double* p, double* R)
{
    if (n < 1 || n > 65536) return -1;
    Dev d;
    const float* dq = d.up(q9, 9 * (size_t)n);
    const int* db = d.up(body, (size_t)n);
    double *dp = d.up<double>(nullptr, 3 * (size_t)n), *dR = d.up<double>(nullptr, 9 * (size_t)n);
    if (d.err == hipSuccess) hipLaunchKernelGGL(k_fk64, dim3(1), dim3(64), 0, 0, n, dq, db, dp, dR);
    d.sync();
    d.down(p, dp, 3 * (size_t)n); d.down(R, dR, 9 * (size_t)n);
    return (int)d.err;
}
/* cyl_redo64<ck> of the puck (free body 0 of each case's state row) against the table only: q9 [n][9], blk [n][13], doorq [n],
 * kc [24] -> out [n][40], nout [n].  Every other pair the routine serves goes through pmgd_cyl_redo64_pairs below */
int pmgd_cyl_redo64(int n, int ck, const float* q9, const float* blk, const float* doorq, const float* kc, float prad, float phl, float* out, int* nout)
{
    if (n < 1 || n > 65536 || ck < -1 || ck > 1) return -1;
    Dev d;
    const float *dq = d.up(q9, 9 * (size_t)n), *db = d.up(blk, 13 * (size_t)n), *dd = d.up(doorq, (size_t)n), *dk = d.up(kc, 24);
    float* dout = d.up<float>(nullptr, 40 * (size_t)n);
    int* dn = d.up<int>(nullptr, (size_t)n);
    for (int i = 0; i < n && d.err == hipSuccess; i += 64) {
        const int np = n - i < 64 ? n - i : 64;
        hipLaunchKernelGGL(k_cyl_redo64, dim3(1), dim3(64), 0, 0, np, ck, dq + 9 * (size_t)i, db + 13 * (size_t)i, dd + i, dk, prad, phl, dout + 40 * (size_t)i, dn + i);
        d.err = hipGetLastError();
    }
    d.sync();
    d.down(out, dout, 40 * (size_t)n); d.down(nout, dn, (size_t)n);
    return (int)d.err;
}

/* cyl_redo64<ck> on any of its pairs, `lanes` (1..64) cases per launch, one per lane.  ids [n][4]: cyl_body (a free-body row 0 / 1,
 * BODY_GBASE or CYL64_HANDLE), box_body (a row 0 / 1, BODY_FINGER1 / 2, BODY_DOOR or BODY_STATIC), wall (-1: table / floor), handed
 * (0 / 1: the robot body's pose handed in as spec_pairs does); q9 [n][9], blk [n][2][13], doorq [n], kc [24] -> out [n][40], nout [n].
 * Ids the routine would index out of these arrays with (the handle, the door or a wall without a chest, a row beyond the second, a
 * wall the chest kind does not have) are refused here */
int pmgd_cyl_redo64_pairs(int n, int ck, int lanes, const int* ids, const float* q9, const float* blk, const float* doorq, const float* kc, float prad, float phl,
                          float* out, int* nout)
{
    if (n < 1 || n > 65536 || ck < -1 || ck > 1 || lanes < 1 || lanes > 64) return -1;
    for (int i = 0; i < n; i++) {
        const int cyl = ids[REDO_IDS * i], box = ids[REDO_IDS * i + 1], wall = ids[REDO_IDS * i + 2], handed = ids[REDO_IDS * i + 3];
        const bool row_c = cyl >= 0 && cyl < REDO_ROWS, row_b = box >= 0 && box < REDO_ROWS;
        if (!(row_c || cyl == pmg::BODY_GBASE || (cyl == pmg::CYL64_HANDLE && ck >= 0))) return -1;
        if (!(row_b || box == pmg::BODY_FINGER1 || box == pmg::BODY_FINGER2 || box == pmg::BODY_STATIC || (box == pmg::BODY_DOOR && ck >= 0))) return -1;
        if ((row_c && row_b && cyl == box) || (cyl == pmg::BODY_GBASE && (box == pmg::BODY_FINGER1 || box == pmg::BODY_FINGER2))) return -1;
        if (wall < -1 || wall >= (ck >= 0 ? pmg::ChestT::nwall(ck) : 0) || (wall >= 0 && box != pmg::BODY_STATIC)) return -1;
        if (handed != 0 && handed != 1) return -1;
    }
    Dev d;
    const int* di = d.up(ids, REDO_IDS * (size_t)n);
    const float *dq = d.up(q9, 9 * (size_t)n), *db = d.up(blk, REDO_ROWS * 13 * (size_t)n), *dd = d.up(doorq, (size_t)n), *dk = d.up(kc, 24);
    float* dout = d.up<float>(nullptr, 40 * (size_t)n);
    int* dn = d.up<int>(nullptr, (size_t)n);
    for (int i = 0; i < n && d.err == hipSuccess; i += lanes) {
        const int np = n - i < lanes ? n - i : lanes;
        hipLaunchKernelGGL(k_cyl_redo64_pairs, dim3(1), dim3(64), 0, 0, np, ck, di + REDO_IDS * (size_t)i, dq + 9 * (size_t)i, db + REDO_ROWS * 13 * (size_t)i, dd + i, dk,
                           prad, phl, dout + 40 * (size_t)i, dn + i);
        d.err = hipGetLastError();
    }
    d.sync();
    d.down(out, dout, 40 * (size_t)n); d.down(nout, dn, (size_t)n);
    return (int)d.err;
}
/* t_sqrt (op 0: x -> o0), t_div (1: x / y -> o0) and sincos64 (2: x -> sin o0, cos o1) in double on arrays of n */
int pmgd_double_maths(int op, int n, const double* x, const double* y, double* o0, double* o1)
{
    if (op < 0 || op > 2 || n < 1 || n > (1 << 20)) return -1;
    Dev d;
    const double *dx = d.up(x, (size_t)n), *dy = d.up(y, (size_t)n);
    double *d0 = d.up<double>(nullptr, (size_t)n), *d1 = d.up<double>(nullptr, (size_t)n);
    if (d.err == hipSuccess) hipLaunchKernelGGL(k_double_maths, dim3(1), dim3(64), 0, 0, op, n, dx, dy, d0, d1);
    d.sync();
    d.down(o0, d0, (size_t)n); d.down(o1, d1, (size_t)n);
    return (int)d.err;
}

/* The plan on the caller's buffer: pmge_plan of tests/emu/pmg_probe.cpp on the device (arguments and their check: pmg_plan_probe.inc).
 * mode 0: pmg_k_plan's body in one workgroup, 1: pmg_k_plan_reach's, 2: pmg_k_plan_count + pmg_k_plan_scatter over ceil(N / 1024)
 * workgroups -- the grids of pmg_launch_plan.  buf: [guard | Sched::words(N) | guard], in and out; every device array is sized
 * from the checked arguments and Sched::words */
int pmgd_plan(int mode, int n_envs, int nb, int chest, int joint_control, float near_r, float chest_reach, int fd_div, int wave_budget, int lpt_thresh, int lpt_permille,
              int lpt_parity, const int* env_cycles, int* lpt_state, const float* hot, const float* blocks, const float* actions, int adim, int guard, int* buf)
{
    if (!plan_args_ok(mode, n_envs, nb, chest, joint_control, lpt_thresh, lpt_permille, lpt_parity, env_cycles, lpt_state, hot, blocks, actions, adim, guard, buf)) return -1;
    const size_t N = (size_t)n_envs, words = pmgx::Sched::words(N) + 2 * (size_t)guard;
    pmg::EnvParams P = plan_params(n_envs, nb, chest, joint_control, near_r, chest_reach, fd_div, wave_budget, lpt_thresh, lpt_permille, lpt_parity, adim);
    Dev d;
    P.hot = const_cast<float*>(d.up(hot, N * pmg::HOT_DIM));
    P.blocks = nb > 0 ? const_cast<float*>(d.up(blocks, N * pmg::BLOCK_DIM * (size_t)nb)) : nullptr;
    const float* dact = d.up(actions, N * (size_t)adim);
    P.env_cycles = env_cycles ? const_cast<int*>(d.up(env_cycles, 2 * N)) : nullptr;
    P.lpt_state = lpt_state ? d.up(lpt_state, (size_t)(2 + pmg::LPT_BINS)) : nullptr;
    int* dbuf = d.up(buf, words);
    P.sched = dbuf + guard;
    if (d.err == hipSuccess) {
        const int nwg = (n_envs + pmg::PLAN_THREADS - 1) / pmg::PLAN_THREADS;
        if (mode == 0) hipLaunchKernelGGL(k_plan, dim3(1), dim3(pmg::PLAN_THREADS), 0, 0, P, dact);
        else if (mode == 1) hipLaunchKernelGGL(k_plan_reach, dim3(1), dim3(pmg::PLAN_THREADS), 0, 0, P, dact);
        else {
            hipLaunchKernelGGL(k_plan_count, dim3(nwg), dim3(pmg::PLAN_THREADS), 0, 0, P, dact);
            hipLaunchKernelGGL(k_plan_scatter, dim3(nwg), dim3(pmg::PLAN_THREADS), 0, 0, P, dact);
        }
    }
    d.sync();
    d.down(buf, dbuf, words);
    if (lpt_state) d.down(lpt_state, P.lpt_state, (size_t)(2 + pmg::LPT_BINS));
    return (int)d.err;
}

}  // extern "C"
