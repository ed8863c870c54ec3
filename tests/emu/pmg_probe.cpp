/* pmg_probe.cpp -- TEST INFRASTRUCTURE: runs individual device functions of
 * pybullet_multigoal_gym_amd/csrc/pmg_device.h on the fiber emulator so that unit tests can
 * compare them with the oracle's probes. */
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include "pmg_kernels.h"

/* the primitive probes of the device probe library (gpu_probe/), here against the emulator's stand-in header */
#define WV wv
#define PRIM_FN prim_probe_wv
#define PRIM_WR 0
#include "../../gpu_probe/pmg_prim_probe.inc"
#undef WV
#undef PRIM_FN
#undef PRIM_WR
#define WV wr
#define PRIM_FN prim_probe_wr
#define PRIM_WR 1
#include "../../gpu_probe/pmg_prim_probe.inc"
#undef WV
#undef PRIM_FN
#undef PRIM_WR

/* same arguments and lane contexts as pmgd_prim (gpu_probe/pmg_gpu_probe.hip) */
extern "C" int pmge_prim(int wr_ns, int fam, int threads, int wave, int rowsel, int src, const float* in, float* out)
{
    if ((threads != 64 && threads != 128 && threads != 192) || wave < 0 || wave >= threads / 64 || fam < 0 || fam >= prim::F_COUNT || rowsel < -1 || rowsel > 4)
        return -1;
    emu::launch(1, threads, [&]() {
        const int t = (int)threadIdx.x;
        if ((t >> 6) != wave) return;
        const int row = (t >> 4) & 3;
        const int k0 = rowsel == 4 ? 0 : rowsel, k1 = rowsel == 4 ? 3 : rowsel;
        for (int k = k0; k <= k1; k++)
            if (k < 0 || row == k) {
                if (wr_ns) prim_probe_wr(fam, src & 63, in, out);
                else prim_probe_wv(fam, src & 63, in, out);
            }
    });
    return 0;
}
extern "C" int pmge_prim_nin() { return prim::NIN; }
extern "C" int pmge_prim_nout() { return prim::NOUT; }
extern "C" int pmge_prim_families() { return prim::F_COUNT; }

extern "C" void pmge_probe_dynamics(const float* q, const float* qd, const float* tau, float* qdd, float* minv_out,
                                    float* tip_out)
{
    emu::launch(1, 64, [&]() {
        using namespace pmg;
        int l = wv::lane();
        __shared__ LaneTabStore lcs;
        LaneConst c;
        load_lane_const(lcs, c);
        float ql = l < NJ ? q[l] : 0.f, qdl = l < NJ ? qd[l] : 0.f, tl = l < NJ ? tau[l] : 0.f;
        Kin k;
        fk(c, ql, k);
        float tip[3], Rt[9];
        tip_frame(k, tip, Rt);
        float I10[10], minv[NJ], v[6];
        body_inertia(c, k, I10);
        if (l >= NJ)
            for (int a = 0; a < 10; a++) I10[a] = 0.f;
        mass_inverse(k, I10, minv);
        float h = bias_torque(c, k, I10, qdl);
        float rq = l < NJ ? tl - h : 0.f;
        float acc = 0.f;
        for (int j = 0; j < NJ; j++) acc += minv[j] * wv::bcast(rq, j);
        if (l < NJ) {
            qdd[l] = acc;
            for (int j = 0; j < NJ; j++) minv_out[9 * l + j] = minv[j];
        }
        if (l == 0) {
            for (int a = 0; a < 3; a++) tip_out[a] = tip[a];
            for (int a = 0; a < 9; a++) tip_out[3 + a] = Rt[a];
        }
    });
}

extern "C" int pmge_probe_ik(const float* q, const float* target, float* q_out)
{
    emu::launch(1, 64, [&]() {
        using namespace pmg;
        int l = wv::lane();
        __shared__ LaneTabStore lcs;
        LaneConst c;
        load_lane_const(lcs, c);
        float ql = l < NJ ? q[l] : 0.f;
        float r = ik_solve(c, ql, target);
        if (l < NJ) q_out[l] = r;
    });
    return 0;
}

/* device narrowphase on one pair (plain call: these functions use no cross-lane primitive).  kind 0: box_box_fast
 * (register front end, box_face_clip for partial face overlaps, box_box_resume for edges), 1: cyl_box with A = cylinder
 * (half = r, r, hl), 2: the general box_box alone, 3: box_box_fast with B's rotation known to be the identity.  out: n x 10 floats */
extern "C" int pmge_probe_narrowphase(int kind, const float* ca, const float* Ra, const float* ha, const float* cb, const float* Rb,
                                      const float* hb, float margin, float* out)
{
    alignas(16) static float W[256];
    if (kind == 0) return pmg::box_box_fast(ca, Ra, ha, cb, Rb, hb, margin, out, W);
    if (kind == 2) return pmg::box_box(ca, Ra, ha, cb, Rb, hb, margin, out, W);
    if (kind == 3) return pmg::box_box_fast<true, true>(ca, Ra, ha, cb, Rb, hb, margin, out, W);   /* the reach kernel's instantiation: Rb known to be the identity */   /* the general routine alone (SAT + clipping through the workspace) */
    return pmg::cyl_box(ca, Ra, ha[0], ha[2], cb, Rb, hb[0], hb[1], hb[2], margin, out, W);
}

/* the double-precision repeat of a cylinder pair (cyl_redo64) and its pieces, called directly: the double forward kinematics of a
 * contact body's link, and the repeat itself for chest kind ck (-1: none).  amb_out (may be NULL): the ambiguity of the FLOAT
 * pass over the same pair taken from float poses (ca, Ra | cb, Rb given by the caller), the trigger of the repeat */
extern "C" void pmge_probe_fk64(const float* q9, int body, double* p, double* R) { pmg::fk64_link(q9, body, p, R); }
extern "C" int pmge_probe_cyl_redo64(int ck, int cyl_body, int box_body, int wall, const float* q9, const float* blk0, const float* doorq,
                                     const float* kc, float prad, float phl, float* out)
{
    alignas(16) static float W[256];
    if (ck == 0) return pmg::cyl_redo64<0>(cyl_body, box_body, wall, q9, blk0, doorq, kc, prad, phl, out, W);
    if (ck == 1) return pmg::cyl_redo64<1>(cyl_body, box_body, wall, q9, blk0, doorq, kc, prad, phl, out, W);
    return pmg::cyl_redo64<-1>(cyl_body, box_body, wall, q9, blk0, doorq, kc, prad, phl, out, W);
}
/* the same on any pair, with the robot body's double pose handed in (handed = 1) as spec_fk / spec_pairs do: sincos64 per arm joint into
 * a table, fk64_chain with that table, then robot_p / robot_R.  blk0: two free-body rows.  (pmgd_cyl_redo64_pairs, gpu_probe/) */
extern "C" int pmge_probe_cyl_redo64_pairs(int ck, int cyl_body, int box_body, int wall, int handed, const float* q9, const float* blk0, const float* doorq,
                                           const float* kc, float prad, float phl, float* out)
{
    alignas(16) static float W[256];
    const int rb = cyl_body == pmg::BODY_GBASE ? pmg::BODY_GBASE : ((box_body == pmg::BODY_FINGER1 || box_body == pmg::BODY_FINGER2) ? box_body : -1);
    double sc[7][2], p[3], R[9];
    const bool hand = handed && rb >= 0;
    if (hand) {
        for (int j = 0; j < 7; j++) pmg::sincos64((double)q9[j], sc[j][0], sc[j][1]);
        pmg::fk64_chain(q9, sc, rb, p, R);
    }
    const double *hp = hand ? p : nullptr, *hR = hand ? R : nullptr;
    if (ck == 0) return pmg::cyl_redo64<0>(cyl_body, box_body, wall, q9, blk0, doorq, kc, prad, phl, out, W, hp, hR);
    if (ck == 1) return pmg::cyl_redo64<1>(cyl_body, box_body, wall, q9, blk0, doorq, kc, prad, phl, out, W, hp, hR);
    return pmg::cyl_redo64<-1>(cyl_body, box_body, wall, q9, blk0, doorq, kc, prad, phl, out, W, hp, hR);
}
/* the double arithmetic of the repeat on arrays (pmgd_double_maths): op 0 t_sqrt(x), 1 t_div(x, y), 2 sincos64(x) -> o0, o1.  In THIS
 * build t_sqrt / t_div are the plain operations; sincos64 is the code the device runs */
extern "C" int pmge_probe_double_maths(int op, int n, const double* x, const double* y, double* o0, double* o1)
{
    if (op < 0 || op > 2 || n < 1) return -1;
    for (int i = 0; i < n; i++) {
        if (op == 0) o0[i] = pmg::t_sqrt(x[i]);
        else if (op == 1) o0[i] = pmg::t_div(x[i], y[i]);
        else pmg::sincos64(x[i], o0[i], o1[i]);
    }
    return 0;
}
extern "C" int pmge_probe_cyl_amb(const float* ca, const float* Ra, float rad, float hl, const float* cb, const float* Rb, const float* hb, float margin,
                                  float* out, float* amb_out)
{
    alignas(16) static float W[256];
    float amb = 1e30f;
    const int n = pmg::cyl_box(ca, Ra, rad, hl, cb, Rb, hb[0], hb[1], hb[2], margin, out, W, &amb);
    *amb_out = amb;
    return n;
}

/* the launch-order plan in isolation: the single-workgroup plan (two_pass = 0) or the two-pass multi-workgroup plan on
 * the same batch; sched_out = [3 + 3 N] as on the device; returns the plan's promotion flag (< 0: not run).  hot: [N, 32] state rows, blocks: [N, 13 nb], actions [N, adim] */
extern "C" int pmge_probe_plan(int n_envs, int nb, const float* hot, const float* blocks, const float* actions, int adim,
                               int wave_budget, int two_pass, int* sched_out)
{
    using namespace pmg;
    EnvParams P;
    memset(&P, 0, sizeof(P));
    P.n_envs = n_envs; P.nb = nb; P.adim = adim; P.chest = -1; P.wave_budget = wave_budget; P.has_obj = nb > 0; P.near_r = 0.065f; P.fd_div = PMG_FD_DIV;
    const float lo[3] = {-0.67f, -0.2f, 0.175f}, hi[3] = {-0.37f, 0.2f, 0.55f};
    for (int a = 0; a < 3; a++) { P.ee_lo[a] = lo[a]; P.ee_hi[a] = hi[a]; }
    P.hot = const_cast<float*>(hot);
    P.blocks = const_cast<float*>(blocks);
    const int nwg = (n_envs + PLAN_THREADS - 1) / PLAN_THREADS;
    std::vector<int> sc(pmgx::Sched::words((size_t)n_envs), -1);
    P.sched = sc.data();
    if (!two_pass) {
        if (n_envs > PLAN_MAX_TILES * 64) return -1;   /* (the launcher switches to two passes at PLAN_SINGLE_MAX already) */
        emu::launch(1, PLAN_THREADS, [&]() { plan_all(P, actions); });
    } else {
        emu::launch(nwg, PLAN_THREADS, [&]() { plan_count(P, actions); });
        emu::launch(nwg, PLAN_THREADS, [&]() { plan_scatter(P, actions); });
    }
    memcpy(sched_out, sc.data(), sizeof(int) * (size_t)(P.schedule().wg_counts() - sc.data()));   /* counts, lists, redo count and list */
    return P.schedule().promoted();                         /* 0 / 1: the word pmg_k_step_list reads for its issue priority */
}

/* The plan with every parameter it reads, on the caller's own buffer (tests/plan_cases.py; pmgd_plan of gpu_probe/ is the same call
 * on the device).  mode 0: plan_all, 1: plan_all<true> (reach under tip control), 2: plan_count + plan_scatter over ceil(N / 1024)
 * workgroups.  buf: [guard | Sched::words(N) | guard] ints, in and out -- the plan works on the words in the middle, the caller
 * fills all of it with a sentinel and sees what was written.  env_cycles: [N, 2] or NULL; lpt_state: [2 + LPT_BINS], in and out, or
 * NULL.  The table and the clip box of the tip target are every task's but slide's.  Returns 0, or < 0 for arguments the plan
 * would read or write out of these arrays with (nothing is run then) */
#include "../../gpu_probe/pmg_plan_probe.inc"
extern "C" int pmge_plan(int mode, int n_envs, int nb, int chest, int joint_control, float near_r, float chest_reach, int fd_div, int wave_budget, int lpt_thresh,
                         int lpt_permille, int lpt_parity, const int* env_cycles, int* lpt_state, const float* hot, const float* blocks, const float* actions, int adim,
                         int guard, int* buf)
{
    using namespace pmg;
    if (!plan_args_ok(mode, n_envs, nb, chest, joint_control, lpt_thresh, lpt_permille, lpt_parity, env_cycles, lpt_state, hot, blocks, actions, adim, guard, buf)) return -1;
    EnvParams P = plan_params(n_envs, nb, chest, joint_control, near_r, chest_reach, fd_div, wave_budget, lpt_thresh, lpt_permille, lpt_parity, adim);
    P.hot = const_cast<float*>(hot);
    P.blocks = const_cast<float*>(blocks);
    P.env_cycles = const_cast<int*>(env_cycles);
    P.lpt_state = lpt_state;
    P.sched = buf + guard;
    const int nwg = (n_envs + PLAN_THREADS - 1) / PLAN_THREADS;
    if (mode == 0) emu::launch(1, PLAN_THREADS, [&]() { plan_all(P, actions); });
    else if (mode == 1) emu::launch(1, PLAN_THREADS, [&]() { plan_all<true>(P, actions); });
    else {
        emu::launch(nwg, PLAN_THREADS, [&]() { plan_count(P, actions); });
        emu::launch(nwg, PLAN_THREADS, [&]() { plan_scatter(P, actions); });
    }
    return 0;
}

/* The wavefront-order detector's own probes (tests/test_wave_order.py; emulator only): 128 threads, wavefront 1 hands one LDS word to
 * wavefront 0 between two workgroup barriers.  _racy: nothing orders the write and the read -- what wavefront 0 sees depends on
 * which wavefront runs first, and the orders 01 and 10 must tell.  _fenced: a barrier between them -- every order agrees.
 * out[0]: the word wavefront 0 read (7 = the initial value, 42 = wavefront 1's) */
static void probe_handover(bool fenced, int* out)
{
    emu::launch(1, 128, [&]() {
        __shared__ int word;
        const int t = (int)threadIdx.x, w = t >> 6;
        if (t == 0) word = 7;
        __syncthreads();
        if (w == 1 && (t & 63) == 0) word = 42;
        if (fenced) __syncthreads();
        int seen = 0;
        if (w == 0) seen = word;
        __syncthreads();
        if (t == 0) out[0] = seen;
    });
}
extern "C" void pmge_probe_handover_racy(int* out) { probe_handover(false, out); }
extern "C" void pmge_probe_handover_fenced(int* out) { probe_handover(true, out); }
