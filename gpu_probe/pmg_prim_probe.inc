/* pmg_prim_probe.inc -- TEST INFRASTRUCTURE: one probe body for every cross-lane primitive of pmg_wave.h whose result is
 * data.  Included once per namespace (WV = wv / wr, PRIM_FN = the function's name, PRIM_WR = 0 / 1) by
 *   - gpu_probe/pmg_gpu_probe.hip: hipcc, gfx950, the SHIPPED pybullet_multigoal_gym_amd/csrc/pmg_wave.h, and
 *   - tests/emu/pmg_probe.cpp:           g++, the fiber emulator's stand-in tests/emu/pmg_wave.h,
 * so that both headers answer to the same numpy models (tests/wave_models.py).
 *
 * in: [prim::NIN][64] floats, out: [prim::NOUT][64] floats, both indexed [slot][lane of the wavefront].  A family covers
 * every template argument of its primitives in one call (slot = template argument); what a family leaves alone keeps the
 * caller's sentinel.  `src` is the run-time lane argument (masked to the namespace's lane count here). */
#ifndef PMG_PRIM_PROBE_COMMON
#define PMG_PRIM_PROBE_COMMON
#include <type_traits>
namespace prim {
constexpr int NIN = 16, NOUT = 160;
enum Fam {
    F_BCAST = 0, F_BCAST_C, F_FMA2_BCAST_C, F_HALF, F_BCAST_R0, F_FMA2_BCAST_R0_C, F_DOT6_BCAST_R0_C, F_GJ9, F_GJ6, F_DOT6_LANES_R0,
    F_ADD_SHR2_BANK2, F_ROW_SHIFT, F_REDUCE, F_PREDICATE, F_LANE_ID, F_SQRT_RCP, F_COUNT
};
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}
/* The matrix-pipe primitive wv::mfma_32x32x2 (the shipped header's own definition in BOTH builds: its device form here, its
 * PMG_EMULATE branch in the emulator), a chain of `steps` calls on one accumulator, all 64 lanes alive:
 * a, b [n][steps][64], c [n][16][64] -> out [n][16][64], the last index the lane.  tests/mfma_cases.py */
constexpr int MFMA_MAX_STEPS = 8, MFMA_MAX_CASES = 64;
__device__ inline void mfma_chain(int n, int steps, const float* a, const float* b, const float* c, float* out)
{
    const int ln = (int)threadIdx.x & 63;
    for (int i = 0; i < n; i++) {
        wv::acc16 acc = wv::acc16_zero();
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = c[(16 * i + r) * 64 + ln];
        for (int s = 0; s < steps; s++) acc = wv::mfma_32x32x2(a[(i * steps + s) * 64 + ln], b[(i * steps + s) * 64 + ln], acc);
#pragma unroll
        for (int r = 0; r < 16; r++) out[(16 * i + r) * 64 + ln] = acc[r];
    }
}
/* The reach row set-up, pmg::reach_rowspace_setup<0, 8> (csrc/pmg_step_body.inc), for n cases one after the other on one wavefront.
 * The lane state is built the way substep() builds it -- forward kinematics, joint subspaces published in the contact store, M^-1 --
 * and the contact list is the caller's: q, qd [n][9]; con [n][8][12] (a b pa3 pb3 n3 dist), mu [n][8], ncs [n] (0..8)
 * -> coef [n][64][24] (a lane's coefficient per source row), resp [n][64][9] (M^-1 J^T), misc [n][64][4] (den, rhs, dinv, mu), and the
 * float32 operands the set-up worked from: S [n][9][6] (joint subspaces), minv [n][9][9].  tests/rowsetup_cases.py */
constexpr int ROWSETUP_MAX_CASES = 64;
__device__ inline void rowsetup_cases(pmg::ContactLds<0, 8>& L, pmg::LaneTabStore& lcs, int n, const float* q, const float* qd, const float* con, const float* mu,
                                      const int* ncs, float* coef, float* resp, float* misc, float* S_out, float* minv_out)
{
    using namespace pmg;
    LaneConst c;
    load_lane_const(lcs, c);
    const int l = wv::lane();
    for (int i = 0; i < n; i++) {
        const float ql = l < NJ ? q[9 * i + l] : 0.f, qdl = l < NJ ? qd[9 * i + l] : 0.f;
        Kin k;
        fk(c, ql, k);
        publish_subspaces<0, 8>(L, k);
        float I10[10], minv[NJ];
        body_inertia(c, k, I10);
        if (l >= NJ)
            for (int a = 0; a < 10; a++) I10[a] = 0.f;
        mass_inverse(k, I10, minv);
        int nc = ncs[i];
        nc = nc < 0 ? 0 : (nc > 8 ? 8 : nc);
        if (l < 8) {
            for (int a = 0; a < 12; a++) L.con[l][a] = l < nc ? con[(8 * i + l) * 12 + a] : 0.f;
            L.con_mu[l] = l < nc ? mu[8 * i + l] : 0.f;
        }
        wv::lds_sync();
        NcRows r;
        r.dinv = r.den = r.rhs_m = r.rhs_l = r.imp_m = r.app_m = r.app_l = r.prev_m = r.prev_l = 0.f;
        r.sg_l = 1.f; r.mot_active = 0x1FFu; r.lim_active = 0u;
        McState mc;
        for (int j = 0; j < NJ; j++) mc.A[j] = mc.sgnw[j] = 0.f;
        mc.hi_l = 0.f; mc.lim_any = 0u; mc.fast = true;
        ReachRowSet<24> w;
        reach_rowspace_setup<0, 8>(L, nc, r, mc, minv, qdl, 0.f, w);
        float* o = coef + (size_t)(64 * i + l) * 24;
#pragma unroll
        for (int s = 0; s < 24; s++) o[s] = w.c24[s];
        o = resp + (size_t)(64 * i + l) * 9;
#pragma unroll
        for (int d = 0; d < NJ; d++) o[d] = w.Rm[d];
        o = misc + (size_t)(64 * i + l) * 4;
        o[0] = w.den; o[1] = w.rhs; o[2] = w.dinv; o[3] = w.mu;
        if (l < NJ) {
            for (int a = 0; a < 6; a++) S_out[(9 * i + l) * 6 + a] = k.S[a];
            for (int j = 0; j < NJ; j++) minv_out[(9 * i + l) * 9 + j] = minv[j];
        }
        wv::lds_sync();
    }
}
}  // namespace prim
#ifdef PMG_EMULATE
extern "C" int pmge_rowsetup(int n, const float* q, const float* qd, const float* con, const float* mu, const int* ncs, float* coef, float* resp, float* misc,
                             float* S_out, float* minv_out)
{
    if (n < 1 || n > prim::ROWSETUP_MAX_CASES) return -1;
    emu::launch(1, 64, [&]() {
        __shared__ pmg::ContactLds<0, 8> L;
        __shared__ pmg::LaneTabStore lcs;
        prim::rowsetup_cases(L, lcs, n, q, qd, con, mu, ncs, coef, resp, misc, S_out, minv_out);
    });
    return 0;
}
extern "C" int pmge_rowspace_mfma() { return PMG_ROWSPACE_MFMA; }
extern "C" int pmge_rowsetup_pipeline() { return PMG_ROWSETUP_PIPELINE; }
extern "C" int pmge_mfma(int n, int steps, const float* a, const float* b, const float* c, float* out)
{
    if (n < 1 || n > prim::MFMA_MAX_CASES || steps < 1 || steps > prim::MFMA_MAX_STEPS) return -1;
    emu::launch(1, 64, [&]() { prim::mfma_chain(n, steps, a, b, c, out); });
    return 0;
}
/* the lean primitives, fk() in float32 and ik_solve() in either layout (PMG_IK_LEAN): pmgd_lean_prim / pmgd_fk / pmgd_ik of the device
 * probe library on the emulator.  pmg_lean_probe.inc once per layout, whatever layout the includer of THIS file is at */
#pragma push_macro("WV")
#undef WV
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
#pragma pop_macro("WV")
extern "C" int pmge_ik_lean() { return PMG_IK_LEAN; }
extern "C" int pmge_lean_prim(int wr_ns, int fam, const float* in, float* out)
{
    if (fam < 0 || fam >= prim::LEAN_FAMILIES) return -1;
    emu::launch(1, 64, [&]() {
        if (wr_ns) lean_probe_wr(fam, in, out);
        else lean_probe_wv(fam, in, out);
    });
    return 0;
}
extern "C" int pmge_fk(int packed, int n, const float* q, float* out)
{
    if (n < 1 || n > 4096) return -1;
    emu::launch(1, 64, [&]() {
        if (packed) { __shared__ pmgp::LaneTabStore lcs; fk_probe_wr(lcs, n, q, out); }
        else { __shared__ pmg::LaneTabStore lcs; fk_probe_wv(lcs, n, q, out); }
    });
    return 0;
}
extern "C" int pmge_ik(int packed, int n, const float* q, const float* target, float* q_out)
{
    if (n < 1 || n > 4096) return -1;
    emu::launch(1, 64, [&]() {
        if (packed) { __shared__ pmgp::LaneTabStore lcs; ik_probe_wr(lcs, n, q, target, q_out); }
        else { __shared__ pmg::LaneTabStore lcs; ik_probe_wv(lcs, n, q, target, q_out); }
    });
    return 0;
}
#endif
#endif

__device__ inline void PRIM_FN(int fam, int src, const float* in, float* out)
{
    using namespace prim;
    const int ln = (int)threadIdx.x & 63;
    src &= WV::LANES - 1;
    auto ld = [&](int k) { return in[64 * k + ln]; };
    auto st = [&](int o, float v) { out[64 * o + ln] = v; };
    auto sti = [&](int o, int v) { out[64 * o + ln] = __int_as_float(v); };
    const float v = ld(0);
    switch (fam) {
    case F_BCAST: {      /* run-time lane, then the same calls with a literal lane (the __builtin_constant_p switches) */
        const int vi = __float_as_int(ld(1));
        st(0, WV::bcast(v, src));
        sti(1, WV::bcast_i(vi, src));
        const float a3[3] = {ld(0), ld(1), ld(2)};
        float o3[3];
        WV::bcastn<3>(a3, src, o3);
        st(2, o3[0]); st(3, o3[1]); st(4, o3[2]);
        static_for<0, WV::LANES>([&](auto s) { constexpr int S = decltype(s)::value; st(8 + S, WV::bcast(v, S)); });
        static_for<0, 16>([&](auto s) { constexpr int S = decltype(s)::value; sti(72 + S, WV::bcast_i(vi, S)); });
        break;
    }
    case F_BCAST_C:
        static_for<0, WV::LANES>([&](auto s) { constexpr int S = decltype(s)::value; st(S, WV::bcast_c<S>(v)); });
#if PRIM_WR
        static_for<0, 16>([&](auto s) { constexpr int S = decltype(s)::value; sti(64 + S, WV::bcast_ci<S>(__float_as_int(ld(1)))); });
#endif
        break;
    case F_FMA2_BCAST_C:
        static_for<0, WV::LANES>([&](auto s) {
            constexpr int S = decltype(s)::value;
            float a1 = ld(1), a2 = ld(2);
            WV::fma2_bcast_c<S>(v, ld(3), a1, ld(4), a2);
            st(2 * S, a1); st(2 * S + 1, a2);
        });
        break;
    case F_HALF:
        static_for<0, 8>([&](auto s) {
            constexpr int S = decltype(s)::value;
            st(S, WV::half_bcast_c<S>(v));
            float acc = ld(1);
            WV::half_fma_bcast_c<S>(v, ld(2), acc);
            st(8 + S, acc);
        });
        break;
    case F_BCAST_R0: {
        static_for<0, 16>([&](auto s) { constexpr int S = decltype(s)::value; st(S, WV::bcast_r0_c<S>(v)); });
        st(16, WV::bcast_r0(v, src & 15));
        static_for<0, 16>([&](auto s) { constexpr int S = decltype(s)::value; st(17 + S, WV::bcast_r0(v, S)); });
        const float a2[2] = {ld(0), ld(1)};
        float o2[2];
        WV::bcastn_r0<2>(a2, src & 15, o2);
        st(33, o2[0]); st(34, o2[1]);
        break;
    }
    case F_FMA2_BCAST_R0_C:
        static_for<0, 16>([&](auto s) {
            constexpr int S = decltype(s)::value;
            float a1 = ld(1), a2 = ld(2);
            WV::fma2_bcast_r0_c<S>(v, ld(3), a1, ld(4), a2);
            st(2 * S, a1); st(2 * S + 1, a2);
        });
        break;
    case F_DOT6_BCAST_R0_C: {
        float x[6], c[6];
        for (int a = 0; a < 6; a++) { x[a] = ld(a); c[a] = ld(6 + a); }
        static_for<0, 16>([&](auto s) { constexpr int S = decltype(s)::value; st(S, WV::dot6_bcast_r0_c<S>(x, c)); });
        break;
    }
    case F_GJ9:
        static_for<0, 9>([&](auto s) {
            constexpr int P = decltype(s)::value;
            float a[9];
#pragma unroll
            for (int j = 0; j < 9; j++) a[j] = ld(j);
            WV::gj9_eliminate_r0_c<P>(a, ld(9));
#pragma unroll
            for (int j = 0; j < 9; j++) st(9 * P + j, a[j]);
        });
        break;
    case F_GJ6:
        static_for<0, 6>([&](auto s) {
            constexpr int P = decltype(s)::value;
            float a[6], e = ld(6);
#pragma unroll
            for (int j = 0; j < 6; j++) a[j] = ld(j);
            WV::gj6_eliminate_r0_c<P>(a, e, ld(7));
#pragma unroll
            for (int j = 0; j < 6; j++) st(7 * P + j, a[j]);
            st(7 * P + 6, e);
        });
        break;
    case F_DOT6_LANES_R0: {
        float c[6];
        for (int a = 0; a < 6; a++) c[a] = ld(a);
        st(0, WV::dot6_lanes_r0(c, ld(6)));
        break;
    }
    case F_ADD_SHR2_BANK2:
        st(0, WV::add_shr2_bank2(v, ld(1)));
        break;
    case F_ROW_SHIFT:
        static_for<1, 16>([&](auto s) {
            constexpr int N = decltype(s)::value;
            st(N - 1, WV::row_shr<N>(v, ld(1)));
            st(15 + N - 1, WV::row_shl<N>(v, ld(1)));
        });
        break;
    case F_REDUCE: {
        const float w = ld(1);
        st(0, WV::row_sum(v)); st(1, WV::half_sum(v)); st(2, WV::row_max(w));
        st(3, WV::sum_row0(v)); st(4, WV::max_row0(w));
        st(5, WV::sum_rows<1>(v)); st(6, WV::sum_rows<2>(v)); st(7, WV::sum_rows<3>(v)); st(8, WV::sum_rows<4>(v));
        st(9, WV::sum_wave(v)); st(10, WV::sum_all(v)); st(11, WV::max_all(w));
        break;
    }
    case F_PREDICATE: {
        const bool p = v != 0.f;
        const unsigned long long b = WV::ballot(p);
        sti(0, (int)(unsigned)(b & 0xFFFFFFFFull)); sti(1, (int)(unsigned)(b >> 32));
        sti(2, (int)WV::any_row_mask(p));
        sti(3, WV::any_lane(p) ? 1 : 0);
        sti(4, WV::uniform_positive(ld(1)) ? 1 : 0);
        st(5, WV::sel_lane(ld(2), ld(3), WV::lane(), src & 15));
        break;
    }
    case F_LANE_ID:
        sti(0, WV::lane()); sti(1, WV::lane_local());
#if PRIM_WR
        sti(2, WV::row());
#endif
        break;
    case F_SQRT_RCP:
        st(0, WV::fsqrt(v)); st(1, WV::rcp(ld(1)));
        break;
    default:
        break;
    }
}
