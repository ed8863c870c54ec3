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
}  // namespace prim
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
