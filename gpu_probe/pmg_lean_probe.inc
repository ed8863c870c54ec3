/* pmg_lean_probe.inc -- TEST INFRASTRUCTURE: probe bodies for the lean primitives of pmg_wave.h (affine_shr, half_gram6, half_max:
 * PMG_IK_LEAN) and for fk() / ik_solve() case after case.  Included once per namespace pair (WV = wv / wr, NSP = pmg / pmgp,
 * LEAN_FN / FK_FN / IK_FN = the functions' names) by gpu_probe/pmg_gpu_probe.hip (hipcc, gfx950, the shipped header) and, for the
 * fiber emulator (g++), by the PMG_EMULATE section of pmg_prim_probe.inc, which also holds the emulator's entry points; always behind
 * prim::static_for of that file.  tests/ik_lean_cases.py
 *
 * LEAN_FN: in [prim::NIN][64], out [prim::NOUT][64], indexed [slot][lane of the wavefront], all 64 lanes together.
 *   fam 0  affine_shr<1 / 2 / 4> of (R = slots 0-8, p = slots 9-11) -> slots 0-11, 12-23, 24-35
 *   fam 1  half_gram6 of slots 0-5 -> slots 0-20
 *   fam 2  half_max of slot 0 -> slot 0
 * FK_FN: fk() of n joint vectors q [n][9] -> out [n][16][18]: R (9), p (3), S (6) of the sixteen lanes of the env's row.
 * IK_FN: ik_solve() of n (start q [n][9], target [n][3]) -> q_out [n][9].
 * One env per wavefront (wv) runs the cases one after the other; four per wavefront (wr) runs four at a time, one per 16-lane
 * row -- a row without a case repeats the last one and stores nothing. */
#ifndef PMG_LEAN_PROBE_COMMON
#define PMG_LEAN_PROBE_COMMON
namespace prim {
constexpr int LEAN_FAMILIES = 3, FK_ROW_FLOATS = 18;
}
#endif

__device__ inline void LEAN_FN(int fam, const float* in, float* out)
{
    const int ln = (int)threadIdx.x & 63;
    auto ld = [&](int k) { return in[64 * k + ln]; };
    auto st = [&](int o, float v) { out[64 * o + ln] = v; };
    if (fam == 0) {
        prim::static_for<0, 3>([&](auto s) {
            constexpr int K = decltype(s)::value;
            float R[9], p[3];
#pragma unroll
            for (int a = 0; a < 9; a++) R[a] = ld(a);
#pragma unroll
            for (int a = 0; a < 3; a++) p[a] = ld(9 + a);
            WV::template affine_shr<(1 << K)>(R, p);
#pragma unroll
            for (int a = 0; a < 9; a++) st(12 * K + a, R[a]);
#pragma unroll
            for (int a = 0; a < 3; a++) st(12 * K + 9 + a, p[a]);
        });
    } else if (fam == 1) {
        float x[6], s[21];
#pragma unroll
        for (int a = 0; a < 6; a++) x[a] = ld(a);
        WV::half_gram6(x, s);
#pragma unroll
        for (int k = 0; k < 21; k++) st(k, s[k]);
    } else if (fam == 2) {
        st(0, WV::half_max(ld(0)));
    }
}

__device__ inline void FK_FN(NSP::LaneTabStore& lcs, int n, const float* q, float* out)
{
    using namespace NSP;
    LaneConst c;
    load_lane_const(lcs, c);
    const int l = WV::lane(), per = 64 / WV::LANES, slot = ((int)threadIdx.x & 63) / WV::LANES;
    for (int i = 0; i < n; i += per) {
        const int mine = i + slot;
        const bool valid = mine < n;
        const int cs = valid ? mine : n - 1;
        Kin k;
        fk(c, l < NJ ? q[9 * cs + l] : 0.f, k);
        if (valid && l < 16) {
            float* o = out + ((size_t)cs * 16 + l) * prim::FK_ROW_FLOATS;
            for (int a = 0; a < 9; a++) o[a] = k.R[a];
            for (int a = 0; a < 3; a++) o[9 + a] = k.p[a];
            for (int a = 0; a < 6; a++) o[12 + a] = k.S[a];
        }
    }
}

__device__ inline void IK_FN(NSP::LaneTabStore& lcs, int n, const float* q, const float* target, float* q_out)
{
    using namespace NSP;
    LaneConst c;
    load_lane_const(lcs, c);
    const int l = WV::lane(), per = 64 / WV::LANES, slot = ((int)threadIdx.x & 63) / WV::LANES;
    for (int i = 0; i < n; i += per) {
        const int mine = i + slot;
        const bool valid = mine < n;
        const int cs = valid ? mine : n - 1;
        const float r = ik_solve(c, l < NJ ? q[9 * cs + l] : 0.f, target + 3 * cs);
        if (valid && l < NJ) q_out[9 * cs + l] = r;
    }
}
