/* pmg_step_body.inc -- observation pack, contact phases, substep and env step; included by pmg_kernels.h once per
 * lane layout (namespace pmg: one env per wavefront; namespace pmgp: four envs per wavefront, see pmg_device.h). */
/* ------------------------------------------------------------------ */
/* component i of the desired goal.  The multi-block tasks re-derive it from the current block poses at
 * every observation (kuka_multi_step_base_env.py:309-312): a block beyond the active curriculum level /
 * sub-goal index "is already at its goal".  cold[7] = level, goal[15] = moved-block mask.          */
constexpr int CURR_DIM = 16;
__device__ __forceinline__ float effective_goal_at_level(const EnvParams& P, int env, int i, int level)
{
    const float* g = P.goal + (size_t)env * GOAL_DIM;
    if (!P.multi) return g[i];
    const float* cold = P.cold + (size_t)env * COLD_DIM;
    const float* bb = P.blocks + (size_t)env * BLOCK_DIM * P.nb;
    if (P.chest >= 0) {
        /* chest tasks (kuka_multi_step_envs.py:256-342, 405-475; oracle chest_goal()): [door open state | per block: the
         * chest floor centre or where the block is now | gripper goal].  The "current tip pose" gripper goal of sub-goal 0
         * is filled in by write_outputs (it equals the achieved value) */
        const float centre[3] = {-0.7f + 0.05f, 0.f, 0.175f}, top[3] = {-0.7f + 0.05f, 0.f, 0.3f};
        const bool pnp = P.grasping != 0;
        int in_chest = (1 << P.nb) - 1, lifted = -1, jb = -1;   /* jb: the gripper goes to block jb */
        float gw = 0.06f;
        if (P.decomposition) {
            if (level == 0) in_chest = 0;
            else if (!P.grip_goal) in_chest = (1 << level) - 1;
            else if (!pnp) {
                int j = (level - 1) / 2, ph = (level - 1) % 2;
                in_chest = (1 << (j + ph)) - 1;
                if (ph == 0) jb = j;
            } else {
                int j = (level - 1) / 3, ph = (level - 1) % 3;
                in_chest = (1 << (j + (ph == 2 ? 1 : 0))) - 1;
                if (ph == 0) jb = j;
                if (ph == 1) lifted = j;
                gw = ph == 2 ? 0.06f : 0.03f;
            }
        } else if (P.curriculum) in_chest = (int)g[15];        /* the blocks chosen at reset (:359-363, 492-496) */
        if (i == 0) return P.grasping ? 0.1f : 0.12f;
        int ii = i - 1;
        int b = ii / 3, a = ii - 3 * b;
        if (b < P.nb) return b == lifted ? top[a] : (((in_chest >> b) & 1) ? centre[a] : bb[BLOCK_DIM * b + a]);
        if (a == 0 && b == P.nb + 1) return gw;               /* finger width (pick and place only) */
        if (jb >= 0) return bb[BLOCK_DIM * jb + a] + ((!pnp && a == 0) ? 0.03f : 0.f);
        return pnp ? top[a] : centre[a] + (a == 0 ? 0.03f : 0.f);
    }
    int b = i / 3, a = i - 3 * b;
    if (P.task == PMG_TASK_BLOCK_STACK) {
        /* plain / curriculum: the first level+1 blocks of the order sit at their targets.  grip-informed sub-goals
         * come in (pick, place) pairs per block j (kuka_multi_step_envs.py:91-111): pick keeps blocks i < j, place
         * blocks i <= j at their targets; the tail is the gripper tip target and the finger width 0.03 */
        const bool pairs = P.grip_goal && P.decomposition;
        const int j = pairs ? level / 2 : level;
        const bool pick = pairs && (level % 2 == 0);
        if (i >= 3 * P.nb) {
            if (i == 3 * P.nb + 3) return 0.03f;
            int bj = (int)cold[8 + j];
            return pick ? bb[BLOCK_DIM * bj + a] : g[3 * bj + a];
        }
        int pos = 0;
        for (int s = 0; s < P.nb; s++) pos = ((int)cold[8 + s] == b) ? s : pos;   /* place of block b in the stack order */
        return (pick ? pos < j : pos <= j) ? g[i] : bb[BLOCK_DIM * b + a];
    }
    int moved = (int)g[15];
    if (!((moved >> b) & 1)) return bb[BLOCK_DIM * b + a];
    int kth = __popc((unsigned)moved & ((1u << b) - 1u));                        /* the k-th moved block takes target k */
    return g[3 * kth + a];
}
__device__ __forceinline__ float effective_goal(const EnvParams& P, int env, int i)
{
    return effective_goal_at_level(P, env, i, P.multi ? (int)P.cold[(size_t)env * COLD_DIM + 7] : 0);
}

/* ------------------------------------------------------------------ */
/* observation / reward pack                                           */
/* single-step tasks: kuka_single_step_base_env.py:193-244; robot state: kuka.py:227-256 */
/* tail = reward | goal_achieved | done of the packed row: TAIL_ZERO after a reset, TAIL_REWARD after a step, TAIL_KEEP
 * for an env that a masked reset left alone (its last step's values stay readable) */
constexpr int TAIL_ZERO = 0, TAIL_REWARD = 1, TAIL_KEEP = 2;
__device__ __forceinline__ void write_outputs(const EnvParams& P, int env, const LaneConst& c, float q, float qd,
                                              int elapsed, int tail_mode)
{
    const bool with_reward = tail_mode == TAIL_REWARD;
    int l = WV::lane();
    Kin k;
    fk(c, q, k);
    float tip[3], Rt[9];
    tip_frame(k, tip, Rt);
    /* spatial velocity of every link; lane 6 = link 7 (tip, gripper base), lane 7 = finger 1 */
    float v[6];
#pragma unroll
    for (int a = 0; a < 6; a++) v[a] = chain_prefix(k.S[a] * qd);
    float v6[6];
    WV::bcastn<6>(v, 6, v6);
    float tv[3], t[3];
    cross3(v6, tip, t);
    tv[0] = v6[3] + t[0]; tv[1] = v6[4] + t[1]; tv[2] = v6[5] + t[2];
    float closeness = 0.f, fvel = 0.f;
    if (P.grasping) {
        /* tabs: finger frame origin -/+ 0.005 along finger y (urdf:480-494) */
        float tab[3];
        float sgn = l == 7 ? -0.005f : 0.005f;
#pragma unroll
        for (int a = 0; a < 3; a++) tab[a] = k.p[a] + k.R[3 * a + 1] * sgn;
        float vt[3];
        cross3(v, tab, vt);
        float pack[4] = {tab[0], tab[1], tab[2], v[4] + vt[1]}, t1[4], t2[4];
        WV::bcastn<4>(pack, 7, t1);
        WV::bcastn<4>(pack, 8, t2);
        float d[3] = {t1[0] - t2[0], t1[1] - t2[1], t1[2] - t2[2]};
        closeness = sqrtf(dot3(d, d));
        /* gripper base origin: link 7 + 0.055 z (urdf:390-395) */
        float gb[3] = {tip[0] + Rt[2] * (0.055f - TIP_Z), tip[1] + Rt[5] * (0.055f - TIP_Z), tip[2] + Rt[8] * (0.055f - TIP_Z)};
        float vb[3];
        cross3(v6, gb, vb);
        fvel = (v6[4] + vb[1]) - t1[3];
    }
    float* o = P.out + (size_t)env * P.packed;
    const float* g = P.goal + (size_t)env * GOAL_DIM;
    int jo = P.joint_control ? 7 : 0;
    float* obs = o;
    float* pol = o + P.odim;
    float* ag = pol + P.pdim;
    float* dg = ag + P.gdim;
    float* tail = dg + P.gdim;
    if (jo && l < 7) { obs[l] = q; pol[l] = q; }
    float agv[3] = {tip[0], tip[1], tip[2]};
    if (P.task == PMG_TASK_REACH) {
        if (l < 3) { float x = l == 0 ? tip[0] : (l == 1 ? tip[1] : tip[2]); obs[jo + l] = x; pol[jo + l] = x; ag[l] = x; }
    } else if (!P.multi) {
        const float* b = P.blocks + (size_t)env * BLOCK_DIM * P.nb;
        float bp[3] = {b[0], b[1], b[2]}, bv[3] = {b[7], b[8], b[9]}, bw[3] = {b[10], b[11], b[12]};
        if (l == 0) {
            float* s = obs + jo;
            s[0] = tip[0]; s[1] = tip[1]; s[2] = tip[2];
            s[3] = bp[0]; s[4] = bp[1]; s[5] = bp[2];
            s[6] = closeness;
            s[7] = tip[0] - bp[0]; s[8] = tip[1] - bp[1]; s[9] = tip[2] - bp[2];
            s[10] = tv[0]; s[11] = tv[1]; s[12] = tv[2];
            s[13] = fvel;
            s[14] = tv[0] - bv[0]; s[15] = tv[1] - bv[1]; s[16] = tv[2] - bv[2];
            s[17] = v6[0] - bw[0]; s[18] = v6[1] - bw[1]; s[19] = v6[2] - bw[2];
            float* ps = pol + jo;
            ps[0] = tip[0]; ps[1] = tip[1]; ps[2] = tip[2]; ps[3] = closeness;
            ps[4] = tip[0] - bp[0]; ps[5] = tip[1] - bp[1]; ps[6] = tip[2] - bp[2];
            ag[0] = bp[0]; ag[1] = bp[1]; ag[2] = bp[2];
        }
        agv[0] = bp[0]; agv[1] = bp[1]; agv[2] = bp[2];
    } else {
        /* block stack: kuka_multi_step_base_env.py:255-336, clipped to +-5 */
        const float* bb = P.blocks + (size_t)env * BLOCK_DIM * P.nb;
        if (l == 0) {
            float* s = obs + jo;
            s[0] = tip[0]; s[1] = tip[1]; s[2] = tip[2]; s[3] = closeness;
            s[4] = tv[0]; s[5] = tv[1]; s[6] = tv[2]; s[7] = fvel;
            float* ps = pol + jo;
            ps[0] = tip[0]; ps[1] = tip[1]; ps[2] = tip[2]; ps[3] = closeness;
        }
        if (l < P.nb) {
            const float* b = bb + BLOCK_DIM * l;
            float* s = obs + jo + 8 + 16 * l;
            float* ps = pol + jo + 4 + 3 * l;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                s[a] = b[a];
                s[3 + a] = tip[a] - b[a];
                ps[a] = tip[a] - b[a];
                s[10 + a] = tv[a] - b[7 + a];
                s[13 + a] = v6[a] - b[10 + a];
                ag[(P.chest >= 0 ? 1 : 0) + 3 * l + a] = b[a];
            }
#pragma unroll
            for (int a = 0; a < 4; a++) s[6 + a] = b[3 + a];
        }
        if (P.chest >= 0 && l == 0) {
            /* kuka_multi_step_base_env.py:289-298 + chest.py:47-57: door joint position / velocity, then position and
             * linear velocity of the three key points riding on the door */
            const float dq = g[0], dqd = g[1];
            const int K = P.chest, cc = ChestT::comp(K);
            const float sg = ChestT::sign(K);
            float* s = obs + jo + 8 + 16 * P.nb;
            float* ps = pol + jo + 4 + 3 * P.nb;
            s[0] = dq; s[1] = dqd; ps[0] = dq;
            for (int kp = 0; kp < 3; kp++)
                for (int a = 0; a < 3; a++) {
                    float x = ChestT::door_c0(K, a) + (a == cc ? sg * dq : 0.f) + ChestT::keypoint(K, kp, a);
                    float vv = a == cc ? sg * dqd : 0.f;
                    s[2 + 6 * kp + a] = x; s[5 + 6 * kp + a] = vv;
                    ps[1 + 6 * kp + a] = x; ps[4 + 6 * kp + a] = vv;
                }
            ag[0] = dq;
        }
        if (P.grip_goal && l == 0) { /* kuka_multi_step_base_env.py:300-304 */
            float* t = ag + (P.chest >= 0 ? 1 : 0) + 3 * P.nb;
            t[0] = tip[0]; t[1] = tip[1]; t[2] = tip[2];
            if (P.grasping) t[3] = closeness;
        }
    }
    WV::lds_sync();
    if (P.multi) {
        for (int i = l; i < P.odim; i += WV::LANES) obs[i] = fminf(fmaxf(obs[i], -5.f), 5.f);
        for (int i = l; i < P.pdim; i += WV::LANES) pol[i] = fminf(fmaxf(pol[i], -5.f), 5.f);
    }
    float dgl = l < P.gdim ? effective_goal(P, env, l) : 0.f;
    /* this lane's component of the achieved goal (multi-block layouts) */
    float agl = 0.f;
    if (P.multi) {
        const float* bb = P.blocks + (size_t)env * BLOCK_DIM * P.nb;
        const int c0 = P.chest >= 0 ? 1 : 0, li = l - c0;
        if (li < 0) agl = g[0];
        else if (li < 3 * P.nb) agl = bb[BLOCK_DIM * (li / 3) + li % 3];
        else if (l < P.gdim) { int t = li - 3 * P.nb; agl = t == 0 ? tip[0] : (t == 1 ? tip[1] : (t == 2 ? tip[2] : closeness)); }
        /* chest sub-goal 0 (open the door): the gripper goal is where the gripper is (kuka_multi_step_envs.py:288-291, 437) */
        /* ... and so it is at curriculum level 0 (:365-369, 498-501) */
        if (P.chest >= 0 && (P.decomposition || P.curriculum) && P.grip_goal && li >= 3 * P.nb && (int)P.cold[(size_t)env * COLD_DIM + 7] == 0) dgl = agl;
    }
    if (l < P.gdim) dg[l] = dgl;
    if (with_reward) {
        /* _compute_reward: d = ||ag - dg||, binary -(d > thr) as float32 or dense -d */
        float dd = 0.f;
        if (P.multi) {
            float e = l < P.gdim ? agl - dgl : 0.f;
            dd = WV::sum_rows<2>(e * e);   /* goal_dim <= 19: lanes of the first two rows */
        } else {
#pragma unroll
            for (int a = 0; a < 3; a++) { float e = agv[a] - g[a]; dd += e * e; }
        }
        float d = sqrtf(dd);
        bool not_achieved = d > P.thr;
        if (l == 0) {
            tail[0] = P.binary_reward ? (not_achieved ? -1.f : -0.f) : -d;
            tail[1] = not_achieved ? 0.f : 1.f;
            tail[2] = elapsed >= P.max_steps ? 1.f : 0.f;
        }
    } else if (l == 0 && tail_mode == TAIL_ZERO) {
        tail[0] = 0.f; tail[1] = 0.f; tail[2] = 0.f;
    }
}

/* ------------------------------------------------------------------ */
/* contact phases of a substep.  For the reach kernel (no free bodies) they
 * are rare (fingers at the table clip plane only), so they are kept out of
 * line there to keep the register budget of the 100-substep loop small. */
template <int NB, int MAXC>
__device__ __noinline__ int collide_cold(ContactLds<NB, MAXC>& L, const float* kc, int nb, float tcx, float tcy, float tcz, float thx, float thy,
                                         float thz, float tmu)
{
    float tc[3] = {tcx, tcy, tcz}, th[3] = {thx, thy, thz};
    return collide<NB, MAXC, false>(L, kc, nb, tc, th, tmu);
}
/* publish (inline, from registers) what the pair / contact lanes need: the frames the narrowphase reads (publish_frames: finger
 * boxes, gripper-base cylinder, block rotations, the chest door's slot) and the joint subspaces the row set-up reads
 * (publish_subspaces).  One-wavefront kernels: both, by the env's wavefront.  Two-wavefront workgroups: the HELPER publishes the
 * frames from its own forward kinematics (helper_wave_loop), wavefront 0 only the subspaces */
template <int NB, int MAXC>
__device__ __forceinline__ void publish_subspaces(ContactLds<NB, MAXC>& L, const Kin& k)
{
    int l = WV::lane_local();
    if (l < NJ) {
#pragma unroll
        for (int a = 0; a < 6; a++) L.S[l][a] = k.S[a];
    }
}
template <int NB, int MAXC, int CYL>
__device__ __forceinline__ void publish_frames(ContactLds<NB, MAXC>& L, int nb, const Kin& k)
{
    int l = WV::lane_local();   /* (its LDS addresses are not worth a spill slot) */
    if (l == 7 || l == 8) {
        float* f = L.fing[l - 7];
#pragma unroll
        for (int a = 0; a < 3; a++) f[a] = k.p[a];
#pragma unroll
        for (int a = 0; a < 9; a++) f[3 + a] = k.R[a];
    }
    if (NB > 0 && l == 6) { /* gripper-base cylinder: link 7 frame shifted 0.055 along its z (urdf:390-395) */
#pragma unroll
        for (int a = 0; a < 3; a++) L.gbase[a] = k.p[a] + k.R[3 * a + 2] * 0.055f;
#pragma unroll
        for (int a = 0; a < 9; a++) L.gbase[3 + a] = k.R[a];
    }
    if (l < nb) quat_to_R(L.blk[l] + 3, L.blkR[l]);
    if (ObjT<CYL>::chest >= 0 && l == nb) {
        /* the door rides in block slot nb: box centre, identity rotation, mass-scaled velocity along its axis */
        constexpr int K = ObjT<CYL>::chest >= 0 ? ObjT<CYL>::chest : 0;
        float* b = L.blk[nb];
#pragma unroll
        for (int a = 0; a < BLOCK_DIM; a++) b[a] = 0.f;
#pragma unroll
        for (int a = 0; a < 3; a++) b[a] = ChestT::door_c0(K, a);
        b[ChestT::comp(K)] += ChestT::sign(K) * L.door[0];
        b[6] = 1.f;
        b[7 + ChestT::comp(K)] = ChestT::sign(K) * L.door[1] / door_scale(K);
#pragma unroll
        for (int a = 0; a < 9; a++) L.blkR[nb][a] = (a % 4 == 0) ? 1.f : 0.f;
    }
    WV::lds_sync();
}
template <int NB, int MAXC, int CYL>
__device__ __forceinline__ void detect_publish(ContactLds<NB, MAXC>& L, int nb, const Kin& k, float q)
{
    /* the joint angles, for the double forward kinematics of a cylinder pair in contact (cyl_redo64): L.qd is free until the
     * rows are set up, behind the detection */
    if (PMG_CYL_REDO64 && NB > 0 && WV::lane_local() < NJ) L.qd[WV::lane_local()] = q;
    publish_subspaces<NB, MAXC>(L, k);
    publish_frames<NB, MAXC, CYL>(L, nb, k);
}
/* ... then run the narrowphase */
template <int NB, int MAXC, int CYL>
__device__ __forceinline__ int detect(ContactLds<NB, MAXC>& L, const float* kc, int nb, const Kin& k, float q, float tcx, float tcy, float tcz, float thx,
                                      float thy, float thz, float tmu)
{
    detect_publish<NB, MAXC, CYL>(L, nb, k, q);
    if (PMG_COLD_CONTACTS && NB == 0) return collide_cold<NB, MAXC>(L, kc, nb, tcx, tcy, tcz, thx, thy, thz, tmu);
    float tc[3] = {tcx, tcy, tcz}, th[3] = {thx, thy, thz};
    return collide<NB, MAXC, CYL>(L, kc, nb, tc, th, tmu);
}

template <int NB, int MAXC>
__device__ __noinline__ void build_rows_cold(ContactLds<NB, MAXC>& L, int nc, int nrob)
{
    build_contact_rows<NB, MAXC, false>(L, nc, nrob);
}
#ifndef PMG_ROWS_BY_LANE
#define PMG_ROWS_BY_LANE 1
#endif
/* One row of a one-object env, set up by ONE lane (M^-1 and the joint velocities must be in LDS): Jacobian
 * [joints (9) | object (6)], response [M^-1 J^T | object], 1/diag, right-hand side, friction coefficient.
 * [BULLET-PRIOR] setupMultiBodyContactConstraint, as build_contact_rows. */
struct ObjRow {
    float Jm[NJ], Jo[6], Rm[NJ], Ro[6];
    float dinv, den, rhs, mu;
};
template <int NB, int MAXC, int CYL>
__device__ __forceinline__ void obj_row_setup(const ContactLds<NB, MAXC>& L, int row, bool is_row, ObjRow& w)
{
    using OB = ObjT<CYL>;
    const int cc = is_row ? row / 3 : 0, tt = is_row ? row - 3 * cc : 0;
    float o[12];
    {
        const float4 a = *(const float4*)L.con[cc], b = *(const float4*)(L.con[cc] + 4), c4 = *(const float4*)(L.con[cc] + 8);
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w; o[8] = c4.x; o[9] = c4.y; o[10] = c4.z; o[11] = c4.w;
    }
    const int ida = (int)o[0], idb = (int)o[1];
    const bool rob_a = ida >= BODY_FINGER1 && ida <= BODY_GBASE, rob_b = idb >= BODY_FINGER1 && idb <= BODY_GBASE;
    const bool obj_a = ida >= 0 && ida < BODY_FINGER1, obj_b = idb >= 0 && idb < BODY_FINGER1;
    const bool has_rob = is_row && (rob_a || rob_b), has_obj = is_row && (obj_a || obj_b);
    const int idr = rob_a ? ida : idb;
    const int own = idr == BODY_FINGER1 ? 7 : (idr == BODY_FINGER2 ? 8 : -1);    /* the gripper base rides on link 7 only */
    const float sgr = rob_a ? 1.f : -1.f, sgo = obj_a ? 1.f : -1.f;
    float prob[3], pobj[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { prob[k] = rob_a ? o[2 + k] : o[5 + k]; pobj[k] = obj_a ? o[2 + k] : o[5 + k]; }
    const float n[3] = {o[8], o[9], o[10]};
    float t1[3], t2[3], dir[3];
    plane_space(n, t1, t2);
#pragma unroll
    for (int k = 0; k < 3; k++) dir[k] = tt == 0 ? n[k] : (tt == 1 ? t1[k] : t2[k]);
#pragma unroll
    for (int d = 0; d < NJ; d++) {
        float S[8];                                          /* two 16-byte reads per subspace, all eighteen in flight together */
        {
            const float4 a4 = *(const float4*)L.S[d], b4 = *(const float4*)(L.S[d] + 4);
            S[0] = a4.x; S[1] = a4.y; S[2] = a4.z; S[3] = a4.w; S[4] = b4.x; S[5] = b4.y;
        }
        float v[3];
        cross3(S, prob, v);
        const float jd = (v[0] + S[3]) * dir[0] + (v[1] + S[4]) * dir[1] + (v[2] + S[5]) * dir[2];
        w.Jm[d] = (has_rob && (d < 7 || d == own)) ? sgr * jd : 0.f;
    }
    float denom, rel;
    {
        const float* bl = L.blk[0];
        const float rv[3] = {pobj[0] - bl[0], pobj[1] - bl[1], pobj[2] - bl[2]};
        float rxn[3];
        cross3(rv, dir, rxn);
#pragma unroll
        for (int k = 0; k < 3; k++) { w.Jo[k] = has_obj ? sgo * dir[k] : 0.f; w.Jo[3 + k] = has_obj ? sgo * rxn[k] : 0.f; }
        float da[3] = {w.Jo[3] * OB::inv_inertia(0), w.Jo[4] * OB::inv_inertia(0), w.Jo[5] * OB::inv_inertia(0)};
        if (OB::cyl) {
            float la[3];
            const float* Rb = L.blkR[0];
            la[0] = (Rb[0] * w.Jo[3] + Rb[3] * w.Jo[4] + Rb[6] * w.Jo[5]) * OB::inv_inertia(0);
            la[1] = (Rb[1] * w.Jo[3] + Rb[4] * w.Jo[4] + Rb[7] * w.Jo[5]) * OB::inv_inertia(1);
            la[2] = (Rb[2] * w.Jo[3] + Rb[5] * w.Jo[4] + Rb[8] * w.Jo[5]) * OB::inv_inertia(2);
            mat3v(Rb, la, da);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) { w.Ro[k] = w.Jo[k] / BLOCK_MASS; w.Ro[3 + k] = da[k]; }
        denom = dot3(w.Jo, w.Jo) / BLOCK_MASS + dot3(w.Jo + 3, da);
        rel = dot3(w.Jo, bl + 7) + dot3(w.Jo + 3, bl + 10);
    }
#pragma unroll
    for (int i = 0; i < NJ; i++) {
        const float* mi = L.minv[i];
        w.Rm[i] = ((w.Jm[0] * mi[0] + w.Jm[1] * mi[1]) + (w.Jm[2] * mi[2] + w.Jm[3] * mi[3])) + ((w.Jm[4] * mi[4] + w.Jm[5] * mi[5]) + (w.Jm[6] * mi[6] + w.Jm[7] * mi[7])) + w.Jm[8] * mi[8];
    }
#pragma unroll
    for (int d = 0; d < NJ; d++) { denom += w.Jm[d] * w.Rm[d]; rel += w.Jm[d] * L.qd[d]; }
    w.dinv = (is_row && denom > SIMD_EPS) ? 1.f / denom : 0.f;
    w.den = (is_row && denom > SIMD_EPS) ? denom : 0.f;
    {
        const float dist = o[11] + LINEAR_SLOP;
        float pos_err = 0.f, vel_err = -rel;
        if (dist > 0.f) vel_err -= dist / DT;
        else pos_err = -dist * CONTACT_ERP / DT;
        w.rhs = is_row ? (tt == 0 ? (pos_err + vel_err) * w.dinv : -rel * w.dinv) : 0.f;
    }
    w.mu = (is_row && tt != 0) ? L.con_mu[cc] : 0.f;
}
/* four envs per wavefront, one object: the LDS rows (DIRECT layout) built one row per lane -- the (row, DoF) item
 * loops of build_contact_rows take 14 rounds each on the 16 lanes of an env with both fingers and the object on the
 * table (36 rows), this takes three */
template <int NB, int MAXC, int CYL>
__device__ __forceinline__ void build_rows_by_lane(ContactLds<NB, MAXC>& L, int nc, int c0 = 0)
{
    const int l = WV::lane();
    for (int r0 = 3 * c0; r0 < 3 * nc; r0 += WV::LANES) {     /* c0: first contact that needs an LDS row (object_run_*) */
        const int row = r0 + l;
        const bool is_row = row < 3 * nc;
        ObjRow w;
        obj_row_setup<NB, MAXC, CYL>(L, row, is_row, w);
        if (is_row) {
            const int c = row / 3, t = row - 3 * c;
            float4* d = (float4*)row_of(L, c, t);
            d[0] = make_float4(w.Jm[0], w.Jm[1], w.Jm[2], w.Jm[3]);
            d[1] = make_float4(w.Jm[4], w.Jm[5], w.Jm[6], w.Jm[7]);
            d[2] = make_float4(w.Jm[8], w.Jo[0], w.Jo[1], w.Jo[2]);
            d[3] = make_float4(w.Jo[3], w.Jo[4], w.Jo[5], 0.f);
            d[4] = make_float4(w.Rm[0], w.Rm[1], w.Rm[2], w.Rm[3]);
            d[5] = make_float4(w.Rm[4], w.Rm[5], w.Rm[6], w.Rm[7]);
            d[6] = make_float4(w.Rm[8], w.Ro[0], w.Ro[1], w.Ro[2]);
            d[7] = make_float4(w.Ro[3], w.Ro[4], w.Ro[5], 0.f);
            d[8] = make_float4(w.rhs, w.dinv, 0.f, w.mu);      /* ROW_RHS, ROW_DINV, ROW_APP, ROW_MU */
            row_of(L, c, t)[ROW_DEN] = w.den;
        }
    }
    WV::lds_sync();
}

template <int NB, int MAXC, int CYL>
__device__ __forceinline__ void prepare_rows(ContactLds<NB, MAXC>& L, const float* minv, float qd, int nc, int c0 = 0)
{
    int l = WV::lane();
    if (PMG_ROWS_BY_LANE && NB == 1 && WV::LANES == 16) {
        if (l < NJ) {
#pragma unroll
            for (int j = 0; j < NJ; j++) L.minv[l][j] = minv[j];
            L.qd[l] = qd;
        }
        WV::lds_sync();
        if (c0 >= 0) build_rows_by_lane<NB, MAXC, CYL>(L, nc, c0);   /* c0 < 0: publish only (the caller builds behind its run) */
        return;
    }
    const int nrob = NB == 0 ? nc : robot_contacts(L, nc);   /* reach: every contact is finger x table */
    if (l < NJ && nrob > 0) {
#pragma unroll
        for (int j = 0; j < NJ; j++) L.minv[l][j] = minv[j];
        L.qd[l] = qd;
    }
    if (NB == 0 && l < nc) L.rob_idx[l] = (unsigned short)l;
    WV::lds_sync();
    if (PMG_COLD_CONTACTS && NB == 0) build_rows_cold<NB, MAXC>(L, nc, nrob);
    else build_contact_rows<NB, MAXC, CYL>(L, nc, nrob, c0);
}

/* reach with finger x table contacts, one env per wavefront: the solve in ROW SPACE.  Lane 16 + r owns contact row
 * r = 3 c + t (normal, two frictions of contact c <= 8) and keeps its unclamped impulse u_r = app_r + rhs_r - (J_r dv) / den_r;
 * lanes 0..8 keep the joint velocity change dv (and, inside a pass over the non-contact rows, their motor / limit u's).
 * A visit of row r is: clamp u_r in lane 16 + r, subtract, v_readlane the impulse change, ONE fma in every lane --
 *      lane 16 + s:  u_s -= (J_s M^-1 J_r^T) / den_s * delta        (0 for s = r: a row's own response cancels its impulse)
 *      lane l < 9 :  dv_l += (M^-1 J_r^T)_l * delta
 * -- instead of a 16-lane butterfly reduction of J_r . dv per visit (robot_rows_iteration).  The 24 x 24 coupling
 * coefficients are 9-term dot products of the rows the build phase left in LDS, one per (lane, source row).  Same rows,
 * same order (normals, then the friction pairs of the contacts whose normal carries an impulse), same clamps. */
#ifndef PMG_ROWSPACE
#define PMG_ROWSPACE 1
#endif
/* PMG_ROWSPACE_MFMA: reach_contact_pgs_rowspace takes M^-1 J^T and the 24 x 24 coupling table from two chains of five
 * v_mfma_f32_32x32x2_f32 (wv::mfma_32x32x2) instead of ~500 VALU instructions on wavefront 0's serial chain; 0 keeps the
 * VALU build.  Measured on one MI355X (profiles/r07_reach_mfma_ab.txt): set-up 4197 -> 3452 cycles per contact substep (response +
 * coefficients 2501 -> 1717), the pressed env alone 0.831 -> 0.775 ms, headline 4.685 -> 4.906 M env-steps/s (+ 4.7 %, four
 * alternating runs each, spreads 0.1 %). */
#ifndef PMG_ROWSPACE_MFMA
#define PMG_ROWSPACE_MFMA 1
#endif
/* PMG_ROWSETUP_PIPELINE: the front of reach_rowspace_setup (contact fetch, plane_space, direction, Jacobian entries) without its
 * stalls; 0 keeps that code as it was.  Same arithmetic, same bits (tests/rowsetup_pipelined_cases.py).  The stalls were not the
 * ones expected: in the =0 build the eighteen reads of the joint subspaces are ALREADY in flight together behind one wait (the
 * compiler unrolls the loop and hoists them).  What its ISA shows instead (profiles/r08_reach_setup_ab.txt, section 1):
 *   - the direction select `tt == 0 ? n : (tt == 1 ? t1 : t2)` behind plane_space's if / else comes out as a cascade of 19 branches
 *     over exec masks, 100 instructions of which 85 scalar, that a wavefront with rows of all three kinds walks arm by arm;
 *   - the subspace reads sit BEHIND that cascade and the contact fetch is waited for in front of it: two exposed LDS latencies;
 *   - the friction coefficient is read under a branch at the very end of the set-up and waited for at once: a third.
 * With the switch on, the operands of each select are plain locals -- clang then emits a select, and nothing is left for the
 * optimiser to thread a branch through: six v_cndmask --, the subspaces of the first PMG_ROWSETUP_PREFETCH joints are read right
 * behind the contact, in front of plane_space (the wait there is for the contact alone; the rest are read where they were, behind
 * the first joints' arithmetic), and the friction coefficient rides with the contact fetch.  Prefetch depth 6, not 9: from 7 on
 * pmg_k_step_reach2 takes a tenth VGPR spill (9 at depth <= 6 as without the switch), and 6 measured fastest of 0 / 6 / 9.
 * Measured on one MI355X (same note): the set-up's front 1569 -> about 1.1 k cycles per contact substep on the stamped one-wavefront
 * kernel, headline + 1 % (four alternating runs each; the slowest new run beats the fastest parent run by more than both spreads).
 * The M^-1 store needed nothing: the compiler already writes the nine floats as two 16-byte stores and a dword. */
#ifndef PMG_ROWSETUP_PIPELINE
#define PMG_ROWSETUP_PIPELINE 1
#endif
#ifndef PMG_ROWSETUP_PREFETCH
#define PMG_ROWSETUP_PREFETCH 6      /* joints (0 .. 9) whose subspace is read in front of plane_space */
#endif
#ifndef PMG_PRE_SWEEP
#define PMG_PRE_SWEEP 1
#endif
#ifndef PMG_PRE_SWEEP_OBJ
#define PMG_PRE_SWEEP_OBJ 1
#endif
template <int NB, int MAXC>
__device__ __forceinline__ const float* contact_row_ptr(const ContactLds<NB, MAXC>& L, int r)
{
    const int c = r / 3, t = r - 3 * c;
    return t == 0 ? L.rows[c] : L.rows[MAXC + 2 * c + (t - 1)];
}
/* nine consecutive floats at a 16-byte aligned LDS address: two 16-byte reads and one dword */
__device__ __forceinline__ void ld9(const float* p, float* v)
{
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; v[8] = p[8];
}
/* what the set-up leaves in a lane: its coefficient per source row (row lanes: -(J_j M^-1 J_s^T) / den_j, 0 for its own row; DoF
 * lanes: (M^-1 J_s^T)_l), and, in a row lane, its response M^-1 J_j^T, diagonal, right-hand side, friction coefficient and bound */
template <int NR>
struct ReachRowSet {
    float c24[NR], Rm[NJ];
    float den, dinv, rhs, mu, hi;
};
/* (mc: in, the motor / limit state of the DoF lanes; out, the same with the row lanes' answers to a joint-space impulse added) */
template <int NB, int MAXC>
__device__ __forceinline__ void reach_rowspace_setup(ContactLds<NB, MAXC>& L, int nc, const NcRows& r, McState& mc, const float* minv, float qd, float dv_pre,
                                                     ReachRowSet<3 * MAXC>& w)
{
    /* The rows are set up HERE, one per lane, straight from the contact list -- prepare_rows / build_contact_rows (four
     * LDS phases shaped for objects) are skipped on this path.  [BULLET-PRIOR] setupMultiBodyContactConstraint, as
     * build_contact_rows: finger (body A) x table: J_d = (w_d x p + v_d) . dir for the arm joints and the finger's own. */
    constexpr int NR = 3 * MAXC;
    const int l = WV::lane_local();
#ifdef PMG_PROFILE
    long long tb_ = prof::now();
#endif
    const int rr = l - 16;                                   /* this lane's contact row, if any */
    const bool is_dof = l < NJ, is_row = rr >= 0 && rr < 3 * nc;
    const int cc = is_row ? rr / 3 : 0, tt = is_row ? rr - 3 * cc : 0;
    if (is_dof) {                                            /* M^-1 and the joint velocities for everybody */
#pragma unroll
        for (int j = 0; j < NJ; j++) L.minv[l][j] = minv[j];
        L.qd[l] = qd + dv_pre;
    }
    float o[12];
    {
        const float4 a = *(const float4*)L.con[cc], b = *(const float4*)(L.con[cc] + 4), c4 = *(const float4*)(L.con[cc] + 8);
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w; o[8] = c4.x; o[9] = c4.y; o[10] = c4.z; o[11] = c4.w;
    }
    constexpr bool PIPE = PMG_ROWSETUP_PIPELINE != 0;
    float mu_c = 0.f;                                        /* PIPE: the contact's friction coefficient rides with the contact fetch */
    if constexpr (PIPE) mu_c = L.con_mu[cc];
    float Sv[NJ][6];                                         /* PIPE: the subspaces of the first NPRE joints, read behind the contact and in front of plane_space */
    constexpr int NPRE = PIPE ? PMG_ROWSETUP_PREFETCH : 0;
    static_assert(NPRE >= 0 && NPRE <= NJ, "PMG_ROWSETUP_PREFETCH counts joints");
    {
#pragma unroll
        for (int d = 0; d < NPRE; d++) {                     /* uniform address: LDS broadcast */
            const float4 a = *(const float4*)L.S[d], b = *(const float4*)(L.S[d] + 4);
            Sv[d][0] = a.x; Sv[d][1] = a.y; Sv[d][2] = a.z; Sv[d][3] = a.w; Sv[d][4] = b.x; Sv[d][5] = b.y;
        }
    }
    const float pt[3] = {o[2], o[3], o[4]}, n[3] = {o[8], o[9], o[10]};
    const int own = (int)o[0] == BODY_FINGER1 ? 7 : 8;
    float t1[3], t2[3], dir[3];
    plane_space(n, t1, t2);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if constexpr (PIPE) {                                /* selects of plain locals: v_cndmask, not branches */
            const float nk = n[k], t1k = t1[k], t2k = t2[k];
            const float tk = tt == 1 ? t1k : t2k;
            dir[k] = tt == 0 ? nk : tk;
        } else {
            dir[k] = tt == 0 ? n[k] : (tt == 1 ? t1[k] : t2[k]);
        }
    }
#ifdef PMG_PROFILE
    PMG_STAMP(tb_, 13);          /* M^-1 / qd stores, contact fetch, plane_space, direction select */
#endif
    float Jm[NJ];
#pragma unroll
    for (int d = 0; d < NJ; d++) {
        float S[8];                                          /* uniform address: LDS broadcast */
        if (d < NPRE) {
#pragma unroll
            for (int a = 0; a < 6; a++) S[a] = Sv[d][a];
        } else {
            const float4 a = *(const float4*)L.S[d], b = *(const float4*)(L.S[d] + 4);
            S[0] = a.x; S[1] = a.y; S[2] = a.z; S[3] = a.w; S[4] = b.x; S[5] = b.y;
        }
        float v[3];
        cross3(S, pt, v);
        const float jd = (v[0] + S[3]) * dir[0] + (v[1] + S[4]) * dir[1] + (v[2] + S[5]) * dir[2];
        Jm[d] = (is_row && (d < 7 || d == own)) ? jd : 0.f;
    }
#ifdef PMG_PROFILE
    PMG_STAMP(tb_, 15);          /* the nine Jacobian entries */
#endif
    /* every row lane leaves its Jacobian in a 12-float slot of the (free) row storage; the slots of rows that do not exist
     * hold zeros (Jm is zero there), so that nothing below has to branch on the contact count */
    float* slots = &L.rows[0][0];
    if (rr >= 0 && rr < NR) {
        float4* my = (float4*)(slots + 12 * rr);
        my[0] = make_float4(Jm[0], Jm[1], Jm[2], Jm[3]);
        my[1] = make_float4(Jm[4], Jm[5], Jm[6], Jm[7]);
        slots[12 * rr + 8] = Jm[8];
    }
    WV::lds_sync();
#ifdef PMG_PROFILE
    PMG_STAMP(tb_, 22);          /* slot store + lds_sync (13 + 15 + 22: contact fetch + Jacobian rows) */
#endif
    float Rm[NJ], denom = 0.f, rel = 0.f;
    constexpr bool MM = PMG_ROWSPACE_MFMA && NB == 0 && MAXC == 8;   /* (every other instantiation of this template is dead code) */
    float cq[24];
    if constexpr (MM) {
    /* The two dense products of the set-up on the matrix pipe (wv::mfma_32x32x2, exact f32): R^T = M^-1 J^T, (9 x 9)(9 x 24),
     * then C = J R^T, (24 x 9)(9 x 24), one 32 x 32 tile each, K = 9 as the pairs (d, d + 4), d < 4, then (8, pad): lane
     * (col, half) = l & 31, l >> 5 feeds entry 4 half + i of its row in step i.  The SAME five registers -- J_col[4 half + i],
     * J_col[8] -- are the B operand of the first product and the A operand of the second, and result register i of the first
     * (R_col[i + 4 half]; register 4: R_col[8], and an exact 0 in the upper half: row 12 of a product whose A rows >= 9
     * are zeros) is the second's B operand as it stands.  Rows, columns and k beyond 9 / 24 are exact zeros.
     * The results go back through the row store, which is this wavefront's from barrier B to the next barrier A: a table
     * T[owner][28], owner l < 9 = DoF lane l holding R_s[l], s < 24 (the transposed read of R^T), owner 9 + j = row lane
     * 16 + j holding C[s][j] -- 33 x 28 floats over the dead Jacobian slots.  Every lane then reads its 24 coefficients with
     * the same six 16-byte reads; a row lane's Rm[d] is T[d][j], the very numbers the DoF lanes take as coefficients. */
    static_assert(NJ == 9 && NR <= 24 && 3 * MAXC * ROW_STRIDE >= (NJ + 24) * 28, "row store too small for the coupling table");
    float* T = slots;
    {
        const int col = l & 31, half = l >> 5;
        const bool colv = col < NR, rowv = col < NJ;
        const float* jp = slots + 12 * (colv ? col : 0);
        const float* mp = &L.minv[rowv ? col : 0][0];
        const float4 j4 = *(const float4*)(jp + 4 * half), m4 = *(const float4*)(mp + 4 * half);
        const float j8 = jp[8], m8 = mp[8];
        const float bj[5] = {colv ? j4.x : 0.f, colv ? j4.y : 0.f, colv ? j4.z : 0.f, colv ? j4.w : 0.f, (colv && half == 0) ? j8 : 0.f};
        const float am[5] = {rowv ? m4.x : 0.f, rowv ? m4.y : 0.f, rowv ? m4.z : 0.f, rowv ? m4.w : 0.f, (rowv && half == 0) ? m8 : 0.f};
        wv::acc16 R = wv::acc16_zero(), C = wv::acc16_zero();
#pragma unroll
        for (int i = 0; i < 5; i++) R = wv::mfma_32x32x2(am[i], bj[i], R);
#pragma unroll
        for (int i = 0; i < 5; i++) C = wv::mfma_32x32x2(bj[i], R[i], C);
        WV::lds_sync();                                      /* every lane has its operands: the slots may go */
        if (colv) {
#pragma unroll
            for (int i = 0; i < 4; i++) T[28 * (4 * half + i) + col] = R[i];
            if (half == 0) T[28 * 8 + col] = R[4];
            float4* tc = (float4*)(T + 28 * (NJ + col) + 4 * half);   /* register 4 q + i: C[8 q + 4 half + i][col] */
            tc[0] = make_float4(C[0], C[1], C[2], C[3]);
            tc[2] = make_float4(C[4], C[5], C[6], C[7]);
            tc[4] = make_float4(C[8], C[9], C[10], C[11]);
        }
        WV::lds_sync();
        const bool rowl = rr >= 0 && rr < NR;
        const float* tr = T + (rowl ? rr : 0);
#pragma unroll
        for (int d = 0; d < NJ; d++) Rm[d] = tr[28 * d];
        const float4* tq = (const float4*)(T + 28 * (is_dof ? l : (rowl ? NJ + rr : 0)));
#pragma unroll
        for (int q = 0; q < 6; q++) {
            const float4 v = tq[q];
            cq[4 * q] = v.x; cq[4 * q + 1] = v.y; cq[4 * q + 2] = v.z; cq[4 * q + 3] = v.w;
        }
    }
    } else {
#pragma unroll
    for (int i = 0; i < NJ; i++) {
        float mi[NJ];
        ld9(L.minv[i], mi);
        Rm[i] = ((Jm[0] * mi[0] + Jm[1] * mi[1]) + (Jm[2] * mi[2] + Jm[3] * mi[3])) + ((Jm[4] * mi[4] + Jm[5] * mi[5]) + (Jm[6] * mi[6] + Jm[7] * mi[7])) + Jm[8] * mi[8];
    }
    }
    {
        float qv[NJ];
        ld9(L.qd, qv);
#pragma unroll
        for (int d = 0; d < NJ; d++) { denom += Jm[d] * Rm[d]; rel += Jm[d] * qv[d]; }
    }
    const float dinv_r = (is_row && denom > SIMD_EPS) ? 1.f / denom : 0.f;
    float rhs_r;
    {
        const float dist = o[11] + LINEAR_SLOP;
        float pos_err = 0.f, vel_err = -rel;
        if (dist > 0.f) vel_err -= dist / DT;
        else pos_err = -dist * CONTACT_ERP / DT;
        rhs_r = is_row ? (tt == 0 ? (pos_err + vel_err) * dinv_r : -rel * dinv_r) : 0.f;
    }
    float mu_r;
    if constexpr (PIPE) mu_r = is_row ? mu_c : 0.f;          /* (=0: a read under a branch at the very end, waited for at once) */
    else mu_r = is_row ? L.con_mu[cc] : 0.f;
    const float hi_r = is_row ? 1e10f : 0.f;
#ifdef PMG_PROFILE
    PMG_STAMP(tb_, 23);          /* M^-1 J^T, diagonal, right-hand side */
#endif
    /* Coefficients.  Row lane 16 + j needs -(J_j . M^-1 J_s^T) / den_j for every source row s, DoF lane l < 9 needs
     * (M^-1 J_s^T)_l.  M^-1 is symmetric, so both are ONE formula: a . J_s with a = M^-1 J_j^T (a row lane's own response,
     * in registers) or a = row l of M^-1 (a DoF lane's own registers), scaled by -1 / den_j or 1 -- the same straight-line
     * code in every lane, three uniform-address LDS reads per source.  (Round 3 dotted J_j with responses read from the
     * slots and gave the DoF lanes a second, per-lane read behind a select: the compiler sank the reads into the arms of
     * the select and emitted a divergent branch per source row -- exec masks reloaded from spilled SGPRs, load -> wait ->
     * use with nothing in flight: 183 cycles per source, 4.4 k of the 7.3 k cycles of the set-up.)  A DoF lane's sum has
     * the terms and the association of the Rm[] above, i.e. the numbers lane s used to publish. */
    const float kk = is_dof ? 1.f : -dinv_r;
#pragma unroll
    for (int D = 0; D < NJ; D++) {                           /* a contact row's answer to the joint-space impulse of DoF D */
        const float aD = kk * Rm[D];                         /* (row lanes; limit visits scale sgnw by sg: sg^2 = 1) */
        mc.A[D] = is_dof ? mc.A[D] : aD;
        mc.sgnw[D] = is_dof ? mc.sgnw[D] : aD * r.sg_l;
    }
    float (&c24)[NR] = w.c24;
    if constexpr (MM) {          /* PMG_ROWSPACE_MFMA: both tables came off the matrix pipe above; a DoF lane's entry is R_s[l] itself (kk = 1) */
#pragma unroll
        for (int s = 0; s < NR; s++) c24[s] = s == rr ? 0.f : kk * cq[s];
    } else {
    float av[NJ];
#pragma unroll
    for (int k = 0; k < NJ; k++) av[k] = is_dof ? minv[k] : Rm[k];
    int off = 0;
#pragma unroll
    for (int s = 0; s < NR; s++) {
        /* sources two by two, the reads of a pair issued once the pair before the last one is done: four sources in flight */
        if ((s & 1) == 0 && s >= 4) WV::chain(off, c24[s - 3]);
        float js[NJ];                                        /* uniform address: LDS broadcast */
        ld9(slots + 12 * s + off, js);
        const float d = ((av[0] * js[0] + av[1] * js[1]) + (av[2] * js[2] + av[3] * js[3])) + ((av[4] * js[4] + av[5] * js[5]) + (av[6] * js[6] + av[7] * js[7])) + av[8] * js[8];
        c24[s] = s == rr ? 0.f : kk * d;
    }
    }
#ifdef PMG_PROFILE
    PMG_STAMP(tb_, 11);          /* coefficient build */
#endif
#pragma unroll
    for (int d = 0; d < NJ; d++) w.Rm[d] = Rm[d];
    w.den = (is_row && denom > SIMD_EPS) ? denom : 0.f;
    w.dinv = dinv_r; w.rhs = rhs_r; w.mu = mu_r; w.hi = hi_r;
}
template <int NB, int MAXC>
__device__ __forceinline__ void reach_contact_pgs_rowspace(ContactLds<NB, MAXC>& L, int nc, NcRows& r, const McState& mc_in, const float* minv, float qd,
                                                           float& dv, bool pre = false, float dv_pre = 0.f)
{
    /* pre: iteration 0's pass over the motor / limit rows has been made already (substep(), while the helper wavefront was
     * colliding); dv_pre = the joint velocity change it left.  The contact rows then start from u = rhs - (J dv_pre) / den,
     * i.e. their right-hand sides are taken at the joint velocity qd + dv_pre. */
    constexpr int NR = 3 * MAXC;
    const int l = WV::lane_local();
    const bool is_dof = l < NJ;
    McState mc = mc_in;
    ReachRowSet<NR> w;
    reach_rowspace_setup<NB, MAXC>(L, nc, r, mc, minv, qd, dv_pre, w);
    const float (&c24)[NR] = w.c24;
    const float dinv_r = w.dinv, rhs_r = w.rhs, mu_r = w.mu, hi_r = w.hi;
#ifdef PMG_PROFILE
    long long tprev = prof::now();
#endif
    float x = is_dof ? dv_pre : rhs_r;                       /* DoF lanes: dv; row lanes: u (app = 0; dv = 0 or dv_pre at entry) */
    float capp = 0.f, cprev = 0.f;                           /* this lane's contact impulse, and its value one iteration ago */
    const float rden = dinv_r != 0.f ? __builtin_amdgcn_rcpf(dinv_r) : 0.f;
    for (int it = 0; it < SOLVER_ITERS; it++) {
        if (!(pre && it == 0)) {   /* the non-contact rows (motors, limits), as nc_sweep_auto; the row lanes ride along with A = their coefficients */
            const float am0 = r.app_m, al0 = r.app_l;
            float um = is_dof ? r.app_m + (r.rhs_m - x * r.dinv) : x;
            float ul = r.app_l + (r.rhs_l - r.sg_l * x * r.dinv);
            mc_sweep<true>(r, mc, (it & 1) != 0, um, ul);
            float xd = x;
            mc_apply(minv, (r.app_m - am0) + r.sg_l * (r.app_l - al0), xd);
            x = is_dof ? xd : um;
        }
        PMG_TICK(24);
#pragma unroll
        for (int c = 0; c < MAXC; c++) {                     /* normals; a contact that does not exist has hi = 0: nothing moves */
            const float napp = __builtin_amdgcn_fmed3f(x, 0.f, hi_r);
            const float delta = napp - capp;
            capp = WV::sel_lane(napp, capp, l, 16 + 3 * c);
            x = fmaf(c24[3 * c], WV::bcast(delta, 16 + 3 * c), x);
        }
        PMG_TICK(25);
#pragma unroll
        for (int c = 0; c < MAXC; c++) {
            const float nimp = WV::bcast(capp, 16 + 3 * c);
            if (WV::uniform_positive(nimp)) {                /* frictions of the contacts whose normal carries an impulse */
                const float lim = mu_r * nimp;
#pragma unroll
                for (int t = 1; t < 3; t++) {
                    const float napp = __builtin_amdgcn_fmed3f(x, -lim, lim);
                    const float delta = napp - capp;
                    capp = WV::sel_lane(napp, capp, l, 16 + 3 * c + t);
                    x = fmaf(c24[3 * c + t], WV::bcast(delta, 16 + 3 * c + t), x);
                }
            }
        }
        /* squared velocity change of this lane's rows during the iteration (each row is visited once) */
        const float dc = (capp - cprev) * rden;
        cprev = capp;
        const float resid = is_dof ? nc_residual(r) : dc * dc;
        PMG_TICK(26);
        if (!WV::any_lane(resid > RESIDUAL_THRESHOLD)) break;
#ifdef PMG_PROFILE
        if (threadIdx.x == 0 && blockIdx.x == 0) prof::acc()[14] += 1;
#endif
    }
    PMG_TICK(12);
    dv = x;
}

/* One free object (push / pick_and_place / slide), one env per wavefront: the same solve in row space.  Lanes 0..8 the
 * joints, 9..14 the object's [v, w] (the lanes of LaneDof<1>), lane 16 + r contact row r = 3 c + t of the first
 * OBJ_ROWSPACE_MAXC contacts; an env with more contacts takes the LDS-row path (prepare_rows + lds_rows_iteration).
 * Rows are set up one per lane straight from the contact list ([BULLET-PRIOR] setupMultiBodyContactConstraint, as
 * build_contact_rows): a robot body (finger / gripper base) on at most one side, the object on at most one side.
 * Each row lane publishes its response [M^-1 J_rob^T (9) | object response (6) | 0] in a 16-float slot of the row
 * store; coefficient (lane, s) is then one 15-term dot product (row lanes) or one slot entry (DoF lanes). */
#ifndef PMG_OBJ_ROWSPACE_MAXC
#define PMG_OBJ_ROWSPACE_MAXC 16     /* (a test build lowers it to reach the path beyond it with few contacts) */
#endif
constexpr int OBJ_ROWSPACE_MAXC = PMG_OBJ_ROWSPACE_MAXC;
template <int NB, int MAXC, int CYL>
__device__ __forceinline__ void obj_contact_pgs_rowspace(ContactLds<NB, MAXC>& L, int nc, NcRows& r, const McState& mc_in, const float* minv,
                                                         float qd, float& dv, bool pre = false, float dv_pre = 0.f)
{   /* pre / dv_pre: iteration 0's pass over the motor / limit rows was made in front of barrier B (reach_contact_pgs_rowspace) */
    if constexpr (NB == 1 && WV::LANES == 64) {
    using OB = ObjT<CYL>;
    constexpr int RC = OBJ_ROWSPACE_MAXC, NR = 3 * RC;
    static_assert(3 * MAXC * ROW_STRIDE >= 16 * NR, "row store too small for the response slots");
    const int l = WV::lane();
#ifdef PMG_PROFILE
    long long tb_ = prof::now();
#endif
    const int rr = l - 16;
    const bool is_jnt = l < NJ, is_dof = l < NJ + 6, is_row = rr >= 0 && rr < 3 * nc;
    const int cc = is_row ? rr / 3 : 0, tt = is_row ? rr - 3 * cc : 0;
    if (is_jnt) {
#pragma unroll
        for (int j = 0; j < NJ; j++) L.minv[l][j] = minv[j];
        L.qd[l] = qd + dv_pre;
    }
    float o[12];
    {
        const float4 a = *(const float4*)L.con[cc], b = *(const float4*)(L.con[cc] + 4), c4 = *(const float4*)(L.con[cc] + 8);
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w; o[8] = c4.x; o[9] = c4.y; o[10] = c4.z; o[11] = c4.w;
    }
    const int ida = (int)o[0], idb = (int)o[1];
    const bool rob_a = ida >= BODY_FINGER1 && ida <= BODY_GBASE, rob_b = idb >= BODY_FINGER1 && idb <= BODY_GBASE;
    const bool obj_a = ida >= 0 && ida < BODY_FINGER1, obj_b = idb >= 0 && idb < BODY_FINGER1;
    const bool has_rob = is_row && (rob_a || rob_b), has_obj = is_row && (obj_a || obj_b);
    const int idr = rob_a ? ida : idb;
    const int own = idr == BODY_FINGER1 ? 7 : (idr == BODY_FINGER2 ? 8 : -1);    /* the gripper base rides on link 7 only */
    const float sgr = rob_a ? 1.f : -1.f, sgo = obj_a ? 1.f : -1.f;
    float ptr_[3], pto[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { ptr_[k] = rob_a ? o[2 + k] : o[5 + k]; pto[k] = obj_a ? o[2 + k] : o[5 + k]; }
    const float n[3] = {o[8], o[9], o[10]};
    float t1[3], t2[3], dir[3];
    plane_space(n, t1, t2);
#pragma unroll
    for (int k = 0; k < 3; k++) dir[k] = tt == 0 ? n[k] : (tt == 1 ? t1[k] : t2[k]);
    /* robot side: J_d = +-(w_d x p + v_d) . dir */
    float Jm[NJ];
#pragma unroll
    for (int d = 0; d < NJ; d++) {
        float S[8];                                          /* uniform address: LDS broadcast */
        {
            const float4 a = *(const float4*)L.S[d], b = *(const float4*)(L.S[d] + 4);
            S[0] = a.x; S[1] = a.y; S[2] = a.z; S[3] = a.w; S[4] = b.x; S[5] = b.y;
        }
        float v[3];
        cross3(S, ptr_, v);
        const float jd = (v[0] + S[3]) * dir[0] + (v[1] + S[4]) * dir[1] + (v[2] + S[5]) * dir[2];
        Jm[d] = (has_rob && (d < 7 || d == own)) ? sgr * jd : 0.f;
    }
    /* object side: J = +-[dir, r x dir], response [J_lin / m, R diag(1/I) R^T J_ang] */
    float Jo[6], Ro[6], denom = 0.f, rel = 0.f;
    {
        const float* bl = L.blk[0];
        const float rv[3] = {pto[0] - bl[0], pto[1] - bl[1], pto[2] - bl[2]};
        float rxn[3];
        cross3(rv, dir, rxn);
#pragma unroll
        for (int k = 0; k < 3; k++) { Jo[k] = has_obj ? sgo * dir[k] : 0.f; Jo[3 + k] = has_obj ? sgo * rxn[k] : 0.f; }
        float da[3] = {Jo[3] * OB::inv_inertia(0), Jo[4] * OB::inv_inertia(0), Jo[5] * OB::inv_inertia(0)};
        if (OB::cyl) {
            float la[3];
            const float* Rm = L.blkR[0];
            la[0] = (Rm[0] * Jo[3] + Rm[3] * Jo[4] + Rm[6] * Jo[5]) * OB::inv_inertia(0);
            la[1] = (Rm[1] * Jo[3] + Rm[4] * Jo[4] + Rm[7] * Jo[5]) * OB::inv_inertia(1);
            la[2] = (Rm[2] * Jo[3] + Rm[5] * Jo[4] + Rm[8] * Jo[5]) * OB::inv_inertia(2);
            mat3v(Rm, la, da);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) { Ro[k] = Jo[k] / BLOCK_MASS; Ro[3 + k] = da[k]; }
        denom = dot3(Jo, Jo) / BLOCK_MASS + dot3(Jo + 3, da);
        rel = dot3(Jo, bl + 7) + dot3(Jo + 3, bl + 10);
    }
    WV::lds_sync();
    float Rm[NJ];
#pragma unroll
    for (int i = 0; i < NJ; i++) {
        float mi[NJ];
        ld9(L.minv[i], mi);
        Rm[i] = ((Jm[0] * mi[0] + Jm[1] * mi[1]) + (Jm[2] * mi[2] + Jm[3] * mi[3])) + ((Jm[4] * mi[4] + Jm[5] * mi[5]) + (Jm[6] * mi[6] + Jm[7] * mi[7])) + Jm[8] * mi[8];
    }
    {
        float qv[NJ];
        ld9(L.qd, qv);
#pragma unroll
        for (int d = 0; d < NJ; d++) { denom += Jm[d] * Rm[d]; rel += Jm[d] * qv[d]; }
    }
    const float dinv_r = (is_row && denom > SIMD_EPS) ? 1.f / denom : 0.f;
    float rhs_r;
    {
        const float dist = o[11] + LINEAR_SLOP;
        float pos_err = 0.f, vel_err = -rel;
        if (dist > 0.f) vel_err -= dist / DT;
        else pos_err = -dist * CONTACT_ERP / DT;
        rhs_r = is_row ? (tt == 0 ? (pos_err + vel_err) * dinv_r : -rel * dinv_r) : 0.f;
    }
    const float mu_r = is_row ? L.con_mu[cc] : 0.f, hi_r = is_row ? 1e10f : 0.f;
    float* slots = &L.rows[0][0];
    if (rr >= 0 && rr < NR) {                                /* rows that do not exist leave zeros: no branch on nc below */
        float4* my = (float4*)(slots + 16 * rr);
        my[0] = make_float4(Rm[0], Rm[1], Rm[2], Rm[3]);
        my[1] = make_float4(Rm[4], Rm[5], Rm[6], Rm[7]);
        my[2] = make_float4(Rm[8], Ro[0], Ro[1], Ro[2]);
        my[3] = make_float4(Ro[3], Ro[4], Ro[5], 0.f);
    }
    WV::lds_sync();
    McState mc = mc_in;
    if (!is_jnt) {                                           /* a row's answer to the joint-space impulse of DoF D (0 in the object's lanes) */
#pragma unroll
        for (int D = 0; D < NJ; D++) { mc.A[D] = -dinv_r * Rm[D]; mc.sgnw[D] = mc.A[D] * r.sg_l; }
    }
    float cf[NR];
    const float k_dot = is_dof ? 0.f : -dinv_r, k_own = is_dof ? 1.f : 0.f;   /* (a DoF lane's Jm and Jo are zeros: its dot product is an exact 0) */
    const float* own_p = slots + (is_dof ? l : 15);
#pragma unroll
    for (int c = 0; c < RC; c++) {
        if (c < nc) {                                        /* uniform */
#pragma unroll
            for (int t = 0; t < 3; t++) {
                const int s = 3 * c + t;
                const float4 s0 = *(const float4*)(slots + 16 * s), s1 = *(const float4*)(slots + 16 * s + 4),
                             s2 = *(const float4*)(slots + 16 * s + 8), s3 = *(const float4*)(slots + 16 * s + 12);
                const float d0 = (Jm[0] * s0.x + Jm[1] * s0.y) + (Jm[2] * s0.z + Jm[3] * s0.w);
                const float d1 = (Jm[4] * s1.x + Jm[5] * s1.y) + (Jm[6] * s1.z + Jm[7] * s1.w);
                const float d2 = (Jm[8] * s2.x + Jo[0] * s2.y) + (Jo[1] * s2.z + Jo[2] * s2.w);
                const float d3 = (Jo[3] * s3.x + Jo[4] * s3.y) + Jo[5] * s3.z;
                const float own_s = own_p[16 * s];
                const float cs = fmaf(k_own, own_s, k_dot * ((d0 + d1) + (d2 + d3)));   /* branch-free blend: see reach_contact_pgs_rowspace */
                cf[s] = s == rr ? 0.f : cs;
            }
        } else {
            cf[3 * c] = cf[3 * c + 1] = cf[3 * c + 2] = 0.f;
        }
    }
#ifdef PMG_PROFILE
    PMG_STAMP(tb_, 11);
    long long tprev = prof::now();
#endif
    float x = is_dof ? dv_pre : rhs_r;                       /* DoF lanes: velocity change (0, or dv_pre in the joint lanes); row lanes: u */
    float capp = 0.f, cprev = 0.f;
    const float rden = dinv_r != 0.f ? __builtin_amdgcn_rcpf(dinv_r) : 0.f;
    for (int it = 0; it < SOLVER_ITERS; it++) {
        if (!(pre && it == 0)) {   /* motors and limits; every other lane rides along with its coefficients in mc.A */
            const float am0 = r.app_m, al0 = r.app_l;
            float um = is_jnt ? r.app_m + (r.rhs_m - x * r.dinv) : x;
            float ul = r.app_l + (r.rhs_l - r.sg_l * x * r.dinv);
            mc_sweep<true>(r, mc, (it & 1) != 0, um, ul);
            float xd = x;
            mc_apply(minv, (r.app_m - am0) + r.sg_l * (r.app_l - al0), xd);
            x = is_jnt ? xd : um;
        }
#pragma unroll
        for (int c = 0; c < RC; c++) {
            if (c < nc) {
                const float napp = __builtin_amdgcn_fmed3f(x, 0.f, hi_r);
                const float delta = napp - capp;
                capp = WV::sel_lane(napp, capp, l, 16 + 3 * c);
                x = fmaf(cf[3 * c], WV::bcast(delta, 16 + 3 * c), x);
            }
        }
#pragma unroll
        for (int c = 0; c < RC; c++) {
            if (c < nc) {
                const float nimp = WV::bcast(capp, 16 + 3 * c);
                if (WV::uniform_positive(nimp)) {
                    const float lim = mu_r * nimp;
#pragma unroll
                    for (int t = 1; t < 3; t++) {
                        const float napp = __builtin_amdgcn_fmed3f(x, -lim, lim);
                        const float delta = napp - capp;
                        capp = WV::sel_lane(napp, capp, l, 16 + 3 * c + t);
                        x = fmaf(cf[3 * c + t], WV::bcast(delta, 16 + 3 * c + t), x);
                    }
                }
            }
        }
        const float dc = (capp - cprev) * rden;
        cprev = capp;
        const float resid = is_jnt ? nc_residual(r) : dc * dc;
        if (!WV::any_lane(resid > RESIDUAL_THRESHOLD)) break;
#ifdef PMG_PROFILE
        if (threadIdx.x == 0 && blockIdx.x == 0) prof::acc()[14] += 1;
#endif
    }
    PMG_TICK(12);
    dv = x;
    }
}

/* Several blocks, one env per wavefront: the leading block x table run in ROW SPACE.  A block owns an 8-lane half row
 * (lanes 0..5 its velocity change, LaneDof) and at most four table contacts = twelve rows that touch that block alone:
 * row r = 3 k + t of the block lives in lane r & 7 of the half row, register r >> 3, with its unclamped impulse u; the
 * twelve-by-twelve coupling of a block's rows and their effect on its six DoFs are coefficients in registers, and the
 * k-th contact of EVERY block is visited in one instruction stream as before (table_runs) -- clamp, subtract, then
 * bank-masked DPP row_newbcast fmas (lane of the half row -> its half row) instead of LDS row fetches, a half-row
 * butterfly and LDS stores per visit.  The rows behind the run stay LDS rows and change the block velocities in
 * DoF space, so u is re-derived from them when a run phase begins (only if there are such rows). */
#ifndef PMG_TABLE_ROWSPACE
#define PMG_TABLE_ROWSPACE 1
#endif
struct TableRun {
    float J[2][6];        /* this lane's rows (register 0: rows 0..7 of the block, 1: rows 8..11) */
    float cu[2][12];      /* -(J_r M^-1 J_s^T) / den_r against the block's source rows s, 0 for r = s */
    float cx[12];         /* DoF role: (M^-1 J_s^T) component of this lane */
    float u[2], capp[2], cprev[2], rhs[2], dinv[2], den[2], mu[2];
};
template <int NB, int MAXC>
__device__ __forceinline__ void table_run_setup(ContactLds<NB, MAXC>& L, const LaneDof<NB>& ld, TableRun& tr)
{
    const int l = WV::lane();
    const bool blk_lane8 = l >= 16 && l < 16 + 8 * NB;       /* any lane of a block's half row */
    const int b = blk_lane8 ? (l - 16) >> 3 : 0, h = l & 7;
    /* every lane of the half row needs the block's run: toff / tcnt live in the DoF lanes (comp 0..5) only */
    const int toff = __float_as_int(WV::template half_bcast_c<0>(__int_as_float(ld.toff)));
    const int tcnt_h = __float_as_int(WV::template half_bcast_c<0>(__int_as_float(ld.tcnt)));
    const int tcnt = blk_lane8 ? tcnt_h : 0;
    const float* bl = L.blk[b];
    float* slots = &L.rows[0][0];                             /* 12 rows x 8 floats per block: [6 b][12][8] response of the row */
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int row = h + 8 * k;
        const bool is_row = blk_lane8 && row < 3 * tcnt;
        const int c = is_row ? toff + row / 3 : 0, t = is_row ? row - 3 * (row / 3) : 0;
        const float* o = L.con[c];
        const float n[3] = {o[8], o[9], o[10]};
        float t1[3], t2[3], dir[3];
        plane_space(n, t1, t2);
#pragma unroll
        for (int a = 0; a < 3; a++) dir[a] = t == 0 ? n[a] : (t == 1 ? t1[a] : t2[a]);
        const float rv[3] = {o[2] - bl[0], o[3] - bl[1], o[4] - bl[2]};     /* the block is body A of its table pair */
        float rxn[3];
        cross3(rv, dir, rxn);
        float R[6];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            tr.J[k][a] = is_row ? dir[a] : 0.f; tr.J[k][3 + a] = is_row ? rxn[a] : 0.f;
            R[a] = tr.J[k][a] / BLOCK_MASS; R[3 + a] = tr.J[k][3 + a] * (1.f / BLOCK_INERTIA);
        }
        const float denom = dot3(tr.J[k], tr.J[k]) / BLOCK_MASS + dot3(tr.J[k] + 3, R + 3);
        const float rel = dot3(tr.J[k], bl + 7) + dot3(tr.J[k] + 3, bl + 10);
        const float dinv = (is_row && denom > SIMD_EPS) ? 1.f / denom : 0.f;
        tr.dinv[k] = dinv;
        tr.den[k] = (is_row && denom > SIMD_EPS) ? denom : 0.f;
        const float dist = o[11] + LINEAR_SLOP;
        float pos_err = 0.f, vel_err = -rel;
        if (dist > 0.f) vel_err -= dist / DT;
        else pos_err = -dist * CONTACT_ERP / DT;
        tr.rhs[k] = is_row ? (t == 0 ? (pos_err + vel_err) * dinv : -rel * dinv) : 0.f;
        tr.mu[k] = is_row ? L.con_mu[c] : 0.f;
        tr.u[k] = tr.rhs[k]; tr.capp[k] = 0.f; tr.cprev[k] = 0.f;
        if (blk_lane8 && row < 12) {
            float4* my = (float4*)(slots + (12 * b + row) * 8);
            my[0] = make_float4(R[0], R[1], R[2], R[3]);
            my[1] = make_float4(R[4], R[5], 0.f, 0.f);
        }
    }
    WV::lds_sync();
#pragma unroll
    for (int s2 = 0; s2 < 12; s2++) {
        const float* sl = slots + (12 * b + s2) * 8;
        const float4 s0 = *(const float4*)sl;
        const float4 s1 = *(const float4*)(sl + 4);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const float d = ((tr.J[k][0] * s0.x + tr.J[k][1] * s0.y) + (tr.J[k][2] * s0.z + tr.J[k][3] * s0.w)) + (tr.J[k][4] * s1.x + tr.J[k][5] * s1.y);
            tr.cu[k][s2] = s2 == h + 8 * k ? 0.f : -tr.dinv[k] * d;
        }
        tr.cx[s2] = (blk_lane8 && h < 6) ? sl[h] : 0.f;
    }
    WV::lds_sync();      /* the slots share storage with the LDS rows of the rest contacts, built next */
}
/* u = app + rhs - (J . dv) / den from the block's current velocity changes (x in the DoF lanes of the half row) */
__device__ __forceinline__ void table_run_refresh(TableRun& tr, float x)
{
    float jd0 = 0.f, jd1 = 0.f;
#define PMG_TR_REFRESH(K) { const float v = WV::template half_bcast_c<K>(x); jd0 = fmaf(tr.J[0][K], v, jd0); jd1 = fmaf(tr.J[1][K], v, jd1); }
    PMG_TR_REFRESH(0) PMG_TR_REFRESH(1) PMG_TR_REFRESH(2) PMG_TR_REFRESH(3) PMG_TR_REFRESH(4) PMG_TR_REFRESH(5)
#undef PMG_TR_REFRESH
    tr.u[0] = tr.capp[0] + (tr.rhs[0] - jd0 * tr.dinv[0]);
    tr.u[1] = tr.capp[1] + (tr.rhs[1] - jd1 * tr.dinv[1]);
}
template <int S>
__device__ __forceinline__ void table_run_visit(TableRun& tr, int h, float lo, float hi, bool act, float& x)
{
    constexpr int sk = S >> 3, sl = S & 7;
    const float napp = __builtin_amdgcn_fmed3f(tr.u[sk], lo, hi);
    const float delta = act ? napp - tr.capp[sk] : 0.f;
    tr.capp[sk] = (h == sl && act) ? napp : tr.capp[sk];
    WV::template half_fma_bcast_c<sl>(delta, tr.cx[S], x);
    WV::template half_fma_bcast_c<sl>(delta, tr.cu[0][S], tr.u[0]);
    WV::template half_fma_bcast_c<sl>(delta, tr.cu[1][S], tr.u[1]);
}
template <int K>
__device__ __forceinline__ void table_run_normal(TableRun& tr, int h, float& x)
{
    constexpr int S = 3 * K;
    table_run_visit<S>(tr, h, 0.f, 1e10f, true, x);      /* a block without a K-th contact: u = 0 and all its coefficients are 0, nothing moves */
}
template <int K>
__device__ __forceinline__ void table_run_friction(TableRun& tr, int h, float& x)
{
    constexpr int S = 3 * K;
    const float nimp = WV::template half_bcast_c<(S & 7)>(tr.capp[S >> 3]);
    const bool act = nimp > 0.f;                                   /* per block */
    const float l1 = tr.mu[(S + 1) >> 3] * nimp, l2 = tr.mu[(S + 2) >> 3] * nimp;
    table_run_visit<S + 1>(tr, h, -l1, l1, act, x);
    table_run_visit<S + 2>(tr, h, -l2, l2, act, x);
}
__device__ __forceinline__ float table_run_residual(TableRun& tr)
{
    const float a = (tr.capp[0] - tr.cprev[0]) * tr.den[0], b = (tr.capp[1] - tr.cprev[1]) * tr.den[1];
    tr.cprev[0] = tr.capp[0]; tr.cprev[1] = tr.capp[1];
    return fmaxf(a * a, b * b);
}

/* One free object, four envs per wavefront: the object x table contacts (pair 0: the first contacts of the list, at
 * most four = twelve rows that touch the object alone) in row space, like a block's run above -- row r lives in lane r of
 * the env's 16-lane row next to the DoFs (another register), twelve coupling coefficients and twelve DoF shares per
 * lane, a visit = clamp, subtract, one v_fmac_f32_dpp pair.  The rows behind them (fingers on the table, gripper on the
 * object) stay LDS rows; u is re-derived from the object's velocity change whenever such rows have run. */
struct ObjectRun {
    float J[6], cu[12], cx[12];
    float u, capp, cprev, rhs, dinv, den, mu;
};
template <int NB, int MAXC, int CYL>
__device__ __forceinline__ void object_run_setup(ContactLds<NB, MAXC>& L, int T, ObjectRun& tr)
{
    const int l = WV::lane();
    const bool is_row = l < 3 * T;
    ObjRow w;
    obj_row_setup<NB, MAXC, CYL>(L, l, is_row, w);           /* (robot part zero: body B of pair 0 is the table) */
#pragma unroll
    for (int k = 0; k < 6; k++) tr.J[k] = w.Jo[k];
    tr.dinv = w.dinv; tr.den = w.den; tr.rhs = w.rhs; tr.mu = w.mu;
    tr.u = w.rhs; tr.capp = 0.f; tr.cprev = 0.f;
    float* slots = &L.rows[0][0];
    if (l < 12) {
        float4* my = (float4*)(slots + 8 * l);
        my[0] = make_float4(w.Ro[0], w.Ro[1], w.Ro[2], w.Ro[3]);
        my[1] = make_float4(w.Ro[4], w.Ro[5], 0.f, 0.f);
    }
    WV::lds_sync();
    const bool obj_lane = l >= NJ && l < NJ + 6;
    const float k_own = obj_lane ? 1.f : 0.f;
    const float* own_p = slots + (obj_lane ? l - NJ : 0);
#pragma unroll
    for (int s2 = 0; s2 < 12; s2++) {
        const float4 s0 = *(const float4*)(slots + 8 * s2), s1 = *(const float4*)(slots + 8 * s2 + 4);
        const float d = ((tr.J[0] * s0.x + tr.J[1] * s0.y) + (tr.J[2] * s0.z + tr.J[3] * s0.w)) + (tr.J[4] * s1.x + tr.J[5] * s1.y);
        tr.cu[s2] = s2 == l ? 0.f : -tr.dinv * d;
        tr.cx[s2] = k_own * own_p[8 * s2];                  /* (an unconditional read: `in ? slots[..] : 0` becomes a divergent branch around the load) */
    }
    WV::lds_sync();      /* the slots share storage with the LDS rows built next */
}
__device__ __forceinline__ void object_run_refresh(ObjectRun& tr, float x)
{
    float jd = 0.f;
#define PMG_OR_REFRESH(K) jd = fmaf(tr.J[K], WV::template bcast_r0_c<NJ + K>(x), jd);
    PMG_OR_REFRESH(0) PMG_OR_REFRESH(1) PMG_OR_REFRESH(2) PMG_OR_REFRESH(3) PMG_OR_REFRESH(4) PMG_OR_REFRESH(5)
#undef PMG_OR_REFRESH
    tr.u = tr.capp + (tr.rhs - jd * tr.dinv);
}
template <int S>
__device__ __forceinline__ void object_run_visit(ObjectRun& tr, int l, float lo, float hi, bool act, float& x)
{
    const float napp = __builtin_amdgcn_fmed3f(tr.u, lo, hi);
    const float delta = act ? napp - tr.capp : 0.f;
    tr.capp = (l == S && act) ? napp : tr.capp;
    WV::template fma2_bcast_r0_c<S>(delta, tr.cx[S], x, tr.cu[S], tr.u);   /* (the rows live in the first 16 lanes) */
}
template <int K>
__device__ __forceinline__ void object_run_normal(ObjectRun& tr, int l, float& x)
{
    object_run_visit<3 * K>(tr, l, 0.f, 1e10f, true, x);          /* an env without a K-th contact: u = 0 and all its coefficients are 0, nothing moves */
}
template <int K>
__device__ __forceinline__ void object_run_friction(ObjectRun& tr, int l, float& x)
{
    const float nimp = WV::template bcast_r0_c<3 * K>(tr.capp);
    const bool act = nimp > 0.f;                                   /* per env */
    const float lim = tr.mu * nimp;
    object_run_visit<3 * K + 1>(tr, l, -lim, lim, act, x);
    object_run_visit<3 * K + 2>(tr, l, -lim, lim, act, x);
}

/* reach: PGS iterations when finger x table contacts exist -- register-resident rows (RobotRows) */
template <int NB, int MAXC>
__device__ __forceinline__ void reach_contact_pgs(ContactLds<NB, MAXC>& L, int nc, NcRows& r, const float* minv_in, float& dv)
{
    float minv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) minv[j] = minv_in[j];
    McState mc;
    mc_init(r, minv, mc);
    RobotRows<MAXC> rr;
    load_robot_rows(L, nc, rr);
    for (int it = 0; it < SOLVER_ITERS; it++) {
        nc_sweep_auto(r, mc, (it & 1) != 0, minv, dv);
        float resid = WV::max_row0(fmaxf(robot_rows_iteration(rr, nc, dv), nc_residual(r)));   /* row 0 holds both */
        if (resid <= RESIDUAL_THRESHOLD) break;
    }
}

/* ------------------------------------------------------------------ */
/* one 2 ms substep: collide, unconstrained velocities, PGS rows, integrate
 * ([BULLET-PRIOR] btMultiBodyDynamicsWorld::internalSingleStepSimulation)  */
/* Two-wave workgroups (the one-env-per-workgroup lists with the full contact store): wavefront 1 of the workgroup runs
 * the narrowphase of a substep WHILE wavefront 0 computes the unconstrained dynamics (CRBA, M^-1, RNEA, free-body
 * update) of the same substep -- both need only the poses of the substep's start, and each is 5-30 k cycles of a serial
 * chain.  Hand-over through the env's LDS: wavefront 0 leaves the substep's joint angles in L.qd, workgroup barrier A; wavefront 1
 * runs its own forward kinematics from them, publishes the frames, collides and leaves the contact list + count (L.ncon),
 * workgroup barrier B.  Exactly two barriers per substep on either side and no data-dependent exits: the full stores
 * cannot overflow. */
template <int NB, int MAXC, int CYL, bool SPEC = false>
__device__ __forceinline__ void helper_wave_loop(const EnvParams& P, ContactLds<NB, MAXC>& L, const LaneTabStore& lcs, SpecLds<CYL>* sp = nullptr)
{
    /* the full-store layouts have no overflow exits.  The packed one-object layout (four envs per wavefront, 12 contacts
     * each) has: a row that overflows leaves the substep loop of wavefront 0 while the other rows -- and this wavefront --
     * carry on (s_barrier counts wavefronts, not lanes; a wavefront that has ended no longer takes part) */
    static_assert(NB == 0 || MAXC >= (NB == 1 ? 24 : 48) || (NB == 1 && WV::LANES == 16), "no helper wavefront for this layout");
    const int nb = NB > 0 ? P.nb : 0;
    const int l = WV::lane();
    LaneConst c;                                            /* (wavefront 0 filled the table before its first barrier A) */
    c.st = &lcs;
    c.col = l < NJ ? l : NJ - 1;
    for (int s = 0; s < RUN_SIM_STEPS * RUN_SUBSTEPS; s++) {
        __syncthreads();                                    /* A: the substep's joint angles are in L.qd */
        /* Round 6: this wavefront runs its OWN forward kinematics from the joint angles (the same fk() on the same numbers as
         * wavefront 0's: identical frames) and publishes the frames itself, instead of waiting for wavefront 0's forward kinematics
         * AND publication: the narrowphase starts 0.9 k cycles earlier and, with the dynamics + first motor sweep of wavefront 0
         * (6.0 k) now level with this branch (fk 1.7 k + narrowphase 4 k), nobody waits at barrier B. */
        LaneConst cc = c;
        WV::opaque(cc.col);
        Kin k;
        fk(cc, l < NJ ? L.qd[l] : 0.f, k);
        const bool low = (l == 7 || l == 8) && (finger_zmin(k.p, k.R) < P.table_c[2] + P.table_h[2] + CONTACT_MARGIN);
        const bool need = NB > 0 || WV::ballot(low) != 0ull;   /* without free bodies: only when a finger is near the table */
        int nc = 0;
        if (need) {
            publish_frames<NB, MAXC, CYL>(L, nb, k);
            /* inline for reach too: this wavefront's loop holds nothing else, and as a function of its own collide_cold
             * saves a callee-saved register to scratch memory on entry and waits for its reload on exit (it calls
             * box_face_clip) -- a memory round trip per substep on what is the longer branch of the hand-over */
            float tc[3] = {P.table_c[0], P.table_c[1], P.table_c[2]}, th[3] = {P.table_h[0], P.table_h[1], P.table_h[2]};
            nc = collide<NB, MAXC, CYL, SPEC>(L, lcs.kc, nb, tc, th, P.table_mu, sp);   /* (SPEC: barrier A2 inside, between narrowphase and compaction) */
        } else if (SPEC) __syncthreads();                   /* A2 */
        if (l == 0) L.ncon = nc;
        __syncthreads();                                    /* B: contacts + count are in LDS */
    }
}
/* Three-wavefront workgroups (slide's list 0): wavefront 2 repeats the finger x puck pairs in double beside the helper's float
 * forward kinematics + narrowphase (SpecLds, spec_fk, spec_pairs).  Three barriers per substep on every wavefront of the
 * workgroup: A (the substep's joint angles in L.qd, the free bodies' rows in L.blk since the last integration), A2 (the double
 * results in LDS; wavefront 0 passes it on its way to B), B (contacts in LDS). */
template <int NB, int MAXC, int CYL>
__device__ __forceinline__ void spec_wave_loop(const EnvParams& P, ContactLds<NB, MAXC>& L, const LaneTabStore& lcs, SpecLds<CYL>& sp)
{
    for (int s = 0; s < RUN_SIM_STEPS * RUN_SUBSTEPS; s++) {
        __syncthreads();                                    /* A */
        SpecFk fk;
        spec_fk<CYL>(sp, L.qd, fk);
        spec_pairs<NB, MAXC, CYL>(L, lcs.kc, sp, fk);
        __syncthreads();                                    /* A2 */
        __syncthreads();                                    /* B */
    }
}
template <int NB, int MAXC, int CYL, bool TWO = false, bool SPEC = false>
__device__ __forceinline__ bool substep(const EnvParams& P, ContactLds<NB, MAXC>& L, const LaneConst& c_in, float& q, float& qd,
                                        float tau, float mtarget, float mimp, int& ncmax, SpecLds<CYL>* sp = nullptr)
{
    static_assert(!SPEC || TWO, "the speculative wavefront rides with the helper wavefront");
    int l = WV::lane();
    if (TWO) {    /* the substep's joint angles for the other wavefronts of the workgroup (the free bodies' rows are in L.blk since the last
                   * substep's integration): the helper's own forward kinematics + narrowphase, the third wavefront's double repeat.
                   * L.qd is free until the rows are set up (and cyl_redo64 reads the angles there) */
        if (l < NJ) L.qd[l] = q;
        __syncthreads();                                    /* A */
    }
    const int nb = NB > 0 ? P.nb : 0;
#ifdef PMG_PROFILE
    long long tprev = prof::now();
#endif
    LaneConst c = c_in;
    WV::opaque(c.col); /* keep the LDS constant reads inside the loop (no 40-register hoist) */
    Kin k;
    fk(c, q, k);
    PMG_TICK(0);
    /* contact detection; without free bodies it is skipped (wave-uniform) unless a finger is near the table */
    int nc = 0;
    bool low = (l == 7 || l == 8) && (finger_zmin(k.p, k.R) < P.table_c[2] + P.table_h[2] + CONTACT_MARGIN);
    if (TWO) publish_subspaces<NB, MAXC>(L, k);            /* (the joint subspaces for this wavefront's own row set-up, behind barrier B) */
    else
    if (NB > 0 || WV::ballot(low) != 0ull)
        nc = detect<NB, MAXC, CYL>(L, c_in.st->kc, nb, k, q, P.table_c[0], P.table_c[1], P.table_c[2], P.table_h[0], P.table_h[1], P.table_h[2], P.table_mu);
    /* a contact store smaller than the task's full one (24 with one object, 48 with several) belongs to a fast
     * path: when it overflows the env is given up, untouched, to the kernel with the full store */
    if (!TWO && NB > 0 && MAXC < (NB == 1 ? 24 : 48) && nc > MAXC) return false;
    if (nc > MAXC) nc = MAXC;

    PMG_TICK(1);
    /* unconstrained velocity update: robot (CRBA + RNEA) ... */
    float I10[10], minv[NJ];
    body_inertia(c, k, I10);
    if (l >= NJ) {
#pragma unroll
        for (int a = 0; a < 10; a++) I10[a] = 0.f;
    }
    float h = bias_torque(c, k, I10, qd);   /* bias first: its temporaries are dead before the matrix work */
    mass_inverse(k, I10, minv);
    float rq = l < NJ ? tau - h : 0.f;
    float qdd = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; j++) qdd += minv[j] * WV::bcast_r0(rq, j);
    qd += DT * qdd;
    /* ... and the free objects: gravity, Bullet's base damping and the gyroscopic term w x (I w)
     * (zero for the isotropic cubes, not for the slide puck) */
    if (l < nb) {
        float* b = L.blk[l];
        /* the puck's rotation for the gyroscopic term.  Two-wavefront workgroups: L.blkR is the HELPER's, written behind barrier A
         * (publish_frames) for its narrowphase, and nothing orders that write against a read here, in front of barrier B -- this
         * wavefront takes the rotation from the quaternion itself, which nobody writes between A and B (the same quat_to_R on the same
         * numbers: the helper's bits).  tests/test_wave_order.py */
        float Rown[9];
        if (TWO && ObjT<CYL>::cyl) quat_to_R(b + 3, Rown);
        const float* Rm = (TWO && ObjT<CYL>::cyl) ? Rown : L.blkR[l];
        float kl = LINK_DAMPING * (1.f + sqrtf(dot3(b + 7, b + 7))), ka = LINK_DAMPING * (1.f + sqrtf(dot3(b + 10, b + 10)));
        float al[3] = {-b[10] * ka, -b[11] * ka, -b[12] * ka};
        if (ObjT<CYL>::cyl) {
            float wl[3], Iw[3], gy[3], tq[3];
            wl[0] = Rm[0] * b[10] + Rm[3] * b[11] + Rm[6] * b[12];
            wl[1] = Rm[1] * b[10] + Rm[4] * b[11] + Rm[7] * b[12];
            wl[2] = Rm[2] * b[10] + Rm[5] * b[11] + Rm[8] * b[12];
#pragma unroll
            for (int a = 0; a < 3; a++) Iw[a] = wl[a] / ObjT<CYL>::inv_inertia(a);
            cross3(wl, Iw, gy);
#pragma unroll
            for (int a = 0; a < 3; a++) tq[a] = (-Iw[a] * ka - gy[a]) * ObjT<CYL>::inv_inertia(a);
            mat3v(Rm, tq, al);
        }
#pragma unroll
        for (int a = 0; a < 3; a++) {
            b[7 + a] += DT * (-b[7 + a] * kl + (a == 2 ? -GRAVITY : 0.f));
            b[10 + a] += DT * al[a];
        }
    }
    PMG_TICK(2);
    NcRows r;
    build_nc_rows(c, minv, q, qd, mtarget, mimp, r);
    McState mc;
    mc_init(r, minv, mc);
    /* Two-wavefront reach kernel: the helper's detection (6.5 k cycles) outlasts the dynamics above (3.5 k since round 4), and
     * this wavefront would wait at barrier B.  Iteration 0's pass over the motor / limit rows starts from zero impulses and
     * depends on nothing the helper produces: it runs HERE, and the solves below resume behind it. */
    bool pre = false;
    float um_pre = 0.f, ul_pre = 0.f, dv_pre = 0.f;
    /* (reach: the one-wavefront kernels too -- the same arithmetic, bit for bit.  The lists with objects: the two-wavefront
     * kernels, whose wavefront 0 waits even longer for its helper) */
    if (PMG_PRE_SWEEP && WV::LANES == 64 && mc.fast && (NB == 0 ? (PMG_ROWSPACE && MAXC <= 8) : (TWO && PMG_PRE_SWEEP_OBJ && NB != 6))) {   /* (not the chest lists: five spilled registers for + 0.5 %) */
        um_pre = r.rhs_m; ul_pre = r.rhs_l;
        mc_sweep(r, mc, false, um_pre, ul_pre);
        mc_apply(minv, r.app_m + r.sg_l * r.app_l, dv_pre);
        pre = true;
    }
    if (TWO) {
        if (SPEC) __syncthreads();                          /* A2: between the helper and the speculative wavefront; nothing of this wavefront's */
        __syncthreads();                                    /* B: the helper wavefront's contacts are in */
        nc = L.ncon;
        if (NB > 0 && MAXC < (NB == 1 ? 24 : 48) && nc > MAXC) return false;   /* (fast-path store: see above) */
        if (nc > MAXC) nc = MAXC;
    }
    ncmax = nc > ncmax ? nc : ncmax;                        /* (diagnostics: PMG_ENV_CYCLES) */    /* reach, one env per wavefront: lanes 16..39 are free, the contact rows are built and solved in row space */
    const bool rowspace = PMG_ROWSPACE && NB == 0 && WV::LANES == 64 && MAXC <= 8 && mc.fast;
    /* one free object, one env per wavefront: the same for up to OBJ_ROWSPACE_MAXC contacts (lanes 16..63 = 48 rows) */
    const bool rowspace1 = PMG_ROWSPACE && NB == 1 && WV::LANES == 64 && mc.fast && nc > 0 && nc <= OBJ_ROWSPACE_MAXC;
    /* several blocks: the leading block x table run in row space (table_run_*); LDS rows only for what comes behind it */
    LaneDof<NB> ld;
    lane_dof(ld);
    int trun = 0, tmax = 0;
    if (NB > 1 && nc > 0) table_runs(L, nb, nc, ld, trun, tmax);
    const bool trs = PMG_TABLE_ROWSPACE && NB > 1 && WV::LANES == 64 && trun > 0;
    TableRun tr;
    if (trs) table_run_setup<NB, MAXC>(L, ld, tr);
    /* one object, four envs per wavefront: the object x table contacts in row space (object_run_*), per env */
    /* (one env per wavefront: the LDS-row path of an env with more contacts than the row-space solve holds) */
    constexpr bool ors = PMG_TABLE_ROWSPACE && NB == 1;
    ObjectRun orun;
    int orT = 0;
    if (ors && !rowspace1 && (WV::LANES == 16 || nc > 0)) {
        orT = L.pair_count[0] < nc ? L.pair_count[0] : nc;
        if (l < NJ) {                                          /* M^-1 and the joint velocities for the row set-ups */
#pragma unroll
            for (int j = 0; j < NJ; j++) L.minv[l][j] = minv[j];
            L.qd[l] = qd;
        }
        WV::lds_sync();
        object_run_setup<NB, MAXC, CYL>(L, orT, orun);
        build_rows_by_lane<NB, MAXC, CYL>(L, nc, orT);
    } else
    if (nc > (trs ? trun : 0) && !rowspace && !rowspace1) prepare_rows<NB, MAXC, CYL>(L, minv, qd, nc, trs ? trun : 0);
    PMG_TICK(3);
    float dv = 0.f; /* lanes 0..8: joint velocity change; block DoFs in the lanes of LaneDof<NB> */
    if (NB == 0) {
        if (nc > 0 && rowspace) reach_contact_pgs_rowspace<NB, MAXC>(L, nc, r, mc, minv, qd, dv, pre, dv_pre);
        else if (nc > 0) reach_contact_pgs<NB, MAXC>(L, nc, r, minv, dv);
        else nc_solve_free(r, mc, minv, dv, pre, um_pre, ul_pre);
    } else if (rowspace1) {
        obj_contact_pgs_rowspace<NB, MAXC, CYL>(L, nc, r, mc, minv, qd, dv, pre, dv_pre);
    } else {
        /* chest door: joint limits and (once latched) the position motor of chest.py:59-68 -- rows on the door DoF alone,
         * solved by its lane between the robot's non-contact rows and the contacts (oracle substep()) */
        constexpr int CK = ObjT<CYL>::chest >= 0 ? ObjT<CYL>::chest : 0;
        float d_rhs[3] = {0.f, 0.f, 0.f}, d_j[3] = {0.f, 0.f, 0.f}, d_lo[3] = {0.f, 0.f, 0.f}, d_hi[3] = {0.f, 0.f, 0.f}, d_app[3] = {0.f, 0.f, 0.f};
        const bool door_lane = ObjT<CYL>::chest >= 0 && l == LaneDof<NB>::lane_of(nb, ChestT::comp(CK));
        if (ObjT<CYL>::chest >= 0) {
            const float dq = L.door[0], dqd = L.door[1], dm = ChestT::mass(CK);
            const float ju = ChestT::sign(CK) * door_scale(CK);    /* d(joint velocity) / d(this lane's scaled velocity) */
            if (L.door[2] != 0.f) {
                float target_v = ARM_KP * (ChestT::open_state(CK) - dq) / DT + dqd + ARM_KD * (0.f - dqd);
                d_j[0] = ju; d_rhs[0] = (target_v - dqd) * dm; d_lo[0] = -500.f * PHYSICS_DT; d_hi[0] = 500.f * PHYSICS_DT;
            }
            if (!(dq > 0.f)) { d_j[1] = ju; d_rhs[1] = (-dq * JOINT_ERP / DT - dqd) * dm; d_hi[1] = LIMIT_MAX_IMPULSE; }
            const float pen = ChestT::upper(CK) - dq;
            if (!(pen > 0.f)) { d_j[2] = -ju; d_rhs[2] = (-pen * JOINT_ERP / DT + dqd) * dm; d_hi[2] = LIMIT_MAX_IMPULSE; }
        }
        if (pre) dv = dv_pre;                                  /* (joint lanes; zero elsewhere) */
        for (int it = 0; it < SOLVER_ITERS; it++) {
            PMG_TICK(10);
            if (!(pre && it == 0)) nc_sweep_auto(r, mc, (it & 1) != 0, minv, dv);
            float dres = 0.f;
            if (ObjT<CYL>::chest >= 0) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    if (d_j[k] != 0.f) {      /* uniform: the row exists */
                        const float dm = ChestT::mass(CK);
                        float sum = d_app[k] + (d_rhs[k] - d_j[k] * dv * dm);
                        float napp = fminf(fmaxf(sum, d_lo[k]), d_hi[k]);
                        float delta = napp - d_app[k];
                        d_app[k] = napp;
                        if (door_lane) { dv += d_j[k] * (1.f / BLOCK_MASS) * delta; dres = fmaxf(dres, (delta / dm) * (delta / dm)); }
                    }
                }
            }
            PMG_TICK(8);
            float resid = 0.f;
            if (trs) {
                const int h = l & 7;
                const bool rest = nc > trun;                  /* rows behind the run change the block velocities in DoF space */
                if (rest && it > 0) table_run_refresh(tr, dv);
                if (0 < tmax) table_run_normal<0>(tr, h, dv);
                if (1 < tmax) table_run_normal<1>(tr, h, dv);
                if (2 < tmax) table_run_normal<2>(tr, h, dv);
                if (3 < tmax) table_run_normal<3>(tr, h, dv);
                unsigned long long loaded;
                resid = lds_rest_normals<NB, MAXC>(L, nc, trun, ld, dv, loaded);
                if (rest) table_run_refresh(tr, dv);
                if (0 < tmax) table_run_friction<0>(tr, h, dv);
                if (1 < tmax) table_run_friction<1>(tr, h, dv);
                if (2 < tmax) table_run_friction<2>(tr, h, dv);
                if (3 < tmax) table_run_friction<3>(tr, h, dv);
                resid = fmaxf(resid, lds_rest_frictions<NB, MAXC>(L, ld, dv, loaded));
                resid = fmaxf(resid, table_run_residual(tr));
            } else if (ors && (WV::LANES == 16 || nc > 0)) {
                const bool rest = nc > orT;
                if (rest && it > 0) object_run_refresh(orun, dv);
                object_run_normal<0>(orun, l, dv); object_run_normal<1>(orun, l, dv);
                object_run_normal<2>(orun, l, dv); object_run_normal<3>(orun, l, dv);
                unsigned long long loaded;
                resid = lds_rest_normals<NB, MAXC>(L, nc, orT, ld, dv, loaded);
                if (rest) object_run_refresh(orun, dv);
                object_run_friction<0>(orun, l, dv); object_run_friction<1>(orun, l, dv);
                object_run_friction<2>(orun, l, dv); object_run_friction<3>(orun, l, dv);
                resid = fmaxf(resid, lds_rest_frictions<NB, MAXC>(L, ld, dv, loaded));
                const float dc = (orun.capp - orun.cprev) * orun.den;
                orun.cprev = orun.capp;
                resid = fmaxf(resid, dc * dc);
            } else if (nc > 0) resid = lds_rows_iteration(L, nc, ld, dv, trun, tmax);
            PMG_TICK(9);
            resid = fmaxf(resid, nc_residual(r));
            if (ObjT<CYL>::chest >= 0) resid = fmaxf(resid, dres);
            /* residuals are per lane (valid where the DoFs live): one reduction per iteration */
            if (!WV::any_lane(resid > RESIDUAL_THRESHOLD)) break;   /* (a ballot, no cross-lane maximum) */
        }
    }
    PMG_TICK(4);
    if (l < NJ) qd += dv;
    q += DT * qd;
    if (NB > 0) {
        {
            LaneDof<NB> sd;
            lane_dof(sd);
            if (sd.blk >= 0 && sd.blk < nb + (ObjT<CYL>::chest >= 0 ? 1 : 0)) L.blk[sd.blk][7 + sd.comp] += dv;
        }
        WV::lds_sync();
        if (ObjT<CYL>::chest >= 0 && l == 0) {
            constexpr int K = ObjT<CYL>::chest >= 0 ? ObjT<CYL>::chest : 0;
            float nqd = ChestT::sign(K) * door_scale(K) * L.blk[nb][7 + ChestT::comp(K)];
            L.door[1] = nqd;
            L.door[0] += DT * nqd;
        }
        if (l < nb) {
            float* b = L.blk[l];
#pragma unroll
            for (int a = 0; a < 3; a++) b[a] += DT * b[7 + a];
            /* quat <- exp(omega dt) * quat */
            float wn = sqrtf(dot3(b + 10, b + 10));
            float ang = wn * DT;
            float dq[4] = {0.f, 0.f, 0.f, 1.f};
            if (ang > 1e-12f) {
                float sh, ch;
                sincos_joint(0.5f * ang, &sh, &ch);   /* (half the rotation of one substep: small; the minimax pair of the joint angles, no libm slow path) */
                float s = sh / wn;
                dq[0] = b[10] * s; dq[1] = b[11] * s; dq[2] = b[12] * s; dq[3] = ch;
            }
            float x = dq[3] * b[3] + dq[0] * b[6] + dq[1] * b[5] - dq[2] * b[4];
            float y = dq[3] * b[4] + dq[1] * b[6] + dq[2] * b[3] - dq[0] * b[5];
            float z = dq[3] * b[5] + dq[2] * b[6] + dq[0] * b[4] - dq[1] * b[3];
            float w = dq[3] * b[6] - dq[0] * b[3] - dq[1] * b[4] - dq[2] * b[5];
            float inv = 1.f / sqrtf(x * x + y * y + z * z + w * w);
            b[3] = x * inv; b[4] = y * inv; b[5] = z * inv; b[6] = w * inv;
        }
        WV::lds_sync();
    }
    return true;
}

/* ------------------------------------------------------------------ */
/* env.step(): kuka.py:167-225 + _get_obs + _compute_reward + TimeLimit */
/* `live` = this env's results are to be stored (false for the shadow rows of a partly filled packed wavefront);
 * returns false when the packed path gave up on the env (more contacts than its small LDS row store holds): nothing
 * has been written then and the caller queues the env for the one-env-per-wavefront kernel */
/* which wavefront of a two-wavefront workgroup is the helper (the other one carries the env's dynamics): PMG_REACH_HELPER_WAVE for
 * reach, wavefront 1 on the tasks with objects (slide's third wavefront is always wavefront 2) */
template <int NB, bool SPEC>
__device__ __forceinline__ constexpr int helper_wave_index() { return (NB == 0 && !SPEC) ? PMG_REACH_HELPER_WAVE : 1; }
template <int NB, int MAXC, int CYL, bool TWO = false, bool SPEC = false>
__device__ __forceinline__ bool step_env_core(const EnvParams& P, const float* actions, int env, ContactLds<NB, MAXC>& L,
                                              LaneTabStore& lcs, bool live, SpecLds<CYL>* sp = nullptr)
{
    if constexpr (TWO) {
#ifdef PMG_PROFILE
        static_assert(!TWO, "PMG_PROFILE adds workgroup barriers to wavefront 0 only: profile the one-wavefront kernels");
#endif
        if (((int)threadIdx.x >> 6) == helper_wave_index<NB, SPEC>()) {   /* the helper wavefront */
            helper_wave_loop<NB, MAXC, CYL, SPEC>(P, L, lcs, sp);
            return true;
        }
        if constexpr (SPEC) {
            if (((int)threadIdx.x >> 6) == 2) {             /* the speculative wavefront */
                spec_wave_loop<NB, MAXC, CYL>(P, L, lcs, *sp);
                return true;
            }
        }
    }
    int l = WV::lane();
#ifdef PMG_PROFILE
    prof::begin();
#endif
    const long long t_begin = P.env_cycles ? wv::cycles() : 0ll;
    int ncmax = 0;
    LaneConst c;
    load_lane_const(lcs, c);
    float* hot = P.hot + (size_t)env * HOT_DIM;
    int ll = l < NJ ? l : 0;
    float q = hot[ll], qd = hot[9 + ll];
    if (l >= NJ) { q = 0.f; qd = 0.f; }
    const int nb = NB > 0 ? P.nb : 0;
    float* gblk = P.blocks + (size_t)env * BLOCK_DIM * P.nb;
    for (int i = l; i < BLOCK_DIM * nb; i += WV::LANES) L.blk[i / BLOCK_DIM][i % BLOCK_DIM] = gblk[i];
    if (ObjT<CYL>::chest >= 0 && l < 4) L.door[l] = l < 3 ? P.goal[(size_t)env * GOAL_DIM + l] : (float)nb; /* door q, qd, motor latch */
    if (l == 0) {   /* the batch's constant narrowphase operands (LaneTabStore::kc; every env of the workgroup writes the same) */
        constexpr float FH[3] = PMG_FINGER_HALF;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lcs.kc[a] = P.table_c[a]; lcs.kc[3 + a] = P.table_h[a];
            lcs.kc[15 + a] = FH[a]; lcs.kc[18 + a] = ObjT<CYL>::half(a);
            constexpr float PH[3] = PMG_PLANE_HALF;
            lcs.kc[KC_PLANE_H + a] = PH[a];
        }
#pragma unroll
        for (int a = 0; a < 9; a++) lcs.kc[6 + a] = (a % 4 == 0) ? 1.f : 0.f;
    }
#ifdef PMG_PROFILE
    long long tprev = prof::now();
#endif
    const float* act = actions + (size_t)env * P.adim;
    float grip = hot[28];
    int elapsed = (int)hot[29];
    if (P.grasping) grip = (float)(((double)act[P.adim - 1] + 1.0) * (0.035 / 2)); /* kuka.py:171 */
    float mtarget = grip, mimp = FINGER_FORCE * PHYSICS_DT;
    float ee[3] = {hot[18], hot[19], hot[20]};
    float jt = l < 7 ? hot[21 + l] : 0.f;
    if (P.joint_control) {
        if (l < 7) jt = act[l] * 0.05f + jt; /* kuka.py:205 */
        if (l < 7) mtarget = jt;
    } else {
#pragma unroll
        for (int a = 0; a < 3; a++) {      /* kuka.py:209-212 */
            float t = ee[a] + act[a] * 0.01f;
            ee[a] = fminf(fmaxf(t, P.ee_lo[a]), P.ee_hi[a]);
        }
        float qik = ik_solve(c, q, ee);    /* kuka.py:214 */
        if (l < 7) mtarget = qik;
    }
    if (l < 7) mimp = ARM_FORCE * PHYSICS_DT; /* kuka.py:282-290 */
    WV::lds_sync();
    PMG_TICK(5);
    bool ok = true;
    for (int s = 0; s < RUN_SIM_STEPS && ok; s++) {  /* kuka.py:223-225 */
        float tau = -c.jdamp() * qd;         /* joint damping latched per stepSimulation */
        for (int ss = 0; ss < RUN_SUBSTEPS && ok; ss++) ok = substep<NB, MAXC, CYL, TWO, SPEC>(P, L, c, q, qd, tau, mtarget, mimp, ncmax, sp);
    }
    PMG_TICK(6);
    if (!ok || !live) return ok;
    if (P.env_cycles && l == 0) {
        P.env_cycles[2 * env] = (int)((wv::cycles() - t_begin) >> 6);
        P.env_cycles[2 * env + 1] = ncmax;
    }
    elapsed++;
    if (l < NJ) { hot[l] = q; hot[9 + l] = qd; }
    if (l < 3) hot[18 + l] = l == 0 ? ee[0] : (l == 1 ? ee[1] : ee[2]);
    if (l < 7) hot[21 + l] = jt;
    if (l == 0) { hot[28] = grip; hot[29] = (float)elapsed; hot[30] = 1.f; }
    for (int i = l; i < BLOCK_DIM * nb; i += WV::LANES) gblk[i] = L.blk[i / BLOCK_DIM][i % BLOCK_DIM];
    if (ObjT<CYL>::chest >= 0 && l < 3) {
        /* _get_obs keeps a door it finds open open: the position motor holds it from now on
         * (kuka_multi_step_base_env.py:296-298) */
        constexpr int K = ObjT<CYL>::chest >= 0 ? ObjT<CYL>::chest : 0;
        float v = L.door[l];
        if (l == 2 && fabsf(ChestT::open_state(K) - L.door[0]) <= 0.01f) v = 1.f;
        P.goal[(size_t)env * GOAL_DIM + l] = v;
    }
    WV::lds_sync();
    write_outputs(P, env, c, q, qd, elapsed, TAIL_REWARD);
    PMG_TICK(7);
#ifdef PMG_PROFILE
    prof::flush(P.prof);
#endif
    return true;
}

