/* pmg_plan_probe.inc -- TEST INFRASTRUCTURE: what the plan probe of the device (pmgd_plan, pmg_gpu_probe.hip) and of the emulator
 * (pmge_plan, tests/emu/pmg_probe.cpp) share: the check of the caller's arguments and the kernel parameters of one call.  Host code */
static bool plan_args_ok(int mode, int n_envs, int nb, int chest, int joint_control, int lpt_thresh, int lpt_permille, int lpt_parity, const int* env_cycles,
                         const int* lpt_state, const float* hot, const float* blocks, const float* actions, int adim, int guard, const int* buf)
{
    if (mode < 0 || mode > 2 || n_envs < 1 || n_envs > 131072 || nb < 0 || nb > 5 || chest < -1 || chest > 1 || adim < 3 || adim > 16) return false;
    if (mode != 2 && n_envs > pmg::PLAN_SINGLE_MAX) return false;
    if (mode == 1 && (nb != 0 || joint_control)) return false;
    if (!hot || !actions || !buf || (nb > 0 && !blocks) || guard < 0 || guard > 4096 || (lpt_parity != 0 && lpt_parity != 1)) return false;
    if (env_cycles && lpt_thresh <= 0 && lpt_permille > 0 && !lpt_state) return false;
    if (env_cycles)
        for (int i = 0; i < n_envs; i++)
            if (env_cycles[2 * i] < 0) return false;       /* (a negative count would index the histogram below its first bin) */
    return true;
}
static pmg::EnvParams plan_params(int n_envs, int nb, int chest, int joint_control, float near_r, float chest_reach, int fd_div, int wave_budget, int lpt_thresh,
                                  int lpt_permille, int lpt_parity, int adim)
{
    pmg::EnvParams P;
    memset(&P, 0, sizeof(P));
    P.n_envs = n_envs; P.nb = nb; P.adim = adim; P.chest = chest; P.joint_control = joint_control; P.has_obj = nb > 0;
    P.near_r = near_r; P.chest_reach = chest_reach; P.fd_div = fd_div; P.wave_budget = wave_budget;
    P.lpt_thresh = lpt_thresh; P.lpt_permille = lpt_permille; P.lpt_parity = lpt_parity;
    const float lo[3] = {-0.67f, -0.2f, 0.175f}, hi[3] = {-0.37f, 0.2f, 0.55f}, th[3] = PMG_TABLE_HALF;
    for (int a = 0; a < 3; a++) { P.ee_lo[a] = lo[a]; P.ee_hi[a] = hi[a]; P.table_h[a] = th[a]; }
    P.table_c[0] = -0.52f; P.table_c[1] = 0.f; P.table_c[2] = 0.08f;
    return P;
}
