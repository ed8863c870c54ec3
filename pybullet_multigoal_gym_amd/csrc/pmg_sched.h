/*
 * pmg_sched.h -- the launch schedule of a batched step: ONE definition of the int buffer EnvParams::sched
 * (PMG_BUF_SCHED of include/pmg.h; mirrored once more in Python, _lib.py schedule()).  The plan kernels fill it, every
 * step kernel reads its env from it, the fast paths queue the envs they give up on its redo list.  With N = n_envs:
 *
 *   [0] [1]                     counts of list 0 (contact-prone / full contact store: one env per wavefront) and of
 *                               list 1 (the fast paths)
 *   [2 .. 2 + N)                list 0
 *   [2 + N .. 2 + 2N)           list 1
 *   [2 + 2N]                    redo count, zeroed by the plan
 *   [3 + 2N .. 3 + 3N)          redo list: envs a fast path gave up, recomputed by the pmg_k_redo kernels
 *   [3 + 3N .. + 3 ceil(N / 1024))  class counts of every workgroup of the two-pass plan (plan_count -> plan_scatter)
 *   last word                   did the plan promote the fingers-down class to list 0 (pmg_k_step_list's issue priority)
 *
 * Host code, device code and the CPU emulator build all go through this view; nothing else does index arithmetic on it.
 */
#ifndef PMG_SCHED_H
#define PMG_SCHED_H

#include <cstddef>

namespace pmgx {
struct Sched {
    int* w;
    int n;   /* n_envs */
    static constexpr int PLAN_WG = 1024;   /* envs per workgroup of the two-pass plan (= pmg::PLAN_THREADS) */
    __host__ __device__ static constexpr size_t words(size_t n_envs) { return 4 + 3 * n_envs + 3 * ((n_envs + PLAN_WG - 1) / PLAN_WG); }
    __host__ __device__ __forceinline__ int& count(int list) const { return w[list]; }
    __host__ __device__ __forceinline__ int& at(int list, int i) const { return w[2 + list * n + i]; }   /* element i of a list */
    __host__ __device__ __forceinline__ int* list(int list) const { return &at(list, 0); }
    __host__ __device__ __forceinline__ int& redo_count() const { return *redo(); }
    __host__ __device__ __forceinline__ int* redo_list() const { return redo() + 1; }
    __host__ __device__ __forceinline__ int* wg_counts() const { return w + 3 + 3 * (size_t)n; }
    __host__ __device__ __forceinline__ int& promoted() const { return *(w + 3 + 3 * (size_t)n + 3 * (size_t)((n + PLAN_WG - 1) / PLAN_WG)); }
    /* a fast path gives env up: nothing of it was written, a pmg_k_redo kernel recomputes it (one lane of the env calls this) */
    __device__ __forceinline__ void push_redo(int env) const
    {
        int* r = redo();
        const int slot = atomicAdd(r, 1);
        r[1 + slot] = env;
    }
    /* the redo pass, one workgroup per env of the redo list: the env of workgroup `block` (< redo_count()) */
    __device__ __forceinline__ int redo_env(unsigned block) const { return redo()[1 + block]; }
    /* four envs of list 1 per wavefront, one per 16-lane row: the env of this row of wavefront `group` (4 * group < count(1)).
     * Surplus rows of the last wavefront shadow the list's last env (have = false) and must write nothing */
    __device__ __forceinline__ int packed_row(int group, int row, bool& have) const
    {
        const int n1 = count(1), idx = 4 * group + row;
        have = idx < n1;
        return at(1, have ? idx : n1 - 1);
    }
    /* one env per workgroup, list 0 first: the env of workgroup `block` (< count(0) + count(1)) */
    __device__ __forceinline__ int env_of_block(int block) const
    {
        const int n0 = count(0);
        return block < n0 ? at(0, block) : at(1, block - n0);
    }

private:
    __host__ __device__ __forceinline__ int* redo() const { return w + 2 + 2 * n; }   /* [0] the count, [1 ..] the list */
};
}  // namespace pmgx
#endif
