// hvp_seq.hip -- the stage glue of the sequential MLD controller (fleet_seq_mld.py:296-440,
// TrackingSequentialMldCoordinator.get_control) on the device; C ABI in include/hvp_seq.h.
//
// The n local problems of a sequential step form a chain: the leader L solves first, then
// L-1 .. 0, then L+1 .. n-1, and every vehicle is handed the trajectory its neighbour on the
// leader's side solved in THIS step (unshifted) and the other neighbour's trajectory of the
// PREVIOUS step (shifted by one sample, last position re-extrapolated).  A batch of P platoons
// runs the chain as n stages of P instances; between two stages this kernel turns the prediction
// store into the next stage's parameter blocks, so the chain stays in HBM.
//
// The store is vehicle-major, xpred [n][P][2][N+1]: stage i's hvp_solve_batch writes its x_out
// straight into slot i, and given the order of solves one buffer serves both readings -- a
// "shifted" neighbour has not solved yet in this step (its slot still holds the previous step's
// trajectory), a "fresh" one has.
#include <hip/hip_runtime.h>

#include <string>

#define HVP_HD __host__ __device__
#include "hvp_seq.h"
#include "hvp_internal.h"

using hvp_detail::fail;

namespace {

// One thread per platoon writes instance p's block (include/hvp.h layout: x0 | x_front | x_back |
// leader_x) and role bits for stage vehicle i.  Thread p reads the 2(N+1) contiguous doubles of
// its platoon in a neighbour's slot, and the threads of a wave read adjacent platoons of the same
// slot, so every cache line fetched is used in full.
__global__ __launch_bounds__(256) void k_seq_stage_params(int P, int n, int N, int i, const double* __restrict__ x,
                                                          const double* __restrict__ xpred,
                                                          const double* __restrict__ leader_x, int leader, int rvar,
                                                          int first, double ts, double* __restrict__ params,
                                                          int32_t* __restrict__ roles) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int K = N + 1;
    const double* xp = x + (size_t)p * 2 * n;
    double* out = params + (size_t)p * (2 + 6 * K);
    out[0] = xp[2 * i];
    out[1] = xp[2 * i + 1];
    auto slot = [&](int j) { return xpred + ((size_t)j * P + p) * 2 * K; };
    // the trajectory vehicle j solved in this step, as it is (get_predicted_state(shifted=False))
    auto fresh = [&](int j, double* dst) {
        const double* s = slot(j);
        for (int k = 0; k < 2 * K; ++k) dst[k] = s[k];
    };
    // vehicle j's previous trajectory shifted by one sample (get_predicted_state(shifted=True):
    // column 0 dropped, the last repeated) with the last position p_N + ts v_N (:342-344); before
    // any prediction exists, the constant-velocity extrapolation of j's state (:413-440)
    auto shifted = [&](int j, double* dst) {
        if (first) {
            double pp = xp[2 * j];
            const double vv = xp[2 * j + 1];
            dst[0] = pp;
            dst[K] = vv;
            for (int k = 0; k < N; ++k) {
                pp = pp + ts * vv;
                dst[k + 1] = pp;
                dst[K + k + 1] = vv;
            }
            return;
        }
        const double* s = slot(j);
        for (int k = 0; k < N; ++k) {
            dst[k] = s[k + 1];
            dst[K + k] = s[K + k + 1];
        }
        dst[N] = s[N] + ts * s[K + N];
        dst[K + N] = s[K + N];
    };
    auto zero = [&](double* dst) {
        for (int k = 0; k < 2 * K; ++k) dst[k] = 0.0;
    };
    double* xf = out + 2;
    double* xb = out + 2 + 2 * K;
    double* xl = out + 2 + 4 * K;
    if (i == 0) zero(xf);
    else if (i > leader) fresh(i - 1, xf);
    else shifted(i - 1, xf);
    if (i == n - 1) zero(xb);
    else if (i < leader) fresh(i + 1, xb);
    else shifted(i + 1, xb);
    const double* lw = leader_x + (size_t)p * 2 * K;
    for (int k = 0; k < 2 * K; ++k) xl[k] = i == leader ? lw[k] : 0.0;
    int r = 0;  // tables.role_bits, as k_decent_params (hvp_env.hip) writes them
    if (i != 0) r |= HVP_ROLE_SAFE_FRONT;
    if (i != n - 1) r |= HVP_ROLE_SAFE_BACK;
    if (i != 0 && i != leader) r |= HVP_ROLE_TRACK_FRONT;
    if (i != n - 1 && i != leader) r |= HVP_ROLE_TRACK_BACK;
    if (i == leader) r |= HVP_ROLE_TRACK_LEADER | (rvar ? HVP_ROLE_LEADER_SPACING : 0);
    roles[p] = r;
}

}  // namespace

extern "C" {

int hvp_seq_stage_params(hvp_handle* h, int P, int n, int i, const double* x, const double* xpred,
                         const double* leader_x, int leader_index, int real_vehicle_as_reference, int first,
                         double* params, int32_t* roles, void* stream) {
    if (!h) return fail(HVP_E_ARG, "hvp_seq_stage_params: null handle");
    if (h->prob.formulation != HVP_FORM_DECENT)
        return fail(HVP_E_ARG, "hvp_seq_stage_params: the handle is not an HVP_FORM_DECENT problem");
    if (P < 0 || n < 1 || leader_index < 0 || leader_index >= n)
        return fail(HVP_E_ARG, "hvp_seq_stage_params: bad layout");
    if (i < 0 || i >= n) return fail(HVP_E_ARG, "hvp_seq_stage_params: stage vehicle out of range");
    if (P == 0) return 0;
    if (!x || !xpred || !leader_x || !params || !roles) return fail(HVP_E_ARG, "hvp_seq_stage_params: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_seq_stage_params, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, n,
                       h->prob.N, i, x, xpred, leader_x, leader_index, real_vehicle_as_reference ? 1 : 0,
                       first ? 1 : 0, h->prob.ts_acc, params, roles);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
