// hvp_event.hip -- the event-based controller (fleet_event_based.py) on the device; C ABI in
// include/hvp_event.h.
//
// The local problem of agent i (LocalMpc, :26-341) is the centralised platoon MIQP over the
// m <= 3 vehicles [i-1, i, i+1] plus the fixed trajectories of the vehicles two places away and a
// leader term on any local vehicle: the wave QP and the joint branch and bound of hvp_cent.h /
// hvp_cent_bnb.h compiled with HVP_CENT_EVENT (the boundary blocks, Inst::xf2 / xb2, and a tenth
// row slot).  One wavefront per local problem, V = m N <= 48 lanes in use; the single-wave search
// (no split tasks).  The evaluation of fixed guesses (eval_cost, :308-327) and the coordinator's
// stages (gather, winner rule, shift; :460-646) are one thread per item.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#define HVP_HD __host__ __device__
#define HVP_CENT_EVENT 1
#include "hvp_event.h"
#include "hvp_internal.h"  // before the centralised headers: it names hvp::cent::Child, their ev::Child comes after
#include "hvp_cent_bnb.h"

using hvp_detail::fail;

namespace {

namespace ce = hvp::cent::ev;

constexpr int kMaxM = 3;  // local vehicles

__device__ inline int ev_stride(int N) { return 6 + 6 * (N + 1); }

// ------------------------------------------------------------------ solve
__global__ __launch_bounds__(64) void k_event_bnb(int B, int N, const hvp_event_desc* __restrict__ desc,
                                                  const hvp_system* __restrict__ systems,
                                                  const int32_t* __restrict__ sys, const double* __restrict__ params,
                                                  const hvp::Consts* __restrict__ Cp, int nreg_max, int max_nodes,
                                                  int exhaustive, int debug, ce::Child* frames, uint64_t* ties,
                                                  double* u_out, double* x_out, int8_t* region_out, int8_t* gear_out,
                                                  double* cost_out, int32_t* status_out, int32_t* nodes_out,
                                                  int32_t* iters_out, unsigned long long* counter) {
    using namespace hvp::cent::ev;
    extern __shared__ double event_lds[];
    const hvp::Consts& C = *Cp;
    const int b = blockIdx.x;
    if (b >= B) return;
    const hvp_event_desc d = desc[b];
    const int m = d.m, V = m * N;
    const double* prm = params + (size_t)b * ev_stride(N);
    const Lds S = lds_carve(event_lds, V);
    Inst I;
    I.n = m;
    I.N = N;
    I.V = V;
    I.L = d.leader;  // -1: no local vehicle tracks the leader
    I.lsp = false;
    I.systems = systems;
    I.vsys = sys + (size_t)b * kMaxM;
    I.x0 = prm;
    I.xf2 = d.has_f2 ? prm + 6 : nullptr;
    I.xb2 = d.has_b2 ? prm + 6 + 2 * (N + 1) : nullptr;
    I.xl = prm + 6 + 4 * (N + 1);
    I.debug = debug;
    Lane L;
    Search st;
    Result res;
    bnb_platoon<false>(L, S, C, I, st, frames + (size_t)b * kMaxM * N * nreg_max, nreg_max,
                       ties + (size_t)b * kTie * kMaxM, max_nodes, exhaustive != 0, 8 * ROWS * V, res, nullptr);
    // the winner's outputs: lane t = i N + a stores u_{i,a}, x_{i,a+1}, region and gear; the slots of
    // vehicles >= m are zeroed by lanes V .. 3 N - 1
    const int t = lane();
    const bool win = res.status == HVP_OPTIMAL;
    const int i = t < V ? t / N : 0, a = t < V ? t % N : 0;
    const uint64_t ci = bc(st.vcode, i);
    double u = 0.0;
    if (win) direct_cost(L, C, I, ci, N, &u);  // wave-uniform branch
    const double yv = win && t < V ? L.y : 0.0;
    const double cum = vehicle_prefix(yv, N);
    if (t < kMaxM * N) {
        const int i3 = t / N, a3 = t % N;
        const size_t veh = (size_t)b * kMaxM + i3;
        const bool used = t < V;
        const hvp_system& Sv = systems[I.vsys[used ? i : 0]];
        const double p0 = used ? I.x0[2 * i] : 0.0, v0 = used ? I.x0[2 * i + 1] : 0.0;
        if (x_out) {
            double* xo = x_out + veh * 2 * (N + 1);
            if (a3 == 0) {
                xo[0] = p0;
                xo[N + 1] = v0;
            }
            // no solution: the constant-velocity trajectory with u = 0 (as hvp_cent_solve_batch)
            xo[a3 + 1] = !used ? 0.0 : (win ? p0 + Sv.ts * v0 + Sv.ts * cum : p0 + Sv.ts * v0 * (a + 1));
            xo[N + 1 + a3 + 1] = !used ? 0.0 : (win ? yv : v0);
        }
        u_out[veh * N + a3] = used && win ? u : 0.0;
        const int r = hvp::code_region(ci, a);
        if (region_out) region_out[veh * N + a3] = (int8_t)(used && win ? r : -1);
        if (gear_out) gear_out[veh * N + a3] = (int8_t)(used && win ? Sv.gear[r] : 0);
    }
    if (t == 0) {
        cost_out[b] = win ? res.cost : 1e300;
        status_out[b] = res.status;
        if (nodes_out) nodes_out[b] = res.nodes;
        if (iters_out) iters_out[b] = res.iters;
        atomicAdd(&counter[0], (unsigned long long)res.nodes);
        atomicAdd(&counter[1], (unsigned long long)res.iters);
    }
}

// ------------------------------------------------------------------ evaluation of fixed guesses
// One thread per instance.  Regions and gears are resolved as k_evaluate (hvp_lane.h) resolves
// them: the mode with the step's gear label whose closed velocity band holds v_k (tolerance 1e-9
// relative; at a shared band edge the PWA dynamics coincide); without gear guesses the band alone.
__global__ __launch_bounds__(64) void k_event_evaluate(int B, int N, const hvp_event_desc* __restrict__ desc,
                                                       const hvp_system* __restrict__ systems,
                                                       const int32_t* __restrict__ sys,
                                                       const double* __restrict__ params, hvp::Consts C,
                                                       const double* __restrict__ xg, const double* __restrict__ ug,
                                                       const int8_t* __restrict__ gg, double* __restrict__ cost_out,
                                                       int32_t* __restrict__ status_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const hvp_event_desc d = desc[b];
    const int m = d.m, K = N + 1;
    const double* prm = params + (size_t)b * ev_stride(N);
    const double* xf2 = prm + 6;
    const double* xb2 = prm + 6 + 2 * K;
    const double* xl = prm + 6 + 4 * K;
    const double Qpv2 = 2.0 * C.Qpv;
    auto quad = [&](double ep, double ev) { return C.Qpp * ep * ep + Qpv2 * ep * ev + C.Qvv * ev * ev; };
    double p[kMaxM], v[kMaxM], up[kMaxM];
    bool ok = true;
    double J = 0.0;
    for (int i = 0; i < m; ++i) {
        const double* xi = xg + ((size_t)b * kMaxM + i) * 2 * K;
        p[i] = xi[0];
        v[i] = xi[K];
        up[i] = 0.0;
    }
    for (int k = 0; k <= N; ++k) {
        // state terms of step k (cost of LocalMpc, :146-210, :228-236 with the slacks at max(0, .))
        for (int i = 0; i < m; ++i) {
            if (i == d.leader) J += quad(p[i] - xl[k], v[i] - xl[K + k]);
            if (i >= 1) {
                J += quad(p[i] + C.t0 * v[i] + C.d0 - p[i - 1], v[i] - v[i - 1]);
                J += C.w * fmax(0.0, p[i] - p[i - 1] + C.d_safe);
            } else if (d.has_f2) {
                J += quad(p[i] + C.t0 * v[i] + C.d0 - xf2[k], v[i] - xf2[K + k]);
                J += C.w * fmax(0.0, p[i] - xf2[k] + C.d_safe);
            }
            if (i == m - 1 && d.has_b2) {
                const double pb = xb2[k], vb = xb2[K + k];
                J += quad(pb + C.t0 * vb + C.d0 - p[i], vb - v[i]);
                J += C.w * fmax(0.0, pb - p[i] + C.d_safe);
            }
        }
        if (k == N) break;
        for (int i = 0; i < m; ++i) {
            const hvp_system& S = systems[sys[(size_t)b * kMaxM + i]];
            const double u = ug[((size_t)b * kMaxM + i) * N + k];
            const int g = gg ? gg[((size_t)b * kMaxM + i) * N + k] : 0;
            int r = -1;
            const double tol = 1e-9 * (1.0 + fabs(v[i]));
            for (int q = 0; q < S.n_regions && r < 0; ++q)
                if ((!gg || S.gear[q] == g) && v[i] >= S.vlo[q] - tol && v[i] <= S.vhi[q] + tol) r = q;
            if (r < 0) {
                ok = false;
                r = 0;
            }
            const double vn = S.a[r] * v[i] + S.b[r] * u + S.c[r];
            const double tolu = 1e-9 * (1.0 + fabs(u));
            if (u < S.umin - tolu || u > S.umax + tolu) ok = false;
            const double dv = vn - v[i], tola = 1e-9 * (1.0 + fabs(dv));
            if (dv < C.dec[k] - tola || dv > C.acc[k] + tola) ok = false;
            p[i] = p[i] + S.ts * v[i];
            v[i] = vn;
            const double tolv = 1e-9 * (1.0 + fabs(v[i])), tolp = 1e-9 * (1.0 + fabs(p[i]));
            if (v[i] < S.vmin - tolv || v[i] > S.vmax + tolv || p[i] < S.pmin - tolp || p[i] > S.pmax + tolp) ok = false;
            if (k + 1 < N) {  // the guess's own states k = 1..N-1 are fixed: the rollout must meet them
                const double* xi = xg + ((size_t)b * kMaxM + i) * 2 * K;
                const double gp = xi[k + 1], gv = xi[K + k + 1];
                if (!(fabs(gp - p[i]) <= 1e-6 * (1.0 + fabs(gp)) && fabs(gv - v[i]) <= 1e-6 * (1.0 + fabs(gv)))) ok = false;
            }
            J += C.Qu * u * u;
            if (k >= 1) J += C.Qdu * (u - up[i]) * (u - up[i]);
            up[i] = u;
        }
    }
    if (!(J < 1e300)) ok = false;  // NaN / inf inputs
    cost_out[b] = ok ? J : 1e300;
    status_out[b] = ok ? HVP_OPTIMAL : HVP_INFEASIBLE;
}

// ------------------------------------------------------------------ coordinator stages
__device__ inline int ev_lo(int i) { return i >= 1 ? i - 1 : 0; }
__device__ inline int ev_m(int i, int n) { return (i + 1 < n ? i + 1 : n - 1) - ev_lo(i) + 1; }

__global__ __launch_bounds__(256) void k_event_gather(int P, int n, int N, int leader, const double* __restrict__ x,
                                                      const int32_t* __restrict__ vsys, const double* __restrict__ xg,
                                                      const double* __restrict__ ug, const int8_t* __restrict__ gg,
                                                      const double* __restrict__ leader_x, int32_t* __restrict__ sys,
                                                      double* __restrict__ params, double* __restrict__ x_guess,
                                                      double* __restrict__ u_guess, int8_t* __restrict__ gear_guess) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P * n) return;
    const int p = b / n, i = b % n, K = N + 1;
    const int lo = ev_lo(i), m = ev_m(i, n);
    double* out = params + (size_t)b * ev_stride(N);
    for (int j = 0; j < kMaxM; ++j) {
        const int v = lo + j;
        const bool used = j < m;
        sys[(size_t)b * kMaxM + j] = vsys[(size_t)p * n + (used ? v : lo)];
        out[2 * j] = used ? x[(size_t)p * 2 * n + 2 * v] : 0.0;
        out[2 * j + 1] = used ? x[(size_t)p * 2 * n + 2 * v + 1] : 0.0;
        double* xo = x_guess + ((size_t)b * kMaxM + j) * 2 * K;
        double* uo = u_guess + ((size_t)b * kMaxM + j) * N;
        const double* xs = xg + ((size_t)(used ? v : lo) * P + p) * 2 * K;
        const double* us = ug + ((size_t)(used ? v : lo) * P + p) * N;
        for (int k = 0; k < 2 * K; ++k) xo[k] = used ? xs[k] : 0.0;
        for (int k = 0; k < N; ++k) uo[k] = used ? us[k] : 0.0;
        if (gg && gear_guess) {
            const int8_t* gs = gg + ((size_t)(used ? v : lo) * P + p) * N;
            for (int k = 0; k < N; ++k) gear_guess[((size_t)b * kMaxM + j) * N + k] = used ? gs[k] : (int8_t)0;
        }
    }
    auto block = [&](double* dst, const double* src) {
        for (int k = 0; k < 2 * K; ++k) dst[k] = src ? src[k] : 0.0;
    };
    block(out + 6, i >= 2 ? xg + ((size_t)(i - 2) * P + p) * 2 * K : nullptr);
    block(out + 6 + 2 * K, i + 2 < n ? xg + ((size_t)(i + 2) * P + p) * 2 * K : nullptr);
    const bool lead = i >= leader - 1 && i <= leader + 1;
    block(out + 6 + 4 * K, lead ? leader_x + (size_t)p * 2 * K : nullptr);
}

__global__ __launch_bounds__(64) void k_event_select(int P, int n, int N, double threshold,
                                                     const double* __restrict__ eval_cost,
                                                     const int32_t* __restrict__ eval_status,
                                                     const double* __restrict__ new_cost,
                                                     const int32_t* __restrict__ new_status,
                                                     const double* __restrict__ x_sol, const double* __restrict__ u_sol,
                                                     const int8_t* __restrict__ gear_sol, double* __restrict__ xg,
                                                     double* __restrict__ ug, int8_t* __restrict__ gg,
                                                     int32_t* __restrict__ active, int32_t* __restrict__ winner_out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    if (!active[p]) {
        if (winner_out) winner_out[p] = -1;
        return;
    }
    const double INF = __builtin_inf();
    const int K = N + 1;
    double best = -INF;
    int idx = -1;
    bool feasible = false;
    for (int i = 0; i < n; ++i) {
        const size_t b = (size_t)p * n + i;
        const double ev = eval_status[b] == HVP_OPTIMAL ? eval_cost[b] : INF;
        const double nw = new_status[b] == HVP_OPTIMAL ? new_cost[b] : INF;
        if (nw < INF) feasible = true;
        const double dec = ev - nw;  // inf - inf is NaN: both comparisons fail, as in the reference
        if (dec > best && dec > threshold) {
            best = dec;
            idx = i;
        }
    }
    if (winner_out) winner_out[p] = feasible ? idx : -2;
    if (idx < 0) {
        active[p] = 0;
        return;
    }
    const size_t b = (size_t)p * n + idx;
    const int lo = ev_lo(idx), m = ev_m(idx, n);
    for (int j = 0; j < m; ++j) {
        const double* xs = x_sol + (b * kMaxM + j) * 2 * K;
        const double* us = u_sol + (b * kMaxM + j) * N;
        double* xd = xg + ((size_t)(lo + j) * P + p) * 2 * K;
        double* ud = ug + ((size_t)(lo + j) * P + p) * N;
        for (int k = 0; k < 2 * K; ++k) xd[k] = xs[k];
        for (int k = 0; k < N; ++k) ud[k] = us[k];
        if (gg && gear_sol)
            for (int k = 0; k < N; ++k) gg[((size_t)(lo + j) * P + p) * N + k] = gear_sol[(b * kMaxM + j) * N + k];
    }
}

__global__ __launch_bounds__(256) void k_event_shift(int P, int n, int N, int init, const double* __restrict__ x,
                                                     const int32_t* __restrict__ vsys,
                                                     const hvp_system* __restrict__ systems, double* __restrict__ xg,
                                                     double* __restrict__ ug, int8_t* __restrict__ gg) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;  // q = i P + p: the store's own order
    if (q >= P * n) return;
    const int i = q / P, p = q % P, K = N + 1;
    double* xs = xg + (size_t)q * 2 * K;
    double* us = ug + (size_t)q * N;
    int8_t* gs = gg ? gg + (size_t)q * N : nullptr;
    if (!init) {
        for (int k = 0; k < N; ++k) {
            xs[k] = xs[k + 1];
            xs[K + k] = xs[K + k + 1];
        }
        for (int k = 0; k + 1 < N; ++k) {
            us[k] = us[k + 1];
            if (gs) gs[k] = gs[k + 1];
        }
        return;
    }
    const hvp_system& S = systems[vsys[(size_t)p * n + i]];
    double pp = x[(size_t)p * 2 * n + 2 * i];
    const double vv = x[(size_t)p * 2 * n + 2 * i + 1];
    xs[0] = pp;
    xs[K] = vv;
    for (int k = 0; k < N; ++k) {
        pp = pp + S.ts * vv;
        xs[k + 1] = pp;
        xs[K + k + 1] = vv;
    }
    // the first band that holds v (lower edge widened by 1e-4: find_region's buffer, as k_gadmm_rollout)
    int r = -1;
    for (int c = 0; c < S.n_regions && r < 0; ++c)
        if (vv >= S.vlo[c] - 1e-4 && vv <= S.vhi[c]) r = c;
    if (r < 0) r = vv < S.vlo[0] ? 0 : S.n_regions - 1;
    const double u = ((1.0 - S.a[r]) * vv - S.c[r]) / S.b[r];
    for (int k = 0; k < N; ++k) {
        us[k] = u;
        if (gs) gs[k] = (int8_t)S.gear[r];
    }
}

int check_handle(hvp_handle* h, const char* who) {
    if (!h) return fail(HVP_E_ARG, std::string(who) + ": null handle");
    if (h->prob.formulation != HVP_FORM_CENT)
        return fail(HVP_E_ARG, std::string(who) + ": the handle is not an HVP_FORM_CENT problem");
    if (!h->prob.quadratic_cost)
        return fail(HVP_E_UNSUPPORTED, std::string(who) + ": the event-based controller is quadratic only (min_1_norm handle)");
    return 0;
}

// the batch's descriptors on the device (uploaded only when they differ from the last batch's)
int upload_desc(hvp_handle* h, int B, const hvp_event_desc* desc, hipStream_t st, const hvp_event_desc** dev) {
    static_assert(sizeof(hvp_event_desc) == 4 * sizeof(int32_t), "descriptor layout");
    const size_t words = (size_t)B * 4;
    const int32_t* src = reinterpret_cast<const int32_t*>(desc);
    const bool same = h->event_desc && h->event_desc_host.size() == words &&
                      std::memcmp(h->event_desc_host.data(), src, words * sizeof(int32_t)) == 0;
    if (!same) {
        if ((size_t)B > h->event_desc_cap) {
            HIP_TRY(hipDeviceSynchronize());
            (void)hipFree(h->event_desc);
            h->event_desc = nullptr;
            h->event_desc_cap = 0;
            h->event_desc_host.clear();
            if (hipMalloc(&h->event_desc, words * sizeof(int32_t)) != hipSuccess)
                return fail(HVP_E_NOMEM, "hvp_event: device allocation failed");
            h->event_desc_cap = (size_t)B;
        }
        // stream-ordered after the kernels that read the previous descriptors; the source is the
        // handle's own copy, which outlives the call
        HIP_TRY(hipStreamSynchronize(st));
        h->event_desc_host.assign(src, src + words);
        HIP_TRY(hipMemcpyAsync(h->event_desc, h->event_desc_host.data(), words * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    *dev = reinterpret_cast<const hvp_event_desc*>(h->event_desc);
    return 0;
}

}  // namespace

extern "C" {

int hvp_event_params_stride(int N) { return 6 + 6 * (N + 1); }

int hvp_event_validate(const hvp_problem* problem, int B, const hvp_event_desc* desc) {
    if (!problem) return fail(HVP_E_ARG, "hvp_event: null problem");
    if (problem->formulation != HVP_FORM_CENT) return fail(HVP_E_ARG, "hvp_event: the problem is not HVP_FORM_CENT");
    if (!problem->quadratic_cost)
        return fail(HVP_E_UNSUPPORTED, "hvp_event: the event-based controller is quadratic only (min_1_norm problem)");
    if (B < 0) return fail(HVP_E_ARG, "hvp_event: negative batch");
    if (B > 0 && !desc) return fail(HVP_E_ARG, "hvp_event: null descriptors");
    for (int b = 0; b < B; ++b) {
        const hvp_event_desc& d = desc[b];
        if (d.m < 1 || d.m > kMaxM)
            return fail(HVP_E_ARG, "hvp_event: instance " + std::to_string(b) + ": m = " + std::to_string(d.m) + " outside 1..3");
        if (d.leader < -1 || d.leader >= d.m)
            return fail(HVP_E_ARG, "hvp_event: instance " + std::to_string(b) + ": leader index " + std::to_string(d.leader) +
                                       " outside -1.." + std::to_string(d.m - 1));
        if (d.m * problem->N > hvp::cent::ev::kMaxV)
            return fail(HVP_E_ARG, "hvp_event: instance " + std::to_string(b) + ": m N > " + std::to_string(hvp::cent::ev::kMaxV));
    }
    return 0;
}

int hvp_event_layout(int n, int leader_index, hvp_event_desc* desc_out) {
    if (n < 2 || leader_index < 0 || leader_index >= n || !desc_out) return fail(HVP_E_ARG, "hvp_event_layout: bad argument");
    for (int i = 0; i < n; ++i) {
        const int lo = i >= 1 ? i - 1 : 0, hi = i + 1 < n ? i + 1 : n - 1;
        desc_out[i].m = hi - lo + 1;
        desc_out[i].has_f2 = i >= 2 ? 1 : 0;
        desc_out[i].has_b2 = i + 2 < n ? 1 : 0;
        desc_out[i].leader = (leader_index >= i - 1 && leader_index <= i + 1) ? leader_index - lo : -1;
    }
    return 0;
}

int hvp_event_solve_batch(hvp_handle* h, int B, const hvp_event_desc* desc, const int32_t* sys, const double* params,
                          int max_nodes, double* u_out, double* x_out, int8_t* region_out, int8_t* gear_out,
                          double* cost_out, int32_t* status_out, int32_t* nodes_out, int32_t* iters_out, void* stream) {
    if (int rc = check_handle(h, "hvp_event_solve_batch")) return rc;
    if (int rc = hvp_event_validate(&h->prob, B, desc)) return rc;
    if (B == 0) return 0;
    if (!sys || !params || !u_out || !cost_out || !status_out) return fail(HVP_E_ARG, "hvp_event_solve_batch: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int N = h->prob.N;
    int mmax = 1;
    for (int b = 0; b < B; ++b) mmax = std::max(mmax, (int)desc[b].m);
    const size_t fb = (size_t)B * kMaxM * N * h->nreg_max * sizeof(ce::Child);
    const size_t tb = (size_t)B * ce::kTie * kMaxM * sizeof(uint64_t);
    // the DFS child slices and tie rows of hvp_cent_solve_batch (same handle, same role)
    if (fb > h->cent_frames_bytes || tb > h->cent_ties_bytes) {
        HIP_TRY(hipDeviceSynchronize());
        if (fb > h->cent_frames_bytes) {
            (void)hipFree(h->cent_frames);
            h->cent_frames = nullptr;
            h->cent_frames_bytes = 0;
            if (hipMalloc(reinterpret_cast<void**>(&h->cent_frames), fb) != hipSuccess)
                return fail(HVP_E_NOMEM, "hvp_event_solve_batch: device allocation failed");
            h->cent_frames_bytes = fb;
        }
        if (tb > h->cent_ties_bytes) {
            (void)hipFree(h->cent_ties);
            h->cent_ties = nullptr;
            h->cent_ties_bytes = 0;
            if (hipMalloc(&h->cent_ties, tb) != hipSuccess)
                return fail(HVP_E_NOMEM, "hvp_event_solve_batch: device allocation failed");
            h->cent_ties_bytes = tb;
        }
    }
    if (!h->d_consts) {
        if (hipMalloc(&h->d_consts, sizeof(hvp::Consts)) != hipSuccess)
            return fail(HVP_E_NOMEM, "hvp_event_solve_batch: device allocation failed");
        HIP_TRY(hipMemcpy(h->d_consts, &h->C, sizeof(hvp::Consts), hipMemcpyHostToDevice));
    }
    const hvp_event_desc* ddesc = nullptr;
    if (int rc = upload_desc(h, B, desc, st, &ddesc)) return rc;
    const size_t lds = ce::lds_doubles(mmax * N) * sizeof(double);
    HIP_TRY(hipFuncSetAttribute((const void*)k_event_bnb, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_TRY(hipMemsetAsync(h->g_counter, 0, 8 * sizeof(unsigned long long), st));
    const int exhaustive = h->prob.method == HVP_METHOD_ENUMERATE ? 1 : 0;
    const char* dbg = std::getenv("HVP_CENT_DEBUG");
    const int debug = dbg && dbg[0] ? std::atoi(dbg) : 0;
    const int cap = max_nodes > 0 ? max_nodes : 2000000;
    HIP_TRY(hipEventRecord(h->ev0, st));
    HIP_TRY(hipEventRecord(h->evq0, st));
    hipLaunchKernelGGL(k_event_bnb, dim3(B), dim3(64), lds, st, B, N, ddesc, h->d_sys, sys, params, h->d_consts,
                       h->nreg_max, cap, exhaustive, debug, reinterpret_cast<ce::Child*>(h->cent_frames), h->cent_ties,
                       u_out, x_out, region_out, gear_out, cost_out, status_out, nodes_out, iters_out, h->g_counter);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->evq1, st));
    HIP_TRY(hipEventRecord(h->ev1, st));
    h->last_stream = st;
    h->last_B = B;
    h->last_bnb = false;
    return 0;
}

int hvp_event_evaluate_batch(hvp_handle* h, int B, const hvp_event_desc* desc, const int32_t* sys,
                             const double* params, const double* x_guess, const double* u_guess,
                             const int8_t* gear_guess, double* cost_out, int32_t* status_out, void* stream) {
    if (int rc = check_handle(h, "hvp_event_evaluate_batch")) return rc;
    if (int rc = hvp_event_validate(&h->prob, B, desc)) return rc;
    if (B == 0) return 0;
    if (!sys || !params || !x_guess || !u_guess || !cost_out || !status_out)
        return fail(HVP_E_ARG, "hvp_event_evaluate_batch: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const hvp_event_desc* ddesc = nullptr;
    if (int rc = upload_desc(h, B, desc, st, &ddesc)) return rc;
    hipLaunchKernelGGL(k_event_evaluate, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, B, h->prob.N, ddesc, h->d_sys,
                       sys, params, h->C, x_guess, u_guess, gear_guess, cost_out, status_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int hvp_event_gather(hvp_handle* h, int P, int n, int leader_index, const double* x, const int32_t* vsys,
                     const double* xg, const double* ug, const int8_t* gg, const double* leader_x, int32_t* sys,
                     double* params, double* x_guess, double* u_guess, int8_t* gear_guess, void* stream) {
    if (int rc = check_handle(h, "hvp_event_gather")) return rc;
    if (P < 0 || n < 2 || leader_index < 0 || leader_index >= n) return fail(HVP_E_ARG, "hvp_event_gather: bad layout");
    if (P == 0) return 0;
    if (!x || !vsys || !xg || !ug || !leader_x || !sys || !params || !x_guess || !u_guess)
        return fail(HVP_E_ARG, "hvp_event_gather: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_event_gather, dim3((unsigned)(((size_t)P * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P,
                       n, h->prob.N, leader_index, x, vsys, xg, ug, gg, leader_x, sys, params, x_guess, u_guess, gear_guess);
    HIP_TRY(hipGetLastError());
    return 0;
}

int hvp_event_select(hvp_handle* h, int P, int n, double threshold, const double* eval_cost,
                     const int32_t* eval_status, const double* new_cost, const int32_t* new_status, const double* x_sol,
                     const double* u_sol, const int8_t* gear_sol, double* xg, double* ug, int8_t* gg, int32_t* active,
                     int32_t* winner_out, void* stream) {
    if (int rc = check_handle(h, "hvp_event_select")) return rc;
    if (P < 0 || n < 2) return fail(HVP_E_ARG, "hvp_event_select: bad layout");
    if (P == 0) return 0;
    if (!eval_cost || !eval_status || !new_cost || !new_status || !x_sol || !u_sol || !xg || !ug || !active)
        return fail(HVP_E_ARG, "hvp_event_select: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_event_select, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, (hipStream_t)stream, P, n, h->prob.N,
                       threshold, eval_cost, eval_status, new_cost, new_status, x_sol, u_sol, gear_sol, xg, ug, gg, active,
                       winner_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int hvp_event_shift(hvp_handle* h, int P, int n, int init, const double* x, const int32_t* vsys, double* xg,
                    double* ug, int8_t* gg, void* stream) {
    if (int rc = check_handle(h, "hvp_event_shift")) return rc;
    if (P < 0 || n < 1) return fail(HVP_E_ARG, "hvp_event_shift: bad layout");
    if (P == 0) return 0;
    if (!xg || !ug || (init && (!x || !vsys))) return fail(HVP_E_ARG, "hvp_event_shift: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_event_shift, dim3((unsigned)(((size_t)P * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P,
                       n, h->prob.N, init ? 1 : 0, x, vsys, h->d_sys, xg, ug, gg);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
