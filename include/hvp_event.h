/*
 * hvp_event.h -- extension header of libhvpsolve.so: the event-based controller
 * (fleet_event_based.py: LocalMpc / LocalMpcGear, TrackingEventBasedCoordinator).
 *
 * An extension of ABI 5 in the way of hvp_seq.h: it adds functions and changes nothing of
 * include/hvp.h, so HVP_ABI_VERSION stays.  Every function takes an HVP_FORM_CENT handle with
 * quadratic_cost = 1 (simulate() of the reference never builds the min_1_norm variant; such a
 * handle is refused with HVP_E_UNSUPPORTED).
 *
 * The local problem of agent i is the centralised MIQP (mpcs/cent_mld.py) over the m <= 3
 * vehicles [i-1, i, i+1] clipped to the platoon, plus
 *   - has_f2: the fixed trajectory x_f2 of vehicle i-2 in front of local vehicle 0: the cost
 *     |x_0 - x_f2 - spacing(x_0)|^2_Q and the soft row p_0 <= p_f2 - d_safe + s, k = 0..N
 *     (fleet_event_based.py:176-185, :268-275);
 *   - has_b2: the fixed trajectory x_b2 of vehicle i+2 behind local vehicle m-1: the cost
 *     |x_b2 - x_{m-1} - spacing(x_b2)|^2_Q and the soft row p_b2 <= p_{m-1} - d_safe + s
 *     (:199-210, :284-291);
 *   - leader: the local vehicle that also tracks leader_x (|x - leader_x|^2_Q, :146-165), or -1.
 * m = 1 with both boundaries is the decentralised follower problem of fleet_decent_mld.py.
 *
 * Instance b of a batch reads
 *     desc[b]                       HOST memory (validated before any GPU call, then cached on the
 *                                   device: a step of unchanged descriptors uploads nothing)
 *     sys[b][3]                     system index of the local vehicles (unused entries: any valid index)
 *     params[b][hvp_event_params_stride(N)] = x0[3][2] (p, v per vehicle) | x_f2 (2, N+1) |
 *                                   x_b2 (2, N+1) | leader_x (2, N+1); unused blocks zero
 * and writes u[b][3][N], x[b][3][2][N+1], region / gear [b][3][N] (slots of vehicles >= m: zero,
 * region -1).  All but desc are device pointers; calls are asynchronous on `stream`.
 *
 * One stream per handle: the device copy of the descriptors is the handle's, and a batch with new
 * descriptors overwrites it after synchronising the stream it is given; a kernel of the same
 * handle still running on ANOTHER stream would read it while it changes.  Each solve / evaluate
 * call checks its B descriptors and compares them with the cached ones on the host (O(B)).
 */
#ifndef HVP_EVENT_H
#define HVP_EVENT_H

#include "hvp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hvp_event_desc {
    int32_t m;      /* local vehicles, 1..3 */
    int32_t has_f2; /* the front boundary block x_f2 is used */
    int32_t has_b2; /* the back boundary block x_b2 is used */
    int32_t leader; /* local index (0..m-1) of the vehicle that tracks leader_x, or -1 for none */
} hvp_event_desc;

/* doubles per instance of params: 6 + 6 (N + 1) */
int hvp_event_params_stride(int N);

/* The argument checks of the two batch calls below, on the host alone (no handle, no device):
 * HVP_E_ARG for a NULL pointer, a problem that is not HVP_FORM_CENT, B < 0, m outside 1..3,
 * a leader index >= m (or < -1) and m N > 64; HVP_E_UNSUPPORTED for quadratic_cost = 0. */
int hvp_event_validate(const hvp_problem* problem, int B, const hvp_event_desc* desc);

/* The agents' descriptors of one platoon of n >= 2 vehicles (host): desc_out[i] for agent i with
 * m, has_f2 = (i >= 2), has_b2 = (i <= n-3) and the leader's local index for agents
 * leader_index-1 .. leader_index+1 (fleet_event_based.py:700-723). */
int hvp_event_layout(int n, int leader_index, hvp_event_desc* desc_out);

/* B local MIQPs, one wavefront each (the joint branch and bound of hvp_cent_solve_batch on the
 * wave QP with the boundary terms; single-wave search, V = m N <= 48).  max_nodes <= 0: the
 * default cap.  x_out, region_out, gear_out, nodes_out, iters_out may be NULL.  cost 1e300 and the
 * constant-velocity trajectory when status != HVP_OPTIMAL. */
int hvp_event_solve_batch(hvp_handle* h, int B, const hvp_event_desc* desc, const int32_t* sys, const double* params,
                          int max_nodes, double* u_out, double* x_out, int8_t* region_out, int8_t* gear_out,
                          double* cost_out, int32_t* status_out, int32_t* nodes_out, int32_t* iters_out, void* stream);

/* LocalMpc.eval_cost (fleet_event_based.py:308-327) restated: the local vehicles' PWA dynamics are
 * rolled out from x_guess[:, :, 0] (NOT params' x0) under u_guess [B][3][N] and gear_guess
 * [B][3][N] (NULL: the region is the velocity band alone, the models without gear decisions).
 * Cost = the local objective of the rollout with every hinge at its optimal slack; 1e300 and
 * HVP_INFEASIBLE when the rollout leaves x_guess [B][3][2][N+1] at a state k = 1..N-1 by more than
 * 1e-6 (1 + |x|), when no mode holds v_k, or when a hard row fails (input / state boxes and the
 * acceleration rows of every step, the step to x_N included; tolerance 1e-9 relative as
 * hvp_evaluate_batch). */
int hvp_event_evaluate_batch(hvp_handle* h, int B, const hvp_event_desc* desc, const int32_t* sys,
                             const double* params, const double* x_guess, const double* u_guess,
                             const int8_t* gear_guess, double* cost_out, int32_t* status_out, void* stream);

/* ---- the coordinator's stages for P platoons of n vehicles (device loop; instance b = p n + i).
 * Guess store, vehicle-major: xg [n][P][2][N+1], ug [n][P][N], gg [n][P][N] (int8, may be NULL).
 *
 * gather: one thread per (platoon, agent) writes sys [P n][3], params [P n][stride] (x0 from the
 * measured states x [P][2n], x_f2 / x_b2 = xg[i-2] / xg[i+2], the leader window leader_x
 * [P][2][N+1] for agents leader_index-1..+1) and the evaluation inputs x_guess / u_guess /
 * gear_guess of the local vehicles.  vsys [P][n]: system index per vehicle. */
int hvp_event_gather(hvp_handle* h, int P, int n, int leader_index, const double* x, const int32_t* vsys,
                     const double* xg, const double* ug, const int8_t* gg, const double* leader_x, int32_t* sys,
                     double* params, double* x_guess, double* u_guess, int8_t* gear_guess, void* stream);

/* select: the winner rule per platoon (:517-569).  eval_cost / new_cost [P n] with their statuses
 * (a status != HVP_OPTIMAL counts as inf).  The winner is the first agent with the largest
 * decrease eval - new that strictly exceeds `threshold`; its 2 or 3 solved trajectories
 * (x_sol [P n][3][2][N+1], u_sol, gear_sol) overwrite the guesses.  active [P]: a platoon whose
 * flag is 0 is left alone; the flag is cleared where nobody wins.  winner_out [P] (may be NULL):
 * the winner, -1 none (or inactive), -2 no agent had a feasible solve (the reference raises). */
int hvp_event_select(hvp_handle* h, int P, int n, double threshold, const double* eval_cost,
                     const int32_t* eval_status, const double* new_cost, const int32_t* new_status, const double* x_sol,
                     const double* u_sol, const int8_t* gear_sol, double* xg, double* ug, int8_t* gg, int32_t* active,
                     int32_t* winner_out, void* stream);

/* shift: init == 0: on_timestep_end (:589-603), every guess one sample on, the last column
 * repeated.  init != 0: on_episode_start (:620-635) from the measured states x [P][2n]:
 * constant-velocity states, the input that holds the velocity in the PWA dynamics of the first
 * mode whose band holds it (get_u_for_constant_vel; on the (gear, friction-region) tables, which
 * are gear-major, that is the lowest gear whose band holds v: get_gear_from_velocity) and that
 * mode's gear label. */
int hvp_event_shift(hvp_handle* h, int P, int n, int init, const double* x, const int32_t* vsys, double* xg,
                    double* ug, int8_t* gg, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HVP_EVENT_H */
