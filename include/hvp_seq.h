/*
 * hvp_seq.h -- extension header of libhvpsolve.so: the stage glue of the sequential MLD
 * controller (fleet_seq_mld.py:296-440, TrackingSequentialMldCoordinator).
 *
 * An extension of ABI 5: it adds a function and changes nothing of include/hvp.h, so a caller
 * that only knows hvp.h is not affected and HVP_ABI_VERSION stays.  The local problem of the
 * sequential controller is the HVP_FORM_DECENT one (same parameter block, same role bits); only
 * the source of the neighbour trajectories differs, which is what this function writes.
 */
#ifndef HVP_SEQ_H
#define HVP_SEQ_H

#include "hvp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Parameter blocks and roles of ONE stage of a sequential step: vehicle i of P platoons
 * (device pointers, async on stream).  Per step the stages run in the order leader L, then
 * L-1 .. 0, then L+1 .. n-1 (fleet_seq_mld.py:336-386), each followed by the hvp_solve_batch
 * of its P instances with x_out = xpred + i * P * 2 * (N+1), so that the prediction store
 *     xpred [n][P][2][N+1]   (vehicle-major)
 * holds in slot j the trajectory vehicle j solved last: this step's once stage j has run
 * ("fresh"), the previous step's before ("shifted" when read: column 0 dropped, the last column
 * repeated, the last position then set to old p_N + ts * old v_N).  Neighbour blocks of vehicle i:
 *     i == L : front = shifted of i-1 (i != 0),  back = shifted of i+1 (i != n-1)
 *     i <  L : front = shifted of i-1 (i != 0),  back = fresh of i+1
 *     i >  L : front = fresh of i-1,             back = shifted of i+1 (i != n-1)
 * first != 0 (the first step of an episode, no prediction yet): a "shifted" block is the
 * constant-velocity extrapolation of that neighbour's state in x (on_episode_start, :413-431)
 * and its xpred slot is not read; "fresh" blocks are read from xpred as always.
 *   x [P][2n] the measured states; leader_x [P][2][N+1] the leader window.
 * Writes params [P][hvp_params_stride(N)] (x0 | x_front | x_back | leader_x; blocks the role
 * does not use are zero) and roles [P] of the instances at batch positions 0..P-1, as
 * hvp_decent_params_batch writes them for vehicle i.  HVP_FORM_DECENT handles (their N and ts). */
int hvp_seq_stage_params(hvp_handle* h, int P, int n, int i, const double* x, const double* xpred,
                         const double* leader_x, int leader_index, int real_vehicle_as_reference, int first,
                         double* params, int32_t* roles, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HVP_SEQ_H */
