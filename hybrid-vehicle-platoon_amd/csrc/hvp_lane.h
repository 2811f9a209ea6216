// hvp_lane.h -- kernel templates of the decentralised / ADMM / switching-ADMM lane paths and
// their launchers (internal).  hvp_lane_inst.hip instantiates the launchers of ONE horizon N
// per object file (the Makefile builds N = 2..16 in parallel); hvp_kernels.hip holds the C ABI
// and dispatches to them.  Kernel design: see the comments below and DESIGN.md section 4.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#ifndef HVP_HD
#define HVP_HD __host__ __device__
#endif
#include "hvp.h"
#include "hvp_internal.h"
#include "hvp_admm.h"
#include "hvp_bnb.h"
#include "hvp_lp.h"
#include "hvp_coop.h"
#include "hvp_gi.h"
#include "hvp_ipm.h"
#include "hvp_l1.h"

namespace hvp_k {

using hvp_detail::fail;
using hvp_detail::Workspace;

constexpr int kBlock = 256;
// HVP_METHOD_AUTO: exhaustive enumeration up to this horizon, branch and bound beyond
constexpr int kAutoEnumMaxN = 0;  // measured: B&B beats enumeration already at N = 5 (profiles/)
// min_1_norm: branch and bound at every horizon too -- C2 (16,384 platoons): 78.0k platoon-steps/s
// against 56.6k by enumeration (2.71M vs 5.0M LPs per step, profiles/r03e_*)
constexpr int kAutoEnumMaxNL1 = 0;
// active-set iteration cap (then the interior-point fallback takes the candidate)
template <int N>
constexpr int kGiMaxIter = 8 * hvp::GiConstraintSet<N>::NC;

// ------------------------------------------------------------------ K_enum
template <int N>
__global__ __launch_bounds__(kBlock) void k_enum(int B, const hvp_system* __restrict__ systems,
                                                 const int32_t* __restrict__ sys, const int32_t* __restrict__ role,
                                                 const double* __restrict__ params, hvp::Consts C, Workspace ws) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const hvp_system& S = systems[sys[i]];
    const double* prm = params + (size_t)i * (2 + 6 * (N + 1));
    const double p0 = prm[0], v0 = prm[1];
    const double P1 = p0 + S.ts * v0;
    // sigma-independent constant row: p_1 = p_0 + ts v_0 inside the position box
    const bool ok = P1 >= S.pmin - 1e-9 * (1.0 + fabs(S.pmin)) && P1 <= S.pmax + 1e-9 * (1.0 + fabs(S.pmax));
    int cnt = 0;
    if (ok) cnt = hvp::enumerate_sequences(S, C, v0, [](uint32_t, int) {});
    ws.inst_cnt[i] = cnt;
    ws.inst_flag[i] = ok ? 0 : 1;
    int off = -1;
    if (cnt > 0) {
        const unsigned long long o = atomicAdd(&ws.counter[0], (unsigned long long)cnt);
        if ((long long)o + cnt <= ws.cap) {
            off = (int)o;
        } else {
            // overflow: the part of the reserved range below the capacity is still swept by
            // K_qp / K_cost (they run over min(reserved, cap)): mark those slots dead
            for (long long t = (long long)o; t < ws.cap && t < (long long)o + cnt; ++t) ws.task_inst[t] = -1;
        }
    }
    ws.inst_off[i] = off;
    if (off < 0) return;
    hvp::enumerate_sequences(S, C, v0, [&](uint32_t code, int j) {
        ws.task_inst[off + j] = i;
        ws.task_code[off + j] = code;
    });
    (void)role;
}

// ------------------------------------------------------------------ K_qp
// Per-lane constant rows in LDS: field f, step j of lane l at s_rows[(f * N + j) * kBlock + l]
// (consecutive lanes -> consecutive 8-byte words: conflict-free ds_read_b64).  refresh() makes
// the lane offset opaque at the start of every IPM sweep so the compiler re-reads the rows from
// LDS instead of hoisting them into VGPRs for the whole solve.
extern __shared__ double s_rows[];

template <int N, int BS = kBlock>
struct LdsMem {
    unsigned lane;
    __device__ double get(int f, int j) const { return s_rows[(f * N + j) * BS + lane]; }
    __device__ void set(int f, int j, double x) { s_rows[(f * N + j) * BS + lane] = x; }
    __device__ void refresh() { asm volatile("" : "+v"(lane)); }
};

// K_qp: every candidate by the Goldfarb-Idnani active-set method (hvp_gi.h).  A lane whose
// result fails the KKT verification (or hits the iteration cap) is queued on the fallback list.
template <int N>
__global__ __launch_bounds__(kBlock) void k_qp_gi(const hvp_system* __restrict__ systems,
                                                  const int32_t* __restrict__ sys, const int32_t* __restrict__ role,
                                                  const double* __restrict__ params, hvp::Consts C, Workspace ws) {
    const unsigned long long reserved = ws.counter[0];
    const long long total = (long long)(reserved < (unsigned long long)ws.cap ? reserved : ws.cap);
    unsigned long long iter_sum = 0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const int inst = ws.task_inst[t];
        if (inst < 0) continue;  // dead slot of an overflowed instance
        const uint32_t code = ws.task_code[t];
        const hvp_system& S = systems[sys[inst]];
        const int rl = role[inst];
        const double* prm = params + (size_t)inst * (2 + 6 * (N + 1));
        hvp::LaneQp<N, LdsMem<N>> q;
        q.mem.lane = threadIdx.x;
        hvp::setup_lane<N>(q, S, C, rl, prm, code);
        int iters = 0;
        int status = hvp::solve_gi<N>(q, C, kGiMaxIter<N>, iters);
        if (status != hvp::GI_OK) {
            const unsigned long long r = atomicAdd(&ws.counter[2], 1ull);
            ws.redo[r] = (int32_t)t;
            status = 4;  // pending: the fallback kernel overwrites it
        }
        ws.task_stat[t] = status | (iters << 8);
#pragma unroll
        for (int k = 0; k < N; ++k) ws.task_y[t * N + k] = q.y[k];
        iter_sum += (unsigned long long)iters;
    }
    // one atomic per wave for the iteration statistics
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) iter_sum += __shfl_down(iter_sum, off, 64);
    if ((threadIdx.x & 63) == 0 && iter_sum) atomicAdd(&ws.counter[1], iter_sum);
}

// K_qp_ipm: the fallback list only (normally empty: the launch reads a zero count and exits),
// full row set by the Mehrotra interior-point method (hvp_ipm.h).
template <int N>
__global__ __launch_bounds__(kBlock) void k_qp_ipm(const hvp_system* __restrict__ systems,
                                                   const int32_t* __restrict__ sys, const int32_t* __restrict__ role,
                                                   const double* __restrict__ params, hvp::Consts C, Workspace ws) {
    const unsigned long long reserved = ws.counter[2];
    const long long total = (long long)(reserved < (unsigned long long)ws.cap ? reserved : ws.cap);
    unsigned long long iter_sum = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long t = (long long)ws.redo[i];
        const int inst = ws.task_inst[t];
        const uint32_t code = ws.task_code[t];
        const hvp_system& S = systems[sys[inst]];
        const int rl = role[inst];
        const double* prm = params + (size_t)inst * (2 + 6 * (N + 1));
        hvp::LaneQp<N, LdsMem<N>> q;
        q.mem.lane = threadIdx.x;
        hvp::setup_lane<N>(q, S, C, rl, prm, code);
        const hvp::QpOut o = hvp::Solver<N, true, LdsMem<N>>::solve(q, C);
        ws.task_stat[t] = o.status | ((o.iters + (ws.task_stat[t] >> 8)) << 8);
#pragma unroll
        for (int k = 0; k < N; ++k) ws.task_y[t * N + k] = q.y[k];
        iter_sum += (unsigned long long)o.iters;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) iter_sum += __shfl_down(iter_sum, off, 64);
    if ((threadIdx.x & 63) == 0 && iter_sum) atomicAdd(&ws.counter[1], iter_sum);
}

// K_qp_l1: min_1_norm problems (hvp_l1.h), every candidate's fixed-sequence LP by the
// interior-point method, ONE LP PER WAVEFRONT: lane l owns hard row l (8N - 2 <= 62 rows) and
// pairs l, l + 64 (10N <= 80) in registers; the N x N Newton system is the wave sum of the
// lanes' row contributions (an LDS all-reduce per wave, bit-identical in every lane, so the control
// flow stays wave-uniform), factorised redundantly per lane and reused by the corrector (only its
// right-hand side is reduced again).  No private segment: the per-lane form of the same method
// (hvp_l1.h l1_solve, the host build's) keeps ~10 KB per lane there and is bound by that traffic.
__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ inline double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ inline double wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}

// LDS all-reduce of M doubles per lane within one wavefront (no block barrier: the waves of a
// block run different LPs).  red: this wave's buffer of kRedRows<M> x 65 doubles (row j = value j
// of the 64 lanes, padded to 65 so that lane j's reads of row j fall in distinct banks, slot 64 =
// the sum).  Lane j < M sums row j in lane order (M <= 32: lanes j and j + 32 a half each); every
// lane reads the M sums back (broadcast reads), so all lanes hold bit-identical results.  M > 64
// (the Newton systems of N >= 9) goes through the buffer in chunks of 32 values.
__device__ inline void lds_wave_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}
template <int M>
constexpr int kRedRows = M <= 64 ? M : 32;

// rows [0, m) of the buffer: two lanes per value (j and j + 32, 32 entries each), halves combined
// across the wave halves (a + b == b + a: both lanes hold the same sum)
__device__ inline void lds_rows_sum32(double* red, int lane, int m) {
    const int j = lane & 31;
    double acc = 0.0;
    if (j < m) {
        const double* row = red + j * 65 + (lane >> 5) * 32;
#pragma unroll 16
        for (int i = 0; i < 32; ++i) acc += row[i];
    }
    acc += __shfl_xor(acc, 32, 64);
    if (lane < m) red[lane * 65 + 64] = acc;
}

// M values in chunks of 32 rows (lds_rows_sum32 for every chunk, whatever M)
template <int M>
__device__ inline void wave_sum_lds32(double* v, double* red, int lane) {
#pragma unroll
    for (int c0 = 0; c0 < M; c0 += 32) {
        constexpr int CH = 32;
#pragma unroll
        for (int j = 0; j < CH; ++j)
            if (c0 + j < M) red[j * 65 + lane] = v[c0 + j];
        lds_wave_sync();
        lds_rows_sum32(red, lane, M - c0 < CH ? M - c0 : CH);
        lds_wave_sync();
#pragma unroll
        for (int j = 0; j < CH; ++j)
            if (c0 + j < M) v[c0 + j] = red[j * 65 + 64];
        lds_wave_sync();
    }
}

template <int M>
__device__ inline void wave_sum_lds(double* v, double* red, int lane) {
    if constexpr (M <= 64) {
#pragma unroll
        for (int j = 0; j < M; ++j) red[j * 65 + lane] = v[j];
        lds_wave_sync();
        if constexpr (M <= 32) {
            lds_rows_sum32(red, lane, M);
        } else {
            if (lane < M) {
                double acc = 0.0;
                const double* row = red + lane * 65;
#pragma unroll 16
                for (int i = 0; i < 64; ++i) acc += row[i];
                red[lane * 65 + 64] = acc;
            }
        }
        lds_wave_sync();
#pragma unroll
        for (int j = 0; j < M; ++j) v[j] = red[j * 65 + 64];
        lds_wave_sync();  // the buffer is reused by the next reduction
    } else {
        wave_sum_lds32<M>(v, red, lane);
    }
}

// A lane's row vectors in LDS: component a of slot q at base[(q N + a) 64] (the wave's 64 lanes
// interleaved, so a wave's read of one component is one conflict-free 512-byte row).  The vectors
// are constant through an LP's iterations; held in registers they pushed the wave solver to ~2 KB
// of scratch per lane at N = 10 (spilled state reloaded every iteration).
struct LdsRow {
    double* p;
    __device__ double& operator[](int a) const { return p[a * 64]; }
};
template <int N>
struct LdsRows {
    double* base;
    __device__ LdsRow operator[](int q) const { return LdsRow{base + q * N * 64}; }
};
}  // namespace hvp_k
namespace hvp {
template <int N>
__device__ inline double l1_dot(const hvp_k::LdsRow& g, const double* y) {  // l1_dot's order
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) s += g[i] * y[i];
    return s;
}
}  // namespace hvp
namespace hvp_k {

// One LP per wavefront: lane l owns hard rows l, l + 64 (8N - 2 <= 126) and pairs l, l + 64,
// l + 128 (10N <= 160): their scalars in registers, their row vectors in LDS (LdsRows; the wave's
// area of kL1GSlots x N x 64 doubles after its reduction rows, kL1LdsAll).
template <int N>
struct L1Wave {
    static constexpr int NHS = (8 * N - 2 + 63) / 64;  // hard-row slots per lane
    static constexpr int NPS = (10 * N + 63) / 64;     // pair slots per lane
    static constexpr int NT = N * (N + 1) / 2;
    bool hon[NHS];
    LdsRows<N> hg;
    double hh[NHS], hs[NHS], hl[NHS], hds[NHS], hdl[NHS];
    bool pon[NPS];
    LdsRows<N> pg;
    double pe0[NPS], pw[NPS], pal[NPS], pt[NPS], ps1[NPS], ps2[NPS], pl1[NPS], pl2[NPS];
    double pds1[NPS], pdl1[NPS], pds2[NPS], pdl2[NPS], pdt[NPS];
    bool rel = false;  // primal residuals relative to the row's constant, |rp| / (1 + |h|) (L1AdmmWave)

    __device__ void clear() {
#pragma unroll
        for (int q = 0; q < NHS; ++q) {
            hon[q] = false;
            hh[q] = 0.0;
            hs[q] = 1.0;
            hl[q] = hds[q] = hdl[q] = 0.0;
#pragma unroll
            for (int a = 0; a < N; ++a) hg[q][a] = 0.0;
        }
#pragma unroll
        for (int q = 0; q < NPS; ++q) {
            pon[q] = false;
            pe0[q] = pw[q] = pal[q] = pt[q] = pl1[q] = pl2[q] = 0.0;
            ps1[q] = ps2[q] = 1.0;
            pds1[q] = pdl1[q] = pds2[q] = pdl2[q] = pdt[q] = 0.0;
#pragma unroll
            for (int a = 0; a < N; ++a) pg[q][a] = 0.0;
        }
    }

    // the rows of the LP of (prm, code) relaxed after K steps (hvp_l1.h l1_rows) that map to this
    // lane (row vectors into gbuf, the wave's LDS row area); false when the constant p_1 row is violated
    __device__ bool load(const hvp_system& S, const hvp::Consts& C, int rl, const double* prm, uint64_t code, int K,
                         double rlo, double rhi, int lane, int& mh, int& mp, double* gbuf, int xl_blk = 4) {
        hg.base = gbuf + lane;
        pg.base = gbuf + NHS * N * 64 + lane;
        clear();
        return hvp::l1_rows<N>(
            S, C, rl, prm, code, K, rlo, rhi, mh, mp,
            [&](int i, const double* g, double sgn, double h) {
#pragma unroll
                for (int q = 0; q < NHS; ++q) {
                    if (i == lane + 64 * q) {
                        hon[q] = true;
#pragma unroll
                        for (int a = 0; a < N; ++a) hg[q][a] = sgn * g[a];
                        hh[q] = h;
                    }
                }
            },
            [&](int j, const double* g, double e0, double w, double alpha) {
#pragma unroll
                for (int q = 0; q < NPS; ++q) {
                    if (j == lane + 64 * q) {
                        pon[q] = true;
#pragma unroll
                        for (int a = 0; a < N; ++a) pg[q][a] = g[a];
                        pe0[q] = e0;
                        pw[q] = w;
                        pal[q] = alpha;
                    }
                }
            },
            xl_blk);
    }

    // this lane's share of: residuals (gap, obj, rd_y, max |rp|, max |rd_t|) and the Newton right-hand
    // side (targets rc = s l [+ ds dl - sigmu when corr]); the matrix is kpart's
    __device__ void contrib(const double* y, bool corr, double sigmu, double* rhs, double& gap, double& obj,
                            double* rdy, double& rpm, double& rdm) const {
#pragma unroll
        for (int q = 0; q < NHS; ++q) {
            if (!hon[q]) continue;
            const double gy = hvp::l1_dot<N>(hg[q], y);
            const double rp = gy + hs[q] - hh[q];
            const double rc = hs[q] * hl[q] + (corr ? hds[q] * hdl[q] : 0.0) - sigmu;
            const double rho = (hl[q] * rp - rc) / hs[q], coef = -(hl[q] + rho);
            gap += hs[q] * hl[q];
            rpm = fmax(rpm, rel ? fabs(rp) / (1.0 + fabs(hh[q])) : fabs(rp));
#pragma unroll
            for (int a = 0; a < N; ++a) {
                rdy[a] += hl[q] * hg[q][a];
                rhs[a] += coef * hg[q][a];
            }
        }
#pragma unroll
        for (int q = 0; q < NPS; ++q) {
            if (!pon[q]) continue;
            const double al = pal[q], gy = hvp::l1_dot<N>(pg[q], y);
            const double rp1 = gy - pt[q] + ps1[q] + pe0[q];
            const double rp2 = -al * gy - pt[q] + ps2[q] - al * pe0[q];
            const double D1 = pl1[q] / ps1[q], D2 = pl2[q] / ps2[q];
            const double rc1 = ps1[q] * pl1[q] + (corr ? pds1[q] * pdl1[q] : 0.0) - sigmu;
            const double rc2 = ps2[q] * pl2[q] + (corr ? pds2[q] * pdl2[q] : 0.0) - sigmu;
            const double rho1 = (pl1[q] * rp1 - rc1) / ps1[q], rho2 = (pl2[q] * rp2 - rc2) / ps2[q];
            const double rdt = pw[q] - pl1[q] - pl2[q];
            const double rhst = -rdt + rho1 + rho2;
            const double mt = D1 + D2, m = al * D2 - D1;
            const double coef = -(pl1[q] - al * pl2[q]) - (rho1 - al * rho2) - m * rhst / mt;
            gap += ps1[q] * pl1[q] + ps2[q] * pl2[q];
            obj += pw[q] * pt[q];
            rpm = fmax(rpm, fmax(fabs(rp1), fabs(rp2)) / (rel ? 1.0 + fabs(pe0[q]) : 1.0));
            rdm = fmax(rdm, fabs(rdt));
#pragma unroll
            for (int a = 0; a < N; ++a) {
                rdy[a] += (pl1[q] - al * pl2[q]) * pg[q][a];
                rhs[a] += coef * pg[q][a];
            }
        }
    }

    // The Newton matrix K = sum_r D_r g_r g_r' is assembled in chunks of its packed triangle
    // (hvp::tri order): weights() takes contrib's per-row D (hard rows) / ce (pairs) of the current
    // iterate, kpart<E0, CH> adds this lane's rows to entries [E0, E0 + CH).  With contrib's
    // expressions and per-entry order, so the matrix is the one a single pass over K built; but only
    // CH accumulators are live at a time instead of the whole triangle (l1_newton_factor).
    struct Wts {
        double dh[NHS], dp[NPS];
    };
    __device__ void weights(const double* /*y*/, Wts& w) const {
#pragma unroll
        for (int q = 0; q < NHS; ++q) w.dh[q] = hl[q] / hs[q];
#pragma unroll
        for (int q = 0; q < NPS; ++q) {
            const double al = pal[q], D1 = pl1[q] / ps1[q], D2 = pl2[q] / ps2[q];
            const double mt = D1 + D2;
            w.dp[q] = D1 * D2 * (1.0 + al) * (1.0 + al) / mt;
        }
    }
    template <int E0, int CH>
    __device__ void kpart(const Wts& w, double* kc) const {
#pragma unroll
        for (int q = 0; q < NHS; ++q) {
            if (!hon[q]) continue;
#pragma unroll
            for (int a = 0; a < N; ++a) {
#pragma unroll
                for (int c = 0; c <= a; ++c) {
                    const int e = hvp::tri(a, c) - E0;
                    if (e >= 0 && e < CH) kc[e] += w.dh[q] * hg[q][a] * hg[q][c];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NPS; ++q) {
            if (!pon[q]) continue;
#pragma unroll
            for (int a = 0; a < N; ++a) {
#pragma unroll
                for (int c = 0; c <= a; ++c) {
                    const int e = hvp::tri(a, c) - E0;
                    if (e >= 0 && e < CH) kc[e] += w.dp[q] * pg[q][a] * pg[q][c];
                }
            }
        }
    }

    // directions of this lane's rows for dy (same targets as contrib), written over the stored
    // ones (each row reads its predictor ds dl before writing); returns the local step limits
    __device__ void directions(const double* y, const double* dy, bool corr, double sigmu, double& ap, double& ad) {
#pragma unroll
        for (int q = 0; q < NHS; ++q) {
            if (!hon[q]) continue;
            const double gy = hvp::l1_dot<N>(hg[q], y), gd = hvp::l1_dot<N>(hg[q], dy);
            const double rp = gy + hs[q] - hh[q], D = hl[q] / hs[q];
            const double rc = hs[q] * hl[q] + (corr ? hds[q] * hdl[q] : 0.0) - sigmu;
            const double rho = (hl[q] * rp - rc) / hs[q];
            hds[q] = -rp - gd;
            hdl[q] = D * gd + rho;
            hvp::l1_ratio(ap, hs[q], hds[q]);
            hvp::l1_ratio(ad, hl[q], hdl[q]);
        }
#pragma unroll
        for (int q = 0; q < NPS; ++q) {
            if (!pon[q]) continue;
            const double al = pal[q], gy = hvp::l1_dot<N>(pg[q], y), gd = hvp::l1_dot<N>(pg[q], dy);
            const double rp1 = gy - pt[q] + ps1[q] + pe0[q];
            const double rp2 = -al * gy - pt[q] + ps2[q] - al * pe0[q];
            const double D1 = pl1[q] / ps1[q], D2 = pl2[q] / ps2[q];
            const double rc1 = ps1[q] * pl1[q] + (corr ? pds1[q] * pdl1[q] : 0.0) - sigmu;
            const double rc2 = ps2[q] * pl2[q] + (corr ? pds2[q] * pdl2[q] : 0.0) - sigmu;
            const double rho1 = (pl1[q] * rp1 - rc1) / ps1[q], rho2 = (pl2[q] * rp2 - rc2) / ps2[q];
            const double rdt = pw[q] - pl1[q] - pl2[q];
            const double rhst = -rdt + rho1 + rho2;
            const double mt = D1 + D2, m = al * D2 - D1;
            pdt[q] = (rhst - m * gd) / mt;
            const double a1 = gd - pdt[q], a2 = -al * gd - pdt[q];
            pds1[q] = -rp1 - a1;
            pds2[q] = -rp2 - a2;
            // as hvp_l1.h l1_direction: the larger-scaled side's multiplier from the t row
            const bool big1 = D1 >= D2;
            const double dls = big1 ? D2 * a2 + rho2 : D1 * a1 + rho1;
            pdl1[q] = big1 ? rdt - dls : dls;
            pdl2[q] = big1 ? dls : rdt - dls;
            hvp::l1_ratio(ap, ps1[q], pds1[q]);
            hvp::l1_ratio(ap, ps2[q], pds2[q]);
            hvp::l1_ratio(ad, pl1[q], pdl1[q]);
            hvp::l1_ratio(ad, pl2[q], pdl2[q]);
        }
    }
};

// Mehrotra predictor-corrector (the algorithm of hvp_l1.h l1_solve), wave-cooperative.
// Returns L1_OK, L1_INFEASIBLE (Farkas certificate of the hard rows over the velocity box
// [ylo, yhi], hvp_l1.h l1_farkas) or L1_FAIL; y (uniform) holds the iterate.
template <int N>
constexpr int kL1Res = 2 + 2 * N;  // gap, obj, rd_y, rhs: one LDS all-reduce per iteration
template <int N>
constexpr int kL1NT = N * (N + 1) / 2;  // the Newton matrix's packed triangle
// A wave's LDS buffer: kL1Rows reduction rows of 65 doubles (the residuals and the K chunks in
// rows of at most 32 values, l1_wave_cert's N + 2), then the K area of kL1NT doubles that holds the
// assembled matrix and then its factor (the chol_solve calls of an iteration read it from there).
constexpr int l1_rows_of(int n) {
    const int nt = n * (n + 1) / 2 < 32 ? n * (n + 1) / 2 : 32, res = 2 + 2 * n < 32 ? 2 + 2 * n : 32;
    const int r = nt > res ? nt : res;
    return r > n + 2 ? r : n + 2;
}
template <int N>
constexpr int kL1Rows = l1_rows_of(N);
template <int N>
constexpr int kL1KOff = kL1Rows<N> * 65;
template <int N>
constexpr int kL1Lds = kL1KOff<N> + kL1NT<N>;
template <int N>
constexpr int kL1GSlots = L1Wave<N>::NHS + L1Wave<N>::NPS;
template <int N, bool ADMM = false>
constexpr int kL1LdsAll = kL1Lds<N> + (kL1GSlots<N> + (ADMM ? 3 : 0)) * N * 64;  // doubles per wave: + the row vectors

// Newton matrix of the current iterate (R: L1Wave or L1AdmmWave; all lanes call it) into the K
// area, factored there (cholesky_l1): the lanes' shares of each chunk of 32 entries are summed
// through the reduction rows (lds_rows_sum32, as wave_sum_lds32 sums them), every lane loads the
// matrix, factors it redundantly, and lane 0 stores the factor.  Only one chunk of accumulators and
// then the triangle are live in registers, never both next to the row state (the one-pass form
// held 2 + 2N + N(N+1)/2 partial sums and spilled ~3 KB per lane at N = 10).
template <int N, int E0, class R>
__device__ inline void l1_k_chunks(const R& rows, const typename R::Wts& w, double* red, int lane) {
    if constexpr (E0 < kL1NT<N>) {
        constexpr int CH = kL1NT<N> - E0 < 32 ? kL1NT<N> - E0 : 32;
        double kc[CH];
#pragma unroll
        for (int e = 0; e < CH; ++e) kc[e] = 0.0;
        rows.template kpart<E0, CH>(w, kc);
#pragma unroll
        for (int e = 0; e < CH; ++e) red[e * 65 + lane] = kc[e];
        lds_wave_sync();
        lds_rows_sum32(red, lane, CH);
        lds_wave_sync();
        if (lane < CH) red[kL1KOff<N> + E0 + lane] = red[lane * 65 + 64];
        lds_wave_sync();
        l1_k_chunks<N, E0 + 32>(rows, w, red, lane);
    }
}
template <int N, class R>
__device__ inline const double* l1_newton_factor(const R& rows, const double* y, double* red, int lane) {
    typename R::Wts w;
    rows.weights(y, w);
    l1_k_chunks<N, 0>(rows, w, red, lane);
    double* KA = red + kL1KOff<N>;
    double K[kL1NT<N>];
#pragma unroll
    for (int i = 0; i < kL1NT<N>; ++i) K[i] = KA[i];
    hvp::cholesky_l1<N>(K);
    lds_wave_sync();  // every lane has read the matrix
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kL1NT<N>; ++i) KA[i] = K[i];
    }
    lds_wave_sync();
    return KA;
}

template <int N>
__device__ int l1_wave_cert(const L1Wave<N>& W, double* red, int lane, double ylo, double yhi) {
    double v[N + 2];
#pragma unroll
    for (int a = 0; a < N + 2; ++a) v[a] = 0.0;
#pragma unroll
    for (int q = 0; q < L1Wave<N>::NHS; ++q) {
        if (!W.hon[q]) continue;
#pragma unroll
        for (int a = 0; a < N; ++a) v[a] += W.hl[q] * W.hg[q][a];
        v[N] += W.hl[q] * W.hh[q];
        v[N + 1] += fabs(W.hl[q] * W.hh[q]);
    }
    wave_sum_lds<N + 2>(v, red, lane);
    return hvp::l1_farkas<N>(v, v[N], v[N + 1], ylo, yhi) ? hvp::L1_INFEASIBLE : hvp::L1_FAIL;
}

template <int N>
__device__ int l1_wave_solve(L1Wave<N>& W, double* y, double v0, int mh, int mp, int max_iter, int& iters,
                             double* red, int lane, double ylo, double yhi) {
    constexpr int NPS = L1Wave<N>::NPS, NHS = L1Wave<N>::NHS;
    const int mtot = mh + 2 * mp;
#pragma unroll
    for (int i = 0; i < N; ++i) y[i] = v0;
    double hsc = 1.0, wmx = 1.0;
#pragma unroll
    for (int q = 0; q < NHS; ++q) {
        if (!W.hon[q]) continue;
        W.hs[q] = fmax(W.hh[q] - hvp::l1_dot<N>(W.hg[q], y), 1.0);
        W.hl[q] = 1.0;
        hsc = fmax(hsc, fabs(W.hh[q]));
    }
#pragma unroll
    for (int q = 0; q < NPS; ++q) {
        if (!W.pon[q]) continue;
        const double e = hvp::l1_dot<N>(W.pg[q], y) + W.pe0[q];
        W.pt[q] = (W.pal[q] > 0.0 ? fabs(e) : fmax(e, 0.0)) + 1.0;
        W.ps1[q] = W.pt[q] - e;
        W.ps2[q] = W.pt[q] + W.pal[q] * e;
        W.pl1[q] = 0.5 * W.pw[q];
        W.pl2[q] = 0.5 * W.pw[q];
        wmx = fmax(wmx, W.pw[q]);
        hsc = fmax(hsc, fabs(W.pe0[q]));
    }
    hsc = wave_max(hsc);
    wmx = wave_max(wmx);
    for (iters = 0; iters < max_iter; ++iters) {
        // acc = [gap, obj, rd_y (N), rhs (N)]: one LDS all-reduce; the matrix after the stop test
        double acc[kL1Res<N>];
#pragma unroll
        for (int i = 0; i < kL1Res<N>; ++i) acc[i] = 0.0;
        double* rdy = acc + 2;
        double* rhs = acc + 2 + N;
        double rpm = 0.0, rdm = 0.0;
        W.contrib(y, false, 0.0, rhs, acc[0], acc[1], rdy, rpm, rdm);
        wave_sum_lds32<kL1Res<N>>(acc, red, lane);
        const double gap = acc[0], obj = acc[1];
        rpm = wave_max(rpm);
        rdm = wave_max(rdm);
#pragma unroll
        for (int i = 0; i < N; ++i) rdm = fmax(rdm, fabs(rdy[i]));
        if (rpm <= 1e-10 * hsc && rdm <= 1e-10 * wmx && gap <= 1e-12 * fmax(1.0, fabs(obj))) return hvp::L1_OK;
        const double mu = gap / mtot;
        const double* K = l1_newton_factor<N>(W, y, red, lane);  // the factor, in LDS
        double dy[N];
        hvp::chol_solve<N>(K, rhs, dy);
        double ap = 1.0, ad = 1.0;
        W.directions(y, dy, false, 0.0, ap, ad);
        ap = wave_min(ap);
        ad = wave_min(ad);
        double gaff = 0.0;
#pragma unroll
        for (int q = 0; q < NHS; ++q)
            if (W.hon[q]) gaff += (W.hs[q] + ap * W.hds[q]) * (W.hl[q] + ad * W.hdl[q]);
#pragma unroll
        for (int q = 0; q < NPS; ++q)
            if (W.pon[q])
                gaff += (W.ps1[q] + ap * W.pds1[q]) * (W.pl1[q] + ad * W.pdl1[q]) +
                        (W.ps2[q] + ap * W.pds2[q]) * (W.pl2[q] + ad * W.pdl2[q]);
        gaff = wave_sum(gaff);
        const double ratio = gaff / gap;
        const double sigmu = ratio * ratio * ratio * mu;
        // corrector: same K, new right-hand side; a step shorter than kL1Short is replaced by a pure
        // centring step (hvp_l1.h l1_solve)
        for (int pass = 0; pass < 2; ++pass) {
            const bool corr = pass == 0;
            const double sm = corr ? sigmu : hvp::kL1Centre * mu;
            double rhs2[N], dum[N];
#pragma unroll
            for (int i = 0; i < N; ++i) rhs2[i] = dum[i] = 0.0;
            double g2 = 0.0, o2 = 0.0, r2 = 0.0, d2 = 0.0;
            W.contrib(y, corr, sm, rhs2, g2, o2, dum, r2, d2);
            wave_sum_lds<N>(rhs2, red, lane);
            hvp::chol_solve<N>(K, rhs2, dy);
            ap = 1.0 / 0.995;
            ad = 1.0 / 0.995;
            W.directions(y, dy, corr, sm, ap, ad);
            ap = wave_min(ap);
            ad = wave_min(ad);
            if (fmin(ap, ad) >= hvp::kL1Short) break;
        }
        ap *= 0.995;
        ad *= 0.995;
#pragma unroll
        for (int a = 0; a < N; ++a) y[a] += ap * dy[a];
#pragma unroll
        for (int q = 0; q < NHS; ++q) {
            if (!W.hon[q]) continue;
            W.hs[q] += ap * W.hds[q];
            W.hl[q] += ad * W.hdl[q];
        }
#pragma unroll
        for (int q = 0; q < NPS; ++q) {
            if (!W.pon[q]) continue;
            W.pt[q] += ap * W.pdt[q];
            W.ps1[q] += ap * W.pds1[q];
            W.ps2[q] += ap * W.pds2[q];
            W.pl1[q] += ad * W.pdl1[q];
            W.pl2[q] += ad * W.pdl2[q];
        }
    }
    return l1_wave_cert<N>(W, red, lane, ylo, yhi);
}

// one (node) LP of instance (S, rl, prm): the rows relaxed after K steps from v_K in [rlo, rhi]
// (K = N: the fixed-sequence LP of code); y (uniform) receives the iterate, cost (on L1_OK) the
// objective term by term (l1_direct_cost of the same relaxation).  Every lane of the wave calls it.
template <int N, bool COST = true>
__device__ int l1_node_lp(const hvp_system& S, const hvp::Consts& C, int rl, const double* prm, uint64_t code, int K,
                          double rlo, double rhi, double* y, double& cost, int& iters, double* red, int lane) {
    if (hvp::l1_infeasible<N>(S, C, prm, code, K, rlo, rhi)) {  // exact test of the hard rows
        iters = 0;
        cost = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) y[i] = prm[1];
        return hvp::L1_INFEASIBLE;
    }
    L1Wave<N> W;
    int mh = 0, mp = 0;
    W.load(S, C, rl, prm, code, K, rlo, rhi, lane, mh, mp, red + kL1Lds<N>);
    const int st = l1_wave_solve<N>(W, y, prm[1], mh, mp, C.max_iter, iters, red, lane, S.vmin, S.vmax);
    cost = COST && st == hvp::L1_OK ? hvp::l1_direct_cost<N>(y, S, C, rl, prm, code, K, rlo, rhi) : 0.0;
    return st;
}

// ---- naive ADMM with min_1_norm (LocalMpcADMM(quadratic_cost=False), fleet_naive_admm.py:74-77)
// The local problem keeps the neighbour COPIES (x_front / x_back, (2, N+1) each, :84-102) as
// variables: their L1 tracking terms (:110-133 under min_1_norm), the soft safe rows on their
// positions (:205-236, slack eliminated: w max(0, .)) and the quadratic ADMM terms
// y'(c - z) + rho/2 |c - z|^2 (:172-198).  With sigma fixed it is a QP whose only curvature is the
// copies' rho -- neither the velocity-space active-set solvers (no curvature in y) nor the simplex
// take it.  Solved by the wave interior point above with the copies as extra variables: lane
// l < 2(N+1) owns the copy GROUP (side = l / (N+1), step k = l % (N+1)), i.e. the two copies
// (position, velocity) of that side and step and the up to three pairs that touch them (the two
// tracking terms, the safe hinge), each the row g.y + h.c + e0 around its epigraph variable.  Each
// group's 2 x 2 block rho I + sum ce h h' is eliminated into the N x N Newton matrix (Schur
// complement) and recovered after the solve (dc = A^-1 (rc - A_cy dy)), so the system stays N x N;
// hard rows and the own pairs (leader tracking, Q_u |u|, Q_du |du|) are L1Wave's.  Primal and dual
// take one common step (the copies' dual residual rho c + q + sum (l1 - al l2) h couples both).
template <int N>
struct L1AdmmWave {
    static constexpr int NQ = 3;  // pairs of a copy group: position tracking, velocity tracking, safe hinge
    L1Wave<N> W;
    bool gon;
    double rho, c[2], q[2], dc[2];  // the group's copies (p, v) and linear terms y - rho z
    double k0;                      // constant of the ADMM terms: y'(c - z) + rho/2 |c - z|^2 = rho/2 c'c + q'c + k0
    bool qon[NQ];
    LdsRows<N> qg;  // the pairs' row vectors in y (LDS, after the own rows' slots)
    double qh[NQ][2], qe0[NQ], qw[NQ], qal[NQ], qt[NQ], qs1[NQ], qs2[NQ], ql1[NQ], ql2[NQ];
    double qds1[NQ], qdl1[NQ], qds2[NQ], qdl2[NQ], qdt[NQ];

    // the own rows (hard rows, leader tracking, inputs: l1_rows with the ADMM params layout) and this
    // lane's copy group; mg = pairs of every group of the wave
    __device__ bool load(const hvp_system& S, const hvp::Consts& C, int rl, const double* prm, uint64_t code, int K,
                         double rlo, double rhi, int lane, int& mh, int& mp, int& mg, double* gbuf) {
        const bool ok = W.load(S, C, rl & HVP_ROLE_TRACK_LEADER, prm, code, K, rlo, rhi, lane, mh, mp, gbuf, 8);
        qg.base = gbuf + kL1GSlots<N> * N * 64 + lane;
        W.rel = true;
        constexpr int K1 = N + 1;
        const int side = lane / K1, k = lane % K1;
        gon = lane < 2 * K1 && (rl & (side == 0 ? HVP_ROLE_SAFE_FRONT : HVP_ROLE_SAFE_BACK)) != 0;
        rho = C.rho;
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            qon[j] = false;
            qe0[j] = qw[j] = qal[j] = qt[j] = ql1[j] = ql2[j] = 0.0;
            qs1[j] = qs2[j] = 1.0;
            qds1[j] = qdl1[j] = qds2[j] = qdl2[j] = qdt[j] = 0.0;
            qh[j][0] = qh[j][1] = 0.0;
#pragma unroll
            for (int a = 0; a < N; ++a) qg[j][a] = 0.0;
        }
        c[0] = c[1] = q[0] = q[1] = dc[0] = dc[1] = k0 = 0.0;
        if (gon) {
            const double* yy = hvp::admm_y(prm, side, N);
            const double* zz = hvp::admm_z(prm, side, N);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                c[i] = zz[i * K1 + k] - yy[i * K1 + k] / rho;  // the ADMM term's own minimiser
                q[i] = yy[i * K1 + k] - rho * zz[i * K1 + k];
                k0 += 0.5 * rho * zz[i * K1 + k] * zz[i * K1 + k] - yy[i * K1 + k] * zz[i * K1 + k];
            }
            const bool tr = (rl & (side == 0 ? HVP_ROLE_TRACK_FRONT : HVP_ROLE_TRACK_BACK)) != 0;
            const double ts = S.ts, P1 = prm[0] + ts * prm[1];
            const double pc = k == 0 ? prm[0] : P1, vc = k == 0 ? prm[1] : 0.0;  // constant parts of p_k, v_k
            const double sg = side == 0 ? 1.0 : -1.0;  // front: own - copy (:110-121), back: copy - own (:122-133)
            // pair 0: position tracking (front: p + t0 v + d0 - c_p; back: c_p + t0 c_v + d0 - p)
            if (tr && C.Qpp > 0.0) {
                qon[0] = true;
#pragma unroll
                for (int a = 0; a < N; ++a) {
                    const double gp = (k >= 2 && a <= k - 2) ? ts : 0.0, gv = (k >= 1 && a == k - 1) ? 1.0 : 0.0;
                    qg[0][a] = side == 0 ? gp + C.t0 * gv : -gp;
                }
                qh[0][0] = -sg;
                qh[0][1] = side == 0 ? 0.0 : C.t0;
                qe0[0] = side == 0 ? pc + C.t0 * vc + C.d0 : C.d0 - pc;
                qw[0] = C.Qpp;
                qal[0] = 1.0;
            }
            // pair 1: velocity tracking (front: v - c_v; back: c_v - v)
            if (tr && C.Qvv > 0.0) {
                qon[1] = true;
#pragma unroll
                for (int a = 0; a < N; ++a) qg[1][a] = (k >= 1 && a == k - 1) ? sg : 0.0;
                qh[1][1] = -sg;
                qe0[1] = sg * vc;
                qw[1] = C.Qvv;
                qal[1] = 1.0;
            }
            // pair 2: the soft safe row, w max(0, p - c_p + d_safe) (front) / w max(0, c_p + d_safe - p) (back)
            if (C.w > 0.0) {
                qon[2] = true;
#pragma unroll
                for (int a = 0; a < N; ++a) qg[2][a] = (k >= 2 && a <= k - 2) ? sg * ts : 0.0;
                qh[2][0] = -sg;
                qe0[2] = side == 0 ? pc + C.d_safe : C.d_safe - pc;
                qw[2] = C.w;
                qal[2] = 0.0;
            }
            cnt = (int)qon[0] + (int)qon[1] + (int)qon[2];
        }
        double cs = (double)cnt;
        mg = (int)wave_sum(cs);
        return ok;
    }

    __device__ double hc(int j, const double* cc) const { return qh[j][0] * cc[0] + qh[j][1] * cc[1]; }

    // the per-pair terms of contrib / directions (hvp_l1.h l1_direction) at the pair's row value gy
    struct PairTerms {
        double rp1, rp2, D1, D2, rho1, rho2, rdt, rhst, mt, m, ce, coef;
    };
    __device__ PairTerms pair_terms(int j, double gy, bool corr, double sigmu) const {
        PairTerms P;
        const double al = qal[j];
        P.rp1 = gy - qt[j] + qs1[j] + qe0[j];
        P.rp2 = -al * gy - qt[j] + qs2[j] - al * qe0[j];
        P.D1 = ql1[j] / qs1[j];
        P.D2 = ql2[j] / qs2[j];
        const double rc1 = qs1[j] * ql1[j] + (corr ? qds1[j] * qdl1[j] : 0.0) - sigmu;
        const double rc2 = qs2[j] * ql2[j] + (corr ? qds2[j] * qdl2[j] : 0.0) - sigmu;
        P.rho1 = (ql1[j] * P.rp1 - rc1) / qs1[j];
        P.rho2 = (ql2[j] * P.rp2 - rc2) / qs2[j];
        P.rdt = qw[j] - ql1[j] - ql2[j];
        P.rhst = -P.rdt + P.rho1 + P.rho2;
        P.mt = P.D1 + P.D2;
        P.m = al * P.D2 - P.D1;
        P.ce = P.D1 * P.D2 * (1.0 + al) * (1.0 + al) / P.mt;
        P.coef = -(ql1[j] - al * ql2[j]) - (P.rho1 - al * P.rho2) - P.m * P.rhst / P.mt;
        return P;
    }

    // the group's copy block A = rho I + sum ce h h' (inverse), A_cy dy (when dy), and rc = -(rho c + q)
    // + sum coef h; also adds the group's pair terms to rhs / residuals when acc (the matrix: kpart)
    __device__ void group_block(const double* y, const double* dy, bool corr, double sigmu,
                                double* rhs, double& gap, double& obj, double* rdy, double& rpm, double& rdm, bool acc,
                                double& i00, double& i01, double& i11, double& rc0, double& rc1, double& ad0,
                                double& ad1) const {
        double a00 = rho, a01 = 0.0, a11 = rho;
        rc0 = -(rho * c[0] + q[0]);
        rc1 = -(rho * c[1] + q[1]);
        double rd0 = -rc0, rd1 = -rc1;
        ad0 = ad1 = 0.0;
        double acy[2][N];
#pragma unroll
        for (int a = 0; a < N; ++a) acy[0][a] = acy[1][a] = 0.0;
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            if (!qon[j]) continue;
            const double gy = hvp::l1_dot<N>(qg[j], y) + hc(j, c);
            const PairTerms P = pair_terms(j, gy, corr, sigmu);
            const double h0 = qh[j][0], h1 = qh[j][1], lm = ql1[j] - qal[j] * ql2[j];
            a00 += P.ce * h0 * h0;
            a01 += P.ce * h0 * h1;
            a11 += P.ce * h1 * h1;
            rc0 += P.coef * h0;
            rc1 += P.coef * h1;
            rd0 += lm * h0;
            rd1 += lm * h1;
            if (dy) {
                const double gd = hvp::l1_dot<N>(qg[j], dy);
                ad0 += P.ce * h0 * gd;
                ad1 += P.ce * h1 * gd;
            }
            if (acc) {
                gap += qs1[j] * ql1[j] + qs2[j] * ql2[j];
                obj += qw[j] * qt[j];
                rpm = fmax(rpm, fmax(fabs(P.rp1), fabs(P.rp2)) / (1.0 + fabs(qe0[j])));
                rdm = fmax(rdm, fabs(P.rdt));
#pragma unroll
                for (int a = 0; a < N; ++a) {
                    rdy[a] += lm * qg[j][a];
                    rhs[a] += P.coef * qg[j][a];
                    acy[0][a] += P.ce * h0 * qg[j][a];
                    acy[1][a] += P.ce * h1 * qg[j][a];
                }
            }
        }
        const double det = a00 * a11 - a01 * a01;
        i00 = a11 / det;
        i01 = -a01 / det;
        i11 = a00 / det;
        if (acc) {
            rdm = fmax(rdm, fmax(fabs(rd0), fabs(rd1)));
            // the objective itself (the ADMM terms are small near the optimum, c ~ z): the gap test's scale
            obj += 0.5 * rho * (c[0] * c[0] + c[1] * c[1]) + q[0] * c[0] + q[1] * c[1] + k0;
            // Schur complement of the copy block: rhs -= A_yc A^-1 rc (K -= A_yc A^-1 A_cy: kpart)
            const double w0 = i00 * rc0 + i01 * rc1, w1 = i01 * rc0 + i11 * rc1;
#pragma unroll
            for (int a = 0; a < N; ++a) rhs[a] -= acy[0][a] * w0 + acy[1][a] * w1;
        }
    }

    __device__ void contrib(const double* y, bool corr, double sigmu, double* rhs, double& gap, double& obj,
                            double* rdy, double& rpm, double& rdm) const {
        W.contrib(y, corr, sigmu, rhs, gap, obj, rdy, rpm, rdm);
        if (!gon) return;
        double i00, i01, i11, rc0, rc1, ad0, ad1;
        group_block(y, nullptr, corr, sigmu, rhs, gap, obj, rdy, rpm, rdm, true, i00, i01, i11, rc0, rc1, ad0, ad1);
    }

    // the Newton matrix in chunks (L1Wave::kpart): the own rows' weights, then per copy group its
    // pairs' ce and the copy block's inverse and A_cy (group_block's, at the predictor's corr =
    // false, sigmu = 0), whose Schur complement K -= A_yc A^-1 A_cy follows the pairs' terms
    struct Wts {
        typename L1Wave<N>::Wts w;
        double ce[NQ], i00, i01, i11, acy[2][N];
    };
    __device__ void weights(const double* y, Wts& g) const {
        W.weights(y, g.w);
        double a00 = rho, a01 = 0.0, a11 = rho;
#pragma unroll
        for (int a = 0; a < N; ++a) g.acy[0][a] = g.acy[1][a] = 0.0;
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            g.ce[j] = 0.0;
            if (!qon[j]) continue;
            const PairTerms P = pair_terms(j, hvp::l1_dot<N>(qg[j], y) + hc(j, c), false, 0.0);
            const double h0 = qh[j][0], h1 = qh[j][1];
            a00 += P.ce * h0 * h0;
            a01 += P.ce * h0 * h1;
            a11 += P.ce * h1 * h1;
            g.ce[j] = P.ce;
#pragma unroll
            for (int a = 0; a < N; ++a) {
                g.acy[0][a] += P.ce * h0 * qg[j][a];
                g.acy[1][a] += P.ce * h1 * qg[j][a];
            }
        }
        const double det = a00 * a11 - a01 * a01;
        g.i00 = a11 / det;
        g.i01 = -a01 / det;
        g.i11 = a00 / det;
    }
    template <int E0, int CH>
    __device__ void kpart(const Wts& g, double* kc) const {
        W.template kpart<E0, CH>(g.w, kc);
        if (!gon) return;
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            if (!qon[j]) continue;
#pragma unroll
            for (int a = 0; a < N; ++a) {
#pragma unroll
                for (int b = 0; b <= a; ++b) {
                    const int e = hvp::tri(a, b) - E0;
                    if (e >= 0 && e < CH) kc[e] += g.ce[j] * qg[j][a] * qg[j][b];
                }
            }
        }
#pragma unroll
        for (int a = 0; a < N; ++a) {
            const double u0 = g.i00 * g.acy[0][a] + g.i01 * g.acy[1][a], u1 = g.i01 * g.acy[0][a] + g.i11 * g.acy[1][a];
#pragma unroll
            for (int b = 0; b <= a; ++b) {
                const int e = hvp::tri(a, b) - E0;
                if (e >= 0 && e < CH) kc[e] -= u0 * g.acy[0][b] + u1 * g.acy[1][b];
            }
        }
    }

    __device__ void directions(const double* y, const double* dy, bool corr, double sigmu, double& ap, double& ad) {
        W.directions(y, dy, corr, sigmu, ap, ad);
        if (!gon) return;
        double i00, i01, i11, rc0, rc1, ad0, ad1, dum = 0.0;
        group_block(y, dy, corr, sigmu, nullptr, dum, dum, nullptr, dum, dum, false, i00, i01, i11, rc0, rc1, ad0, ad1);
        dc[0] = i00 * (rc0 - ad0) + i01 * (rc1 - ad1);
        dc[1] = i01 * (rc0 - ad0) + i11 * (rc1 - ad1);
        // every pair's terms from the stored (predictor) directions first, then the new directions
        PairTerms P[NQ];
        double gys[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            gys[j] = hvp::l1_dot<N>(qg[j], y) + hc(j, c);
            P[j] = pair_terms(j, gys[j], corr, sigmu);
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            if (!qon[j]) continue;
            const double al = qal[j];
            const double gd = hvp::l1_dot<N>(qg[j], dy) + hc(j, dc);
            qdt[j] = (P[j].rhst - P[j].m * gd) / P[j].mt;
            const double a1 = gd - qdt[j], a2 = -al * gd - qdt[j];
            qds1[j] = -P[j].rp1 - a1;
            qds2[j] = -P[j].rp2 - a2;
            const bool big1 = P[j].D1 >= P[j].D2;
            const double dls = big1 ? P[j].D2 * a2 + P[j].rho2 : P[j].D1 * a1 + P[j].rho1;
            qdl1[j] = big1 ? P[j].rdt - dls : dls;
            qdl2[j] = big1 ? dls : P[j].rdt - dls;
            hvp::l1_ratio(ap, qs1[j], qds1[j]);
            hvp::l1_ratio(ap, qs2[j], qds2[j]);
            hvp::l1_ratio(ad, ql1[j], qdl1[j]);
            hvp::l1_ratio(ad, ql2[j], qdl2[j]);
        }
    }

    // the group's copies at their exact minimisers given the own trajectory y (hvp_l1.h copy_exact)
    // and its objective term by term: ADMM terms and the pairs' w |e| / w max(0, e)
    __device__ double group_cost(const double* y, const hvp_system& S, const hvp::Consts& C, int rl, const double* prm,
                                 int lane) {
        if (!gon) return 0.0;
        constexpr int K1 = N + 1;
        const int side = lane / K1, k = lane % K1;
        const double* yy = hvp::admm_y(prm, side, N);
        const double* zz = hvp::admm_z(prm, side, N);
        double p = prm[0], v = prm[1];  // own state at step k
        if (k >= 1) {
            p = prm[0] + S.ts * prm[1];
#pragma unroll
            for (int a = 0; a < N; ++a)
                if (a <= k - 2) p += S.ts * y[a];
#pragma unroll
            for (int a = 0; a < N; ++a)
                if (a == k - 1) v = y[a];
        }
        const double m[2] = {zz[k] - yy[k] / rho, zz[K1 + k] - yy[K1 + k] / rho};
        hvp::copy_exact(hvp::copy_terms(C, rl, side, p, v), rho, m, c);
        double J = 0.0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const double d = c[i] - zz[i * K1 + k];
            J += yy[i * K1 + k] * d + 0.5 * rho * d * d;
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            if (!qon[j]) continue;
            const double e = hvp::l1_dot<N>(qg[j], y) + hc(j, c) + qe0[j];
            J += qw[j] * (qal[j] > 0.0 ? fabs(e) : fmax(e, 0.0));
        }
        return J;
    }
};

// Mehrotra predictor-corrector of l1_wave_solve with the copy groups (L1AdmmWave).
template <int N>
__device__ int l1_admm_wave_solve(L1AdmmWave<N>& A, double* y, double v0, int mh, int mp, int mg, int max_iter,
                                  int& iters, double* red, int lane, double ylo, double yhi, bool leaf) {
    constexpr int NPS = L1Wave<N>::NPS, NHS = L1Wave<N>::NHS, NQ = L1AdmmWave<N>::NQ;
    L1Wave<N>& W = A.W;
    const int mtot = mh + 2 * mp + 2 * mg;
#pragma unroll
    for (int i = 0; i < N; ++i) y[i] = v0;
    double hsc = 1.0, wmx = 1.0;
#pragma unroll
    for (int q = 0; q < NHS; ++q) {
        if (!W.hon[q]) continue;
        W.hs[q] = fmax(W.hh[q] - hvp::l1_dot<N>(W.hg[q], y), 1.0);
        W.hl[q] = 1.0;
        hsc = fmax(hsc, fabs(W.hh[q]));
    }
#pragma unroll
    for (int q = 0; q < NPS; ++q) {
        if (!W.pon[q]) continue;
        const double e = hvp::l1_dot<N>(W.pg[q], y) + W.pe0[q];
        W.pt[q] = (W.pal[q] > 0.0 ? fabs(e) : fmax(e, 0.0)) + 1.0;
        W.ps1[q] = W.pt[q] - e;
        W.ps2[q] = W.pt[q] + W.pal[q] * e;
        W.pl1[q] = 0.5 * W.pw[q];
        W.pl2[q] = 0.5 * W.pw[q];
        wmx = fmax(wmx, W.pw[q]);
        hsc = fmax(hsc, fabs(W.pe0[q]));
    }
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        if (!A.qon[j]) continue;
        const double e = hvp::l1_dot<N>(A.qg[j], y) + A.hc(j, A.c) + A.qe0[j];
        A.qt[j] = (A.qal[j] > 0.0 ? fabs(e) : fmax(e, 0.0)) + 1.0;
        A.qs1[j] = A.qt[j] - e;
        A.qs2[j] = A.qt[j] + A.qal[j] * e;
        A.ql1[j] = 0.5 * A.qw[j];
        A.ql2[j] = 0.5 * A.qw[j];
        wmx = fmax(wmx, A.qw[j]);
        hsc = fmax(hsc, fabs(A.qe0[j]));
    }
    if (A.gon) wmx = fmax(wmx, fmax(fabs(A.q[0]), fabs(A.q[1])));
    hsc = wave_max(hsc);
    wmx = wave_max(wmx);
    double ybest[N], best_rdm = 1e300;
    for (iters = 0; iters < max_iter; ++iters) {
        double acc[kL1Res<N>];
#pragma unroll
        for (int i = 0; i < kL1Res<N>; ++i) acc[i] = 0.0;
        double* rdy = acc + 2;
        double* rhs = acc + 2 + N;
        double rpm = 0.0, rdm = 0.0;
        A.contrib(y, false, 0.0, rhs, acc[0], acc[1], rdy, rpm, rdm);
        wave_sum_lds32<kL1Res<N>>(acc, red, lane);
        const double gap = acc[0], obj = acc[1];
        rpm = wave_max(rpm);
        rdm = wave_max(rdm);
#pragma unroll
        for (int i = 0; i < N; ++i) rdm = fmax(rdm, fabs(rdy[i]));
        // (primal residuals relative to each row's constant, W.rel; the objective's own scale)
        if (rpm <= 1e-11 && rdm <= 1e-10 * wmx && gap <= 1e-12 * fmax(1.0, fabs(obj))) return hvp::L1_OK;
        // Past primal convergence the dual residual of some nodes oscillates (0.2 .. 7 at wmx = 1e4
        // for 100 iterations: admm_l1_local_ct_N5 instance 5, profiles/r06r.log) while y, the copies
        // and the objective stay put.  The iterate with the smallest dual residual among those within
        // a looser test is kept and returned when the strict test is never met (the copies are
        // re-priced exactly from y, copy_exact).  Only at a leaf (K = N), where the price of a feasible
        // point is what the search compares: at an interior node the price is used as a lower bound,
        // which a primal point short of the strict test (dual residual up to 1e-8 wmx) does not give
        // -- such a node stays unresolved (L1_FAIL: it prunes nothing).
        const bool loose = leaf && rpm <= 1e-9 && rdm <= 1e-8 * wmx && gap <= 1e-10 * fmax(1.0, fabs(obj));
        if (loose && rdm < best_rdm) {
            best_rdm = rdm;
#pragma unroll
            for (int i = 0; i < N; ++i) ybest[i] = y[i];
        }
        const double mu = gap / mtot;
        const double* K = l1_newton_factor<N>(A, y, red, lane);  // the factor, in LDS
        double dy[N];
        hvp::chol_solve<N>(K, rhs, dy);
        double ap = 1.0, ad = 1.0;
        A.directions(y, dy, false, 0.0, ap, ad);
        ap = wave_min(fmin(ap, ad));
        ad = ap;
        double gaff = 0.0;
#pragma unroll
        for (int q = 0; q < NHS; ++q)
            if (W.hon[q]) gaff += (W.hs[q] + ap * W.hds[q]) * (W.hl[q] + ad * W.hdl[q]);
#pragma unroll
        for (int q = 0; q < NPS; ++q)
            if (W.pon[q])
                gaff += (W.ps1[q] + ap * W.pds1[q]) * (W.pl1[q] + ad * W.pdl1[q]) +
                        (W.ps2[q] + ap * W.pds2[q]) * (W.pl2[q] + ad * W.pdl2[q]);
#pragma unroll
        for (int j = 0; j < NQ; ++j)
            if (A.qon[j])
                gaff += (A.qs1[j] + ap * A.qds1[j]) * (A.ql1[j] + ad * A.qdl1[j]) +
                        (A.qs2[j] + ap * A.qds2[j]) * (A.ql2[j] + ad * A.qdl2[j]);
        gaff = wave_sum(gaff);
        const double ratio = gaff / gap;
        const double sigmu = ratio * ratio * ratio * mu;
        for (int pass = 0; pass < 2; ++pass) {
            const bool corr = pass == 0;
            const double sm = corr ? sigmu : hvp::kL1Centre * mu;
            double rhs2[N], dum[N];
#pragma unroll
            for (int i = 0; i < N; ++i) rhs2[i] = dum[i] = 0.0;
            double g2 = 0.0, o2 = 0.0, r2 = 0.0, d2 = 0.0;
            A.contrib(y, corr, sm, rhs2, g2, o2, dum, r2, d2);
            wave_sum_lds<N>(rhs2, red, lane);
            hvp::chol_solve<N>(K, rhs2, dy);
            ap = 1.0 / 0.995;
            ad = 1.0 / 0.995;
            A.directions(y, dy, corr, sm, ap, ad);
            ap = wave_min(fmin(ap, ad));
            ad = ap;
            if (ap >= hvp::kL1Short) break;
        }
        ap *= 0.995;
        ad *= 0.995;
#pragma unroll
        for (int a = 0; a < N; ++a) y[a] += ap * dy[a];
        A.c[0] += ap * A.dc[0];
        A.c[1] += ap * A.dc[1];
#pragma unroll
        for (int q = 0; q < NHS; ++q) {
            if (!W.hon[q]) continue;
            W.hs[q] += ap * W.hds[q];
            W.hl[q] += ad * W.hdl[q];
        }
#pragma unroll
        for (int q = 0; q < NPS; ++q) {
            if (!W.pon[q]) continue;
            W.pt[q] += ap * W.pdt[q];
            W.ps1[q] += ap * W.pds1[q];
            W.ps2[q] += ap * W.pds2[q];
            W.pl1[q] += ad * W.pdl1[q];
            W.pl2[q] += ad * W.pdl2[q];
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            if (!A.qon[j]) continue;
            A.qt[j] += ap * A.qdt[j];
            A.qs1[j] += ap * A.qds1[j];
            A.qs2[j] += ap * A.qds2[j];
            A.ql1[j] += ad * A.qdl1[j];
            A.ql2[j] += ad * A.qdl2[j];
        }
    }
    if (best_rdm < 1e300) {  // (wave-uniform: the residuals are wave reductions)
#pragma unroll
        for (int i = 0; i < N; ++i) y[i] = ybest[i];
        return hvp::L1_OK;
    }
    return l1_wave_cert<N>(W, red, lane, ylo, yhi);
}

// The naive-ADMM form's LDS buffer (reduction rows, K area, row vectors) as a module-scope variable:
// its kernels run one wave per block (kL1BlockOfA), and the node LP below is an outlined function of
// three kernels; reached through this variable its LDS accesses stay ds_* instructions (through the
// kernels' pointer argument the callee saw a generic pointer: flat instructions).
template <int N>
__shared__ double g_l1_admm_lds[kL1LdsAll<N, true>];

// one (node) LP of the naive-ADMM min_1_norm form, as l1_node_lp; xf_o / xb_o (optional, the
// instance's (2, N+1) rows): the optimal copies, written by the lanes that own them
template <int N>
__device__ int l1_admm_node_lp(const hvp_system& S, const hvp::Consts& C, int rl, const double* prm, uint64_t code,
                               int K, double rlo, double rhi, double* y, double& cost, int& iters, double* red, int lane,
                               double* xf_o = nullptr, double* xb_o = nullptr) {
    if (hvp::l1_infeasible<N>(S, C, prm, code, K, rlo, rhi)) {  // the hard rows do not involve the copies
        iters = 0;
        cost = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) y[i] = prm[1];
        return hvp::L1_INFEASIBLE;
    }
    red = g_l1_admm_lds<N>;  // the caller's buffer (one wave per block), with its address space
    L1AdmmWave<N> A;
    int mh = 0, mp = 0, mg = 0;
    A.load(S, C, rl, prm, code, K, rlo, rhi, lane, mh, mp, mg, red + kL1Lds<N>);
    const int st = l1_admm_wave_solve<N>(A, y, prm[1], mh, mp, mg, C.max_iter, iters, red, lane, S.vmin, S.vmax,
                                            K == N);
    cost = 0.0;
    if (st == hvp::L1_OK) {
        const double own = hvp::l1_direct_cost<N>(y, S, C, rl & HVP_ROLE_TRACK_LEADER, prm, code, K, rlo, rhi, 8);
        cost = own + wave_sum(A.group_cost(y, S, C, rl, prm, lane));
    }
    constexpr int K1 = N + 1;
    if (lane < 2 * K1) {
        double* o = lane < K1 ? xf_o : xb_o;
        const int k = lane % K1;
        if (o) {
            o[k] = st == hvp::L1_OK && A.gon ? A.c[0] : 0.0;
            o[K1 + k] = st == hvp::L1_OK && A.gon ? A.c[1] : 0.0;
        }
    }
    return st;
}

constexpr int kL1Block = 256;
template <int N>
constexpr int kL1BlockOf = N <= HVP_MAX_N_ENUM ? kL1Block : 128;  // LDS: kL1LdsAll doubles per wave
// the naive-ADMM form: one wave per block (one wave per SIMD by registers; its copy groups' row
// vectors make a wave's LDS ~41 KB at N = 8, ~53 KB at N = 10: three or four blocks of one wave fit a
// CU where blocks of two or four waves would leave SIMDs idle or not fit at all)
template <int N, bool ADMM>
constexpr int kL1BlockOfA = ADMM ? 64 : kL1BlockOf<N>;

template <int N>
__global__ __launch_bounds__(kL1Block) void k_qp_l1(const hvp_system* __restrict__ systems,
                                                    const int32_t* __restrict__ sys, const int32_t* __restrict__ role,
                                                    const double* __restrict__ params, hvp::Consts C, Workspace ws) {
    static_assert(8 * N - 2 <= 64, "enumeration: one hard row per lane");
    __shared__ double s_red[kL1Block / 64][kL1LdsAll<N>];
    const unsigned long long reserved = ws.counter[0];
    const long long total = (long long)(reserved < (unsigned long long)ws.cap ? reserved : ws.cap);
    const int lane = threadIdx.x & 63;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    unsigned long long iter_sum = 0;
    for (long long t = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; t < total; t += nwaves) {
        const int inst = ws.task_inst[t];  // wave-uniform
        if (inst < 0) continue;             // dead slot of an overflowed instance
        const hvp_system& S = systems[sys[inst]];
        const double* prm = params + (size_t)inst * (2 + 6 * (N + 1));
        double y[N], cost;
        int iters = 0;
        const int status = l1_node_lp<N, false>(S, C, role[inst], prm, ws.task_code[t], N, 0.0, -1.0, y, cost,
                                                iters, s_red[threadIdx.x >> 6], lane);  // k_cost prices it
        if (lane == 0) {
            ws.task_stat[t] = status | (iters << 8);
#pragma unroll
            for (int k = 0; k < N; ++k) ws.task_y[t * N + k] = y[k];
            iter_sum += (unsigned long long)iters;
        }
    }
    if (lane == 0 && iter_sum) atomicAdd(&ws.counter[1], iter_sum);
}

// ------------------------------------------------------------------ K_cost
// Objective of every converged candidate, evaluated term by term on its trajectory (separate
// launch: fused into K_qp its reference loads stay live across the IPM and spill).
template <int N>
__global__ __launch_bounds__(kBlock) void k_cost(const hvp_system* __restrict__ systems,
                                                 const int32_t* __restrict__ sys, const int32_t* __restrict__ role,
                                                 const double* __restrict__ params, hvp::Consts C, Workspace ws) {
    const unsigned long long reserved = ws.counter[0];
    const long long total = (long long)(reserved < (unsigned long long)ws.cap ? reserved : ws.cap);
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const int inst = ws.task_inst[t];
        double cost = 1e300;
        if (inst >= 0 && (ws.task_stat[t] & 0xff) == 0) {
            const hvp_system& S = systems[sys[inst]];
            const double* prm = params + (size_t)inst * (2 + 6 * (N + 1));
            hvp::LaneQp<N> q;
            const int rl = role[inst];
            q.has_sf = (rl & HVP_ROLE_SAFE_FRONT) != 0;
            q.has_sb = (rl & HVP_ROLE_SAFE_BACK) != 0;
#pragma unroll
            for (int k = 0; k < N; ++k) q.y[k] = ws.task_y[t * N + k];
            cost = C.l1 ? hvp::l1_direct_cost<N>(q.y, S, C, rl, prm, ws.task_code[t])
                        : hvp::direct_cost<N>(q, S, C, rl, prm, ws.task_code[t]);
        }
        ws.task_cost[t] = cost;
    }
}

// ------------------------------------------------------------------ K_select
template <int N>
__global__ __launch_bounds__(kBlock) void k_select(int B, const hvp_system* __restrict__ systems,
                                                   const int32_t* __restrict__ sys, const double* __restrict__ params,
                                                   Workspace ws, double* __restrict__ u_out, double* __restrict__ x_out,
                                                   int8_t* __restrict__ region_out, int8_t* __restrict__ gear_out,
                                                   double* __restrict__ cost_out, int32_t* __restrict__ status_out,
                                                   int32_t* __restrict__ nodes_out, int32_t* __restrict__ iters_out,
                                                   int l1) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const int cnt = ws.inst_cnt[i], off = ws.inst_off[i];
    const hvp_system& S = systems[sys[i]];
    const double* prm = params + (size_t)i * (2 + 6 * (N + 1));
    int status;
    int win = -1;
    int iters = 0;
    if (ws.inst_flag[i] != 0 || cnt == 0) {
        status = HVP_INFEASIBLE;
    } else if (off < 0) {
        status = HVP_OVERFLOW;
    } else {
        double best = 1e300;
        bool unresolved = false;  // min_1_norm: an LP neither solved nor proven infeasible
        for (int j = 0; j < cnt; ++j) {
            const int st = ws.task_stat[off + j];
            iters += st >> 8;
            if ((st & 0xff) == 0) best = fmin(best, ws.task_cost[off + j]);
            unresolved = unresolved || (l1 && (st & 0xff) == hvp::L1_FAIL);
        }
        if (best < 1e300) {
            const double tol = 1e-9 * fmax(1.0, fabs(best));
            for (int j = 0; j < cnt; ++j)
                if ((ws.task_stat[off + j] & 0xff) == 0 && ws.task_cost[off + j] <= best + tol) {
                    win = off + j;
                    break;
                }
        }
        // an unresolved LP may hold the optimum (its cost is unknown): never report a possibly
        // worse sequence as optimal.  (The quadratic path's fallback IPM leaves only infeasible
        // candidates unsolved: excluded, as the oracle excludes them.)
        status = win >= 0 && !unresolved ? HVP_OPTIMAL : HVP_MAXITER;
        if (l1 && best >= 1e300 && !unresolved) status = HVP_INFEASIBLE;  // every LP proven infeasible
        if (status != HVP_OPTIMAL) win = -1;
    }
    if (status_out) status_out[i] = status;
    if (nodes_out) nodes_out[i] = cnt;
    if (iters_out) iters_out[i] = iters;
    if (cost_out) cost_out[i] = win >= 0 ? ws.task_cost[win] : 1e300;
    const uint32_t code = win >= 0 ? ws.task_code[win] : 0u;
    double p = prm[0], v = prm[1];
    if (x_out) {
        x_out[(size_t)i * 2 * (N + 1)] = p;
        x_out[(size_t)i * 2 * (N + 1) + N + 1] = v;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int r = hvp::code_region(code, k);
        const double vn = win >= 0 ? ws.task_y[(size_t)win * N + k] : v;
        const double u = win >= 0 ? (vn - S.a[r] * v - S.c[r]) / S.b[r] : 0.0;
        p = p + S.ts * v;
        v = vn;
        if (u_out) u_out[(size_t)i * N + k] = u;
        if (x_out) {
            x_out[(size_t)i * 2 * (N + 1) + k + 1] = p;
            x_out[(size_t)i * 2 * (N + 1) + N + 1 + k + 1] = v;
        }
        if (region_out) region_out[(size_t)i * N + k] = (int8_t)(win >= 0 ? r : -1);
        if (gear_out) gear_out[(size_t)i * N + k] = (int8_t)(win >= 0 ? S.gear[r] : 0);
    }
}

// ================================================================== branch and bound
// Level-synchronous over the whole batch (hvp_bnb.h): K_root (relaxed root QP + greedy dive ->
// incumbent), then for every depth k = 1..N  K_expand (children of the unpruned parents, one
// atomicAdd per parent) and K_bound (one lane per child: QP with the tail relaxed after k steps;
// exact QP at k = N), then K_key / K_write / K_finish (argmin + tie rule over the leaves).
// Every kernel grid-strides over a count that lives on the device: no host round trip.
template <int N>
constexpr int kBnbBlock = N <= 8 ? 256 : 64;  // LDS rows: 7 N doubles per lane

// The incumbent is kept as an order-preserving 64-bit key of the double so that atomicMin on the
// key is a min on the cost -- for negative costs too (the ADMM objective carries y'(c - z)).
__device__ inline unsigned long long cost_key(double c) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(c);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double key_cost(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
__device__ inline double inc_of(const Workspace& ws, int inst) { return key_cost(ws.inc[inst]); }

// Occupancy target of the lane B&B kernels (waves per SIMD).  Measured at C2: 2 waves/SIMD forces
// 800 B/lane of spills and runs 2.7x slower than 1 wave/SIMD with the register file to itself
#ifndef HVP_LANE_WAVES
#define HVP_LANE_WAVES 1
#endif
#define HVP_LANE_OCC __attribute__((amdgpu_waves_per_eu(HVP_LANE_WAVES)))

// ADMM: the formulation is a template parameter so that each kernel instantiation holds ONE
// QP path (both paths in one kernel pushed the lane kernels to 256 VGPRs + scratch spills)
template <int N, int BS, bool ADMM>
__device__ inline int bnb_qp(hvp::LaneQp<N, LdsMem<N, BS>>& q, const hvp_system& S, const hvp::Consts& C, int rl,
                             const double* prm, uint64_t code, int K, double lo, double hi, double& cost,
                             int cap = kGiMaxIter<N>) {
    int it = 0, st;
    if constexpr (ADMM) {
        st = hvp::solve_admm_lane<N>(q, S, C, rl, prm, code, K, cap, it);
        cost = st == hvp::GI_OK ? hvp::admm_direct_cost<N>(q, S, C, rl, prm, code, K) : 0.0;
    } else {
        hvp::setup_lane<N>(q, S, C, rl, prm, code, K, lo, hi);  // tail relaxed from v_K in [lo, hi]
        st = hvp::solve_gi<N>(q, C, kGiMaxIter<N>, it);
        cost = st == hvp::GI_OK ? hvp::direct_cost<N>(q, S, C, rl, prm, code, K) : 0.0;
    }
    return st == hvp::GI_OK ? it : -1 - it;
}

// regions r the node's next step (`step`, from the interval [lo, hi] of v_step) can take
__device__ inline unsigned bnb_children(const hvp_system& S, const hvp::Consts& C, int step, double lo, double hi) {
    unsigned mask = 0;
    for (int r = 0; r < S.n_regions; ++r) {
        double a, b;
        if (hvp::bnb_child(S, C, step, lo, hi, r, &a, &b)) mask |= 1u << r;
    }
    return mask;
}

__device__ inline unsigned long long* bucket_count(const Workspace& ws, int b, int k);

// Naive-ADMM node records (the 16-lane path at 8 < N <= 12, Workspace::nrec): ADMM iteration t + 1
// meets most of iteration t's tree nodes again (same region prefix and depth, so the same Hessian
// for the same hinge states -- only the linear term and the row bounds move with y, z), and a
// node's QP can then start from the equality-constrained optimum on its previous active set with
// its previous factors (hvp_coop.h warm_start) instead of a Cholesky and ~10 active-set steps.
// One direct-mapped table of `nslots` records per (instance, depth); slot = hash of the code.  The
// children of a level claim their slots when they are written (bnb_put_children): the largest
// priority wins, i.e. this solve's epoch first and then the smallest code, so among the nodes of
// one level that share a slot the same one owns it in every run (the answers do not depend on
// scheduling); only the owner reads and rewrites the record.  The root owns depth 0, and the
// dive / hint leaves of k_bnb_root_coop write depth N before any level-N claim exists.
__device__ inline int node_slot(uint64_t code, int nslots) {
    return (int)((code * 0x9E3779B97F4A7C15ull) >> 40) & (nslots - 1);
}
__device__ inline size_t node_index(const Workspace& ws, int inst, int depth, uint64_t code) {
    return ((size_t)inst * ws.ndepth + depth) * ws.nslots + node_slot(code, ws.nslots);
}
__device__ inline unsigned long long node_prio(const Workspace& ws, uint64_t code) {
    return ws.nepoch | (~code & 0xFFFFFFFFFFFFull);  // codes of N <= 12 steps fit 48 bits
}

// writes the children (regions in mask) of a level-(lv-1) node into level lv's list at slots
// off.. (reserved by the caller) below `limit` (the end of the reservation's bucket segment,
// LevelList).  A reservation past its segment spills: the lane reserves its nc slots again in
// each other bucket in turn (one atomic each; rare) and writes the children into the first
// segment that holds them -- the bucket only orders the claims, so the tree is unchanged.  Only
// when no segment has room is the instance flagged HVP_OVERFLOW (reported, never truncated).
// The slots of a failed reservation below its segment's end are marked dead (-1), which the
// next kernels sweep.
// CLAIM: the 16-lane path's k_bnb_expand, the only writer whose levels can have node records
// pass >= 0 (the decentralised lane path's fused levels, a parent whose QP succeeded, lv < N): a
// single child whose region's band holds the parent's whole interval of v_{lv-1} has the parent's
// QP (kPassFlag below) and is written as a pass-through node carrying `pass` (the parent's active-set
// steps, its children's bucket).  Returns 1 when it wrote one.
constexpr uint64_t kPassFlag = 1ull << 63;  // codes of N <= 8 steps use 32 bits
constexpr uint64_t kPassCode = (1ull << 56) - 1;
template <bool CLAIM = false>
__device__ inline int bnb_put_children(const Workspace& ws, int lv, unsigned long long off, unsigned long long limit,
                                        unsigned mask, int inst, const hvp_system& S, const hvp::Consts& C,
                                        uint64_t code, double lo, double hi, double plb, int pass = -1) {
    const int nc = __popc(mask), d = lv & 1;
    if (off + nc > limit) {
        for (unsigned long long t = off; t < limit && t < off + nc; ++t) ws.nd_inst[d][t] = -1;
        // (dead slots are listed and are no nodes: counter[0], free in the branch and bound, takes
        // them out of hvp_stats.n_candidates)
        if (off < limit) atomicAdd(&ws.counter[0], limit - off);
        bool placed = false;
        if (ws.split > 1) {
            const unsigned long long cap = (unsigned long long)ws.cap, seg = cap >> ws.split_shift;
            for (int j = 0; j < ws.split && !placed; ++j) {
                const unsigned long long base = (unsigned long long)j * seg,
                                         end = j + 1 < ws.split ? base + seg : cap;
                if (end == limit) continue;  // the bucket that is full
                const unsigned long long o = base + atomicAdd(bucket_count(ws, j, lv), (unsigned long long)nc);
                if (o + nc <= end) {
                    off = o;
                    placed = true;
                    atomicAdd(&ws.counter[5], 1ull);  // hvp_stats.n_spilled
                } else {
                    for (unsigned long long t = o; t < end; ++t) ws.nd_inst[d][t] = -1;
                    if (o < end) atomicAdd(&ws.counter[0], end - o);
                }
            }
        }
        if (!placed) {
            atomicOr(&ws.inst_flag[inst], 2);
            return 0;
        }
    }
    int j = 0, passed = 0;
    for (int r = 0; r < S.n_regions; ++r) {
        if (!((mask >> r) & 1u)) continue;
        double a, b;
        hvp::bnb_child(S, C, lv - 1, lo, hi, r, &a, &b);
        uint64_t cc = hvp::code_with(code, lv - 1, r);
        if (ws.pass && pass >= 0 && nc == 1 && lo >= S.vlo[r] && hi <= S.vhi[r]) {
            cc |= kPassFlag | ((uint64_t)(pass < 127 ? pass : 127) << 56);
            passed = 1;
        }
        ws.nd_inst[d][off + j] = inst;
        ws.nd_code[d][off + j] = cc;
        if (CLAIM && ws.nclaim) atomicMax(&ws.nclaim[node_index(ws, inst, lv, cc)], node_prio(ws, cc));
        ws.nd_lo[d][off + j] = a;
        ws.nd_hi[d][off + j] = b;
        ws.nd_lb[d][off + j] = plb;  // inherited: kept by a leaf whose QP fails (a pass-through node's bound)
        ++j;
    }
    return passed;
}

// wave-level reservation of nc slots per lane in level lv's list (an inclusive scan, one atomic
// by the last lane); every lane of the wave must call it.  Returns the lane's first slot.
__device__ inline unsigned long long wave_reserve(unsigned long long* counter, int nc, int lane, bool& any) {
    int incl = nc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    const int wave_total = __shfl(incl, 63, 64);
    any = wave_total != 0;
    unsigned long long base = 0;
    if (lane == 63 && wave_total) base = atomicAdd(counter, (unsigned long long)wave_total);
    base = ((unsigned long long)(unsigned)__shfl((int)(base >> 32), 63, 64) << 32) |
           (unsigned)__shfl((int)(base & 0xffffffffu), 63, 64);
    return base + (unsigned long long)(incl - nc);
}

// Level lists of the decentralised lane path (k_bnb_root, k_bnb_bound_refill; Workspace::split)
// are kept in `split` equal segments of the capacity (buckets), by the active-set step count of
// the parent's QP: 2 buckets split at 6 steps, 4 buckets at 4 / 6 / 8.  A child's step count
// follows its parent's (correlation 0.84 at C2, profiles/diag_dualstop.cpp), and the refill
// kernel claims bucket 0 before bucket 1 and so on, so its 64-node generations -- as long as
// their slowest lane -- hold QPs of similar length.  The order of a level's nodes changes nothing
// else: the incumbent only moves at the leaves, where the tie rule is order-free.  Every other
// path keeps one list over the whole capacity (split = 1: slot(c) = c).
constexpr int kMaxBuckets = 4;
#ifndef HVP_BUCKETS
#define HVP_BUCKETS 2
#endif
constexpr int kDefaultBuckets = HVP_BUCKETS;
constexpr int kLvlM = HVP_MAX_N + 1;  // ws.lvl: [0, M) bucket-0 counts, [M, 2M) claims, [(1 + b) M, (2 + b) M) bucket b
__device__ inline int bucket_of(int nb, int steps) {
    return nb == 2 ? (steps >= 6 ? 1 : 0) : (nb == 4 ? (steps >= 4) + (steps >= 6) + (steps >= 8) : 0);
}
__device__ inline unsigned long long* bucket_count(const Workspace& ws, int b, int k) {
    return b == 0 ? &ws.lvl[k] : &ws.lvl[(1 + b) * kLvlM + k];
}

struct LevelList {
    unsigned long long n[kMaxBuckets];  // nodes per bucket (clamped to the segment)
    unsigned long long seg;             // segment size, cap / split
    int nb;
    // (loops over the static kMaxBuckets: a runtime-indexed n[] would live in scratch)
    __device__ long long count() const {
        unsigned long long c = 0;
#pragma unroll
        for (int b = 0; b < kMaxBuckets; ++b) c += n[b];  // n[b] = 0 for b >= nb
        return (long long)c;
    }
    __device__ long long slot(long long c) const {
        long long t = c, base = 0;
        bool found = false;
#pragma unroll
        for (int b = 0; b < kMaxBuckets; ++b) {
            const bool here = !found && (b + 1 >= nb || c < (long long)n[b]);
            t = here ? base + c : t;
            found = found || here;
            c -= (long long)n[b];
            base += (long long)seg;
        }
        return t;
    }
};
__device__ inline LevelList level_list(const Workspace& ws, int k) {
    LevelList L;
    // (level 0, the roots, is one list whatever the split: k_inst_prep writes it in instance order)
    L.nb = ws.split > 1 && k > 0 ? ws.split : 1;
    L.seg = k > 0 ? (unsigned long long)ws.cap >> ws.split_shift : (unsigned long long)ws.cap;
#pragma unroll
    for (int b = 0; b < kMaxBuckets; ++b) {
        const unsigned long long v = b < L.nb ? *bucket_count(ws, b, k) : 0ull;
        const unsigned long long lim = b + 1 < L.nb ? L.seg : (unsigned long long)ws.cap - (L.nb - 1) * L.seg;
        L.n[b] = v < lim ? v : lim;
    }
    return L;
}

// wave-level reservation of nc slots per lane of level lv in the bucket of the lane's parent
// (its QP took `steps` active-set steps): one packed scan of the per-bucket counts, one atomic per
// non-empty bucket by the last lane.  Returns the lane's first slot and the end of its segment.
__device__ inline unsigned long long split_reserve(const Workspace& ws, int lv, int nc, int steps, int lane,
                                                   unsigned long long& limit) {
    const unsigned long long cap = (unsigned long long)ws.cap;
    if (ws.split <= 1) {
        bool any;
        limit = cap;
        return wave_reserve(&ws.lvl[lv], nc, lane, any);
    }
    const int nb = ws.split;
    const unsigned long long seg = cap >> ws.split_shift;
    const int b = bucket_of(nb, steps);
    unsigned long long incl = (unsigned long long)nc << (16 * b);  // <= 64 lanes x 16 children per field
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long v = ((unsigned long long)(unsigned)__shfl_up((int)(incl >> 32), off, 64) << 32) |
                                     (unsigned)__shfl_up((int)(incl & 0xffffffffu), off, 64);
        if (lane >= off) incl += v;
    }
    unsigned long long base[kMaxBuckets] = {0ull, 0ull, 0ull, 0ull};
    if (lane == 63) {
#pragma unroll
        for (int j = 0; j < kMaxBuckets; ++j) {
            const unsigned long long tot = (incl >> (16 * j)) & 0xffffull;
            if (j < nb && tot) base[j] = atomicAdd(bucket_count(ws, j, lv), tot);
        }
    }
    unsigned long long mine = 0;
#pragma unroll
    for (int j = 0; j < kMaxBuckets; ++j) {
        const unsigned long long bj = ((unsigned long long)(unsigned)__shfl((int)(base[j] >> 32), 63, 64) << 32) |
                                      (unsigned)__shfl((int)(base[j] & 0xffffffffu), 63, 64);
        mine = j == b ? bj : mine;
    }
    limit = b + 1 < nb ? (b + 1) * seg : cap;
    return (unsigned long long)b * seg + mine + ((incl >> (16 * b)) & 0xffffull) - (unsigned long long)nc;
}

// The region sequence of hvp_set_region_hint for instance i as a leaf code, if every step is a
// region of the table reachable from the previous step's interval (a stale or uninitialised hint
// is simply not used).  Its leaf QP only tightens the initial incumbent: the prune margin
// (1e-7 relative) is wider than the tie window (1e-9), so every leaf that can win is still
// reached by the search and the answer does not depend on the hint.
template <int N>
__device__ inline bool hint_code(const Workspace& ws, int i, const hvp_system& S, const hvp::Consts& C, double v0,
                                 uint64_t* code_out) {
    double lo = v0, hi = v0;
    uint64_t code = 0;
    for (int k = 0; k < N; ++k) {
        const int r = ws.hint[(size_t)i * N + k];
        double nlo, nhi;
        if (r < 0 || r >= S.n_regions || !hvp::bnb_child(S, C, k, lo, hi, r, &nlo, &nhi)) return false;
        code = hvp::code_with(code, k, r);
        lo = nlo;
        hi = nhi;
    }
    *code_out = code;
    return true;
}

template <int N, bool ADMM>
__global__ __launch_bounds__(kBnbBlock<N>) HVP_LANE_OCC void k_bnb_root(int B, const hvp_system* __restrict__ systems,
                                                           const int32_t* __restrict__ sys,
                                                           const int32_t* __restrict__ role,
                                                           const double* __restrict__ params, hvp::Consts C,
                                                           Workspace ws) {
    constexpr int BS = kBnbBlock<N>;
    const int i = blockIdx.x * BS + threadIdx.x;
    if (i == 0) ws.lvl[0] = (unsigned long long)B;
    if (i >= B) return;
    const hvp_system& S = systems[sys[i]];
    const int rl = role[i];
    const double* prm = params + (size_t)i * C.stride;
    const double v0 = prm[1], P1 = prm[0] + S.ts * v0;
    const bool ok = P1 >= S.pmin - 1e-9 * (1.0 + fabs(S.pmin)) && P1 <= S.pmax + 1e-9 * (1.0 + fabs(S.pmax));
    ws.key[i] = ~0ull;
    ws.inst_flag[i] = ok ? 0 : 1;
    ws.nd_inst[0][i] = ok ? i : -1;
    ws.nd_code[0][i] = 0;
    ws.nd_lo[0][i] = v0;
    ws.nd_hi[0][i] = v0;
    double inc = __longlong_as_double(0x7ff0000000000000ll);  // +inf: no incumbent
    double lb = -1e300;
    int nodes = 0, iters = 0, root_steps = 0;
    if (ok) {
        hvp::LaneQp<N, LdsMem<N, BS>> q;
        q.mem.lane = threadIdx.x;
        double c0;
        int it = bnb_qp<N, BS, ADMM>(q, S, C, rl, prm, 0, 0, v0, v0, c0);
        ++nodes;
        iters += it >= 0 ? it : -1 - it;
        root_steps = it;
        if (it >= 0) {
            lb = c0;
            double ystar[N];
#pragma unroll
            for (int k = 0; k < N; ++k) ystar[k] = q.y[k];
            uint64_t code;
            const bool dived = hvp::bnb_dive<N>(S, C, v0, ystar, &code);
            if (dived) {
                double c1;
                it = bnb_qp<N, BS, ADMM>(q, S, C, rl, prm, code, N, 0.0, -1.0, c1);
                ++nodes;
                iters += it >= 0 ? it : -1 - it;
                if (it >= 0) inc = c1;
            }
            if constexpr (ADMM) {  // the previous ADMM iteration's sequence as a second incumbent
                uint64_t hc;
                if (ws.hint && hint_code<N>(ws, i, S, C, v0, &hc) && !(dived && hc == code)) {
                    double c2;
                    it = bnb_qp<N, BS, ADMM>(q, S, C, rl, prm, hc, N, 0.0, -1.0, c2);
                    ++nodes;
                    iters += it >= 0 ? it : -1 - it;
                    if (it >= 0 && !(c2 >= inc)) inc = c2;
                }
            }
        }
    }
    ws.nd_lb[0][i] = lb;
    ws.inc[i] = cost_key(inc);
    ws.nodes[i] = nodes;
    ws.iters[i] = iters;
    atomicAdd(&ws.counter[3], (unsigned long long)nodes);
    atomicAdd(&ws.counter[1], (unsigned long long)iters);
    if constexpr (!ADMM) {
        // the level-1 nodes (k_bnb_expand's work, fused): the incumbent only changes at the
        // leaves (level N), so the pruning test here sees the value the expand kernel would
        if (ok && !hvp::bnb_pruned(lb, inc)) {
            const unsigned mask = bnb_children(S, C, 0, v0, v0);
            if (mask) {
                // the root's children all go to bucket 0 (LevelList; level 1 is the smallest level,
                // and a bucket choice here measured 3x slower in this kernel: r03v)
                const unsigned long long off = atomicAdd(&ws.lvl[1], (unsigned long long)__popc(mask));
                // (a pass-through child when it has the root's QP: k_bnb_bound_refill)
                if (bnb_put_children(ws, 1, off, (unsigned long long)ws.cap >> ws.split_shift, mask, i, S, C, 0, v0,
                                     v0, lb, 1 < N && lb > -1e300 ? root_steps : -1))
                    atomicAdd(&ws.counter[6], 1ull);
            }
        }
    }
}

// ---- long horizons: one QP per 16-lane group (hvp_coop.h), 4 groups per 64-lane block
// (HVP_COOP_MIN_N: the shortest horizon on the 16-lane path; an A/B build with -DHVP_COOP_MIN_N=5
// runs configs[1] there)
#ifndef HVP_COOP_MIN_N
#define HVP_COOP_MIN_N (HVP_MAX_N_ENUM + 1)
#endif
template <int N>
constexpr bool kCoop = N >= HVP_COOP_MIN_N;
constexpr int kCoopBlock = 64;
// waves per SIMD of the 16-lane group kernels (A/B builds: -DHVP_COOP_WAVES=2 caps them at 256 VGPRs)
#ifdef HVP_COOP_WAVES
#define HVP_COOP_OCC __attribute__((amdgpu_waves_per_eu(HVP_COOP_WAVES)))
#else
#define HVP_COOP_OCC
#endif
constexpr int kCoopGroups = kCoopBlock / hvp::coop::G;

template <int N>
__global__ __launch_bounds__(kCoopBlock) HVP_COOP_OCC void k_bnb_root_coop(int B, const hvp_system* __restrict__ systems,
                                                              const int32_t* __restrict__ sys,
                                                              const int32_t* __restrict__ role,
                                                              const double* __restrict__ params, hvp::Consts C,
                                                              Workspace ws, int leaf_list) {
    __shared__ hvp::coop::GroupLds lds[kCoopGroups];
    const int g = threadIdx.x / hvp::coop::G, t = threadIdx.x % hvp::coop::G;
    const int i = blockIdx.x * kCoopGroups + g;
    if (blockIdx.x == 0 && threadIdx.x == 0) ws.lvl[0] = (unsigned long long)B;
    if (i >= B) return;  // group-uniform
    const hvp_system& S = systems[sys[i]];
    const int rl = role[i];
    const double* prm = params + (size_t)i * C.stride;
    const double v0 = prm[1], P1 = prm[0] + S.ts * v0;
    const bool ok = P1 >= S.pmin - 1e-9 * (1.0 + fabs(S.pmin)) && P1 <= S.pmax + 1e-9 * (1.0 + fabs(S.pmax));
    double inc = __longlong_as_double(0x7ff0000000000000ll);
    double lb = -1e300;
    int nodes = 0, iters = 0;
    if (ok) {
        hvp::coop::Lane<N> L;
        double c0 = 0.0;
        int it = 0;
        // naive-ADMM node records (node_index): the root owns depth 0, the dive / hint leaves write
        // depth N before the level-N claims
        using Rec = hvp::coop::WarmRec<N>;
        Rec* recs = reinterpret_cast<Rec*>(ws.nrec);
        const uint64_t wkey = ((uint64_t)(uint32_t)sys[i] << 32) | (uint32_t)rl;
        Rec* w0 = ws.nclaim ? recs + node_index(ws, i, 0, 0) : nullptr;
        int st = hvp::coop::solve_qp<N, Rec>(L, lds[g], S, C, rl, prm, 0, 0, kGiMaxIter<N>, it, &c0, nullptr, prm[1],
                                             prm[1], w0, w0 != nullptr, wkey);
        ++nodes;
        iters += it;
        if (st == hvp::GI_OK) {
            lb = c0;
            lds[g].v[t] = t < N ? L.y : 0.0;
            hvp::coop::gsync();
            unsigned long long code = 0;
            int dive_ok = 0;
            if (t == 0) {
                double ystar[N];
#pragma unroll
                for (int k = 0; k < N; ++k) ystar[k] = lds[g].v[k];
                uint64_t c64;
                dive_ok = hvp::bnb_dive<N>(S, C, v0, ystar, &c64) ? 1 : 0;
                code = c64;
            }
            dive_ok = hvp::coop::bcast(dive_ok, 0);
            code = hvp::coop::bcast(code, 0);
            if (leaf_list) {
                // the incumbent leaves (the dive's, the hint's) as a list of their own, solved by
                // k_bnb_leaf_coop: here every group solves exactly one QP, its root
                if (t == 0) {
                    uint64_t hc = 0;
                    const int hok = ws.hint && hint_code<N>(ws, i, S, C, v0, &hc) && (!dive_ok || hc != code) ? 1 : 0;
                    if (dive_ok + hok) {
                        const unsigned long long o = atomicAdd(&ws.counter[7], (unsigned long long)(dive_ok + hok));
                        if (dive_ok) {
                            ws.nd_inst[1][o] = i;
                            ws.nd_code[1][o] = code;
                            ws.nd_lo[1][o] = 0.0;
                        }
                        if (hok) {
                            ws.nd_inst[1][o + dive_ok] = i;
                            ws.nd_code[1][o + dive_ok] = hc;
                            // one writer per record: a hint whose slot is the dive's solves without it
                            ws.nd_lo[1][o + dive_ok] =
                                dive_ok && ws.nclaim && node_slot(hc, ws.nslots) == node_slot(code, ws.nslots) ? 1.0 : 0.0;
                        }
                    }
                }
            } else if (dive_ok) {
                double c1 = 0.0;
                Rec* w1 = ws.nclaim ? recs + node_index(ws, i, N, code) : nullptr;
                st = hvp::coop::solve_qp<N, Rec>(L, lds[g], S, C, rl, prm, code, N, kGiMaxIter<N>, it, &c1, nullptr,
                                                 0.0, -1.0, w1, w1 != nullptr, wkey);
                ++nodes;
                iters += it;
                if (st == hvp::GI_OK) inc = c1;
            }
            if (!leaf_list && ws.hint) {  // see hint_code (set for the ADMM and decentralised forms only)
                unsigned long long hc = 0;
                int hok = 0;
                if (t == 0) {
                    uint64_t c64;
                    hok = hint_code<N>(ws, i, S, C, v0, &c64) && (!dive_ok || c64 != code) ? 1 : 0;
                    hc = c64;
                }
                hok = hvp::coop::bcast(hok, 0);
                hc = hvp::coop::bcast(hc, 0);
                if (hok) {
                    double c2 = 0.0;
                    Rec* w2 = ws.nclaim ? recs + node_index(ws, i, N, hc) : nullptr;
                    st = hvp::coop::solve_qp<N, Rec>(L, lds[g], S, C, rl, prm, hc, N, kGiMaxIter<N>, it, &c2, nullptr,
                                                     0.0, -1.0, w2, w2 != nullptr, wkey);
                    ++nodes;
                    iters += it;
                    if (st == hvp::GI_OK && !(c2 >= inc)) inc = c2;
                }
            }
        }
    }
    if (t == 0) {
        ws.key[i] = ~0ull;
        ws.inst_flag[i] = ok ? 0 : 1;
        ws.nd_inst[0][i] = ok ? i : -1;
        ws.nd_code[0][i] = 0;
        ws.nd_lo[0][i] = v0;
        ws.nd_hi[0][i] = v0;
        ws.nd_lb[0][i] = lb;
        ws.inc[i] = cost_key(inc);
        ws.nodes[i] = nodes;
        ws.iters[i] = iters;
        atomicAdd(&ws.counter[3], (unsigned long long)nodes);
        atomicAdd(&ws.counter[1], (unsigned long long)iters);
    }
}

// The incumbent leaves of k_bnb_root_coop's list (leaf_list): the greedy dive's sequence and the hint's
// (the previous ADMM iteration's / time step's winner), one QP per 16-lane group, grid-stride over
// the list.  Run inline after each root (round 5) a group solved one to three QPs while the other
// three groups of its wave waited for the longest chain (lane utilisation 0.26).  Same
// QPs, same node records (a leaf owns its depth-N slot; a hint that shares the dive's slot solves
// cold), same incumbents (atomicMin of the leaves' costs).  The list lives in level 1's node arrays,
// which k_bnb_expand fills only afterwards; its length is counter[7].
template <int N>
__global__ __launch_bounds__(kCoopBlock) HVP_COOP_OCC void k_bnb_leaf_coop(const hvp_system* __restrict__ systems,
                                                              const int32_t* __restrict__ sys,
                                                              const int32_t* __restrict__ role,
                                                              const double* __restrict__ params, hvp::Consts C,
                                                              Workspace ws) {
    __shared__ hvp::coop::GroupLds lds[kCoopGroups];
    const int g = threadIdx.x / hvp::coop::G, t = threadIdx.x % hvp::coop::G;
    const long long total = (long long)ws.counter[7];
    using Rec = hvp::coop::WarmRec<N>;
    for (long long q = (long long)blockIdx.x * kCoopGroups + g; q < total; q += (long long)gridDim.x * kCoopGroups) {
        const int inst = ws.nd_inst[1][q];
        const uint64_t code = ws.nd_code[1][q];
        const hvp_system& S = systems[sys[inst]];
        const int rl = role[inst];
        const double* prm = params + (size_t)inst * C.stride;
        Rec* w = ws.nclaim && ws.nd_lo[1][q] == 0.0 ? reinterpret_cast<Rec*>(ws.nrec) + node_index(ws, inst, N, code)
                                                   : nullptr;
        hvp::coop::Lane<N> L;
        double c = 0.0;
        int it = 0;
        const int st = hvp::coop::solve_qp<N, Rec>(L, lds[g], S, C, rl, prm, code, N, kGiMaxIter<N>, it, &c, nullptr, 0.0,
                                                   -1.0, w, w != nullptr,
                                                   ((uint64_t)(uint32_t)sys[inst] << 32) | (uint32_t)rl);
        if (t == 0) {
            atomicAdd(&ws.nodes[inst], 1);
            atomicAdd(&ws.iters[inst], it);
            atomicAdd(&ws.counter[3], 1ull);
            atomicAdd(&ws.counter[1], (unsigned long long)it);
            if (st == hvp::GI_OK) atomicMin(&ws.inc[inst], cost_key(c));
        }
    }
}

template <int N>
__global__ __launch_bounds__(kCoopBlock) HVP_COOP_OCC void k_bnb_bound_coop(int k, const hvp_system* __restrict__ systems,
                                                               const int32_t* __restrict__ sys,
                                                               const int32_t* __restrict__ role,
                                                               const double* __restrict__ params, hvp::Consts C,
                                                               Workspace ws) {
    __shared__ hvp::coop::GroupLds lds[kCoopGroups];
    const int g = threadIdx.x / hvp::coop::G, t = threadIdx.x % hvp::coop::G;
    const int dst = k & 1;
    const unsigned long long nn = ws.lvl[k];
    const long long total = (long long)(nn < (unsigned long long)ws.cap ? nn : ws.cap);
    for (long long q0 = (long long)blockIdx.x * kCoopGroups + g; q0 < total; q0 += (long long)gridDim.x * kCoopGroups) {
        // with node records, the level in k_node_order's order: the warm-started nodes first, so
        // the 4 groups of a wave mostly hold QPs of one kind (a wave lasts as long as its slowest)
        const long long q = ws.norder ? (long long)ws.task_inst[q0] : q0;
        const int inst = ws.nd_inst[dst][q];
        if (inst < 0) {
            if (t == 0) {
                if (k == N) ws.leaf_stat[q] = HVP_OVERFLOW;
                else ws.nd_lb[dst][q] = 1e300;
            }
            continue;
        }
        const uint64_t code = ws.nd_code[dst][q];
        const hvp_system& S = systems[sys[inst]];
        const int rl = role[inst];
        const double* prm = params + (size_t)inst * C.stride;
        hvp::coop::Lane<N> L;
        double c = 0.0;
        int it = 0;
        const int cap = k == N && C.leaf_cap > 0 ? C.leaf_cap : kGiMaxIter<N>;
        using Rec = hvp::coop::WarmRec<N>;
        Rec* wq = nullptr;  // the node's record, when it owns the slot (node_index)
        if (ws.nclaim) {
            const size_t ni = node_index(ws, inst, k, code);
            if (ws.nclaim[ni] == node_prio(ws, code)) wq = reinterpret_cast<Rec*>(ws.nrec) + ni;
        }
        const int st = hvp::coop::solve_qp<N, Rec>(L, lds[g], S, C, rl, prm, code, k, cap, it, &c, nullptr,
                                                   ws.nd_lo[dst][q], ws.nd_hi[dst][q], wq, wq != nullptr,
                                                   ((uint64_t)(uint32_t)sys[inst] << 32) | (uint32_t)rl);
        const bool ok = st == hvp::GI_OK;
        if (k == N && t < N) ws.task_y[q * N + t] = L.y;
        if (t == 0) {
            atomicAdd(&ws.nodes[inst], 1);
            atomicAdd(&ws.iters[inst], it);
            atomicAdd(&ws.counter[1], (unsigned long long)it);
            if (k < N) {
                ws.nd_lb[dst][q] = ok ? c : -1e300;
                if (!ok) atomicAdd(&ws.counter[4], 1ull);
            } else {
                if (ok) ws.nd_lb[dst][q] = c;
                ws.leaf_stat[q] = ok ? 0 : HVP_MAXITER;
                if (ok) {
                    atomicMin(&ws.inc[inst], cost_key(c));
                } else {
                    atomicOr(&ws.inst_flag[inst], 8);
                    if (C.form == HVP_FORM_DECENT || C.form == HVP_FORM_ADMM) {  // K_bnb_ipm re-solves it
                        const unsigned long long r = atomicAdd(&ws.counter[2], 1ull);
                        if (r < (unsigned long long)ws.cap) ws.redo[r] = (int32_t)q;
                    }
                }
            }
        }
    }
}

// children of the level-(k-1) nodes that survive the incumbent test.
// The level's node list is shared by the whole batch: a heavy tree (trajectories riding a region
// boundary, naive-ADMM hinge states) uses the room the light ones leave (a per-instance share of
// capacity / B made 68 of 80 naive-ADMM solves at C3 re-run).  An instance whose children do not
// fit is reported HVP_OVERFLOW, never truncated silently, and re-solved alone by the caller
// (solve_device(retry_overflow)).  One thread per parent; the slots are reserved per WAVE (an
// inclusive scan of the children counts, one atomic by the last lane): a per-thread atomic on the
// level counter serialised ~1e5 atomics on one address per level (0.076 ms per launch at C2).
template <int N>
__global__ __launch_bounds__(kBlock) void k_bnb_expand(int k, const hvp_system* __restrict__ systems,
                                                       const int32_t* __restrict__ sys, hvp::Consts C, Workspace ws) {
    const int src = (k - 1) & 1;
    const unsigned long long np = ws.lvl[k - 1];
    const long long total = (long long)(np < (unsigned long long)ws.cap ? np : ws.cap);
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long pw = wave0; pw < total; pw += stride) {  // wave-uniform loop
        const long long p = pw + lane;
        int inst = -1;
        unsigned mask = 0;
        double lo = 0.0, hi = 0.0, plb = 0.0;
        uint64_t code = 0;
        if (p < total) {
            inst = ws.nd_inst[src][p];
            if (inst >= 0 && !(ws.inst_flag[inst] & 2)) {
                plb = ws.nd_lb[src][p];
                if (!hvp::bnb_pruned(plb, inc_of(ws, inst))) {
                    lo = ws.nd_lo[src][p];
                    hi = ws.nd_hi[src][p];
                    code = ws.nd_code[src][p];
                    mask = bnb_children(systems[sys[inst]], C, k - 1, lo, hi);
                }
            }
        }
        bool any;
        const unsigned long long off = wave_reserve(&ws.lvl[k], __popc(mask), lane, any);
        if (!any || !mask) continue;
        bnb_put_children<kCoop<N>>(ws, k, off, (unsigned long long)ws.cap, mask, inst, systems[sys[inst]], C, code, lo,
                                   hi, plb);
    }
}

// one lane per level-k node: bound (k < N) or exact leaf QP (k = N)
template <int N, bool ADMM>
__global__ __launch_bounds__(kBnbBlock<N>) HVP_LANE_OCC void k_bnb_bound(int k, const hvp_system* __restrict__ systems,
                                                            const int32_t* __restrict__ sys,
                                                            const int32_t* __restrict__ role,
                                                            const double* __restrict__ params, hvp::Consts C,
                                                            Workspace ws) {
    constexpr int BS = kBnbBlock<N>;
    const int dst = k & 1;
    const unsigned long long nn = ws.lvl[k];
    const long long total = (long long)(nn < (unsigned long long)ws.cap ? nn : ws.cap);
    unsigned long long iter_sum = 0, fails = 0;
    for (long long t = (long long)blockIdx.x * BS + threadIdx.x; t < total; t += (long long)gridDim.x * BS) {
        const int inst = ws.nd_inst[dst][t];
        if (inst < 0) {  // dead slot of an overflowed reservation
            if (k == N) ws.leaf_stat[t] = HVP_OVERFLOW;
            else ws.nd_lb[dst][t] = 1e300;
            continue;
        }
        const uint64_t code = ws.nd_code[dst][t];
        const hvp_system& S = systems[sys[inst]];
        const int rl = role[inst];
        const double* prm = params + (size_t)inst * C.stride;
        hvp::LaneQp<N, LdsMem<N, BS>> q;
        q.mem.lane = threadIdx.x;
        double c;
        // HVP_LEAF_GI_CAP (tests): the ADMM leaves' active-set cap, to send them through K_bnb_ipm
        const int cap = ADMM && k == N && C.leaf_cap > 0 ? C.leaf_cap : kGiMaxIter<N>;
        const int it = bnb_qp<N, BS, ADMM>(q, S, C, rl, prm, code, k, ws.nd_lo[dst][t], ws.nd_hi[dst][t], c, cap);
        const bool ok = it >= 0;
        const int its = ok ? it : -1 - it;
        iter_sum += (unsigned long long)its;
        atomicAdd(&ws.nodes[inst], 1);
        atomicAdd(&ws.iters[inst], its);
        if (k < N) {
            // a failed bound QP prunes nothing
            ws.nd_lb[dst][t] = ok ? c : -1e300;
            if (!ok) atomicAdd(&ws.counter[4], 1ull);
        } else {
            // a failed leaf keeps its parent's bound (K_key: MAXITER if it stays in contention
            // and no fallback exists)
            if (ok) ws.nd_lb[dst][t] = c;
            ws.leaf_stat[t] = ok ? 0 : HVP_MAXITER;
#pragma unroll
            for (int j = 0; j < N; ++j) ws.task_y[t * N + j] = q.y[j];
            if (ok) {
                atomicMin(&ws.inc[inst], cost_key(c));
            } else {
                ++fails;
                atomicOr(&ws.inst_flag[inst], 8);  // a velocity-feasible sequence exists
                if (C.form == HVP_FORM_DECENT || C.form == HVP_FORM_ADMM) {  // K_bnb_ipm re-solves it
                    const unsigned long long r = atomicAdd(&ws.counter[2], 1ull);
                    if (r < (unsigned long long)ws.cap) ws.redo[r] = (int32_t)t;
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) iter_sum += __shfl_down(iter_sum, off, 64);
    if ((threadIdx.x & 63) == 0 && iter_sum) atomicAdd(&ws.counter[1], iter_sum);
    (void)fails;
}

// ---- min_1_norm (the MILP, hvp_l1.h): the same level-synchronous search with the node LPs solved
// one per WAVEFRONT (l1_node_lp).  Root: the fully relaxed LP (K = 0) gives the root bound and the
// greedy dive's target velocities; the dive's leaf LP (and the hinted sequence's, if any) the
// initial incumbent.  Node statuses: an LP proven infeasible prunes its subtree (bound +inf) or
// drops its leaf; an unresolved LP prunes nothing (bound -inf) and, at a leaf still in contention,
// makes the instance HVP_MAXITER (k_bnb_key).  Children: k_bnb_expand per level.
// 2 waves per SIMD up to N = 8 (the wave solver fits 256 registers; at 1 wave the LP rate halves)
// (the naive-ADMM form's copy groups need the registers of one wave per SIMD)
template <int N>
constexpr int kL1Waves = N <= HVP_MAX_N_ENUM ? 2 : 1;
template <int N, bool ADMM>
constexpr int kL1WavesOf = ADMM ? 1 : kL1Waves<N>;

// the node LP of either form (ADMM: the naive-ADMM min_1_norm local problem, l1_admm_node_lp)
template <int N, bool ADMM>
__device__ inline int l1_any_node_lp(const hvp_system& S, const hvp::Consts& C, int rl, const double* prm,
                                     uint64_t code, int K, double rlo, double rhi, double* y, double& cost, int& iters,
                                     double* red, int lane) {
    if constexpr (ADMM) return l1_admm_node_lp<N>(S, C, rl, prm, code, K, rlo, rhi, y, cost, iters, red, lane);
    else return l1_node_lp<N>(S, C, rl, prm, code, K, rlo, rhi, y, cost, iters, red, lane);
}

template <int N, bool ADMM>
__global__ __launch_bounds__((kL1BlockOfA<N, ADMM>)) __attribute__((amdgpu_waves_per_eu(kL1WavesOf<N, ADMM>))) void k_l1_root(int B, const hvp_system* __restrict__ systems,
                                                           const int32_t* __restrict__ sys,
                                                           const int32_t* __restrict__ role,
                                                           const double* __restrict__ params, hvp::Consts C,
                                                           Workspace ws) {
    __shared__ double s_red[kL1BlockOfA<N, ADMM> / 64][ADMM ? 1 : kL1LdsAll<N, ADMM>];
    double* red = ADMM ? g_l1_admm_lds<N> : s_red[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) ws.lvl[0] = (unsigned long long)B;
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < B; i += nwaves) {
        const hvp_system& S = systems[sys[i]];
        const int rl = role[i];
        const double* prm = params + (size_t)i * C.stride;
        const double v0 = prm[1], P1 = prm[0] + S.ts * v0;
        const bool ok = P1 >= S.pmin - 1e-9 * (1.0 + fabs(S.pmin)) && P1 <= S.pmax + 1e-9 * (1.0 + fabs(S.pmax));
        double inc = __longlong_as_double(0x7ff0000000000000ll);  // +inf: no incumbent
        double lb = -1e300;
        int nodes = 0, iters = 0;
        // up to three LPs with ONE call site (the LP body is inlined once): 0 the root relaxation,
        // 1 the greedy dive's leaf, 2 the hinted sequence's leaf
        uint64_t code = 0, dive_code = 0;
        int job = ok ? 0 : 3, K = 0;
        double rlo = v0, rhi = v0;
        bool dived = false;
        while (job < 3) {
            double y[N], c = 0.0;
            int it = 0;
            const int st = l1_any_node_lp<N, ADMM>(S, C, rl, prm, code, K, rlo, rhi, y, c, it, red, lane);
            ++nodes;
            iters += it;
            int next = 3;
            if (job == 0) {
                if (st == hvp::L1_INFEASIBLE) lb = 1e300;  // no completion is feasible
                if (st == hvp::L1_OK) {
                    lb = c;
                    dived = hvp::bnb_dive<N>(S, C, v0, y, &dive_code);
                    next = dived ? 1 : 2;
                }
            } else {
                if (st == hvp::L1_OK && !(c >= inc)) inc = c;
                next = job + 1;
            }
            if (next == 1) code = dive_code;
            if (next == 2) {
                uint64_t hc = 0;
                if (ws.hint && hint_code<N>(ws, (int)i, S, C, v0, &hc) && !(dived && hc == dive_code)) code = hc;
                else next = 3;
            }
            job = next;
            K = N;
            rlo = 0.0;
            rhi = -1.0;
        }
        if (lane == 0) {
            ws.key[i] = ~0ull;
            ws.inst_flag[i] = ok ? 0 : 1;
            ws.nd_inst[0][i] = ok ? (int)i : -1;
            ws.nd_code[0][i] = 0;
            ws.nd_lo[0][i] = v0;
            ws.nd_hi[0][i] = v0;
            ws.nd_lb[0][i] = lb;
            ws.inc[i] = cost_key(inc);
            ws.nodes[i] = nodes;
            ws.iters[i] = iters;
            atomicAdd(&ws.counter[3], (unsigned long long)nodes);
            atomicAdd(&ws.counter[1], (unsigned long long)iters);
        }
    }
}

template <int N, bool ADMM>
__global__ __launch_bounds__((kL1BlockOfA<N, ADMM>)) __attribute__((amdgpu_waves_per_eu(kL1WavesOf<N, ADMM>))) void k_l1_bound(int k, const hvp_system* __restrict__ systems,
                                                            const int32_t* __restrict__ sys,
                                                            const int32_t* __restrict__ role,
                                                            const double* __restrict__ params, hvp::Consts C,
                                                            Workspace ws) {
    __shared__ double s_red[kL1BlockOfA<N, ADMM> / 64][ADMM ? 1 : kL1LdsAll<N, ADMM>];
    double* red = ADMM ? g_l1_admm_lds<N> : s_red[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    const int dst = k & 1;
    const unsigned long long nn = ws.lvl[k];
    const long long total = (long long)(nn < (unsigned long long)ws.cap ? nn : ws.cap);
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    unsigned long long iter_sum = 0;
    for (long long t = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; t < total; t += nwaves) {
        const int inst = ws.nd_inst[dst][t];  // wave-uniform
        if (inst < 0) {                        // dead slot of an overflowed reservation
            if (lane == 0) {
                if (k == N) ws.leaf_stat[t] = HVP_OVERFLOW;
                else ws.nd_lb[dst][t] = 1e300;
            }
            continue;
        }
        const hvp_system& S = systems[sys[inst]];
        const double* prm = params + (size_t)inst * C.stride;
        double y[N], c = 0.0;
        int it = 0;
        const int st = l1_any_node_lp<N, ADMM>(S, C, role[inst], prm, ws.nd_code[dst][t], k, ws.nd_lo[dst][t],
                                               ws.nd_hi[dst][t], y, c, it, red, lane);
        iter_sum += (unsigned long long)it;
        if (lane != 0) continue;
        atomicAdd(&ws.nodes[inst], 1);
        atomicAdd(&ws.iters[inst], it);
        if (k < N) {
            // proven infeasible: the subtree holds no feasible completion; unresolved: prunes nothing
            ws.nd_lb[dst][t] = st == hvp::L1_OK ? c : (st == hvp::L1_INFEASIBLE ? 1e300 : -1e300);
            if (st == hvp::L1_FAIL) atomicAdd(&ws.counter[4], 1ull);
        } else {
            if (st == hvp::L1_OK) ws.nd_lb[dst][t] = c;  // an unresolved leaf keeps its parent's bound
            ws.leaf_stat[t] = st == hvp::L1_OK ? 0 : (st == hvp::L1_INFEASIBLE ? HVP_INFEASIBLE : HVP_MAXITER);
#pragma unroll
            for (int j = 0; j < N; ++j) ws.task_y[t * N + j] = y[j];
            if (st == hvp::L1_OK) atomicMin(&ws.inc[inst], cost_key(c));
            if (st == hvp::L1_FAIL) atomicOr(&ws.inst_flag[inst], 8);  // a sequence exists, unresolved
        }
    }
    if (lane == 0 && iter_sum) atomicAdd(&ws.counter[1], iter_sum);
}

// Second pass over level k of the decentralised min_1_norm search after k_l1_bound: the LPs the
// wave interior point left unresolved (L1_FAIL: at some degenerate optima -- active w = 1e4 safe
// hinges, a slow front and a fast back vehicle -- its complementarity gap collapses while the dual
// residual stays above the stop test, whatever the iteration cap) go to the per-lane simplex of
// hvp_lp.h, one LP per lane, the step data in the lane's own array.  They are rare (about one
// instance in 2,500 at n = 10, N = 10 holds any), so the kernel normally reads the level's
// statuses and ends; the wave kernels' registers and LDS are untouched.  Only a vertex the simplex
// certifies optimal resolves the node; anything else leaves it as k_l1_bound wrote it (an interior
// node prunes nothing, a leaf in contention makes the instance HVP_MAXITER).  Every unresolved LP
// of the level is tried, whatever the incumbent, so the LP counts do not depend on the scheduling.
// The host build runs the same pass (hvp_hostref.cpp solve_one_bnb).
constexpr int kL1RetryBlock = 64;
template <int N>
__global__ __launch_bounds__(kL1RetryBlock) void k_l1_retry(int k, const hvp_system* __restrict__ systems,
                                                            const int32_t* __restrict__ sys,
                                                            const int32_t* __restrict__ role,
                                                            const double* __restrict__ params, hvp::Consts C,
                                                            Workspace ws) {
    const int dst = k & 1;
    const unsigned long long nn = ws.lvl[k];
    const long long total = (long long)(nn < (unsigned long long)ws.cap ? nn : ws.cap);
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const int inst = ws.nd_inst[dst][t];
        if (inst < 0) continue;
        // k_l1_bound's marks of an unresolved LP (a solved node's bound is a finite cost)
        if (k < N ? ws.nd_lb[dst][t] != -1e300 : ws.leaf_stat[t] != HVP_MAXITER) continue;
        const hvp_system& S = systems[sys[inst]];
        const double* prm = params + (size_t)inst * C.stride;
        const uint64_t code = ws.nd_code[dst][t];
        const double rlo = ws.nd_lo[dst][t], rhi = ws.nd_hi[dst][t];
        hvp::LpData<N> D;
        double y[N];
        int it = 0;
        const int st = hvp::lp_solve_l1<N>(D, S, C, role[inst], prm, code, k, rlo, rhi, C.max_iter, y, it);
        atomicAdd(&ws.nodes[inst], 1);
        atomicAdd(&ws.iters[inst], it);
        atomicAdd(&ws.counter[3], 1ull);
        atomicAdd(&ws.counter[1], (unsigned long long)it);
        if (st != hvp::L1_OK) continue;
        const double c = hvp::l1_direct_cost<N>(y, S, C, role[inst], prm, code, k, rlo, rhi);
        ws.nd_lb[dst][t] = c;
        if (k == N) {
            ws.leaf_stat[t] = 0;
#pragma unroll
            for (int j = 0; j < N; ++j) ws.task_y[t * N + j] = y[j];
            atomicMin(&ws.inc[inst], cost_key(c));
        }
    }
}

// The optimal copies (mpc.x_front.X / x_back.X, fleet_naive_admm.py:413-446) of the naive-ADMM
// min_1_norm winners: one wave per instance re-solves the winning sequence's LP (the same LP as its
// leaf, the same iterate) and the lanes that own the copy groups write them.  After k_bnb_finish
// (which zeroes the copies of instances without an optimal answer).
template <int N>
__global__ __launch_bounds__((kL1BlockOfA<N, true>)) __attribute__((amdgpu_waves_per_eu(1))) void k_l1_admm_write(int B, const hvp_system* __restrict__ systems,
                                                                 const int32_t* __restrict__ sys,
                                                                 const int32_t* __restrict__ role,
                                                                 const double* __restrict__ params, hvp::Consts C,
                                                                 Workspace ws, double* __restrict__ xf_out,
                                                                 double* __restrict__ xb_out) {
    double* red = g_l1_admm_lds<N>;  // one wave per block
    const int lane = threadIdx.x & 63;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < B; i += nwaves) {
        const unsigned long long key = ws.key[i];
        const int flag = ws.inst_flag[i];
        if (key == ~0ull || (flag & 7)) continue;  // not HVP_OPTIMAL (k_bnb_finish)
        uint64_t code = 0;
#pragma unroll
        for (int k = 0; k < N; ++k)
            code = hvp::code_with(code, k, (int)((key >> (hvp::kCodeBits * (N - 1 - k))) & ((1u << hvp::kCodeBits) - 1)));
        double y[N], c = 0.0;
        int it = 0;
        const size_t o = (size_t)i * 2 * (N + 1);
        l1_admm_node_lp<N>(systems[sys[i]], C, role[i], params + (size_t)i * C.stride, code, N, 0.0, -1.0, y, c, it,
                           red, lane, xf_out ? xf_out + o : nullptr, xb_out ? xb_out + o : nullptr);
    }
}

// ---- min_1_norm by the per-lane simplex (hvp_lp.h), N <= 8: one node LP per LANE (64 per wave)
// where k_l1_root / k_l1_bound spend a wavefront on each interior-point LP.  Same search, statuses
// and bounds as those kernels (the LP optimum is the same; where it is a face the simplex returns
// a vertex of it, the interior point a point inside -- equal costs).  The LP's per-step data live
// in LDS (LdsMem rows, hvp_lp.h LF_*), its simplex state (vertex, basis inverse, basis ids) in
// registers.
template <int N, int BS = kBnbBlock<N>>
__device__ inline int lp_node(const hvp_system& S, const hvp::Consts& C, int rl, const double* prm, uint64_t code,
                              int K, double rlo, double rhi, double* y, double& cost, int& it) {
    hvp::LpData<N, LdsMem<N, BS>> D;
    D.mem.lane = threadIdx.x;
    const int st = hvp::lp_solve_l1<N>(D, S, C, rl, prm, code, K, rlo, rhi, C.max_iter, y, it);
    cost = st == hvp::L1_OK ? hvp::l1_direct_cost<N>(y, S, C, rl, prm, code, K, rlo, rhi) : 0.0;
    return st;
}

// the enumeration candidates' LPs, one per lane (k_cost prices them, as after k_qp_l1)
template <int N>
__global__ __launch_bounds__(kBnbBlock<N>) void k_qp_lp(const hvp_system* __restrict__ systems,
                                                        const int32_t* __restrict__ sys,
                                                        const int32_t* __restrict__ role,
                                                        const double* __restrict__ params, hvp::Consts C,
                                                        Workspace ws) {
    constexpr int BS = kBnbBlock<N>;
    const unsigned long long reserved = ws.counter[0];
    const long long total = (long long)(reserved < (unsigned long long)ws.cap ? reserved : ws.cap);
    unsigned long long iter_sum = 0;
    for (long long t = (long long)blockIdx.x * BS + threadIdx.x; t < total; t += (long long)gridDim.x * BS) {
        const int inst = ws.task_inst[t];
        if (inst < 0) continue;  // dead slot of an overflowed instance
        const hvp_system& S = systems[sys[inst]];
        const double* prm = params + (size_t)inst * (2 + 6 * (N + 1));
        hvp::LpData<N, LdsMem<N, BS>> D;
        D.mem.lane = threadIdx.x;
        double y[N];
        int iters = 0;
        const int status = hvp::lp_solve_l1<N>(D, S, C, role[inst], prm, ws.task_code[t], N, 0.0, -1.0, C.max_iter, y,
                                               iters);
        ws.task_stat[t] = status | (iters << 8);
#pragma unroll
        for (int k = 0; k < N; ++k) ws.task_y[t * N + k] = y[k];
        iter_sum += (unsigned long long)iters;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) iter_sum += __shfl_down(iter_sum, off, 64);
    if ((threadIdx.x & 63) == 0 && iter_sum) atomicAdd(&ws.counter[1], iter_sum);
}

// (one lane per instance: 64-lane blocks, so the B / 64 waves spread over every CU instead of
// filling a quarter of them four waves deep)
constexpr int kLpRootBlock = 64;
template <int N>
__global__ __launch_bounds__(kLpRootBlock) void k_lp_root(int B, const hvp_system* __restrict__ systems,
                                                          const int32_t* __restrict__ sys,
                                                          const int32_t* __restrict__ role,
                                                          const double* __restrict__ params, hvp::Consts C,
                                                          Workspace ws) {
    constexpr int BS = kLpRootBlock;
    const int i = blockIdx.x * BS + threadIdx.x;
    if (i == 0) ws.lvl[0] = (unsigned long long)B;
    if (i >= B) return;
    const hvp_system& S = systems[sys[i]];
    const int rl = role[i];
    const double* prm = params + (size_t)i * C.stride;
    const double v0 = prm[1], P1 = prm[0] + S.ts * v0;
    const bool ok = P1 >= S.pmin - 1e-9 * (1.0 + fabs(S.pmin)) && P1 <= S.pmax + 1e-9 * (1.0 + fabs(S.pmax));
    double inc = __longlong_as_double(0x7ff0000000000000ll);  // +inf: no incumbent
    double lb = -1e300;
    int nodes = 0, iters = 0;
    // up to four LPs with ONE call site: 0 the root relaxation, 1 the greedy dive's leaf from the
    // root optimum, 2 a second dive towards the constant-velocity trajectory (the simplex's root
    // optimum is a vertex -- an extreme point where the LP optimum is a face; the two dives find
    // different incumbents: at n = 10, N = 5 / 8 the search solves 17.2 / 114 LPs per instance
    // against 18.6 / 194 with the first alone, host replay), 3 the hinted sequence's leaf
    uint64_t code = 0, dive_code = 0, dive2 = 0;
    int job = ok ? 0 : 4, K = 0;
    double rlo = v0, rhi = v0;
    bool dived = false, dived2 = false;
    while (job < 4) {
        double y[N], c = 0.0;
        int it = 0;
        const int st = lp_node<N, BS>(S, C, rl, prm, code, K, rlo, rhi, y, c, it);
        ++nodes;
        iters += it;
        int next = 4;
        if (job == 0) {
            if (st == hvp::L1_INFEASIBLE) lb = 1e300;  // no completion is feasible
            if (st == hvp::L1_OK) {
                lb = c;
                dived = hvp::bnb_dive<N>(S, C, v0, y, &dive_code);
#pragma unroll
                for (int j = 0; j < N; ++j) y[j] = v0;
                dived2 = hvp::bnb_dive<N>(S, C, v0, y, &dive2) && !(dived && dive2 == dive_code);
                next = dived ? 1 : 2;
            }
        } else {
            if (st == hvp::L1_OK && !(c >= inc)) inc = c;
            next = job + 1;
        }
        if (next == 1) code = dive_code;
        if (next == 2) {
            if (dived2) code = dive2;
            else next = 3;
        }
        if (next == 3) {
            uint64_t hc = 0;
            if (ws.hint && hint_code<N>(ws, i, S, C, v0, &hc) && !(dived && hc == dive_code) && !(dived2 && hc == dive2))
                code = hc;
            else next = 4;
        }
        job = next;
        K = N;
        rlo = 0.0;
        rhi = -1.0;
    }
    ws.key[i] = ~0ull;
    ws.inst_flag[i] = ok ? 0 : 1;
    ws.nd_inst[0][i] = ok ? i : -1;
    ws.nd_code[0][i] = 0;
    ws.nd_lo[0][i] = v0;
    ws.nd_hi[0][i] = v0;
    ws.nd_lb[0][i] = lb;
    ws.inc[i] = cost_key(inc);
    ws.nodes[i] = nodes;
    ws.iters[i] = iters;
    atomicAdd(&ws.counter[3], (unsigned long long)nodes);
    atomicAdd(&ws.counter[1], (unsigned long long)iters);
}

template <int N>
__global__ __launch_bounds__(kBnbBlock<N>) void k_lp_bound(int k, const hvp_system* __restrict__ systems,
                                                           const int32_t* __restrict__ sys,
                                                           const int32_t* __restrict__ role,
                                                           const double* __restrict__ params, hvp::Consts C,
                                                           Workspace ws) {
    constexpr int BS = kBnbBlock<N>;
    const int dst = k & 1;
    const unsigned long long nn = ws.lvl[k];
    const long long total = (long long)(nn < (unsigned long long)ws.cap ? nn : ws.cap);
    unsigned long long iter_sum = 0;
    for (long long t = (long long)blockIdx.x * BS + threadIdx.x; t < total; t += (long long)gridDim.x * BS) {
        const int inst = ws.nd_inst[dst][t];
        if (inst < 0) {  // dead slot of an overflowed reservation
            if (k == N) ws.leaf_stat[t] = HVP_OVERFLOW;
            else ws.nd_lb[dst][t] = 1e300;
            continue;
        }
        const hvp_system& S = systems[sys[inst]];
        const double* prm = params + (size_t)inst * C.stride;
        double y[N], c = 0.0;
        int it = 0;
        const int st = lp_node<N>(S, C, role[inst], prm, ws.nd_code[dst][t], k, ws.nd_lo[dst][t], ws.nd_hi[dst][t],
                                  y, c, it);
        iter_sum += (unsigned long long)it;
        atomicAdd(&ws.nodes[inst], 1);
        atomicAdd(&ws.iters[inst], it);
        if (k < N) {
            // proven infeasible: the subtree holds no feasible completion; unresolved: prunes nothing
            ws.nd_lb[dst][t] = st == hvp::L1_OK ? c : (st == hvp::L1_INFEASIBLE ? 1e300 : -1e300);
            if (st == hvp::L1_FAIL) atomicAdd(&ws.counter[4], 1ull);
        } else {
            if (st == hvp::L1_OK) ws.nd_lb[dst][t] = c;  // an unresolved leaf keeps its parent's bound
            ws.leaf_stat[t] = st == hvp::L1_OK ? 0 : (st == hvp::L1_INFEASIBLE ? HVP_INFEASIBLE : HVP_MAXITER);
#pragma unroll
            for (int j = 0; j < N; ++j) ws.task_y[t * N + j] = y[j];
            if (st == hvp::L1_OK) atomicMin(&ws.inc[inst], cost_key(c));
            if (st == hvp::L1_FAIL) atomicOr(&ws.inst_flag[inst], 8);  // a sequence exists, unresolved
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) iter_sum += __shfl_down(iter_sum, off, 64);
    if ((threadIdx.x & 63) == 0 && iter_sum) atomicAdd(&ws.counter[1], iter_sum);
}

// ---- the same bound / leaf QPs, persistent waves (decentralised form, N <= 8)
// Every wave loops over { one active-set trip per busy lane (scan if due, one step) } and, when
// at least kRefillMin lanes are free, an EVENT: the lanes whose QP finished write their results
// together, then every free lane takes a node (one atomic per wave for the batch) and builds
// its QP together.  A lane's solver state (hvp_gi.h GiLane: J, packed R, multipliers) stays in
// registers across trips; the sigma-independent part of every node's QP (tracking terms,
// safe-row bounds) is computed once per instance by K_inst_prep.  2 waves per SIMD (the solver
// fits 256 VGPRs with a little spill around the event code; 2 x 72 KB of per-lane rows in LDS
// per CU).  kRefillMin trades idle lanes against events run by few lanes -- measured at C2
// (profiles/r02e_*): 8 -> 3.52M, 16 -> 3.95M, 32 -> 4.41M, 48 -> 4.69M, 64 -> 4.86M
// platoon-steps/s: the setup and write code run at full width beats refilling lanes early, so
// the default refills a wave when ALL its lanes are free (generations of 64 nodes).
// A variant written as explicit generations (claim 64 nodes -> set up -> trips until the wave is
// done -> write 64 results) ran at 2.73M against this kernel's 4.87M (profiles/r02q_*): with two
// trip-loop levels the compiler's allocation spills ~3x more scratch traffic inside the trips.
// Same results per node as k_bnb_bound (the node -> lane mapping does not matter).
#ifndef HVP_REFILL_WAVES
#define HVP_REFILL_WAVES 2
#endif
#ifndef HVP_REFILL_MIN
#define HVP_REFILL_MIN 64
#endif
constexpr int kRefillMin = HVP_REFILL_MIN;
constexpr int kRefillBlocksPerCu = HVP_REFILL_WAVES;

// per-instance sigma-independent QP part, instance-major: instance i's fields at
// iq[i * kIqStride + f], each row padded to whole 128-byte lines.  The refill kernel's event reads
// the rows of ~20 distinct instances per 64-node generation; a field-major (SoA) layout made every
// one of the 28 fields (N = 5) a separate line per instance -- about 1 KB of L2 misses per node,
// most of the kernel's 304 MB of HBM traffic per launch (profiles/r04k, r05c) -- where a row is
// two lines.
template <int N>
constexpr int kIqFields = N * (N + 1) / 2 + N + 2 * (N - 1);  // H, f, hf, hb
template <int N>
constexpr int kIqStride = (kIqFields<N> + 15) / 16 * 16;  // doubles per row (hvp_kernels.hip hvp_reserve)

template <int N>
__global__ __launch_bounds__(kBlock) void k_inst_prep(int B, const hvp_system* __restrict__ systems,
                                                      const int32_t* __restrict__ sys,
                                                      const int32_t* __restrict__ role,
                                                      const double* __restrict__ params, hvp::Consts C, Workspace ws) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) ws.lvl[0] = (unsigned long long)B;
    if (i >= B) return;
    constexpr int NT = N * (N + 1) / 2;
    double H[NT], f[N], C0, hf[N - 1], hb[N - 1];
    const hvp_system& S = systems[sys[i]];
    const double* prm = params + (size_t)i * C.stride;
    hvp::setup_track<N>(S, C, role[i], prm, H, f, C0, hf, hb);
    // the search's per-instance state and the root node (level 0, list 0), as k_bnb_root sets them:
    // the refill kernel solves the root level like any other (launch_bnb)
    const double v0 = prm[1], P1 = prm[0] + S.ts * v0;
    const bool ok = P1 >= S.pmin - 1e-9 * (1.0 + fabs(S.pmin)) && P1 <= S.pmax + 1e-9 * (1.0 + fabs(S.pmax));
    ws.key[i] = ~0ull;
    ws.inst_flag[i] = ok ? 0 : 1;
    ws.nd_inst[0][i] = ok ? i : -1;
    ws.nd_code[0][i] = 0;
    ws.nd_lo[0][i] = v0;
    ws.nd_hi[0][i] = v0;
    ws.nd_lb[0][i] = -1e300;
    ws.inc[i] = cost_key(__longlong_as_double(0x7ff0000000000000ll));  // +inf: no incumbent
    ws.nodes[i] = 0;
    ws.iters[i] = 0;
    double* o = ws.iq + (size_t)i * kIqStride<N>;
#pragma unroll
    for (int j = 0; j < NT; ++j) o[j] = H[j];
#pragma unroll
    for (int j = 0; j < N; ++j) o[NT + j] = f[j];
#pragma unroll
    for (int j = 0; j < N - 1; ++j) {
        o[NT + N + j] = hf[j];
        o[NT + 2 * N - 1 + j] = hb[j];
    }
#pragma unroll
    for (int j = kIqFields<N>; j < kIqStride<N>; ++j) o[j] = 0.0;  // whole lines: no partial-line write-back
}

// The greedy dive of every instance whose root QP (level 0, solved by the refill kernel) succeeded:
// its leaf goes to the dive list (ws.dv_*), which the refill kernel solves next as a level-N list
// of its own (launch_bnb) -- its leaf costs set the incumbents before level 1, as in k_bnb_root.
template <int N>
__global__ __launch_bounds__(kBlock) void k_bnb_dive_prep(int B, const hvp_system* __restrict__ systems,
                                                          const int32_t* __restrict__ sys,
                                                          const double* __restrict__ params, hvp::Consts C,
                                                          Workspace ws) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        ws.dv_lvl[N] = (unsigned long long)B;
        ws.dv_lvl[(HVP_MAX_N + 1) + N] = 0ull;  // claims
    }
    if (i >= B) return;
    const bool root_ok = ws.nd_inst[0][i] >= 0 && ws.nd_lb[0][i] > -1e300;
    uint64_t code = 0;
    bool dived = false;
    if (root_ok) {
        double ystar[N];
#pragma unroll
        for (int j = 0; j < N; ++j) ystar[j] = ws.task_y[(size_t)i * N + j];
        dived = hvp::bnb_dive<N>(systems[sys[i]], C, params[(size_t)i * C.stride + 1], ystar, &code);
    }
    ws.dv_inst[i] = dived ? i : -1;
    ws.dv_code[i] = code;
    ws.dv_lo[i] = 0.0;
    ws.dv_hi[i] = -1.0;
    // root + dive QPs (hvp_get_stats counts the levels' nodes from their lists)
    const unsigned qp = (ws.nd_inst[0][i] >= 0 ? 1u : 0u) + (dived ? 1u : 0u);
    if (qp) atomicAdd(&ws.counter[3], (unsigned long long)qp);
}

// the node QP of instance inst from the per-instance part + the node's regions / relaxation, for
// the refill event.  Its loads are issued together: the instance's system index, role and x0
// first, the ws.iq row behind them, and one wait for all (not one wait for sys[inst] to address
// the table, one for the role and x0, and only then the row).  kmask: the regions the node can
// take at step K (setup_input), the event's child set.
template <int N, class Q>
__device__ inline bool setup_node_batch(Q& q, const hvp_system* tab, const int32_t* sys, const int32_t* role,
                                        const double* params, const hvp::Consts& C, const Workspace& ws, int inst,
                                        uint64_t code, int K, double rlo, double rhi, unsigned* kmask) {
    constexpr int NT = N * (N + 1) / 2;
    const double* o = static_cast<const double*>(__builtin_assume_aligned(ws.iq + (size_t)inst * kIqStride<N>, 128));
    const double* prm = params + (size_t)inst * C.stride;
    int si = sys[inst], rl = role[inst];
    double p0 = prm[0], v0 = prm[1];
    double hf[N > 1 ? N - 1 : 1], hb[N > 1 ? N - 1 : 1];
#pragma unroll
    for (int j = 0; j < NT; ++j) q.H[j] = o[j];
#pragma unroll
    for (int j = 0; j < N; ++j) q.f[j] = o[NT + j];
#pragma unroll
    for (int j = 0; j < N - 1; ++j) {
        hf[j] = o[NT + N + j];
        hb[j] = o[NT + 2 * N - 1 + j];
    }
    hvp::pin_value(si);
    hvp::pin_value(rl);
    hvp::pin_value(p0);
    hvp::pin_value(v0);
    const hvp_system& S = tab[si];
    const bool ok = hvp::setup_scalars<N>(q, S, rl, p0, v0);
#pragma unroll
    for (int j = 0; j < N - 1; ++j) {
        q.mem.set(hvp::F_HF, j, hf[j]);
        q.mem.set(hvp::F_HB, j, hb[j]);
    }
    q.C0 = 0.0;  // not used by the active-set path (costs come from direct_cost)
    hvp::setup_input<N>(q, S, C, code, K, rlo, rhi, kmask);
    return ok;
}

// LEAF / UPPER: the caller's level is known to be N / below N (k_bnb_bound_refill's phases), and
// only that side of the write-back is instantiated
template <int N, bool LEAF = false, bool UPPER = false>
__device__ inline void bnb_node_done(int k, long long t, int inst, bool ok, int its, double c, const double* y,
                                     const hvp::Consts& C, const Workspace& ws) {
    static_assert(!(LEAF && UPPER), "one phase");
    const int dst = k & 1;
    atomicAdd(&ws.nodes[inst], 1);
    atomicAdd(&ws.iters[inst], its);
    if (UPPER || (!LEAF && k < N)) {
        ws.nd_lb[dst][t] = ok ? c : -1e300;  // a failed bound QP prunes nothing
        if (!ok) atomicAdd(&ws.counter[4], 1ull);
        if (k == 0 && ok) {  // the root's optimum: the greedy dive's target (k_bnb_dive_prep)
#pragma unroll
            for (int j = 0; j < N; ++j) ws.task_y[t * N + j] = y[j];
        }
    } else {
        if (ok) ws.nd_lb[dst][t] = c;  // a failed leaf keeps its parent's bound
        ws.leaf_stat[t] = ok ? 0 : HVP_MAXITER;
#pragma unroll
        for (int j = 0; j < N; ++j) ws.task_y[t * N + j] = y[j];
        // the dive list's leaf (entry t = inst): its steps, for the level-N copy it may stand for
        // (Workspace::reuse)
        if (ws.lvl == ws.dv_lvl) ws.dv_redo[t] = its;
        if (ok) {
            atomicMin(&ws.inc[inst], cost_key(c));
        } else if (ws.lvl != ws.dv_lvl) {
            // (a failed greedy-dive leaf -- the dive list's descriptor, launch_bnb -- only fails to set
            // an incumbent, as in k_bnb_root: no flag, no interior-point re-solve)
            atomicOr(&ws.inst_flag[inst], 8);  // a velocity-feasible sequence exists
            if (C.form == HVP_FORM_DECENT) {  // K_bnb_ipm re-solves it
                const unsigned long long r = atomicAdd(&ws.counter[2], 1ull);
                if (r < (unsigned long long)ws.cap) ws.redo[r] = (int32_t)t;
            }
        }
    }
}

// wave-level claim of `nfree` consecutive work items from *claim (one atomic per wave): returns
// the first item; the free lanes take base + their rank among the free lanes (wave_rank)
__device__ inline unsigned long long wave_claim(unsigned long long* claim, unsigned long long free, int nfree,
                                                int lane) {
    const int leader = __ffsll((long long)free) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(claim, (unsigned long long)nfree);
    return ((unsigned long long)(unsigned)__shfl((int)(base >> 32), leader, 64) << 32) |
           (unsigned)__shfl((int)(base & 0xffffffffu), leader, 64);
}
__device__ inline int wave_rank(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// The order in which k_bnb_bound_coop takes a level's nodes when the naive-ADMM node records are
// on (node_index): the nodes whose slot they own and whose record is theirs (a warm start, ~2
// active-set steps) from the front of ws.task_inst (unused by the branch and bound), the others
// (a cold start, ~16) from the back.  Which group solves a node changes nothing in its result.
// The two fill counters are level k's entries of ws.lvl's spare rows (5M + k: front, 2M + k: back,
// M = HVP_MAX_N + 1; zeroed per solve, unused at split = 1).
template <int N>
__global__ __launch_bounds__(kBlock) void k_node_order(int k, Workspace ws) {
    constexpr int M = HVP_MAX_N + 1;
    using Rec = hvp::coop::WarmRec<N>;
    const int dst = k & 1;
    const unsigned long long nn = ws.lvl[k];
    const long long total = (long long)(nn < (unsigned long long)ws.cap ? nn : ws.cap);
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63);
    const long long stride = (long long)gridDim.x * blockDim.x;
    const Rec* recs = reinterpret_cast<const Rec*>(ws.nrec);
    for (long long qw = wave0; qw < total; qw += stride) {  // wave-uniform loop
        const long long q = qw + lane;
        bool warm = false;
        if (q < total) {
            const int inst = ws.nd_inst[dst][q];
            if (inst >= 0) {
                const uint64_t code = ws.nd_code[dst][q];
                const size_t ni = node_index(ws, inst, k, code);
                warm = ws.nclaim[ni] == node_prio(ws, code) && recs[ni].valid && recs[ni].code == code;
            }
        }
        const unsigned long long wm = __ballot(q < total && warm), cm = __ballot(q < total && !warm);
        const int nw = __popcll(wm), nc = __popcll(cm);
        unsigned long long bw = 0, bc = 0;
        if (lane == 0) {
            if (nw) bw = atomicAdd(&ws.lvl[5 * M + k], (unsigned long long)nw);
            if (nc) bc = atomicAdd(&ws.lvl[2 * M + k], (unsigned long long)nc);
        }
        bw = __shfl((int)bw, 0, 64);  // (< 2^31: a level's node count)
        bc = __shfl((int)bc, 0, 64);
        if (q < total) {
            const long long pos = warm ? (long long)(bw + wave_rank(wm)) : total - 1 - (long long)(bc + wave_rank(cm));
            ws.task_inst[pos] = (int32_t)q;
        }
    }
}

// min_1_norm root level through the LP refill kernel (HVP_LP_ROOT_REFILL, default on): the search
// state and the root nodes (k_lp_root's, without its LPs) ...
template <int N>
__global__ __launch_bounds__(kBlock) void k_lp_root_init(int B, const hvp_system* __restrict__ systems,
                                                         const int32_t* __restrict__ sys,
                                                         const double* __restrict__ params, hvp::Consts C,
                                                         Workspace ws) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) ws.lvl[0] = (unsigned long long)B;
    if (i >= B) return;
    const hvp_system& S = systems[sys[i]];
    const double* prm = params + (size_t)i * C.stride;
    const double v0 = prm[1], P1 = prm[0] + S.ts * v0;
    const bool ok = P1 >= S.pmin - 1e-9 * (1.0 + fabs(S.pmin)) && P1 <= S.pmax + 1e-9 * (1.0 + fabs(S.pmax));
    ws.key[i] = ~0ull;
    ws.inst_flag[i] = ok ? 0 : 1;
    ws.nd_inst[0][i] = ok ? i : -1;
    ws.nd_code[0][i] = 0;
    ws.nd_lo[0][i] = v0;
    ws.nd_hi[0][i] = v0;
    ws.nd_lb[0][i] = -1e300;
    ws.inc[i] = cost_key(__longlong_as_double(0x7ff0000000000000ll));  // +inf: no incumbent
    ws.nodes[i] = 0;
    ws.iters[i] = 0;
}

// ... then, from each root optimum, k_lp_root's incumbent leaves -- the greedy dive, the dive
// towards the constant-velocity trajectory, the hinted sequence (each skipped when it repeats an
// earlier one) -- as a list of up to 3 leaves per instance (ws.dv_*), solved by the refill kernel
// at K = N before level 1: only their costs are used (the incumbents), as in k_lp_root.
template <int N>
__global__ __launch_bounds__(kBlock) void k_lp_dive_prep(int B, const hvp_system* __restrict__ systems,
                                                         const int32_t* __restrict__ sys,
                                                         const double* __restrict__ params, hvp::Consts C,
                                                         Workspace ws) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        ws.dv_lvl[N] = 3ull * (unsigned long long)B;
        ws.dv_lvl[(HVP_MAX_N + 1) + N] = 0ull;  // claims
    }
    if (i >= B) return;
    const hvp_system& S = systems[sys[i]];
    const double v0 = params[(size_t)i * C.stride + 1];
    const double lb = ws.nd_lb[0][i];
    const bool root_ok = ws.nd_inst[0][i] >= 0 && lb > -1e300 && lb < 1e300;  // the root LP solved
    uint64_t c1 = 0, c2 = 0, hc = 0;
    bool d1 = false, d2 = false, dh = false;
    if (root_ok) {
        double y[N];
#pragma unroll
        for (int j = 0; j < N; ++j) y[j] = ws.task_y[(size_t)i * N + j];
        d1 = hvp::bnb_dive<N>(S, C, v0, y, &c1);
#pragma unroll
        for (int j = 0; j < N; ++j) y[j] = v0;
        d2 = hvp::bnb_dive<N>(S, C, v0, y, &c2) && !(d1 && c2 == c1);
        dh = ws.hint && hint_code<N>(ws, i, S, C, v0, &hc) && !(d1 && hc == c1) && !(d2 && hc == c2);
    }
    const size_t o = 3 * (size_t)i;
    ws.dv_inst[o] = d1 ? i : -1;
    ws.dv_inst[o + 1] = d2 ? i : -1;
    ws.dv_inst[o + 2] = dh ? i : -1;
    ws.dv_code[o] = c1;
    ws.dv_code[o + 1] = c2;
    ws.dv_code[o + 2] = hc;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        ws.dv_lo[o + q] = 0.0;
        ws.dv_hi[o + q] = -1.0;
    }
    // root + dive LPs (hvp_get_stats counts the levels' nodes from their lists)
    const unsigned lps = (ws.nd_inst[0][i] >= 0 ? 1u : 0u) + (d1 ? 1u : 0u) + (d2 ? 1u : 0u) + (dh ? 1u : 0u);
    if (lps) atomicAdd(&ws.counter[3], (unsigned long long)lps);
}

// occupancy of the LP refill kernel (A/B builds: -DHVP_LP_WAVES=2 asks for two waves per SIMD)
#ifdef HVP_LP_WAVES
#define HVP_LP_OCC __attribute__((amdgpu_waves_per_eu(HVP_LP_WAVES)))
#else
#define HVP_LP_OCC
#endif
#ifndef HVP_LP_INV_BATCH
#define HVP_LP_INV_BATCH 12
#endif
constexpr int kLpInvBatch = HVP_LP_INV_BATCH;

// The same node LPs through persistent waves: every lane keeps its LP's simplex state (hvp_lp.h
// LpLane) in registers and runs one iteration per trip; when at least `refill_min` lanes of the
// wave are free, their finished LPs are written (k_lp_bound's outputs, node for node) and every
// free lane claims the level's next node (one atomic per wave).  A node LP takes 6.5 pivots on
// average and a wave of 64 one-per-lane LPs waits for its slowest (~17 pivots, host histogram):
// the grid-stride kernel idles ~60 % of its lanes.  HVP_LP_REFILL=<min free lanes> (0: k_lp_bound).
template <int N>
__global__ __launch_bounds__(kBnbBlock<N>) HVP_LP_OCC void k_lp_bound_refill(int k, const hvp_system* __restrict__ systems,
                                                                   const int32_t* __restrict__ sys,
                                                                   const int32_t* __restrict__ role,
                                                                   const double* __restrict__ params, hvp::Consts C,
                                                                   Workspace ws, int refill_arg) {
    constexpr int BS = kBnbBlock<N>;
    enum { IDLE = 0, RUN = 1, DONE = 2 };
    // refill_arg: the refill threshold (free lanes, bits 0-7) and the rebuild batch (bits 8-15)
    const int refill_min = refill_arg & 255, inv_batch = (refill_arg >> 8) & 255;
    const int dst = k & 1;
    const int lane = threadIdx.x & 63;
    const unsigned long long nn = ws.lvl[k];
    const long long total = (long long)(nn < (unsigned long long)ws.cap ? nn : ws.cap);
    hvp::LpData<N, LdsMem<N, BS>> D;
    D.mem.lane = threadIdx.x;
    hvp::LpLane<N> L;
    double y[N];
#pragma unroll
    for (int j = 0; j < N; ++j) y[j] = 0.0;
    long long t = -1;
    int inst = 0, stage = IDLE, st = 0;
    bool exhausted = false;
    unsigned long long iter_sum = 0;
    for (;;) {
        const unsigned long long free = __ballot(stage != RUN);
        const int nfree = __popcll(free);
        if (nfree >= refill_min || nfree == 64) {
            if (stage == DONE) {
                const hvp_system& S = systems[sys[inst]];
                const double* prm = params + (size_t)inst * C.stride;
                double c = 0.0;
                if (st == hvp::L1_OK)
                    c = hvp::l1_direct_cost<N>(y, S, C, role[inst], prm, ws.nd_code[dst][t], k, ws.nd_lo[dst][t],
                                               ws.nd_hi[dst][t]);
                const int it = L.iters;
                iter_sum += (unsigned long long)it;
                atomicAdd(&ws.nodes[inst], 1);
                atomicAdd(&ws.iters[inst], it);
                if (k < N) {
                    ws.nd_lb[dst][t] = st == hvp::L1_OK ? c : (st == hvp::L1_INFEASIBLE ? 1e300 : -1e300);
                    if (st == hvp::L1_FAIL) atomicAdd(&ws.counter[4], 1ull);
                    if (k == 0 && st == hvp::L1_OK) {  // the root optimum: the greedy dive's start
#pragma unroll
                        for (int j = 0; j < N; ++j) ws.task_y[t * N + j] = y[j];
                    }
                } else {
                    if (st == hvp::L1_OK) ws.nd_lb[dst][t] = c;
                    ws.leaf_stat[t] = st == hvp::L1_OK ? 0 : (st == hvp::L1_INFEASIBLE ? HVP_INFEASIBLE : HVP_MAXITER);
#pragma unroll
                    for (int j = 0; j < N; ++j) ws.task_y[t * N + j] = y[j];
                    if (st == hvp::L1_OK) atomicMin(&ws.inc[inst], cost_key(c));
                    // (an unresolved incumbent leaf of the dive list only sets no incumbent, as in k_lp_root)
                    if (st == hvp::L1_FAIL && ws.lvl != ws.dv_lvl) atomicOr(&ws.inst_flag[inst], 8);
                }
                stage = IDLE;
            }
            if (exhausted && nfree == 64) break;
            if (!exhausted) {
                const unsigned long long base = wave_claim(ws.lvl + (HVP_MAX_N + 1) + k, free, nfree, lane);
                if (base + nfree >= (unsigned long long)total) exhausted = true;
                const long long mc = (long long)base + wave_rank(free);
                if (stage == IDLE && mc < total) {
                    const int in = ws.nd_inst[dst][mc];
                    if (in < 0) {  // dead slot of an overflowed reservation
                        if (k == N) ws.leaf_stat[mc] = HVP_OVERFLOW;
                        else ws.nd_lb[dst][mc] = 1e300;
                    } else {
                        t = mc;
                        inst = in;
                        const hvp_system& S = systems[sys[inst]];
                        const double* prm = params + (size_t)inst * C.stride;
                        const uint64_t code = ws.nd_code[dst][mc];
                        const double rlo = ws.nd_lo[dst][mc], rhi = ws.nd_hi[dst][mc];
                        if (hvp::l1_infeasible<N>(S, C, prm, code, k, rlo, rhi)) {
                            st = hvp::L1_INFEASIBLE;
                            L.iters = 0;
                            stage = DONE;
                        } else {
                            hvp::lp_data<N>(D, S, C, role[inst], prm, code, k, rlo, rhi);
                            L.init(D, C);
                            stage = RUN;
                        }
                    }
                }
            }
        }
        // every trip is one scan over the terms for every running lane (hvp_lp.h LpLane::trip); the
        // lanes that wait for a rebuild of A_B^-1 (about one scan of work, taken by the whole wave
        // whenever any lane runs it) are served together: when inv_batch of them wait, or a quarter
        // of the running lanes
        const unsigned long long run_m = __ballot(stage == RUN);
        const unsigned long long inv_m = __ballot(stage == RUN && L.wants_inv());
        const int ninv = __popcll(inv_m);
        const bool do_inv = ninv > 0 && (ninv >= inv_batch || 4 * ninv >= __popcll(run_m));
        if (stage == RUN) {
            const int r = L.trip(D, C, C.max_iter, y, do_inv);
            if (r != hvp::LP_RUN) {
                st = r == hvp::LP_OK ? hvp::L1_OK : hvp::L1_FAIL;
                stage = DONE;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) iter_sum += __shfl_down(iter_sum, off, 64);
    if (lane == 0 && iter_sum) atomicAdd(&ws.counter[1], iter_sum);
}

// lane stages of the refill kernels
// RS_PASS: a pass-through node (bnb_put_children kPassFlag), finished without a QP
enum { RS_IDLE = 0, RS_SCAN = 1, RS_STEP = 2, RS_FAIL = 3, RS_OPT = 4, RS_PASS = 5 };

#ifdef HVP_REFILL_PROF
// Switches of the diagnostics build:
//   HVP_REFILL_PROF_PIN   1: gi_trip's stamps wait for the code they close (see gi_trip); 0: the
//                         bare stamps of the earlier rounds, for comparison
//   HVP_REFILL_PROF_ROWS  1: per-row counts of the scan's selection blocks (their ballots and
//                         atomics sit inside the scan: a build for the counts, not for the cycles)
#ifndef HVP_REFILL_PROF_PIN
#define HVP_REFILL_PROF_PIN 1
#endif
#ifndef HVP_REFILL_PROF_ROWS
#define HVP_REFILL_PROF_ROWS 0
#endif
// [0, 64): busy trips per node; [64, 128): trips per generation (event to event);
// [128, 128 + kPfRows): per row id of the scan, the scans (one per wave and trip) in which at
// least one scanning lane violates the row, i.e. the wave runs the row's selection block;
// [128 + kPfRows]: all scans (wave trips with a scanning lane)
constexpr int kPfRows = 80;  // row ids of N <= 8 (at most 76)
constexpr int kPfHist = 128 + kPfRows + 1;
__device__ unsigned long long g_pf_hist[kPfHist];

// the scan's diagnostics hook (hvp_gi.h gi_most_violated): one ballot per row over the lanes that
// scan, counted by the first of them
struct ScanProbe {
    __device__ void operator()(int id, bool viol) const {
        const unsigned long long any = __ballot(viol), me = __ballot(true);
        const bool first = (int)(threadIdx.x & 63) == __ffsll((long long)me) - 1;
        if (first && id == 0) atomicAdd(&g_pf_hist[128 + kPfRows], 1ull);
        if (first && any) atomicAdd(&g_pf_hist[128 + id], 1ull);
    }
};
#endif

// one active-set trip of a busy lane (RS_SCAN / RS_STEP); finished lanes end in RS_FAIL / RS_OPT
//
// Diagnostics build: the wave's cycles in the scan and in the step.  A stamp is no barrier for
// arithmetic: the scan and the step are register code, and the compiler is free to finish them
// after the stamp that should close them.  With HVP_REFILL_PROF_PIN the values a half returns
// pass through an empty asm before its closing stamp, so they are computed by then (measured:
// it moves little, scan 0.029 -> 0.044 of a wave's life).
template <int N, class Q>
__device__ inline void gi_trip(Q& q, hvp::GiLane<N>& g, const hvp::Consts& C, int& stage, int& fail
#ifdef HVP_REFILL_PROF
                        , unsigned long long* pf_scan = nullptr, unsigned long long* pf_step = nullptr
#endif
) {
    q.mem.refresh();
    g.fence(q);
#ifdef HVP_REFILL_PROF
    const unsigned long long pf_s0 = __builtin_amdgcn_s_memtime();
#endif
#if defined(HVP_REFILL_PROF) && HVP_REFILL_PROF_ROWS
    if (stage == RS_SCAN) stage = g.scan(q, C, ScanProbe()) ? RS_STEP : RS_OPT;
#else
    if (stage == RS_SCAN) stage = g.scan(q, C) ? RS_STEP : RS_OPT;
#endif
#ifdef HVP_REFILL_PROF
#if HVP_REFILL_PROF_PIN
    asm volatile("" : "+v"(g.p), "+v"(g.pd), "+v"(g.pa), "+v"(stage));
#endif
    const unsigned long long pf_s1 = __builtin_amdgcn_s_memtime();
    if (pf_scan) *pf_scan += pf_s1 - pf_s0;
#endif
    if (stage == RS_STEP) {
        const int r = g.step(q, C, kGiMaxIter<N>);
        if (r == hvp::GI_STEP_NEXT) stage = RS_SCAN;
        else if (r != hvp::GI_STEP_MORE) stage = RS_FAIL, fail = r;
    }
#ifdef HVP_REFILL_PROF
#if HVP_REFILL_PROF_PIN
    g.fence(q);
    asm volatile("" : "+v"(g.unew), "+v"(g.nact), "+v"(stage), "+v"(fail));
#endif
    if (pf_step) *pf_step += __builtin_amdgcn_s_memtime() - pf_s1;
#endif
}

// Persistent refill kernel: where its data lives, and why (the measurements are DESIGN.md
// section 4's dated entries; the alternatives are no longer in the source).
//
// Arguments.  The workspace descriptor and the problem constants are by-value kernel arguments and
// the level list is hoisted above the loop.  Reading them inside the event through device copies
// took the kernel off most of its scratch and was slower all the same (2.97-3.15 against 2.68 ms
// of QP launches per step: every load through an opaque pointer is issued again after each store
// of the event; DESIGN.md "Round 4: where the refill event reads its descriptors",
// profiles/r04i_bench_*, r04j_bench_*).
//
// System tables.  The event's region loops (relax_step, bnb_child, bnb_put_children) and
// direct_cost read hvp_system fields tens of times per node, each a dependent per-lane load
// (systems[sys[inst]]).  STAGE: the block copies the handle's n_sys tables into LDS at entry and
// the event indexes that copy by sys[inst] (a batch may mix systems).  At most kRefillSysCap
// tables: at N = 5 the per-lane rows take 71,680 B of the 81,920 B a block may use with two
// blocks per CU, and 8 tables are 6,144 B.  A handle with more systems runs the STAGE = false
// instantiation, which reads them from global memory (launch_refill).  (DESIGN.md 2026-10-19,
// profiles/r07a_refill_tables_ab.jsonl.)
//
// Child set.  A node's children are the mask its set-up's relax_step at step k found, kept in a
// lane register (nmask) until the write-back: bnb_children's calls with the same arguments, made
// once (profiles/r07a_refill_tables_stack_ab.jsonl).
//
// Loads in batches.  direct_cost loads the lane's whole parameter row before its step loop
// (hvp_ipm.h, BATCH) and the incumbent's key with it; the claimed slot's four node fields are
// loaded together, then sys, role, x0 and the ws.iq row together (setup_node_batch).  (DESIGN.md
// 2026-10-20 "loads in batches", profiles/r07b_refill_event_ab.jsonl.)
constexpr int kRefillSysCap = 8;
// Uniform data.  The block's copy of what is uniform over a launch and holds no pointer: the
// problem constants (~95 dwords with dec[16] and acc[16]) and the hoisted level list, written to
// LDS once at entry (before the one barrier) and read from there by the event.  Together with the
// workspace descriptor's ~120 dwords the kernel arguments, live across the persistent loop, are
// twice the 102 SGPRs: the rest sits in VGPR lanes (v_writelane / v_readlane, one dword at a
// time) and pushes lane state into scratch.  The readers bind references to the __shared__
// object itself, so the address space stays known after inlining (ds_read, never flat_load), and
// LDS reads cannot alias the event's global stores.  uni_view() makes the object's offset opaque
// where it is called, once per event, so the loads stay there instead of being hoisted above the
// loop into registers again (as LdsMem::refresh() does for the lane rows).
// The descriptor itself stays a by-value argument: a pointer read back from LDS is a generic one
// to the compiler (flat_load / flat_store / flat_atomic for every access of the event -- a cast
// through the global address space is folded away, and a local copy with the casts is indexed by
// the level's parity at run time, so it lands in scratch), where a kernel argument is known to
// point to global memory.
// The trips read the constants from the argument: with the event off it, what the scan needs fits
// the scalar registers, and uniform values read from LDS land in VGPRs, of which the trip has
// none to spare (event alone -5.1 %, event and trips -4.0 %: DESIGN.md 2026-10-20 "from LDS",
// profiles/r08a_refill_uniform_ab.jsonl, series 1).
// The claim's atomic follows the write-back: issued at the top of the event and consumed after
// it, it was 1.7-1.8 % slower in every run (the same entry and file, series 3).
// The event reads the copy at the horizons where that takes the kernel off scratch (N >= 5: every
// one of them holds less scratch per lane with it, profiles/r08a_refill_static.txt).  Below, the
// arguments fit the registers, the copy only costs a few (N = 2: 162 -> 171 VGPRs, N = 2 and 4:
// 36 B/lane of scratch that the by-value reads do not have): those horizons read the arguments,
// take no LDS for the copy and no barrier for it.
constexpr int kRefillUniMinN = 5;
template <int N>
constexpr bool kRefillUniEvent = N >= kRefillUniMinN;
struct RefillUni {
    hvp::Consts C;
    LevelList lvl;
    long long total;  // lvl.count()
};
static_assert(sizeof(RefillUni) <= 4096 - 64, "N = 5: rows 71,680 B + tables 6,144 B + this <= 81,920 B (2 blocks per CU)");
template <class T>
__device__ inline const T& uni_view(const T& obj) {
    unsigned off = 0;
    asm volatile("" : "+s"(off));
    return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(&obj) + off);
}
// Phases.  The level k is a run-time argument, and a launch of one level carried the code and the
// registers of every kind of level.  PH says which levels an instantiation serves, and the event
// leaves out of its source path what those cannot reach (launch_refill picks it from k):
//   RP_ANY    every level: the kernel before, line for line.
//   RP_LEAF   k == N, a constant (level N and the dive list).  A leaf has no children: no child
//             mask (nmask, cmask, clb), no pruning test, no split_reserve / bnb_put_children, no
//             reuse block, no relaxed step in its set-up.  No RS_PASS either: a level-N slot never
//             carries kPassFlag (bnb_put_children is called with pass = -1 at k + 1 == N, and
//             k_bnb_dive_prep's codes are bnb_dive's, plain region digits).
//   RP_UPPER  k + 1 < N, k at run time (levels 0..N-2): no leaf write-back (leaf_stat, task_y of a
//             leaf, the incumbent's atomicMin, the redo list), no reuse block.
// Level N - 1, the only one that enters the reuse block, runs RP_ANY.
// The statements that remain are the same, in the same order: results are bit-equal.  At run time
// HVP_REFILL_PHASES=0 sends every launch through RP_ANY (launch_bnb; tests, A/B).  Measured -4.3 %
// per flagship step (DESIGN.md 2026-10-21 "by the level's phase", profiles/r11a_refill_phase_ab.jsonl);
// an instantiation for level N - 1 or level 0 alone fails the static gate below (the same entry).
enum { RP_ANY = 0, RP_LEAF = 1, RP_UPPER = 2 };
// Which instantiations ship: those whose trip section (the stretch without a global access) has no
// more instructions, scratch instructions or v_readlanes than RP_ANY's in the same build, at the
// same waves per SIMD and LDS (profiles/r11a_refill_phase_static.txt, profiles/refill_static.py).
// The register allocation of the trip moves with every edit of the event, although the trip's
// source is the same in all three: a pair that misses keeps RP_ANY.  Bit N of [STAGE], N up to
// HVP_MAX_N_ENUM (the refill path's horizons; the launchers of longer ones only test their bit).
constexpr unsigned kRefillLeafOk[2] = {1u << 2 | 1u << 3 | 1u << 5 | 1u << 6 | 1u << 7 | 1u << 8,
                                       1u << 2 | 1u << 3 | 1u << 5 | 1u << 6 | 1u << 8};
constexpr unsigned kRefillUpperOk[2] = {1u << 3 | 1u << 4, 1u << 3 | 1u << 4 | 1u << 5 | 1u << 8};
template <int N, bool STAGE>
constexpr bool kRefillPhLeaf = (kRefillLeafOk[STAGE] >> N) & 1u;
template <int N, bool STAGE>
constexpr bool kRefillPhUpper = (kRefillUpperOk[STAGE] >> N) & 1u;
template <int N, bool STAGE, int PH = RP_ANY>
__global__ __launch_bounds__(kBnbBlock<N>) __attribute__((amdgpu_waves_per_eu(HVP_REFILL_WAVES)))
void k_bnb_bound_refill(int k_arg, const hvp_system* __restrict__ systems, int n_sys, const int32_t* __restrict__ sys,
                        const int32_t* __restrict__ role, const double* __restrict__ params, hvp::Consts C_arg,
                        Workspace ws_arg) {
    constexpr int BS = kBnbBlock<N>;
    static_assert(N <= HVP_MAX_N_ENUM, "lane refill is the N <= 8 path");
    constexpr bool kLeaf = PH == RP_LEAF, kUpper = PH == RP_UPPER;
    const int k = kLeaf ? N : k_arg;
    if constexpr (kUpper) __builtin_assume(k + 1 < N);
    constexpr bool kUniEvent = kRefillUniEvent<N>;
    __shared__ RefillUni s_uni;  // (takes no LDS where nothing below uses it)
    const RefillUni& U = s_uni;
    if constexpr (kUniEvent) {
        if (threadIdx.x == 0) {  // (from the arguments' scalar registers; the barrier is below)
            s_uni.C = C_arg;
            s_uni.lvl = level_list(ws_arg, k);
            s_uni.total = s_uni.lvl.count();
        }
    }
    const hvp_system* tab = systems;  // the tables the event reads
    if constexpr (STAGE) {
        __shared__ hvp_system s_sys[kRefillSysCap];
        static_assert(sizeof(hvp_system) % sizeof(unsigned long long) == 0, "copied in 8-byte words");
        constexpr int kWords = (int)(sizeof(hvp_system) / sizeof(unsigned long long));
        const unsigned long long* src = reinterpret_cast<const unsigned long long*>(systems);
        unsigned long long* dstw = reinterpret_cast<unsigned long long*>(s_sys);
        const int nw = (n_sys < kRefillSysCap ? n_sys : kRefillSysCap) * kWords;
        for (int i = threadIdx.x; i < nw; i += BS) dstw[i] = src[i];
        tab = s_sys;
    }
    if (STAGE || kUniEvent) __syncthreads();  // the only barrier: waves leave the loop at different times
    const int dst = k & 1;
    const Workspace& ws = ws_arg;
    const LevelList lvl_arg = level_list(ws, k);  // (N < kRefillUniMinN; unused where the event reads the copy)
    const long long total_arg = lvl_arg.count();
    unsigned long long* const claim_arg = ws.lvl + (HVP_MAX_N + 1) + k;
    const int lane = threadIdx.x & 63;
    hvp::LaneQp<N, LdsMem<N, BS>> q;
    q.mem.lane = threadIdx.x;
    hvp::GiLane<N> g;
    long long t = -1;  // node of the lane
    int inst = 0, stage = RS_IDLE, fail = 0;  // (RS_PASS: fail holds the pass-through node's steps)
    uint64_t code = 0;
    unsigned nmask = 0;  // regions the lane's node can take at step k (its set-up's relax_step)
    bool exhausted = false;
    unsigned long long iter_sum = 0, pass_n = 0;  // (pass_n: pass-through nodes | reused dive leaves << 32)
#ifdef HVP_REFILL_PROF  // diagnostics build: event / trip cycles and busy lane-trips per wave
    unsigned long long pf_ev = 0, pf_all = 0, pf_busy = 0, pf_trips = 0, pf_wb = 0, pf_cl = 0, pf_dc = 0, pf_rs = 0;
    unsigned long long pf_scan = 0, pf_step = 0;
    const unsigned long long pf_t0 = __builtin_amdgcn_s_memtime();
    int pf_mine = 0, pf_gen = 0;
#endif
    for (;;) {
        const bool done = stage >= RS_FAIL;
        const unsigned long long free = __ballot(stage == RS_IDLE || done);
        const int nfree = __popcll(free);
#ifdef HVP_REFILL_PROF
        const bool pf_event = nfree >= kRefillMin || nfree == 64;
        pf_busy += (unsigned long long)(64 - nfree);
        pf_trips += 1;
        if (pf_event) {
            // (the histogram's atomics -- 64 lanes on a few shared words -- complete before the
            // event's stamp, so they are charged to neither the event nor "until cost")
            if (done) atomicAdd(&g_pf_hist[pf_mine < 63 ? pf_mine : 63], 1ull);
            if (lane == 0) atomicAdd(&g_pf_hist[64 + (pf_gen < 63 ? pf_gen : 63)], 1ull);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            pf_gen = 0;
            pf_mine = 0;
        }
        ++pf_gen;
        if (stage == RS_SCAN || stage == RS_STEP) ++pf_mine;
        const unsigned long long pf_e0 = __builtin_amdgcn_s_memtime();
#endif
        if (nfree >= kRefillMin || nfree == 64) {
            // ---- event: write the finished lanes' results, then refill every free lane
            const RefillUni* E = nullptr;
            if constexpr (kUniEvent) E = &uni_view(U);
            const hvp::Consts& C = kUniEvent ? E->C : C_arg;
            const LevelList& lvl = kUniEvent ? E->lvl : lvl_arg;
            const long long total = kUniEvent ? E->total : total_arg;
            unsigned long long* const claim = kUniEvent ? ws.lvl + (HVP_MAX_N + 1) + k : claim_arg;
            unsigned cmask = 0;  // children of a finished bound node (k_bnb_expand's work, fused)
            double clb = 0.0;
            int csteps = 0;      // the finished node's active-set steps (its children's bucket)
            if (!kLeaf && done && stage == RS_PASS) {  // (no level-N slot is a pass-through node)
                // a pass-through node: its QP is its parent's (bound inherited in nd_lb), so only its
                // children are written.  A tree node all the same (nodes_out, the NodeCount
                // analogue); hvp_stats.n_candidates counts QPs and leaves it out (counter[6])
                stage = RS_IDLE;
                atomicAdd(&ws.nodes[inst], 1);
                clb = ws.nd_lb[dst][t];
                csteps = fail;
                if (!(ws.inst_flag[inst] & 2) && !hvp::bnb_pruned(clb, inc_of(ws, inst)))
                    cmask = bnb_children(tab[sys[inst]], C, k, ws.nd_lo[dst][t], ws.nd_hi[dst][t]);
            } else if (done) {
                const int st = stage == RS_OPT ? g.verify(C, nullptr) : fail;
                const bool ok = st == hvp::GI_OK;
                // the incumbent's key, fetched with the cost's row (only leaves move it, and a launch
                // of level k < N runs none; at k == N it is not read)
                constexpr bool kInc = !kLeaf;
                unsigned long long inck = 0;
                if (kInc && !ok) inck = ws.inc[inst];
                const double c = ok ? hvp::direct_cost<N, true>(
                                          q, tab[sys[inst]], C, role[inst], params + (size_t)inst * C.stride, code,
                                          k, kInc ? ws.inc + inst : nullptr, &inck)
                                    : 0.0;
                iter_sum += (unsigned long long)g.iter;
                csteps = ok ? g.iter : -1;
#ifdef HVP_REFILL_PROF
                {
                    const double cc = __builtin_amdgcn_readfirstlane(__double_as_longlong(c) & 0xffffffff);
                    (void)cc;
                    pf_dc += __builtin_amdgcn_s_memtime() - pf_e0;
                }
#endif
                bnb_node_done<N, kLeaf, kUpper>(k, t, inst, ok, g.iter, c, q.y, C, ws);
                stage = RS_IDLE;
                if constexpr (!kLeaf) {
                // the incumbent only changes at the leaves (level N): below N this pruning test
                // sees the value a separate expand kernel would
                clb = ok ? c : -1e300;
                if (k < N && !(ws.inst_flag[inst] & 2) &&
                    !hvp::bnb_pruned(clb, kInc ? key_cost(inck) : inc_of(ws, inst)))
                    cmask = nmask;  // (the child set its set-up's relax_step found: bnb_children's)
                }
            }
            if constexpr (PH == RP_ANY)
            if (k + 1 == N && ws.reuse && cmask) {
                // The child that is the greedy dive's sequence is the dive list's leaf over again (the
                // same code, K = N: the same QP, steps and bits), and its parent is never pruned
                // before level N: every ancestor's bound is a relaxation of that leaf's QP, whose cost
                // is the incumbent until the first level-N leaf.  Where that leaf's QP succeeded the
                // child is not written: the dive entry stands for it in the tie rule (flag 16:
                // k_bnb_key, k_bnb_write, k_bnb_finish) and in the tree's counts.  A failed dive leaf
                // is written as before: its level-N copy raises flag 8 and goes to k_bnb_ipm.
                const uint64_t dcode = ws.dv_code[inst];
                const int dstat = ws.dv_stat[inst];  // (nonzero too where the instance did not dive)
                constexpr uint64_t kPrefix = (1ull << (hvp::kCodeBits * (N - 1))) - 1;
                const unsigned bit = 1u << hvp::code_region(dcode, N - 1);
                if (dstat == 0 && ((dcode ^ code) & kPrefix) == 0 && (cmask & bit)) {
                    cmask &= ~bit;
                    atomicOr(&ws.inst_flag[inst], 16);
                    atomicAdd(&ws.nodes[inst], 1);
                    atomicAdd(&ws.iters[inst], ws.dv_redo[inst]);
                    pass_n += 1ull << 32;  // (the high half: reused leaves)
                }
            }
            if constexpr (!kLeaf)
            if (k < N) {
                unsigned long long limit;
                const unsigned long long off =
                    split_reserve(ws, k + 1, __popc(cmask), csteps > 0 ? csteps : 0, lane, limit);
                if (cmask)
                    pass_n += bnb_put_children(ws, k + 1, off, limit, cmask, inst, tab[sys[inst]], C, code,
                                               ws.nd_lo[dst][t], ws.nd_hi[dst][t], clb, k + 1 < N ? csteps : -1);
#ifdef HVP_REFILL_PROF
                pf_rs += __builtin_amdgcn_s_memtime() - pf_e0;
#endif
            }
            if (exhausted && nfree == 64) break;
#ifdef HVP_REFILL_PROF
            const unsigned long long pf_w1 = __builtin_amdgcn_s_memtime();
            pf_wb += pf_w1 - pf_e0;
#endif
            if (!exhausted) {
                // the claim, after the write-back (issued at the top of the event it was slower)
                const unsigned long long base = wave_claim(claim, free, nfree, lane);
#ifdef HVP_REFILL_PROF
                {
                    const unsigned long long bb = __builtin_amdgcn_readfirstlane((unsigned)base);
                    (void)bb;
                    pf_cl += __builtin_amdgcn_s_memtime() - pf_w1;
                }
#endif
                if (base + nfree >= (unsigned long long)total) exhausted = true;
                const long long mc = (long long)base + wave_rank(free);
                const long long mine = lvl.slot(mc);
                if (stage == RS_IDLE && mc < total) {
                    // the slot's four fields together (a dead slot's other three are allocated
                    // and not looked at)
                    int ninst = ws.nd_inst[dst][mine];
                    uint64_t ncode = ws.nd_code[dst][mine];
                    double nlo = ws.nd_lo[dst][mine], nhi = ws.nd_hi[dst][mine];
                    hvp::pin_value(ninst);
                    hvp::pin_value(ncode);
                    hvp::pin_value(nlo);
                    hvp::pin_value(nhi);
                    inst = ninst;
                    if (inst < 0) {  // dead slot of an overflowed reservation
                        if (k == N) ws.leaf_stat[mine] = HVP_OVERFLOW;
                        else ws.nd_lb[dst][mine] = 1e300;
                    } else {
                        t = mine;
                        code = ncode;
                        if (!kLeaf && (code & kPassFlag)) {  // its parent's QP: finished at the next event
                            fail = (int)((code >> 56) & 127);
                            code &= kPassCode;
                            stage = RS_PASS;
                        } else {
                            setup_node_batch<N>(q, tab, sys, role, params, C, ws, inst, code, k, nlo, nhi,
                                                !kLeaf ? &nmask : nullptr);
                            stage = g.init(q) == hvp::GI_OK ? RS_SCAN : RS_FAIL;
                            fail = hvp::GI_FAIL_CHOL;
                        }
                    }
                }
            }
        }
#ifdef HVP_REFILL_PROF
        if (pf_event) pf_ev += __builtin_amdgcn_s_memtime() - pf_e0;
#endif
#ifdef HVP_REFILL_PROF
        // (the trip's two stamps are the wave's, but only the busy lanes run it: they are taken
        // from the first busy lane and added by all, so lane 0, which reports them, holds every
        // trip's.  Added inside the branch, lane 0 only held the trips it was busy in: about half,
        // which is what earlier rounds' splits left outside the event, the scan and the step.)
        const unsigned long long pf_busy_m = __ballot(stage == RS_SCAN || stage == RS_STEP);
        unsigned long long pf_dscan = 0, pf_dstep = 0;
#endif
        if (stage == RS_SCAN || stage == RS_STEP) {
            // the trip reads the argument, not the copy.  (Through this reference: with C_arg
            // named in the call the same code comes out with a few instructions in another order.)
            const hvp::Consts& Ct = C_arg;
#ifdef HVP_REFILL_PROF
            gi_trip<N>(q, g, Ct, stage, fail, &pf_dscan, &pf_dstep);
#else
            gi_trip<N>(q, g, Ct, stage, fail);
#endif
        }
#ifdef HVP_REFILL_PROF
        if (pf_busy_m) {
            const int src = __ffsll((long long)pf_busy_m) - 1;
            pf_scan += __shfl(pf_dscan, src, 64);
            pf_step += __shfl(pf_dstep, src, 64);
        }
#endif
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        iter_sum += __shfl_down(iter_sum, off, 64);
        pass_n += __shfl_down(pass_n, off, 64);
    }
    if (lane == 0 && iter_sum) atomicAdd(&ws.counter[1], iter_sum);
    // pass-through nodes (no QP; hvp_get_stats) and, in the high half, the dive leaves that stand
    // for their level-N copies (QPs of the tree that ran once)
    if (lane == 0 && (pass_n & 0xffffffffull)) atomicAdd(&ws.counter[6], pass_n & 0xffffffffull);
    if (lane == 0 && (pass_n >> 32)) atomicAdd(&ws.counter[7], pass_n >> 32);
#ifdef HVP_REFILL_PROF
    pf_all = __builtin_amdgcn_s_memtime() - pf_t0;
    if (lane == 0) {  // the claim slots of levels > N are free (prof builds need N <= 6)
        unsigned long long* pf = ws.lvl + 2 * (HVP_MAX_N + 1) - 8;
        atomicAdd(&pf[-2], pf_scan);
        atomicAdd(&pf[-1], pf_step);
        atomicAdd(&pf[0], pf_ev);
        atomicAdd(&pf[1], pf_all);
        atomicAdd(&pf[2], pf_busy);
        atomicAdd(&pf[3], pf_trips);
        atomicAdd(&pf[4], pf_wb);
        atomicAdd(&pf[5], pf_cl);
        atomicAdd(&pf[6], pf_dc);
        atomicAdd(&pf[7], pf_rs);
    }
#endif
}

// Leaves whose active-set solve failed its verification (degenerate vertices, e.g. the
// position box at p_max): re-solved by the interior-point method on the full row set
// (hvp_ipm.h), as K_qp_ipm does for the enumeration path.  Normally an empty list.  ADMM: the
// hinge-state iteration around the interior point (hvp_admm.h solve_admm_ipm).  The two forms are
// separate kernels: with both bodies in one kernel the decentralised re-solve at N = 10 did not
// finish on MI355X (r04e: k_bnb_ipm<10> never returned, the round-3 single-form kernel takes ms).
template <int N, bool ADMM>
__global__ __launch_bounds__(kBnbBlock<N>) void k_bnb_ipm(const hvp_system* __restrict__ systems,
                                                          const int32_t* __restrict__ sys,
                                                          const int32_t* __restrict__ role,
                                                          const double* __restrict__ params, hvp::Consts C,
                                                          Workspace ws) {
    constexpr int BS = kBnbBlock<N>;
    const int src = N & 1;
    const unsigned long long nr = ws.counter[2];
    const long long total = (long long)(nr < (unsigned long long)ws.cap ? nr : ws.cap);
    for (long long i = (long long)blockIdx.x * BS + threadIdx.x; i < total; i += (long long)gridDim.x * BS) {
        const long long t = ws.redo[i];
        const int inst = ws.nd_inst[src][t];
        const uint64_t code = ws.nd_code[src][t];
        const hvp_system& S = systems[sys[inst]];
        const int rl = role[inst];
        const double* prm = params + (size_t)inst * C.stride;
        hvp::LaneQp<N, LdsMem<N, BS>> q;
        q.mem.lane = threadIdx.x;
        double c;
        if constexpr (ADMM) {
            int its = 0;
            const int st = hvp::solve_admm_ipm<N>(q, S, C, rl, prm, code, N, its);
            atomicAdd(&ws.iters[inst], its);
            if (st != hvp::GI_OK) continue;
            c = hvp::admm_direct_cost<N>(q, S, C, rl, prm, code, N);
        } else {
            hvp::setup_lane<N>(q, S, C, rl, prm, code);
            const hvp::QpOut o = hvp::Solver<N, true, LdsMem<N, BS>>::solve(q, C);
            atomicAdd(&ws.iters[inst], o.iters);
            if (o.status != 0) continue;  // stays HVP_MAXITER with its parent's bound (K_key flags it)
            c = hvp::direct_cost<N>(q, S, C, rl, prm, code);
        }
#pragma unroll
        for (int j = 0; j < N; ++j) ws.task_y[t * N + j] = q.y[j];
        ws.nd_lb[src][t] = c;
        ws.leaf_stat[t] = 0;
        atomicMin(&ws.inc[inst], cost_key(c));
    }
}

// tie rule: the lexicographically first leaf within 1e-9 relative of the minimum
// n_dive: entries of the dive list (one per instance) to scan as well, 0 without Workspace::reuse.
// The entry of an instance with flag 16 is the level-N leaf that the refill event did not write
// (its QP succeeded), under the same rule.
template <int N>
__global__ __launch_bounds__(kBlock) void k_bnb_key(Workspace ws, int form, int l1, int n_dive) {
    const int src = N & 1;
    const LevelList lvl = level_list(ws, N);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_dive; i += gridDim.x * blockDim.x) {
        if (!(ws.inst_flag[i] & 16)) continue;
        const double best = inc_of(ws, i);
        if (ws.dv_lb[i] <= best + 1e-9 * fmax(1.0, fabs(best)))
            atomicMin(&ws.key[i], (unsigned long long)hvp::bnb_lexkey(ws.dv_code[i], N));
    }
#pragma unroll
    for (int b = 0; b < kMaxBuckets; ++b)
    for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < (long long)lvl.n[b];
         c += (long long)gridDim.x * blockDim.x) {
        const long long t = (long long)(b * lvl.seg) + c;
        const int inst = ws.nd_inst[src][t];
        if (inst < 0) continue;
        const double best = inc_of(ws, inst);
        if (ws.leaf_stat[t] != 0) {
            // A decentralised leaf that fails the active-set method AND the interior-point fallback
            // (K_bnb_ipm, every N) is an infeasible QP (position box), excluded exactly as the
            // enumeration path and the oracle exclude it.  A naive-ADMM leaf that fails both is not
            // known to be infeasible (the interior point also fails on some feasible Huber-piece
            // QPs): still in contention, it makes the instance MAXITER rather than a possibly wrong
            // answer.  The min_1_norm leaves are HVP_INFEASIBLE (certified, excluded) or
            // HVP_MAXITER (unresolved, treated the same way).
            const bool strict = form != HVP_FORM_DECENT || l1;
            if (ws.leaf_stat[t] == HVP_MAXITER && strict && !hvp::bnb_pruned(ws.nd_lb[src][t], best))
                atomicOr(&ws.inst_flag[inst], 4);
            continue;
        }
        if (ws.nd_lb[src][t] <= best + 1e-9 * fmax(1.0, fabs(best)))
            atomicMin(&ws.key[inst], (unsigned long long)hvp::bnb_lexkey(ws.nd_code[src][t], N));
    }
}

template <int N>
__device__ inline void write_solution(int i, const hvp_system& S, const double* prm, bool win, uint64_t code,
                                      const double* y, double* u_out, double* x_out, int8_t* region_out,
                                      int8_t* gear_out) {
    double p = prm[0], v = prm[1];
    if (x_out) {
        x_out[(size_t)i * 2 * (N + 1)] = p;
        x_out[(size_t)i * 2 * (N + 1) + N + 1] = v;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int r = hvp::code_region(code, k);
        const double vn = win ? y[k] : v;
        const double u = win ? (vn - S.a[r] * v - S.c[r]) / S.b[r] : 0.0;
        p = p + S.ts * v;
        v = vn;
        if (u_out) u_out[(size_t)i * N + k] = u;
        if (x_out) {
            x_out[(size_t)i * 2 * (N + 1) + k + 1] = p;
            x_out[(size_t)i * 2 * (N + 1) + N + 1 + k + 1] = v;
        }
        if (region_out) region_out[(size_t)i * N + k] = (int8_t)(win ? r : -1);
        if (gear_out) gear_out[(size_t)i * N + k] = (int8_t)(win ? S.gear[r] : 0);
    }
}

// optimal neighbour copies of an ADMM solution (fleet_naive_admm.py: mpc.x_front.X / x_back.X)
template <int N>
__device__ inline void write_copies(int i, const hvp_system& S, const hvp::Consts& C, int rl, const double* prm,
                                    bool win, const double* y, double* xf_out, double* xb_out) {
    const bool side_on[2] = {(rl & HVP_ROLE_SAFE_FRONT) != 0, (rl & HVP_ROLE_SAFE_BACK) != 0};
    const bool track[2] = {(rl & HVP_ROLE_TRACK_FRONT) != 0, (rl & HVP_ROLE_TRACK_BACK) != 0};
    double* outs[2] = {xf_out, xb_out};
    const int K1 = N + 1;
    for (int side = 0; side < 2; ++side) {
        double* o = outs[side];
        if (!o) continue;
        o += (size_t)i * 2 * K1;
        double p = prm[0], v = prm[1];
        for (int k = 0; k <= N; ++k) {
            double e = 0.0, g = 0.0;
            if (win && side_on[side])
                hvp::admm_copy_value(C, track[side], side, hvp::admm_y(prm, side, N)[k],
                                     hvp::admm_y(prm, side, N)[K1 + k], hvp::admm_z(prm, side, N)[k],
                                     hvp::admm_z(prm, side, N)[K1 + k], p, v, &e, &g);
            o[k] = e;
            o[K1 + k] = g;
            if (k < N) {
                p = p + S.ts * v;
                v = win ? y[k] : v;
            }
        }
    }
}

// The winning leaf of every instance (its lexicographic key equals the instance's key, k_bnb_key):
// only its slot is recorded here (4 bytes, scattered in leaf order); k_bnb_finish writes the
// outputs in instance order, so every output line is written whole by one wave.  (Writing u, x,
// regions, gears and cost here, in leaf order, scattered 150 B per instance over lines that other
// waves -- on other XCDs -- complete: 116 MB of HBM writes per C2 solve for ~25 MB of outputs,
// profiles/r05zc.)
template <int N>
__global__ __launch_bounds__(kBlock) void k_bnb_write(Workspace ws, int n_dive) {
    const int src = N & 1;
    const LevelList lvl = level_list(ws, N);
    // a winning dive entry (k_bnb_key's n_dive): ~i, which no slot of the list is.  The instance's
    // level-N leaves all have other sequences, so one writer per instance remains.
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_dive; i += gridDim.x * blockDim.x) {
        if (!(ws.inst_flag[i] & 16)) continue;
        if (hvp::bnb_lexkey(ws.dv_code[i], N) == ws.key[i]) ws.win[i] = ~i;
    }
#pragma unroll
    for (int b = 0; b < kMaxBuckets; ++b)
    for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < (long long)lvl.n[b];
         c += (long long)gridDim.x * blockDim.x) {
        const long long t = (long long)(b * lvl.seg) + c;
        if (ws.leaf_stat[t] != 0) continue;
        const int inst = ws.nd_inst[src][t];
        if (inst < 0) continue;
        if (hvp::bnb_lexkey(ws.nd_code[src][t], N) != ws.key[inst]) continue;
        ws.win[inst] = (int32_t)t;
    }
}

template <int N>
__global__ __launch_bounds__(kBlock) void k_bnb_finish(int B, const hvp_system* __restrict__ systems,
                                                       const int32_t* __restrict__ sys,
                                                       const int32_t* __restrict__ role,
                                                       const double* __restrict__ params, hvp::Consts C, Workspace ws,
                                                       double* __restrict__ u_out, double* __restrict__ x_out,
                                                       int8_t* __restrict__ region_out, int8_t* __restrict__ gear_out,
                                                       double* __restrict__ cost_out, int32_t* __restrict__ status_out,
                                                       int32_t* __restrict__ nodes_out,
                                                       int32_t* __restrict__ iters_out,
                                                       double* __restrict__ xf_out, double* __restrict__ xb_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && ws.dv_counter && ws.dv_counter[1]) atomicAdd(&ws.counter[1], ws.dv_counter[1]);  // the dives' steps
    if (i >= B) return;
    const int flag = ws.inst_flag[i];
    const bool win = ws.key[i] != ~0ull;
    int status;
    if (flag & 1) status = HVP_INFEASIBLE;
    else if (flag & 2) status = HVP_OVERFLOW;
    else if (flag & 4) status = HVP_MAXITER;  // a leaf in contention whose QP did not converge
    else if (win) status = HVP_OPTIMAL;
    else status = (flag & 8) ? HVP_MAXITER : HVP_INFEASIBLE;  // sequences exist but no QP converged
    if (status_out) status_out[i] = status;
    if (nodes_out) nodes_out[i] = ws.nodes[i];
    if (iters_out) iters_out[i] = ws.iters[i];
    if (ws.nclaim && (flag & 2)) {
        // an overflowed search wrote some of its node records in an order that depends on the
        // scheduling (which reservation ran out first): none of them starts a later solve
        hvp::coop::WarmRec<N>* recs = reinterpret_cast<hvp::coop::WarmRec<N>*>(ws.nrec);
        const size_t nr = (size_t)ws.ndepth * ws.nslots;
        for (size_t r = 0; r < nr; ++r) recs[(size_t)i * nr + r].valid = 0;
    }
    const double* prm = params + (size_t)i * C.stride;
    const hvp_system& S = systems[sys[i]];
    if (!win || status != HVP_OPTIMAL) {
        if (cost_out) cost_out[i] = 1e300;
        write_solution<N>(i, S, prm, false, 0, nullptr, u_out, x_out, region_out, gear_out);
        if (C.form == HVP_FORM_ADMM) write_copies<N>(i, S, C, role[i], prm, false, nullptr, xf_out, xb_out);
        return;
    }
    // the winner recorded by k_bnb_write: a slot of level N's list, or the instance's dive entry
    // (~i, only with Workspace::reuse)
    const int src = N & 1;
    const int w = ws.win[i];
    const bool dive = ws.reuse && w < 0;
    const long long t = dive ? (long long)i : (long long)w;
    const uint64_t code = dive ? ws.dv_code[t] : ws.nd_code[src][t];
    const double* ty = dive ? ws.dv_y : ws.task_y;
    double y[N];
#pragma unroll
    for (int j = 0; j < N; ++j) y[j] = ty[t * N + j];
    write_solution<N>(i, S, prm, true, code, y, u_out, x_out, region_out, gear_out);
    // (the min_1_norm copies come from the winner's LP: k_l1_admm_write)
    if (C.form == HVP_FORM_ADMM && !C.l1) write_copies<N>(i, S, C, role[i], prm, true, y, xf_out, xb_out);
    if (cost_out) cost_out[i] = dive ? ws.dv_lb[t] : ws.nd_lb[src][t];
}

// ================================================================== fixed-control evaluation
// MpcGear.evaluate_cost (mpcs/mpc_gear.py:137-170): with u (u_g for the gear model) and the
// gear of every step fixed, the MIQP has no free decision left but the slacks: the trajectory
// follows from the dynamics of the mode (gear label, region band containing v_k -- at a shared
// band edge the PWA dynamics coincide), the slacks take max(0, .), and the objective is the
// direct cost of that trajectory.  Status HVP_INFEASIBLE when a row of the MLD model fails.
template <int N>
__global__ __launch_bounds__(kBlock) void k_evaluate(int B, const hvp_system* __restrict__ systems,
                                                     const int32_t* __restrict__ sys, const int32_t* __restrict__ role,
                                                     const double* __restrict__ params, hvp::Consts C,
                                                     const int8_t* __restrict__ gear_in, const double* __restrict__ u_in,
                                                     double* __restrict__ cost_out, int32_t* __restrict__ status_out,
                                                     double* __restrict__ x_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const hvp_system& S = systems[sys[i]];
    const int rl = role[i];
    const double* prm = params + (size_t)i * (2 + 6 * (N + 1));
    hvp::LaneQp<N> q;
    q.has_sf = (rl & HVP_ROLE_SAFE_FRONT) != 0;
    q.has_sb = (rl & HVP_ROLE_SAFE_BACK) != 0;
    double p = prm[0], v = prm[1];
    uint64_t code = 0;
    bool ok = true;
    if (x_out) {
        x_out[(size_t)i * 2 * (N + 1)] = p;
        x_out[(size_t)i * 2 * (N + 1) + N + 1] = v;
    }
    for (int k = 0; k < N; ++k) {
        const int g = gear_in[(size_t)i * N + k];
        const double u = u_in[(size_t)i * N + k];
        int r = -1;
        for (int m = 0; m < S.n_regions && r < 0; ++m) {
            const double tol = 1e-9 * (1.0 + fabs(v));
            if (S.gear[m] == g && v >= S.vlo[m] - tol && v <= S.vhi[m] + tol) r = m;
        }
        if (r < 0) { ok = false; r = 0; }
        const double vn = S.a[r] * v + S.b[r] * u + S.c[r];
        const double tolu = 1e-9 * (1.0 + fabs(u));
        if (u < S.umin - tolu || u > S.umax + tolu) ok = false;
        const double dv = vn - v, tola = 1e-9 * (1.0 + fabs(dv));
        if (dv < C.dec[k] - tola || dv > C.acc[k] + tola) ok = false;
        p = p + S.ts * v;
        v = vn;
        const double tolv = 1e-9 * (1.0 + fabs(v)), tolp = 1e-9 * (1.0 + fabs(p));
        if (v < S.vmin - tolv || v > S.vmax + tolv || p < S.pmin - tolp || p > S.pmax + tolp) ok = false;
        q.y[k] = v;
        code = hvp::code_with(code, k, r);
        if (x_out) {
            x_out[(size_t)i * 2 * (N + 1) + k + 1] = p;
            x_out[(size_t)i * 2 * (N + 1) + N + 1 + k + 1] = v;
        }
    }
    const double cost = C.l1 ? hvp::l1_direct_cost<N>(q.y, S, C, rl, prm, code) : hvp::direct_cost<N>(q, S, C, rl, prm, code);
    cost_out[i] = ok ? cost : 1e300;
    status_out[i] = ok ? HVP_OPTIMAL : HVP_INFEASIBLE;
}

// ================================================================== switching ADMM (HVP_FORM_GADMM)
// TrackingGAdmmCoordinator / GAdmmCoordinator (fleet_g_admm.py:208-301, dmpcpwa [EXT]) for P
// platoons: rollout of the warm start, per ADMM iteration one local-QP launch + one consensus
// launch, sequence switching per round (include/hvp.h "Switching ADMM").  Instance b holds
// vehicle i = lo + b % m of platoon p = b / m; trajectories live in full-platoon slots p n + i.
__device__ inline int gadmm_slot(int b, int n, int lo, int m) { return (b / m) * n + lo + b % m; }

__device__ inline void gadmm_fail(int32_t* state, int p) {
    atomicOr(&state[p], 2);
    atomicAnd(&state[p], ~1);
}

// a local QP the active-set method failed on goes to k_gadmm_ipm (counter[3]: the list's size in
// this launch; counter[2]: the fallbacks since the rollout, hvp_get_stats n_fallback)
__device__ inline void gadmm_redo(int b, unsigned long long* counter, int32_t* redo) {
    const unsigned long long r = atomicAdd(&counter[3], 1ull);
    atomicAdd(&counter[2], 1ull);
    redo[r] = b;  // r < P m: one entry per local QP and launch
}

// first region whose closed velocity band holds v (buf widens the lower edge: the [0, 1e-4]
// buffer of PwaGearVehicle.find_region used by get_u_for_constant_vel, models.py:519-540)
__device__ inline int gadmm_region(const hvp_system& S, double v, double buf) {
    for (int r = 0; r < S.n_regions; ++r)
        if (v >= S.vlo[r] - buf && v <= S.vhi[r]) return r;
    return -1;
}

template <int N>
__global__ __launch_bounds__(kBlock) void k_gadmm_rollout(int P, int n, int lo, int m,
                                                          const hvp_system* __restrict__ systems,
                                                          const int32_t* __restrict__ sys,
                                                          const double* __restrict__ params, int stride, int mode,
                                                          const double* __restrict__ u_prev, double* __restrict__ x,
                                                          int8_t* __restrict__ seq, double* __restrict__ u_ws,
                                                          int32_t* __restrict__ state) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P * m) return;
    const int p = b / m;
    const hvp_system& S = systems[sys[b]];
    const double* prm = params + (size_t)b * stride;
    double pk = prm[0], vk = prm[1];
    double* xs = x + (size_t)gadmm_slot(b, n, lo, m) * 2 * (N + 1);
    bool ok = true;
    double ucv = 0.0;
    if (mode == 0) {
        const int r = gadmm_region(S, vk, 1e-4);
        if (r < 0) ok = false;
        else ucv = ((1.0 - S.a[r]) * vk - S.c[r]) / S.b[r];
    }
    xs[0] = pk;
    xs[N + 1] = vk;
    for (int k = 0; k < N; ++k) {
        const double u = mode == 0 ? ucv : u_prev[(size_t)b * N + (k + 1 < N ? k + 1 : N - 1)];
        int r = gadmm_region(S, vk, 0.0);
        if (r < 0) { ok = false; r = 0; }
        seq[(size_t)b * N + k] = (int8_t)r;
        if (u_ws) u_ws[(size_t)b * N + k] = u;
        const double vn = S.a[r] * vk + S.b[r] * u + S.c[r];
        pk = pk + S.ts * vk;
        vk = vn;
        xs[k + 1] = pk;
        xs[N + 1 + k + 1] = vk;
    }
    if (!ok) gadmm_fail(state, p);
}

// edge bits of the switching rule: active V rows at a region edge strictly inside the state box
template <int N>
__device__ inline uint32_t gadmm_edges(const hvp_system& S, uint64_t code, uint32_t raw) {
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j + 1 < N; ++j) {
        const int r = hvp::code_region(code, j + 1);
        const double lo = S.vlo[r], hi = S.vhi[r];
        if (((raw >> (2 * j)) & 1u) && lo > S.vmin + 1e-9 * (1.0 + fabs(lo))) out |= 1u << (2 * j);
        if (((raw >> (2 * j + 1)) & 1u) && hi < S.vmax - 1e-9 * (1.0 + fabs(hi))) out |= 1u << (2 * j + 1);
    }
    return out;
}

// outputs of one solved local problem: u, trajectory slot, copies (front: closed-form optimum of
// its hinge problem, back: z_b - y_b / rho)
template <int N>
__device__ inline void gadmm_write(int b, int slot, const hvp_system& S, const hvp::Consts& C, int rl,
                                   const double* prm, uint64_t code, const double* y, double* u_out, double* x,
                                   double* xf, double* xb) {
    const int K1 = N + 1;
    double* xs = x + (size_t)slot * 2 * K1;
    double* fs = xf + (size_t)slot * 2 * K1;
    double* bs = xb + (size_t)slot * 2 * K1;
    const bool front = (rl & HVP_ROLE_SAFE_FRONT) != 0, back = (rl & HVP_ROLE_BACK_COPY) != 0;
    const bool tf = (rl & HVP_ROLE_TRACK_FRONT) != 0;
    const double* yb = hvp::admm_y(prm, 1, N);
    const double* zb = hvp::admm_z(prm, 1, N);
    double p = prm[0], v = prm[1];
    for (int k = 0; k <= N; ++k) {
        xs[k] = p;
        xs[K1 + k] = v;
        double e = 0.0, g = 0.0;
        if (front)
            hvp::admm_copy_value(C, tf, 0, hvp::admm_y(prm, 0, N)[k], hvp::admm_y(prm, 0, N)[K1 + k],
                                 hvp::admm_z(prm, 0, N)[k], hvp::admm_z(prm, 0, N)[K1 + k], p, v, &e, &g);
        fs[k] = e;
        fs[K1 + k] = g;
        bs[k] = back ? zb[k] - yb[k] / C.rho : 0.0;
        bs[K1 + k] = back ? zb[K1 + k] - yb[K1 + k] / C.rho : 0.0;
        if (k < N) {
            const int r = hvp::code_region(code, k);
            const double vn = y[k];
            u_out[(size_t)b * N + k] = (vn - S.a[r] * v - S.c[r]) / S.b[r];
            p = p + S.ts * v;
            v = vn;
        }
    }
}

template <int N>
__device__ inline uint64_t gadmm_code(const int8_t* seq, int b) {
    uint64_t code = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) code = hvp::code_with(code, k, seq[(size_t)b * N + k]);
    return code;
}

// x-update, one lane per local QP (N <= 8)
template <int N>
__global__ __launch_bounds__(kBnbBlock<N>) void k_gadmm_qp(int P, int n, int lo, int m,
                                                           const hvp_system* __restrict__ systems,
                                                           const int32_t* __restrict__ sys,
                                                           const int32_t* __restrict__ role,
                                                           const double* __restrict__ params, hvp::Consts C,
                                                           const int8_t* __restrict__ seq,
                                                           int32_t* __restrict__ state, double* __restrict__ u_out,
                                                           double* __restrict__ x, double* __restrict__ xf,
                                                           double* __restrict__ xb, double* __restrict__ cost_out,
                                                           int32_t* __restrict__ status_out,
                                                           uint32_t* __restrict__ edge_out,
                                                           int32_t* __restrict__ iters_out,
                                                           unsigned long long* __restrict__ counter,
                                                           int32_t* __restrict__ redo) {
    constexpr int BS = kBnbBlock<N>;
    const int b = blockIdx.x * BS + threadIdx.x;
    if (b >= P * m) return;
    const int p = b / m;
    if (!(state[p] & 1)) return;
    const hvp_system& S = systems[sys[b]];
    const int rl = role[b];
    const double* prm = params + (size_t)b * C.stride;
    const uint64_t code = gadmm_code<N>(seq, b);
    hvp::LaneQp<N, LdsMem<N, BS>> q;
    q.mem.lane = threadIdx.x;
    int it = 0;
    uint32_t raw = 0;
    const int cap = C.leaf_cap > 0 ? C.leaf_cap : kGiMaxIter<N>;  // HVP_LEAF_GI_CAP: tests of k_gadmm_ipm
    const int st = hvp::solve_admm_lane<N>(q, S, C, rl, prm, code, N, cap, it, &raw);
    if (iters_out) iters_out[b] = it;
    atomicAdd(&counter[1], (unsigned long long)it);
    if (st == hvp::GI_OK) {
        cost_out[b] = hvp::admm_direct_cost<N>(q, S, C, rl, prm, code, N);
        status_out[b] = HVP_OPTIMAL;
        edge_out[b] = gadmm_edges<N>(S, code, raw);
        gadmm_write<N>(b, gadmm_slot(b, n, lo, m), S, C, rl, prm, code, q.y, u_out, x, xf, xb);
    } else {
        gadmm_redo(b, counter, redo);
    }
}

// x-update, one 16-lane group per local QP (long horizons, hvp_coop.h)
template <int N>
__global__ __launch_bounds__(kCoopBlock) HVP_COOP_OCC void k_gadmm_qp_coop(int P, int n, int lo, int m,
                                                              const hvp_system* __restrict__ systems,
                                                              const int32_t* __restrict__ sys,
                                                              const int32_t* __restrict__ role,
                                                              const double* __restrict__ params, hvp::Consts C,
                                                              const int8_t* __restrict__ seq,
                                                              int32_t* __restrict__ state, double* __restrict__ u_out,
                                                              double* __restrict__ x, double* __restrict__ xf,
                                                              double* __restrict__ xb, double* __restrict__ cost_out,
                                                              int32_t* __restrict__ status_out,
                                                              uint32_t* __restrict__ edge_out,
                                                              int32_t* __restrict__ iters_out,
                                                              unsigned long long* __restrict__ counter,
                                                              hvp::coop::WarmQp* __restrict__ warm_ws, int warm,
                                                              int32_t* __restrict__ redo) {
    __shared__ hvp::coop::GroupLds lds[kCoopGroups];
    const int g = threadIdx.x / hvp::coop::G, t = threadIdx.x % hvp::coop::G;
    const int b = blockIdx.x * kCoopGroups + g;
    if (b >= P * m) return;  // group-uniform
    const int p = b / m;
    if (!(state[p] & 1)) return;
    const hvp_system& S = systems[sys[b]];
    const int rl = role[b];
    const double* prm = params + (size_t)b * C.stride;
    const uint64_t code = gadmm_code<N>(seq, b);
    hvp::coop::Lane<N> L;
    double cost = 0.0;
    int it = 0;
    unsigned raw = 0;
    const int cap = C.leaf_cap > 0 ? C.leaf_cap : kGiMaxIter<N>;  // HVP_LEAF_GI_CAP: tests of k_gadmm_ipm
    const int st = hvp::coop::solve_qp<N>(L, lds[g], S, C, rl, prm, code, N, cap, it, &cost, &raw, 0.0,
                                          -1.0, warm_ws ? warm_ws + b : nullptr, warm != 0,
                                          ((uint64_t)(uint32_t)sys[b] << 32) | (uint32_t)rl);
    if (st == hvp::GI_OK) {
        lds[g].v[t] = t < N ? L.y : 0.0;
        hvp::coop::gsync();
    }
    if (t != 0) return;
    if (iters_out) iters_out[b] = it;
    atomicAdd(&counter[1], (unsigned long long)it);
    if (st == hvp::GI_OK) {
        double y[N];
#pragma unroll
        for (int k = 0; k < N; ++k) y[k] = lds[g].v[k];
        cost_out[b] = cost;
        status_out[b] = HVP_OPTIMAL;
        edge_out[b] = gadmm_edges<N>(S, code, raw);
        gadmm_write<N>(b, gadmm_slot(b, n, lo, m), S, C, rl, prm, code, y, u_out, x, xf, xb);
    } else {
        gadmm_redo(b, counter, redo);
    }
}

// Local QPs the active-set method failed on (k_gadmm_qp / _coop put them on the redo list):
// re-solved by the interior point inside the hinge-state iteration (hvp_admm.h solve_admm_ipm),
// one lane per QP.  Only a QP that fails here too fails its platoon (gadmm_fail), as a qpOASES
// failure fails the reference's local solve (fleet_g_admm.py:162,195-205).  Normally an empty list.
template <int N>
__global__ __launch_bounds__(kBnbBlock<N>) void k_gadmm_ipm(int P, int n, int lo, int m,
                                                            const hvp_system* __restrict__ systems,
                                                            const int32_t* __restrict__ sys,
                                                            const int32_t* __restrict__ role,
                                                            const double* __restrict__ params, hvp::Consts C,
                                                            const int8_t* __restrict__ seq,
                                                            int32_t* __restrict__ state, double* __restrict__ u_out,
                                                            double* __restrict__ x, double* __restrict__ xf,
                                                            double* __restrict__ xb, double* __restrict__ cost_out,
                                                            int32_t* __restrict__ status_out,
                                                            uint32_t* __restrict__ edge_out,
                                                            int32_t* __restrict__ iters_out,
                                                            unsigned long long* __restrict__ counter,
                                                            const int32_t* __restrict__ redo) {
    constexpr int BS = kBnbBlock<N>;
    const unsigned long long nr = counter[3];
    const long long total = (long long)(nr < (unsigned long long)P * m ? nr : (unsigned long long)P * m);
    for (long long i = (long long)blockIdx.x * BS + threadIdx.x; i < total; i += (long long)gridDim.x * BS) {
        const int b = redo[i];
        const int p = b / m;
        const hvp_system& S = systems[sys[b]];
        const int rl = role[b];
        const double* prm = params + (size_t)b * C.stride;
        const uint64_t code = gadmm_code<N>(seq, b);
        hvp::LaneQp<N, LdsMem<N, BS>> q;
        q.mem.lane = threadIdx.x;
        int it = 0;
        uint32_t raw = 0;
        const int st = hvp::solve_admm_ipm<N>(q, S, C, rl, prm, code, N, it, &raw);
        if (iters_out) iters_out[b] += it;
        atomicAdd(&counter[1], (unsigned long long)it);
        if (st == hvp::GI_OK) {
            cost_out[b] = hvp::admm_direct_cost<N>(q, S, C, rl, prm, code, N);
            status_out[b] = HVP_OPTIMAL;
            edge_out[b] = gadmm_edges<N>(S, code, raw);
            gadmm_write<N>(b, gadmm_slot(b, n, lo, m), S, C, rl, prm, code, q.y, u_out, x, xf, xb);
        } else {
            cost_out[b] = 1e300;
            status_out[b] = HVP_MAXITER;
            edge_out[b] = 0;
            gadmm_fail(state, p);
        }
    }
}

inline int grid_for(long long n) { return (int)std::max<long long>(1, (n + kBlock - 1) / kBlock); }

// The naive-ADMM node records of the 16-lane path (node_index): HVP_ADMM_NODE_SLOTS records per
// (instance, depth), a power of two (default 256; 0: none), allocated for the reserve's batch at
// the first solve that needs them (hipMalloc outside any capture: the ADMM engine's first
// iteration) and zeroed (no record valid, no claim).  Each solve takes the next epoch, so the claims
// of the previous solve lose to every claim of this one; at the epoch counter's wrap the claims
// are cleared.  The slot count is halved (down to 16) until the table fits in half of the free HBM;
// an allocation that still fails only turns the records off (a cold start for every node) and is
// not tried again until the slot request or the batch grows.
template <int N>
hipError_t node_records(hvp_handle* h, int B, Workspace& ws) {
    const char* e = std::getenv("HVP_ADMM_NODE_SLOTS");
    int want = e && e[0] ? std::atoi(e) : 256;
    int req = 0;
    if (want > 0) {
        req = 1;
        while (req < want && req < (1 << 16)) req <<= 1;
    }
    const long long batch = std::max<long long>(B, h->ws.max_batch);
    if (req != h->nrec_want || (req && batch > h->nrec_batch)) {
        hipError_t err = hipDeviceSynchronize();
        if (err != hipSuccess) return err;
        (void)hipFree(h->nrec);
        (void)hipFree(h->nclaim);
        h->nrec = nullptr;
        h->nclaim = nullptr;
        h->nrec_want = req;
        h->nrec_batch = req ? batch : 0;  // also on failure: one attempt per request / batch size
        h->nrec_epoch = 0;
        constexpr size_t per = sizeof(hvp::coop::WarmRec<N>) + sizeof(unsigned long long);
        int slots = req;
        size_t free_b = 0, total_b = 0;
        if (slots && hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            while (slots > 16 && (size_t)batch * (N + 1) * slots * per > free_b / 2) slots >>= 1;
        h->nrec_slots = slots;
        if (slots) {
            const size_t n = (size_t)batch * (N + 1) * slots;
            if (hipMalloc(&h->nrec, n * sizeof(hvp::coop::WarmRec<N>)) == hipSuccess &&
                hipMalloc(&h->nclaim, n * sizeof(unsigned long long)) == hipSuccess &&
                hipMemset(h->nrec, 0, n * sizeof(hvp::coop::WarmRec<N>)) == hipSuccess &&
                hipMemset(h->nclaim, 0, n * sizeof(unsigned long long)) == hipSuccess) {
                if (slots < req)
                    std::fprintf(stderr, "[hvp] naive-ADMM node records: %d of %d slots per node fit the free HBM\n",
                                 slots, req);
            } else {
                (void)hipGetLastError();
                (void)hipFree(h->nrec);
                (void)hipFree(h->nclaim);
                h->nrec = nullptr;
                h->nclaim = nullptr;
                h->nrec_slots = 0;
                std::fprintf(stderr, "[hvp] naive-ADMM node records: %zu bytes not available, cold starts\n",
                             n * per);
            }
        }
    }
    const int slots = h->nrec_slots;
    if (!h->nrec || !h->nrec_enable) return hipSuccess;
    if (++h->nrec_epoch > 0xFFFFull) {
        hipError_t err = hipDeviceSynchronize();  // (a solve in flight may still claim)
        if (err != hipSuccess) return err;
        err = hipMemset(h->nclaim, 0, (size_t)h->nrec_batch * (N + 1) * slots * sizeof(unsigned long long));
        if (err != hipSuccess) return err;
        h->nrec_epoch = 1;
    }
    ws.nrec = h->nrec;
    ws.nclaim = h->nclaim;
    ws.nslots = slots;
    ws.ndepth = N + 1;
    ws.nepoch = h->nrec_epoch << 48;
    const char* no = std::getenv("HVP_ADMM_NODE_ORDER");  // 0: the list order (A/B)
    ws.norder = !(no && no[0] == '0');
    return hipSuccess;
}

// The descriptor of the dive list as a level-N list: ws with the dive's arrays, counts and claims
// in place of level N's, one bucket of `cap` slots (launch_bnb: the quadratic and the LP search).
inline Workspace dive_list_ws(const Workspace& ws, int N, long long cap) {
    Workspace wd = ws;
    wd.nd_inst[N & 1] = ws.dv_inst;
    wd.nd_code[N & 1] = ws.dv_code;
    wd.nd_lo[N & 1] = ws.dv_lo;
    wd.nd_hi[N & 1] = ws.dv_hi;
    wd.nd_lb[N & 1] = ws.dv_lb;
    wd.leaf_stat = ws.dv_stat;
    wd.task_y = ws.dv_y;
    wd.redo = ws.dv_redo;
    wd.lvl = ws.dv_lvl;
    wd.counter = ws.dv_counter;
    wd.cap = cap;
    wd.split = 1;
    wd.split_shift = 0;
    return wd;
}

// one launch of the refill kernel over level k's list of `ws` (the level lists, or dive_list_ws).
// The instantiation that stages the system tables in LDS when the handle's systems fit its cap,
// else the one that reads them from global memory; and, with `phases`, the one of the level's
// phase (k_bnb_bound_refill: RP_LEAF at k == N, RP_UPPER at k + 1 < N; level N - 1, and every
// level without `phases`, RP_ANY).
template <int N, bool STAGE>
void launch_refill_ph(hvp_handle* h, int grid, size_t lds, hipStream_t st, int k, const int32_t* sys,
                      const int32_t* role, const double* params, const Workspace& ws, bool phases) {
    constexpr int BS = kBnbBlock<N>;
    if constexpr (kRefillPhLeaf<N, STAGE>) {
        if (phases && k == N) {
            hipLaunchKernelGGL((k_bnb_bound_refill<N, STAGE, RP_LEAF>), dim3(grid), dim3(BS), lds, st, k, h->d_sys,
                               h->n_systems, sys, role, params, h->C, ws);
            return;
        }
    }
    if constexpr (kRefillPhUpper<N, STAGE>) {
        if (phases && k + 1 < N) {
            hipLaunchKernelGGL((k_bnb_bound_refill<N, STAGE, RP_UPPER>), dim3(grid), dim3(BS), lds, st, k, h->d_sys,
                               h->n_systems, sys, role, params, h->C, ws);
            return;
        }
    }
    hipLaunchKernelGGL((k_bnb_bound_refill<N, STAGE, RP_ANY>), dim3(grid), dim3(BS), lds, st, k, h->d_sys,
                       h->n_systems, sys, role, params, h->C, ws);
}
template <int N>
void launch_refill(hvp_handle* h, int grid, size_t lds, hipStream_t st, int k, const int32_t* sys,
                   const int32_t* role, const double* params, const Workspace& ws, bool phases) {
    if (h->n_systems <= kRefillSysCap) return launch_refill_ph<N, true>(h, grid, lds, st, k, sys, role, params, ws, phases);
    launch_refill_ph<N, false>(h, grid, lds, st, k, sys, role, params, ws, phases);
}

template <int N>
int launch_bnb(hvp_handle* h, int B, const int32_t* sys, const int32_t* role, const double* params, double* u_out,
               double* x_out, int8_t* region_out, int8_t* gear_out, double* cost_out, int32_t* status_out,
               int32_t* nodes_out, int32_t* iters_out, hipStream_t st, double* xf_out = nullptr,
               double* xb_out = nullptr) {
    Workspace ws = h->ws;
    constexpr int BS = kBnbBlock<N>;
    // the decentralised lane path generates every level's nodes inside k_bnb_root / the bound
    // kernel of the level above (fused expand) and keeps each level in two halves (LevelList);
    // the other paths run k_bnb_expand per level over one list
    const bool fused = !kCoop<N> && h->C.form == HVP_FORM_DECENT && !h->C.l1;
    if constexpr (kCoop<N> && N <= 12) {
        if (h->C.form == HVP_FORM_ADMM && !h->C.l1) HIP_TRY(node_records<N>(h, B, ws));
    }
    const char* sp = std::getenv("HVP_SPLIT_LEVELS");  // buckets per level list: 1 (one list), 2, 4 (A/B runs)
    const int want = sp && sp[0] ? std::atoi(sp) : kDefaultBuckets;
    ws.split = fused ? (want >= 4 ? 4 : (want >= 2 ? 2 : 1)) : 1;
    ws.split_shift = ws.split == 4 ? 2 : (ws.split == 2 ? 1 : 0);
    h->last_split = ws.split;
    // pass-through nodes (bnb_put_children): off by default -- 12 % fewer QPs at C2 but no faster,
    // in any of three forms (a pass node holding its lane for a generation; finished inside the
    // claim; compacted out of the level by a pre-pass kernel): profiles/r06n, r06w, r06x.
    // HVP_PASS_THROUGH=1 turns them on
    const char* pt = std::getenv("HVP_PASS_THROUGH");
    ws.pass = pt && pt[0] == '1';
    // the root level and the dives' leaves through the refill kernel (below); HVP_ROOT_REFILL=0
    // selects k_bnb_root (A/B), and so does a workspace that cannot hold the root level (one list
    // whatever the split, level_list: a capacity that fits the tree with one list per level fits it
    // with buckets too, which k_bnb_root's tree, with the dive's leaf listed again, need not)
    const char* rr = std::getenv("HVP_ROOT_REFILL");
    const bool root_refill = fused && !(rr && rr[0] == '0') && ws.dv_mem &&
                             (unsigned long long)ws.cap >= (unsigned long long)B;
    // The dive's leaf is a level-N node of the tree (its ancestors are never pruned), and level N
    // solved it a second time: 163,840 of 2,069,224 QPs per flagship step, all in the longest
    // launch.  With the dive list present the refill event at level N - 1 leaves that child out
    // and the dive entry takes its place in the tie rule and the counts (k_bnb_bound_refill,
    // k_bnb_key).  HVP_DIVE_REUSE=0: every leaf of level N is solved there (A/B)
    const char* dr = std::getenv("HVP_DIVE_REUSE");
    ws.reuse = root_refill && !(dr && dr[0] == '0');
    h->last_reuse = ws.reuse != 0;
    // the refill kernel's instantiation by the level's phase (launch_refill); HVP_REFILL_PHASES=0:
    // every launch through the one kernel for all levels (A/B, tests)
    const char* rp = std::getenv("HVP_REFILL_PHASES");
    const bool phases = !(rp && rp[0] == '0');
    HIP_TRY(hipMemsetAsync(ws.counter, 0, 8 * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(ws.lvl, 0, (2 + kMaxBuckets) * (HVP_MAX_N + 1) * sizeof(unsigned long long), st));  // + claims, buckets
    if (ws.dv_counter) HIP_TRY(hipMemsetAsync(ws.dv_counter, 0, 8 * sizeof(unsigned long long), st));
    HIP_TRY(hipEventRecord(h->ev0, st));
    HIP_TRY(hipEventRecord(h->evq0, st));
    const size_t lds = sizeof(double) * hvp::F_COUNT * N * BS;
    HIP_TRY(hipEventRecord(h->evb[0], st));
    const int g_l1 = std::max(1, h->n_cu) * (N <= HVP_MAX_N_ENUM ? 8 : 16);  // waves grid-stride over nodes
    // min_1_norm: the per-lane simplex up to N = 8 (HVP_L1_SIMPLEX=0: the wave interior point, A/B)
    const char* lsx = std::getenv("HVP_L1_SIMPLEX");
    const bool lp_lane = h->C.l1 && h->C.form == HVP_FORM_DECENT && !kCoop<N> && !(lsx && lsx[0] == '0');
    const bool l1_admm = h->C.l1 && h->C.form == HVP_FORM_ADMM;  // copies in the wave interior point
    const size_t lds_lp = sizeof(double) * hvp::LF_COUNT * N * BS;
    // the node LPs through persistent waves (k_lp_bound_refill, one 256-lane block per CU: the
    // simplex kernels run one wave per SIMD), refilled when this many lanes are free
    const char* lrf = std::getenv("HVP_LP_REFILL");
    const int lp_refill_min = lrf && lrf[0] ? std::max(0, std::min(64, std::atoi(lrf))) : 12;  // (r05c sweep)
    // lanes that wait for a rebuild of A_B^-1 before the wave runs one (k_lp_bound_refill)
    const char* lib_ = std::getenv("HVP_LP_INV_BATCH");
    const int lp_inv_batch = lib_ && lib_[0] ? std::max(1, std::min(64, std::atoi(lib_))) : kLpInvBatch;
    const int lp_refill = lp_refill_min > 0 ? lp_refill_min | (lp_inv_batch << 8) : 0;
    const int g_lp = (int)std::min<long long>((h->ws.cap + BS - 1) / BS, (long long)std::max(1, h->n_cu));
    if (lp_lane) {
        if constexpr (!kCoop<N>) {
            // root level and the incumbent dives through the LP refill kernel (k_lp_root solves
            // root + up to 3 dive leaves one after another per lane: HVP_LP_ROOT_REFILL=0, A/B)
            const char* lrr = std::getenv("HVP_LP_ROOT_REFILL");
            const bool lp_root_refill = lp_refill > 0 && !(lrr && lrr[0] == '0') && ws.dv_mem;
            if (lp_root_refill) {
                const Workspace wd = dive_list_ws(ws, N, 3LL * ws.max_batch);
                hipLaunchKernelGGL(k_lp_root_init<N>, dim3(grid_for(B)), dim3(kBlock), 0, st, B, h->d_sys, sys, params,
                                   h->C, ws);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(k_lp_bound_refill<N>, dim3(g_lp), dim3(BS), lds_lp, st, 0, h->d_sys, sys, role,
                                   params, h->C, ws, lp_refill);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(k_lp_dive_prep<N>, dim3(grid_for(B)), dim3(kBlock), 0, st, B, h->d_sys, sys, params,
                                   h->C, ws);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(k_lp_bound_refill<N>, dim3(g_lp), dim3(BS), lds_lp, st, N, h->d_sys, sys, role,
                                   params, h->C, wd, lp_refill);
            } else {
                hipLaunchKernelGGL(k_lp_root<N>, dim3((B + kLpRootBlock - 1) / kLpRootBlock), dim3(kLpRootBlock),
                                   sizeof(double) * hvp::LF_COUNT * N * kLpRootBlock, st, B, h->d_sys, sys, role,
                                   params, h->C, ws);
            }
        }
    } else if (h->C.l1) {
        if (l1_admm)
            hipLaunchKernelGGL((k_l1_root<N, true>), dim3(g_l1 * kL1BlockOf<N> / kL1BlockOfA<N, true>), dim3(kL1BlockOfA<N, true>), 0, st, B, h->d_sys, sys, role, params,
                               h->C, ws);
        else
            hipLaunchKernelGGL((k_l1_root<N, false>), dim3(g_l1), dim3(kL1BlockOf<N>), 0, st, B, h->d_sys, sys, role,
                               params, h->C, ws);
    } else if constexpr (kCoop<N>) {
        // the roots, then their incumbent leaves as a list (k_bnb_leaf_coop; HVP_COOP_LEAF_LIST=0: each
        // root's group solves its leaves right after it, A/B); the list needs 2 B slots of level 1
        const char* ll = std::getenv("HVP_COOP_LEAF_LIST");
        const int leaf_list = !(ll && ll[0] == '0') && ws.cap >= 2LL * B ? 1 : 0;
        hipLaunchKernelGGL(k_bnb_root_coop<N>, dim3((B + kCoopGroups - 1) / kCoopGroups), dim3(kCoopBlock), 0, st, B,
                           h->d_sys, sys, role, params, h->C, ws, leaf_list);
        if (leaf_list) {
            HIP_TRY(hipGetLastError());
            const int g_leaf = (int)std::min<long long>((2LL * B + kCoopGroups - 1) / kCoopGroups,
                                                        (long long)h->n_cu * 32);
            hipLaunchKernelGGL(k_bnb_leaf_coop<N>, dim3(g_leaf), dim3(kCoopBlock), 0, st, h->d_sys, sys, role, params,
                               h->C, ws);
        }
    } else {
        if (h->C.form == HVP_FORM_ADMM) {
            hipLaunchKernelGGL((k_bnb_root<N, true>), dim3((B + BS - 1) / BS), dim3(BS), lds, st, B, h->d_sys, sys,
                               role, params, h->C, ws);
        } else {
            // sigma-independent QP part + the root nodes once per instance
            hipLaunchKernelGGL(k_inst_prep<N>, dim3(grid_for(B)), dim3(kBlock), 0, st, B, h->d_sys, sys, role, params,
                               h->C, ws);
            HIP_TRY(hipGetLastError());
            // The root level through the refill kernel (the root QPs as level-0 nodes, their
            // children into level 1's buckets), then the greedy dives' leaves as a list of their own
            // (k_bnb_dive_prep) through the same kernel at K = N, whose costs set the incumbents.
            // The tree is k_bnb_root's: the root's children are never pruned (the root bound is <=
            // every leaf), and the dives' incumbents are in place before level 1.  The refill kernel
            // keeps every lane busy where k_bnb_root (one lane per instance, 1 wave per SIMD) waits
            // for each wave's slowest root + dive.  (root_refill: above.)
            if (root_refill) {
                const int g_root = (int)std::min<long long>((B + BS - 1) / BS, (long long)h->n_cu * kRefillBlocksPerCu);
                launch_refill<N>(h, g_root, lds, st, 0, sys, role, params, ws, phases);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(k_bnb_dive_prep<N>, dim3(grid_for(B)), dim3(kBlock), 0, st, B, h->d_sys, sys, params,
                                   h->C, ws);
                HIP_TRY(hipGetLastError());
                launch_refill<N>(h, g_root, lds, st, N, sys, role, params, dive_list_ws(ws, N, ws.max_batch), phases);
            } else {
                // (one lane per instance, 1 wave per SIMD)
                hipLaunchKernelGGL((k_bnb_root<N, false>), dim3((B + BS - 1) / BS), dim3(BS), lds, st, B, h->d_sys,
                                   sys, role, params, h->C, ws);
            }
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->evb[1], st));
    const int g_small = (int)std::min<long long>(grid_for(h->ws.cap), (long long)h->n_cu * 8);
    const int g_qp = (int)std::min<long long>((h->ws.cap + BS - 1) / BS, (long long)h->n_cu * 8 * (kBlock / BS));
    for (int k = 1; k <= N; ++k) {
        if (!fused)
            hipLaunchKernelGGL(k_bnb_expand<N>, dim3(g_small), dim3(kBlock), 0, st, k, h->d_sys, sys, h->C, ws);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(h->evb[2 * k], st));
        if (lp_lane) {
            if constexpr (!kCoop<N>) {
                if (lp_refill > 0)
                    hipLaunchKernelGGL(k_lp_bound_refill<N>, dim3(g_lp), dim3(BS), lds_lp, st, k, h->d_sys, sys, role,
                                       params, h->C, ws, lp_refill);
                else
                    hipLaunchKernelGGL(k_lp_bound<N>, dim3(g_qp), dim3(BS), lds_lp, st, k, h->d_sys, sys, role, params,
                                       h->C, ws);
            }
        } else if (h->C.l1) {
            if (l1_admm)
                hipLaunchKernelGGL((k_l1_bound<N, true>), dim3(g_l1 * kL1BlockOf<N> / kL1BlockOfA<N, true>), dim3(kL1BlockOfA<N, true>), 0, st, k, h->d_sys, sys, role,
                                   params, h->C, ws);
            else {
                hipLaunchKernelGGL((k_l1_bound<N, false>), dim3(g_l1), dim3(kL1BlockOf<N>), 0, st, k, h->d_sys, sys, role,
                                   params, h->C, ws);
                HIP_TRY(hipGetLastError());
                // the level's LPs the interior point left unresolved, by the simplex (normally none)
                hipLaunchKernelGGL(k_l1_retry<N>, dim3(std::max(1, h->n_cu)), dim3(kL1RetryBlock), 0, st, k, h->d_sys,
                                   sys, role, params, h->C, ws);
            }
        } else if constexpr (kCoop<N>) {
            if (ws.norder) {
                // its counters live in rows 2M and 5M of ws.lvl, bucket 1's count row (hvp_internal.h)
                if (ws.split != 1) return fail(HVP_E_ARG, "k_node_order needs one bucket per level list");
                hipLaunchKernelGGL(k_node_order<N>, dim3(g_small), dim3(kBlock), 0, st, k, ws);
                HIP_TRY(hipGetLastError());
            }
            const int g_coop = (int)std::min<long long>((h->ws.cap + kCoopGroups - 1) / kCoopGroups,
                                                        (long long)h->n_cu * 32);
            hipLaunchKernelGGL(k_bnb_bound_coop<N>, dim3(g_coop), dim3(kCoopBlock), 0, st, k, h->d_sys, sys, role,
                               params, h->C, ws);
        } else {
            if (h->C.form == HVP_FORM_ADMM) {
                hipLaunchKernelGGL((k_bnb_bound<N, true>), dim3(g_qp), dim3(BS), lds, st, k, h->d_sys, sys, role,
                                   params, h->C, ws);
            } else {
                // persistent waves: 2 blocks per CU, every wave refills its lanes until the level is done
                const int g_refill = (int)std::min<long long>((h->ws.cap + BS - 1) / BS,
                                                              (long long)h->n_cu * kRefillBlocksPerCu);
                launch_refill<N>(h, g_refill, lds, st, k, sys, role, params, ws, phases);
            }
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(h->evb[2 * k + 1], st));
    }
    HIP_TRY(hipEventRecord(h->evq1, st));
    if (!h->C.l1 && (h->C.form == HVP_FORM_DECENT || h->C.form == HVP_FORM_ADMM)) {
        // failed leaves (normally none: reads a zero count)
        if (h->C.form == HVP_FORM_ADMM)
            hipLaunchKernelGGL((k_bnb_ipm<N, true>), dim3(std::max(1, h->n_cu)), dim3(BS), lds, st, h->d_sys, sys,
                               role, params, h->C, ws);
        else  // (a small grid: the list is normally empty, and every resident wave of this 1-wave-per-SIMD
              // kernel gets its scratch -- a full-chip grid cost 0.06 ms per solve for reading a zero count,
              // profiles/r05c_decent_n10_N5_P16384_s3_summary.json)
            hipLaunchKernelGGL((k_bnb_ipm<N, false>), dim3(std::max(1, std::min(h->n_cu, 16))), dim3(BS), lds, st,
                               h->d_sys, sys, role, params, h->C, ws);
        HIP_TRY(hipGetLastError());
    }
    const int n_dive = ws.reuse ? B : 0;  // the dive entries in the tie rule (every other form: none)
    hipLaunchKernelGGL(k_bnb_key<N>, dim3(g_small), dim3(kBlock), 0, st, ws, h->C.form, h->C.l1, n_dive);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_bnb_write<N>, dim3(g_small), dim3(kBlock), 0, st, ws, n_dive);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_bnb_finish<N>, dim3(grid_for(B)), dim3(kBlock), 0, st, B, h->d_sys, sys, role, params, h->C,
                       ws, u_out, x_out, region_out, gear_out, cost_out, status_out, nodes_out, iters_out, xf_out,
                       xb_out);
    HIP_TRY(hipGetLastError());
    if (l1_admm && (xf_out || xb_out)) {
        constexpr int wpb = kL1BlockOfA<N, true> / 64;  // waves per block, one instance per wave
        hipLaunchKernelGGL(k_l1_admm_write<N>, dim3(std::max(1, std::min((B + wpb - 1) / wpb, h->n_cu * 8 / wpb))),
                           dim3(kL1BlockOfA<N, true>), 0, st, B, h->d_sys, sys, role, params, h->C, ws, xf_out, xb_out);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(h->ev1, st));
    h->last_stream = st;
    h->last_B = B;
    h->last_bnb = true;
#ifdef HVP_REFILL_PROF
    if constexpr (N <= HVP_MAX_N_ENUM) {
        unsigned long long hist[kPfHist];
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpyFromSymbol(hist, HIP_SYMBOL(g_pf_hist), sizeof(hist)));
        std::fprintf(stderr, "[refill-hist] node trips:");
        for (int i = 0; i < 64; ++i) std::fprintf(stderr, " %llu", hist[i]);
        std::fprintf(stderr, "\n[refill-hist] generation trips:");
        for (int i = 64; i < 128; ++i) std::fprintf(stderr, " %llu", hist[i]);
        // per row id (hvp_gi.h: 6j + r, then 6N + 4m + r): scans in which the wave selects at it
        if (HVP_REFILL_PROF_ROWS) {
            std::fprintf(stderr, "\n[refill-hist] scans %llu, with a violating lane per row:", hist[128 + kPfRows]);
            for (int i = 0; i < hvp::GiConstraintSet<N>::NC; ++i) std::fprintf(stderr, " %llu", hist[128 + i]);
        }
        std::fprintf(stderr, "\n");
        std::memset(hist, 0, sizeof(hist));
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_pf_hist), hist, sizeof(hist)));
    }
#endif
    return 0;
}

template <int N>
int launch_all(hvp_handle* h, int B, const int32_t* sys, const int32_t* role, const double* params, double* u_out,
               double* x_out, int8_t* region_out, int8_t* gear_out, double* cost_out, int32_t* status_out,
               int32_t* nodes_out, int32_t* iters_out, hipStream_t st) {
    Workspace ws = h->ws;
    HIP_TRY(hipMemsetAsync(ws.counter, 0, 8 * sizeof(unsigned long long), st));
    HIP_TRY(hipEventRecord(h->ev0, st));
    hipLaunchKernelGGL(k_enum<N>, dim3(grid_for(B)), dim3(kBlock), 0, st, B, h->d_sys, sys, role, params, h->C, ws);
    HIP_TRY(hipGetLastError());
    // the candidate count is only known on the device: size the grid for the capacity bound
    // (≈ every CU x 8 blocks) and let the kernel grid-stride over the real count
    const long long want = std::min<long long>(grid_for(h->ws.cap), (long long)h->n_cu * 8);
    HIP_TRY(hipEventRecord(h->evq0, st));
    const size_t lds = sizeof(double) * hvp::F_COUNT * N * kBlock;
    const char* lsx = std::getenv("HVP_L1_SIMPLEX");
    if (h->C.l1 && !(lsx && lsx[0] == '0')) {
        // min_1_norm: the fixed-sequence LPs by the per-lane simplex (hvp_lp.h), one per lane
        constexpr int BS = kBnbBlock<N>;
        hipLaunchKernelGGL(k_qp_lp<N>, dim3((int)std::min<long long>((h->ws.cap + BS - 1) / BS, (long long)h->n_cu * 8)),
                           dim3(BS), sizeof(double) * hvp::LF_COUNT * N * BS, st, h->d_sys, sys, role, params, h->C,
                           ws);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(h->evq1, st));
    } else if (h->C.l1) {
        // min_1_norm: the fixed-sequence LPs, one per wavefront (wave grid-stride over the candidates;
        // HVP_L1_SIMPLEX=0, A/B)
        hipLaunchKernelGGL(k_qp_l1<N>, dim3(std::max(1, h->n_cu) * 8), dim3(kL1Block), 0, st, h->d_sys, sys, role,
                           params, h->C, ws);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(h->evq1, st));
    } else {
        hipLaunchKernelGGL(k_qp_gi<N>, dim3((int)want), dim3(kBlock), lds, st, h->d_sys, sys, role, params, h->C, ws);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(h->evq1, st));
        // fallback list (normally empty: the launch reads a zero count and exits)
        hipLaunchKernelGGL(k_qp_ipm<N>, dim3(std::max(1, h->n_cu)), dim3(kBlock), lds, st, h->d_sys, sys, role,
                           params, h->C, ws);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_cost<N>, dim3((int)want), dim3(kBlock), 0, st, h->d_sys, sys, role, params, h->C, ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_select<N>, dim3(grid_for(B)), dim3(kBlock), 0, st, B, h->d_sys, sys, params, ws, u_out,
                       x_out, region_out, gear_out, cost_out, status_out, nodes_out, iters_out, h->C.l1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev1, st));
    h->last_stream = st;
    h->last_B = B;
    h->last_bnb = false;
    return 0;
}

template <int N>
int launch_gadmm_qp(hvp_handle* h, int P, int n, int lo, int m, const int32_t* sys, const int32_t* role,
                           const double* params, const int8_t* seq, int32_t* state, double* u_out, double* x,
                           double* xf, double* xb, double* cost_out, int32_t* status_out, uint32_t* edge_out,
                           int32_t* iters_out, hipStream_t st) {
    const int B = P * m;
    if (B > h->gadmm_redo_cap) {  // the interior-point fallback's list (k_gadmm_ipm)
        HIP_TRY(hipDeviceSynchronize());
        (void)hipFree(h->gadmm_redo);
        h->gadmm_redo = nullptr;
        h->gadmm_redo_cap = 0;
        if (hipMalloc(&h->gadmm_redo, sizeof(int32_t) * (size_t)B) != hipSuccess)
            return fail(HVP_E_NOMEM, "hvp_gadmm_solve: device allocation failed");
        h->gadmm_redo_cap = B;
    }
    HIP_TRY(hipMemsetAsync(h->g_counter + 3, 0, sizeof(unsigned long long), st));
    HIP_TRY(hipEventRecord(h->ev0, st));  // (hvp_get_stats times ev0 -> ev1 of the last call)
    HIP_TRY(hipEventRecord(h->evq0, st));
    if constexpr (kCoop<N>) {
        // each local QP's final hinge states, active set and factors, carried from one ADMM
        // iteration to the next (hvp_coop.h WarmQp)
        if (B > h->gadmm_hs_cap) {
            HIP_TRY(hipDeviceSynchronize());
            (void)hipFree(h->gadmm_hs);
            h->gadmm_hs = nullptr;
            h->gadmm_hs_cap = 0;
            if (hipMalloc(&h->gadmm_hs, sizeof(hvp::coop::WarmQp) * (size_t)B) != hipSuccess)
                return fail(HVP_E_NOMEM, "hvp_gadmm_solve: device allocation failed");
            h->gadmm_hs_cap = B;
            h->gadmm_hs_valid = 0;
        }
        const char* wh = std::getenv("HVP_GADMM_WARM");  // "0": every QP from the cold start (A/B runs)
        const int use = h->gadmm_hs_valid && !(wh && wh[0] == '0') ? 1 : 0;
        hipLaunchKernelGGL(k_gadmm_qp_coop<N>, dim3((B + kCoopGroups - 1) / kCoopGroups), dim3(kCoopBlock), 0, st, P, n,
                           lo, m, h->d_sys, sys, role, params, h->C, seq, state, u_out, x, xf, xb, cost_out,
                           status_out, edge_out, iters_out, h->g_counter,
                           reinterpret_cast<hvp::coop::WarmQp*>(h->gadmm_hs), use, h->gadmm_redo);
        h->gadmm_hs_valid = 1;
    } else {
        constexpr int BS = kBnbBlock<N>;
        const size_t lds = sizeof(double) * hvp::F_COUNT * N * BS;
        hipLaunchKernelGGL(k_gadmm_qp<N>, dim3((B + BS - 1) / BS), dim3(BS), lds, st, P, n, lo, m, h->d_sys, sys, role,
                           params, h->C, seq, state, u_out, x, xf, xb, cost_out, status_out, edge_out, iters_out,
                           h->g_counter, h->gadmm_redo);
    }
    HIP_TRY(hipGetLastError());
    {  // failed local QPs (normally none: reads a zero count)
        constexpr int BS = kBnbBlock<N>;
        const size_t lds = sizeof(double) * hvp::F_COUNT * N * BS;
        hipLaunchKernelGGL(k_gadmm_ipm<N>, dim3(std::max(1, h->n_cu)), dim3(BS), lds, st, P, n, lo, m, h->d_sys, sys,
                           role, params, h->C, seq, state, u_out, x, xf, xb, cost_out, status_out, edge_out, iters_out,
                           h->g_counter, h->gadmm_redo);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(h->evq1, st));
    HIP_TRY(hipEventRecord(h->ev1, st));
    h->last_stream = st;
    h->last_B = B;
    h->last_bnb = false;
    return 0;
}

template <int N>
int launch_evaluate(hvp_handle* h, int B, const int32_t* sys, const int32_t* role, const double* params,
                    const int8_t* gear_in, const double* u_in, double* cost_out, int32_t* status_out, double* x_out,
                    hipStream_t st) {
    hipLaunchKernelGGL(k_evaluate<N>, dim3(grid_for(B)), dim3(kBlock), 0, st, B, h->d_sys, sys, role, params, h->C,
                       gear_in, u_in, cost_out, status_out, x_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int N>
int launch_gadmm_rollout(hvp_handle* h, int P, int n, int lo, int m, const int32_t* sys, const double* params,
                         int mode, const double* u_prev, double* x, int8_t* seq, double* u_ws, int32_t* state,
                         hipStream_t st) {
    const int B = P * m;
    hipLaunchKernelGGL(k_gadmm_rollout<N>, dim3(grid_for(B)), dim3(kBlock), 0, st, P, n, lo, m, h->d_sys, sys,
                       params, h->C.stride, mode, u_prev, x, seq, u_ws, state);
    HIP_TRY(hipGetLastError());
    return 0;
}

// One object file per horizon: every other translation unit sees only these declarations.
#define HVP_LANE_LAUNCHERS(EXT, n)                                                                                  \
    EXT template int launch_bnb<n>(hvp_handle*, int, const int32_t*, const int32_t*, const double*, double*, double*, \
                                   int8_t*, int8_t*, double*, int32_t*, int32_t*, int32_t*, hipStream_t, double*,   \
                                   double*);                                                                          \
    EXT template int launch_evaluate<n>(hvp_handle*, int, const int32_t*, const int32_t*, const double*,             \
                                        const int8_t*, const double*, double*, int32_t*, double*, hipStream_t);      \
    EXT template int launch_gadmm_rollout<n>(hvp_handle*, int, int, int, int, const int32_t*, const double*, int,    \
                                             const double*, double*, int8_t*, double*, int32_t*, hipStream_t);       \
    EXT template int launch_gadmm_qp<n>(hvp_handle*, int, int, int, int, const int32_t*, const int32_t*,             \
                                        const double*, const int8_t*, int32_t*, double*, double*, double*, double*,  \
                                        double*, int32_t*, uint32_t*, int32_t*, hipStream_t);
#define HVP_ENUM_LAUNCHER(EXT, n)                                                                                    \
    EXT template int launch_all<n>(hvp_handle*, int, const int32_t*, const int32_t*, const double*, double*, double*, \
                                   int8_t*, int8_t*, double*, int32_t*, int32_t*, int32_t*, hipStream_t);
#define HVP_FOR_LANE_N(X, EXT) X(EXT, 2) X(EXT, 3) X(EXT, 4) X(EXT, 5) X(EXT, 6) X(EXT, 7) X(EXT, 8) X(EXT, 9) \
    X(EXT, 10) X(EXT, 11) X(EXT, 12) X(EXT, 13) X(EXT, 14) X(EXT, 15) X(EXT, 16)
#define HVP_FOR_ENUM_N(X, EXT) X(EXT, 2) X(EXT, 3) X(EXT, 4) X(EXT, 5) X(EXT, 6) X(EXT, 7) X(EXT, 8)

#ifndef HVP_LANE_INST
HVP_FOR_LANE_N(HVP_LANE_LAUNCHERS, extern)
HVP_FOR_ENUM_N(HVP_ENUM_LAUNCHER, extern)
#endif

}  // namespace hvp_k
