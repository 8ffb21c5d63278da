// pt_pointwise_joint.h -- the joint predictive density of a block of data beside a pointwise fold (pt_pointwise.h) that
// was begun at the caller's data (apemost_hip_pointwise_begin_at with joint = 1): per kept chain k, whose block is the
// L = n_at[k] data the fold scores it on, the running log-sum-exp over the kept samples of
//   J_t = sum over the block of l_i(theta_t),
// so that ln mean_t exp(J_t) = m + ln(S / n) is the log predictive density of the block as a whole: what leave-block-out
// cross-validation of a series scores.  It is not the sum of the pointwise scores, and no sample dump holds its terms.
//
// The rule.  l_i is the fold's own term of datum i, PointwiseTermAt<MODEL>::at of the same parameter row, so its bits
// are the fold's.  Contraction is off and every line is one rounding.
//   lane partials   p[j] = +0.0 for j = 0 .. 63; then for i = 0, 1, ..., L - 1 in ascending order
//                     p[i % 64] = p[i % 64] + l_i;
//   the tree        six times: p[j] = p[2 j] + p[2 j + 1] for j = 0 .. (half the length) - 1;  J = p[0].
//                   This is the association of wave_allreduce_sum (pt_device.h) -- adjacent pairs, quads, octets, rows
//                   of 16, then (r0 + r1) + (r2 + r3) -- because floating-point addition commutes.
// J_t depends on L and on the terms and on nothing else: not on the grid, the piece, the calls' boundaries or the other
// kept chains' lengths.  joint_lane_partials and joint_tree_sum below state the rule for the host compiler
// (tests/joint_check.cpp); tests/kfold_ref.py restates it in numpy.
//
// The state, five words per kept chain, each equal to a sequential host loop over the kept samples whatever the calls'
// boundaries are:
//   origin[k]        J of the first sample ever accumulated;
//   sum[k], sq[k]    with d = J - origin: sum += d; sq += d * d (the product rounded, then added); the first sample
//                    takes part like every other (its d is J - J);
//   m[k], S[k]       the first sample sets m = J, S = 1; later ones are evidence_lse_step (pt_evidence.h), unchanged.
// lpd_joint[k] = m + ln(S / n) is taken on the host.  There is no filter: a non-finite term does to J, and through it to
// the five words of its own kept chain only, what IEEE arithmetic does.
//
// Two launches behind every piece of the fold (at most kPointwisePiece kept steps), on the fold's stream:
//   pointwise_joint_sum_kernel   grid (n_keep, ceil(n / rows)), one wave per workgroup, rows = joint_rows(n_par) kept
//                                samples per wave (4 where n_par <= 128).  The wave stages its parameter rows through
//                                an LDS tile, as the fold does, and walks the block 64 data at a time: a lane loads its
//                                x_i and y_i once per 64 data and evaluates the term of each of the wave's samples
//                                side by side, every sample's partial a register of its own.  wave_allreduce_sum
//                                closes each sample and lane 0 writes J[k][t], the scratch [n_keep][kPointwisePiece].
//   pointwise_joint_fold_kernel  one wave per kept chain.  The wave takes 64 samples of the piece at a time, one per
//                                lane: d, d * d and -- where none of the 64 exceeds m -- exp(J - m) are a lane's own
//                                and are computed side by side; the additions into sum, sq and S are then made in
//                                sample order from the lanes' values (v_readlane), the same in every lane.  Where a
//                                sample exceeds m the 64 are taken one by one through evidence_lse_step.  Both ways
//                                are the recurrence above, operation for operation, as in evidence_fold_kernel.
// No float atomics, plain vector loads and stores, no scratch memory.  Registers (hipcc -O3, gfx950,
// -Rpass-analysis=kernel-resource-usage): the sum kernel holds 4 partials, x, y and four curves' temporaries: 94
// (simplesin), 92 (sine3), 82 (pulse) and 102 (pulse_vrot) VGPRs, 4 or 5 waves per SIMD, where pointwise_fold_kernel
// itself has 126 and 4; the budget is the fold's, 128.  The fold kernel has 52 VGPRs.  No kernel has scratch; LDS is
// the 4 KiB tile of the sum kernel.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_device.h"
#include "pt_pointwise.h"

namespace apemost {

constexpr int kJointSide = 4; // kept samples a wave of the sum kernel evaluates side by side

// kept samples per wave of the sum kernel: what fits the LDS tile, at most kJointSide, at least 1
__host__ __device__ inline int joint_rows(int n_par) {
    const int fit = kPointwiseTile / n_par;
    return fit < 1 ? 1 : fit > kJointSide ? kJointSide : fit;
}

// the rule's first stage: the 64 lane partials of the L terms
__host__ __device__ inline void joint_lane_partials(const double *terms, int L, double *p) {
#pragma clang fp contract(off)
    for (int j = 0; j < kPointwiseWave; j++)
        p[j] = 0.0;
    for (int i = 0; i < L; i++) {
        const double t = p[i % kPointwiseWave] + terms[i];
        p[i % kPointwiseWave] = t;
    }
}

// the rule's second stage: the adjacent-pairs tree over the 64 partials (p is overwritten)
__host__ __device__ inline double joint_tree_sum(double *p) {
#pragma clang fp contract(off)
    for (int half = kPointwiseWave / 2; half >= 1; half /= 2)
        for (int j = 0; j < half; j++) {
            const double t = p[2 * j] + p[2 * j + 1];
            p[j] = t;
        }
    return p[0];
}

struct PointwiseJointArgs {
    double *J;                         // [n_keep][kPointwisePiece]: J of the piece's kept samples
    double *origin, *sum, *sq, *m, *S; // [n_keep]
};

// grid (a.n_keep, ceil(a.n / joint_rows(a.n_par))), one wave each; a: the arguments of the fold's piece
template <int MODEL>
__global__ void __launch_bounds__(kPointwiseWave) pointwise_joint_sum_kernel(PointwiseArgs a, PointwiseJointArgs q) {
#pragma clang fp contract(off)
    __shared__ double tile[kPointwiseTile];
    const int lane = threadIdx.x, k = blockIdx.x;
    const int np = a.n_par, rows = joint_rows(np);
    const int t0 = (int)blockIdx.y * rows;
    const int cnt = (int)a.n - t0 < rows ? (int)a.n - t0 : rows; // >= 1 by the grid
    const size_t w = (size_t)np + 2, stride = (size_t)a.thin * a.n_chains * w;
    const double *src = a.rows + a.skip * a.n_chains * w + (size_t)a.chains[k] * w + (size_t)t0 * stride;
    for (int e = lane; e < cnt * np; e += kPointwiseWave) {
        const int r = e / np, p = e - r * np;
        tile[e] = src[(size_t)r * stride + p];
    }
    __syncthreads();
    const int L = a.len ? a.len[k] : a.n_data;
    const double *x = a.x + (size_t)k * a.n_data, *y = a.y + (size_t)k * a.n_data;
    PointwiseTermAt<MODEL> ev;
    ev.init(a, k, 0, 0, false);
    double *out = q.J + (size_t)k * kPointwisePiece + t0;
    if (cnt == kJointSide) {
        double p[kJointSide];
#pragma unroll
        for (int j = 0; j < kJointSide; j++)
            p[j] = 0.0;
        for (int i = lane; i < L; i += kPointwiseWave) {
            ev.x = x[i];
            ev.y = y[i];
            double l[kJointSide];
#pragma unroll
            for (int j = 0; j < kJointSide; j++)
                l[j] = ev.at(tile + j * np);
#pragma unroll
            for (int j = 0; j < kJointSide; j++)
                p[j] += l[j];
        }
#pragma unroll
        for (int j = 0; j < kJointSide; j++)
            p[j] = wave_allreduce_sum(p[j]);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < kJointSide; j++)
                out[j] = p[j];
        }
    } else {
        for (int r = 0; r < cnt; r++) { // (cnt is the same in every lane)
            double p = 0.0;
            for (int i = lane; i < L; i += kPointwiseWave) {
                ev.x = x[i];
                ev.y = y[i];
                p += ev.at(tile + r * np);
            }
            p = wave_allreduce_sum(p);
            if (lane == 0)
                out[r] = p;
        }
    }
}

// grid n_keep, one wave each: folds J[k][0 .. n) in sample order; first: J[k][0] is the first sample ever
__global__ void __launch_bounds__(kPointwiseWave) pointwise_joint_fold_kernel(PointwiseJointArgs q, unsigned int n,
                                                                              int first) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, k = blockIdx.x;
    const double *J = q.J + (size_t)k * kPointwisePiece;
    double origin, m, S, sum = q.sum[k], sq = q.sq[k];
    if (first) {
        origin = J[0];
        m = origin;
        S = 1.0;
    } else {
        origin = q.origin[k];
        m = q.m[k];
        S = q.S[k];
    }
    for (unsigned int t0 = 0; t0 < n; t0 += kPointwiseWave) {
        const int cnt = n - t0 < (unsigned int)kPointwiseWave ? (int)(n - t0) : kPointwiseWave;
        const int from = first && t0 == 0 ? 1 : 0; // the first sample ever has set m and S
        const double v = lane < cnt ? J[t0 + lane] : 0.0;
        const double d = v - origin;
        const double dd = d * d;
        if (__any(lane >= from && lane < cnt && v > m)) {
            for (int r = 0; r < cnt; r++) {
                sum += read_lane(d, r);
                sq += read_lane(dd, r);
                if (r >= from)
                    evidence_lse_step(read_lane(v, r), m, S);
            }
        } else {
            const double e = exp(v - m);
            for (int r = 0; r < cnt; r++) {
                sum += read_lane(d, r);
                sq += read_lane(dd, r);
                if (r >= from)
                    S += read_lane(e, r);
            }
        }
    }
    if (lane == 0) {
        if (first)
            q.origin[k] = origin;
        q.sum[k] = sum;
        q.sq[k] = sq;
        q.m[k] = m;
        q.S[k] = S;
    }
}

} // namespace apemost
