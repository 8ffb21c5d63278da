// pt_derived.h -- on-device derived quantities: the posterior of functions of the parameters, folded from the sample
// rows [n_steps][n_chains][n_par+2] while they are still on the device.  A derived column is a small stack program
// over one row (the specification, with the opcode table, is in include/apemost_hip.h); what is accumulated per kept
// chain and column is the run summary's histogram and batch sums, the joint fold's pair counts and moments, and the
// count of non-finite values with the least and the greatest value.  Launches per staged piece of kept steps:
//   derived_gather_kernel    on the joint fold's grid (ceil(n / 2048), n_keep * n_col): the workgroup copies its
//                            column's program and the constants to LDS, every thread interprets the program for its
//                            rows and writes the value into vals[k][c][chunk] and its bin (bisected over the column's
//                            edges in LDS, summary_edge / summary_bin called and not restated) into bins[k][c][chunk];
//   derived_marginal_kernel  one workgroup per (k, c): the staged 16-bit bins into LDS counters, then into its own
//                            slice of hist with plain loads and stores; lane 0 walks the staged values in sample order
//                            for the batch sums, as summary_kernel does; a workgroup reduction gives the non-finite
//                            count, the least and the greatest value;
//   joint_pair_kernel, joint_moments_kernel (pt_joint.h), unchanged, with JointArgs.n_par = n_col.
// The interpreter keeps the top of the stack in a register and the rest in LDS as [16][256] doubles, one column of the
// array per thread: a stack indexed at run time in registers would go to scratch memory.  Every thread of a workgroup
// runs the same program, so the instruction word is made scalar (readfirstlane) and the dispatch is a scalar branch.
// No float atomics, no global atomics, contraction off.
#pragma once

#include <hip/hip_runtime.h>

#include "apemost_hip.h"
#include "pt_joint.h"

namespace apemost {

constexpr int kDerivedThreads = kJointThreads;   // the stack's row length; the gather grid is the joint fold's
constexpr int kDerivedMaxCols = APEMOST_DERIVED_MAX_COLUMNS;
constexpr int kDerivedMaxCode = APEMOST_DERIVED_MAX_CODE;
constexpr int kDerivedMaxConsts = APEMOST_DERIVED_MAX_CONSTS;
constexpr int kDerivedMaxDepth = APEMOST_DERIVED_MAX_DEPTH;
constexpr int kDerivedPass = 1024;               // values of one (k, c) staged in LDS per pass of the marginal kernel

struct DerivedProgram {
    const int *code;       // all columns' programs, one after the other
    const int *start;      // [n_col + 1]
    const double *consts;  // [n_const]
    int n_const;
    int row_par;           // the rows hold row_par + 2 values
};

struct DerivedArgs {
    JointArgs j;           // n_par = n_col; lo, hi, origin, sum: [n_col] and [n_keep][n_col]
    DerivedProgram prog;
    unsigned long long bs, left, n_closed, batch_stride; // the summary's batch rule (SummaryArgs)
    unsigned long long *hist;      // [n_keep][n_col][nbins]
    double *batch;                 // [n_keep][n_col][batch_stride]
    unsigned long long *nonfinite; // [n_keep][n_col]
    double *vmin, *vmax;           // [n_keep][n_col]
};

// The value of one program for the row x.  code and consts are in LDS; stk is this thread's column of the
// [kDerivedMaxDepth][kDerivedThreads] stack in LDS.  The program has passed apemost_hip_derived_check: no pop from an
// empty stack, at most kDerivedMaxDepth values, one value left.  Slot 0 of the column receives the meaningless `top` of
// the first push, so that a push never branches; the deepest program's 15 values under its top fill slots 1 .. 15.
__device__ inline double derived_run(const int *code, int len, const double *consts, const double *x, double *stk) {
#pragma clang fp contract(off)
    double top = 0;
    int sp = 0;
    for (int pc = 0; pc < len; pc++) {
        const int ins = __builtin_amdgcn_readfirstlane(code[pc]);
        const int arg = (int)((unsigned int)ins >> 8);
        switch (ins & 255) {
        case APEMOST_DERIVED_COL:
            stk[sp++ * kDerivedThreads] = top;
            top = x[arg];
            break;
        case APEMOST_DERIVED_CONST:
            stk[sp++ * kDerivedThreads] = top;
            top = consts[arg];
            break;
        case APEMOST_DERIVED_DUP:
            stk[sp++ * kDerivedThreads] = top;
            break;
        case APEMOST_DERIVED_SWAP: {
            const double b = stk[(sp - 1) * kDerivedThreads];
            stk[(sp - 1) * kDerivedThreads] = top;
            top = b;
            break;
        }
        case APEMOST_DERIVED_ADD: top = stk[--sp * kDerivedThreads] + top; break;
        case APEMOST_DERIVED_SUB: top = stk[--sp * kDerivedThreads] - top; break;
        case APEMOST_DERIVED_MUL: top = stk[--sp * kDerivedThreads] * top; break;
        case APEMOST_DERIVED_DIV: top = stk[--sp * kDerivedThreads] / top; break;
        case APEMOST_DERIVED_NEG: top = -top; break;
        case APEMOST_DERIVED_ABS: top = fabs(top); break;
        case APEMOST_DERIVED_INV: top = 1.0 / top; break;
        case APEMOST_DERIVED_SQRT: top = sqrt(top); break;
        case APEMOST_DERIVED_FLOOR: top = floor(top); break;
        case APEMOST_DERIVED_MIN: {
            const double b = stk[--sp * kDerivedThreads];
            top = b < top ? b : top;
            break;
        }
        case APEMOST_DERIVED_MAX: {
            const double b = stk[--sp * kDerivedThreads];
            top = b > top ? b : top;
            break;
        }
        case APEMOST_DERIVED_LOG: top = log(top); break;
        case APEMOST_DERIVED_EXP: top = exp(top); break;
        case APEMOST_DERIVED_SIN: top = sin(top); break;
        case APEMOST_DERIVED_COS: top = cos(top); break;
        case APEMOST_DERIVED_ATAN2: top = atan2(stk[--sp * kDerivedThreads], top); break;
        default: break; // (derived_check admits no other opcode)
        }
    }
    return top;
}

// the workgroup's copy of column c's program and of the constants; returns the program's length.  A barrier follows
// at the caller.
__device__ inline int derived_load_program(const DerivedProgram &p, int c, int *code, double *consts) {
    const int s0 = p.start[c], len = p.start[c + 1] - s0;
    for (int i = threadIdx.x; i < len; i += kDerivedThreads)
        code[i] = p.code[s0 + i];
    for (int i = threadIdx.x; i < p.n_const; i += kDerivedThreads)
        consts[i] = p.consts[i];
    return len;
}

// grid (ceil(n / kJointGatherPer), n_keep * n_col): consecutive threads write consecutive slots of one column
__global__ void __launch_bounds__(kDerivedThreads) derived_gather_kernel(DerivedArgs d) {
#pragma clang fp contract(off)
    __shared__ double stack[kDerivedMaxDepth * kDerivedThreads];
    __shared__ double edges[kJointMaxBins + 1];
    __shared__ double consts[kDerivedMaxConsts];
    __shared__ int code[kDerivedMaxCode];
    const JointArgs &a = d.j;
    const int t = threadIdx.x;
    const int kc = blockIdx.y, k = kc / a.n_par, c = kc - k * a.n_par;
    const int len = derived_load_program(d.prog, c, code, consts);
    const double lo = a.lo[c], hi = a.hi[c];
    for (int b = t; b <= a.nbins; b += kDerivedThreads)
        edges[b] = summary_edge(lo, hi, b, a.nbins);
    __syncthreads();
    const int w = d.prog.row_par + 2;
    const size_t row = (size_t)a.n_chains * w;
    const double *src = a.rows + a.skip * row + (size_t)a.chains[k] * w;
    const size_t stride = (size_t)a.thin * row;
    double *vals = a.vals + (size_t)kc * a.chunk;
    unsigned short *bins = a.bins + (size_t)kc * a.chunk;
    const unsigned int i0 = blockIdx.x * (unsigned int)kJointGatherPer;
    for (unsigned int r = t; r < (unsigned int)kJointGatherPer; r += kDerivedThreads) {
        const unsigned int i = i0 + r;
        if (i >= a.n)
            break;
        const double v = derived_run(code, len, consts, src + i * stride, stack + t);
        const int b = summary_bin(v, edges, a.nbins);
        vals[i] = v;
        bins[i] = b < 0 ? kJointNoBin : (unsigned short)b;
        if (a.first && i == 0)
            a.origin[kc] = v;
    }
}

// the lesser and the greater of two values that are not NaN, -0.0 below +0.0: the order of a reduction cannot
// change a bit of the result
__device__ inline double derived_lesser(double a, double b) { return (b < a || (b == a && signbit(b))) ? b : a; }
__device__ inline double derived_greater(double a, double b) { return (b > a || (b == a && !signbit(b))) ? b : a; }

// grid (n_keep * n_col)
__global__ void __launch_bounds__(kDerivedThreads) derived_marginal_kernel(DerivedArgs d) {
#pragma clang fp contract(off)
    __shared__ unsigned int cell[kJointMaxBins];
    __shared__ double pass[kDerivedPass];
    __shared__ double red_min[kDerivedThreads], red_max[kDerivedThreads];
    __shared__ unsigned int red_bad[kDerivedThreads];
    const JointArgs &a = d.j;
    const int t = threadIdx.x;
    const int kc = blockIdx.x;
    const double *vals = a.vals + (size_t)kc * a.chunk;
    const unsigned short *bins = a.bins + (size_t)kc * a.chunk;
    for (int b = t; b < a.nbins; b += kDerivedThreads)
        cell[b] = 0;
    double *batch = d.batch + (size_t)kc * d.batch_stride;
    unsigned long long nb = d.n_closed, left = d.left;
    double part = 0;
    if (t == 0)
        part = batch[nb];
    double mn = INFINITY, mx = -INFINITY;
    unsigned int bad = 0;
    __syncthreads();
    for (unsigned int i0 = 0; i0 < a.n; i0 += kDerivedPass) {
        const int len = a.n - i0 < (unsigned int)kDerivedPass ? (int)(a.n - i0) : kDerivedPass;
        for (int i = t; i < len; i += kDerivedThreads) {
            const double v = vals[i0 + i];
            const unsigned int b = bins[i0 + i];
            pass[i] = v;
            if (b != kJointNoBin)
                atomicAdd(&cell[b], 1u);
            if (!isfinite(v))
                bad++;
            if (v == v) {
                mn = derived_lesser(mn, v);
                mx = derived_greater(mx, v);
            }
        }
        __syncthreads();
        if (t == 0) {
            // batch_means_error(): batchsum += v; a batch closes after its last sample
            for (int i = 0; i < len; i++) {
                part += pass[i];
                if (--left == 0) {
                    batch[nb++] = part;
                    part = 0;
                    left = d.bs;
                }
            }
        }
        __syncthreads(); // pass is rewritten
    }
    if (t == 0)
        batch[nb] = part; // the open batch
    red_min[t] = mn;
    red_max[t] = mx;
    red_bad[t] = bad;
    __syncthreads();
    for (int h = kDerivedThreads / 2; h > 0; h >>= 1) {
        if (t < h) {
            red_min[t] = derived_lesser(red_min[t], red_min[t + h]);
            red_max[t] = derived_greater(red_max[t], red_max[t + h]);
            red_bad[t] += red_bad[t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        d.vmin[kc] = derived_lesser(d.vmin[kc], red_min[0]);
        d.vmax[kc] = derived_greater(d.vmax[kc], red_max[0]);
        d.nonfinite[kc] += red_bad[0];
    }
    unsigned long long *hist = d.hist + (size_t)kc * a.nbins;
    for (int b = t; b < a.nbins; b += kDerivedThreads)
        hist[b] += cell[b]; // this workgroup's slice alone
}

// grid (ceil(n / kDerivedThreads), n_col): out[i][c] = column c's program on rows[i][0 .. row_par+1]
__global__ void __launch_bounds__(kDerivedThreads) derived_eval_kernel(DerivedProgram p, int n_col, unsigned int n,
                                                                       const double *rows, double *out) {
#pragma clang fp contract(off)
    __shared__ double stack[kDerivedMaxDepth * kDerivedThreads];
    __shared__ double consts[kDerivedMaxConsts];
    __shared__ int code[kDerivedMaxCode];
    const int t = threadIdx.x, c = blockIdx.y;
    const int len = derived_load_program(p, c, code, consts);
    __syncthreads();
    const unsigned int i = blockIdx.x * (unsigned int)kDerivedThreads + t;
    if (i >= n)
        return;
    out[(size_t)i * n_col + c] = derived_run(code, len, consts, rows + (size_t)i * (p.row_par + 2), stack + t);
}

} // namespace apemost
