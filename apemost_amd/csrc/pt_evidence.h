// pt_evidence.h -- on-device evidence fold: what the thermodynamic-integration and stepping-stone estimators of
// ln p(D|M,I) need from column n_par+1 (v = beta * loglike) of EVERY chain, folded from the sample rows
// [n_steps][n_chains][n_par+2] while they are still on the device.  Per chain c, each equal to a sequential host loop
// over the kept samples, whatever the calls' boundaries are:
//   origin[c]          v of the first sample ever accumulated;
//   sum[c], sq[c]      with d = v - origin[c]: sum += d and sq += d * d (the product rounded, then added), the moments
//                      about a fixed origin of pt_joint.h;
//   batch[c][k]        batch sums of v under the closing rule of the summary's batch sums (pt_summary.h): sample n,
//                      counted from 1, closes a batch when n % bs == bs - 1; slot n_batches holds the open batch;
//   m[s][c], S[s][c]   for s = 0 (up), 1 (down) a running log-sum-exp of x = a[s][c] * v (one rounded multiply; the
//                      host supplies the coefficients, the kernels never see a beta): the first sample sets m = x,
//                      S = 1; later ones  if (x > m) { S = S * exp(m - x) + 1; m = x; } else S += exp(x - m);
//                      ln mean exp(x) = m + ln(S / n) is taken on the host.  exp is the device library's fp64 exp.
// Two launches per piece of kept steps:
//   evidence_gather_kernel  reads the rows once: column n_par+1 of the kept steps of every chain goes into
//                           vals[i][c], step-major.  Unlike pt_joint.h's vals[k][p][chunk] the chain is the fastest index:
//                           here every chain is kept and the fold gives consecutive lanes consecutive chains, so both
//                           the gather's stores and the fold's loads are whole cache lines per wave instruction, where
//                           a column per chain would have every lane of a load on a line of its own;
//   evidence_fold_kernel    grid (ceil(n_chains / 64), 5): one thread per (chain, quantity), the quantity uniform over
//                           the workgroup (one wave), so no wave diverges on it.  The five quantities of a chain -- sum,
//                           sq, batch, the two log-sum-exps -- are independent chains of additions and share nothing
//                           but the staged values.  Each carries its state across calls in global memory.
// The log-sum-exp walks its samples four at a time: where none of the four exceeds m -- the usual case once the chain
// has seen its maximum -- the four exps do not depend on each other and are issued together, and only the four
// additions stay in order; where one does, the four are taken one by one.  Both ways are the recurrence above,
// operation for operation.
// No float atomics, contraction off, plain vector stores.
#pragma once

#include <hip/hip_runtime.h>

namespace apemost {

constexpr int kEvidenceThreads = 64;       // fold: one wave per workgroup
constexpr int kEvidenceGatherThreads = 256;
constexpr int kEvidenceQuantities = 5;     // sum, sq, batch, log-sum-exp up, log-sum-exp down

struct EvidenceArgs {
    const double *rows;                    // [n_steps][n_chains][n_par+2]
    int n_chains, n_par;
    unsigned long long skip, thin;         // kept steps of this piece: skip, skip + thin, ... (n of them)
    unsigned int n;                        // kept steps of this piece, 1 .. chunk
    int first;                             // this piece holds the first sample ever accumulated
    unsigned long long bs;                 // batch size
    unsigned long long left;               // samples still to come before the open batch closes (1 .. bs)
    unsigned long long n_closed;           // batches closed before this piece = slot of the open batch
    unsigned long long batch_stride;       // max_batches + 1
    const double *coef;                    // [2][n_chains]: up, down
    double *vals;                          // [chunk][n_chains]
    double *origin, *sum, *sq;             // [n_chains]
    double *batch;                         // [n_chains][max_batches + 1]
    double *m, *S;                         // [2][n_chains]
};

// grid (ceil(n_chains / 256), ceil(n / 8)): consecutive threads take consecutive chains of one kept step
__global__ void __launch_bounds__(kEvidenceGatherThreads) evidence_gather_kernel(EvidenceArgs a) {
    const int c = blockIdx.x * kEvidenceGatherThreads + threadIdx.x;
    if (c >= a.n_chains)
        return;
    const size_t w = (size_t)a.n_par + 2, row = (size_t)a.n_chains * w;
    const double *src = a.rows + a.skip * row + (size_t)c * w + a.n_par + 1;
    const size_t stride = (size_t)a.thin * row;
    const unsigned int i0 = blockIdx.y * 8u;
#pragma unroll
    for (unsigned int r = 0; r < 8u; r++) {
        const unsigned int i = i0 + r;
        if (i >= a.n)
            break;
        const double v = src[i * stride];
        a.vals[(size_t)i * a.n_chains + c] = v;
        if (a.first && i == 0)
            a.origin[c] = v;
    }
}

// one log-sum-exp update, as the header states it
__device__ inline void evidence_lse_step(double x, double &m, double &S) {
#pragma clang fp contract(off)
    if (x > m) {
        const double t = S * exp(m - x);
        S = t + 1.0;
        m = x;
    } else
        S += exp(x - m);
}

// grid (ceil(n_chains / 64), 5)
__global__ void __launch_bounds__(kEvidenceThreads) evidence_fold_kernel(EvidenceArgs a) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * kEvidenceThreads + threadIdx.x;
    if (c >= a.n_chains)
        return;
    const int q = blockIdx.y;
    const size_t nc = (size_t)a.n_chains;
    const double *v = a.vals + c;
    if (q == 0) {
        const double o = a.origin[c];
        double s = a.sum[c];
#pragma unroll 8
        for (unsigned int i = 0; i < a.n; i++)
            s += v[i * nc] - o;
        a.sum[c] = s;
    } else if (q == 1) {
        const double o = a.origin[c];
        double s = a.sq[c];
#pragma unroll 8
        for (unsigned int i = 0; i < a.n; i++) {
            const double d = v[i * nc] - o;
            const double prod = d * d;
            s += prod;
        }
        a.sq[c] = s;
    } else if (q == 2) {
        // batch_means_error(): batchsum += v; a batch closes after its last sample (pt_summary.h)
        double *batch = a.batch + (size_t)c * a.batch_stride;
        unsigned long long nb = a.n_closed, left = a.left;
        double part = batch[nb];
        for (unsigned int i = 0; i < a.n; i++) {
            part += v[i * nc];
            if (--left == 0) {
                batch[nb++] = part;
                part = 0;
                left = a.bs;
            }
        }
        batch[nb] = part; // the open batch
    } else {
        const size_t at = (size_t)(q - 3) * nc + c;
        const double coef = a.coef[at];
        double m = a.m[at], S = a.S[at];
        unsigned int i = 0;
        if (a.first) {
            m = coef * v[0];
            S = 1.0;
            i = 1;
        }
        for (; i + 4 <= a.n; i += 4) {
            const double x0 = coef * v[i * nc], x1 = coef * v[(i + 1) * nc], x2 = coef * v[(i + 2) * nc],
                         x3 = coef * v[(i + 3) * nc];
            if (x0 > m || x1 > m || x2 > m || x3 > m) {
                evidence_lse_step(x0, m, S);
                evidence_lse_step(x1, m, S);
                evidence_lse_step(x2, m, S);
                evidence_lse_step(x3, m, S);
            } else {
                const double e0 = exp(x0 - m), e1 = exp(x1 - m), e2 = exp(x2 - m), e3 = exp(x3 - m);
                S += e0;
                S += e1;
                S += e2;
                S += e3;
            }
        }
        for (; i < a.n; i++)
            evidence_lse_step(coef * v[i * nc], m, S);
        a.m[at] = m;
        a.S[at] = S;
    }
}

} // namespace apemost
