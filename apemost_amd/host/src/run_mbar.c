/* mbar.bin reader and writer, the solver loop and mbar.txt of the APEMOST_DUMP token `mbar` (run_mbar.h).  No device
 * symbol: the passes come through run_mbar_passes. */
#include "run_mbar.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "run_io.h"

/* run_io.h with this file's word in the messages */
#define alloc_or_die(count) ((double *)run_alloc_or_die(count, sizeof(double), "mbar"))
#define read_or_die(p, size, count, f, path) run_read_or_die(p, size, count, f, path, "mbar file")

#define RUN_MBAR_MAGIC "APEMOSTM"
#define RUN_MBAR_VERSION 1
#define TILE 4096
#define LANES 64

void run_mbar_alloc(run_mbar *r) {
    r->betas = alloc_or_die(r->n_chains);
    r->g = alloc_or_die(r->n_chains);
    r->ell = alloc_or_die((size_t)r->n * r->n_chains);
}

void run_mbar_free(run_mbar *r) {
    free(r->betas);
    free(r->g);
    free(r->ell);
    memset(r, 0, sizeof *r);
}

int run_mbar_read(const char *path, run_mbar *r) {
    FILE *f = fopen(path, "rb");
    char magic[8];
    uint32_t u32[4];
    uint64_t u64[4];
    if (f == NULL)
        return -1;
    read_or_die(magic, 1, 8, f, path);
    read_or_die(u32, sizeof(uint32_t), 4, f, path);
    read_or_die(u64, sizeof(uint64_t), 4, f, path);
    if (memcmp(magic, RUN_MBAR_MAGIC, 8) != 0 || u32[0] != RUN_MBAR_VERSION || u32[2] != 1) {
        fprintf(stderr, "%s: not an mbar file of version %d with one ladder\n", path, RUN_MBAR_VERSION);
        exit(1);
    }
    memset(r, 0, sizeof *r);
    r->n_chains = u32[1];
    r->solved = u32[3];
    r->n = u64[0];
    r->thin = u64[1];
    r->t0 = u64[2];
    r->t_count = u64[3];
    if (r->n_chains < 1 || r->n > ((uint64_t)1 << 28) / r->n_chains || r->t0 > r->n || r->t_count > r->n - r->t0) {
        fprintf(stderr, "%s: %lu samples of %lu chains and the range [%lu, +%lu) do not fit\n", path, (unsigned long)r->n,
                (unsigned long)r->n_chains, (unsigned long)r->t0, (unsigned long)r->t_count);
        exit(1);
    }
    run_mbar_alloc(r);
    read_or_die(r->betas, sizeof(double), r->n_chains, f, path);
    read_or_die(&r->n_bad, sizeof(uint64_t), 1, f, path);
    read_or_die(r->g, sizeof(double), r->n_chains, f, path);
    read_or_die(r->ell, sizeof(double), (size_t)r->n * r->n_chains, f, path);
    fclose(f);
    return 0;
}

void run_mbar_write(const char *path, const run_mbar *r) {
    FILE *f = run_open_or_die(path, "wb");
    uint32_t u32[4];
    uint64_t u64[4];
    u32[0] = RUN_MBAR_VERSION;
    u32[1] = r->n_chains;
    u32[2] = 1;
    u32[3] = r->solved ? 1 : 0;
    u64[0] = r->n;
    u64[1] = r->thin;
    u64[2] = r->solved ? r->t0 : 0;
    u64[3] = r->solved ? r->t_count : 0;
    fwrite(RUN_MBAR_MAGIC, 1, 8, f);
    fwrite(u32, sizeof(uint32_t), 4, f);
    fwrite(u64, sizeof(uint64_t), 4, f);
    fwrite(r->betas, sizeof(double), r->n_chains, f);
    fwrite(&r->n_bad, sizeof(uint64_t), 1, f);
    fwrite(r->g, sizeof(double), r->n_chains, f);
    fwrite(r->ell, sizeof(double), (size_t)r->n * r->n_chains, f);
    run_close_or_die(f, path);
}

double run_mbar_tol_from_env(void) {
    const char *spec = getenv("APEMOST_MBAR_TOL");
    char *end;
    double tol;
    if (spec == NULL || *spec == 0)
        return 1e-10;
    tol = strtod(spec, &end);
    if (*end != 0 || !(tol > 0) || tol - tol != 0) {
        fprintf(stderr, "APEMOST_MBAR_TOL: expected a positive number, got '%s'\n", spec);
        exit(1);
    }
    return tol;
}

unsigned long run_mbar_iter_from_env(void) {
    const char *spec = getenv("APEMOST_MBAR_ITER");
    char *end;
    long n;
    if (spec == NULL || *spec == 0)
        return 10000;
    n = strtol(spec, &end, 10);
    if (*end != 0 || n < 1) {
        fprintf(stderr, "APEMOST_MBAR_ITER: expected a positive integer, got '%s'\n", spec);
        exit(1);
    }
    return (unsigned long)n;
}

/* g - g_0 in place */
static void relative(double *g, unsigned int nc) {
    const double g0 = g[0];
    unsigned int c;
    for (c = 0; c < nc; c++)
        g[c] -= g0;
}

void run_mbar_start(const run_mbar *r, uint64_t t0, uint64_t t_count, double *g) {
    const unsigned int nc = r->n_chains;
    double *mean = alloc_or_die(nc);
    unsigned int c;
    uint64_t t;
    for (c = 0; c < nc; c++) {
        double s = 0;
        for (t = 0; t < t_count; t++)
            s += r->ell[(size_t)(t0 + t) * nc + c];
        mean[c] = s / (double)t_count;
    }
    g[nc - 1] = 0;
    for (c = nc - 1; c-- > 0;)
        g[c] = g[c + 1] + (r->betas[c] - r->betas[c + 1]) * (mean[c] + mean[c + 1]) / 2;
    relative(g, nc);
    free(mean);
}

long run_mbar_solve(const run_mbar *r, const run_mbar_passes *p, double tol, unsigned long max_iter, uint64_t t0,
                    uint64_t t_count, double *g, double *change) {
    const unsigned int nc = r->n_chains;
    double *prev = alloc_or_die(nc);
    unsigned long used = 0;
    unsigned int c;
    *change = HUGE_VAL;
    relative(g, nc);
    while (used < max_iter) {
        const unsigned long k = max_iter - used < RUN_MBAR_CHECK_EVERY ? max_iter - used : RUN_MBAR_CHECK_EVERY;
        p->iterate(p->ctx, t0, t_count, (uint32_t)k, g, prev);
        used += k;
        relative(g, nc);
        relative(prev, nc);
        *change = 0;
        for (c = 0; c < nc; c++)
            if (!(fabs(g[c] - prev[c]) <= *change)) /* (a NaN stays) */
                *change = fabs(g[c] - prev[c]);
        if (*change <= tol)
            break;
    }
    free(prev);
    return *change <= tol ? (long)used : -1;
}

/* G(1) and G(0) less G(beta_0), then their difference: Mbar.ln_evidence */
static double ln_evidence(const run_mbar *r, const run_mbar_passes *p, uint64_t t0, uint64_t t_count, const double *g) {
    double targets[3], G[3], ell_first;
    double *words[6] = {NULL, NULL, NULL, NULL, NULL, NULL};
    targets[0] = 1.0;
    targets[1] = 0.0;
    targets[2] = r->betas[0];
    words[5] = G;
    p->evaluate(p->ctx, t0, t_count, g, targets, 3, words, &ell_first);
    return (G[0] - G[2]) - (G[1] - G[2]);
}

void run_mbar_write_text(const char *path, const run_mbar *r, const run_mbar_passes *p, double tol, unsigned long max_iter) {
    const unsigned int nc = r->n_chains;
    double *targets = alloc_or_die(nc + 1), *w = alloc_or_die(6 * (size_t)(nc + 1)), *g = alloc_or_die(nc);
    double *words[6];
    double ell_first, est[RUN_MBAR_BLOCKS], mean = 0, ss = 0, change;
    unsigned int c, i;
    FILE *f = run_open_or_die(path, "w");
    for (i = 0; i < 6; i++)
        words[i] = w + (size_t)i * (nc + 1);
    memcpy(targets, r->betas, nc * sizeof(double));
    targets[nc] = r->betas[0];
    p->evaluate(p->ctx, r->t0, r->t_count, r->g, targets, (int)(nc + 1), words, &ell_first);
    for (c = 0; c < nc; c++) {
        const double S0 = words[1][c], ratio = words[2][c] / S0;
        run_print_values(f, 5, r->betas[c], words[5][c] - words[5][nc], ell_first + ratio, words[3][c] / S0 - ratio * ratio,
                         S0 * S0 / words[4][c]);
        fprintf(f, "\n");
    }
    for (i = 0; i < RUN_MBAR_BLOCKS; i++) { /* Mbar.error: every block solved on its own from the whole run's g */
        const uint64_t lo = r->t0 + (uint64_t)i * r->t_count / RUN_MBAR_BLOCKS;
        const uint64_t hi = r->t0 + (uint64_t)(i + 1) * r->t_count / RUN_MBAR_BLOCKS;
        est[i] = sqrt(-1.0);
        if (hi > lo) {
            memcpy(g, r->g, nc * sizeof(double));
            if (run_mbar_solve(r, p, tol, max_iter, lo, hi - lo, g, &change) < 0)
                fprintf(stderr, "%s: block %u of the error estimate left a change of %g, above %g\n", path, i, change, tol);
            else
                est[i] = ln_evidence(r, p, lo, hi - lo, g);
        }
        mean += est[i];
    }
    mean /= RUN_MBAR_BLOCKS;
    for (i = 0; i < RUN_MBAR_BLOCKS; i++)
        ss += (est[i] - mean) * (est[i] - mean);
    fprintf(f, "ln_evidence\t");
    run_print_values(f, 2, ln_evidence(r, p, r->t0, r->t_count, r->g), sqrt(ss / (RUN_MBAR_BLOCKS - 1)) / sqrt((double)RUN_MBAR_BLOCKS));
    fprintf(f, "\n");
    free(targets);
    free(w);
    free(g);
    run_close_or_die(f, path);
}

/* ---- the passes in C, in the order csrc/pt_mbar.h states ---- */
/* lnD of the N = t_count * K samples of the range, in stored order */
static double *host_row_pass(const run_mbar *r, uint64_t t0, uint64_t t_count, const double *g) {
    const unsigned int K = r->n_chains;
    const size_t N = (size_t)t_count * K;
    const double lnT = log((double)t_count);
    const double *ell = r->ell + (size_t)t0 * K;
    double *lnD = alloc_or_die(N), *c = alloc_or_die(K);
    unsigned int j;
    size_t n;
    for (j = 0; j < K; j++)
        c[j] = lnT - g[j];
    for (n = 0; n < N; n++) {
        const double l = ell[n];
        double prod = r->betas[0] * l, m, S = 0.0;
        m = prod + c[0];
        for (j = 1; j < K; j++) {
            double x;
            prod = r->betas[j] * l;
            x = prod + c[j];
            if (x > m)
                m = x;
        }
        for (j = 0; j < K; j++) {
            double x;
            prod = r->betas[j] * l;
            x = prod + c[j];
            S += exp(x - m);
        }
        lnD[n] = m + log(S);
    }
    free(c);
    return lnD;
}

/* m and the four sums of one target: tiles of 4096 from the range's first sample, 64 lane partials, the
 * adjacent-pairs tree, tiles in order */
static void host_col_pass(const double *ell, const double *lnD, size_t N, double bt, int full, double *m_out, double S[4]) {
    double m = bt * ell[0], p[4][LANES];
    size_t n, base;
    int w, j, half;
    m = m - lnD[0];
    for (n = 1; n < N; n++) {
        const double prod = bt * ell[n];
        const double x = prod - lnD[n];
        if (x > m)
            m = x;
    }
    S[0] = S[1] = S[2] = S[3] = 0.0;
    for (base = 0; base < N; base += TILE) {
        const size_t cnt = N - base < TILE ? N - base : TILE;
        for (w = 0; w < 4; w++)
            for (j = 0; j < LANES; j++)
                p[w][j] = 0.0;
        for (n = 0; n < cnt; n++) {
            const double l = ell[base + n], prod = bt * l;
            const double x = prod - lnD[base + n];
            const double e = exp(x - m);
            p[0][n % LANES] += e;
            if (full) {
                const double d = l - ell[0], ed = e * d;
                const double edd = ed * d, ee = e * e;
                p[1][n % LANES] += ed;
                p[2][n % LANES] += edd;
                p[3][n % LANES] += ee;
            }
        }
        for (w = 0; w < (full ? 4 : 1); w++) {
            for (half = LANES / 2; half >= 1; half /= 2)
                for (j = 0; j < half; j++)
                    p[w][j] = p[w][2 * j] + p[w][2 * j + 1];
            S[w] += p[w][0];
        }
    }
    *m_out = m;
}

static int host_iterate(void *ctx, uint64_t t0, uint64_t t_count, uint32_t n_iter, double *g, double *g_prev) {
    const run_mbar *r = (const run_mbar *)ctx;
    const unsigned int K = r->n_chains;
    const size_t N = (size_t)t_count * K;
    uint32_t it;
    unsigned int t;
    for (it = 0; it < n_iter; it++) {
        double *lnD = host_row_pass(r, t0, t_count, g);
        memcpy(g_prev, g, K * sizeof(double));
        for (t = 0; t < K; t++) {
            double m, S[4];
            host_col_pass(r->ell + (size_t)t0 * K, lnD, N, r->betas[t], 0, &m, S);
            g[t] = m + log(S[0]);
        }
        free(lnD);
    }
    return 0;
}

static int host_evaluate(void *ctx, uint64_t t0, uint64_t t_count, const double *g, const double *betas_t, int n_t,
                         double *const words[6], double *ell_first) {
    const run_mbar *r = (const run_mbar *)ctx;
    const unsigned int K = r->n_chains;
    const size_t N = (size_t)t_count * K;
    double *lnD = host_row_pass(r, t0, t_count, g);
    int t, w;
    for (t = 0; t < n_t; t++) {
        double m, S[4];
        host_col_pass(r->ell + (size_t)t0 * K, lnD, N, betas_t[t], 1, &m, S);
        if (words[0] != NULL)
            words[0][t] = m;
        for (w = 0; w < 4; w++)
            if (words[1 + w] != NULL)
                words[1 + w][t] = S[w];
        if (words[5] != NULL)
            words[5][t] = m + log(S[0]);
    }
    *ell_first = r->ell[(size_t)t0 * K];
    free(lnD);
    return 0;
}

run_mbar_passes run_mbar_host_passes(const run_mbar *r) {
    run_mbar_passes p;
    p.ctx = (void *)r;
    p.iterate = host_iterate;
    p.evaluate = host_evaluate;
    return p;
}
