/* The C host's resample.bin writer, the resampled text dumps and the environment of APEMOST_RESAMPLE_DRAWS and
 * APEMOST_RESAMPLE_SEED (apemost_amd/host/src/run_reweight.c) with a main of their own: run_resample_check [name ...]
 * prints the draws and the seed the environment asks for and, where there are draws, writes resample.bin and the dumps
 * of two targets and two columns filled by a rule tests/test_run_resample_cpu.py repeats: x = (m + 1) / (a + 3) - t,
 * index = m (t + 1), q_total = seed + t.  Built without the device library. */
#include "run_reweight.h"

#include <stdio.h>
#include <stdlib.h>

int main(int argc, char **argv) {
    run_reweight r;
    const uint32_t n_draws = run_resample_draws_from_env();
    const uint64_t seed = run_resample_seed_from_env();
    uint64_t q_total[2];
    uint32_t *index, m;
    double *x;
    unsigned int t, a;
    printf("%lu draws; seed %lu\n", (unsigned long)n_draws, (unsigned long)seed);
    if (n_draws == 0)
        return 0;
    r.n_chains = 5;
    r.n_cols = 2;
    r.n_t = 2;
    r.nbins = 0;
    run_reweight_alloc(&r);
    r.shift = 49;
    r.n = 1639;
    r.thin = 3;
    r.t0 = 100;
    r.t_count = 1500;
    r.cols[0] = 1;
    r.cols[1] = 4;
    r.betas_t[0] = 1.0;
    r.betas_t[1] = 0.3;
    index = (uint32_t *)malloc(2 * (size_t)n_draws * sizeof(uint32_t));
    x = (double *)malloc(4 * (size_t)n_draws * sizeof(double));
    if (index == NULL || x == NULL)
        return 2;
    for (t = 0; t < 2; t++) {
        q_total[t] = seed + t;
        for (m = 0; m < n_draws; m++) {
            index[(size_t)t * n_draws + m] = m * (t + 1);
            for (a = 0; a < 2; a++)
                x[((size_t)t * n_draws + m) * 2 + a] = (double)(m + 1) / (double)(a + 3) - (double)t;
        }
    }
    run_resample_write(RUN_RESAMPLE_FILE, &r, n_draws, seed, q_total, index, x);
    for (t = 0; t < 2; t++)
        run_resample_write_dumps(&r, t, n_draws, x + (size_t)t * n_draws * 2, argc > 1 ? (const char *const *)(argv + 1) : NULL);
    free(index);
    free(x);
    run_reweight_free(&r);
    return 0;
}
