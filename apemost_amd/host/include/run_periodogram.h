/* The APEMOST_DUMP token `periodogram`: the residual periodogram of chain 0 folded on the device while the run steps
 * (include/apemost_hip.h, apemost_hip_periodogram_*; the quantities are specified in apemost_amd/csrc/pt_periodogram.h).
 * For simplesin and sine3.  The frequency grid comes from APEMOST_PERIODOGRAM_FREQS=lo:hi:n, which the token requires:
 * n frequencies (1 .. 2^20), nu_j = lo + j * ((hi - lo) / (n - 1)) with lo <= hi both finite (n = 1: lo alone).  The weights
 * are Lomb-Scargle's, computed here from column 0 of the data and the ladder's sigma (run_periodogram_weights: with
 * G = [[sum c^2, sum c s], [sum c s, sum s^2]] of a frequency, G^-1 / (2 sigma^2), zero where G is singular; what
 * periodogram.weights of apemost_amd/periodogram.py computes with numpy's cos and sin, here with libm's); the level of the
 * exceedance count is -ln(0.01 / n), a false-alarm probability of 1 % over the grid under white noise.  At the end of the
 * run:
 *   periodogram.bin  the state, in the format of apemost_amd/periodogram.py (Periodogram.read), which --append loads;
 *   periodogram.txt  one line per frequency: nu, the mean, standard deviation, minimum and maximum of the power over the
 *                    kept samples, the power of the mean residual (coherent) and the share of the kept samples whose
 *                    highest peak it held ("%.15e", tab separated, a NaN as nan): Periodogram.text.
 * A bounded run is needed: the files are written when the run ends.  A pulse model or a device model ends the program.
 * run_periodogram.c needs neither the device nor the chains; run_periodogram_device.c holds run_periodogram_open and
 * _close. */
#ifndef RUN_PERIODOGRAM_H
#define RUN_PERIODOGRAM_H
#include <stdint.h>

#define RUN_PERIODOGRAM_FILE "periodogram.bin"
#define RUN_PERIODOGRAM_TEXT "periodogram.txt"
#define RUN_PERIODOGRAM_WORDS 7      /* origin, sum, sq, pmin, pmax, sum_c, sum_s */
#define RUN_PERIODOGRAM_PEAK_WORDS 5 /* origin, sum, sq, min, max */
#define RUN_PERIODOGRAM_MAX_FREQ (1 << 20)

typedef struct {
    uint32_t n_freq, n_data, model;
    uint64_t n, thin;
    double sigma, level;
    int32_t chain;
    double *freqs;                              /* [n_freq] */
    double *weights;                            /* [n_freq][3] */
    double *state[RUN_PERIODOGRAM_WORDS];       /* [n_freq] each */
    uint64_t *exceed;                           /* [n_freq] */
    double peak[RUN_PERIODOGRAM_PEAK_WORDS];
    uint64_t *peak_counts;                      /* [n_freq + 1] */
} run_periodogram;

/* APEMOST_PERIODOGRAM_FREQS parsed into lo, hi, n; an unset or malformed value prints one line and ends the program */
void run_periodogram_grid_from_env(double *lo, double *hi, uint32_t *n);
/* allocates every array for the n_freq already set (zeroed); frees them */
void run_periodogram_alloc(run_periodogram *r);
void run_periodogram_free(run_periodogram *r);
/* freqs[j] of the grid; the Lomb-Scargle weights [n_freq][3] over the abscissae x [n_data] */
void run_periodogram_grid(double lo, double hi, uint32_t n, double *freqs);
void run_periodogram_weights(const double *x, uint32_t n_data, const double *freqs, uint32_t n_freq, double sigma,
                             double *weights);
/* -1: no such file; 0: read (arrays allocated); 1: a file of more than one kept chain.  Anything else that is not a
 * periodogram file of this version ends the program. */
int run_periodogram_read(const char *path, run_periodogram *r);
void run_periodogram_write(const char *path, const run_periodogram *r);
void run_periodogram_write_text(const char *path, const run_periodogram *r);

#endif
