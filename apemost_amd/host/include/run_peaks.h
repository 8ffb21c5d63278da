/* <paramname>.peaks: the APEMOST_DUMP token `peaks` (include/apemost_hip.h, apemost_hip_peaks_*).  The run phase
 * keeps chain 0's parameter columns on the device and leaves, per parameter, the output of the reference's
 * `peaks.exe min max <paramname>-chain-0.prob.dump` over the parameter's prior box [min, max] -- the analysis its
 * manual prefers to reading the marginal histograms -- without the sample dump having been written. */
#ifndef RUN_PEAKS_H
#define RUN_PEAKS_H
#include <stdint.h>

#include "apemost_hip.h"
#include "mcmc.h"

/* begins peaks for local chain 0 of shard `s` over the prior box of `chain0`, for `capacity` kept samples.  With
 * `append` one line on stderr says that the files will cover this run's samples only. */
void run_peaks_open(apemost_hip_sampler *s, const mcmc *chain0, uint64_t capacity, int append);
/* sorts on the device, writes <paramname>.peaks for every parameter and frees the columns.  A parameter with 100
 * peaks or more ends the program, as the reference's assert does. */
void run_peaks_close(apemost_hip_sampler *s, const mcmc *chain0);

#endif
