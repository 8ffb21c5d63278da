/*
 * rwm_compat.h -- force-included (gcc -include) into the reference's -DRWM build only.
 *
 * With -DRWM the reference's adapt() calls markov_chain_step(chain, 0) (src/parallel_tempering.c:278),
 * but the function takes ONE argument (src/markov_chain.h, src/markov_chain.c:369), so that variant
 * does not compile as published.  This macro drops every argument after the first, at the call and --
 * harmlessly -- at the declaration and the definition, which have only one.  Nothing else changes:
 * the step that runs is the reference's own markov_chain_step.
 */
#ifndef APEMOST_REFGSL_RWM_COMPAT_H
#define APEMOST_REFGSL_RWM_COMPAT_H
#define REFGSL_FIRST(a, ...) a
#define markov_chain_step(...) markov_chain_step(REFGSL_FIRST(__VA_ARGS__, 0))
#endif
