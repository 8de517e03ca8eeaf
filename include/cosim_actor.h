/* cosim_actor.h -- extended actors: the entry points that evaluate an actor with an observation normaliser, LayerNorm and an
 * output stage in the one launch of cosim_mlp_forward / cosim_policy_table_forward (cosim.h, which this header extends; the table
 * handle and its forward, rotate, lists and destroy are declared there).  cosim_amd/engine.py: ABI_ACTOR. */
#ifndef COSIM_ACTOR_H
#define COSIM_ACTOR_H

#include "cosim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* EXTENDED actors: what exported actors carry besides the Gemm / activation chain, fused into the same launch.
 *   input stage   up to 4 elementwise items on the observation, in listed order: op 1 add, 2 sub, 3 mul, 4 div with a vector of the
 *                 observation's width (y = y op v[column]; each ONE fp32 operation, the division correctly rounded), 5 clip to
 *                 [lo, hi] (-INFINITY / INFINITY: no bound; NaN stays NaN) -- an observation normaliser (x - mean) / std [clipped]
 *   LayerNorm     slot s normalises over the dims[s] columns of: s = 0 the observation (behind the input stage), s = l + 1 the output
 *                 of layer l.  ln_where[s]: 0 none, 1 ahead of layer l's activation, 2 behind it; ln_gamma[s] required, ln_beta[s]
 *                 may be NULL, ln_eps[s] > 0 and finite.  Two-pass statistics over the row's own columns in a fixed order.  Not on
 *                 the last layer.
 *   output stage  up to 4 items of the same kind on the last layer's output, behind its activation and ahead of `clip`; vectors of
 *                 the action's width.
 * cosim_mlp_forward_ex: cosim_mlp_forward with such a description; every vector is a DEVICE pointer.  extras NULL or all zero: the
 * launch, and the bits, of cosim_mlp_forward.  Refuses (COSIM_EINVAL, cosim_last_error names the field): more than 4 items in a
 * stage, an unknown op code or placement, a null vector, a non-finite or non-positive eps, LayerNorm on the last layer. */
typedef struct {
  int32_t n_in, n_out;
  int32_t in_op[4], out_op[4];
  const float* in_vec[4];
  const float* out_vec[4];
  float in_lo[4], in_hi[4], out_lo[4], out_hi[4];
  int32_t ln_where[7];
  float ln_eps[7];
  const float* ln_gamma[7];
  const float* ln_beta[7];
} cosim_mlp_extras_t;
int cosim_mlp_forward_ex(const float* x_dev, int n, int n_layers, const int* dims, const float* const* w_dev, const float* const* b_dev,
                         const int* act, const float* act_alpha, const cosim_mlp_extras_t* extras, float clip, float* out_dev,
                         void* stream);

/* create with extended actors: extras[K] (NULL: cosim_policy_table_create), one cosim_mlp_extras_t per policy with HOST vectors, all
 * zero for a plain policy.  The vectors go into the weight image behind their policy's layers, each begun at a multiple of 4 words,
 * and a second 64-word record per policy holds their offsets.  A table in which no policy has extras is the table create makes; one
 * with such a policy runs the extended kernel for all of its tiles, and every env still gets the bits of cosim_mlp_forward[_ex] for
 * its policy.  forward, rotate, forward_rotating, lists and destroy are the ones above.  Refusals as cosim_mlp_forward_ex, naming
 * the policy. */
int cosim_policy_table_create_ex(int n_policies, const int* n_layers, const int* dims, const int* act, const float* act_alpha,
                                 const float* const* w_host, const float* const* b_host, const cosim_mlp_extras_t* extras, int n,
                                 const int* policy_of_row, int n_ranges, const int* ranges, cosim_policy_table_t** out);

#ifdef __cplusplus
}
#endif

#endif
