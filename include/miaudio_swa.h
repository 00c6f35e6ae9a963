/*
 * miaudio_swa.h — stochastic weight averaging over a device table of tensors (part of libmiaudio.so): the running
 * average of the parameters, and its transfer back into the parameters and their bf16 operand copies.  Replaces
 * what Lightning's StochasticWeightAveraging callback (the reference's src/training/callbacks.py:71-79) does with
 * torch.optim.swa_utils.AveragedModel's update_parameters and its final copy into the model.
 *
 * Conventions as in miaudio.h: extern "C", stream-ordered, the caller owns all memory, 0 on success and a
 * negative code on error (mia_last_error_string() explains).
 *
 * Tables as mia_clip_adam's: device arrays f32* avg[n], f32* params[n], bf16* shadow[n] (the table or any entry
 * may be NULL), int64 sizes[n] (elements per tensor); max_numel, the largest of them, sizes the grid.  Both passes
 * are the optimizers' streaming walker: 16-B non-temporal loads and stores on 16-B aligned tensors, element by
 * element for the n % 4 tail and for a tensor with any misaligned pointer -- the same bits either way.
 */
#ifndef MIAUDIO_SWA_H
#define MIAUDIO_SWA_H
#include "miaudio.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The running average after one more sample, per element:
 *   n_averaged == 0:  avg = p
 *   otherwise:        avg = avg + (p - avg) / (float)(n_averaged + 1)
 * -- one f32 subtract, one correctly rounded f32 divide and one f32 add, in that order, nothing contracted.
 * Writes every element of every avg[i] and nothing else; params is read only.  Traffic: 12 B per parameter
 * (8 B at n_averaged == 0, where avg is not read).  n_averaged >= 0. */
int mia_swa_update(void* const* avg, void* const* params, const int64_t* sizes, int32_t ntensors, int64_t max_numel,
                   int64_t n_averaged, mia_stream_t stream);

/* p = avg, and where shadow_bf16 and shadow_bf16[i] are non-NULL, shadow = bf16(avg) with the rounding of the
 * optimizers' shadow write (round to nearest even).  Writes every element of every params[i] (and of every
 * non-NULL shadow) and nothing else; avg is read only.  Traffic: 8 B per parameter, + 2 B where shadowed. */
int mia_swa_transfer(void* const* params, void* const* avg, void* const* shadow_bf16, const int64_t* sizes,
                     int32_t ntensors, int64_t max_numel, mia_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MIAUDIO_SWA_H */
