// oi_screen_i8.h -- what the int8 screening tier (cosine_screen_i8.hip) and the residual plane behind it (screen_i8_residual.hip)
// share: the layout constant of a plane and the two device functions a pair's lower-bound key is made from.
#pragma once
#include "oi_device.h"

#define I8S_PAD_ROWS 64

// The lower bound a pair is keyed by, l = s~ - (e_r |q^| + c_q) with s~ = f32(S) (scale a / 128): ONE body for the screen's
// survivor path and the sample pass, so both round alike (qa = a / 128).
__device__ __forceinline__ float i8s_screen_score(int S, float scale, float qa) { return (float)S * (scale * qa); }
__device__ __forceinline__ float i8s_lower_bound(float sc, float er, float qn, float cq) { return sc - fmaf(er, qn, cq); }
