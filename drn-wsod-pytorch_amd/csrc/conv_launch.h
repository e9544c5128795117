// What the convolution forward's plan and launch (conv_fwd_plan / conv_fwd_launch, conv.hip) use of the other two conv
// translation units.  The class conditions are in conv_fwd_plan; these launch the decided form.  Library-internal.
#pragma once
#include "drn_common.h"
#include "tune.h"
#include "conv_params.h"

__attribute__((visibility("hidden"))) int drn_conv_ring_launch(const drn_conv::ConvParams& p, int tile, hipStream_t st);  // conv_ring.hip: tile 64 / 128
__attribute__((visibility("hidden"))) int drn_pp8_conv_launch(const drn_conv::ConvParams& p, bool wide, hipStream_t st);  // pp8.hip: 128x128 / 256x128
__attribute__((visibility("hidden"))) bool drn_pp8_wide_ok(long rows_one, int N, const DrnTune& t, int cus);  // pp8.hip (also drn_linear_act_fwd's rule)
