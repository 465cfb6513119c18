// Host-only planner of the BigVGAN stages: decides, once per forward and for the whole vocoder, what every stage runs
// (its precision, its upsampler form, its AMPBlock form and how the resblock chains share buffers, streams and the
// closing sum).  Same rules as alcm_convplan.h: no HIP header, no device call, no pointer dereferenced.
// bigvgan_forward (alcm_models.cpp) executes the plans and decides nothing.
#pragma once
#include "alcm_actplan.h"
#include "alcm_convplan.h"

namespace alcm {

using VocStageShape = alcm_voc_stage_shape;
using VocStagePlan = alcm_voc_stage_plan;

enum VocUps { VU_PLANES = 0, VU_UPS2, VU_PHASES };
enum VocAmp { VA_FUSED = 0, VA_FUSED_DENSE, VA_WIDE };

// the plans of stages 0 .. n-1 at batch B and M mel frames; streams: the chains' auxiliary streams exist (the model
// has them switched on and they could be created).  0, or ALCM_E_INVALID for a shape beyond the struct's bounds
int voc_plan(const VocStageShape* st, int n, int policy, bool streams, int B, int M, int ncu, const Knobs& k,
             VocStagePlan* out);

// the stride-2 / 4-tap upsampler with both phases in one split-precision pass (alcm_ups.hip)
bool ups2_supported(int cin, int cout, int cpad, int rate, int taps);

}  // namespace alcm
