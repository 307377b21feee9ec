// tvam_dproj.h -- what the host shares with the projector derivatives (DESIGN.md section 4n;
// tvam_dproj.hip): the parameter of a call and the launcher.
#pragma once
#include "tvam_internal.h"

// The parameter a call differentiates in (TVAM_DPROJ_*) and what the kernels need of the descriptor
// beyond TvamConsts: pixel_size_x, pixel_size_y (TVAM_DPROJ_PIXEL_SIZE moves both pixel sizes
// together: d xc / d p_x = xc / p_x, and the ray weight ~ p_x p_y adds (1 / p_x + 1 / p_y) dose).
struct TvamDproj {
    int32_t param;
    float px, py;
};

// One thread per (ray, sample) of a telecentric / lens plan behind the index-matched vial.
// FWD: the tangent film d dose / d theta added into `tangent` (zeroed by the caller).  ADJ:
// sum_v gin[v] * tangent[v] into g[0] (device, overwritten) through `partials`, one fp64 partial per
// workgroup of the launch's grid (tvam_dsigma_grid of the ray count); no atomics.
hipError_t tvam_launch_dproj(int mode, const TvamConsts& k, const TvamTiles& t, const TvamDproj& dp, const float* pat,
                             const int32_t* idxmap, const float* gin, float* tangent, double* partials, double* g,
                             hipStream_t stream);
