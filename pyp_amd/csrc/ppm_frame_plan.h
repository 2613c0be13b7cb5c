// ppm_frame_plan.h — the two host rules of movie-frame refinement (ppm_frame_refine, host_frames.h): the step of the
// shift grid and the number of grid steps either side of a row's shift.  Plain C++, no HIP types: compiled alone by
// tests/test_frames_cpu.py; pyp_amd/frames.py states the same rules in numpy.
#pragma once

#include <cmath>

#ifndef PPM_HD
#ifdef __HIPCC__
#define PPM_HD __host__ __device__
#else
#define PPM_HD
#endif
#endif

#ifndef PPM_FRAME_MAX_STEPS
#define PPM_FRAME_MAX_STEPS 8 /* also in include/ppm.h */
#endif

namespace ppm {

// grid step in pixels: step_px, 0 = half a pixel (a negative step is refused by the caller)
PPM_HD inline float frame_step(float step_px) { return step_px > 0.f ? step_px : 0.5f; }

// Grid steps either side of a row's shift for a search of +-range_px in steps of h: W = ceil(range_px / h - 1e-6), so that the grid reaches
// the range (the 1e-6 keeps quotients such as 0.3 / 0.1 at 3; a range below 1e-6 steps leaves the single point 0), at most `cap` (PPM_FRAME_MAX_STEPS); *clipped says that the cap
// cut the range.  The quotient is formed in double from the two floats.
PPM_HD inline int frame_steps(float range_px, float h, int cap, int *clipped) {
    int w = (int)std::ceil((double)range_px / (double)h - 1e-6);
    if (w < 0) w = 0;
    const int clip = w > cap;
    if (clipped) *clipped = clip;
    return clip ? cap : w;
}

}  // namespace ppm
