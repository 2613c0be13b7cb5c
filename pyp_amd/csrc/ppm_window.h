// ppm_window.h — where the values of k_global's folded shift window sit: one definition for the kernel's tail and its arg-max.
// Plain C++, no HIP types: compiled alone by tests/test_global_xfold_cpu.py.
//
// k_global<.., TWO = false> searches on the Ns = 128 grid with lane = kx: lanes l and l + 32 hold columns a quarter period apart,
//     e^{i j theta (l + 32)} = i^j e^{i j theta l},    theta = 2 pi / Ns,
// so that the two columns are FOLDED ahead of the x twiddles (a radix-4 step of the kx transform, as ppm_rows.h folds along ky).  With
// G the per-lane value of a window row, G' the one 32 lanes up, S = G + G', D = G - G', P = G + i G', Q = G - i G' and
// c_j = cos(j theta l), s_j = sin(j theta l), the sum over the 64 columns of shift jx becomes a sum over l < 32 of
//     jx = 0   S_x                       jx = +-2   D_x c_2 -+ D_y s_2
//     jx = +1  P_x c_1 - P_y s_1         jx = -1    Q_x c_1 + Q_y s_1
//     jx = +3  Q_x c_3 - Q_y s_3         jx = -3    P_x c_3 + P_y s_3
// The window rows iy = 0 .. NS - 1 (NS = 2 R + 1) are taken in pairs, SLOT s = rows 2 s and 2 s + 1: one 32-lane swap per register
// brings the column pair of row 2 s into lanes 0 - 31 (HALF 0) and that of row 2 s + 1 into lanes 32 - 63 (half 1).  A lane then forms
// the NS shift columns of its half's row for every slot — VALUE INDEX vi = s NS + ix, (R + 1) NS of them — and each half reduces its
// values over its own 32 lanes: lane l ends up with the total of value index bitrev5(l & 31).  The last slot has no second row: what
// its upper half holds is not a window position.
#pragma once

#ifndef PPM_HD
#ifdef __HIPCC__
#define PPM_HD __host__ __device__
#else
#define PPM_HD
#endif
#endif

namespace ppm {

PPM_HD constexpr int win_slots(int R) { return R + 1; }                        // row pairs of the (2 R + 1)-row window, the unpaired last row included
PPM_HD constexpr int win_values(int R) { return (R + 1) * (2 * R + 1); }       // values a lane forms and a half reduces (<= 32 for R <= 3)

// the value index lane `lane` holds after the halving reduction inside its half (five stages: 16, 8, 4, 2, 1)
PPM_HD inline int win_lane_value(int lane) {
    const int l = lane & 31;
    return ((l & 1) << 4) | ((l & 2) << 2) | (l & 4) | ((l & 8) >> 2) | ((l & 16) >> 4);
}
PPM_HD inline int win_lane_half(int lane) { return (lane >> 5) & 1; }

// Window position (iy, ix) of value index vi in half `half`; false: not a position of the window (an index beyond the values, or the
// upper half of the unpaired last row).
PPM_HD inline bool win_pos(int R, int vi, int half, int &iy, int &ix) {
    const int NS = 2 * R + 1;
    if (vi < 0 || vi >= win_values(R)) return false;
    const int slot = vi / NS;
    iy = 2 * slot + half; ix = vi - slot * NS;
    return iy < NS;
}

// ... and whether it competes in a search limited to +-RSx by +-RSy steps
PPM_HD inline bool win_valid(int R, int vi, int half, int RSx, int RSy, int &iy, int &ix) {
    if (!win_pos(R, vi, half, iy, ix)) return false;
    const int ay = iy < R ? R - iy : iy - R, ax = ix < R ? R - ix : ix - R;
    return ax <= RSx && ay <= RSy;
}

// the order of the arg-max: ties go to the lowest key, the scan order (sy, then sx) of the window
PPM_HD inline int win_key(int R, int iy, int ix) { return iy * (2 * R + 1) + ix; }

}  // namespace ppm
