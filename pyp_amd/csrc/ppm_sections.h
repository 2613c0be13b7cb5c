// ppm_sections.h — sections of the grid search: contiguous ranges of grid directions whose slice banks are built and searched one
// after another, so that the angular step is limited by the per-particle tables alone and not by what the banks of the whole grid
// would take.  Plain C++, no HIP types: compiled alone by tests/test_grid_sections_plan.py.
//
// A section is a range of whole DIRECTIONS: the in-plane set of a direction is never split (k_gfft and k_global serve psi and
// psi + 180 deg from one stored slice).  Two limits decide the split:
//   * the transform path reads its bank (`bank4`) through a buffer descriptor whose size field has 32 bits: a section's bank4 stays
//     below 4 GB;
//   * the banks of one section together stay within a byte budget (host_refine.h: a share of the device's total memory, lowered by
//     PPM_BANK_BYTES in tests).
// The sections are as even as the direction count allows, so that every section's bank fits the allocation of the first.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace ppm {

struct GridSection { int d0, nd; };      // first direction, number of directions

constexpr uint64_t kBank4Limit = (uint64_t)1 << 32;      // a section's bank4 is smaller than this

// bank_slice_bytes / bank4_slice_bytes: bytes of one stored slice in k_global's bank and in k_gfft's (0: that bank is not in use).
// False with `err` set when not even one direction fits.
inline bool plan_sections(int n_dir, int npsi_store, uint64_t bank_slice_bytes, uint64_t bank4_slice_bytes, uint64_t budget,
                          std::vector<GridSection> &out, std::string &err) {
    out.clear();
    if (n_dir < 1 || npsi_store < 1 || bank_slice_bytes + bank4_slice_bytes == 0) { err = "grid search sections: empty grid"; return false; }
    const uint64_t per_dir = (uint64_t)npsi_store * (bank_slice_bytes + bank4_slice_bytes);
    uint64_t cap = budget / per_dir;
    if (bank4_slice_bytes) cap = std::min<uint64_t>(cap, (kBank4Limit - 1) / ((uint64_t)npsi_store * bank4_slice_bytes));
    if (cap < 1) {
        err = "slice bank of the grid search: the " + std::to_string(npsi_store) + " stored in-plane slices of one direction take " +
              std::to_string(per_dir) + " bytes, the bank may take " + std::to_string(budget) +
              (bank4_slice_bytes && budget >= per_dir ? " and 4 GB per section" : "") + "; use a coarser angular step or a narrower search band";
        return false;
    }
    if (cap > (uint64_t)n_dir) cap = (uint64_t)n_dir;
    const int S = (int)(((uint64_t)n_dir + cap - 1) / cap), base = n_dir / S, rem = n_dir % S;
    for (int s = 0, d = 0; s < S; s++) {
        const int nd = base + (s < rem ? 1 : 0);
        out.push_back({ d, nd });
        d += nd;
    }
    return true;
}

}  // namespace ppm
