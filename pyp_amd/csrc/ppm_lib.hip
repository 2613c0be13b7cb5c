// ppm_lib.hip — C-ABI entry points of libpypmatch.so (include/ppm.h) for MI355X (gfx950).
// Host glue only: workspace management, launch sequencing on one HIP stream, event timing.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/ppm.h"
#include "ppm_geom.h"
#include "ppm_sections.h"
#include "ppm_overlap.h"
#include "ppm_defocus_plan.h"
#include "ppm_sva_plan.h"
#include "ppm_kernels2.h"
#include "ppm_csp_kernels.h"
#include "ppm_frame_kernels.h"
#include "ppm_sva_kernels.h"
#include "ppm_gfft.h"
#include "ppm_mask_kernels.h"
#include "ppm_label_kernels.h"
#include "ppm_post_kernels.h"
#include "ppm_locres_kernels.h"
#include "ppm_resample_plan.h"
#include "ppm_resample_kernels.h"
#include "ppm_rank.h"
#include "ppm_ctf_plan.h"
#include "ppm_ctf_kernels.h"

using namespace ppm;

#include "host_ctx.h"
#include "host_refine.h"
#include "host_recon.h"
#include "host_csp.h"
#include "host_frames.h"
#include "host_sva.h"
#include "host_volume.h"
#include "host_mask.h"
#include "host_label.h"
#include "host_post.h"
#include "host_locres.h"
#include "host_resample.h"
#include "host_ctf.h"
