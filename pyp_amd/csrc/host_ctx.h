// host_ctx.h — process context of libpypmatch.so: errors, streams, profiling, FFT plans, device buffers, the handle structs and the
// entry points that take no handle.  Included by ppm_lib.hip only (one translation unit).
#pragma once

namespace {

thread_local std::string g_err;
int fail(int code, const std::string &msg) { g_err = "ERROR: " + msg; return code; }

#define HIPCHK(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            g_err = std::string("ERROR: HIP: ") + hipGetErrorString(e_) + " at " #call;        \
            return -5;                                                                        \
        }                                                                                     \
    } while (0)
#define HIPCHKP(call)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            g_err = std::string("ERROR: HIP: ") + hipGetErrorString(e_) + " at " #call;        \
            return nullptr;                                                                   \
        }                                                                                     \
    } while (0)

struct Ctx {
    bool inited = false;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy = nullptr;     // uploads of the next chunk's images overlap the current chunk's kernels
    hipStream_t upload = nullptr;   // ppm_device_upload (may be called from a helper thread of the caller)
    struct PlanDev { FftPlan plan; bool ready = false; };
    PlanDev plans[513];             // FFT plans by length (tables live in device memory)
    size_t total_mem = 0;           // of the device (hipDeviceProp_t::totalGlobalMem): what the byte budgets of the workspaces are shares of
    int cu_count = 0;               // compute units: the resident grid of k_global (launch_global)
    size_t lds_per_cu = 0;          // bytes of LDS a CU shares among its blocks (ppm_overlap.h)
    bool prof_on = false;
    double prof_ms[PPM_K_COUNT] = { 0 };
    long prof_n[PPM_K_COUNT] = { 0 };
    struct Pending { int id; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
} g;

// Streams are per HANDLE (ppm_reference / ppm_accum own a compute and a copy stream each): an entry point that takes a handle makes
// them the calling thread's current streams for its duration (StreamScope), everything below launches on cur_stream().  Calls
// on DIFFERENT handles may therefore run concurrently from different threads; process-wide state (FFT plan tables, the profiling
// event lists) is guarded by g_mu.  Entry points without a handle use the library's own pair of streams.
thread_local hipStream_t tl_stream = nullptr, tl_copy = nullptr;
std::mutex g_mu;
inline hipStream_t cur_stream() { return tl_stream ? tl_stream : g.stream; }
inline hipStream_t cur_copy() { return tl_copy ? tl_copy : g.copy; }
struct StreamScope {
    hipStream_t ps, pc;
    StreamScope(hipStream_t s_, hipStream_t c_) : ps(tl_stream), pc(tl_copy) { tl_stream = s_; tl_copy = c_; if (g.inited) (void)hipSetDevice(g.device); }
    ~StreamScope() { tl_stream = ps; tl_copy = pc; }
};

hipEvent_t ev_get() {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g.pool.empty()) { hipEvent_t e = g.pool.back(); g.pool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}
void prof_flush() {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto &p : g.pending) {
        (void)hipEventSynchronize(p.b);
        float ms = 0; (void)hipEventElapsedTime(&ms, p.a, p.b);
        g.prof_ms[p.id] += ms; g.prof_n[p.id] += 1;
        g.pool.push_back(p.a); g.pool.push_back(p.b);
    }
    g.pending.clear();
}
struct ProfScope {
    int id; hipEvent_t a = nullptr;
    explicit ProfScope(int id_) : id(id_) { if (g.prof_on) { a = ev_get(); (void)hipEventRecord(a, cur_stream()); } }
    ~ProfScope() { if (a) { hipEvent_t b = ev_get(); (void)hipEventRecord(b, cur_stream()); std::lock_guard<std::mutex> lk(g_mu); g.pending.push_back({ id, a, b }); } }
};

// PPM_TRACE=1: wall-clock marks of a call on stderr (the device is synchronised at every mark, so the phases do not overlap when tracing)
struct Trace {
    const char *who; bool on; std::chrono::steady_clock::time_point t0;
    explicit Trace(const char *w) : who(w), on(getenv("PPM_TRACE") != nullptr), t0(std::chrono::steady_clock::now()) {}
    void mark(const char *what) const {
        if (!on) return;
        const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        (void)hipStreamSynchronize(cur_stream());
        fprintf(stderr, "%s: %8.2f ms  (host reached this mark)\n", who, host_ms);
        fprintf(stderr, "%s: %8.2f ms  %s\n", who, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), what);
    }
};

int ensure_plan(int n) {
    if (n < 2 || n > 512) return fail(-22, "FFT length out of range");
    std::lock_guard<std::mutex> lk(g_mu);
    if (g.plans[n].ready) return 0;
    std::vector<int> fac; std::vector<unsigned short> perm;
    fft_factors(n, fac, perm);
    int prod = 1; for (int f : fac) prod *= f;
    if (prod != n || fac.size() > 12) return fail(-22, "FFT length must have prime factors 2, 3, 5 and 7 only");
    std::vector<float2> t(n);
    for (int k = 0; k < n; k++) t[k] = make_float2((float)std::cos(2.0 * kPi * k / n), (float)std::sin(2.0 * kPi * k / n));
    float2 *dtw = nullptr; unsigned short *dperm = nullptr;
    HIPCHK(hipMalloc(&dtw, sizeof(float2) * n));
    HIPCHK(hipMalloc(&dperm, sizeof(unsigned short) * n));
    HIPCHK(hipMemcpy(dtw, t.data(), sizeof(float2) * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dperm, perm.data(), sizeof(unsigned short) * n, hipMemcpyHostToDevice));
    FftPlan &p = g.plans[n].plan;
    p.n = n; p.nfac = (int)fac.size(); for (size_t i = 0; i < fac.size(); i++) p.fac[i] = fac[i];
    p.tw = dtw; p.perm = dperm;
    g.plans[n].ready = true;
    return 0;
}


// one pass of length-n transforms over strided lines of `d` (see FftLinesP)
int fft_lines_pass(float2 *d, int n, long nlines, long inner, long inner_stride, long outer_stride, long elem_stride, int line_major, bool inverse) {
    if (nlines <= 0) return 0;
    if (int rc = ensure_plan(n)) return rc;
    int L = std::max(1, std::min(16, 7600 / (n + 1)));
    while (nlines % L) L--;
    FftLinesP P;
    P.data = d; P.plan = g.plans[n].plan; P.n = n; P.inverse = inverse ? 1 : 0; P.L = L; P.nlines = nlines;
    P.inner = inner; P.inner_stride = inner_stride; P.outer_stride = outer_stride; P.elem_stride = elem_stride; P.line_major = line_major;
    hipLaunchKernelGGL(k_fft_lines, dim3((unsigned)((nlines + L - 1) / L)), dim3(256), (size_t)L * (n + 1) * sizeof(float2), cur_stream(), P);
    HIPCHK(hipGetLastError());
    return 0;
}

// 2-D FFTs of `nimg` complex n x n images in place (rows, then columns)
int fft2d_batch(float2 *d, int n, long nimg, bool inverse) {
    const long nlines = nimg * n;
    if (int rc = fft_lines_pass(d, n, nlines, nlines, n, 0, 1, 0, inverse)) return rc;
    return fft_lines_pass(d, n, nlines, n, 1, (long)n * n, n, 1, inverse);
}

// 3-D FFT of an n^3 complex array in place (three strided passes through LDS: x, y, z)
int fft3d(float2 *d, int n, bool inverse) {
    const long nlines = (long)n * n;
    if (int rc = fft_lines_pass(d, n, nlines, nlines, n, 0, 1, 0, inverse)) return rc;
    if (int rc = fft_lines_pass(d, n, nlines, n, 1, nlines, n, 1, inverse)) return rc;
    return fft_lines_pass(d, n, nlines, nlines, 1, 0, nlines, 1, inverse);
}

// device buffer of a handle: grown on demand, freed with the handle (ppm_reference_destroy / ppm_accum_destroy list no buffers)
template <typename T>
struct DevBuf {
    T *p = nullptr; size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int ensure(size_t n) {
        if (n <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        HIPCHK(hipMalloc(&p, n * sizeof(T)));
        cap = n;
        return 0;
    }
};

// a kernel's limit of dynamic LDS, raised ahead of its first launch: one hipFuncSetAttribute per kernel and process, whoever launches it
int raise_lds_limit(const void *fn, int bytes) {
    static std::vector<const void *> raised;
    std::lock_guard<std::mutex> lk(g_mu);
    if (std::find(raised.begin(), raised.end(), fn) != raised.end()) return 0;
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    raised.push_back(fn);
    return 0;
}

// device temporary freed on every exit path (error returns included)
template <typename T>
struct DevTmp {
    T *p = nullptr;
    DevTmp() = default;
    DevTmp(const DevTmp &) = delete;
    DevTmp &operator=(const DevTmp &) = delete;
    ~DevTmp() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n * sizeof(T)); }
};


}  // namespace

// The per-chunk workspaces the local stage of ppm_refine_batch reads, as a set.  A handle has two: every chunk of a serial call takes
// lane[0]; when the call runs the local stage of a chunk beside the search of the next (ppm_overlap.h), chunks of odd index take lane[1],
// which the first such call allocates (ensure_lane, host_refine.h).
struct Lane { DevBuf<double> rows_in, rows_out; DevBuf<float> wring, cw, ddef; DevBuf<float2> Il; DevBuf<Hit> hits; DevBuf<LState> states, states2; };

// Workspaces of the searches without a grid search, by owner (DevBufs: grown on demand, reused across calls, freed with the handle).  An
// ensure may move a pointer: kernel parameters take `.p` after the last ensure of the buffers they name (see where CspEvalP / SvaEvalP are filled).
// Prepared spectra of a tilt series.  Grown and filled by csp_prepare_spectra only; read by csp, csp mode 4 and the frame refinement.
struct SpectraWs { DevBuf<float2> Il, band; DevBuf<float> cw, img, wring; DevBuf<double> rows; };
// State of the device-resident compass search (k_csp_step_*), one row per state.  Grown by ensure() only: csp_compass calls it per
// search, ppm_sva_align once per call for a chunk's states (allocating and freeing these per call cost 7 ms of a 57 ms alignment).
struct CompassWs {
    DevBuf<double> acc, dtrial, fpm, delta_t, tmean;
    int ensure(size_t n_states) {
        if (int rc = acc.ensure(n_states * 6)) return rc;
        if (int rc = dtrial.ensure(n_states * 6)) return rc;
        if (int rc = fpm.ensure(n_states * 12)) return rc;
        if (int rc = delta_t.ensure(n_states * 6)) return rc;
        return tmean.ensure(n_states);
    }
};
// The constrained search proper.  Grown by csp_upload_tables (the unit tables, delta, eval, out, uoff, mean), csp_compass and
// csp_global_rank (active), csp_defocus_sweep (states, out).
struct CspWs {
    DevBuf<double> N, p, tl, delta, s0, g0, out, mean; DevBuf<int> eval, rp, rt, slot, uoff, active; DevBuf<LState> states;
    // its exhaustive stage (k_csp_global), grown by csp_global_rank: per-row tables, per-rotation maxima of a particle chunk, the kept
    // candidates; and what ppm_csp_search_candidates answers from (the last call's candidates: PIND of every searched particle, K entries each)
    struct Search {
        DevBuf<double> rowtab; DevBuf<float> gbest, cscore; DevBuf<int> gshift, cshift; DevBuf<long> crot;
        std::vector<long> cand_unit, cand_rot; std::vector<int> cand_shift; std::vector<float> cand_score; int cand_K = 0;
    } search;
};
// Movie-frame refinement, grown by ppm_frame_refine only: the frame tables, the own and pooled maps, the slice store of a band too wide for LDS.
struct FrameWs { DevBuf<int> ints; DevBuf<float> flts, own, pool; DevBuf<double> dbls; DevBuf<float2> store; };
// Sub-volume transforms: the two work arrays (grown by sva_bind_work), staged host volumes and, in a reference, the band-limited transforms
// of a chunk (grown by ppm_sva_align / ppm_sva_insert).  GBs: allocating and freeing them on every call cost ~20 ms of a 120 ms call.
struct SvaWork { DevBuf<float2> f, g, F; DevBuf<float> vols; };
// The alignment's band: the sample list (built and sorted on the host: ~25 ms at 192^3 / 452 k samples) is kept while the band-pass settings
// stay, the window's transform at the samples (Fw) while the window stays; keys compare bit for bit.  Grown by sva_band_plan and sva_transform_chunk.
struct SvaBandKey {
    float box = 0, highpass_cutoff = 0, highpass_decay = 0, lowpass_cutoff = 0, lowpass_decay = 0;
    bool operator==(const SvaBandKey &o) const { return std::memcmp(this, &o, sizeof(o)) == 0; }
};
struct SvaWindowKey {
    float w[3] = { 0, 0, 0 }, sigma = 0;
    bool operator==(const SvaWindowKey &o) const { return std::memcmp(this, &o, sizeof(o)) == 0; }
};
struct SvaBandPlan {
    bool valid = false, fw_valid = false; SvaBandKey key; SvaWindowKey wkey;
    int S = 0; std::vector<int> shell_off; DevBuf<uint32_t> samples, pos; DevBuf<float> bandw; DevBuf<float2> Fw;
};

struct ppm_ref {
    hipStream_t stream = nullptr, copy = nullptr;       // this handle's compute and copy streams (StreamScope)
    hipStream_t local = nullptr;                        // second compute stream: the local stage of chunk i beside the search of chunk i + 1 (made on first use)
    int N = 0, B = 0, CX = 0, CY = 0, NBX = 0, NBY = 0, pad = 1; unsigned LB = 0;   // B, CX, CY count samples of the padded transform
    float2 *cube = nullptr;
    // workspaces (grown on demand, reused across calls)
    Lane lane[2];
    DevBuf<double> dir_theta, dir_phi;
    DevBuf<float> images, C2, nP, nI, cc, mats;
    SpectraWs spectra; CompassWs compass; CspWs csp; FrameWs frames;    // ppm_csp_refine, ppm_frame_refine (and the compass state of ppm_sva_align)
    SvaWork sva; SvaBandPlan sva_band;                                  // ppm_sva_align
    DevBuf<float2> band, Wp, bank, twN;
    DevBuf<float2> spill;            // k_prep outside the scratch-free path: the half spectrum between the row and the column phase, [n][N][W]
    DevBuf<float4> rowtw;            // k_global's row-pair twiddles for this reference's current search grid
    DevBuf<int> sh;
    DevBuf<uint32_t> samples;
    DevBuf<Hit> hits_t;              // per-tile top-K lists of a shift window wider than the kernel's
    DevBuf<int> tile_c;
    DevBuf<Hit> hits_s; DevBuf<int> sec_k;      // grid search in sections: the sections' top-K lists of a chunk and the offsets of the lists
    // full-window correlation (k_gfft): the bank in the column pass's layout, window maxima per (particle, orientation), column penalties
    DevBuf<float4> bank4; DevBuf<float> part, gtw;       // gtw: twiddle tables of the search grid (butterfly table, line table), then the window's column penalties
    std::string grid_key, bank_key, bank4_key; int gtw_ns = 0, gtw_rsx = -1;     // what mats / dir_* / twN / rowtw and the two banks hold (grid; grid + section)
    long last_counts[4] = { 0, 0, 0, 0 };
    int last_sections = 0;           // sections of the last call's grid search (0: it had none)
    int last_overlap = 0;            // hit-stage blocks per CU beside k_global in the last call (0: serial order)
    DevBuf<unsigned long long> reuse; long last_reuse[2] = { 0, 0 };    // tap reuse of the last call's full-band k_local launches (PPM_LOCAL_REUSE_COUNT=1): neighbour lane-gathers, reused ones
    std::string note;
};

struct ppm_accum {
    hipStream_t stream = nullptr, copy = nullptr;       // this handle's compute and copy streams (StreamScope)
    int N = 0; float pixel = 1.f;
    float *acc = nullptr; bool external = false;
    std::vector<double> symops; int nsym = 1;
    float *d_sym = nullptr;
    unsigned long long *d_counts = nullptr;
    unsigned *d_max = nullptr;       // chunk maxima for the fixed-point scales of k_insert_bricks
    long counts[2] = { 0, 0 };
    DevBuf<double> rows; DevBuf<float> images, dose; DevBuf<float2> band, spill; DevBuf<PartIns> pp; DevBuf<CullEnt> cull; DevBuf<BrickItem> items;
    SvaWork sva;                     // ppm_sva_insert: the transforms' work arrays and staged host volumes
    std::vector<float> brick_load; float load_r = -1.f; int n_items = 0, items_cap = -1;
};

// the reference's cube as the kernels address it
static CubeView cube_view(const ppm_ref *ref) {
    CubeView cv;
    cv.cube = ref->cube; cv.NBX = ref->NBX; cv.NBY = ref->NBY; cv.LB = ref->LB; cv.off = ref->B + 1; cv.scale = (float)ref->pad;
    return cv;
}

// tap addresses from LDS tables (ppm_dev.h) unless the tables would crowd the ring sums out of a CU (PPM_LOCAL_TABLES=0: arithmetic)
// the compass neighbours of the full-band k_local launch take the centre pose's taps where they can (PPM_LOCAL_REUSE=0: every lane gathers)
static bool local_reuse_wanted() { return !(getenv("PPM_LOCAL_REUSE") && atoi(getenv("PPM_LOCAL_REUSE")) == 0); }
static bool local_tables_wanted(int tabR) {
    return !(getenv("PPM_LOCAL_TABLES") && atoi(getenv("PPM_LOCAL_TABLES")) == 0) && cube_tab_bytes(tabR) <= 16 * 1024;
}
// ... and only where the ring sums of a launch (`ring_bytes` of dynamic LDS), the tables and the kernel's static LDS stay inside the
// 64 KB a launch may ask for (box 512 at the full band: arithmetic).  k_local and k_csp_eval share the test.
static bool tables_fit_lds(size_t ring_bytes, int tabR) { return ring_bytes + cube_tab_bytes(tabR) + 2048 <= (size_t)64 * 1024; }

// Double-buffered staging of host images for a chunk loop: `buf` holds two chunks of `chunk` images of `nn` floats; the first chunk is
// copied before the loop, chunk i + 1 travels on the copy stream while chunk i computes, and both streams are drained at the end of
// every chunk.  Images already in device memory are used where they are.
struct ChunkStager {
    const float *src; float *buf; bool on_device; int n_img, chunk; size_t nn;
    int prime() const {
        if (on_device) return 0;
        HIPCHK(hipMemcpyAsync(buf, src, (size_t)std::min(chunk, n_img) * nn * sizeof(float), hipMemcpyHostToDevice, cur_copy()));
        HIPCHK(hipStreamSynchronize(cur_copy()));
        return 0;
    }
    const float *chunk_ptr(int c0, int ci) const { return on_device ? src + (size_t)c0 * nn : buf + (size_t)(ci & 1) * chunk * nn; }
    int prefetch_next(int c0, int ci) const {
        if (on_device || c0 + chunk >= n_img) return 0;
        const int n_next = std::min(chunk, n_img - (c0 + chunk));
        HIPCHK(hipMemcpyAsync(buf + (size_t)((ci + 1) & 1) * chunk * nn, src + (size_t)(c0 + chunk) * nn, (size_t)n_next * nn * sizeof(float), hipMemcpyHostToDevice, cur_copy()));
        return 0;
    }
    int sync() const {
        HIPCHK(hipStreamSynchronize(cur_stream()));
        HIPCHK(hipStreamSynchronize(cur_copy()));
        return 0;
    }
};

// Error returns after a call's first enqueue drain the stream: pageable host memory that asynchronous copies still read or write (the
// run's own vectors, the caller's rows) must not go out of scope under them.  Declared BELOW every such host buffer, so that it is
// destroyed first; armed where the first enqueue happens; a success return goes through ok() and waits for nothing.
struct DrainOnError {
    bool armed = false;
    int ok() { armed = false; return 0; }
    ~DrainOnError() { if (armed) (void)hipStreamSynchronize(cur_stream()); }
};

static __global__ void k_noop() {}

extern "C" {

const char *ppm_last_error(void) { return g_err.c_str(); }
const char *ppm_version(void) { return "pypmatch 0.1 (gfx950)"; }
const char *ppm_build_id(void) { return "pypmatch " __DATE__ " " __TIME__; }
int ppm_device_mem_info(size_t *free_bytes, size_t *total_bytes) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    (void)hipSetDevice(g.device);
    size_t f = 0, t = 0;
    HIPCHK(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return 0;
}

int ppm_init(int device) {
    static std::mutex init_mu;                       // a caller may start the device from a helper thread and call again from its main thread
    std::lock_guard<std::mutex> lk(init_mu);
    const auto t_init0 = std::chrono::steady_clock::now();
    if (g.inited && g.device == device) { (void)hipSetDevice(device); return 0; }      // the current device is a per-thread setting
    if (g.inited) return fail(-16, "libpypmatch is bound to device " + std::to_string(g.device) + " in this process (one process per GPU); start another process for device " + std::to_string(device));
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(-19, "no HIP device visible; libpypmatch has no CPU path");
    if (device < 0 || device >= count) return fail(-22, "device index out of range");
    // how a host thread waits for the device: PPM_SYNC=block sleeps on an interrupt instead of spinning (the drop-in executables
    // set it: their reader threads need the cores a spinning wait would burn); default = the runtime's own choice
    if (const char *e = getenv("PPM_SYNC")) {
        const std::string v(e);
        (void)hipSetDeviceFlags(v == "block" ? hipDeviceScheduleBlockingSync : (v == "yield" ? hipDeviceScheduleYield : (v == "spin" ? hipDeviceScheduleSpin : hipDeviceScheduleAuto)));
    }
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return fail(-19, std::string("device is ") + prop.gcnArchName + ", libpypmatch is built for gfx950 only");
    g.total_mem = prop.totalGlobalMem;
    g.cu_count = std::max(1, prop.multiProcessorCount);
    g.lds_per_cu = std::max((size_t)prop.maxSharedMemoryPerMultiProcessor, (size_t)160 * 1024);     // gfx950: 160 KB, what the kernels' launches are sized for
    if (!g.stream) HIPCHK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    if (!g.copy) HIPCHK(hipStreamCreateWithFlags(&g.copy, hipStreamNonBlocking));
    if (!g.upload) HIPCHK(hipStreamCreateWithFlags(&g.upload, hipStreamNonBlocking));
    const auto t_ctx = std::chrono::steady_clock::now();
    // the code object is loaded at the first launch (tens of ms): here, where a caller can overlap it with its own start-up
    hipLaunchKernelGGL(k_noop, dim3(1), dim3(64), 0, g.stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g.stream));
    g.device = device; g.inited = true;
    if (getenv("PPM_TRACE"))
        fprintf(stderr, "ppm_init: context + streams %.1f ms, code object + first launch %.1f ms\n",
                std::chrono::duration<double, std::milli>(t_ctx - t_init0).count(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_ctx).count());
    return 0;
}

void ppm_profile_enable(int on) { g.prof_on = on != 0; }
void ppm_profile_reset(void) { prof_flush(); for (int i = 0; i < PPM_K_COUNT; i++) { g.prof_ms[i] = 0; g.prof_n[i] = 0; } }
int ppm_profile_get(int id, double *ms, long *n) {
    if (id < 0 || id >= PPM_K_COUNT) return fail(-22, "bad kernel id");
    prof_flush();
    if (ms) *ms = g.prof_ms[id];
    if (n) *n = g.prof_n[id];
    return 0;
}

// (the current device is a per-thread setting of the runtime: helper threads of the caller get the library's device here)
void *ppm_device_alloc(size_t bytes) { if (g.inited) (void)hipSetDevice(g.device); void *p = nullptr; if (hipMalloc(&p, bytes) != hipSuccess) { g_err = "ERROR: device allocation failed"; return nullptr; } return p; }
void ppm_device_free(void *p) { if (p) (void)hipFree(p); }
// own stream: a helper thread of the caller may upload the next chunk while another thread's library call computes (and uses
// cur_copy() for its internal double buffering); returns when the copy has completed
int ppm_device_upload(void *dst, const void *src, size_t bytes) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    HIPCHK(hipSetDevice(g.device));
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, g.upload));
    HIPCHK(hipStreamSynchronize(g.upload));
    return 0;
}
void *ppm_host_alloc(size_t bytes) { if (g.inited) (void)hipSetDevice(g.device); void *p = nullptr; if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { g_err = "ERROR: pinned host allocation failed"; return nullptr; } return p; }
void ppm_host_free(void *p) { if (p) (void)hipHostFree(p); }
// ---- file reads for the executables' reader stage: a persistent pool, one pread loop per part
extern "C++" {
namespace {
struct ReadPool {
    std::mutex mu;                      // one ppm_host_read at a time
    std::mutex qmu;
    std::condition_variable wake, done;
    std::vector<std::thread> threads;
    struct Part { int fd; long long off; char *dst; size_t bytes; };
    std::vector<Part> parts;
    size_t next = 0, pending = 0;
    int err = 0;
    bool quit = false;
    void worker() {
        std::unique_lock<std::mutex> lk(qmu);
        for (;;) {
            wake.wait(lk, [&] { return quit || next < parts.size(); });
            if (quit) return;
            Part p = parts[next++];
            lk.unlock();
            int e = 0;
            size_t got = 0;
            while (got < p.bytes) {
                ssize_t r = pread(p.fd, p.dst + got, std::min(p.bytes - got, (size_t)64 << 20), p.off + (long long)got);
                if (r < 0) { if (errno == EINTR) continue; e = -errno; break; }
                if (r == 0) { e = -5; break; }
                got += (size_t)r;
            }
            lk.lock();
            if (e && !err) err = e;
            if (--pending == 0) done.notify_all();
        }
    }
    int run(int fd, long long off, char *dst, size_t bytes, int nt) {
        std::lock_guard<std::mutex> one(mu);
        nt = std::max(1, std::min(nt, 16));
        std::unique_lock<std::mutex> lk(qmu);
        while ((int)threads.size() < nt) threads.emplace_back([this] { worker(); });
        // parts of whole MB so that every pread starts on a page boundary of the destination
        const size_t per = std::max((size_t)1 << 20, ((bytes + nt - 1) / nt + ((size_t)1 << 20) - 1) >> 20 << 20);
        parts.clear(); next = 0; err = 0;
        for (size_t a = 0; a < bytes; a += per) parts.push_back({fd, off + (long long)a, dst + a, std::min(per, bytes - a)});
        pending = parts.size();
        if (!pending) return 0;
        wake.notify_all();
        done.wait(lk, [&] { return pending == 0; });
        parts.clear(); next = 0;
        return err;
    }
    ~ReadPool() {
        { std::lock_guard<std::mutex> lk(qmu); quit = true; }
        wake.notify_all();
        for (auto &t : threads) t.join();
    }
};
ReadPool &read_pool() { static ReadPool *p = new ReadPool(); return *p; }      // leaked on purpose: no joins at process exit
}
}
int ppm_host_read(int fd, long long offset, void *dst, size_t bytes, int n_threads) {
    if (fd < 0 || offset < 0 || (!dst && bytes)) return fail(-22, "ppm_host_read: bad argument");
    int e = read_pool().run(fd, offset, (char *)dst, bytes, n_threads);
    if (e == -5) return fail(-5, "short read from the particle stack");
    if (e) return fail(e, std::string("reading the particle stack failed: ") + strerror(-e));
    return 0;
}

int ppm_device_sync(void) { if (cur_stream()) HIPCHK(hipStreamSynchronize(cur_stream())); HIPCHK(hipDeviceSynchronize()); return 0; }

int ppm_extract_boxes(const void *image, int image_on_device, int rows, int cols, const double *coords, int m,
                      int box, double coordinate_binning, double radius_px, int normalize, int fix_empty,
                      void *out, int out_on_device) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!image || !coords || !out) return fail(-22, "null argument");
    if (rows <= 0 || cols <= 0 || box < 2 || box > 4096 || !(coordinate_binning > 0)) return fail(-22, "bad extraction geometry");
    if (!(radius_px >= 0)) return fail(-22, "ppm_extract_boxes: radius_px is negative or not a number");
    // the kernel turns floor(coordinate / binning) into an int and adds the box to it: refuse what does not fit, before anything is enqueued
    for (int i = 0; i < m; i++)
        for (int a = 0; a < 2; a++) {
            const double f = floor(coords[2 * i + a] / coordinate_binning);
            if (!std::isfinite(coords[2 * i + a]) || !(fabs(f) <= 2147483647.0 - 2.0 * box))
                return fail(-22, "ppm_extract_boxes: coordinate " + std::to_string(i) + (a ? " (y)" : " (x)") + " is not finite or too large");
        }
    if (m <= 0) return 0;
    if (radius_px > box / 2.0) radius_px = box / 2.0;        // "Particle radius falls outside box" (image.py:323-331)
    float *d_img = nullptr, *d_out = nullptr;
    DevTmp<float> t_img, t_out; DevTmp<double> t_xy;
    const size_t npix = (size_t)rows * cols, nout = (size_t)m * box * box;
    if (image_on_device) d_img = (float *)image;
    else { HIPCHK(t_img.alloc(npix)); d_img = t_img.p; HIPCHK(hipMemcpy(d_img, image, npix * sizeof(float), hipMemcpyHostToDevice)); }
    if (out_on_device) d_out = (float *)out; else { HIPCHK(t_out.alloc(nout)); d_out = t_out.p; }
    HIPCHK(t_xy.alloc((size_t)m * 2));
    double *d_xy = t_xy.p;
    HIPCHK(hipMemcpyAsync(d_xy, coords, (size_t)m * 2 * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
    ExtractP P; P.image = d_img; P.rows = rows; P.cols = cols; P.coords = d_xy; P.box = box; P.cbin = coordinate_binning;
    P.radius2 = (float)(radius_px * radius_px); P.normalize = normalize; P.fix_empty = fix_empty; P.out = d_out;
    {
        ProfScope ps(PPM_K_EXTRACT);
        hipLaunchKernelGGL(k_extract, dim3(m), dim3(256), 0, cur_stream(), P);
    }
    HIPCHK(hipGetLastError());
    if (!out_on_device) HIPCHK(hipMemcpyAsync(out, d_out, nout * sizeof(float), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));
    return 0;
}

}  // extern "C"
