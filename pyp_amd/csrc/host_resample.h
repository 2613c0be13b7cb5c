// host_resample.h — ppm_resample, ppm_resize, ppm_fit_plan, ppm_fit_volume: Fourier resampling and real-space resizing of maps and image
// stacks (the work of cistem2's resample / resize and frealign_v9.11's resample_mp.exe).  Included by ppm_lib.hip only.
#pragma once

namespace {

constexpr long kResampleLds = 48 * 1024;         // dynamic LDS of a k_resample_lines block: three blocks share a CU's 160 KB
constexpr long kResampleMaxItems = 32768;        // items of one launch (they are a grid dimension of k_face_sums / k_resize)

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

std::string resample_sizes_hint(int n) {
    int lo = 0, hi = 0;
    resample_nearest_ok(n, &lo, &hi);
    std::string s = "the transforms take even sizes 32..512 with prime factors 2, 3, 5 and 7 only; nearest to " + std::to_string(n) + ":";
    if (lo) s += " " + std::to_string(lo);
    if (hi && hi != lo) s += std::string(lo ? " and " : " ") + std::to_string(hi);
    return s;
}

// one pass of k_resample_lines over strided lines (see ResampleLinesP)
int resample_pass(const float *src, float *dst, int N, int M, long nlines, long inner, long s_inner, long s_outer, long s_elem,
                  long d_inner, long d_outer, long d_elem, int line_major) {
    if (nlines <= 0) return 0;
    if (int rc = ensure_plan(N)) return rc;
    if (int rc = ensure_plan(M)) return rc;
    const int L = resample_lines_per_block(N, M, kResampleLds);
    if (L < 2) return fail(-22, "resample: the work arrays of these lengths do not fit the LDS");
    ResampleLinesP P;
    P.src = src; P.dst = dst; P.pn = g.plans[N].plan; P.pm = g.plans[M].plan; P.N = N; P.M = M; P.L = L; P.line_major = line_major;
    P.nlines = nlines; P.inner = inner; P.s_inner = s_inner; P.s_outer = s_outer; P.s_elem = s_elem;
    P.d_inner = d_inner; P.d_outer = d_outer; P.d_elem = d_elem; P.scale = (float)(1.0 / N);
    const bool al = aligned16(src) && aligned16(dst) && L % 4 == 0;
    if (line_major) P.vec = al && nlines % 4 == 0 && inner % 4 == 0 && s_inner == 1 && d_inner == 1 && s_outer % 4 == 0 && d_outer % 4 == 0 && s_elem % 4 == 0 && d_elem % 4 == 0;
    else P.vec = al;             // a block starts at line l0 = k L: l0 N and l0 M are multiples of 4
    hipLaunchKernelGGL(k_resample_lines, dim3((unsigned)((nlines + L - 1) / L)), dim3(256), (size_t)resample_lines_lds(N, M, L), cur_stream(), P);
    HIPCHK(hipGetLastError());
    return 0;
}

// n_items images (dims 2) or volumes (dims 3) of edge N in device memory -> edge M; `tmp` holds resample_tmp_floats() floats
size_t resample_tmp_floats(int dims, long n_items, int N, int M) {
    return dims == 2 ? (size_t)n_items * N * M : (size_t)N * N * M + (size_t)N * M * M;
}
int resample_device(const float *src, float *dst, int dims, long n_items, int N, int M, float *tmp) {
    if (N == M) {
        if (src != dst) HIPCHK(hipMemcpyAsync(dst, src, (size_t)n_items * (dims == 3 ? (size_t)N * N * N : (size_t)N * N) * sizeof(float), hipMemcpyDeviceToDevice, cur_stream()));
        return 0;
    }
    if (dims == 2) {
        // rows [n][N][N] -> [n][N][M], then columns -> [n][M][M] (tiles of adjacent columns)
        if (int rc = resample_pass(src, tmp, N, M, n_items * N, n_items * N, N, 0, 1, M, 0, 1, 0)) return rc;
        return resample_pass(tmp, dst, N, M, n_items * M, M, 1, (long)N * M, M, 1, (long)M * M, M, 1);
    }
    for (long v = 0; v < n_items; v++) {
        const float *s = src + (size_t)v * N * N * N;
        float *d = dst + (size_t)v * M * M * M, *t1 = tmp, *t2 = tmp + (size_t)N * N * M;
        const long nn = (long)N * N, nm = (long)N * M, mm = (long)M * M;
        if (int rc = resample_pass(s, t1, N, M, nn, nn, N, 0, 1, M, 0, 1, 0)) return rc;               // x: [N][N][N] -> [N][N][M]
        if (int rc = resample_pass(t1, t2, N, M, nm, M, 1, nm, M, 1, mm, M, 1)) return rc;             // y: -> [N][M][M]
        if (int rc = resample_pass(t2, d, N, M, mm, mm, 1, 0, mm, 1, 0, mm, 1)) return rc;             // z: -> [M][M][M]
    }
    return 0;
}

// stats[item] = {face mean, mean, standard deviation} of n_items (<= kResampleMaxItems) items in device memory (k_face_sums, k_face_stats);
// with `check` they are read back and an item whose deviation is 0 is refused (item0: its number in the caller's count)
int face_stats_device(const float *src, int dims, long n_items, int n, double *d_stats, bool check, long item0) {
    const long per = dims == 3 ? (long)n * n * n : (long)n * n;
    const int nchunk = (int)((per + kFaceChunk - 1) / kFaceChunk);
    DevTmp<double> t_part;
    HIPCHK(t_part.alloc((size_t)n_items * nchunk * 3));
    hipStream_t st = cur_stream();
    hipLaunchKernelGGL(k_face_sums, dim3((unsigned)nchunk, (unsigned)n_items), dim3(256), 0, st, src, t_part.p, n, dims, per, nchunk);
    hipLaunchKernelGGL(k_face_stats, dim3((unsigned)n_items), dim3(256), 0, st, t_part.p, d_stats, n, dims, per, nchunk);
    HIPCHK(hipGetLastError());
    std::vector<double> stats;
    if (check) {
        stats.resize((size_t)n_items * 3);
        HIPCHK(hipMemcpyAsync(stats.data(), d_stats, stats.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));                 // t_part is freed on return
    for (long i = 0; check && i < n_items; i++)
        if (!(stats[i * 3 + 2] > 0.0))
            return fail(-22, std::string("resize: ") + (dims == 3 ? "volume " : "image ") + std::to_string(item0 + i) + " has a standard deviation of 0 and cannot be normalised");
    return 0;
}

// Crop / pad of n_items (<= kResampleMaxItems) items in device memory; the statistics come first, so that a refusal (standard
// deviation 0 under `normalize`) leaves dst as it was.  pads (host, may be null): the pad value of every item.
int resize_device(const float *src, float *dst, int dims, long n_items, int n, int b, int normalize, float *pads, long item0) {
    const long per_out = dims == 3 ? (long)b * b * b : (long)b * b;
    DevTmp<double> t_stats; DevTmp<float> t_pad;
    HIPCHK(t_stats.alloc((size_t)n_items * 3));
    HIPCHK(t_pad.alloc((size_t)n_items));
    if (int rc = face_stats_device(src, dims, n_items, n, t_stats.p, normalize != 0, item0)) return rc;
    hipStream_t st = cur_stream();
    hipLaunchKernelGGL(k_resize, dim3((unsigned)((per_out + 255) / 256), (unsigned)n_items), dim3(256), 0, st, src, dst, t_stats.p, t_pad.p, n, b, dims, normalize);
    HIPCHK(hipGetLastError());
    if (pads) HIPCHK(hipMemcpyAsync(pads, t_pad.p, (size_t)n_items * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// items of one trip through the device for a host source: a share of the device's TOTAL memory (free memory is what other handles
// and the caller's own tensors happen to leave at this moment)
long resample_chunk_items(long n_items, size_t bytes_per_item) {
    const size_t budget = std::max((size_t)64 << 20, g.total_mem / 8);
    return std::max(1L, std::min(std::min(n_items, kResampleMaxItems), (long)(budget / std::max((size_t)1, bytes_per_item))));
}

}  // namespace

extern "C" int ppm_resample(const void *src, int on_device, int dims, long n_items, int n_in, int n_out, void *dst) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!src || !dst) return fail(-22, "null argument");
    if (dims != 2 && dims != 3) return fail(-22, "resample: dims must be 2 (a stack of images) or 3 (volumes), got " + std::to_string(dims));
    if (n_items < 1) return fail(-22, "resample: nothing to resample");
    if (!resample_len_ok(n_in)) return fail(-22, "resample: input size " + std::to_string(n_in) + " is not supported: " + resample_sizes_hint(n_in));
    if (!resample_len_ok(n_out)) return fail(-22, "resample: output size " + std::to_string(n_out) + " is not supported: " + resample_sizes_hint(n_out));
    HIPCHK(hipSetDevice(g.device));
    hipStream_t st = cur_stream();
    const size_t per_in = dims == 3 ? (size_t)n_in * n_in * n_in : (size_t)n_in * n_in, per_out = dims == 3 ? (size_t)n_out * n_out * n_out : (size_t)n_out * n_out;
    const size_t per_tmp = resample_tmp_floats(dims, 1, n_in, n_out);
    const long chunk = dims == 3 ? 1 : resample_chunk_items(n_items, (per_in + per_out + per_tmp) * sizeof(float));
    DevTmp<float> t_src, t_dst, t_tmp;
    if (n_in != n_out) HIPCHK(t_tmp.alloc(per_tmp * (size_t)chunk));
    if (!on_device) { HIPCHK(t_src.alloc(per_in * (size_t)chunk)); HIPCHK(t_dst.alloc(per_out * (size_t)chunk)); }
    for (long i0 = 0; i0 < n_items; i0 += chunk) {
        const long m = std::min(chunk, n_items - i0);
        const float *s = (const float *)src + (size_t)i0 * per_in;
        float *d = (float *)dst + (size_t)i0 * per_out;
        if (!on_device) { HIPCHK(hipMemcpyAsync(t_src.p, s, (size_t)m * per_in * sizeof(float), hipMemcpyHostToDevice, st)); s = t_src.p; }
        if (int rc = resample_device(s, on_device ? d : t_dst.p, dims, m, n_in, n_out, t_tmp.p)) return rc;
        if (!on_device) HIPCHK(hipMemcpyAsync(d, t_dst.p, (size_t)m * per_out * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return 0;
}

extern "C" int ppm_resize(const void *src, int on_device, int dims, long n_items, int n_in, int n_out, int normalize, void *dst, float *pad_values) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!src || !dst) return fail(-22, "null argument");
    if (dims != 2 && dims != 3) return fail(-22, "resize: dims must be 2 (a stack of images) or 3 (volumes), got " + std::to_string(dims));
    if (n_items < 1) return fail(-22, "resize: nothing to resize");
    if (n_in < 8 || n_in > 512 || n_out < 8 || n_out > 512) return fail(-22, "resize: sizes must be 8..512, got " + std::to_string(n_in) + " -> " + std::to_string(n_out));
    if (src == dst) return fail(-22, "resize: works out of place");
    HIPCHK(hipSetDevice(g.device));
    hipStream_t st = cur_stream();
    const size_t per_in = dims == 3 ? (size_t)n_in * n_in * n_in : (size_t)n_in * n_in, per_out = dims == 3 ? (size_t)n_out * n_out * n_out : (size_t)n_out * n_out;
    const long chunk = resample_chunk_items(n_items, (per_in + per_out) * sizeof(float));
    DevTmp<float> t_src, t_dst;
    if (!on_device) { HIPCHK(t_src.alloc(per_in * (size_t)chunk)); HIPCHK(t_dst.alloc(per_out * (size_t)chunk)); }
    if (normalize && n_items > chunk) {
        // a refusal must leave dst as it was: look at every item's deviation before the first chunk is written
        for (long i0 = 0; i0 < n_items; i0 += chunk) {
            const long m = std::min(chunk, n_items - i0);
            const float *s = (const float *)src + (size_t)i0 * per_in;
            if (!on_device) { HIPCHK(hipMemcpyAsync(t_src.p, s, (size_t)m * per_in * sizeof(float), hipMemcpyHostToDevice, st)); s = t_src.p; }
            DevTmp<double> t_stats;
            HIPCHK(t_stats.alloc((size_t)m * 3));
            if (int rc = face_stats_device(s, dims, m, n_in, t_stats.p, true, i0)) return rc;
        }
    }
    for (long i0 = 0; i0 < n_items; i0 += chunk) {
        const long m = std::min(chunk, n_items - i0);
        const float *s = (const float *)src + (size_t)i0 * per_in;
        float *d = (float *)dst + (size_t)i0 * per_out;
        if (!on_device) { HIPCHK(hipMemcpyAsync(t_src.p, s, (size_t)m * per_in * sizeof(float), hipMemcpyHostToDevice, st)); s = t_src.p; }
        if (int rc = resize_device(s, on_device ? d : t_dst.p, dims, m, n_in, n_out, normalize, pad_values ? pad_values + i0 : nullptr, i0)) return rc;
        if (!on_device) HIPCHK(hipMemcpyAsync(d, t_dst.p, (size_t)m * per_out * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return 0;
}

// host only: no device is touched (and none is needed)
extern "C" int ppm_fit_plan(int n_in, double pixel_in, double pixel_out, int box_out, ppm_fit_info *out) {
    if (!out) return fail(-22, "null argument");
    std::memset(out, 0, sizeof(*out));
    if (n_in < 8 || n_in > 512) return fail(-22, "fit: the reference must be 8..512 voxels, got " + std::to_string(n_in));
    if (box_out < 8 || box_out > 512) return fail(-22, "fit: the output box must be 8..512 voxels, got " + std::to_string(box_out));
    if (!(pixel_in > 0) || !(pixel_out > 0) || !std::isfinite(pixel_in) || !std::isfinite(pixel_out)) return fail(-22, "fit: pixel sizes must be positive");
    const FitPlan f = fit_plan(n_in, pixel_in, pixel_out, box_out);
    out->n_in = n_in; out->box_out = box_out; out->n_c = f.n_c; out->P = f.P; out->M = f.M;
    out->scale = f.scale; out->pixel_achieved = f.pixel_achieved; out->rel_error = f.rel_error;
    if (!f.P) return fail(-22, "fit: no supported size holds the " + std::to_string(f.n_c) + " voxels the output box shows");
    if (!f.ok) {
        char msg[256];
        snprintf(msg, sizeof msg, "fit: a pixel size of %.6g A is not within 1 %% of any supported pair of sizes for a %d-voxel reference at %.6g A; the best "
                 "is %d -> %d = %.6g A (%.2f %% off)", pixel_out, n_in, pixel_in, f.P, f.M, f.pixel_achieved, 100.0 * f.rel_error);
        return fail(-22, msg);
    }
    return 0;
}

extern "C" int ppm_fit_volume(const void *vol, int on_device, int n_in, double pixel_in, double pixel_out, int box_out, void *out, ppm_fit_info *info) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!vol || !out || !info) return fail(-22, "null argument");
    if (int rc = ppm_fit_plan(n_in, pixel_in, pixel_out, box_out, info)) return rc;
    HIPCHK(hipSetDevice(g.device));
    hipStream_t st = cur_stream();
    const int P = info->P, M = info->M, B = box_out;
    const size_t n3 = (size_t)n_in * n_in * n_in, p3 = (size_t)P * P * P, m3 = (size_t)M * M * M, b3 = (size_t)B * B * B;
    StagedMap s_in;
    DevTmp<float> t_p, t_m, t_tmp, t_out;
    if (int rc = s_in.in(vol, n3, on_device)) return rc;
    const float *d_in = s_in.p;
    float *d_out = (float *)out;
    if (!on_device) { HIPCHK(t_out.alloc(b3)); d_out = t_out.p; }
    HIPCHK(t_p.alloc(p3));
    HIPCHK(t_m.alloc(m3));
    if (P != M) HIPCHK(t_tmp.alloc(resample_tmp_floats(3, 1, P, M)));
    float pad1 = 0.f, pad2 = 0.f;
    if (int rc = resize_device(d_in, t_p.p, 3, 1, n_in, P, 0, &pad1, 0)) return rc;
    if (int rc = resample_device(t_p.p, t_m.p, 3, 1, P, M, t_tmp.p)) return rc;
    if (int rc = resize_device(t_m.p, d_out, 3, 1, M, B, 0, &pad2, 0)) return rc;
    if (int rc = copy_out(out, d_out, b3, on_device)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    info->pad_value_1 = pad1; info->pad_value_2 = pad2;
    return 0;
}
