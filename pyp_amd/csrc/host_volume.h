// host_volume.h — what the map entry points share (ppm_mask_volume, ppm_create_mask, ppm_postprocess, ppm_local_resolution,
// ppm_fit_volume; DESIGN.md §2a′): device time per stage under PPM_TRACE, maps to the device and results back, the low-pass of a map,
// the k-th value by two histogram passes.  Included by ppm_lib.hip only, after host_ctx.h and ahead of host_mask.h.
#pragma once

namespace {

// PPM_TRACE: device time per named stage of a call, by pairs of pooled events on the call's stream.  A stage entered several times adds
// up.  Every event goes back to the pool when the call ends, whichever way it ends.
struct StageTimer {
    struct Span { const char *stage; hipEvent_t a, b; };
    const bool on = getenv("PPM_TRACE") != nullptr;
    std::vector<Span> spans;
    StageTimer() = default;
    StageTimer(const StageTimer &) = delete;
    StageTimer &operator=(const StageTimer &) = delete;
    ~StageTimer() {
        if (spans.empty()) return;
        std::lock_guard<std::mutex> lk(g_mu);
        for (auto &s : spans) { g.pool.push_back(s.a); g.pool.push_back(s.b); }
    }
    void begin(const char *stage) {
        if (!on) return;
        spans.push_back({stage, ev_get(), ev_get()});
        (void)hipEventRecord(spans.back().a, cur_stream());
    }
    void end() { if (on) (void)hipEventRecord(spans.back().b, cur_stream()); }
    // one line on stderr, after the call's last synchronisation: "who: header: stage X ms, stage Y ms, ..." in the order of first entry
    void report(const char *who, const std::string &header) const {
        if (!on) return;
        std::vector<std::pair<const char *, double>> total;
        for (auto &s : spans) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, s.a, s.b);
            auto it = std::find_if(total.begin(), total.end(), [&](const std::pair<const char *, double> &t) { return !strcmp(t.first, s.stage); });
            if (it == total.end()) total.push_back({s.stage, (double)ms}); else it->second += ms;
        }
        std::string line = std::string(who) + ": " + header + ":";
        char buf[96];
        for (size_t k = 0; k < total.size(); k++) {
            snprintf(buf, sizeof(buf), "%s %s %.3f ms", k ? "," : "", total[k].first, total[k].second);
            line += buf;
        }
        fprintf(stderr, "%s\n", line.c_str());
    }
};

// `count` floats of the caller's where the kernels can read them: the caller's own pointer if it is device memory (and, with aligned16,
// starts on a 16-byte boundary), a copy that lives as long as this object otherwise.  A null source stays null.
struct StagedMap {
    DevTmp<float> copy;             // copy.p: null where the caller's memory is read in place
    const float *p = nullptr;
    int in(const void *src, size_t count, int on_device, bool aligned16 = false) {
        p = (const float *)src;
        if (!src || (on_device && !(aligned16 && ((uintptr_t)src & 15)))) return 0;
        HIPCHK(copy.alloc(count));
        HIPCHK(hipMemcpyAsync(copy.p, src, count * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, cur_stream()));
        p = copy.p;
        return 0;
    }
};

// the result to where the caller wants it (nothing to do where it was built there); the caller synchronises
int copy_out(void *dst, const void *d_src, size_t count, int on_device) {
    if (dst == d_src) return 0;
    HIPCHK(hipMemcpyAsync(dst, d_src, count * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, cur_stream()));
    return 0;
}

// H(|k|) / n^3 by the integer |k|^2, up to the first radius at which the filter is zero for good
std::vector<float> mask_lowpass_table(int n, double r_c, double e) {
    const double r_end = r_c + 0.5 * e, r_one = r_c - 0.5 * e;
    const long k2_box = 3L * (n / 2) * (n / 2);
    const long nh = std::min(k2_box, (long)std::floor(r_end * r_end) + 1) + 1;
    const double inv = 1.0 / ((double)n * n * n);
    std::vector<float> t((size_t)nh);
    for (long k2 = 0; k2 < nh; k2++) {
        const double r = std::sqrt((double)k2);
        double h;
        if (r <= r_one) h = 1.0;
        else if (r >= r_end) h = 0.0;
        else h = 0.5 * (1.0 + std::cos(kPi * (r - r_one) / e));
        t[k2] = (float)(h * inv);
    }
    return t;
}

// a real map as the complex array the transforms take
int real_to_complex(const float *src, float2 *z, size_t n3) {
    hipLaunchKernelGGL(k_mask_r2c, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, cur_stream(), src, z, n3);
    HIPCHK(hipGetLastError());
    return 0;
}

// The low-pass of an n^3 map: cosine edge of width `edge` Fourier pixels about the radius r_c.  The table and its device copy live as
// long as the object (the device copy is freed first, which waits for the device), so the asynchronous upload never outlives its source.
struct LowPass {
    int n = 0;
    std::vector<float> h;
    DevTmp<float> d_h;
    int init(int n_, double r_c, double edge) {
        n = n_;
        h = mask_lowpass_table(n, r_c, edge);
        HIPCHK(d_h.alloc(h.size()));
        HIPCHK(hipMemcpyAsync(d_h.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, cur_stream()));
        return 0;
    }
    // forward, filter, back, in place: two transforms
    int apply(float2 *z) const {
        if (int rc = fft3d(z, n, false)) return rc;
        hipLaunchKernelGGL(k_mask_lowpass, dim3((unsigned)((n + 63) / 64), (unsigned)n, (unsigned)n), dim3(64), 0, cur_stream(), z, d_h.p, (int)h.size(), n);
        HIPCHK(hipGetLastError());
        return fft3d(z, n, true);
    }
};

// The k-th value of a set of floats on the device, 16 bits of its order-preserving key at a time (ppm_rank.h): two histograms, each
// cleared, filled by the caller's kernel, read back and walked.
struct RankPasses {
    std::vector<unsigned> hist;
    DevTmp<unsigned> d_hist;
    int alloc() { hist.resize(65536); HIPCHK(d_hist.alloc(65536)); return 0; }
    // launch(pass, prefix, bins on the device): the histogram of pass 0 (the keys' upper halves, bins0 bins) or of pass 1 (the lower halves
    // of the keys whose upper half is prefix, 65536 bins).  count(histogram of pass 0, its bins): which value is wanted, 1 = the first from
    // the bottom or, from_top, from the top.  Returns 0 and the key, 1 where a histogram holds fewer values than wanted, a negative code on a HIP error.
    template <typename Count, typename Launch>
    int run(int bins0, bool from_top, Count count, Launch launch, unsigned *key) {
        hipStream_t st = cur_stream();
        unsigned prefix = 0;
        long long want = 0;
        for (int pass = 0; pass < 2; pass++) {
            const int bins = pass == 0 ? bins0 : 65536;
            HIPCHK(hipMemsetAsync(d_hist.p, 0, bins * sizeof(unsigned), st));
            launch(pass, prefix, d_hist.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(hist.data(), d_hist.p, bins * sizeof(unsigned), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (pass == 0) want = count(hist.data(), bins);
            const RankBin r = rank_walk(hist.data(), bins, want, from_top);
            if (r.bin < 0) return 1;
            want = r.want;
            if (pass == 0) prefix = (unsigned)r.bin; else *key = (prefix << 16) | (unsigned)r.bin;
        }
        return 0;
    }
};

}  // namespace
