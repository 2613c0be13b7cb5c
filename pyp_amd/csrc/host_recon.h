// host_recon.h — reconstruction: the accumulator handle, particle insertion, the RCCL reduction and the finalisation.
#pragma once

// Work items of the brick insertion (k_insert_bricks): expected load of a brick = share of random slice planes that cut
// its box, estimated with a fixed set of normals; heavy bricks are cut into up to `cap` particle slices and the
// items are sorted heavy-first.  Bricks wholly outside the band carry no item.
static int build_brick_items(ppm_accum *a, const Geom &gm, int BE, int nb) {
    const int N = gm.N, nbx = (N / 2 + 1 + BE - 1) / BE, nby = (N + BE - 1) / BE;
    const float r = (float)gm.r_hi, hh = 0.5f * BE;
    if (a->load_r != r || a->brick_load.empty()) {
        const int NS = 192;
        std::vector<float> nrm(NS * 3);
        for (int i = 0; i < NS; i++) {          // Fibonacci sphere
            double z = 1.0 - 2.0 * (i + 0.5) / NS, ph = i * 2.399963229728653, rr = std::sqrt(std::max(0.0, 1.0 - z * z));
            nrm[i * 3] = (float)(rr * std::cos(ph)); nrm[i * 3 + 1] = (float)(rr * std::sin(ph)); nrm[i * 3 + 2] = (float)z;
        }
        a->brick_load.assign((size_t)nbx * nby * nby, -1.f);
        for (int bz = 0; bz < nby; bz++) for (int by = 0; by < nby; by++) for (int bx = 0; bx < nbx; bx++) {
            const int x_lo = bx * BE, y_lo = by * BE - N / 2, z_lo = bz * BE - N / 2;
            const float dx = std::max(std::max((float)x_lo, -(float)(x_lo + BE)), 0.f), dy = std::max(std::max((float)y_lo, -(float)(y_lo + BE)), 0.f),
                        dz = std::max(std::max((float)z_lo, -(float)(z_lo + BE)), 0.f);
            if (dx * dx + dy * dy + dz * dz >= r * r) continue;
            const float cx = x_lo + hh, cy = y_lo + hh, cz = z_lo + hh;
            int cut = 0;
            for (int i = 0; i < NS; i++) {
                const float *n = &nrm[i * 3];
                if (std::fabs(n[0] * cx + n[1] * cy + n[2] * cz) <= (std::fabs(n[0]) + std::fabs(n[1]) + std::fabs(n[2])) * hh) cut++;
            }
            a->brick_load[((size_t)bz * nby + by) * nbx + bx] = 0.02f + (float)cut / NS;
        }
        a->load_r = r; a->items_cap = -1;
    }
    constexpr int kBrickSlices = 16;        // most slices one brick's particles are split into
    const int minp_env = getenv("PPM_BRICK_MINP") ? atoi(getenv("PPM_BRICK_MINP")) : 1024;
    const int cap = std::max(1, std::min(kBrickSlices, nb / std::max(1, minp_env)));
    if (cap == a->items_cap) return 0;
    struct Tmp { BrickItem it; float load; };
    std::vector<Tmp> v;
    for (int bz = 0; bz < nby; bz++) for (int by = 0; by < nby; by++) for (int bx = 0; bx < nbx; bx++) {
        const float L = a->brick_load[((size_t)bz * nby + by) * nbx + bx];
        if (L < 0.f) continue;
        const int S = std::max(1, std::min(cap, (int)std::lround(L * kBrickSlices)));
        for (int sl = 0; sl < S; sl++) {
            Tmp t; t.it.bx = (unsigned short)bx; t.it.by = (unsigned short)by; t.it.bz = (unsigned short)bz; t.it.s = (unsigned char)sl; t.it.S = (unsigned char)S;
            t.load = L / S; v.push_back(t);
        }
    }
    std::stable_sort(v.begin(), v.end(), [](const Tmp &x, const Tmp &y) { return x.load > y.load; });
    std::vector<BrickItem> items(v.size());
    for (size_t i = 0; i < v.size(); i++) items[i] = v[i].it;
    if (int rc = a->items.ensure(items.size())) return rc;
    HIPCHK(hipMemcpyAsync(a->items.p, items.data(), items.size() * sizeof(BrickItem), hipMemcpyHostToDevice, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));
    a->n_items = (int)items.size(); a->items_cap = cap;
    return 0;
}

extern "C" {

// ------------------------------------------------------------------------------ reconstruction
size_t ppm_accum_floats(int box) { return (size_t)2 * box * box * (box / 2 + 1) * 3; }

ppm_accum_t *ppm_accum_create(int box, float pixel_size, const char *symmetry, void *ext) {
    if (!g.inited) { fail(-1, "ppm_init has not been called"); return nullptr; }
    if (!box_ok(box) || !(pixel_size > 0)) { fail(-22, "box must be even, 32..512, with prime factors 2, 3, 5, 7, and the pixel size positive"); return nullptr; }
    struct Undo { ppm_accum *p; ~Undo() { ppm_accum_destroy(p); } } guard{ new ppm_accum() };          // freed on every error return
    ppm_accum *a = guard.p;
    HIPCHKP(hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking));
    HIPCHKP(hipStreamCreateWithFlags(&a->copy, hipStreamNonBlocking));
    a->N = box; a->pixel = pixel_size;
    a->nsym = symmetry_ops(symmetry, a->symops);
    if (a->nsym < 1) { fail(-22, std::string("unknown symmetry symbol '") + (symmetry ? symmetry : "") + "'"); return nullptr; }
    size_t nf = ppm_accum_floats(box);
    if (ext) { a->acc = (float *)ext; a->external = true; }
    else {
        if (hipMalloc(&a->acc, nf * sizeof(float)) != hipSuccess) { a->acc = nullptr; fail(-12, "out of device memory for the accumulators"); return nullptr; }
        (void)hipMemset(a->acc, 0, nf * sizeof(float));
    }
    std::vector<float> s(a->symops.begin(), a->symops.end());
    HIPCHKP(hipMalloc(&a->d_sym, s.size() * sizeof(float)));
    HIPCHKP(hipMemcpy(a->d_sym, s.data(), s.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHKP(hipMalloc(&a->d_counts, 2 * sizeof(unsigned long long)));
    HIPCHKP(hipMemset(a->d_counts, 0, 2 * sizeof(unsigned long long)));
    HIPCHKP(hipMalloc(&a->d_max, 2 * sizeof(unsigned)));
    if (raise_lds_limit((const void *)k_insert_bricks<16, 16>, 17 * (17 * 52 + 3) * 8)) return nullptr;
    return std::exchange(guard.p, nullptr);
}

// the workspaces (DevBuf) go with `delete`, after the streams: see ppm_reference_destroy
void ppm_accum_destroy(ppm_accum_t *a) {
    if (!a) return;
    if (a->acc && !a->external) (void)hipFree(a->acc);
    if (a->d_sym) (void)hipFree(a->d_sym);
    if (a->d_counts) (void)hipFree(a->d_counts);
    if (a->d_max) (void)hipFree(a->d_max);
    if (a->stream) (void)hipStreamDestroy(a->stream);
    if (a->copy) (void)hipStreamDestroy(a->copy);
    delete a;
}

int ppm_insert_batch(ppm_accum_t *a, const ppm_recon_cfg *cfg, const void *images, int images_on_device, int n_img, const double *rows) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!a || !cfg || !images || !rows) return fail(-22, "null argument");
    StreamScope ss_(a->stream, a->copy);
    if (cfg->box != a->N) return fail(-22, "box differs from the accumulator's");
    if (n_img <= 0) return 0;
    ppm_refine_cfg rc; std::memset(&rc, 0, sizeof(rc));
    rc.box = a->N; rc.pixel_size = cfg->pixel_size; rc.res_high = cfg->res_limit > 0 ? cfg->res_limit : 2.f * cfg->pixel_size; rc.angular_step = 15.f;
    Geom gm; std::string err;
    if (!geom_init(gm, rc, err)) return fail(-22, err);
    const size_t NN = (size_t)gm.N * gm.N, HW = (size_t)gm.H * gm.W;
    // particles per k_prep / k_insert_bricks launch: 16 GB of images + band spectra (32 k particles at 256^2) where the device has them to
    // spare, 8 GB otherwise; swept on the 500 k x 256^2 reconstruction (scripts/sweep_insert2.sh): 4 / 8 / 16 / 24 / 32 / 48 GB -> 1.44 / 1.51 /
    // 1.55 / 1.54 / 1.54 / 1.54 M particles/s
    size_t chunk_gb = 8;
    {
        size_t free_b = 0, total_b = 0;
        // ... and only for calls of at least four such chunks: the buffers are allocated per accumulator, and a 100 k-particle call
        // through the resident server (0.18 s in all) lost more to the larger allocation than the launches gained
        const bool big_call = (size_t)n_img * (NN * 4 + HW * 8) >= ((size_t)64 << 30);
        if (big_call && hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b >= ((size_t)128 << 30) && free_b >= ((size_t)64 << 30)) chunk_gb = 16;
    }
    if (getenv("PPM_INSERT_GB")) chunk_gb = (size_t)std::max(1, atoi(getenv("PPM_INSERT_GB")));
    int CH = (int)std::min<size_t>((size_t)n_img, std::max<size_t>(32, (chunk_gb << 30) / (NN * 4 + HW * 8)));
    CH = std::min(CH, 32768);
    if (const char *e = std::getenv("PPM_CHUNK")) { int v = std::atoi(e); if (v > 0) CH = std::min(CH, v); }   // tests: force several chunks
    if (int r = a->rows.ensure((size_t)CH * PPM_NCOL)) return r;
    if (!images_on_device) if (int r = a->images.ensure((size_t)2 * CH * NN)) return r;       // double-buffered staging
    if (int r = a->band.ensure((size_t)CH * HW)) return r;
    const float *d_dose = nullptr;
    float dose_cap2 = 1.f;
    if (cfg->dose_weights && cfg->n_dose_weights > 0 && cfg->dose_exponent > 0) {
        if (int r = a->dose.ensure(cfg->n_dose_weights)) return r;
        HIPCHK(hipMemcpyAsync(a->dose.p, cfg->dose_weights, (size_t)cfg->n_dose_weights * sizeof(float), hipMemcpyHostToDevice, cur_stream()));
        d_dose = a->dose.p;
        const float tr = cfg->dose_transition > 0 && cfg->dose_transition <= 1 ? cfg->dose_transition : 1.f;
        dose_cap2 = (tr * gm.N / 2) * (tr * gm.N / 2);
    }
    const ChunkStager stage{ (const float *)images, a->images.p, images_on_device != 0, n_img, CH, NN };
    if (int r = stage.prime()) return r;
    for (int c0 = 0, ci = 0; c0 < n_img; c0 += CH, ci++) {
        const int nb = std::min(CH, n_img - c0);
        HIPCHK(hipMemcpyAsync(a->rows.p, rows + (size_t)c0 * PPM_NCOL, (size_t)nb * PPM_NCOL * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
        const float *d_img = stage.chunk_ptr(c0, ci);
        // the chunk's value bounds ([0] max |band| from k_prep, [1] max weight from k_insert_params) scale the fixed point
        HIPCHK(hipMemsetAsync(a->d_max, 0, 2 * sizeof(unsigned), cur_stream()));
        if (int prc = launch_prep(a->spill, d_img, a->rows.p, nb, gm, (double)cfg->mask_radius / (double)cfg->pixel_size, 1.f, cfg->normalize, cfg->invert, 0, 0,
                                  a->band.p, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, a->d_max)) return prc;
        // per-particle constants, then one block per (brick, particle slice, half)
        if (int r = a->pp.ensure(nb)) return r;
        if (int r = a->cull.ensure((size_t)nb * a->nsym)) return r;
        hipLaunchKernelGGL(k_insert_params, dim3((nb + 255) / 256), dim3(256), 0, cur_stream(), a->rows.p, a->pp.p, a->cull.p, a->d_sym, a->nsym, nb, gm.N, (double)cfg->pixel_size,
                           (double)cfg->score_weight_bfactor, (double)cfg->score_average, (double)cfg->score_threshold, cfg->split_by_pind,
                           gm.r_hi * gm.r_hi, a->d_counts, a->d_max, d_dose, cfg->n_dose_weights, cfg->dose_exponent, dose_cap2);
        const int BE = gm.N >= 128 ? 16 : 8;
        if (int r = build_brick_items(a, gm, BE, nb)) return r;
        InsertBrickP IP;
        IP.band = a->band.p; IP.pp = a->pp.p; IP.cull = a->cull.p; IP.symops = a->d_sym; IP.nsym = a->nsym; IP.acc = a->acc;
        IP.N = gm.N; IP.B = gm.B; IP.W = gm.W; IP.H = gm.H; IP.n_img = nb; IP.items = a->items.p; IP.maxima = a->d_max;
        IP.r2 = (float)(gm.r_hi * gm.r_hi);
        {
            ProfScope ps(PPM_K_INSERT);
            dim3 grid((unsigned)a->n_items, 2);
            if (BE == 16) hipLaunchKernelGGL((k_insert_bricks<16, 16>), grid, dim3(1024), 17 * (17 * 52 + 3) * sizeof(long long), cur_stream(), IP);
            else hipLaunchKernelGGL((k_insert_bricks<8, 4>), grid, dim3(256), 9 * (9 * 28 + 3) * sizeof(long long), cur_stream(), IP);
        }
        HIPCHK(hipGetLastError());
#ifdef PPM_INS_STAMPS
        {   // diagnostic build: cycles per phase summed over the waves of this launch (ppm_kernels2.h)
            unsigned long long st[24], z[24] = { 0 };
            HIPCHK(hipStreamSynchronize(cur_stream()));
            HIPCHK(hipMemcpyFromSymbol(st, HIP_SYMBOL(g_ins_stamps), sizeof(st)));
            HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_ins_stamps), z, sizeof(z)));
            const char *names[10] = { "zero brick", "cull", "wait after cull", "cut set-up", "row intervals + prefix", "deal-out + test", "evaluate 64", "evaluate tail", "wait at round end", "write-back" };
            double tot = 0; for (int i = 0; i < 10; i++) tot += (double)st[i];
            fprintf(stderr, "k_insert_bricks stamps, %d particles, %d items:", nb, a->n_items);
            for (int i = 0; i < 10; i++) fprintf(stderr, " | %s %.1f%%", names[i], 100.0 * (double)st[i] / tot);
            fprintf(stderr, " || wave-cycles per particle %.0f, cuts per particle %.1f, candidates per cut %.1f, hits per cut %.1f, full evaluations per cut %.2f, tails per cut %.2f\n",
                    tot / nb, (double)st[12] / nb, (double)st[13] / (double)st[12], (double)st[14] / (double)st[12], (double)st[15] / (double)st[12], (double)st[16] / (double)st[12]);
        }
#endif
        if (int r = stage.prefetch_next(c0, ci)) return r;
        if (int r = stage.sync()) return r;
    }
    unsigned long long c[2];
    HIPCHK(hipMemcpy(c, a->d_counts, sizeof(c), hipMemcpyDeviceToHost));
    a->counts[0] = (long)c[0]; a->counts[1] = (long)c[1];
    return 0;
}

long ppm_accum_count(ppm_accum_t *a, int half) { return (a && (half == 0 || half == 1)) ? a->counts[half] : -1; }
void ppm_accum_set_count(ppm_accum_t *a, int half, long count) {
    if (!a || (half != 0 && half != 1)) return;
    a->counts[half] = count;
    unsigned long long c = (unsigned long long)count;
    (void)hipMemcpy(a->d_counts + half, &c, sizeof(c), hipMemcpyHostToDevice);
}

int ppm_accum_download(ppm_accum_t *a, float *host) {
    if (!a || !host) return fail(-22, "null argument");
    StreamScope ss_(a->stream, a->copy);
    HIPCHK(hipStreamSynchronize(cur_stream()));
    HIPCHK(hipMemcpy(host, a->acc, ppm_accum_floats(a->N) * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int ppm_accum_download_range(ppm_accum_t *a, float *host, size_t first, size_t count) {
    if (!a || !host) return fail(-22, "null argument");
    if (first > ppm_accum_floats(a->N) || count > ppm_accum_floats(a->N) - first) return fail(-22, "range beyond the accumulators");
    StreamScope ss_(a->stream, a->copy);
    HIPCHK(hipStreamSynchronize(cur_stream()));
    HIPCHK(hipMemcpy(host, a->acc + first, count * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int ppm_accum_add(ppm_accum_t *a, const float *host) {
    if (!a || !host) return fail(-22, "null argument");
    StreamScope ss_(a->stream, a->copy);
    size_t nf = ppm_accum_floats(a->N);
    DevTmp<float> tmp;
    HIPCHK(tmp.alloc(nf));
    HIPCHK(hipMemcpy(tmp.p, host, nf * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_axpy, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, cur_stream(), a->acc, tmp.p, nf);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(cur_stream()));
    return 0;
}

// ------------------------------------------------------------------------------ the one collective of the path (RCCL)
// librccl is opened on first use (dlopen), not linked: the single-GPU executables never pay for loading it.  Only the plain C
// entry points of rccl.h are used; their prototypes are restated here so that the library builds without the RCCL headers.
namespace {
struct Rccl {
    void *h = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, ppm_comm_id, int) = nullptr;      // ncclUniqueId is passed by value: 128 opaque bytes
    int (*CommDestroy)(void *) = nullptr;
    int (*CommCount)(const void *, int *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*Reduce)(const void *, void *, size_t, int, int, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    std::string err;
};
static void rccl_load(Rccl &r) {
    const char *names[] = { getenv("PPM_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" };
    for (const char *n : names) { if (!n) continue; r.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (r.h) break; }
    if (!r.h) { r.err = std::string("librccl could not be opened: ") + dlerror(); return; }
    auto sym = [&](const char *n) { void *p = dlsym(r.h, n); if (!p && r.err.empty()) r.err = std::string("librccl lacks ") + n; return p; };
    r.GetUniqueId = (int (*)(void *))sym("ncclGetUniqueId");
    r.CommInitRank = (int (*)(void **, int, ppm_comm_id, int))sym("ncclCommInitRank");
    r.CommDestroy = (int (*)(void *))sym("ncclCommDestroy");
    r.CommCount = (int (*)(const void *, int *))sym("ncclCommCount");
    r.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))sym("ncclAllReduce");
    r.Reduce = (int (*)(const void *, void *, size_t, int, int, int, void *, hipStream_t))sym("ncclReduce");
    r.GetErrorString = (const char *(*)(int))sym("ncclGetErrorString");
}
static Rccl &rccl() {           // opened once, whichever thread asks first (the handle-less entry points are thread-safe, include/ppm.h)
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, rccl_load, std::ref(r));
    return r;
}
constexpr int kNcclInt64 = 4, kNcclFloat32 = 7, kNcclSum = 0;      // ncclDataType_t / ncclRedOp_t values of rccl.h
int rccl_fail(Rccl &r, int rc, const char *what) {
    return fail(-5, std::string(what) + " failed: " + (r.GetErrorString ? r.GetErrorString(rc) : "RCCL error") + " (" + std::to_string(rc) + ")");
}
}  // namespace

int ppm_comm_unique_id(ppm_comm_id *id) {
    if (!id) return fail(-22, "null argument");
    Rccl &r = rccl();
    if (!r.err.empty()) return fail(-38, r.err);
    static_assert(sizeof(ppm_comm_id) == 128, "ncclUniqueId is 128 bytes");
    if (int rc = r.GetUniqueId(id)) return rccl_fail(r, rc, "ncclGetUniqueId");
    return 0;
}

void *ppm_comm_create(int n_ranks, int rank, const ppm_comm_id *id) {
    if (!g.inited) { fail(-1, "ppm_init has not been called"); return nullptr; }
    if (!id || n_ranks < 1 || rank < 0 || rank >= n_ranks) { fail(-22, "bad communicator arguments"); return nullptr; }
    Rccl &r = rccl();
    if (!r.err.empty()) { fail(-38, r.err); return nullptr; }
    void *comm = nullptr;
    (void)hipSetDevice(g.device);                    // the communicator binds to the calling thread's current device
    if (int rc = r.CommInitRank(&comm, n_ranks, *id, rank)) { rccl_fail(r, rc, "ncclCommInitRank"); return nullptr; }
    return comm;
}

int ppm_comm_count(void *comm) {
    if (!comm) return fail(-22, "null communicator");
    Rccl &r = rccl();
    if (!r.err.empty()) return fail(-38, r.err);
    int n = 0;
    if (int rc = r.CommCount(comm, &n)) return rccl_fail(r, rc, "ncclCommCount");
    return n;
}

void ppm_comm_destroy(void *comm) {
    Rccl &r = rccl();
    if (comm && r.CommDestroy) (void)r.CommDestroy(comm);
}

int ppm_accum_reduce(ppm_accum_t *a, void *comm, int root) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!a || !comm) return fail(-22, "null argument");
    StreamScope ss_(a->stream, a->copy);
    Rccl &r = rccl();
    if (!r.err.empty()) return fail(-38, r.err);
    const size_t nf = ppm_accum_floats(a->N);
    // the particle counters travel with the sums: brought up to date on the device, reduced as two int64
    unsigned long long c[2] = { (unsigned long long)a->counts[0], (unsigned long long)a->counts[1] };
    HIPCHK(hipMemcpyAsync(a->d_counts, c, sizeof(c), hipMemcpyHostToDevice, cur_stream()));
    int rc;
    if (root < 0) {
        rc = r.AllReduce(a->acc, a->acc, nf, kNcclFloat32, kNcclSum, comm, cur_stream());
        if (!rc) rc = r.AllReduce(a->d_counts, a->d_counts, 2, kNcclInt64, kNcclSum, comm, cur_stream());
    } else {
        rc = r.Reduce(a->acc, a->acc, nf, kNcclFloat32, kNcclSum, root, comm, cur_stream());
        if (!rc) rc = r.Reduce(a->d_counts, a->d_counts, 2, kNcclInt64, kNcclSum, root, comm, cur_stream());
    }
    if (rc) return rccl_fail(r, rc, root < 0 ? "ncclAllReduce" : "ncclReduce");
    HIPCHK(hipMemcpyAsync(c, a->d_counts, sizeof(c), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));
    a->counts[0] = (long)c[0]; a->counts[1] = (long)c[1];      // on ranks other than a root the values are undefined, as ncclReduce leaves them
    return 0;
}

int ppm_finalize(ppm_accum_t *a, const ppm_final_cfg *cfg, float *half1, float *half2, float *filtered, double *stats) {
    if (!g.inited) return fail(-1, "ppm_init has not been called");
    if (!a || !cfg) return fail(-22, "null argument");
    StreamScope ss_(a->stream, a->copy);
    const int N = a->N, ns = N / 2;
    const double px = a->pixel;
    const size_t nf = ppm_accum_floats(N), n3 = (size_t)N * N * N, tot = (size_t)N * N * (N / 2 + 1);
    DevTmp<float> t_tmp, t_out; DevTmp<double> t_s; DevTmp<float2> t_f;
    HIPCHK(t_tmp.alloc(nf));
    HIPCHK(t_s.alloc((size_t)8 * ns));
    float *tmp = t_tmp.p; double *d_s = t_s.p;
    // every device step of the finalisation is ordered on the handle's stream: the stream is non-blocking, so a plain hipMemset / hipMemcpy
    // (legacy null stream) is not ordered against the kernels below and the shell sums could start from a buffer not yet zeroed
    HIPCHK(hipMemsetAsync(d_s, 0, 8 * ns * sizeof(double), cur_stream()));
    HIPCHK(hipMemcpyAsync(tmp, a->acc, nf * sizeof(float), hipMemcpyDeviceToDevice, cur_stream()));
    {
    ProfScope ps(PPM_K_FINAL);
    hipLaunchKernelGGL(k_fold_plane, dim3((unsigned)(((size_t)2 * N * N + 255) / 256)), dim3(256), 0, cur_stream(), a->acc, tmp, N);
    hipLaunchKernelGGL(k_shell_den, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, cur_stream(), tmp, d_s, N);
    hipLaunchKernelGGL(k_shell_fsc, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, cur_stream(), tmp, d_s, d_s + 4 * ns, N);
    }
    std::vector<double> hs(8 * ns);
    HIPCHK(hipMemcpyAsync(hs.data(), d_s, 8 * ns * sizeof(double), hipMemcpyDeviceToHost, cur_stream()));
    HIPCHK(hipStreamSynchronize(cur_stream()));
    double vfrac = cfg->molecular_mass_kda > 0 ? (cfg->molecular_mass_kda * 1000.0 / 0.81) / std::pow(N * px, 3.0) : 1.0;
    vfrac = std::min(1.0, std::max(1e-6, vfrac));
    std::vector<double> kap(ns);
    for (int b = 0; b < ns; b++) {
        double c12 = hs[4 * ns + b], c11 = hs[5 * ns + b], c22 = hs[6 * ns + b], cnt = hs[2 * ns + b], sdt = hs[3 * ns + b];
        double fsc = (c11 > 0 && c22 > 0) ? c12 / std::sqrt(c11 * c22) : 0.0;
        double fc = fsc < 0 ? 0 : (fsc > 0.999 ? 0.999 : fsc);
        double rec = 2.0 * fc / (1.0 - fc), md = cnt > 0 ? sdt / cnt : 0;
        kap[b] = b == 0 ? 1e-20 : md / (rec > 1e-6 ? rec : 1e-6);
        if (b >= 1 && stats) {
            double *s = stats + (size_t)(b - 1) * PPM_STATS_COLS;
            s[0] = b; s[1] = N * px / b; s[2] = b / (N * px); s[3] = fsc;
            s[4] = fc / (fc + vfrac * (1 - fc)); s[5] = md > 0 ? rec / md / vfrac : 0; s[6] = rec;
        }
    }
    HIPCHK(hipMemcpyAsync(d_s, kap.data(), ns * sizeof(double), hipMemcpyHostToDevice, cur_stream()));     // kap outlives the syncs below
    HIPCHK(t_f.alloc(n3));
    HIPCHK(t_out.alloc(n3));
    float2 *d_f = t_f.p; float *d_out = t_out.p;
    float *outs[3] = { half1, half2, filtered };
    const float rout = (float)(cfg->outer_radius / px), rin = (float)(cfg->inner_radius / px);
    const float fo = (float)((cfg->mask_falloff > 0 ? cfg->mask_falloff : 10.0) / px);
    for (int which = 0; which < 3; which++) {
        if (!outs[which]) continue;
        {
            ProfScope p2(PPM_K_FINAL);
            HIPCHK(hipMemsetAsync(d_f, 0, n3 * sizeof(float2), cur_stream()));
            hipLaunchKernelGGL(k_wiener, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, cur_stream(), tmp, d_s, d_f, N, which);
            if (int rc = fft3d(d_f, N, true)) return rc;
            hipLaunchKernelGGL(k_map_post, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, cur_stream(), d_f, d_out, N, rout, rin, fo);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(outs[which], d_out, n3 * sizeof(float), hipMemcpyDeviceToHost, cur_stream()));
        HIPCHK(hipStreamSynchronize(cur_stream()));
    }
    return 0;
}

}  // extern "C"
