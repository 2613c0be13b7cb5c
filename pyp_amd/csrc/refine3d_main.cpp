// refine3d — native drop-in for the program PYP scripts at src/pyp/refine/frealign/frealign.py:3918-3994
// ("<dir>/refine3d << eot >> log ... eot": 50 answers on stdin).
//
// The reference's refine3d is a compiled program; so is this one.  It covers the call PYP makes by default (a .cistem table in
// the standard column order, a float32 stack and reference, no statistics weighting, no priors, no matching projections, no 2-D
// focus mask) and does nothing but parse, prepare the reference (ppm_reference_create_padded), stream the particle range from
// the stack file into libpypmatch (include/ppm.h: ppm_host_read -> ppm_device_upload -> ppm_refine_batch) and write the output
// tables.  Everything else — the `.par` surface, the other answers, every input it would have to refuse — is handed to
// bin/refine3d.py (pyp_amd/surface/cli.py:refine3d_main) as a child process with the same stdin, BEFORE the GPU is touched, so
// that behaviour and messages have one definition.  With PPM_STACK_CACHE=1 the call is served by the resident per-GPU server
// (dropin_server.h): the context, the prepared reference and the particle range uploaded by an earlier call are already there.
//
// Built by pyp_amd/csrc/Makefile into bin/refine3d (g++, no HIP: the C ABI only).
#include "dropin_server.h"

using namespace dropin;

int main() {
    const auto t0 = Clock::now();
    const std::string input = read_all_stdin();
    auto fall_back = [&]() { hand_to_python("refine3d.py", input); };
    if (const char *e = getenv("PPM_NATIVE")) if (!strcmp(e, "0")) fall_back();
    RefineJob j;
    if (!refine_parse(input, j)) fall_back();
    {
        Reply rp;
        if (run_through_server(kProgRefine, input, rp)) {
            if (rp.status == kHandOver) fall_back();
            fputs(rp.text.c_str(), stdout); fflush(stdout);
            _exit(rp.status);
        }
    }
    // ---- from here on the GPU is in use: no more hand-overs.  The lock comes first (PYP may start several processes per node:
    // a waiting process holds neither a context nor page-locked memory); then the device, the page-locked staging buffers and the
    // reference are brought up by threads of their own while the parameter file is read.
    setenv("PPM_SYNC", "block", 0);
    const int lockfd = gpu_lock(device_index());
    long chunk_mb = 64, call_mb = 512;         // compute-bound: 64 MB chunks, 512 MB per refinement call (scripts/dropin_ab.py)
    if (const char *e = getenv("PPM_IO_CHUNK_MB")) chunk_mb = std::max(1L, atol(e));
    const size_t pin_bytes = staging_bytes(j.ilast - j.ifirst + 1, j.sec, chunk_mb);
    Stream st;
    const auto t_dev = Clock::now();
    StartUp up(device_index(), pin_bytes, st.pinned);
    ppm_ref_t *ref = nullptr; std::string ref_err; double ref_s = 0;          // the reference thread's, read after it is joined
    std::thread refmaker([&] {
        std::vector<float> vol;
        if (!read_volume(j.reference, j.box, vol)) ref_err = "ERROR: refine3d: cannot read the reference " + j.reference;
        else if (!up.wait_device()) ref_err = up.error();
        else {
            ref = ppm_reference_create_padded(vol.data(), j.box, (float)(j.box / 2.0), j.pad);
            if (!ref) ref_err = error_line(ppm_last_error());
        }
        ref_s = since(t_dev);
    });
    auto bail = [&](const std::string &msg) { leave(st, up, &refmaker, msg); };
    try { select_rows(j); } catch (const Fail &f) { bail(f.msg); }
    const long n = j.n;
    Out out;
    refine_banner(j, out, "native");
    const auto t1 = Clock::now();

    // ---- reader -> uploader -> refinement
    const StreamPlan plan = stream_plan(pin_bytes, n, j.sec, call_mb);
    up.want_pinned = plan.npin;
    st.wait_pinned = [&](int slot) { return up.wait_pinned(slot); };
    if (!up.wait_device()) bail(up.error());
    if (!st.start(plan, j)) bail("ERROR: refine3d: cannot open " + j.stack);
    std::vector<double> rout((size_t)n * 32);
    auto t2 = Clock::now();
    const Consumed done = consume(st, "refine3d", [&](void *ptr, long lo, long hi) {
        return ppm_refine_batch(ref, &j.cfg, ptr, 1, (int)(hi - lo), j.rin.data() + (size_t)lo * 32, rout.data() + (size_t)lo * 32);
    }, [&] { refmaker.join(); t2 = Clock::now(); return ref != nullptr; });       // the reference was prepared while the first images arrived
    if (!done.err.empty()) bail(!ref ? ref_err : !up.error().empty() ? up.error() : done.err);
    st.finish(); up.finish();
    const auto t3 = Clock::now();
    const std::string note = ppm_refine_note(ref);
    ppm_reference_destroy(ref);
    gpu_unlock(lockfd);
    double mean = 0;
    try { refine_outputs(j, rout, note, out, mean); } catch (const Fail &f) { bail(f.msg); }
    printf("\nRefined %ld particles in %.1f s; mean score %.4f\n", n, since(t0), mean);
    printf("Timing: inputs %.2f s, device + reference %.2f s, particles %.2f s, outputs %.2f s\n", secs(t0, t1), secs(t1, t2), secs(t2, t3), since(t3));
    printf("Start-up: device context %.2f s, reference ready %.2f s after the answers were read (threads of their own)\n", up.init_s, ref_s);
    printf("Pipeline: %ld chunks; reader: read %.2f s, waited for a buffer %.2f s; uploader: copied %.2f s, waited for a buffer %.2f s; main thread: computed %.2f s, "
           "waited for data %.2f s\n", done.ncalls, st.t_read, st.w_pin, st.t_up, st.w_dev, done.t_comp, done.w_data);
    printf("\nRefine3D: Normal termination\n\n");
    fflush(stdout);
    _exit(0);          // the library's reader pool is parked on purpose
}
