// reconstruct3d — native drop-in for the program PYP scripts at src/pyp/refine/frealign/frealign.py:1780-1824
// ("<dir>/reconstruct3d << eot >> log ... eot": 39 answers on stdin, 43 with the dose-weighting block).
//
// The reference's reconstruct3d is a compiled program; so is this one.  It covers the call PYP makes by default (a .cistem table
// in the standard column order, a float32 stack, no dose weighting, no likelihood blurring) and does nothing but parse, stream
// the particle range from the stack file into libpypmatch (include/ppm.h: ppm_host_read -> ppm_device_upload -> ppm_insert_batch)
// and write the two dump files.  Everything else — the other answers, and every input it would have to refuse — is handed to
// bin/reconstruct3d.py (pyp_amd/surface/cli.py:reconstruct3d_main) as a child process with the same stdin, BEFORE the GPU is
// touched, so that behaviour and messages have one definition.  Start-up is what this buys: no interpreter and no numpy import in
// front of a run that moves 26 GB in half a second (bench.py, "dropin").  With PPM_STACK_CACHE=1 the call is served by the resident
// per-GPU server instead (dropin_server.h): no context creation and, when an earlier call uploaded the range, no PCIe pass.
//
// Built by pyp_amd/csrc/Makefile into bin/reconstruct3d (g++, no HIP: the C ABI only).
#include "dropin_server.h"

using namespace dropin;

int main() {
    const auto t0 = Clock::now();
    const std::string input = read_all_stdin();
    auto fall_back = [&]() { hand_to_python("reconstruct3d.py", input); };
    if (const char *e = getenv("PPM_NATIVE")) if (!strcmp(e, "0")) fall_back();
    ReconJob j;
    if (!recon_parse(input, j)) fall_back();
    {   // the resident server, if asked for (it answers "hand over" exactly where this program would)
        Reply rp;
        if (run_through_server(kProgRecon, input, rp)) {
            if (rp.status == kHandOver) fall_back();
            fputs(rp.text.c_str(), stdout); fflush(stdout);
            _exit(rp.status);
        }
    }
    // ---- from here on the GPU is in use: no more hand-overs.  The lock comes first (PYP may start several processes per node,
    // src/pyp/system/mpi.py:104: a waiting process holds neither a context nor page-locked memory); then the device start-up (context,
    // code object, accumulators, page-locked staging buffers) runs in a thread of its own while the parameter file is read.
    setenv("PPM_SYNC", "block", 0);
    const int lockfd = gpu_lock(device_index());
    long chunk_mb = 256, call_mb = 2048;
    if (const char *e = getenv("PPM_IO_CHUNK_MB")) chunk_mb = std::max(1L, atol(e));
    const size_t pin_bytes = staging_bytes(j.ilast - j.ifirst + 1, j.sec, chunk_mb);
    ppm_accum_t *acc = nullptr;
    Stream st;
    StartUp up(device_index(), pin_bytes, st.pinned, [&] { acc = ppm_accum_create(j.box, (float)j.px, j.symmetry.c_str(), nullptr); return acc != nullptr; });
    auto bail = [&](const std::string &msg) { leave(st, up, nullptr, msg); };
    try { recon_rows(j); } catch (const Fail &f) { bail(f.msg); }
    const long n = j.n;
    Out out;
    recon_banner(j, out, "native");
    const auto t1 = Clock::now();
    if (!up.wait_device()) bail(up.error());
    const auto t2 = Clock::now();

    // ---- reader -> uploader -> insertion (the stages of pyp_amd/surface/cli.py:_iter_image_chunks)
    const StreamPlan plan = stream_plan(pin_bytes, n, j.sec, call_mb);
    up.want_pinned = plan.npin;
    st.wait_pinned = [&](int slot) { return up.wait_pinned(slot); };          // page-locked by the start-up thread
    if (!st.start(plan, j)) bail("ERROR: reconstruct3d: cannot open " + j.stack);
    const Consumed done = consume(st, "reconstruct3d", [&](void *ptr, long lo, long hi) {
        return ppm_insert_batch(acc, &j.rc, ptr, 1, (int)(hi - lo), j.rin.data() + (size_t)lo * 32);
    });
    if (!done.err.empty()) bail(!up.error().empty() ? up.error() : done.err);
    st.finish(); up.finish();
    const auto t3 = Clock::now();
    long c0 = 0, c1 = 0;
    try { recon_outputs(j, acc, st.pinned, pin_bytes, c0, c1); }
    catch (const Fail &f) { bail(f.msg); }
    catch (const std::bad_alloc &) { bail("ERROR: reconstruct3d: out of memory for the dump files"); }
    ppm_accum_destroy(acc);
    gpu_unlock(lockfd);
    printf("\nInserted %ld of %ld particles in %.1f s\n", c0 + c1, n, since(t0));
    printf("Timing: inputs %.2f s, device %.2f s, particles %.2f s, dumps %.2f s\n", secs(t0, t1), secs(t1, t2), secs(t2, t3), since(t3));
    printf("Start-up: device context %.2f s, accumulators %.2f s after the answers were read (in a thread of its own)\n", up.init_s, up.ready_s);
    printf("Pipeline: %ld chunks; reader: read %.2f s, waited for a buffer %.2f s; uploader: copied %.2f s, waited for a buffer %.2f s; main thread: computed %.2f s, "
           "waited for data %.2f s\n", done.ncalls, st.t_read, st.w_pin, st.t_up, st.w_dev, done.t_comp, done.w_data);
    recon_footer(out);
    fflush(stdout);
    _exit(0);          // the library's reader pool is parked on purpose
}
