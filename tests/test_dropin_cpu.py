"""The host layer of the compiled drop-in executables (pyp_amd/csrc/dropin_plan.h, dropin_common.h, dropin_server.h) without a GPU and
without the library: small C++ programs with their own main are compiled against the real headers with the host compiler under
sanitizers and run as processes of their own.

* the stream's plan (staging-buffer size, chunk, chunks, group, buffers in rotation, reader threads) over a table, against the formulas
  of the programs written out below;
* the stream itself (reader -> uploader -> consume) over test doubles of the five library calls it makes, once under ThreadSanitizer and
  once under AddressSanitizer + UBSan: every record exactly once and in order, or the expected ERROR with every thread joined;
* the settings a request carries: applied for the request, undone afterwards, the server's own left alone (PPM_SYNC among them)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyp_amd", "csrc")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
TSAN = ["-fsanitize=thread"]


def compile_program(tmp, name, src, flags):
    (tmp / (name + ".cpp")).write_text(src)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", *flags, "-I", CSRC, "-o", str(tmp / name), str(tmp / (name + ".cpp"))])
    return str(tmp / name)


# ---------------------------------------------------------------------------------------------------------------- the plan
PLAN_SRC = r'''
#include <cstdio>
#include <cstring>
#include "dropin_plan.h"
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    long range_len, n, chunk_mb, call_mb; unsigned long long sec; char threads[32];
    while (fscanf(f, "%ld %ld %llu %ld %ld %31s", &range_len, &n, &sec, &chunk_mb, &call_mb, threads) == 6) {
        const size_t pin = dropin::staging_bytes(range_len, (size_t)sec, chunk_mb);
        if (strcmp(threads, "-")) setenv("PPM_IO_THREADS", threads, 1); else unsetenv("PPM_IO_THREADS");
        const dropin::StreamPlan p = dropin::stream_plan(pin, n, (size_t)sec, call_mb);
        printf("%zu %ld %ld %ld %d %d %d\n", pin, p.chunk, p.nchunks, p.group, p.npin, p.ndev, p.nread);
    }
    fclose(f);
    return 0;
}
'''


def plan(range_len, n, sec, chunk_mb, call_mb, threads):
    """The arithmetic of refine3d_main.cpp / reconstruct3d_main.cpp / with_stack as they had it, each for itself."""
    pin = min(max(16, (chunk_mb << 20) // sec), range_len) * sec
    chunk = max(1, min(n, pin // sec))
    nchunks = (n + chunk - 1) // chunk
    group = max(1, min(nchunks, (call_mb << 20) // (chunk * sec)))
    nread = 8 if threads is None else max(1, min(16, int(threads)))
    return (pin, chunk, nchunks, group, min(3, nchunks), min(2, (nchunks + group - 1) // group), nread)


S32, S64, S256, S512 = (b * b * 4 for b in (32, 64, 256, 512))
# (range_len, n, sec, chunk_mb, call_mb, PPM_IO_THREADS); the server sizes its buffers from n, the one-shot programs from last - first + 1
PLANS = [
    (1, 1, S64, 256, 2048, None), (1, 1, S512, 1, 512, "0"),                                    # one image
    (7, 7, S64, 64, 512, None), (15, 15, S32, 1, 512, "3"), (60, 9, S64, 64, 512, None),        # fewer than 16 images; rows missing from the range
    (49, 49, S64, 4096, 2048, None), (60, 49, S64, 4096, 512, "99"), (1000, 1000, S256, 256, 2048, None),      # a chunk larger than the range
    (192, 192, S64, 1, 2048, None), (256, 256, S64, 1, 2048, None), (193, 193, S64, 1, 512, "3"), (300, 256, S64, 1, 512, None),      # 3 and 4 chunks
    (320, 320, S64, 1, 2, None), (448, 448, S64, 1, 3, "0"), (1000, 999, S32, 1, 4, "99"),     # groups of 2 / 3 / 4 chunks that do not divide nchunks
    (100000, 100000, S256, 256, 2048, "99"), (100000, 100000, S256, 64, 512, None), (5000, 5000, S512, 64, 512, "3"), (5000, 4000, S512, 4096, 2048, None),
    (3, 3, S512, 1, 1, None), (40, 40, S512, 1, 2048, "16"), (100000, 100000, S32, 4096, 2048, "1"),
]
PLAN_LITERALS = {
    (1, 1, S64, 256, 2048, None): (16384, 1, 1, 1, 1, 1, 8),
    (60, 9, S64, 64, 512, None): (60 * 16384, 9, 1, 1, 1, 1, 8),                                # the buffer is sized before the rows are read
    (1000, 1000, S256, 256, 2048, None): (262144000, 1000, 1, 1, 1, 1, 8),                      # 1024 images fit 256 MB, the range has 1000
    (192, 192, S64, 1, 2048, None): (1 << 20, 64, 3, 3, 3, 1, 8), (256, 256, S64, 1, 2048, None): (1 << 20, 64, 4, 4, 3, 1, 8),
    (320, 320, S64, 1, 2, None): (1 << 20, 64, 5, 2, 3, 2, 8),                                  # 5 chunks in groups of 2: 3 groups, 2 device buffers
    (100000, 100000, S256, 256, 2048, "99"): (1 << 28, 1024, 98, 8, 3, 2, 16),
    (3, 3, S512, 1, 1, None): (3 << 20, 3, 1, 1, 1, 1, 8),                                      # at least 16 images a buffer - or the whole range
    (40, 40, S512, 1, 2048, "16"): (16 << 20, 16, 3, 3, 3, 1, 16), (1, 1, S512, 1, 512, "0"): (1 << 20, 1, 1, 1, 1, 1, 1),
}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dropin_plan")
    (tmp / "cases.txt").write_text("".join("%d %d %d %d %d %s\n" % (c[:5] + ("-" if c[5] is None else c[5],)) for c in PLANS))
    exe = compile_program(tmp, "plan", PLAN_SRC, ASAN)
    out = subprocess.check_output([exe, str(tmp / "cases.txt")], timeout=20).decode().splitlines()
    assert len(out) == len(PLANS)
    return dict(zip(PLANS, (tuple(int(x) for x in line.split()) for line in out)))


@pytest.mark.parametrize("case", PLANS, ids=lambda c: "range%d-n%d-sec%d-chunk%dMB-call%dMB-threads_%s" % c)
def test_stream_plan(plans, case):
    assert plans[case] == plan(*case)
    if case in PLAN_LITERALS:
        assert plans[case] == PLAN_LITERALS[case]
    pin, chunk, nchunks, group, npin, ndev, nread = plans[case]
    n, sec = case[1], case[2]
    assert pin % sec == 0 and chunk * sec <= pin and (nchunks - 1) * chunk < n <= nchunks * chunk      # whole images, no chunk larger than its buffer
    assert 1 <= group <= nchunks and 1 <= npin <= 3 and 1 <= ndev <= 2 and 1 <= nread <= 16


def test_the_plan_table_has_the_cases_it_names():
    assert set(PLAN_LITERALS) <= set(PLANS)
    got = {c: plan(*c) for c in PLANS}
    assert {3, 4} <= {g[2] for g in got.values()} and any(g[2] % g[3] for g in got.values()) and any(c[3] == 4096 and g[2] == 1 for c, g in got.items())
    assert {c[2] for c in PLANS} == {S32, S64, S256, S512} and {1, 4096} <= {c[3] for c in PLANS} and {None, "0", "3", "99"} <= {c[5] for c in PLANS}


# -------------------------------------------------------------------------------------------------------------- the stream
STREAM_SRC = r'''
// usage: stream <stack file> n=<rows> group=<chunks per call> [resident=1] [scattered=1] [fail_read=<k>] [no_pinned=<slot>] [fail_use=<k>]
// The stack file holds 2 n + 1 records of 16 bytes, record r filled with (r * 16 + byte) & 255.  Row i of the range is record i + 3
// (contiguous) or record 2 i (scattered).  Prints "OK <calls>" or "FAILED <error text>" once every thread is joined; a record that is
// wrong, missing, repeated or out of order ends the program with status 3.
#include <atomic>
#include "dropin_common.h"
static thread_local const char *g_err = "";
static std::atomic<long> g_reads{0};
static long g_fail_read = 0;
extern "C" {
int ppm_host_read(int fd, long long offset, void *dst, size_t bytes, int n_threads) {
    if (++g_reads == g_fail_read) { g_err = "short read (test double)"; return -1; }
    if (n_threads < 1 || pread(fd, dst, bytes, (off_t)offset) != (ssize_t)bytes) { g_err = "pread failed"; return -1; }
    return 0;
}
int ppm_device_upload(void *dst, const void *src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
void *ppm_device_alloc(size_t bytes) { return malloc(bytes); }
void ppm_device_free(void *p) { free(p); }
const char *ppm_last_error(void) { return g_err; }
}
using namespace dropin;
int main(int argc, char **argv) {
    long n = 1, group = 1, resident = 0, scattered = 0, no_pinned = -1, fail_use = 0;
    for (int i = 2; i < argc; i++) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) return 2;
        const std::string k(argv[i], (size_t)(eq - argv[i])); const long v = atol(eq + 1);
        if (k == "n") n = v; else if (k == "group") group = v; else if (k == "resident") resident = v; else if (k == "scattered") scattered = v;
        else if (k == "fail_read") g_fail_read = v; else if (k == "no_pinned") no_pinned = v; else if (k == "fail_use") fail_use = v; else return 2;
    }
    RangeJob j;
    j.stack = argv[1]; j.sec = 16; j.mh.offset = 0; j.n = n; j.contiguous = !scattered;
    j.rin.assign((size_t)n * 32, 0.0);
    for (long i = 0; i < n; i++) j.rin[(size_t)i * 32 + COL_POS] = scattered ? 2 * i + 1 : i + 4;            // positions are 1-based
    StreamPlan p = stream_plan(staging_bytes(2, j.sec, 1), n, j.sec, 1);                                       // a range of 2 to size the buffers: 2 records a chunk
    if (p.chunk != std::min(2L, n) || p.nchunks != (n + 1) / 2) return 2;
    p.group = group; p.ndev = (int)std::min(2L, (p.nchunks + group - 1) / group);                              // MB units cannot say "2 chunks a call"
    std::vector<char> pinned[3], whole((size_t)n * j.sec);
    Stream st;
    for (int k = 0; k < p.npin; k++) { pinned[k].resize(32); st.pinned[k] = pinned[k].data(); }
    if (resident) st.resident = whole.data();
    if (no_pinned >= 0) st.wait_pinned = [&](int slot) { return slot != no_pinned; };
    long expect_lo = 0, calls = 0;
    Consumed done;
    if (!st.start(p, j)) done.err = "ERROR: cannot open the stack";
    else done = consume(st, "stream", [&](void *ptr, long lo, long hi) {
        if (++calls == fail_use) { g_err = "use failed (test double)"; return -1; }
        if (lo != expect_lo || hi <= lo || hi > n || (hi - lo > group * p.chunk)) _exit(3);
        for (long i = lo; i < hi; i++) {
            const long r = scattered ? 2 * i : i + 3;
            for (int b = 0; b < 16; b++) if (((unsigned char *)ptr)[(i - lo) * 16 + b] != (unsigned char)((r * 16 + b) & 255)) _exit(3);
        }
        expect_lo = hi;
        return 0;
    });
    st.finish();
    if (st.reader_t.joinable() || st.uploader_t.joinable() || st.fd >= 0 || st.dbuf[0] || st.dbuf[1]) return 4;
    if (!done.err.empty()) { printf("FAILED %s\n", done.err.c_str()); return 0; }
    if (expect_lo != n || done.ncalls != calls) return 3;
    printf("OK %ld\n", done.ncalls);
    return 0;
}
'''
READ_ERR = "ERROR: reading the particle stack failed: short read (test double)"
UPLOAD_ERR = "ERROR: upload failed (PPM_TEST_FAIL_UPLOAD)"
# (arguments, PPM_TEST_FAIL_UPLOAD, expected line)
STREAMS = [
    ("n=1 group=1", None, "OK 1"),
    ("n=11 group=2", None, "OK 3"),                   # six chunks, three groups: the staging slots and both device slots are recycled, hi == n closes the last
    ("n=11 group=2 resident=1", None, "OK 3"),
    ("n=11 group=2 scattered=1", None, "OK 3"),
    ("n=11 group=2", "1", "FAILED " + UPLOAD_ERR), ("n=11 group=2", "3", "FAILED " + UPLOAD_ERR), ("n=11 group=2", "6", "FAILED " + UPLOAD_ERR),
    ("n=11 group=2 resident=1", "3", "FAILED " + UPLOAD_ERR),
    ("n=11 group=2 fail_read=4", None, "FAILED " + READ_ERR),
    ("n=11 group=2 no_pinned=1", None, "FAILED ERROR: page-locked staging memory could not be prepared"),
    ("n=11 group=2 fail_use=2", None, "FAILED ERROR: use failed (test double)"),
    ("n=12 group=6", None, "OK 1"), ("n=5 group=1", None, "OK 3"),
]


@pytest.fixture(scope="module")
def stream_programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dropin_stream")
    (tmp / "stack.bin").write_bytes(bytes((r * 16 + b) & 255 for r in range(2 * 12 + 1) for b in range(16)))
    return {"tsan": compile_program(tmp, "stream_tsan", STREAM_SRC, TSAN), "asan": compile_program(tmp, "stream_asan", STREAM_SRC, ASAN)}, str(tmp / "stack.bin")


@pytest.mark.parametrize("sanitizer", ["tsan", "asan"])
@pytest.mark.parametrize("case", STREAMS, ids=lambda c: c[0].replace(" ", "-") + ("-fail_upload%s" % c[1] if c[1] else ""))
def test_stream_delivers_every_record_once_or_ends_with_its_error(stream_programs, case, sanitizer):
    programs, stack = stream_programs
    args, fail_upload, want = case
    env = {k: v for k, v in os.environ.items() if not k.startswith("PPM_")}
    if fail_upload:
        env["PPM_TEST_FAIL_UPLOAD"] = fail_upload
    r = subprocess.run([programs[sanitizer], stack] + args.split(), env=env, capture_output=True, text=True, timeout=20)      # a hang fails through the timeout
    assert r.returncode == 0 and r.stdout == want + "\n" and r.stderr == "", (r.returncode, r.stdout, r.stderr[-3000:])


# ------------------------------------------------------------------------------------------------- the settings of a request
SETTINGS_SRC = r'''
#include <sys/stat.h>
#include "dropin_server.h"
static void show(const char *when) {
    const mode_t m = umask(0); umask(m);
    printf("%s umask=%03o", when, (unsigned)m);
    for (const char *k : { "PPM_SYNC", "PPM_FOO", "PPM_BAR", "PPM_STACK_CACHE_GB", "PPM_LOCK_DIR" }) { const char *v = getenv(k); printf(" %s=%s", k, v ? v : "(unset)"); }
    printf("\n");
}
int main() {
    umask(077);
    setenv("PPM_SYNC", "block", 1); setenv("PPM_FOO", "1", 1); setenv("PPM_STACK_CACHE_GB", "5", 1);
    show("before");
    {
        dropin::RequestSettings as_the_client("umask=23\nPPM_BAR=2\nPPM_LOCK_DIR=/x\n");
        show("inside");
    }
    show("after");
    return 0;
}
'''


def test_request_settings_leave_the_servers_own_alone_and_are_undone(tmp_path):
    exe = compile_program(tmp_path, "settings", SETTINGS_SRC, ASAN)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PPM_")}
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=20)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    outside = " umask=077 PPM_SYNC=block PPM_FOO=1 PPM_BAR=(unset) PPM_STACK_CACHE_GB=5 PPM_LOCK_DIR=(unset)"
    assert r.stdout.splitlines() == ["before" + outside,
                                     "inside umask=023 PPM_SYNC=block PPM_FOO=(unset) PPM_BAR=2 PPM_STACK_CACHE_GB=5 PPM_LOCK_DIR=(unset)",
                                     "after" + outside]
