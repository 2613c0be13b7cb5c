// dropin_plan.h — how the drop-in executables cut a particle range for their stream (dropin_common.h: reader -> uploader -> compute):
// the size of a page-locked staging buffer, and from it the chunks, the groups of chunks one library call takes, and how many buffers
// and reader threads are in play.  Plain C++ with no ppm.h and no threads, so the rule is tested on its own (tests/test_dropin_cpu.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>

namespace dropin {

// one staging buffer: whole images, `chunk_mb` MB of them but at least 16, and no larger than a range of `range_len` images can fill
// (page-locking costs ~0.2 s per GB).  The one-shot programs size it before the rows are read, from last - first + 1; the server from n.
inline size_t staging_bytes(long range_len, size_t sec, long chunk_mb) {
    return std::min(std::max((size_t)16, ((size_t)chunk_mb << 20) / sec), (size_t)range_len) * sec;
}

struct StreamPlan {
    long chunk = 1, nchunks = 1, group = 1;     // images per chunk (one staging buffer), chunks of the range, chunks per library call
    int npin = 1, ndev = 1, nread = 8;          // staging buffers (<= 3) and device buffers (<= 2) in rotation, threads of one ppm_host_read
};
// n images of `sec` bytes through staging buffers of `pin_bytes`, `call_mb` MB per library call; io_threads is PPM_IO_THREADS (1..16, default 8)
inline StreamPlan stream_plan(size_t pin_bytes, long n, size_t sec, long call_mb, const char *io_threads = getenv("PPM_IO_THREADS")) {
    StreamPlan p;
    p.chunk = std::max(1L, std::min(n, (long)(pin_bytes / sec)));
    p.nchunks = (n + p.chunk - 1) / p.chunk;
    p.group = std::max(1L, std::min(p.nchunks, (long)(((size_t)call_mb << 20) / ((size_t)p.chunk * sec))));
    p.npin = (int)std::min(3L, p.nchunks);
    p.ndev = (int)std::min(2L, (p.nchunks + p.group - 1) / p.group);
    p.nread = io_threads ? std::max(1, std::min(16, atoi(io_threads))) : 8;
    return p;
}

}  // namespace dropin
