"""A directory for the resident server's socket (PPM_LOCK_DIR) in tests.  A unix socket's path holds at most 107 bytes, and a
pytest tmp_path under a deep TMPDIR is longer than that: the server then cannot bind and the tests see no server at all."""
import os
import tempfile

SUN_PATH_MAX = 107
SOCKET_NAME = "pyp_amd_gpu0.u%d.sock" % 4294967295          # the server's socket with the longest user id (pyp_amd/csrc/dropin_server.h)


def short_dir():
    """A fresh, private directory in the first temporary directory whose paths fit a socket address; the caller removes it."""
    for base in (tempfile.gettempdir(), "/tmp", "/var/tmp", "/dev/shm"):
        if os.path.isdir(base) and os.access(base, os.W_OK | os.X_OK) and len(os.path.join(base, "ppm_12345678", SOCKET_NAME)) <= SUN_PATH_MAX:
            return tempfile.mkdtemp(prefix="ppm_", dir=base)
    raise RuntimeError("no writable temporary directory with a path short enough for a unix socket")
