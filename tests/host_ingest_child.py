"""Child process of tests/test_host_malformed.py (not a test module), and the damaged cache files that it and
tests/test_host.py share.

    python host_ingest_child.py product <outdir> <jobs.json>
    python host_ingest_child.py oracle  <outdir> <jobs.json>

jobs.json is a list of {"key", "path", "elem_is_int", "normalise", "truncate", "env"}.

product: the product loader ends the process on a file it refuses (exit(-1)), so every job runs in a fork of this
process, which has loaded the library but never run it (no OpenMP team exists yet when it forks).  The child sends
its stderr to <outdir>/<key>.err, calls sh_mm_load_ex and saves the six results to <outdir>/<key>.npz.  Its exit
status (negative: the signal that ended it) goes to <outdir>/status.json.

oracle: the oracle's fscanf loop, like the reference's, spins for ever on some inputs; it runs here, one job after
the other, so that the test's time limit on this process ends it.  <outdir>/progress names the job in hand.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# CacheHeader of host/src/sparse_matrix.cpp: magic[8], int32 elem_is_int, truncated, int64 src_size, src_mtime_ns,
# int32 rows, cols, nonz, uint32 max_width, int64 nnz; then int32 row_ptr[rows + 1], int32 col_idx[nnz], val[nnz]
CACHE_HEADER, OFF_ROWS, OFF_COLS, OFF_NNZ = 56, 32, 36, 48


def damaged_caches(valid):
    """name -> bytes: a valid cache file damaged in one way each; the loader must fall back to parsing on every one."""
    rows = int(np.frombuffer(valid, np.int32, 1, OFF_ROWS)[0])
    cols = int(np.frombuffer(valid, np.int32, 1, OFF_COLS)[0])
    nnz = int(np.frombuffer(valid, np.int64, 1, OFF_NNZ)[0])
    assert len(valid) == CACHE_HEADER + 4 * (rows + 1) + 8 * nnz and rows > 4 and nnz > 4

    def patched(offset, value, dtype):
        b = bytearray(valid)
        b[offset:offset + np.dtype(dtype).itemsize] = np.array([value], dtype).tobytes()
        return bytes(b)

    rp = np.frombuffer(valid, np.int32, rows + 1, CACHE_HEADER)
    mid = rows // 2
    return {
        "nnz_2_pow_40": patched(OFF_NNZ, 2 ** 40, np.int64),
        "rows_int_max": patched(OFF_ROWS, 2 ** 31 - 1, np.int32),
        "rows_negative": patched(OFF_ROWS, -1, np.int32),
        "four_bytes_long": valid + b"\0\0\0\0",
        "four_bytes_short": valid[:-4],
        "header_only": valid[:CACHE_HEADER],
        "row_ptr_decreases": patched(CACHE_HEADER + 4 * mid, int(rp[mid + 1]) + 1, np.int32),
        "col_idx_is_width": patched(CACHE_HEADER + 4 * (rows + 1) + 4 * (nnz // 2), cols, np.int32),
        "col_idx_negative": patched(CACHE_HEADER + 4 * (rows + 1), -1, np.int32),
    }


def save(outdir, key, res):
    rows, cols, hdr, rp, ci, va = res
    np.savez(os.path.join(outdir, key + ".npz"), dims=np.array([rows, cols, hdr], np.int64), row_ptr=rp, col_idx=ci,
             val=va.view(np.uint32))


def product(outdir, jobs):
    from sparseharness_amd import hostlib as H
    H.load()
    status = {}
    for j in jobs:
        sys.stdout.flush()
        pid = os.fork()
        if pid == 0:
            code = 3
            try:
                fd = os.open(os.path.join(outdir, j["key"] + ".err"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                os.dup2(fd, 2)
                os.environ.update(j.get("env") or {})
                save(outdir, j["key"], H.mm_load(j["path"], elem_is_int=bool(j["elem_is_int"]), truncate=bool(j["truncate"]),
                                                 normalise=j["normalise"]))
                code = 0
            finally:
                os._exit(code)
        _, st = os.waitpid(pid, 0)
        status[j["key"]] = os.WEXITSTATUS(st) if os.WIFEXITED(st) else -os.WTERMSIG(st)
    with open(os.path.join(outdir, "status.json"), "w") as f:
        json.dump(status, f)


def oracle(outdir, jobs):
    from oracle import oracle as O
    for j in jobs:
        with open(os.path.join(outdir, "progress"), "w") as f:
            f.write(j["key"])
        save(outdir, j["key"], O.mm_load(j["path"], elem_is_int=bool(j["elem_is_int"]), normalise=j["normalise"]))
    with open(os.path.join(outdir, "progress"), "w") as f:
        f.write("done")


if __name__ == "__main__":
    with open(sys.argv[3]) as f:
        todo = json.load(f)
    {"product": product, "oracle": oracle}[sys.argv[1]](sys.argv[2], todo)
