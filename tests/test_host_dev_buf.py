"""DevBuf<T> (povar_amd/csrc/dev_buf.hpp), the self-freeing device allocation every buffer of a context is, checked without the
library or a device by tests/cpp/dev_buf_check.cpp against its own hipMalloc / hipFree (a table of live blocks, a failure on the
k-th call): scope exit frees; release() twice is harmless and leaves n == 0; alloc on an owning buffer frees the old block and
counts only the new one; alloc(0) allocates nothing; a failed alloc leaves the buffer empty and the counter untouched; a move
leaves the source empty and frees what the target held; std::swap of two buffers, and of two structs of buffers with counts
(the shape of povar_ctx::CkDev), frees nothing; assigning an empty base frees every buffer and keeps the counts; nothing is
live and nothing was freed twice at the end of every case."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "dev_buf_check")


def test_dev_buf_frees_what_it_owns_once():
    # (always through make: the rule lists dev_buf.hpp, so an edited header rebuilds the checker)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "../../build/dev_buf_check"],
                          stdout=subprocess.DEVNULL)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "dev_buf_check: ok" in r.stdout
