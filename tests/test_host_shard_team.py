"""The threading under the sharded linearizor (host/shard_team.hpp), checked without the library or a device by
tests/cpp/shard_team_check.cpp: a team of one without a worker calls on the caller's thread; teams of 1, 2 and 3 workers
run the call once per rank per run on as many distinct threads, 200 runs in a row; the in-process all-reduce leaves the
left-to-right sum over ranks on every rank, bit for bit, for values whose sum depends on the order and for buffer lengths
that change from call to call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "shard_team_check")


def test_shard_team_runs_every_rank_once_and_reduces_in_rank_order():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "../../build/shard_team_check"],
                              stdout=subprocess.DEVNULL)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "shard_team_check: ok" in r.stdout
