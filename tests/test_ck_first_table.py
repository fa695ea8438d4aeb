"""The table e0_ck reads the first requests of a launch from (ck_layout.hpp: ck_first_tables) against the kernel's own walk of
its tiles, through tests/cpp/ck_first_check.cpp (host only, no GPU)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_first_request_table_matches_the_kernels_walk(tmp_path):
    exe = str(tmp_path / "ck_first_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "ck_first_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "OK", out.stdout + out.stderr
