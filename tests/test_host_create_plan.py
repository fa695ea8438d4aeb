"""The resolver behind povar_create (povar_amd/csrc/create_plan.hpp): options, environment and problem size to a CreatePlan, checked
without the library or a device by tests/cpp/create_plan_check.cpp against a table written down from povar_create's statement
order before the resolver existed and from INTEGRATION.md section 6: the defaults by size (65536 observations: lane per landmark;
2^20: rows placed on a host thread), the environment over the flag in both directions, what deterministic mode pins, the four
fp32 refusals in their order with their texts and what an accepted fp32 context is forced to, the E0 variants' cuts, the shapes
of step 1's chunk layout, every clamp, the CU mask and its message.  tests/test_gpu_create_plan.py holds the same expectations to
povar_layout_info on a device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "create_plan_check")


def test_create_plan_resolves_as_povar_create_did():
    # (always through make: the rule lists the headers, so an edited resolver rebuilds the checker)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "../../build/create_plan_check"],
                          stdout=subprocess.DEVNULL)
    # (its last case reads the process's environment: none of the library's variables may leak in from the caller's)
    env = {k: v for k, v in os.environ.items() if not k.startswith("POVAR_")}
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "create_plan_check: ok" in r.stdout
