"""End to end through the drop-in surface: the restated `bal` program (loader, CLI, LM/VarPro loops,
Linearizor) with the HIP library vs the same program with the oracle-backed Linearizor
(tests/cpp/bal_oracle.cpp) on the same data_custom file.  Bar: identical
accept/reject sequence, cost per iteration within 1e-6 relative (LM amplifies ulp differences)."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(binary, path, log, extra):
    cmd = [os.path.join(ROOT, binary), "--input", path, "--log-log-path", log, "--quiet"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.load(open(log)), r.stdout


@pytest.mark.parametrize("extra", [
    ["--max-num-iterations-step-1", "8", "--max-num-iterations-step-2", "6", "--power-sc-iterations", "20"],
    ["--max-num-iterations-step-1", "8", "--max-num-iterations-step-2", "6", "--power-sc-iterations", "20", "--e0-mode", "implicit"],
    ["--solver-type-step-1", "POWER_SCHUR_COMPLEMENT", "--max-num-iterations-step-1", "6",
     "--max-num-iterations-step-2", "3", "--power-sc-iterations", "10", "--eta", "0"],
    ["--residual-robust-norm", "HUBER", "--residual-huber-parameter", "5", "--max-num-iterations-step-1", "5",
     "--max-num-iterations-step-2", "3", "--e0-mode", "tiles"],
    # the explicit-Schur-complement linearizor (LinearizorSC): PCG / RIPCG and the direct solve
    ["--solver-type-step-1", "PCG", "--solver-type-step-2", "RIPCG", "--max-num-iterations-step-1", "8",
     "--max-num-iterations-step-2", "4", "--e0-mode", "implicit"],
    ["--solver-type-step-1", "PCG", "--solver-type-step-2", "RIPCG", "--max-num-iterations-step-1", "6",
     "--max-num-iterations-step-2", "3", "--max-linear-solver-iterations", "25", "--eta", "1e-4"],
    ["--solver-type-step-1", "CHOLESKY", "--max-num-iterations-step-1", "8", "--max-num-iterations-step-2", "3"],
])
def test_bal_hip_matches_bal_oracle(tmp_path, extra):
    from povar_amd import synth
    p = synth.make_problem(10, 300, 1300, seed=21)
    f = str(tmp_path / "problem-10-300.txt")
    synth.write_data_custom(f, p)
    a, out_a = _run("bin/bal", f, str(tmp_path / "hip.json"), extra)
    b, out_b = _run("build/bal_oracle", f, str(tmp_path / "oracle.json"), extra)
    assert a["iteration"] == b["iteration"]
    assert a["step_is_successful"] == b["step_is_successful"], (a["step_is_successful"], b["step_is_successful"])
    assert a["linear_solver_iterations"] == b["linear_solver_iterations"]
    ca, cb = np.array(a["cost"]), np.array(b["cost"])
    # the iteration counter restarts at 0 where step 2 begins (the summary is not reset between the
    # steps, bal_bundle_adjustment.cpp:581-583)
    n1 = [i for i, it in enumerate(a["iteration"]) if it == 0][1]
    relerr = np.abs(ca / cb - 1)
    assert relerr[:n1].max() <= 1e-6, relerr[:n1].max()
    # step 2 on these synthetic inputs is violently ill-conditioned (projective costs swing between
    # 1e6 and 1e12 from one trial step to the next), so ulp-level differences in the increment are
    # amplified; the accept/reject sequence above is the sharp check.  The cost of a REJECTED step-2 trial
    # (far outside the trust region of the projective model) is not a stable quantity at all -- it can
    # differ by factors between two runs of the reference itself -- so costs are compared on the
    # accepted iterates (and the initial one)
    ok2 = np.array(a["step_is_successful"][n1:], dtype=bool) | (np.array(a["iteration"][n1:]) == 0)
    assert relerr[n1:][ok2].max() <= 1e-2, relerr[n1:]
    assert np.allclose(a["trust_region_radius"][:n1], b["trust_region_radius"][:n1], rtol=1e-5)
    assert a["_static"]["solver"]["termination_type"] == b["_static"]["solver"]["termination_type"]
    assert "Final Cost" in out_a and a["_type"] == "rootba_povar"


@pytest.mark.gpu
@pytest.mark.parametrize("gpus", [2, 3])
def test_bal_gpus_n_matches_one_device(tmp_path, gpus):
    """`bal --gpus N`: the single-process N-shard Linearizor (host/linearizor_power_varproj_hip.cpp: one host thread per
    shard context, landmark shards from povar_shard_range, one exchange step per power-series term) against `bal` on one
    context, trafalgar-257 shape from a start inside the basin, both LM steps run to convergence: identical accept/reject
    sequences and inner iteration counts, every cost to 1e-6, the same trust-region schedule, the same final state file.
    On a one-GPU box the shards share device 0 and the exchange is the in-process all-reduce through the library's host
    hook (RCCL refuses duplicate devices); on a multi-GPU node the same command runs RCCL over the devices."""
    from povar_amd import synth
    p = synth.make_bal_problem("trafalgar-257", init="gt", init_noise=0.02)
    f = str(tmp_path / "problem-257-65132-gt.txt")
    synth.write_data_custom(f, p)
    extra = ["--max-num-iterations-step-1", "30", "--max-num-iterations-step-2", "30", "--power-sc-iterations", "20"]
    one, _ = _run("bin/bal", f, str(tmp_path / "one.json"), extra)
    many, _ = _run("bin/bal", f, str(tmp_path / "many.json"), extra + ["--gpus", str(gpus)])
    assert one["iteration"] == many["iteration"] and len(one["iteration"]) > 6
    assert one["step_is_successful"] == many["step_is_successful"]
    assert one["linear_solver_iterations"] == many["linear_solver_iterations"]
    ca, cb = np.array(one["cost"]), np.array(many["cost"])
    assert np.abs(ca / cb - 1).max() <= 1e-6, np.abs(ca / cb - 1).max()
    assert np.allclose(one["trust_region_radius"], many["trust_region_radius"], rtol=1e-4)
    assert one["_static"]["solver"]["termination_type"] == many["_static"]["solver"]["termination_type"]


@pytest.mark.gpu
@pytest.mark.parametrize("graph_comm", ["0", "1"])
def test_bal_rccl_branch_of_the_shard_team_with_one_rank(tmp_path, graph_comm):
    """The RCCL branch of the sharded LinearizorPowerVarprojHip on the one GPU there is: POVAR_FORCE_MULTI=1
    routes `bal --gpus 1` through the shard team -- ncclCommInitRank on the worker thread, every exchange step of the run
    an ncclAllReduce of one rank on the context's stream, with POVAR_GRAPH_COMM=1 inside the captured term loop -- against
    plain `bal`: identical accept / reject sequences and iteration counts, every cost to 1e-9."""
    from povar_amd import synth
    p = synth.make_bal_problem("trafalgar-257", init="gt", init_noise=0.02)
    f = str(tmp_path / "problem-257-65132-gt.txt")
    synth.write_data_custom(f, p)
    extra = ["--max-num-iterations-step-1", "12", "--max-num-iterations-step-2", "8", "--power-sc-iterations", "20"]
    one, _ = _run("bin/bal", f, str(tmp_path / "one.json"), extra)
    env = dict(os.environ, POVAR_FORCE_MULTI="1", POVAR_GRAPH_COMM=graph_comm, POVAR_HOST_COMM="0")
    cmd = [os.path.join(ROOT, "bin/bal"), "--input", f, "--log-log-path", str(tmp_path / "team.json"), "--quiet"] + extra + ["--gpus", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "exchange: RCCL" in r.stdout + r.stderr, (r.stdout + r.stderr)[-1500:]
    team = json.load(open(str(tmp_path / "team.json")))
    assert one["iteration"] == team["iteration"] and len(one["iteration"]) > 6
    assert one["step_is_successful"] == team["step_is_successful"]
    assert one["linear_solver_iterations"] == team["linear_solver_iterations"]
    ca, cb = np.array(one["cost"]), np.array(team["cost"])
    assert np.abs(ca / cb - 1).max() <= 1e-9, np.abs(ca / cb - 1).max()


@pytest.mark.gpu
def test_bal_gpus_2_from_the_random_start(tmp_path):
    """`bal --gpus 2` against one context from the reference's RANDOM initial cameras (bal_problem.cpp:398-407), where no
    route gets near the noise floor.  Step 1 agrees in the accept / reject sequence and to 1e-3 in
    every cost (measured 5e-7 ... 4e-5 after 30 iterations, run to run: the summation order of the shards' partial sums and of
    the LDS accumulation, amplified by thirty LM steps from a start far outside the basin).  The first step-2 cost is a sum dominated by a dozen observations whose depth (P X)_z is within 1e-3 of zero
    after step 1 (r = (P X)_xy / (P X)_z: a relative change of 1e-9 in such a depth moves the cost by per cent, and the cost
    has a pole where a depth crosses zero).  It CANNOT have a tolerance: measured ratios between the two runs are 1.015, 10 and
    318 on the same sources -- which of the near-zero depths lands on which side of zero, and how near, is decided by the last
    bits of step 1.  What is asserted of it: finite and positive on both routes (the reference's own step 2 starts from the
    same kind of number); the converged comparison of the two routes is test_bal_gpus_n_matches_one_device."""
    from povar_amd import synth
    p = synth.make_bal_problem("trafalgar-257")
    f = str(tmp_path / "problem-257-65132.txt")
    synth.write_data_custom(f, p)
    extra = ["--max-num-iterations-step-1", "30", "--max-num-iterations-step-2", "2", "--power-sc-iterations", "20"]
    one, _ = _run("bin/bal", f, str(tmp_path / "one.json"), extra)
    two, _ = _run("bin/bal", f, str(tmp_path / "two.json"), extra + ["--gpus", "2"])
    n1 = [i for i, it in enumerate(one["iteration"]) if it == 0][1]
    assert one["iteration"][:n1] == two["iteration"][:n1] and n1 > 5
    assert one["step_is_successful"][:n1] == two["step_is_successful"][:n1]
    ca, cb = np.array(one["cost"]), np.array(two["cost"])
    assert np.abs(ca[:n1] / cb[:n1] - 1).max() <= 1e-3
    assert np.isfinite(ca[n1]) and np.isfinite(cb[n1]) and ca[n1] > 0 and cb[n1] > 0, (ca[n1], cb[n1])


@pytest.mark.gpu
def test_bal_is_bit_reproducible_with_povar_deterministic(tmp_path):
    """`bal --deterministic` (SolverOptions::deterministic -> povar_options.flags: POVAR_FLAG_DETERMINISTIC; no environment
    variable: VERDICT r05 item 6) at the drop-in boundary: two runs of `bal`
    -- file -> step-1 LM iterations -> step-2 LM iterations -> log -- on trafalgar-257 from the perturbed ground truth write
    the SAME costs, digit for digit (the JSON log prints them with 17 significant digits), with the same accept / reject
    sequence; the default mode ends on the same costs to 1e-6 (its sums are in arrival order, the LM loop amplifies the last
    bits)."""
    from povar_amd import synth
    p = synth.make_bal_problem("trafalgar-257", init="gt", init_noise=0.02)
    f = str(tmp_path / "problem-257-65132-gt.txt")
    synth.write_data_custom(f, p)
    extra = ["--max-num-iterations-step-1", "10", "--max-num-iterations-step-2", "6", "--power-sc-iterations", "20"]

    def run(tag, det):
        env = dict(os.environ)
        env.pop("POVAR_DETERMINISTIC", None)
        log = str(tmp_path / f"{tag}.json")
        cmd = [os.path.join(ROOT, "bin/bal"), "--input", f, "--log-log-path", log, "--quiet"] + extra + (["--deterministic"] if det else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return json.load(open(log))

    a, b, c = run("det1", True), run("det2", True), run("default", False)
    assert a["cost"] == b["cost"] and a["step_is_successful"] == b["step_is_successful"] and a["iteration"] == b["iteration"]
    assert len(a["cost"]) > 10
    assert a["step_is_successful"] == c["step_is_successful"]
    assert np.abs(np.array(a["cost"]) / np.array(c["cost"]) - 1).max() <= 1e-6
