"""The mathematics behind povar_observation_covariance_pose / _joint, on the CPU (tests/observation_covariance_reference.py),
and the declarations of the two calls.

* the per-observation factors U_i, L_i, A_i reproduce the full scaled system: J^T J = System.full(0);
* route A (gauge fixed on the cameras, Schur formulas, long double) and route B (J pinv(J^T J) J^T) agree inside the bound of
  the GPU test: the rows do not depend on the gauge;
* sum_i h_i = rank J inside the summed bound, 0 <= h_i <= d, and in step 2 h_i = w_i (c_uu + c_vv);
* damped: block elimination and the dense long-double inverse of System.full(lam) agree;
* an fp64 emulation of the kernel's formula (pair walk in chunks, nq = 0) stays inside the bound on every case of the GPU
  test, and five mutations of it each leave the bound on some observation: the GPU test can see these mistakes.
"""
import fnmatch
import os
import re

import numpy as np
import pytest

import observation_covariance_reference as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("small", "NONE"), ("p22", "NONE"), ("long", "NONE"), ("small", "HUBER")]
_PINV = {}


def _pinv_rows(name, step, norm):
    key = (name, step, norm)
    if key not in _PINV:
        _PINV[key] = O.obs_system(name, step, norm).pinv_rows()
    return _PINV[key]


def _err(got, ref):
    return np.abs((np.asarray(got, dtype=np.longdouble) - ref.rows).astype(np.float64))


@pytest.mark.parametrize("name,norm", CASES)
@pytest.mark.parametrize("step", [1, 2])
def test_factors_reproduce_the_system(step, name, norm):
    s = O.obs_system(name, step, norm)
    J = s.dense()
    H, want = J.T @ J, s.sys.full(0.0)
    assert np.abs(H - want).max() <= 1e-13 * np.abs(want).max()
    if norm == "HUBER":
        assert s.w.min() < 1.0  # the weights act


@pytest.mark.parametrize("name,norm", CASES)
@pytest.mark.parametrize("step", [1, 2])
def test_routes_a_and_b_agree(step, name, norm):
    ref = O.reference(name, step, norm, 0.0, True)
    B, rank = _pinv_rows(name, step, norm)
    assert rank == ref.rank
    err = _err(B, ref)
    print(f"step {step} {name} {norm}: cond {ref.lm_ref.cond:.3g}, worst |A - B| {err.max():.2e} = {(err / ref.bound).max():.2e} of the bound")
    assert np.all(err <= ref.bound)


@pytest.mark.parametrize("name,norm", CASES)
@pytest.mark.parametrize("step", [1, 2])
def test_leverages_sum_to_the_rank(step, name, norm):
    ref = O.reference(name, step, norm, 0.0, True)
    s = ref.osys
    assert ref.rank == s.dim * s.sys.n_cams + 3 * s.sys.n_lms - (12 if step == 1 else 15)
    for tag, h in (("A", ref.rows[:, 0]), ("B", _pinv_rows(name, step, norm)[0][:, 0])):
        total = float(np.sum(h.astype(np.longdouble)))
        print(f"step {step} {name} {norm} route {tag}: sum h = {total:.13f}, rank {ref.rank}")
        assert abs(total - ref.rank) <= ref.bound[:, 0].sum()
        assert np.all(h >= 0) and np.all(h <= s.d)


@pytest.mark.parametrize("name,norm", CASES)
def test_step2_leverage_is_the_weighted_trace(name, norm):
    ref = O.reference(name, 2, norm, 0.0, True)
    rows = ref.rows.astype(np.float64)
    assert np.all(np.abs(rows[:, 0] - ref.osys.w * (rows[:, 1] + rows[:, 3])) <= ref.bound[:, 0])
    assert np.all(rows[:, 1] > 0) and np.all(rows[:, 3] > 0) and np.all(rows[:, 2] ** 2 <= rows[:, 1] * rows[:, 3])


@pytest.mark.parametrize("lam", [1e-4, 1.0])
@pytest.mark.parametrize("step", [1, 2])
def test_damped_block_elimination_is_the_dense_inverse(step, lam):
    ref = O.reference("small", step, "NONE", lam, False)
    err = _err(ref.osys.dense_inverse_rows(lam), ref)
    print(f"step {step} lambda {lam:g}: block elimination vs dense long-double inverse {(err / ref.bound).max():.2e} of the bound")
    assert np.all(err <= 1e-3 * ref.bound)
    assert np.all(ref.rows[:, 0] > 0) and np.all(ref.rows[:, 0] < ref.osys.d)


@pytest.mark.parametrize("step,name,norm,lam,free_gauge", O.GPU_CASES)
def test_emulation_of_the_kernel_stays_inside_the_bound(step, name, norm, lam, free_gauge):
    ref = O.reference(name, step, norm, lam, free_gauge)
    C, hi = ref.osys.emulation_operands(lam, free_gauge)
    err = _err(ref.osys.emulate(C, hi), ref)
    print(f"step {step} {name} {norm} lambda {lam:g}: emulation, worst err / bound {(err / ref.bound).max():.2e}; "
          f"bound / value: h {(ref.bound[:, 0] / np.abs(ref.rows[:, 0].astype(np.float64))).max():.2e}")
    assert np.all(err <= ref.bound)
    # the bound means something: it resolves every leverage to 1 % (the damped system at lambda = 1e-4 is the worst conditioned)
    assert np.all(ref.bound[:, 0] <= 1e-2 * np.abs(ref.rows[:, 0].astype(np.float64)))


MUTATIONS = [("no_cross", "small", "NONE"), ("transposed", "small", "NONE"), ("second_chunk", "long", "NONE"),
             ("corrected", "small", "NONE"), ("weighted", "small", "HUBER")]


@pytest.mark.parametrize("mutation,name,norm", MUTATIONS)
@pytest.mark.parametrize("step", [1, 2])
def test_mutations_of_the_emulation_leave_the_bound(step, mutation, name, norm):
    ref = O.reference(name, step, norm, 0.0, True)
    s = ref.osys
    if mutation == "second_chunk":
        assert np.diff(s.lm_off).max() > O.CHUNK[step]
    C, hi = s.emulation_operands(0.0, True)
    err = _err(s.emulate(C, hi, mutation), ref)
    cols = slice(1, 4) if mutation == "weighted" else slice(0, 4)
    worst = (err / ref.bound)[:, cols].max()
    print(f"step {step} {name} {norm}: mutation {mutation}: worst err / bound {worst:.3g}")
    assert worst > 1.0


def test_header_and_export_map_declare_the_calls():
    header = open(os.path.join(ROOT, "include", "povar_hip.h")).read()
    vmap = open(os.path.join(ROOT, "povar_amd", "csrc", "povar.map")).read()
    exported = re.search(r"global:([^}]*?)local:", vmap).group(1).replace(";", " ").split()
    for name in ("povar_observation_covariance_pose", "povar_observation_covariance_joint"):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*povar_ctx\s*\*", header), name
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), name
    text = " ".join(header.replace("*", " ").split())
    assert "do not depend on the gauge, on the Jacobi scaling or on povar_set_jl_col_scaling" in text
    assert "sum_i h_i = rank J = DIM n_cams + 3 n_lms - nq" in text
    assert "y2 == 0" in text
