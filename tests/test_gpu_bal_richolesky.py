"""`bal --solver-type-step-1 CHOLESKY --solver-type-step-2 RICHOLESKY` end to end on the GPU: exact reduced solves in both
steps must end on the generator's noise floor (tests/test_known_answer.py).  The CPU twin with RIPCG driven to the exact
solve (--eta 1e-13: at most 66 CG iterations per solve on n = 110) ends at 201.37 against 200.6 +- 7.1 on this problem."""
import pytest

from test_known_answer import COMMON, check_floor, run_bal, write_problem

pytestmark = pytest.mark.gpu


def test_bal_richolesky_reaches_noise_floor(tmp_path):
    p, f = write_problem(tmp_path, (10, 300, 1300), 21)
    res = run_bal("bin/bal", f, str(tmp_path / "log.json"),
                  ["--solver-type-step-1", "CHOLESKY", "--solver-type-step-2", "RICHOLESKY"] + COMMON + ["--quiet"])
    check_floor(p, res)
    d, n1 = res["log"], res["n1"]
    its = d["linear_solver_iterations"][n1 + 1:]
    assert len(its) > 0 and all(i == 0 for i in its)          # every step-2 solve is direct
    assert all(i == 0 for i in d["linear_solver_iterations"][1:n1])
    assert "Final Cost:" in res["stdout"]
