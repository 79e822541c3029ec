"""Every stage of the Ceres branch (Optimizer/Framework=1) on the device, held to an extended-precision truth of ITS OWN inputs.

check_optimize (test_gpu_ceres.py) holds that branch to the oracle's accept / reject decisions and to 1e-6 of a whole buffer, which a
step wrong by a part in 1e8 passes: the trust region absorbs it.  Here a device / oracle pair is stepped through the stage hooks — an
iteration-zero linearisation (k_linearize's Ceres arm, k_ceres_lin_finalize: cost, ||g||_inf, ||x||, the Jacobi scaling), trials with the
per-variable damping of damp_of in every gather form and solver, the dogleg's two back-substitution passes and k_dogleg_mid, commit, a
linearisation that keeps the scaling, the outlier rule — and after every step each side's buffers are judged by tests/stage_truth.py on
that side's own inputs; the device has to be as near the truth as the oracle is:
    eg <= 10 * max(eo, (64 + n) u)          n: the most terms summed into one block of the stage
The cases and the per-record assertions live in tests/ceres_stage_forms.py; measured values: profiles/ceres_stage_truth.log (one line per
case and step with every stage's n, eo, eg and ratio, printed here before any assertion and appended to the file VISFS_STAGE_LOG names
when that is set)."""
import os

import pytest

import ceres_stage_forms as CF
import stage_forms as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CF.CASES))
def test_ceres_stage_against_the_truth_of_its_own_inputs(olib, monkeypatch, name):
    for k in F.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    records = CF.run_case(olib, name)
    assert records
    lines = CF.log_lines(records)
    print("\n".join(lines))
    if os.environ.get("VISFS_STAGE_LOG"):
        with open(os.environ["VISFS_STAGE_LOG"], "a") as f:
            f.write("\n".join(lines) + "\n")
    CF.check_form(name, records[0]["info"])
    failures = []
    for check in [lambda: CF.check_sequence(name, records)] + [lambda rec=rec: CF.check_record(rec) for rec in records]:
        try:
            check()
        except AssertionError as ex:
            failures.append(str(ex))
    assert not failures, "\n".join(failures)
