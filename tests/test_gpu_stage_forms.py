"""Every linearisation, Schur and back-substitution form of the library, held to an extended-precision truth of ITS OWN inputs.

check_stages (test_gpu_parity.py) bounds every stage buffer at 1e-9 of the largest entry of the whole buffer, each stage computed from
the other side's inputs.  Here a device / oracle pair is stepped through linearize, two trials, commit, linearize, mark_outliers,
linearize and a trial; after every step each side's buffers are fetched and judged by tests/stage_truth.py — numpy.longdouble, every
stage on that side's own inputs, block by block — and the device has to be as near the truth as the oracle is:
    eg <= 10 * max(eo, (64 + n) u)          n: the most terms summed into one block of the stage
for every lanes-per-landmark instance of k_linearize with a partial last workgroup, the pose-major chunk counts 0, 1, 255, 256, 257
and 513, more than 840 poses, odometry and laser factors, every chunking and run length of the Schur complement and every place its
finalisation runs, the ill-conditioned landmarks (fast_recip, the device's 3x3 inverse), no robust kernel and Gauss-Newton.  The cases
and the per-record assertions live in tests/stage_forms.py; measured values: profiles/stage_forms_truth.log (one line per case and step
with every stage's n, eo, eg and ratio, printed here before any assertion and appended to the file VISFS_STAGE_LOG names when that is
set)."""
import os

import pytest

import stage_forms as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(F.CASES))
def test_stage_form_against_the_truth_of_its_own_inputs(olib, monkeypatch, name):
    for k in F.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    records = F.run_case(olib, name)
    assert records
    lines = F.log_lines(records)
    print("\n".join(lines))
    if os.environ.get("VISFS_STAGE_LOG"):
        with open(os.environ["VISFS_STAGE_LOG"], "a") as f:
            f.write("\n".join(lines) + "\n")
    F.check_form(name, records[0]["info"])
    failures = []
    for rec in records:
        try:
            F.check_record(rec)
        except AssertionError as ex:
            failures.append(str(ex))
    assert not failures, "\n".join(failures)
