"""Runs the named cases of tests/solver_forms.py in a process of its own and prints one JSON line with their records.

TEST INFRASTRUCTURE ONLY.  The switches that the library reads once per process (VISFS_BA_PCG_GATHER, VISFS_BA_SMALL_PCG_LDS) need a fresh
process each, with the variable set before the library loads: tests/test_gpu_solver_forms.py starts this script for them.
"""
import json
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main(argv):
    import oracle_lib
    import solver_forms
    olib = oracle_lib.load()
    records = []
    for name in argv:
        records.extend(solver_forms.run_case(olib, name))
    print(json.dumps(dict(records=records)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
