"""Generate tests/golden/side_plan_refusals.json: the code and message of every refused call of
tests/test_gpu_refusals.py, from the library in use (FFS_LIBRARY_PATH selects a build).  The committed file was
recorded from a library built from the commit before the side plans' host code was folded onto shared helpers, so the
test holds the folded code to the messages and the order of checks it had before.  Needs a real MI355X.

    python tests/golden/make_side_plan_refusals.py [output path]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import test_gpu_refusals as tr  # noqa: E402

if __name__ == "__main__":
    out = tr.record(*sys.argv[1:2])
    print("recorded %d refusals" % sum(len(cases) for cases in out.values()))
