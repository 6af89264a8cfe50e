"""Stores what oracle/_ref (the reference's own C for the DF J/K path) returns on the small cases of tests/test_oracle_ref_c.py
in tests/golden/ref_c_h2o_dz.npz, so that those checks also run where oracle/_ref cannot be built.  Run where it can
(oracle/Makefile, target `ref`):

    python tools/gen_golden_ref_c.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import test_oracle_ref_c as t     # noqa: E402

if not t.LIVE:
    raise SystemExit('oracle/_ref is not built here: it needs the reference sources (oracle/Makefile, REF=...)')
out = t.reference_outputs()
np.savez(t.GOLDEN, **out)
print('%s: %s' % (os.path.relpath(t.GOLDEN, ROOT), ', '.join('%s%s' % (k, list(v.shape)) for k, v in sorted(out.items()))))
