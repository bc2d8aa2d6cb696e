#!/usr/bin/env python
"""Host cost of an eager 16-bit step: wall microseconds per vaeb_update call over 2000 calls with
use_graph=False at 256-128-32, B = 256, bf16 (the step's GPU work is a few launches of one tile
each, so the time is the host's: argument structs, views and launches).  Prints one JSON line.
VAEB_LIB_VARIANT=<name> measures libvaeb_hip_<name>.so instead."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import vaeb_oracle as O   # noqa: E402
from vaeb_amd import _lib             # noqa: E402

D, H, Z, B, CALLS, WARM = 256, 128, 32, 256, 2000, 200
ctx = _lib.Context(D, H, Z, B, max_eval_rows=B, use_graph=False, dtype=_lib.DTYPE_BF16)
ctx.set_data(O.synthetic_mnist(n=8 * B, D=D))
ctx.set_params(O.flatten(O.init_params(O.Config(D=D, H=H, Z=Z))))
ctx.set_eps_mode(_lib.EPS_PHILOX, 10)
for i in range(WARM):
    ctx.update(i % 8)
t0 = time.perf_counter()
for i in range(CALLS):
    last = ctx.update(i % 8)
el = time.perf_counter() - t0
print(json.dumps({"lib": os.environ.get("VAEB_LIB_VARIANT", "branch"), "calls": CALLS, "us_per_update": el / CALLS * 1e6,
                  "last_elbo": last}))
ctx.close()
