#!/usr/bin/env python
"""Cost of an evaluation call through the context layer: wall microseconds per
vaeb_validate_resident call over 200 calls on 10 000 resident rows at the default shape
(784-500-20, fp32, the default max_eval_rows), each call timed on its own.  Prints one JSON line
(median, mean, min, the last value).  VAEB_LIB_VARIANT=<name> measures libvaeb_hip_<name>.so instead."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import vaeb_oracle as O   # noqa: E402
from vaeb_amd import _lib             # noqa: E402

D, H, Z, B, ROWS, CALLS, WARM = 784, 500, 20, 100, 10000, 200, 20
ctx = _lib.Context(D, H, Z, B)
ctx.set_params(O.flatten(O.init_params(O.Config(D=D, H=H, Z=Z))))
ctx.set_eps_mode(_lib.EPS_PHILOX, 10)
ctx.set_valid_data(O.synthetic_mnist(n=ROWS, D=D))
for _ in range(WARM):
    ctx.validate_resident()
us = []
for _ in range(CALLS):
    t0 = time.perf_counter()
    last = ctx.validate_resident()
    us.append((time.perf_counter() - t0) * 1e6)
print(json.dumps({"lib": os.environ.get("VAEB_LIB_VARIANT", "branch"), "calls": CALLS, "rows": ROWS,
                  "us_per_call_median": float(np.median(us)), "us_per_call_mean": float(np.mean(us)),
                  "us_per_call_min": float(np.min(us)), "last_value": last}))
ctx.close()
