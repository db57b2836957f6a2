#!/usr/bin/env python
"""Write tests/golden/math_truth.npz: for every device-library builtin and float dtype, 256 seeded arguments
(tests/float_tables.arguments) and the true result from mpmath at 200 bits.  float64: a double-double pair, `hi` the
correctly rounded value and `lo` the rest; float32: the float64 value of the truth.  Needs mpmath, nothing else.

    python scripts/make_math_truth.py              # the fixture
    python scripts/make_math_truth.py --accuracy   # the fixture, then the reference rows of profiles/math_builtins_accuracy.txt
                                                   # (device columns of rows already recorded are kept)
"""

import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent / "tests"))
import float_tables as ft  # noqa: E402

HEADER = """# Worst error of the math builtins in units in the last place, against the true value (mpmath, 200 bits) at the 256
# arguments per function and dtype of tests/golden/math_truth.npz.  `reference` is numpy / scipy on the host
# (scripts/make_math_truth.py --accuracy); `bound` = reference + the ulps tests/test_math_builtins.py grants between device and
# reference; `device` is the generated gfx950 kernel (printed by tests/test_gpu_float_tables.py, recorded after a run).
# function dtype  reference  at                         bound     device  at
"""


def main(argv):
    out = {}
    for name in ft.BUILTINS:
        for dtype in ft.FLOATS:
            x = ft.arguments(name, dtype)
            hi, lo = ft.mp_truth(name, x)
            assert np.isfinite(hi).all(), (name, dtype, x[~np.isfinite(hi)])
            out[f"{name}_{dtype}_x"], out[f"{name}_{dtype}_hi"] = x, hi
            if dtype == "float64":
                out[f"{name}_{dtype}_lo"] = lo
        print(name, flush=True)
    ft.TRUTH_FILE.parent.mkdir(exist_ok=True)
    np.savez_compressed(ft.TRUTH_FILE, **out)
    print(f"{ft.TRUTH_FILE}: {ft.TRUTH_FILE.stat().st_size} bytes")
    if "--accuracy" in argv:
        device = {}
        if ft.ACCURACY_FILE.exists():
            for line in ft.ACCURACY_FILE.read_text().splitlines():
                w = line.split()
                if len(w) >= 7 and not line.startswith("#") and w[5] != "-":
                    device[(w[0], w[1])] = (float(w[5]), float.fromhex(w[6]))
        ft._TRUTH.clear()
        rows = [ft.accuracy_row(n, d, device.get((n, d))) for n in ft.BUILTINS for d in ft.FLOATS]
        ft.ACCURACY_FILE.write_text(HEADER + "\n".join(rows) + "\n")
        print("".join(r + "\n" for r in rows))


if __name__ == "__main__":
    main(sys.argv[1:])
