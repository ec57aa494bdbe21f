"""Compare two bench.py --dump-outputs directories array by array (the form of profiles/*_dump_compare.txt):

    python tools/compare_dumps.py DIR_A DIR_B

rel max diff = max |a - b| / max |a|; arrays that are bit-identical are marked so."""
import os
import sys

import numpy as np

a_dir, b_dir = sys.argv[1], sys.argv[2]
names = sorted(f for f in os.listdir(a_dir) if f.endswith(".npy"))
assert names and names == sorted(f for f in os.listdir(b_dir) if f.endswith(".npy")), "the two dumps hold different arrays"
worst, same = 0.0, 0
for n in names:
    a, b = np.load(os.path.join(a_dir, n)), np.load(os.path.join(b_dir, n))
    assert a.shape == b.shape, n
    ident = a.tobytes() == b.tobytes()
    same += ident
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    scale = float(np.abs(a64).max()) if a.size else 0.0
    rel = float(np.abs(a64 - b64).max()) / (scale + 1e-300) if a.size else 0.0
    worst = max(worst, rel)
    if not ident or len(names) <= 12:
        print("%-60s rel max diff %.3e (scale %.3e)%s" % (n, rel, scale, "  bit-identical" if ident else ""))
print("files %d bit-identical %d worst rel max diff %.3e" % (len(names), same, worst))
