"""The results of the three chain-step kernels as bits, for the comparison of two builds of the library.

  TTSK_LIB=<library> python profiles/scripts/chain_bits.py run OUT.npz
      every accepted case of tests/chain_step_ref.py through the C entry point of the library TTSK_LIB names (default: the
      tree's libttsk.so), as tests/test_gpu_chain_edges.py calls it: seeded standard-normal operands, both layouts of X, every
      way of storing T; cases marked `pack` once more with the packed core.  Out and T of every call (guards included) go
      to OUT.npz, one array per (case, layout, T mode, tensor).
  python profiles/scripts/chain_bits.py compare A.npz B.npz
      the same names, and every array np.array_equal as 64-bit patterns.  Exit status 1 otherwise.

One process per library: the library is picked when tt_sketch_amd._native is first imported.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def run(out):
    from tests import chain_step_ref as ref
    from tests.test_gpu_chain_edges import Device
    from tt_sketch_amd import _native as nat
    nat.call("ttsk_init", 0)
    arrays = {}
    cases = ref.all_cases()
    for i, c in enumerate(cases):
        vals = ref.values(c, False, sum(map(ord, c.id)) + 1)
        for layout in ref.layouts(c):
            dev = Device(nat, c, layout, vals)
            for wt in ref.T_MODES[c.kind]:
                for packed in ((0, 1) if c.opts.get("pack") else (0,)):
                    if packed:
                        dev.pack()
                    try:
                        o, t, _ = dev.call(wt)
                    finally:
                        if packed:
                            dev.unpack()
                    for name, bufs in (("Out", o), ("T", t or [])):
                        for b, x in enumerate(bufs):
                            arrays["%s/%s/T%d/p%d/%s%d" % (c.id, layout, wt, packed, name, b)] = x.view(np.uint64)
        if i % 25 == 0:
            print("%d / %d cases" % (i, len(cases)), flush=True)
    np.savez_compressed(out, **arrays)
    print("%s: %d cases, %d arrays -> %s" % (nat.LIB_PATH, len(cases), len(arrays), out))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    if sorted(A.files) != sorted(B.files):
        print("the two files hold different arrays")
        return 1
    bad = [k for k in A.files if not np.array_equal(A[k], B[k])]
    print("%d arrays compared, %d differ%s" % (len(A.files), len(bad), (": " + ", ".join(bad[:10])) if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
