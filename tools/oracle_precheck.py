"""CPU only: the oracle side of tests/test_gpu_reference_shapes.py, without the code under test.

For every case of that file (or the ones named on the command line) the oracle runs on the case's own weights, inputs and injected
randomness in fp64, in numpy float32, and in numpy float32 with only the CTC lattice in fp64, in the process pool the GPU test uses.
Asserted on both float32 legs: every per-sample loss within 1e-5 relative and every gradient tensor within 1e-4 of its largest
fp64 entry - the seeds are not in a chaotic regime, so a float32 implementation can meet the GPU test's bounds.  Printed: the
distances and the oracle's wall time per case (profiles/reference_shapes_parity.txt records them).

As recorded there, the plain numpy-float32 leg meets the gradient bound only at T = 200: at T >= 1000 the oracle's log-space
CTC lattice in float32 (log-likelihood -3000 ... -6000) puts every gradient 1e-4 ... 6e-3 from fp64 (the size of the log-likelihood, not the seed, decides that), so the
script ends with an AssertionError that lists those legs; the leg with the lattice in fp64 (2e-6 at most) is the one that speaks
about the conditioning of the network's inputs.

    python tools/oracle_precheck.py [case ...]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgr_amd  # noqa: E402,F401  (first: sizes the BLAS pools before numpy is imported)
import numpy as np  # noqa: E402

from tests.helpers import oracle_by_slices, rel_err  # noqa: E402
from tests.test_gpu_reference_shapes import CASES, case_inputs  # noqa: E402


def main():
    bad = []
    for name in sys.argv[1:] or list(CASES):
        spec, B, T, Lmax, w, xs, labels, il, ll, rand = case_inputs(name)
        t0 = time.time()
        ref = oracle_by_slices(spec.to_dict(), w, xs, labels, il, ll, rand, start_server=True, precisions=("", "32", "32c"))
        print("%-16s %-5s B=%-2d T=%-4d labels %3d..%-3d seed %d  oracle x 3 %6.1f s  mean loss %.8f"
              % (name, CASES[name][0], B, T, ll.min(), ll.max(), CASES[name][5], time.time() - t0, ref["lb"].mean()), flush=True)
        for p, what in (("32", "numpy float32"), ("32c", "numpy float32, CTC lattice in fp64")):
            el = float(np.abs(ref["lb" + p] / ref["lb"] - 1).max())
            eg = {k: rel_err(ref["g" + p][k], ref["g"][k]) for k in ref["g"]}
            kmax = max(eg, key=eg.get)
            print("    %-36s loss %.2e, softmax %.2e, gradients %.2e .. %.2e (%s)"
                  % (what + ":", el, rel_err(ref["P" + p], ref["P"]), min(eg.values()), eg[kmax], kmax), flush=True)
            if not (el < 1e-5 and eg[kmax] < 1e-4):
                bad.append((name, what, el, kmax, eg[kmax]))
    assert not bad, bad


if __name__ == "__main__":
    main()
