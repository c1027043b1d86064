"""Generate tests/golden/ref_live.npz: the reference kernels' outputs for the inputs of tests/test_oracle_pinning.py's
test_live_reference_* tests -- what those tests compare the oracle with where oracle/_ref is not built.

    make -C oracle ref && python tests/golden/make_ref_live.py

Data only: the outputs oracle/_ref (the reference's own OpenCL C, compiled for x86-64) gave, keyed "<test>/<array>".
"""
import sys
from pathlib import Path

import numpy as np

TESTS = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(TESTS))
from oracle_binding import Oracle, Ref  # noqa: E402
import test_oracle_pinning as T  # noqa: E402


def main():
    ref, oracle = Ref(), Oracle()
    out = {}
    for name, got in (("rng", T.rng_reference(ref)), ("density", T.density_reference(ref)), ("mix", T.mix_reference(ref)),
                      ("rng_kernel", T.rng_kernel_reference(ref, oracle))):
        out.update({f"{name}/{k}": v for k, v in got.items()})
    np.savez_compressed(T.REF_LIVE, **out)


if __name__ == "__main__":
    main()
