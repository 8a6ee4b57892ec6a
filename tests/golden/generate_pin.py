"""Generate tests/golden/pin_reference.npz (BUILD CONTAINER ONLY: needs the reference tree and its native helper,
`make -C oracle`).

Runs every test of tests/test_oracle_pin.py with the reference present and stores what the reference returned in them
(oracle.pin_against_reference.Recorded: outputs only, on the tests' own seeded inputs), so that the same tests run
against the stored values where the reference tree is absent.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import pin_against_reference as pin  # noqa: E402
from oracle import ref_leaf  # noqa: E402


def main():
    if not ref_leaf.available():
        raise SystemExit("reference tree absent")
    import test_oracle_pin as T
    for name in sorted(n for n in dir(T) if n.startswith("test_")):
        getattr(T, name)()
    np.savez_compressed(pin.GOLDEN, **T.REC.kept)
    print("wrote %s: %d arrays, %d bytes" % (pin.GOLDEN, len(T.REC.kept), os.path.getsize(pin.GOLDEN)))


if __name__ == "__main__":
    main()
