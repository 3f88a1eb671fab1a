"""One process, one library (NEMAR_AB_LIBRARY chooses it before nemar_amd is imported): the first_outlier and spike cases of
tests/norm_cases.py at HW 4096, 65536 and 110592, and a checksum of every raw output byte (y, stats, gx) on the last line:
RESULT <library file> <sha256>.  Run by tests/test_norm_conditioning_gpu.py."""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import norm_cases as NC
    from backends import HipBackend
    from nemar_amd import _lib
    lib = _lib.load()
    be = HipBackend(lib)
    h = hashlib.sha256()
    for HW in (4096, 65536, 110592):
        for family in ("first_outlier", "spike"):
            for misalign in (False, True):
                for buf in NC.case_instnorm_conditioned(be, 6, HW, family, NC.ACT_RELU, True, misalign, seed=21):
                    h.update(buf.tobytes())
    print("RESULT", os.path.basename(lib.path), h.hexdigest())


if __name__ == "__main__":
    main()
