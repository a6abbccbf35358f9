"""The patch-size limit of the in-kernel reference statistics (csrc/amvs_fast_common.h AMVS_REF_IN_KERNEL_MAX_PATCH,
exported as amvs_step_sources_max_patch) is the true limit up to which a k x k window's sum of squared 8-bit codes --
and every partial sum on the way to it, in any order -- is an integer float32 holds exactly: k^2 * 255^2 < 2^24.  No GPU."""
import numpy as np


def _limit():
    from amvs import _lib
    return int(_lib.load().amvs_step_sources_max_patch())


def test_step_header_and_table_agree():
    """include/amvs_step.h declares exactly what _lib.STEP_SIGNATURES binds, the library exports it, and nothing of it
    sits in the other tables."""
    import ctypes
    import os
    import re
    from amvs import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "amvs_step.h")).read(), flags=re.S)
    declared = set(re.findall(r"^int\s+(amvs_\w+)\(", hdr, re.M))
    assert declared == set(_lib.STEP_SIGNATURES) == {"amvs_set_step_sources", "amvs_get_step_sources",
                                                          "amvs_step_sources_max_patch"}
    for table in (_lib.SIGNATURES, _lib.DEPTH_SIGNATURES, _lib.LENS_SIGNATURES, _lib.MATCH_SIGNATURES, _lib.EPIPOLAR_SIGNATURES):
        assert not declared & set(table)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} not exported"


def test_limit_is_the_largest_odd_patch_whose_sums_fit_24_bits():
    k = _limit()
    assert k % 2 == 1
    assert k * k * 65025 < 2 ** 24 <= (k + 2) * (k + 2) * 65025
    assert (k, k * k * 65025, (k + 2) * (k + 2) * 65025) == (15, 14630625, 18792225)


def test_float32_holds_every_partial_sum_up_to_the_limit_and_not_beyond():
    k = _limit()
    # every integer up to the largest sum is a float32: checked at the top of the range, where the spacing is widest
    top = k * k * 65025
    n = np.arange(top - 4096, top + 1, dtype=np.int64)
    assert np.array_equal(n.astype(np.float32).astype(np.int64), n)
    # a float32 chain over an all-255 window in the kernel's order (column sums top to bottom, then k - 1 adds along
    # the row) and in the reverse association gives the integer
    col = np.float32(0)
    for _ in range(k):
        col = np.float32(col + np.float32(65025))
    row = col
    for _ in range(k - 1):
        row = np.float32(row + col)
    assert int(row) == top and int(np.float32(top)) == top
    # two sizes up the largest sum is odd and above 2^24: float32 cannot hold it, the conversion rounds
    beyond = (k + 2) * (k + 2) * 65025
    assert beyond > 2 ** 24 and beyond % 2 == 1 and int(np.float32(beyond)) != beyond
    # an all-254/255 image one size up already loses a unit somewhere below its top
    m = np.arange(2 ** 24, beyond + 1, dtype=np.int64)
    assert not np.array_equal(m.astype(np.float32).astype(np.int64), m)
