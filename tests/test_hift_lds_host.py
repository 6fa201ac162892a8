"""CPU: the LDS carve-up of the vocoder's row-owning kernels (hc_lds_layout in jyutvoice_amd/csrc/hift_common.h) asks for
exactly the bytes the two hand-written formulas asked for before the kernels and the host shared one description.

hiftconv_kernel and hiftpair_kernel used to form their LDS pointers by pointer arithmetic while hc_lds_bytes / hp_lds_bytes
repeated the sizes as a byte formula; nothing tied the two together.  The formulas below are those two, as they stood; the
library's count (jv_hift_lds_bytes: host only) must equal them for every instantiated (C, NG) and every (k, dil) the host accepts."""
import os

import pytest

CONV = [(64, 2), (64, 4), (128, 1), (128, 2), (256, 1)]      # hiftconv_kernel<C, NG> (the second of each width: JV_HIFT_WG8)
PAIR = [(64, 2), (128, 2)]                                    # hiftpair_kernel<C, NG, k>
SHAPES = [(k, d) for k in (3, 7, 11) for d in (1, 3, 5) if (k - 1) * d <= 56]


def wrpad(R, k, d):
    return ((R + (k - 1) * d + 7) & ~7) + 1


def conv_bytes(C, NG, k, d):
    R = 80 * NG
    wr = wrpad(R, k, d)
    return ((wr * 4 + 255) & ~255) + R * 8 + (C // 32) * 2 * wr * 64 + NG * (C // 32) * 16 * 36 * 4


def pair_bytes(C, NG, k, d):
    R = 80 * NG
    w1, w2 = wrpad(R, k, d), wrpad(R, k, 1)
    return ((w1 * 4 + 255) & ~255) + R * 16 + (C // 32) * 2 * max(w1, w2) * 64 + NG * (C // 32) * 16 * 36 * 4


@pytest.fixture(scope="module")
def lib():
    from jyutvoice_amd import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from jyutvoice_amd import _lib
    return _lib.load()


def test_lds_bytes_equal_the_former_formulas(lib):
    assert len(SHAPES) == 9      # the widest window, k = 11 at dilation 5, has a 50-row halo
    for pair, cases, want in ((0, CONV, conv_bytes), (1, PAIR, pair_bytes)):
        for C, NG in cases:
            for k, d in SHAPES:
                assert lib.jv_hift_lds_bytes(pair, C, NG, k, d) == want(C, NG, k, d), (pair, C, NG, k, d)


def test_every_launch_fits_lds(lib):
    """160 KB per workgroup is the launchers' limit; shapes without an instantiation answer -1"""
    for pair, cases in ((0, CONV), (1, PAIR)):
        for C, NG in cases:
            for k, d in SHAPES:
                assert 0 < lib.jv_hift_lds_bytes(pair, C, NG, k, d) <= 160 * 1024
    assert lib.jv_hift_lds_bytes(0, 96, 1, 3, 1) == -1 and lib.jv_hift_lds_bytes(1, 256, 1, 3, 1) == -1
