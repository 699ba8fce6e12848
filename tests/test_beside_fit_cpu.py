"""mf_beside_fit: the host arithmetic that decides whether the RMSE pass may
run beside a resident persistent sweep -- exactly one 4-wave pass workgroup
must fit on a CU next to one sweep workgroup, and a second must not (then a
grid of one pass workgroup per CU is pinned one per CU by the registers alone).

The register counts are those of the rank-64 kernels compiled for gfx950
(profiles/sse_beside/resource_usage_f64.txt); a CU has 4 SIMDs of 512
registers per lane (granule 8) and 160 KiB of LDS.
"""

import pytest

CU = (512, 4, 160 << 10)
SWEEP_LDS = 138 << 10          # the C3 FP64 sweep's slab + slices
PASS_LDS = 32


def _fit(*a):
    from matrix_factorization import _lib

    return int(_lib.load().mf_beside_fit(*a, *CU))


def test_fp64_rank64_stream_kernels_fit_exactly_one():
    # KB = 2: 2 waves/SIMD x 160 + 136 = 456 <= 512 < 592
    assert _fit(154, 8, SWEEP_LDS, 132, 4, PASS_LDS) == 1
    # KB = 4: 2 x 176 + 136 = 488 <= 512 < 624
    assert _fit(170, 8, SWEEP_LDS, 132, 4, PASS_LDS) == 1


@pytest.mark.parametrize("regs,waves", [(8, 1), (64, 4), (132, 4), (512, 4)])
def test_fp32_rank64_sweep_leaves_no_room(regs, waves):
    # 16 waves x 128 registers: 4 waves/SIMD x 128 = the whole register file
    assert _fit(128, 16, SWEEP_LDS, regs, waves, PASS_LDS) == 0


def test_two_pass_workgroups_fitting_is_a_no():
    # 320 + 64 = 384 and 320 + 128 = 448 <= 512: a second one would fit too
    assert _fit(154, 8, SWEEP_LDS, 64, 4, PASS_LDS) == 0
    # the granule of 8 decides: 2 x 160 + 96 = 416, + 96 = 512 still fits
    assert _fit(154, 8, SWEEP_LDS, 92, 4, PASS_LDS) == 0
    assert _fit(154, 8, SWEEP_LDS, 97, 4, PASS_LDS) == 1     # 104: 424, 528


def test_lds_counts_too():
    assert _fit(154, 8, SWEEP_LDS, 132, 4, 30 << 10) == 0    # 138 + 30 KiB > 160 KiB
    # registers would admit two, the LDS only one
    assert _fit(154, 8, SWEEP_LDS, 64, 4, 12 << 10) == 1


def test_bad_arguments_are_a_no():
    assert _fit(0, 8, SWEEP_LDS, 132, 4, PASS_LDS) == 0
    assert _fit(154, 0, SWEEP_LDS, 132, 4, PASS_LDS) == 0
    assert _fit(154, 8, -1, 132, 4, PASS_LDS) == 0
