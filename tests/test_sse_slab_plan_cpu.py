"""mf_sse_slab_plan: the host arithmetic that cuts the items into the LDS
groups of the item-stationary RMSE pass (no GPU needed)."""
import pytest

from matrix_factorization import _lib
from matrix_factorization.engine import sse_slab_plan

CUS = 256
NI = 100_000          # C3's items


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("k", [20, 64, 128])
def test_plan_fits_and_covers_every_item_once(dtype, k):
    limit = int(_lib.load().mf_strata_lds_limit())
    size = 4 if dtype == "float32" else 8
    pl = sse_slab_plan(NI, k, dtype, CUS)
    assert pl is not None
    G, nit = pl["groups"], pl["items"]
    assert G % CUS == 0 and pl["phases"] == G // CUS
    assert pl["stride"] >= k
    assert pl["lds"] == nit * (pl["stride"] + 1) * size
    assert 0 < pl["lds"] < limit                       # (the reduction words beside it)
    # group g holds the items i with i * G // NI == g: the ranges
    # [ceil(g NI / G), ceil((g + 1) NI / G)) -- every item exactly once,
    # none larger than the LDS rows
    lo = [-(-g * NI // G) for g in range(G + 1)]
    assert lo[0] == 0 and lo[-1] == NI
    assert all(0 <= b - a <= nit for a, b in zip(lo, lo[1:]))
    for g in (0, 1, G // 3, G - 1):
        assert all(i * G // NI == g for i in range(lo[g], lo[g + 1]))
    # the smallest such multiple of the workgroup count
    if G > CUS:
        fewer = -(-NI // (G - CUS))
        assert fewer * (pl["stride"] + 1) * size > limit - 256


def test_c3_plans():
    assert sse_slab_plan(NI, 64, "float64", CUS)["groups"] == 512
    assert sse_slab_plan(NI, 64, "float32", CUS)["groups"] == 256
    assert sse_slab_plan(NI, 64, "float32", CUS)["items"] == 391


def test_row_padding_keeps_16_byte_rows():
    assert sse_slab_plan(NI, 64, "float64", CUS, pad=1)["stride"] == 66
    assert sse_slab_plan(NI, 64, "float32", CUS, pad=1)["stride"] == 68
    assert sse_slab_plan(NI, 21, "float64", CUS, pad=1)["stride"] == 22


def test_row_larger_than_budget_does_not_fit():
    assert sse_slab_plan(NI, 1024, "float64", CUS, lds_budget=4096) is None
    assert sse_slab_plan(NI, 64, "float64", CUS, lds_budget=512) is None
    assert sse_slab_plan(NI, 64, "float64", CUS, lds_budget=520) is not None
