"""CPU test of the top-k workspace sizes: they follow from the split
heuristics of the exact path (mf_topk.hip: topk_splits) and of the MFMA
filter (mf_topk_mm.hip: topk_mm_splits / topk_mw_splits), so the literals
below -- what the library returned before the filter's probe switches were
retired and the unit was split -- pin those heuristics.  No GPU."""

import pytest

from matrix_factorization import _lib

# (n_query, n_items) -> mf_topk_mm_workspace_bytes
MM_BYTES = {
    (10000, 100000): 148933152,
    (2000, 20000): 38101152,
    (333, 5003): 2788592,
    (1, 100): 167980,
    (100000, 2048): 206657440,
}
# (n_query, n_items, amount) -> mf_topk_workspace_bytes: the fused path's
# partial lists up to amount 64, the two-stage path's key matrix above
EXACT_BYTES = {
    (300, 5003, 10): 324000,
    (300, 5003, 64): 2073600,
    (300, 5003, 65): 12007200,
}


@pytest.fixture
def lib(monkeypatch):
    monkeypatch.delenv("MF_TOPK_TWO_STAGE", raising=False)
    return _lib.load()


def test_topk_mm_workspace_bytes_pinned(lib):
    for args, want in MM_BYTES.items():
        assert lib.mf_topk_mm_workspace_bytes(*args) == want, args
    for args in ((0, 5), (5, 0), (-1, 5), (5, -3)):
        assert lib.mf_topk_mm_workspace_bytes(*args) == 0, args


def test_topk_workspace_bytes_pinned(lib):
    for args, want in EXACT_BYTES.items():
        assert lib.mf_topk_workspace_bytes(*args) == want, args
    for args in ((0, 5, 10), (5, 0, 10), (-2, 5, 10), (5, -1, 65)):
        assert lib.mf_topk_workspace_bytes(*args) == 0, args
